// The arithmetic of msclip_resized_crop (include/msclip_input.h), written once for the device and for the host: input.hip runs
// `phase` from 256 threads of a workgroup with a barrier between the phases; a host program (tests/input_host.cpp) includes this
// file as plain C++ and runs the same three phases from one "thread" (tid 0, step 1).  No HIP type or builtin in here.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define CROP_HD __host__ __device__ __forceinline__
#else
#define CROP_HD static inline
#endif

// The clamps marked "a guard, not a path" below never fire while make_plan's formulas bound what the taps need.  A host build that
// defines MSCLIP_CROP_CHECK_GUARDS (tests/input_host.cpp) aborts where one would fire, so that an edit of the plan shows up there.
#if defined(MSCLIP_CROP_CHECK_GUARDS) && !defined(__HIPCC__)
#include <assert.h>
#define CROP_GUARD(cond) assert(cond)
#else
#define CROP_GUARD(cond) ((void)0)
#endif

namespace msclip_crop {

constexpr int MAX_SCALE = 8;          // MSCLIP_CROP_MAX_SCALE
constexpr int LDS_BYTES = 65536;      // MSCLIP_CROP_LDS_BYTES

struct Args {
  const unsigned char* src;
  int slot_h, slot_w;
  const int* dims;
  const int* boxes;
  const int* flip;
  const float* lut;
  int B, filter, out_h, out_w;
  void* out;
  int out_bf16;
  unsigned char* out_u8;
  int band, kx, ky, rows;             // the plan below
};

// ---- the plan: band and LDS bytes from the extents alone (host side; the kernel is sized for the worst box the slot allows)
struct Plan {
  int band, kx, ky, rows, lds_bytes;
};

static inline int plan_rows(int band, int slot_h, int out_h, int S) {
  const double sy = (double)slot_h / (double)out_h, fy = sy > 1.0 ? sy : 1.0;
  return (int)floor((band - 1) * sy + 2.0 * S * fy) + 2;
}

// false: these extents are rejected
static inline bool make_plan(int slot_h, int slot_w, int out_h, int out_w, int filter, Plan* p) {
  if (slot_h <= 0 || slot_w <= 0 || out_h <= 0 || out_w <= 0 || (filter != 2 && filter != 3)) return false;
  if ((long long)slot_h > (long long)MAX_SCALE * out_h || (long long)slot_w > (long long)MAX_SCALE * out_w) return false;
  const int S = filter == 2 ? 1 : 2;
  const double sx = (double)slot_w / (double)out_w, sy = (double)slot_h / (double)out_h;
  p->kx = 2 * (int)ceil(S * (sx > 1.0 ? sx : 1.0)) + 1;
  p->ky = 2 * (int)ceil(S * (sy > 1.0 ? sy : 1.0)) + 1;
  const int cand[10] = {32, 24, 16, 12, 8, 6, 4, 3, 2, 1};
  for (int i = 0; i < 10; ++i) {
    const int band = cand[i] < out_h ? cand[i] : out_h;
    const int rows = plan_rows(band, slot_h, out_h, S);
    const long long bytes = 4ll * out_w * (p->kx + 2) + 4ll * band * (p->ky + 2) + 4ll * rows * out_w;
    if (bytes <= LDS_BYTES) {
      p->band = band;
      p->rows = rows;
      p->lds_bytes = (int)bytes;
      return true;
    }
  }
  return false;
}

// ---- the arithmetic
CROP_HD float filter_value(int filter, float x) {
  x = fabsf(x);
  if (filter == 2) return x < 1.f ? 1.f - x : 0.f;                       // triangle
  const float a = -0.5f;                                                 // cubic, a = -0.5
  if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
  if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * a;
  return 0.f;
}

// The taps of output index i on an axis with box extent n and output extent m: first source index, count (1 ... kmax) and the
// normalised weights.
CROP_HD void taps(int filter, int n, int m, int i, int kmax, int* lo_out, int* cnt_out, float* w) {
  const float scale = (float)n / (float)m;
  const float fs = scale > 1.f ? scale : 1.f;
  const float sup = (filter == 2 ? 1.f : 2.f) * fs;
  const float c = ((float)i + 0.5f) * scale;
  int lo = (int)(c - sup + 0.5f);
  int hi = (int)(c + sup + 0.5f);
  CROP_GUARD(lo <= n - 1);
  lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
  hi = hi > n ? n : hi;
  int cnt = hi - lo;
  CROP_GUARD(cnt >= 1 && cnt <= kmax);
  cnt = cnt < 1 ? 1 : (cnt > kmax ? kmax : cnt);       // (1 <= hi - lo <= kmax by the plan; a guard, not a path)
  float s = 0.f;
  for (int k = 0; k < cnt; ++k) {
    w[k] = filter_value(filter, ((float)(k + lo) - c + 0.5f) / fs);
    s += w[k];
  }
  if (s != 0.f)
    for (int k = 0; k < cnt; ++k) w[k] = w[k] / s;
  *lo_out = lo;
  *cnt_out = cnt;
}

CROP_HD uint32_t round_u8(float x) {
  float r = floorf(x + 0.5f);
  r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
  return (uint32_t)r;
}

CROP_HD uint16_t bf16_rne(float f) {                  // finite values only (the table's)
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

CROP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// dims into the slot, the box into dims: each value is clamped on its own, nothing is added before it is in range
CROP_HD void clamp_box(const Args& a, int b, int* top, int* left, int* bh, int* bw) {
  const int h = clampi(a.dims[2 * b], 1, a.slot_h), w = clampi(a.dims[2 * b + 1], 1, a.slot_w);
  *top = clampi(a.boxes[4 * b], 0, h - 1);
  *left = clampi(a.boxes[4 * b + 1], 0, w - 1);
  *bh = clampi(a.boxes[4 * b + 2], 1, h - *top);
  *bw = clampi(a.boxes[4 * b + 3], 1, w - *left);
}

// One phase of the workgroup of sample b and the band of output rows [band0, band0 + band): "threads" tid, tid + nthr, ...
//   phase 0: the taps of every output column and of the band's rows into LDS
//   phase 1: the horizontal pass over the source rows the band needs, rounded to uint8, three channels in one LDS dword
//   phase 2: the vertical pass, rounding, table look-up, stores
// LDS, in dwords: wx [out_w][kx] | lox [out_w] | nx [out_w] | wy [band][ky] | loy [band] | ny [band] | inter [rows][out_w]
CROP_HD void phase(const Args& a, int b, int band0, uint32_t* lds, int tid, int nthr, int ph) {
  float* wx = (float*)lds;
  int* lox = (int*)(lds + (size_t)a.out_w * a.kx);
  int* nx = lox + a.out_w;
  float* wy = (float*)(nx + a.out_w);
  int* loy = (int*)(wy + (size_t)a.band * a.ky);
  int* ny = loy + a.band;
  uint32_t* inter = (uint32_t*)(ny + a.band);
  int top, left, bh, bw;
  clamp_box(a, b, &top, &left, &bh, &bw);
  const int nband = (a.out_h - band0 < a.band) ? a.out_h - band0 : a.band;      // rows of this band
  if (ph == 0) {
    for (int x = tid; x < a.out_w; x += nthr) taps(a.filter, bw, a.out_w, x, a.kx, &lox[x], &nx[x], wx + (size_t)x * a.kx);
    for (int i = tid; i < nband; i += nthr) taps(a.filter, bh, a.out_h, band0 + i, a.ky, &loy[i], &ny[i], wy + (size_t)i * a.ky);
    return;
  }
  // the first and one past the last source row of the band (lo and hi do not decrease with the output index)
  const int r0 = loy[0];
  int nrows = loy[nband - 1] + ny[nband - 1] - r0;
  CROP_GUARD(nrows >= 1 && nrows <= a.rows);
  nrows = nrows < 1 ? 1 : (nrows > a.rows ? a.rows : nrows);                    // (<= rows by the plan; a guard, not a path)
  if (ph == 1) {
    const unsigned char* base = a.src + ((size_t)b * a.slot_h + top) * a.slot_w * 3 + (size_t)left * 3;
    for (int idx = tid; idx < nrows * a.out_w; idx += nthr) {
      const int r = idx / a.out_w, x = idx - r * a.out_w;
      CROP_GUARD(r0 + r < bh);
      const int sr = r0 + r < bh ? r0 + r : bh - 1;
      const unsigned char* p = base + (size_t)sr * a.slot_w * 3 + (size_t)lox[x] * 3;
      const float* w = wx + (size_t)x * a.kx;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int k = 0; k < nx[x]; ++k) {
        s0 += w[k] * (float)p[3 * k];
        s1 += w[k] * (float)p[3 * k + 1];
        s2 += w[k] * (float)p[3 * k + 2];
      }
      inter[idx] = round_u8(s0) | (round_u8(s1) << 8) | (round_u8(s2) << 16);
    }
    return;
  }
  const bool fl = a.flip && a.flip[b] != 0;
  for (int idx = tid; idx < nband * a.out_w; idx += nthr) {
    const int i = idx / a.out_w, x = idx - i * a.out_w;
    const float* w = wy + (size_t)i * a.ky;
    const int rr = loy[i] - r0;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < ny[i]; ++k) {
      CROP_GUARD(rr + k < nrows);
      const int r = rr + k < nrows ? rr + k : nrows - 1;
      const uint32_t v = inter[(size_t)r * a.out_w + x];
      s0 += w[k] * (float)(v & 255u);
      s1 += w[k] * (float)((v >> 8) & 255u);
      s2 += w[k] * (float)(v >> 16);
    }
    const uint32_t p[3] = {round_u8(s0), round_u8(s1), round_u8(s2)};
    const int y = band0 + i, xo = fl ? a.out_w - 1 - x : x;
    if (a.out_u8) {
      unsigned char* q = a.out_u8 + (((size_t)b * a.out_h + y) * a.out_w + xo) * 3;
      q[0] = (unsigned char)p[0];
      q[1] = (unsigned char)p[1];
      q[2] = (unsigned char)p[2];
    }
    for (int ch = 0; ch < 3; ++ch) {
      const float v = a.lut[ch * 256 + p[ch]];
      const size_t o = (((size_t)b * 3 + ch) * a.out_h + y) * a.out_w + xo;
      if (a.out_bf16) ((uint16_t*)a.out)[o] = bf16_rne(v);
      else ((float*)a.out)[o] = v;
    }
  }
}

}  // namespace msclip_crop
