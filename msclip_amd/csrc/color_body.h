// The arithmetic of msclip_color_augment (include/msclip_color.h), written once for the device and for the host: color.hip runs
// `partial_sum` and `phase` from the threads of a workgroup; a host program (tests/color_host.cpp) includes this file as plain C++
// and runs the same code from one "thread" (tid 0, step 1).  No HIP type or builtin in here.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define COLOR_HD __host__ __device__ __forceinline__
#else
#define COLOR_HD static inline
#endif

namespace msclip_color {

constexpr int RADIUS = 6;             // MSCLIP_COLOR_RADIUS
constexpr int LDS_BYTES = 65536;      // MSCLIP_COLOR_LDS_BYTES
constexpr int OPS = 8, COEF = 12;     // entries per image of `ops` and `coef`

struct Args {
  const unsigned char* src;
  const int* ops;
  const float* coef;
  const float* lut;
  int B, H, W, stages;
  int* work;
  void* out;
  int out_bf16;
  unsigned char* out_u8;
  int band;                           // the plan below
};

// ---- the plan: band and LDS bytes of a blurring launch from the extents alone; false: these extents are rejected
struct Plan {
  int band, lds_bytes;
};

static inline bool make_plan(int H, int W, Plan* p) {
  if (H <= 0 || W <= 0) return false;
  const int cand[10] = {32, 24, 16, 12, 8, 6, 4, 3, 2, 1};
  for (int i = 0; i < 10; ++i) {
    const int band = cand[i] < H ? cand[i] : H;
    const long long bytes = 8ll * (band + 2 * RADIUS) * W;
    if (bytes <= LDS_BYTES) {
      p->band = band;
      p->lds_bytes = (int)bytes;
      return true;
    }
  }
  return false;
}

// ---- one image's record, read from ops / coef with the guards of the header
struct Rec {
  int order[4];                       // 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 skipped
  int cpos;                           // the position of contrast in order, 4: none
  int shift;                          // hue, 0 ... 255
  bool gray, blur;
  float f[3];                         // brightness, contrast, saturation
  float w[RADIUS + 1];
};

COLOR_HD bool finite_f(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return (u & 0x7f800000u) != 0x7f800000u;
}

COLOR_HD void read_rec(const Args& a, int b, Rec* r) {
  const int* o = a.ops + (size_t)b * OPS;
  const float* c = a.coef + (size_t)b * COEF;
  int seen = 0;
  r->cpos = 4;
  for (int i = 0; i < 4; ++i) {
    int op = o[i];
    if (!(a.stages & 1) || op < 0 || op > 3 || (seen >> op & 1)) op = -1;
    if (op >= 0) seen |= 1 << op;
    if (op == 1) r->cpos = i;
    r->order[i] = op;
  }
  r->shift = o[4] & 255;
  r->gray = (a.stages & 2) && o[5] != 0;
  r->blur = (a.stages & 4) && o[6] != 0;
  for (int i = 0; i < 3; ++i) {
    float f = c[i];
    if (!finite_f(f)) f = 1.f;
    r->f[i] = f < 0.f ? 0.f : (f > 4.f ? 4.f : f);
  }
  for (int k = 0; k <= RADIUS; ++k) r->w[k] = finite_f(c[4 + k]) ? c[4 + k] : 0.f;
}

// ---- the pointwise arithmetic
COLOR_HD int gray_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

COLOR_HD int blend(int d, int x, float f) {
  const float diff = (float)(x - d);
  const float prod = f * diff;
  const float t = (float)d + prod;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

COLOR_HD int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

COLOR_HD int round8_d(double x) {
  const double r = floor(x + 0.5);
  return r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r);
}

COLOR_HD void hue_shift(int q, int* pr, int* pg, int* pb) {
  const int r = *pr, g = *pg, b = *pb;
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  int h = 0, s8 = 0;
  const int v = maxc;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float hh;
    if (r == maxc) hh = bc - gc;
    else if (g == maxc) hh = (float)(2.0 + (double)rc - (double)bc);
    else hh = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)hh / 6.0 + 1.0;                   // in [5/6, 11/6]: fmod(x, 1.0) = x - floor(x), exactly
    hh = (float)(x - floor(x));
    h = clamp8((int)((double)hh * 255.0));
    s8 = clamp8((int)((double)s * 255.0));
  }
  h = (h + q) & 255;
  if (s8 == 0) {
    *pr = *pg = *pb = v;
    return;
  }
  const float fh6 = (float)h * 6.f;
  const float fh = fh6 / 255.f;
  const float fs = (float)s8 / 255.f;
  const float fi = floorf(fh);
  const float f = fh - fi;
  const float fv = (float)v;
  const float one_fs = 1.f - fs;
  const float fsf = fs * f;
  const float one_fsf = 1.f - fsf;
  const float one_f = 1.f - f;
  const float fs1f = fs * one_f;
  const float one_fs1f = 1.f - fs1f;
  const float pf = fv * one_fs, qf = fv * one_fsf, tf = fv * one_fs1f;
  const int p = round8_d((double)pf), qq = round8_d((double)qf), t = round8_d((double)tf);
  switch ((int)fi % 6) {
    case 0: *pr = v; *pg = t; *pb = p; break;
    case 1: *pr = qq; *pg = v; *pb = p; break;
    case 2: *pr = p; *pg = v; *pb = t; break;
    case 3: *pr = p; *pg = qq; *pb = v; break;
    case 4: *pr = t; *pg = p; *pb = v; break;
    default: *pr = v; *pg = p; *pb = qq; break;
  }
}

// the jitter ops order[first ... last) on one pixel; m: the contrast mean
COLOR_HD void jitter(const Rec& rec, int first, int last, int m, int* r, int* g, int* b) {
  for (int i = first; i < last; ++i) {
    const int op = rec.order[i];
    if (op == 0) {
      *r = blend(0, *r, rec.f[0]);
      *g = blend(0, *g, rec.f[0]);
      *b = blend(0, *b, rec.f[0]);
    } else if (op == 1) {
      *r = blend(m, *r, rec.f[1]);
      *g = blend(m, *g, rec.f[1]);
      *b = blend(m, *b, rec.f[1]);
    } else if (op == 2) {
      const int L = gray_of(*r, *g, *b);
      *r = blend(L, *r, rec.f[2]);
      *g = blend(L, *g, rec.f[2]);
      *b = blend(L, *b, rec.f[2]);
    } else if (op == 3) {
      hue_shift(rec.shift, r, g, b);
    }
  }
}

// The sum of L over the pixels tid, tid + nthr, ... of image b as it stands when contrast's turn comes (0 without contrast).
COLOR_HD unsigned long long partial_sum(const Args& a, int b, const Rec& rec, int tid, int nthr) {
  unsigned long long s = 0;
  if (rec.cpos == 4) return s;
  const size_t n = (size_t)a.H * a.W;
  const unsigned char* p = a.src + (size_t)b * n * 3;
  for (size_t i = tid; i < n; i += nthr) {
    int r = p[3 * i], g = p[3 * i + 1], bl = p[3 * i + 2];
    jitter(rec, 0, rec.cpos, 0, &r, &g, &bl);
    s += (unsigned long long)gray_of(r, g, bl);
  }
  return s;
}

COLOR_HD int mean_of(unsigned long long sum, int H, int W) {
  return (int)floor((double)sum / ((double)H * (double)W) + 0.5);
}

// jitter and grayscale of pixel (y, x) of image b -> r | g << 8 | b << 16
COLOR_HD uint32_t pointwise(const Args& a, int b, const Rec& rec, int m, int y, int x) {
  const unsigned char* p = a.src + (((size_t)b * a.H + y) * a.W + x) * 3;
  int r = p[0], g = p[1], bl = p[2];
  jitter(rec, 0, 4, m, &r, &g, &bl);
  if (rec.gray) r = g = bl = gray_of(r, g, bl);
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)bl << 16);
}

// ---- the blur
COLOR_HD int mirror(int j, int n) {
  if (j >= 0 && j < n) return j;
  if (n == 1) return 0;
  const int m = 2 * (n - 1);
  const int once = j < 0 ? -j : m - j;                   // one bounce: all an overrun of at most RADIUS needs where n > RADIUS
  if (once >= 0 && once < n) return once;
  j = ((j % m) + m) % m;
  return j >= n ? m - j : j;
}

COLOR_HD uint32_t round_u8(float x) {                    // an x that is not a number gives 0
  const float r = floorf(x + 0.5f);
  return r > 0.f ? (r >= 255.f ? 255u : (uint32_t)r) : 0u;
}

COLOR_HD uint16_t bf16_rne(float f) {                    // finite values only (the table's)
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

COLOR_HD void store(const Args& a, int b, int y, int x, uint32_t v) {
  const uint32_t p[3] = {v & 255u, (v >> 8) & 255u, v >> 16};
  if (a.out_u8) {
    unsigned char* q = a.out_u8 + (((size_t)b * a.H + y) * a.W + x) * 3;
    q[0] = (unsigned char)p[0];
    q[1] = (unsigned char)p[1];
    q[2] = (unsigned char)p[2];
  }
  for (int ch = 0; ch < 3; ++ch) {
    const float t = a.lut[ch * 256 + p[ch]];
    const size_t o = (((size_t)b * 3 + ch) * a.H + y) * a.W + x;
    if (a.out_bf16) ((uint16_t*)a.out)[o] = bf16_rne(t);
    else ((float*)a.out)[o] = t;
  }
}

// One phase of the workgroup of image b and the band of rows [band0, band0 + band): "threads" tid, tid + nthr, ...; m: work[b].
//   phase 0 (blurred images): the pointwise chain over rows band0 - 6 ... band0 + nband + 5, mirrored into the image, into `pw`
//   phase 1 (blurred images): the horizontal pass over all those rows, `pw` -> `hz`
//   phase 2: blurred images: the vertical pass out of `hz`, stores; other images: the pointwise chain, stores (no LDS touched)
// LDS, in dwords: pw [band + 12][W] | hz [band + 12][W].  A thread takes pixels with the column fastest, so the lanes of a wave read
// CONSECUTIVE dwords in both passes (horizontal: tap k of lane x is pw[r][x + k]; vertical: hz[i + k][x]): no bank conflicts
// but where the mirror folds a row's end back.
COLOR_HD void phase(const Args& a, int b, int band0, const Rec& rec, int m, uint32_t* lds, int tid, int nthr, int ph) {
  const int nband = (a.H - band0 < a.band) ? a.H - band0 : a.band;
  if (!rec.blur) {
    if (ph == 2)
      for (int idx = tid; idx < nband * a.W; idx += nthr) {
        const int i = idx / a.W, x = idx - i * a.W;
        store(a, b, band0 + i, x, pointwise(a, b, rec, m, band0 + i, x));
      }
    return;
  }
  const int rows = nband + 2 * RADIUS;
  uint32_t* pw = lds;
  uint32_t* hz = lds + (size_t)(a.band + 2 * RADIUS) * a.W;
  if (ph == 0) {
    for (int idx = tid; idx < rows * a.W; idx += nthr) {
      const int r = idx / a.W, x = idx - r * a.W;
      pw[idx] = pointwise(a, b, rec, m, mirror(band0 - RADIUS + r, a.H), x);
    }
  } else if (ph == 1) {
    for (int idx = tid; idx < rows * a.W; idx += nthr) {
      const int r = idx / a.W, x = idx - r * a.W;
      const uint32_t* row = pw + (size_t)r * a.W;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int k = -RADIUS; k <= RADIUS; ++k) {
        const float w = rec.w[k < 0 ? -k : k];
        const uint32_t v = row[mirror(x + k, a.W)];
        s0 += w * (float)(v & 255u);
        s1 += w * (float)((v >> 8) & 255u);
        s2 += w * (float)(v >> 16);
      }
      hz[idx] = round_u8(s0) | (round_u8(s1) << 8) | (round_u8(s2) << 16);
    }
  } else {
    for (int idx = tid; idx < nband * a.W; idx += nthr) {
      const int i = idx / a.W, x = idx - i * a.W;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int k = -RADIUS; k <= RADIUS; ++k) {
        const float w = rec.w[k < 0 ? -k : k];
        const uint32_t v = hz[(size_t)(i + RADIUS + k) * a.W + x];
        s0 += w * (float)(v & 255u);
        s1 += w * (float)((v >> 8) & 255u);
        s2 += w * (float)(v >> 16);
      }
      store(a, b, band0 + i, x, round_u8(s0) | (round_u8(s1) << 8) | (round_u8(s2) << 16));
    }
  }
}

}  // namespace msclip_color
