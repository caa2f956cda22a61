// The counting of msclip_rank_counts (include/msclip_metrics.h), written once for the device and for the host: metrics.hip runs
// `begin`, `stage`, `count` and `store` from the threads of a workgroup; a host program (tests/metrics_host.cpp) includes this file as
// plain C++ and runs the same code one "thread" after the other.  No HIP type or builtin in here.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define RANK_HD __host__ __device__ __forceinline__
#else
#define RANK_HD static inline
#endif

namespace msclip_rank {

constexpr int ROWS = 256;             // MSCLIP_RANK_ROWS
constexpr int STAGE = 1024;           // MSCLIP_RANK_STAGE
constexpr int LOG2_MAX_PAIRS = 42;    // MSCLIP_RANK_LOG2_MAX_PAIRS

struct Args {
  const float* S;
  int lds;
  const unsigned char* Y;
  int ldy;
  int N, C;
  int* ge_pos;
  int* ge_neg;
  int* gt_neg;                        // optional
  int ldn;
  int* npos;
  int* nbad;
};

// What the entry point rejects apart from the pointers (host arithmetic).
static inline bool shape_ok(int lds, int ldy, int N, int C, int ldn) {
  if (N < 1 || C < 1 || lds < C || ldy < C || ldn < N) return false;
  if ((unsigned long long)N > (1ull << (LOG2_MAX_PAIRS / 2))) return false;          // N * N alone is over the bound
  return (unsigned long long)C <= (1ull << LOG2_MAX_PAIRS) / ((unsigned long long)N * (unsigned long long)N);
}

// One thread's registers: its sample's score, the three counts, and its share of the column's totals.
struct Lane {
  float x;
  int ge_pos, ge_neg, gt_neg;
  int npos, nbad;
};

// Four staged scores: the LDS arrays are read 16 bytes at a time.
struct alignas(16) Quad {
  float v[4];
};

RANK_HD float quiet_nan() {
  const uint32_t u = 0x7fc00000u;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// Sample i of column c; a thread past the end holds a NaN: it counts nothing and stores nothing.
RANK_HD void begin(const Args& a, int c, long long i, Lane* l) {
  l->x = i < a.N ? a.S[(size_t)i * (size_t)a.lds + (size_t)c] : quiet_nan();
  l->ge_pos = l->ge_neg = l->gt_neg = l->npos = l->nbad = 0;
}

// Samples [j0, j0 + STAGE) of column c into the two LDS arrays (STAGE floats = STAGE / 4 Quads each): sp = the score where the label is positive, NaN
// elsewhere; sn = the reverse.  Entries past N are NaN in both.  Thread `tid` of `nthreads` fills entries tid, tid + nthreads, ...
// and adds what it staged to its share of npos / nbad.
RANK_HD void stage(const Args& a, int c, int j0, Quad* qp, Quad* qn, int tid, int nthreads, Lane* l) {
  const float nan = quiet_nan();
  float* sp = &qp[0].v[0];
  float* sn = &qn[0].v[0];
  for (int k = tid; k < STAGE; k += nthreads) {
    const long long j = (long long)j0 + k;
    float p = nan, n = nan;
    if (j < a.N) {
      const float s = a.S[(size_t)j * (size_t)a.lds + (size_t)c];
      const bool pos = a.Y[(size_t)j * (size_t)a.ldy + (size_t)c] != 0;
      if (pos) p = s; else n = s;
      l->npos += pos ? 1 : 0;
      l->nbad += (s != s) ? 1 : 0;
    }
    sp[k] = p;
    sn[k] = n;
  }
}

// The first `n` staged samples against this thread's score (n <= STAGE; the loop runs over whole Quads, whose tail is NaN).
RANK_HD void count(const Quad* qp, const Quad* qn, int n, Lane* l) {
  const float x = l->x;
  const int nq = (n + 3) >> 2;
  int gp = 0, gn = 0, tn = 0;
#ifdef __HIPCC__
#pragma unroll 4
#endif
  for (int k = 0; k < nq; ++k) {
    const Quad p = qp[k], q = qn[k];
    for (int u = 0; u < 4; ++u) {                       // (four iterations: unrolled at -O2 and above)
      gp += (p.v[u] >= x) ? 1 : 0;
      gn += (q.v[u] >= x) ? 1 : 0;
      tn += (q.v[u] > x) ? 1 : 0;
    }
  }
  l->ge_pos += gp;
  l->ge_neg += gn;
  l->gt_neg += tn;
}

RANK_HD void store(const Args& a, int c, long long i, const Lane& l) {
  if (i >= a.N) return;
  const size_t o = (size_t)c * (size_t)a.ldn + (size_t)i;
  a.ge_pos[o] = l.ge_pos;
  a.ge_neg[o] = l.ge_neg;
  if (a.gt_neg) a.gt_neg[o] = l.gt_neg;
}

}  // namespace msclip_rank
