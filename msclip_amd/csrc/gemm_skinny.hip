// Latency-tuned dense GEMM for the small-M launches behind msclip_gemm's "dense128" choice (the live rows of the compact
// last block and the two heads: M = 1024 or 512 rows, N = 512 .. 3072, K = 768 .. 3072).
//
//   out[m, n] = epilogue( alpha * sum_k X[m, k] * W[n, k] )        (same operands and epilogue forms as gemm_kernel<0, ...>)
//
// At these shapes 128 x 128 tiles leave most CUs without a workgroup and the launch time is K-steps x one memory round
// trip.  This kernel trades tile size for workgroups and keeps the memory pipe full instead:
//  * 64 x 64 output tiles, one per workgroup (4 waves as 2 x 2, one 32 x 32 MFMA tile each): M = 1024, N = 768 is 192
//    workgroups, c_fc 768;
//  * a ring of SK_RING 64-deep K-slabs in LDS (16 KiB each: X rows | W rows, the XOR-swizzled lane-linear image of
//    gemm_kernel), filled by LDS-DMA SK_RING - 1 slabs ahead.  A K-step waits with a COUNTED vmcnt for its own slab only
//    (the younger slabs stay in flight across the raw barrier), so it costs issue time, not a round trip;
//  * every output tile is contracted by one wave in K order with the instruction and operand order of gemm_kernel: no
//    split-K, no atomics, no workspace.
// Ordering of the ring (one barrier per K-step).  RAW: a wave's "s_waitcnt vmcnt(N)" retires its own pieces of slab kt, the
// barrier behind it publishes every wave's; the fragment reads follow that barrier.  WAR: slab kt + SK_RING - 1 overwrites
// the buffer of slab kt - 1; it is issued behind the same barrier, which every wave reaches only after the fragment reads
// of slab kt - 1 have returned (lgkmcnt(0) in the same wait).
#include <stdlib.h>
#include "common.h"
#include "../../include/msclip_hip.h"
#include "gemm_epilogue.h"

namespace {

constexpr int BK = 64;
constexpr int SK_BM = 64, SK_BN = 64;
constexpr int SK_RING = 4;                               // K-slabs of LDS; SK_RING - 1 are in flight ahead of the MFMAs
constexpr int SK_SLAB = (SK_BM + SK_BN) * BK;            // bf16 elements per slab
constexpr int SK_PIECES = (SK_BM + SK_BN) / 8 / 4;       // 1-KiB LDS-DMA pieces per wave and slab

template <int N>
__device__ __forceinline__ void sk_wait() {              // all but this wave's youngest N LDS-DMA pieces have landed
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}

template <int D>
__device__ __forceinline__ void sk_wait_younger(int younger) {   // wave-uniform: min(younger, D) whole slabs stay in flight
  if constexpr (D == 0) {
    sk_wait<0>();
  } else {
    if (younger >= D) sk_wait<D * SK_PIECES>();
    else sk_wait_younger<D - 1>(younger);
  }
}

__global__ __launch_bounds__(256) void gemm_skinny_kernel(const msclip_gemm_desc a) {
  static_assert(SK_RING >= 3 && (SK_RING - 2) * SK_PIECES <= 63, "ring depth against the 6-bit vmcnt");
  static_assert(SK_SLAB * 2 >= 4 * STG_BYTES, "one slab holds the four waves' staging");
  __shared__ __attribute__((aligned(1024))) bf16_t smem[SK_RING * SK_SLAB];   // [slab][X rows | W rows][64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int nt_n = (a.N + SK_BN - 1) / SK_BN;
  const int ntiles = (int)gridDim.x;
  int m0, n0;
  {
    // XCD-aware bijective remap: tiles with consecutive ids run on one XCD (they share X rows in its L2)
    const int t = (int)blockIdx.x;
    const int q = ntiles >> 3, r = ntiles & 7, x = t & 7;
    const int id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (t >> 3);
    m0 = (id / nt_n) * SK_BM;
    n0 = (id % nt_n) * SK_BN;
  }

  // ---- loader: piece i of the wave covers rows (i * 4 + wave) * 8 + lane / 8 of X (i < 2) and of W; physical chunk lane % 8
  // holds logical chunk pc ^ ((row >> 1) & 7)
  const bf16_t* __restrict__ Z = (const bf16_t*)a.zero;
  const int pc = lane & 7;
  const int lc = pc ^ ((lane >> 4) | ((wave & 1) << 2));
  const int rsub = lane >> 3;
  const bf16_t* src[SK_PIECES];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (i * 4 + wave) * 8 + rsub;
    const int n = n0 + (i * 4 + wave) * 8 + rsub;
    src[i] = m < a.M ? (const bf16_t*)a.X + (size_t)m * a.ldx + lc * 8 : nullptr;
    src[2 + i] = n < a.N ? (const bf16_t*)a.W + (size_t)n * a.ldw + lc * 8 : nullptr;
  }
  auto issue = [&](int kt) {                             // slab kt -> ring buffer kt % SK_RING
    bf16_t* dst = smem + (kt % SK_RING) * SK_SLAB + wave * 8 * BK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(src[i] ? src[i] + kt * BK : Z, dst + i * 32 * BK);
      glds16(src[2 + i] ? src[2 + i] + kt * BK : Z, dst + SK_BM * BK + i * 32 * BK);
    }
  };

  const int nk = a.K / BK;
#pragma unroll
  for (int s = 0; s < SK_RING - 1; ++s)
    if (s < nk) issue(s);

  // ---- fragment reads: the wave's 32 W rows (MFMA A operand) and 32 X rows (B operand)
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int fr = lane & 31, fhi = lane >> 5;
  const int fsw = (lane >> 1) & 7;
  f32x16 acc[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;

  for (int kt = 0; kt < nk; ++kt) {
    sk_wait_younger<SK_RING - 2>(nk - 1 - kt);           // slabs issued behind slab kt: min(nk - 1 - kt, SK_RING - 2)
    __builtin_amdgcn_s_barrier();
    if (kt + SK_RING - 1 < nk) issue(kt + SK_RING - 1);
    const bf16_t* buf = smem + (kt % SK_RING) * SK_SLAB;
    const bf16_t* xs = buf + (wm + fr) * BK;
    const bf16_t* ws = buf + SK_BM * BK + (wn + fr) * BK;
    bf16x8 wf[4], xf[4];                                 // all eight reads first: one LDS latency per slab, not four
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ph = ((kk * 2 + fhi) ^ fsw) * 8;
      wf[kk] = *(const bf16x8*)(ws + ph);
      xf[kk] = *(const bf16x8*)(xs + ph);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[kk], xf[kk], acc[0][0], 0, 0, 0);
  }

  // ---- epilogue.  No LDS-DMA is in flight (the last K-step waited for everything) and every wave has passed the last
  // barrier, so only the last slab's buffer may still be read: the buffer after it is the staging area.
  const bool vec = !((a.N | a.ldo | (a.resid_kind ? a.ldr : 0)) & 3);
  if (vec && m0 + SK_BM <= a.M)
    epilogue_interior<1, 1>(acc, a, (char*)(smem + (nk % SK_RING) * SK_SLAB) + wave * STG_BYTES, m0 + wm, n0 + wn, lane);
  else
    epilogue_generic<1, 1>(acc, a, vec, m0 + wm, n0 + wn, lane);
}

}  // namespace

// Does the small-M kernel take this launch of the "dense128" variant?  Everything it does not carry (row scatter, table /
// bf16 / masked residuals, ReLU, the training-step and LayerNorm-fold forms, device-side row counts, an explicit tile or
// workgroup cap) stays with gemm_kernel<0, 128, 128, 2, 2>, and so does every problem whose 128 x 128 grid fills the chip.
static bool skinny_eligible(const msclip_gemm_desc* d, int ncu) {
  if (d->mode != 0 || d->tile != 0 || d->wg_cap || (d->K % BK)) return false;
  if ((long long)((d->M + 127) / 128) * ((d->N + 127) / 128) >= ncu) return false;
  if (d->resid_kind < 0 || d->resid_kind > 1 || (d->resid_kind == 1 && !d->resid)) return false;
  if (d->out_kind < 0 || d->out_kind > 1 || d->act < 0 || d->act > 1) return false;
  if (d->rpg != 0x7fffffff || d->roff) return false;
  if (d->M_dev || d->out2 || d->W2 || d->rowstat || d->xb || d->part || d->bn_mode || d->resid2) return false;
  return true;
}

// Takes the launch if the problem qualifies; MSCLIP_GEMM_SKINNY=0 keeps the 128 x 128 kernel (A/B runs, cross-checks).
bool msclip_gemm_skinny_try(const msclip_gemm_desc* d, hipStream_t st, int ncu) {
  const char* sw = getenv("MSCLIP_GEMM_SKINNY");
  if (sw && sw[0] == '0') return false;
  if (!skinny_eligible(d, ncu)) return false;
  const int tiles = ((d->M + SK_BM - 1) / SK_BM) * ((d->N + SK_BN - 1) / SK_BN);
  hipLaunchKernelGGL(gemm_skinny_kernel, dim3(tiles), dim3(256), 0, st, *d);
  return true;
}
