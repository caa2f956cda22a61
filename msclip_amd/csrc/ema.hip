// Exponential moving average of the weights (TRAIN.EMA_DECAY): shadow = decay * shadow + (1 - decay) * parameter over all
// parameter tensors in a handful of launches (multi_tensor.h), after the AdamW launch of a training step.  Streaming, bound
// by HBM: 12 B per element, accumulate_kernel<1>'s traffic and access pattern (optim.hip).  A launch of its own on a table of
// its own: fused into AdamW it would move 8 B, but msclip_adamw_tensor and adamw_multi_kernel are pinned as they are.
// build.sh compiles this file without fast-math and without contraction (pack.hip's flags): the update is three separately
// rounded IEEE operations, which is what makes it bitwise torch's `d * s + (1. - d) * p`; in optim.hip it would become an fma.
#include "common.h"
#include "multi_tensor.h"
#include "plan.h"
#include "../../include/msclip_ext.h"

#pragma clang fp contract(off)                               // (whatever the command line says)

namespace {

// 36 x 24 B + 768 x 4 B of kernel arguments
using EmaBatch = MtBatch<msclip_ema_tensor, 36, 768>;

__device__ __forceinline__ float ema_update(float s, float p, float d, float omd) { return d * s + omd * p; }

__global__ __launch_bounds__(256) void ema_kernel(const EmaBatch a, float d, float omd) {
  MT_DECODE_CHUNK(a, t, lo, cnt);
  float* __restrict__ s = t.ema + lo;
  const float* __restrict__ p = t.p + lo;
  // 16-byte body [v0, v1) where ema and p sit at the same offset within 16 bytes (a piece starts a multiple of 128 KiB behind
  // its tensor, so that holds for every piece of a tensor or for none); scalar head [0, v0) and tail [v1, cnt)
  int v0 = 0, v1 = 0;
  if (!(((size_t)s ^ (size_t)p) & 15)) {
    v0 = (int)(((16 - ((size_t)s & 15)) & 15) >> 2);
    if (v0 > cnt) v0 = cnt;
    v1 = v0 + ((cnt - v0) & ~3);
  }
  const int edge = v0 + (cnt - v1);
  for (int i = threadIdx.x; i < edge; i += 256) {
    const int j = i < v0 ? i : v1 + (i - v0);
    s[j] = ema_update(s[j], p[j], d, omd);
  }
  const int n4 = (v1 - v0) >> 2;
  float4* __restrict__ s4 = (float4*)(s + v0);
  const float4* __restrict__ p4 = (const float4*)(p + v0);
  for (int i = threadIdx.x; i < n4; i += 1024) {             // four independent 16-byte loads per operand in flight per lane
    float4 pv[4], sv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 256;
      if (j < n4) {
        pv[u] = p4[j];
        sv[u] = s4[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 256;
      if (j < n4)
        s4[j] = make_float4(ema_update(sv[u].x, pv[u].x, d, omd), ema_update(sv[u].y, pv[u].y, d, omd),
                            ema_update(sv[u].z, pv[u].z, d, omd), ema_update(sv[u].w, pv[u].w, d, omd));
    }
  }
}

}  // namespace

extern "C" int msclip_ext_abi_version(void) { return MSCLIP_EXT_ABI_VERSION; }

extern "C" int msclip_ema_multi(const msclip_ema_tensor* tensors, int count, float decay, float one_minus_decay, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_ema_multi);
  if (count < 0 || (!tensors && count > 0)) return MSCLIP_EINVAL;
  if (!(decay >= 0.f && decay <= 1.f) || !(one_minus_decay >= 0.f && one_minus_decay <= 1.f)) return MSCLIP_EINVAL;   // (NaN included)
  for (int i = 0; i < count; ++i)
    if (!tensors[i].ema || !tensors[i].p || tensors[i].n <= 0 || (((size_t)tensors[i].ema | (size_t)tensors[i].p) & 3))
      return MSCLIP_EINVAL;
  mt_for_each_launch<EmaBatch>(
      tensors, count,
      [](msclip_ema_tensor& t, long long k) {
        t.ema += k;
        t.p += k;
        t.n -= k;
      },
      [&](const EmaBatch& b, int nb, long long) {
        hipLaunchKernelGGL(ema_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, decay, one_minus_decay);
      });
  return msclip_launch_status();
}
