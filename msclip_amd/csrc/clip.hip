// Gradient clipping by the global L2 norm: the sum of squares of every gradient tensor in a handful of launches, one fp32
// partial per 32 K-element chunk, then one workgroup that adds the partials in double and writes {total_norm, coef}.  The
// clipped AdamW that consumes coef is adamw_multi_kernel<true> (optim.hip).  Streaming, bound by HBM: 4 B per element, one
// more read of the gradients than the unclipped step.  Fixed addition order, no atomics: bitwise repeatable.  build.sh
// compiles this file without fast-math (pack.hip's flags): the squares are explicit fmaf, NaN and Inf must travel, and
// min(1, c) must keep a NaN.
#include "common.h"
#include "multi_tensor.h"
#include "plan.h"
#include "../../include/msclip_hip.h"
#include "../../include/msclip_ext3.h"
#include "../../include/msclip_ext4.h"

namespace {

// block b writes partials[b] (multi_tensor.h); 36 x 16 B + 400 x 4 B of kernel arguments
using SumsqBatch = MtBatch<msclip_sumsq_tensor, 36, 400>;

// Addition order of a chunk (what the error bound of tests/test_gpu_clip_grad.py counts): a thread keeps one accumulator per
// float4 component, <= 32 fmaf each, folds them as (x + y) + (z + w), adds at most one head / tail element; six xor-shuffle
// steps; (w0 + w1) + (w2 + w3) over the four waves.  <= 43 roundings on the path of any term.
__global__ __launch_bounds__(256) void sumsq_kernel(const SumsqBatch a, float* __restrict__ partials) {
  MT_DECODE_CHUNK(a, t, lo, cnt);
  const float* __restrict__ g = t.g + lo;
  // 16-byte body [v0, v1), scalar head [0, v0) and tail [v1, cnt): gradients are views at 4-byte offsets inside the buckets
  int v0 = (int)(((16 - ((size_t)g & 15)) & 15) >> 2);
  if (v0 > cnt) v0 = cnt;
  const int v1 = v0 + ((cnt - v0) & ~3);
  const int n4 = (v1 - v0) >> 2;
  const float4* __restrict__ g4 = (const float4*)(g + v0);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int i = threadIdx.x; i < n4; i += 1024) {             // four independent 16-byte loads in flight per lane
    float4 gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 256;
      gv[u] = j < n4 ? g4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      s0 = fmaf(gv[u].x, gv[u].x, s0);
      s1 = fmaf(gv[u].y, gv[u].y, s1);
      s2 = fmaf(gv[u].z, gv[u].z, s2);
      s3 = fmaf(gv[u].w, gv[u].w, s3);
    }
  }
  float s = (s0 + s1) + (s2 + s3);
  const int edge = v0 + (cnt - v1);                          // <= 6 elements
  if ((int)threadIdx.x < edge) {
    const int j = (int)threadIdx.x < v0 ? (int)threadIdx.x : v1 + ((int)threadIdx.x - v0);
    s = fmaf(g[j], g[j], s);
  }
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The fold in double of clip_coef_kernel and lamb_ratios_kernel, sumsq_kernel's tree, N sums at once: s[k] of every thread
// -> six xor-shuffle steps -> one value per wave in LDS, behind a barrier: -> red, sum k's four values from red[4 k] on.
// One call per kernel: red is one array per N, a second call would write over the first one's values.
template <int N>
__device__ __forceinline__ const double* wave_sums_double(double (&s)[N]) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] += __shfl_xor(s[k], o, 64);
  __shared__ double red[4 * N];
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) red[4 * k + (threadIdx.x >> 6)] = s[k];
  __syncthreads();
  return red;
}

// -> (w0 + w1) + (w2 + w3) over the four waves
__device__ __forceinline__ double sum_of_waves(const double* red) { return (red[0] + red[1]) + (red[2] + red[3]); }

// One workgroup: thread t adds partials t, t + 256, ... in double (a serial fp32 fold over the ~4 600 partials of the B/32 model
// would by itself allow 3e-4 of relative error), then the tree above.  GUARD = false is msclip_clip_coef's kernel: `state` is not
// read, and the instructions are those the kernel had before the parameter existed (the kernel itself is the template: the body
// as an inlined helper moved one instruction, profiles/nonfinite_guard_isa.md).  GUARD (msclip_clip_coef_guarded,
// include/msclip_ext4.h): the same fold and the same {total_norm, coef}, plus the verdict on the partials in state[0..4).
// Non-finite is read off the bit pattern (exponent field all ones), so the verdict does not depend on what a compiler flag makes
// of a floating-point comparison.  The count and the smallest index travel through a tree of their own (ints: sum and min) in
// front of the doubles'; state is written by thread 0 alone, state[1] read and written in stream order -- one workgroup, no
// atomics.
template <bool GUARD>
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partials, long long n, float max_norm,
                                                        float* __restrict__ out, int* __restrict__ state) {
  double s[1] = {0.0};
  int bad = 0, first = 0x7fffffff;
  for (long long i = threadIdx.x; i < n; i += 256) {
    s[0] += (double)partials[i];
    if constexpr (GUARD) {
      if ((__float_as_uint(partials[i]) & 0x7f800000u) == 0x7f800000u) {
        if (!bad) first = i < 0x7fffffff ? (int)i : 0x7fffffff;    // (a thread's indices grow: its first one is its smallest)
        ++bad;
      }
    }
  }
  if constexpr (GUARD) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      bad += __shfl_xor(bad, o, 64);
      const int other = __shfl_xor(first, o, 64);
      first = other < first ? other : first;
    }
    __shared__ int verdict[8];
    if ((threadIdx.x & 63) == 0) {
      verdict[threadIdx.x >> 6] = bad;
      verdict[4 + (threadIdx.x >> 6)] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int count = (verdict[0] + verdict[1]) + (verdict[2] + verdict[3]);
      int lo = verdict[4];
      for (int w = 5; w < 8; ++w) lo = verdict[w] < lo ? verdict[w] : lo;
      const int skip = count != 0;
      state[0] = skip;
      state[1] += skip;
      state[2] = skip ? lo : -1;
      state[3] = count;
    }
  }
  const double* red = wave_sums_double(s);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(sum_of_waves(red));
    const float c = max_norm / (norm + 1e-6f);               // torch: max_norm / (total_norm + 1e-6), clamped to 1 from above
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;                              // (a NaN stays a NaN, as torch.clamp keeps it)
  }
}

// LAMB's trust ratios (include/msclip_ext3.h; the partials are lamb_partials_kernel's of optim.hip, two per chunk): workgroup k
// adds parameter k's {sum p^2, sum u^2} over its chunks as clip_coef_kernel adds -- thread t takes chunks t, t + 256, ... in
// double, then the same tree.  In this file because the rule is made of comparisons that a NaN must fail and a division by Inf
// that must give 0.
__global__ __launch_bounds__(256) void lamb_ratios_kernel(const float* __restrict__ partials, const int* __restrict__ first_chunk,
                                                          int n_params, long long n_chunks, int trust_clip,
                                                          float* __restrict__ out) {
  const int k = blockIdx.x;
  long long c0 = first_chunk[k], c1 = first_chunk[k + 1];
  c0 = c0 < 0 ? 0 : (c0 > n_chunks ? n_chunks : c0);         // (a table that does not match the partials reads none beyond them)
  c1 = c1 < 0 ? 0 : (c1 > n_chunks ? n_chunks : c1);
  double s[2] = {0.0, 0.0};                                  // sum p^2, sum u^2
  for (long long c = c0 + threadIdx.x; c < c1; c += 256) {
    s[0] += (double)partials[2 * c];
    s[1] += (double)partials[2 * c + 1];
  }
  const double* red = wave_sums_double(s);
  if (threadIdx.x == 0) {
    const float wn = (float)sqrt(sum_of_waves(red)), un = (float)sqrt(sum_of_waves(red + 4));
    float r = (wn > 0.f && un > 0.f) ? wn / un : 1.f;        // NaN: both comparisons false; un = Inf: 0
    if (trust_clip && r > 1.f) r = 1.f;
    out[k] = r;
    out[(size_t)n_params + k] = wn;
    out[2 * (size_t)n_params + k] = un;
  }
}

}  // namespace

extern "C" int msclip_grad_sumsq(const msclip_sumsq_tensor* tensors, int count, float* partials, long long n_partials,
                                 void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_grad_sumsq);
  if (!tensors || count < 0 || !partials || ((size_t)partials & 3) || n_partials < 0) return MSCLIP_EINVAL;
  long long need = 0;
  for (int i = 0; i < count; ++i) {
    if (!tensors[i].g || tensors[i].n <= 0 || ((size_t)tensors[i].g & 3)) return MSCLIP_EINVAL;
    need += (tensors[i].n + MT_CHUNK - 1) / MT_CHUNK;
  }
  if (need != n_partials) return MSCLIP_EINVAL;              // every slot the fold will read is written, none beyond the array
  mt_for_each_launch<SumsqBatch>(
      tensors, count,
      [](msclip_sumsq_tensor& t, long long k) {
        t.g += k;
        t.n -= k;
      },
      [&](const SumsqBatch& b, int nb, long long first_chunk) {
        hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, partials + first_chunk);
      });
  return msclip_launch_status();
}

extern "C" int msclip_clip_coef(const float* partials, long long n, float max_norm, float* out, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_clip_coef, stream, partials, n, max_norm, out);
  if (!partials || !out || n <= 0 || !(max_norm >= 0.f) || (((size_t)partials | (size_t)out) & 3)) return MSCLIP_EINVAL;
  hipLaunchKernelGGL(clip_coef_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, max_norm, out, (int*)nullptr);
  return msclip_launch_status();
}

extern "C" int msclip_clip_coef_guarded(const float* partials, long long n, float max_norm, float* out, int* state, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_clip_coef_guarded, stream, partials, n, max_norm, out, state);
  if (!partials || !out || !state || n <= 0 || !(max_norm >= 0.f) || (((size_t)partials | (size_t)out | (size_t)state) & 3))
    return MSCLIP_EINVAL;
  hipLaunchKernelGGL(clip_coef_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n, max_norm, out, state);
  return msclip_launch_status();
}

extern "C" int msclip_lamb_ratios(const float* partials, const int* first_chunk_dev, int n_params, long long n_chunks,
                                  int trust_clip, float* out, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_lamb_ratios, stream, partials, first_chunk_dev, n_params, n_chunks, trust_clip, out);
  if (!partials || !first_chunk_dev || !out || n_params <= 0 || n_chunks <= 0 ||
      (((size_t)partials | (size_t)first_chunk_dev | (size_t)out) & 3))
    return MSCLIP_EINVAL;
  hipLaunchKernelGGL(lamb_ratios_kernel, dim3(n_params), dim3(256), 0, (hipStream_t)stream, partials, first_chunk_dev, n_params,
                     n_chunks, trust_clip, out);
  return msclip_launch_status();
}
