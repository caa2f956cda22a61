// The optimizer phase of the training step: AdamW and LAMB over all parameter tensors and gradient accumulation over the chunks
// of TrainStep.accumulate (train.py), each over its 325-406 tensors in a handful of launches (multi_tensor.h).  Streaming, bound
// by HBM.  The sum of squares and the coefficient of gradient clipping are in clip.hip, which is compiled without fast-math.
#include "common.h"
#include "multi_tensor.h"
#include "plan.h"
#include "../../include/msclip_hip.h"
#include "../../include/msclip_ext3.h"
#include "../../include/msclip_ext4.h"

namespace {

// ---- AdamW (decoupled weight decay), one fused pass per parameter tensor; fp32 states.  One statement of the update with
// the contractions written out, shared by every kernel below: their results are bitwise the same.  adam_direction forms the
// new moments and u = m_hat / (sqrt(v_hat) + eps) + wd * p, adamw_update steps along it.
__device__ __forceinline__ float adam_direction(float gi, float& mi, float& vi, float pi, float b1, float b2, float eps, float wd,
                                                float c1, float c2) {
  mi = __fmaf_rn(b1, mi, (1.f - b1) * gi);
  vi = __fmaf_rn(b2, vi, (1.f - b2) * gi * gi);
  return __fmaf_rn(wd, pi, mi * c1 / (sqrtf(vi * c2) + eps));
}

__device__ __forceinline__ void adamw_update(float gi, float& mi, float& vi, float& pi, float lr, float b1, float b2, float eps,
                                             float wd, float c1, float c2) {
  pi = __fmaf_rn(-lr, adam_direction(gi, mi, vi, pi, b1, b2, eps, wd, c1, c2), pi);
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, size_t n, float lr, float b1, float b2, float eps,
                                                    float wd, float c1, float c2) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float mi = m[i], vi = v[i], pi = p[i];
    adamw_update(g[i], mi, vi, pi, lr, b1, b2, eps, wd, c1, c2);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// ---- the same update over many tensors per launch (multi_tensor.h): 36 x 64 B + 400 x 4 B of kernel arguments
using AdamwBatch = MtBatch<msclip_adamw_tensor, 36, 400>;

// CLIP (msclip_adamw_multi_clipped, the LAMB calls with a coefficient): the update sees g[i] * coef[0], the clipping coefficient
// that msclip_clip_coef left on the device.  The product is ONE fp32 multiply, rounded before the moment updates -- the value
// torch's clip_grad_norm_ stores back into .grad: the empty asm keeps this file's fast-math from re-associating
// (1 - b1) * (g * coef) into ((1 - b1) * coef) * g.  CLIP = false: coef is not read.
template <bool CLIP>
__device__ __forceinline__ float clipped(float gi, float coef) {
  if constexpr (CLIP) {
    gi *= coef;
    asm volatile("" : "+v"(gi));
  }
  return gi;
}

// The update of one chunk, the body of adamw_multi_kernel and lamb_apply_kernel: 16-byte path where every operand allows it,
// 4-byte path for the rest.  pkb / pkf: the packed copy of the new values (the engine's GEMM operand) in bf16 or fp32, or both
// null: same rounding as a cast of the updated tensor.  Operands by value, not the table item by reference, for the reason
// MT_DECODE_CHUNK is a macro (multi_tensor.h); profiles/optim_dedup_isa.md compares the kernels with their earlier text.
template <bool CLIP>
__device__ __forceinline__ void adamw_apply_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, bf16_t* __restrict__ pkb, float* __restrict__ pkf, float ps,
                                                  int cnt, float lr, float wd, float coef, float b1, float b2, float eps, float c1,
                                                  float c2) {
  auto upd = [&](float gi, float& mi, float& vi, float& pi) {
    adamw_update(clipped<CLIP>(gi, coef), mi, vi, pi, lr, b1, b2, eps, wd, c1, c2);
  };
  int i0 = 0;
  if (!(((size_t)p | (size_t)g | (size_t)m | (size_t)v | (size_t)pkf) & 15) && !((size_t)pkb & 7)) {
    const int n4 = cnt >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const float4 g4 = ((const float4*)g)[i];
      float4 m4 = ((float4*)m)[i], v4 = ((float4*)v)[i], p4 = ((float4*)p)[i];
      upd(g4.x, m4.x, v4.x, p4.x);
      upd(g4.y, m4.y, v4.y, p4.y);
      upd(g4.z, m4.z, v4.z, p4.z);
      upd(g4.w, m4.w, v4.w, p4.w);
      ((float4*)m)[i] = m4;
      ((float4*)v)[i] = v4;
      ((float4*)p)[i] = p4;
      if (pkb) ((uint2*)pkb)[i] = make_uint2(pack_bf16x2(p4.x * ps, p4.y * ps), pack_bf16x2(p4.z * ps, p4.w * ps));
      if (pkf) ((float4*)pkf)[i] = make_float4(p4.x * ps, p4.y * ps, p4.z * ps, p4.w * ps);
    }
    i0 = n4 << 2;
  }
  for (int i = i0 + threadIdx.x; i < cnt; i += 256) {
    float mi = m[i], vi = v[i], pi = p[i];
    upd(g[i], mi, vi, pi);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (pkb) pkb[i] = f32_to_bf16(pi * ps);
    if (pkf) pkf[i] = pi * ps;
  }
}

// GUARD (include/msclip_ext4.h): every workgroup reads the verdict skip_dev[0] of msclip_clip_coef_guarded once, a uniform read
// at its head, and leaves where it is not 0 -- a skipped step writes no p, m, v and no packed copy.  GUARD = false: skip_dev is
// not read, and the kernel is the one it was before the parameter existed (profiles/nonfinite_guard_isa.md).
template <bool CLIP, bool GUARD>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const AdamwBatch a, float b1, float b2, float eps, float c1, float c2,
                                                          const float* __restrict__ coef_dev, const int* __restrict__ skip_dev) {
  if constexpr (GUARD) {
    if (*skip_dev) return;
  }
  float coef = 1.f;
  if constexpr (CLIP) coef = *coef_dev;
  MT_DECODE_CHUNK(a, t, lo, cnt);
  const float lr = t.lr, wd = t.weight_decay;                // (read first: their load then leaves with the item's other loads)
  adamw_apply_chunk<CLIP>(t.p + lo, t.g + lo, t.m + lo, t.v + lo, t.pk && !t.pk_f32 ? (bf16_t*)t.pk + lo : nullptr,
                          t.pk && t.pk_f32 ? (float*)t.pk + lo : nullptr, t.pk_scale, cnt, lr, wd, coef, b1, b2, eps, c1, c2);
}

// ---- gradient accumulation: 8 B per element in mode 0 (acc = g), 12 B in mode 1 (acc += g).  One IEEE add per element in
// call order, no atomics: bitwise torch's acc + g and bitwise repeatable.  36 x 24 B + 768 x 4 B of kernel arguments.
using AccumBatch = MtBatch<msclip_accum_tensor, 36, 768>;

template <int MODE>
__global__ __launch_bounds__(256) void accumulate_kernel(const AccumBatch a) {
  MT_DECODE_CHUNK(a, t, lo, cnt);
  float* __restrict__ acc = t.acc + lo;
  const float* __restrict__ g = t.g + lo;
  // 16-byte body [v0, v1) where acc and g sit at the same offset within 16 bytes (a piece starts a multiple of 128 KiB behind
  // its tensor, so that holds for every piece of a tensor or for none); scalar head [0, v0) and tail [v1, cnt)
  int v0 = 0, v1 = 0;
  if (!(((size_t)acc ^ (size_t)g) & 15)) {
    v0 = (int)(((16 - ((size_t)acc & 15)) & 15) >> 2);
    if (v0 > cnt) v0 = cnt;
    v1 = v0 + ((cnt - v0) & ~3);
  }
  const int edge = v0 + (cnt - v1);
  for (int i = threadIdx.x; i < edge; i += 256) {
    const int j = i < v0 ? i : v1 + (i - v0);
    acc[j] = MODE ? acc[j] + g[j] : g[j];
  }
  const int n4 = (v1 - v0) >> 2;
  float4* __restrict__ a4 = (float4*)(acc + v0);
  const float4* __restrict__ g4 = (const float4*)(g + v0);
  for (int i = threadIdx.x; i < n4; i += 1024) {           // four independent 16-byte loads per operand in flight per lane
    float4 gv[4], av[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 256;
      if (j < n4) {
        gv[u] = g4[j];
        if (MODE) av[u] = a4[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 256;
      if (j < n4) {
        if (MODE) gv[u] = make_float4(av[u].x + gv[u].x, av[u].y + gv[u].y, av[u].z + gv[u].z, av[u].w + gv[u].w);
        a4[j] = gv[u];
      }
    }
  }
}

// ---- LAMB (include/msclip_ext3.h): a trust ratio ||w|| / ||u|| per parameter tensor scales the rate of the AdamW update.  u
// exists only inside the update, so the step is two passes over the table: lamb_partials_kernel forms the new moments and u
// in registers and leaves the sums of p^2 and u^2 of every chunk (16 B read per element), lamb_ratios_kernel (clip.hip) folds
// them per parameter, lamb_apply_kernel runs adamw_multi_kernel's body with the rate scaled (28 B per element).  A table of
// its own (the item carries its parameter and whether it adapts): 32 x 72 B + 400 x 4 B of kernel arguments.
using LambBatch = MtBatch<msclip_lamb_tensor, 32, 400>;

// a + b as written: this file's fast-math may not re-associate the folds below (the addition order is what the error bound of
// tests/test_gpu_lamb.py counts, sumsq_kernel's of clip.hip)
__device__ __forceinline__ float add_fixed(float a, float b) {
  float s = a + b;
  asm volatile("" : "+v"(s));
  return s;
}

// Block b writes partials[2 b] = sum p^2 and partials[2 b + 1] = sum u^2 of its chunk.  Addition order, for either sum: a
// thread keeps four accumulators of <= 32 fmaf each (the float4 components in the 16-byte body; elements tid + 256 (4 k + j)
// for accumulator j on the 4-byte path), folds them as (s0 + s1) + (s2 + s3), adds at most one tail element of the body; six xor-shuffle
// steps; (w0 + w1) + (w2 + w3) over the four waves.  <= 43 roundings on the path of any term.
template <bool CLIP>
__global__ __launch_bounds__(256) void lamb_partials_kernel(const LambBatch a, float b1, float b2, float eps, float c1, float c2,
                                                            const float* __restrict__ coef_dev, float* __restrict__ partials) {
  float coef = 1.f;
  if constexpr (CLIP) coef = *coef_dev;
  MT_DECODE_CHUNK(a, t, lo, cnt);
  const float* __restrict__ p = t.p + lo;
  const float* __restrict__ g = t.g + lo;
  const float* __restrict__ m = t.m + lo;
  const float* __restrict__ v = t.v + lo;
  const float wd = t.weight_decay;
  auto dir = [&](float gi, float mi, float vi, float pi) {   // u of adamw_update on copies of the moments: this pass stores none
    return adam_direction(clipped<CLIP>(gi, coef), mi, vi, pi, b1, b2, eps, wd, c1, c2);
  };
  float sp[4] = {0.f, 0.f, 0.f, 0.f}, su[4] = {0.f, 0.f, 0.f, 0.f};
  int i0 = 0;
  if (!(((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15)) {
    const int n4 = cnt >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {            // four independent 16-byte loads in flight per lane
      const float4 g4 = ((const float4*)g)[i], m4 = ((const float4*)m)[i], v4 = ((const float4*)v)[i], p4 = ((const float4*)p)[i];
      const float ux = dir(g4.x, m4.x, v4.x, p4.x), uy = dir(g4.y, m4.y, v4.y, p4.y);
      const float uz = dir(g4.z, m4.z, v4.z, p4.z), uw = dir(g4.w, m4.w, v4.w, p4.w);
      sp[0] = __fmaf_rn(p4.x, p4.x, sp[0]);
      sp[1] = __fmaf_rn(p4.y, p4.y, sp[1]);
      sp[2] = __fmaf_rn(p4.z, p4.z, sp[2]);
      sp[3] = __fmaf_rn(p4.w, p4.w, sp[3]);
      su[0] = __fmaf_rn(ux, ux, su[0]);
      su[1] = __fmaf_rn(uy, uy, su[1]);
      su[2] = __fmaf_rn(uz, uz, su[2]);
      su[3] = __fmaf_rn(uw, uw, su[3]);
    }
    i0 = n4 << 2;                                            // <= 3 elements are left
  } else {
    for (int i = threadIdx.x; i < cnt; i += 1024) {          // rounds of 4 x 256 elements, accumulator j takes the j-th quarter
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = i + j * 256;
        if (k < cnt) {
          const float pi = p[k], ui = dir(g[k], m[k], v[k], pi);
          sp[j] = __fmaf_rn(pi, pi, sp[j]);
          su[j] = __fmaf_rn(ui, ui, su[j]);
        }
      }
    }
    i0 = cnt;
  }
  float s_p = add_fixed(add_fixed(sp[0], sp[1]), add_fixed(sp[2], sp[3]));
  float s_u = add_fixed(add_fixed(su[0], su[1]), add_fixed(su[2], su[3]));
  const int k = i0 + (int)threadIdx.x;                       // the tail: at most one element per thread
  if (k < cnt) {
    const float pi = p[k], ui = dir(g[k], m[k], v[k], pi);
    s_p = __fmaf_rn(pi, pi, s_p);
    s_u = __fmaf_rn(ui, ui, s_u);
  }
  s_p = wave_sum(s_p);
  s_u = wave_sum(s_u);
  __shared__ float red[8];
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = s_p;
    red[4 + (threadIdx.x >> 6)] = s_u;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (size_t)blockIdx.x] = add_fixed(add_fixed(red[0], red[1]), add_fixed(red[2], red[3]));
    partials[2 * (size_t)blockIdx.x + 1] = add_fixed(add_fixed(red[4], red[5]), add_fixed(red[6], red[7]));
  }
}

// adamw_multi_kernel with the item's rate scaled by its parameter's trust ratio: lr_eff is ONE fp32 multiply, rounded -- the
// empty asm keeps fast-math from folding it into the update -- and adamw_update sees it as its lr.
// GUARD: as in adamw_multi_kernel.
template <bool CLIP, bool GUARD>
__global__ __launch_bounds__(256) void lamb_apply_kernel(const LambBatch a, float b1, float b2, float eps, float c1, float c2,
                                                         const float* __restrict__ coef_dev, const float* __restrict__ ratio_dev,
                                                         const int* __restrict__ skip_dev) {
  if constexpr (GUARD) {
    if (*skip_dev) return;
  }
  float coef = 1.f;
  if constexpr (CLIP) coef = *coef_dev;
  MT_DECODE_CHUNK(a, t, lo, cnt);
  float* p = t.p + lo;                                       // (in front of the rate: the item's loads then leave together)
  const float* g = t.g + lo;
  float* m = t.m + lo;
  float* v = t.v + lo;
  float lr_eff = t.lr;
  if (t.adapt) {
    lr_eff *= ratio_dev[t.param];
    asm volatile("" : "+v"(lr_eff));
  }
  adamw_apply_chunk<CLIP>(p, g, m, v, t.pk && !t.pk_f32 ? (bf16_t*)t.pk + lo : nullptr,
                          t.pk && t.pk_f32 ? (float*)t.pk + lo : nullptr, t.pk_scale, cnt, lr_eff, t.weight_decay, coef, b1, b2, eps,
                          c1, c2);
}

// ---- host side, common to the AdamW and the LAMB tables (their items share p, g, m, v, n, pk, pk_f32)
template <class T>
void adam_advance(T& t, long long k) {
  t.p += k;
  t.g += k;
  t.m += k;
  t.v += k;
  t.n -= k;
  if (t.pk) t.pk = (char*)t.pk + (size_t)k * (t.pk_f32 ? 4 : 2);
}

// The bias corrections 1 / (1 - beta^step) of the two moments.  beta^step is powf's in the AdamW calls and repeated squaring
// (SQUARING, __builtin_powif) in the LAMB calls: what this file's fast-math made of the one expression powf(beta, (float)step)
// in the two kinds of entry point while each wrote it out, and what each therefore has always computed; the two can differ in
// the last bit.  Stated here so that neither depends on the code around the call: the empty asm keeps powf a call of powf.
struct BiasCorrections { float c1, c2; };
template <bool SQUARING>
BiasCorrections bias_corrections(float beta1, float beta2, int step) {
  float fstep = (float)step;
  asm volatile("" : "+m"(fstep));
  const float p1 = SQUARING ? __builtin_powif(beta1, step) : powf(beta1, fstep);
  const float p2 = SQUARING ? __builtin_powif(beta2, step) : powf(beta2, fstep);
  return {1.f / (1.f - p1), 1.f / (1.f - p2)};
}

// what every table must satisfy before a kernel may see it; an entry point adds its own conditions
template <class T>
bool adam_table_ok(const T* tensors, int count, int step) {
  if (!tensors || count < 0 || step < 1) return false;
  for (int i = 0; i < count; ++i) {
    const T& t = tensors[i];
    if (!t.p || !t.g || !t.m || !t.v || t.n <= 0 || (t.pk && (t.pk_f32 < 0 || t.pk_f32 > 1))) return false;
  }
  return true;
}

// the CLIP instantiation of a kernel: the clipped one where a coefficient is given
template <class Kernel>
Kernel pick_clip(const float* coef_dev, Kernel clipped, Kernel plain) {
  return coef_dev ? clipped : plain;
}

// skip_dev: NULL, or the verdict of the guarded entry points (include/msclip_ext4.h); every launch of the call is handed it
int adamw_multi_launch(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                       const float* coef_dev, const int* skip_dev, void* stream) {
  if (!adam_table_ok(tensors, count, step)) return MSCLIP_EINVAL;
  const BiasCorrections bc = bias_corrections<false>(beta1, beta2, step);
  const auto kernel = skip_dev ? pick_clip(coef_dev, adamw_multi_kernel<true, true>, adamw_multi_kernel<false, true>)
                               : pick_clip(coef_dev, adamw_multi_kernel<true, false>, adamw_multi_kernel<false, false>);
  mt_for_each_launch<AdamwBatch>(tensors, count, adam_advance<msclip_adamw_tensor>, [&](const AdamwBatch& b, int nb, long long) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, bc.c1, bc.c2, coef_dev, skip_dev);
  });
  return msclip_launch_status();
}

int lamb_apply_launch(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                      const float* coef_dev, const float* ratio_dev, const int* skip_dev, void* stream) {
  const BiasCorrections bc = bias_corrections<true>(beta1, beta2, step);
  const auto kernel = skip_dev ? pick_clip(coef_dev, lamb_apply_kernel<true, true>, lamb_apply_kernel<false, true>)
                               : pick_clip(coef_dev, lamb_apply_kernel<true, false>, lamb_apply_kernel<false, false>);
  mt_for_each_launch<LambBatch>(tensors, count, adam_advance<msclip_lamb_tensor>, [&](const LambBatch& b, int nb, long long) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, bc.c1, bc.c2, coef_dev, ratio_dev,
                       skip_dev);
  });
  return msclip_launch_status();
}

// -> the chunk count of the table, or -1 for a table that no kernel may see
long long lamb_table_chunks(const msclip_lamb_tensor* tensors, int count, int step, const float* coef_dev) {
  if (!adam_table_ok(tensors, count, step) || ((size_t)coef_dev & 3)) return -1;
  long long chunks = 0;
  for (int i = 0; i < count; ++i) {
    const msclip_lamb_tensor& t = tensors[i];
    if (((size_t)t.p | (size_t)t.g | (size_t)t.m | (size_t)t.v) & 3) return -1;
    const int prev = i ? tensors[i - 1].param : -1;          // 0, then the same parameter or the next one
    if (t.param != prev && t.param != prev + 1) return -1;
    if (i == 0 && t.param != 0) return -1;
    chunks += (t.n + MT_CHUNK - 1) / MT_CHUNK;
  }
  return chunks;
}

}  // namespace

extern "C" int msclip_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int step, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_adamw, stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step);
  if (!p || !g || !m || !v || n <= 0 || step < 1) return MSCLIP_EINVAL;
  const BiasCorrections bc = bias_corrections<false>(beta1, beta2, step);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for((size_t)n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (size_t)n,
                     lr, beta1, beta2, eps, weight_decay, bc.c1, bc.c2);
  return msclip_launch_status();
}

extern "C" int msclip_adamw_multi(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                                  void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_adamw_multi);
  return adamw_multi_launch(tensors, count, beta1, beta2, eps, step, nullptr, nullptr, stream);
}

extern "C" int msclip_adamw_multi_clipped(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps,
                                          int step, const float* coef_dev, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_adamw_multi_clipped);
  if (!coef_dev || ((size_t)coef_dev & 3)) return MSCLIP_EINVAL;
  return adamw_multi_launch(tensors, count, beta1, beta2, eps, step, coef_dev, nullptr, stream);
}

extern "C" int msclip_adamw_multi_guarded(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps,
                                          int step, const float* coef_dev, const int* skip_dev, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_adamw_multi_guarded);
  if (!skip_dev || (((size_t)skip_dev | (size_t)coef_dev) & 3)) return MSCLIP_EINVAL;
  return adamw_multi_launch(tensors, count, beta1, beta2, eps, step, coef_dev, skip_dev, stream);
}

extern "C" int msclip_grad_accumulate(const msclip_accum_tensor* tensors, int count, int mode, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_grad_accumulate);
  if (!tensors || count < 0 || mode < 0 || mode > 1) return MSCLIP_EINVAL;
  for (int i = 0; i < count; ++i)
    if (!tensors[i].acc || !tensors[i].g || tensors[i].n <= 0 || (((size_t)tensors[i].acc | (size_t)tensors[i].g) & 3))
      return MSCLIP_EINVAL;
  mt_for_each_launch<AccumBatch>(
      tensors, count,
      [](msclip_accum_tensor& t, long long k) {
        t.acc += k;
        t.g += k;
        t.n -= k;
      },
      [&](const AccumBatch& b, int nb, long long) {
        if (mode) hipLaunchKernelGGL(accumulate_kernel<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b);
        else hipLaunchKernelGGL(accumulate_kernel<0>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b);
      });
  return msclip_launch_status();
}

extern "C" int msclip_ext3_abi_version(void) { return MSCLIP_EXT3_ABI_VERSION; }

extern "C" int msclip_lamb_partials(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                                    const float* coef_dev, float* partials, long long n_partials, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_lamb_partials);
  const long long chunks = lamb_table_chunks(tensors, count, step, coef_dev);
  if (chunks < 0 || !partials || ((size_t)partials & 3)) return MSCLIP_EINVAL;
  if (n_partials != 2 * chunks) return MSCLIP_EINVAL;        // every slot the fold will read is written, none beyond the array
  const BiasCorrections bc = bias_corrections<true>(beta1, beta2, step);
  const auto kernel = pick_clip(coef_dev, lamb_partials_kernel<true>, lamb_partials_kernel<false>);
  mt_for_each_launch<LambBatch>(tensors, count, adam_advance<msclip_lamb_tensor>, [&](const LambBatch& b, int nb, long long first) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, bc.c1, bc.c2, coef_dev,
                       partials + 2 * first);
  });
  return msclip_launch_status();
}

extern "C" int msclip_lamb_apply(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                                 const float* coef_dev, const float* ratio_dev, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_lamb_apply);
  if (lamb_table_chunks(tensors, count, step, coef_dev) < 0 || !ratio_dev || ((size_t)ratio_dev & 3)) return MSCLIP_EINVAL;
  return lamb_apply_launch(tensors, count, beta1, beta2, eps, step, coef_dev, ratio_dev, nullptr, stream);
}

extern "C" int msclip_ext4_abi_version(void) { return MSCLIP_EXT4_ABI_VERSION; }

extern "C" int msclip_lamb_apply_guarded(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                                         const float* coef_dev, const float* ratio_dev, const int* skip_dev, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_lamb_apply_guarded);
  if (lamb_table_chunks(tensors, count, step, coef_dev) < 0 || !ratio_dev || !skip_dev || (((size_t)ratio_dev | (size_t)skip_dev) & 3))
    return MSCLIP_EINVAL;
  return lamb_apply_launch(tensors, count, beta1, beta2, eps, step, coef_dev, ratio_dev, skip_dev, stream);
}
