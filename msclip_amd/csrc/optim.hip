// The optimizer phase of the training step: AdamW over all parameter tensors and gradient accumulation over the chunks of
// TrainStep.accumulate (train.py), each over its 325-406 tensors in a handful of launches (multi_tensor.h).  Streaming, bound
// by HBM.  The sum of squares and the coefficient of gradient clipping are in clip.hip, which is compiled without fast-math.
#include "common.h"
#include "multi_tensor.h"
#include "plan.h"
#include "../../include/msclip_hip.h"
#include "../../include/msclip_ext3.h"

namespace {

// ---- AdamW (decoupled weight decay), one fused pass per parameter tensor; fp32 states.  One statement of the update with
// the contractions written out, shared by both kernels: their results are bitwise the same.
__device__ __forceinline__ void adamw_update(float gi, float& mi, float& vi, float& pi, float lr, float b1, float b2, float eps,
                                             float wd, float c1, float c2) {
  mi = __fmaf_rn(b1, mi, (1.f - b1) * gi);
  vi = __fmaf_rn(b2, vi, (1.f - b2) * gi * gi);
  const float upd = __fmaf_rn(wd, pi, mi * c1 / (sqrtf(vi * c2) + eps));
  pi = __fmaf_rn(-lr, upd, pi);
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

// CLIP (msclip_adamw_multi_clipped): the update sees g[i] * coef[0], the clipping coefficient that msclip_clip_coef left on
// the device.  The product is ONE fp32 multiply, rounded before the moment updates -- the value torch's clip_grad_norm_ stores
// back into .grad: the empty asm keeps this file's fast-math from re-associating (1 - b1) * (g * coef) into
// ((1 - b1) * coef) * g.  CLIP = false: coef is not read.
template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const AdamwBatch a, float b1, float b2, float eps, float c1, float c2,
                                                          const float* __restrict__ coef_dev) {
  float coef = 1.f;
  if constexpr (CLIP) coef = *coef_dev;
  MT_DECODE_CHUNK(a, t, lo, cnt);
  float* __restrict__ p = t.p + lo;
  const float* __restrict__ g = t.g + lo;
  float* __restrict__ m = t.m + lo;
  float* __restrict__ v = t.v + lo;
  const float lr = t.lr, wd = t.weight_decay;
  auto upd = [&](float gi, float& mi, float& vi, float& pi) {
    if constexpr (CLIP) {
      gi *= coef;
      asm volatile("" : "+v"(gi));
    }
    adamw_update(gi, mi, vi, pi, lr, b1, b2, eps, wd, c1, c2);
  };
  // packed copy of the new values (the engine's GEMM operand): same rounding as a cast of the updated tensor
  bf16_t* __restrict__ pkb = t.pk && !t.pk_f32 ? (bf16_t*)t.pk + lo : nullptr;
  float* __restrict__ pkf = t.pk && t.pk_f32 ? (float*)t.pk + lo : nullptr;
  const float ps = t.pk_scale;
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
// them per parameter, lamb_apply_kernel is adamw_multi_kernel with the rate scaled (28 B per element).  The kernels above
// are not touched: these are kernels of their own on a table of their own.  32 x 72 B + 400 x 4 B of kernel arguments.
using LambBatch = MtBatch<msclip_lamb_tensor, 32, 400>;

// u of adamw_update, the same statements on the same values: the moments are not stored by this pass
__device__ __forceinline__ float lamb_direction(float gi, float mi, float vi, float pi, float b1, float b2, float eps, float wd,
                                                float c1, float c2) {
  mi = __fmaf_rn(b1, mi, (1.f - b1) * gi);
  vi = __fmaf_rn(b2, vi, (1.f - b2) * gi * gi);
  return __fmaf_rn(wd, pi, mi * c1 / (sqrtf(vi * c2) + eps));
}

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
  auto dir = [&](float gi, float mi, float vi, float pi) {
    if constexpr (CLIP) {
      gi *= coef;
      asm volatile("" : "+v"(gi));
    }
    return lamb_direction(gi, mi, vi, pi, b1, b2, eps, wd, c1, c2);
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
template <bool CLIP>
__global__ __launch_bounds__(256) void lamb_apply_kernel(const LambBatch a, float b1, float b2, float eps, float c1, float c2,
                                                         const float* __restrict__ coef_dev, const float* __restrict__ ratio_dev) {
  float coef = 1.f;
  if constexpr (CLIP) coef = *coef_dev;
  MT_DECODE_CHUNK(a, t, lo, cnt);
  float* __restrict__ p = t.p + lo;
  const float* __restrict__ g = t.g + lo;
  float* __restrict__ m = t.m + lo;
  float* __restrict__ v = t.v + lo;
  float lr = t.lr;
  if (t.adapt) {
    lr *= ratio_dev[t.param];
    asm volatile("" : "+v"(lr));
  }
  const float wd = t.weight_decay;
  auto upd = [&](float gi, float& mi, float& vi, float& pi) {
    if constexpr (CLIP) {
      gi *= coef;
      asm volatile("" : "+v"(gi));
    }
    adamw_update(gi, mi, vi, pi, lr, b1, b2, eps, wd, c1, c2);
  };
  bf16_t* __restrict__ pkb = t.pk && !t.pk_f32 ? (bf16_t*)t.pk + lo : nullptr;
  float* __restrict__ pkf = t.pk && t.pk_f32 ? (float*)t.pk + lo : nullptr;
  const float ps = t.pk_scale;
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

}  // namespace

extern "C" int msclip_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int step, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_adamw, stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step);
  if (!p || !g || !m || !v || n <= 0 || step < 1) return MSCLIP_EINVAL;
  const float c1 = 1.f / (1.f - powf(beta1, (float)step)), c2 = 1.f / (1.f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for((size_t)n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (size_t)n,
                     lr, beta1, beta2, eps, weight_decay, c1, c2);
  return msclip_launch_status();
}

template <bool CLIP>
static int adamw_multi_launch(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                              const float* coef_dev, void* stream) {
  if (!tensors || count < 0 || step < 1) return MSCLIP_EINVAL;
  for (int i = 0; i < count; ++i)
    if (!tensors[i].p || !tensors[i].g || !tensors[i].m || !tensors[i].v || tensors[i].n <= 0 ||
        (tensors[i].pk && (tensors[i].pk_f32 < 0 || tensors[i].pk_f32 > 1)))
      return MSCLIP_EINVAL;
  const float c1 = 1.f / (1.f - powf(beta1, (float)step)), c2 = 1.f / (1.f - powf(beta2, (float)step));
  mt_for_each_launch<AdamwBatch>(
      tensors, count,
      [](msclip_adamw_tensor& t, long long k) {
        t.p += k;
        t.g += k;
        t.m += k;
        t.v += k;
        t.n -= k;
        if (t.pk) t.pk = (char*)t.pk + (size_t)k * (t.pk_f32 ? 4 : 2);
      },
      [&](const AdamwBatch& b, int nb, long long) {
        hipLaunchKernelGGL(adamw_multi_kernel<CLIP>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, c1, c2,
                           coef_dev);
      });
  return msclip_launch_status();
}

extern "C" int msclip_adamw_multi(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                                  void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_adamw_multi);
  return adamw_multi_launch<false>(tensors, count, beta1, beta2, eps, step, nullptr, stream);
}

extern "C" int msclip_adamw_multi_clipped(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps,
                                          int step, const float* coef_dev, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_adamw_multi_clipped);
  if (!coef_dev || ((size_t)coef_dev & 3)) return MSCLIP_EINVAL;
  return adamw_multi_launch<true>(tensors, count, beta1, beta2, eps, step, coef_dev, stream);
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

// ---- LAMB
static void lamb_advance(msclip_lamb_tensor& t, long long k) {
  t.p += k;
  t.g += k;
  t.m += k;
  t.v += k;
  t.n -= k;
  if (t.pk) t.pk = (char*)t.pk + (size_t)k * (t.pk_f32 ? 4 : 2);
}

// -> the chunk count of the table, or -1 for a table that no kernel may see
static long long lamb_table_chunks(const msclip_lamb_tensor* tensors, int count, int step, const float* coef_dev) {
  if (!tensors || count < 0 || step < 1 || ((size_t)coef_dev & 3)) return -1;
  long long chunks = 0;
  for (int i = 0; i < count; ++i) {
    const msclip_lamb_tensor& t = tensors[i];
    if (!t.p || !t.g || !t.m || !t.v || t.n <= 0 || (t.pk && (t.pk_f32 < 0 || t.pk_f32 > 1))) return -1;
    if (((size_t)t.p | (size_t)t.g | (size_t)t.m | (size_t)t.v) & 3) return -1;
    const int prev = i ? tensors[i - 1].param : -1;          // 0, then the same parameter or the next one
    if (t.param != prev && t.param != prev + 1) return -1;
    if (i == 0 && t.param != 0) return -1;
    chunks += (t.n + MT_CHUNK - 1) / MT_CHUNK;
  }
  return chunks;
}

extern "C" int msclip_ext3_abi_version(void) { return MSCLIP_EXT3_ABI_VERSION; }

extern "C" int msclip_lamb_partials(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                                    const float* coef_dev, float* partials, long long n_partials, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_lamb_partials);
  const long long chunks = lamb_table_chunks(tensors, count, step, coef_dev);
  if (chunks < 0 || !partials || ((size_t)partials & 3)) return MSCLIP_EINVAL;
  if (n_partials != 2 * chunks) return MSCLIP_EINVAL;        // every slot the fold will read is written, none beyond the array
  const float c1 = 1.f / (1.f - powf(beta1, (float)step)), c2 = 1.f / (1.f - powf(beta2, (float)step));
  mt_for_each_launch<LambBatch>(tensors, count, lamb_advance, [&](const LambBatch& b, int nb, long long first_chunk) {
    if (coef_dev)
      hipLaunchKernelGGL(lamb_partials_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, c1, c2,
                         coef_dev, partials + 2 * first_chunk);
    else
      hipLaunchKernelGGL(lamb_partials_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, c1, c2,
                         coef_dev, partials + 2 * first_chunk);
  });
  return msclip_launch_status();
}

extern "C" int msclip_lamb_apply(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                                 const float* coef_dev, const float* ratio_dev, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_lamb_apply);
  if (lamb_table_chunks(tensors, count, step, coef_dev) < 0 || !ratio_dev || ((size_t)ratio_dev & 3)) return MSCLIP_EINVAL;
  const float c1 = 1.f / (1.f - powf(beta1, (float)step)), c2 = 1.f / (1.f - powf(beta2, (float)step));
  mt_for_each_launch<LambBatch>(tensors, count, lamb_advance, [&](const LambBatch& b, int nb, long long) {
    if (coef_dev)
      hipLaunchKernelGGL(lamb_apply_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, c1, c2,
                         coef_dev, ratio_dev);
    else
      hipLaunchKernelGGL(lamb_apply_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b, beta1, beta2, eps, c1, c2,
                         coef_dev, ratio_dev);
  });
  return msclip_launch_status();
}
