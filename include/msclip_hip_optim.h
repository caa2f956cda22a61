/* msclip_hip_optim.h -- optimizer-phase entry points of libmsclip_hip.so that came after msclip_hip.h (ABI 8) and
 * msclip_hip_train.h (version 1) were frozen: gradient clipping by the global L2 norm, fused into the AdamW launch.
 *
 * Same library, same conventions and the same declaration style as msclip_hip.h (msclip_amd/abi.py reads all three; this
 * file's version macro is MSCLIP_OPTIM_ABI_VERSION).  msclip_amd/hip.py binds these symbols into hip.OPTIM_EXPORTS.
 *
 * The three calls of a clipped step, in stream order (hip.AdamwPlan.run): msclip_grad_sumsq -> msclip_clip_coef ->
 * msclip_adamw_multi_clipped.  Semantics: torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2,
 * error_if_nonfinite=False) followed by the optimizer, except that no gradient is rewritten.
 */
#ifndef MSCLIP_HIP_OPTIM_H
#define MSCLIP_HIP_OPTIM_H

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor of msclip_grad_sumsq (host-side array): `n` fp32 elements at `g`, 4-byte aligned. */
typedef struct msclip_sumsq_tensor {
  const float* g;
  long long n;
} msclip_sumsq_tensor;

/* Sum of squares of `count` tensors in a handful of launches (32 K-element chunks, up to 36 tensors and 400 chunks per
 * launch, the tensor table travels in the kernel arguments as msclip_adamw_multi's does).  Chunk c of the list (tensors in
 * table order, a tensor's chunks in address order) writes ONE fp32 partial to partials[c]: the workgroup adds in a fixed
 * order (per-thread serial sums, wave64 shuffle tree, four waves through LDS), so the result is bitwise repeatable; no
 * atomics and no zero-fill pass, every slot is overwritten.  16-byte loads where the pointer allows, a scalar head and tail
 * otherwise.  n_partials must equal sum_i ceil(n_i / 32768).  `tensors` is a HOST array, read before the call returns (so a
 * plan recording that meets this call is marked unusable). */
int msclip_grad_sumsq(const msclip_sumsq_tensor* tensors, int count, float* partials, long long n_partials, void* stream);

/* out[0] = total_norm = sqrt(sum of the n partials), out[1] = coef = min(1, max_norm / (total_norm + 1e-6)), both fp32.  One
 * workgroup, the partials added in a fixed order in double.  NaN / Inf in a partial reaches both outputs the way it does in
 * torch (NaN -> NaN, NaN; Inf -> Inf, 0). */
int msclip_clip_coef(const float* partials, long long n, float max_norm, float* out, void* stream);

/* msclip_adamw_multi on g[i] * coef_dev[0]: the product is one IEEE fp32 multiply, rounded before the moment updates (the
 * value torch would have stored back into .grad); g itself is not written.  Everything else, the packed copies included,
 * is msclip_adamw_multi: with coef 1.0f the results are bitwise the same.  `tensors` is a HOST array of `count`
 * msclip_adamw_tensor (msclip_hip.h; declared void here because this header's reader resolves only the structs this header
 * declares), read before the call returns; coef_dev is a DEVICE pointer, read by the kernels. */
int msclip_adamw_multi_clipped(const void* tensors, int count, float beta1, float beta2, float eps, int step,
                               const float* coef_dev, void* stream);

#define MSCLIP_OPTIM_ABI_VERSION 1
int msclip_optim_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
