/* msclip_hip_train.h -- training-only entry points of libmsclip_hip.so that came after msclip_hip.h was frozen at ABI 8.
 *
 * Same library, same conventions and the same declaration style as msclip_hip.h (msclip_amd/abi.py reads both; this file's
 * version macro is MSCLIP_TRAIN_ABI_VERSION).  msclip_amd/hip.py binds these symbols into hip.TRAIN_EXPORTS.
 */
#ifndef MSCLIP_HIP_TRAIN_H
#define MSCLIP_HIP_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor of msclip_grad_accumulate (host-side array): `n` fp32 elements of a fresh gradient `g` and of its persistent
 * accumulator `acc`.  Neither pointer needs more than 4-byte alignment; the two ranges must not overlap. */
typedef struct msclip_accum_tensor {
  float* acc;
  const float* g;
  long long n;
} msclip_accum_tensor;

/* Gradient accumulation over the chunks of TrainStep.accumulate, all `count` tensors in a handful of launches (32 K-element
 * pieces of up to 36 tensors per launch, the tensor table travels in the kernel arguments as msclip_adamw_multi's does).
 * mode 0: acc[i] = g[i] (the first chunk: no zero-fill pass); mode 1: acc[i] = acc[i] + g[i], one IEEE fp32 add per element
 * in call order: bitwise torch's acc + g, bitwise repeatable (no atomics).  16-byte accesses wherever acc and g share their
 * offset within 16 bytes (scalar head and tail around them), 4-byte accesses otherwise.  `tensors` is a HOST array, read
 * before the call returns (so a plan recording that meets this call is marked unusable). */
int msclip_grad_accumulate(const msclip_accum_tensor* tensors, int count, int mode, void* stream);

#define MSCLIP_TRAIN_ABI_VERSION 1
int msclip_train_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
