/* msclip_ext.h -- entry points of libmsclip_hip.so that are newer than ABI version 9 of msclip_hip.h.
 *
 * An extension header: msclip_hip.h and everything that is pinned to it stay as they are, the declarations below are versioned
 * on their own (MSCLIP_EXT_ABI_VERSION, msclip_ext_abi_version) and bound as a second table (msclip_amd/hip.py: EXT_EXPORTS).
 * This file is folded into msclip_hip.h by the next ABI clean-up, which bumps MSCLIP_ABI_VERSION and removes it.
 *
 * Conventions and declaration style: those of msclip_hip.h (device pointers owned by the caller, ordered on `stream`, 0 = launched,
 * -1 = rejected arguments, -2 = HIP launch error; msclip_amd/abi.py reads this text with the same rules).
 */
#ifndef MSCLIP_EXT_H
#define MSCLIP_EXT_H

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor of msclip_ema_multi (host-side array): `n` fp32 elements of a parameter `p` and of its shadow `ema`.  Neither
 * pointer needs more than 4-byte alignment.  The ranges of one call must not overlap (a shadow with a parameter, or two
 * shadows): that is the caller's error, it is not checked. */
typedef struct msclip_ema_tensor {
  float* ema;
  const float* p;
  long long n;
} msclip_ema_tensor;

/* Exponential moving average of the weights (TRAIN.EMA_DECAY), all `count` tensors in a handful of launches (32 K-element
 * pieces of up to 36 tensors per launch, the tensor table travels in the kernel arguments as msclip_grad_accumulate's does):
 * ema[i] = fl(fl(decay * ema[i]) + fl(one_minus_decay * p[i])), three separately rounded IEEE fp32 operations, no fused
 * multiply-add -- bitwise `decay * ema + (1. - decay) * p` on fp32 torch tensors when the caller passes one_minus_decay =
 * (float)(1.0 - (double)decay).  p is not written.  12 B per element.  16-byte accesses where ema and p share their offset
 * within 16 bytes (scalar head and tail around them), 4-byte accesses otherwise.  decay and one_minus_decay each in [0, 1].
 * `tensors` is a HOST array, read before the call returns (so a plan recording that meets this call is marked unusable). */
int msclip_ema_multi(const msclip_ema_tensor* tensors, int count, float decay, float one_minus_decay, void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_EXT_ABI_VERSION 1
int msclip_ext_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
