/* msclip_ext4.h -- the non-finite guard of the optimizer phase (TrainStep(nonfinite="skip" | "raise")): a verdict on the
 * gradient's partial sums of squares, taken on the device, and the two update calls that honour it.  Newer than ABI version 9
 * of msclip_hip.h and than version 1 of msclip_ext.h, msclip_ext2.h and msclip_ext3.h.
 *
 * A fourth extension header, for the reason msclip_ext.h gives: the four older headers and everything that is pinned to them
 * stay as they are; the declarations below are versioned on their own (MSCLIP_EXT4_ABI_VERSION, msclip_ext4_abi_version) and
 * bound as a fifth table (msclip_amd/hip.py: EXT4_EXPORTS).
 *
 * Conventions and declaration style: those of msclip_hip.h (device pointers owned by the caller, ordered on `stream`, 0 = launched,
 * -1 = rejected arguments, -2 = HIP launch error; msclip_amd/abi.py reads this text with the same rules).
 *
 * The calls of a guarded step, in stream order (hip.AdamwPlan.run / hip.LambPlan.run with guard=True):
 *     msclip_grad_sumsq -> msclip_clip_coef_guarded -> msclip_adamw_multi_guarded
 *     msclip_grad_sumsq -> msclip_clip_coef_guarded -> msclip_lamb_partials -> msclip_lamb_ratios -> msclip_lamb_apply_guarded
 * Nothing is read back: the verdict stays in device memory, and a step whose gradient holds a NaN or an Inf writes no
 * parameter, no moment and no packed copy.  msclip_lamb_partials and msclip_lamb_ratios write only their own scratch; on a skipped
 * step its values mean nothing. */
#ifndef MSCLIP_EXT4_H
#define MSCLIP_EXT4_H

#include "msclip_hip.h"
#include "msclip_ext3.h"

#ifdef __cplusplus
extern "C" {
#endif

/* msclip_clip_coef with a verdict: out = {total_norm, coef} bit for bit as msclip_clip_coef writes them for the same
 * partials, n and max_norm (one workgroup, the same fold in double), and the DEVICE array state[0..4) of ints:
 *     state[0] = skip:   1 if any of the n partials is NaN, +Inf or -Inf, else 0
 *     state[1] += skip:  the running count of skipped steps; the caller zeroes it once, this call never does.  Read and written
 *                        in stream order by the one workgroup: no atomics, and calls on ONE stream count exactly
 *     state[2] = the smallest index of a non-finite partial, or -1
 *     state[3] = the number of non-finite partials
 * A partial is non-finite where the exponent field of its bit pattern is all ones.  An element of a gradient that is NaN or Inf
 * makes its chunk's partial NaN or Inf (msclip_grad_sumsq squares and adds, compiled without fast-math), so skip = 1 exactly when
 * some element read by msclip_grad_sumsq was non-finite or a chunk's sum of squares overflowed fp32.  With skip = 1, out[0] is
 * NaN or Inf.  state: not NULL, 4-byte aligned; the other arguments as msclip_clip_coef's (max_norm 0: the norm alone).
 * Device pointers only: recordable in a launch plan. */
int msclip_clip_coef_guarded(const float* partials, long long n, float max_norm, float* out, int* state, void* stream);

/* msclip_adamw_multi (msclip_adamw_multi_clipped when coef_dev is not NULL) under the verdict: every workgroup of every launch
 * of the call reads skip_dev[0] (msclip_clip_coef_guarded's state) once and returns where it is not 0 -- then no p, m, v and no
 * packed copy is written.  With skip_dev[0] == 0 the result is bit for bit the unguarded call's.  skip_dev: not NULL, 4-byte
 * aligned; coef_dev: NULL or 4-byte aligned.  `step` is the number of APPLIED updates this one would be (the caller's count of
 * calls minus the skipped ones), >= 1.  `tensors` is a HOST array, read before the call returns. */
int msclip_adamw_multi_guarded(const msclip_adamw_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                               const float* coef_dev, const int* skip_dev, void* stream);

/* msclip_lamb_apply under the verdict, in the same way. */
int msclip_lamb_apply_guarded(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                              const float* coef_dev, const float* ratio_dev, const int* skip_dev, void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_EXT4_ABI_VERSION 1
int msclip_ext4_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
