/* msclip_ext3.h -- the LAMB entry points of libmsclip_hip.so (TRAIN.OPTIMIZER lamb: a trust ratio per parameter tensor),
 * newer than ABI version 9 of msclip_hip.h and than version 1 of msclip_ext.h and msclip_ext2.h.
 *
 * A third extension header, for the reason msclip_ext.h gives: msclip_hip.h, msclip_ext.h, msclip_ext2.h and everything that is
 * pinned to them stay as they are; the declarations below are versioned on their own (MSCLIP_EXT3_ABI_VERSION,
 * msclip_ext3_abi_version) and bound as a fourth table (msclip_amd/hip.py: EXT3_EXPORTS).  The next ABI clean-up folds this
 * file into msclip_hip.h and removes it.
 *
 * Conventions and declaration style: those of msclip_hip.h (device pointers owned by the caller, ordered on `stream`, 0 = launched,
 * -1 = rejected arguments, -2 = HIP launch error; msclip_amd/abi.py reads this text with the same rules).
 *
 * The update (timm's Lamb with grad_averaging and bias_correction; INTEGRATION.md states the two deviations).  For a parameter
 * tensor w with gradient g, moments m, v, step t >= 1 and its group's lr, wd:
 *     g' = g * coef                                             (coef = coef_dev[0]; 1 when coef_dev is NULL)
 *     m  = b1 * m + (1 - b1) * g',   v = b2 * v + (1 - b2) * g' * g'
 *     u  = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd * w
 *     r  = ||w|| / ||u||  if ||w|| > 0 and ||u|| > 0, else 1    (a NaN norm fails both comparisons: r = 1; ||u|| = inf: r = 0)
 *     r  = min(r, 1)      if trust_clip
 *     w  = w - lr * (adapt ? r : 1) * u
 * with the L2 norms over the whole parameter.  The three calls of a step, in stream order (hip.LambPlan.run):
 * msclip_lamb_partials -> msclip_lamb_ratios -> msclip_lamb_apply, behind msclip_grad_sumsq -> msclip_clip_coef when the step
 * clips.  m, v and w are written by the last call only: the first forms the new moments and u in registers and keeps their
 * squares' sums, 16 B read per element; the last is the AdamW launch (28 B per element) with the rate scaled. */
#ifndef MSCLIP_EXT3_H
#define MSCLIP_EXT3_H

#include "msclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One item of msclip_lamb_partials / msclip_lamb_apply (host-side array): the members of msclip_adamw_tensor with their
 * meaning there, then the parameter the item belongs to.  A parameter whose packed copies differ between its parts (the q rows
 * of in_proj_weight carry a scale) is several ADJACENT items with one `param`; `param` starts at 0 and grows by 0 or 1 from
 * one item to the next.  adapt: 0 = the item takes a plain Adam step (rate lr, the ratio is not read); otherwise lr * ratio. */
typedef struct msclip_lamb_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
  float lr;
  float weight_decay;
  void* pk;
  float pk_scale;
  int pk_f32;
  int param;
  int adapt;
} msclip_lamb_tensor;

/* The squared norms, in partial sums: chunk c of the list (items in table order, 32 K-element chunks of an item in address
 * order; up to 32 items and 400 chunks per launch, the table travels in the kernel arguments) writes TWO fp32 values,
 * partials[2 c] = sum of p^2 and partials[2 c + 1] = sum of u^2 over the chunk, u formed from the NEW moments as above; p, g,
 * m, v are read and nothing else is written.  Addition order: msclip_grad_sumsq's (four accumulators of <= 32 fmaf per thread,
 * folded pairwise; wave64 shuffle tree; four waves through LDS), fixed, no atomics, no zero-fill pass: bitwise repeatable.
 * 16-byte loads where p, g, m and v are all 16-byte aligned, 4-byte loads otherwise.  n_partials must equal
 * 2 * sum_i ceil(n_i / 32768).  coef_dev: NULL, or the DEVICE address of the clipping coefficient (msclip_clip_coef's out + 1).
 * `tensors` is a HOST array, read before the call returns (so a plan recording that meets this call is marked unusable). */
int msclip_lamb_partials(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                         const float* coef_dev, float* partials, long long n_partials, void* stream);

/* One workgroup per parameter k < n_params: adds the partials of chunks first_chunk_dev[k] .. first_chunk_dev[k + 1] (a DEVICE
 * array of n_params + 1 non-decreasing ints, the chunk index of each parameter's first item and the chunk count at the end;
 * bounds outside [0, n_chunks] are clamped to it) in double, in a fixed order, and writes fp32
 *     out[k] = r,   out[n_params + k] = ||w||,   out[2 n_params + k] = ||u||
 * with r by the rule above from the two fp32 norms (before `adapt`, which msclip_lamb_apply looks at); trust_clip != 0 caps r at
 * 1.  Device pointers only: recordable in a launch plan. */
int msclip_lamb_ratios(const float* partials, const int* first_chunk_dev, int n_params, long long n_chunks, int trust_clip,
                       float* out, void* stream);

/* msclip_adamw_multi (msclip_adamw_multi_clipped when coef_dev is not NULL) with each item's rate replaced by
 * lr_eff = adapt ? lr * ratio_dev[param] : lr -- one IEEE fp32 multiply, rounded before it meets the update.  Everything else,
 * the packed copies and the 16-byte / 4-byte access rule included, is that call: handed lr_eff as the rate it writes bitwise
 * the same p, m, v and packed values.  ratio_dev: DEVICE array with an entry for every `param` of the table (msclip_lamb_ratios'
 * out).  `tensors` is a HOST array, read before the call returns. */
int msclip_lamb_apply(const msclip_lamb_tensor* tensors, int count, float beta1, float beta2, float eps, int step,
                      const float* coef_dev, const float* ratio_dev, void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_EXT3_ABI_VERSION 1
int msclip_ext3_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
