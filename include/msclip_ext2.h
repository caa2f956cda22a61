/* msclip_ext2.h -- the row-scale entry points of libmsclip_hip.so (stochastic depth, MODEL.SPEC.VISION.DROP_PATH), newer than
 * ABI version 9 of msclip_hip.h and than version 1 of msclip_ext.h.
 *
 * A second extension header, for the reason msclip_ext.h gives: msclip_hip.h (struct layouts included: msclip_gemm_desc keeps its
 * 280 bytes) and msclip_ext.h and everything that is pinned to them stay as they are; the declarations below are versioned on
 * their own (MSCLIP_EXT2_ABI_VERSION, msclip_ext2_abi_version) and bound as a third table (msclip_amd/hip.py: EXT2_EXPORTS).
 * The next ABI clean-up folds this file into msclip_hip.h -- row_scale then becomes the last member of msclip_gemm_desc and the
 * last argument of msclip_layernorm_bwd / msclip_cast_bf16_colsum -- and removes it.
 *
 * Conventions and declaration style: those of msclip_hip.h (msclip_amd/abi.py reads this text with the same rules; the struct
 * names of msclip_hip.h are known to it).
 *
 * What the scale is: timm's DropPath(p) in train() multiplies a residual branch's output by r / keep, r ~ Bernoulli(keep),
 * keep = 1 - p, one draw per index of dimension 0 of its input (M.py:801, 1027-1028: both branches of every vision
 * ResidualAttentionBlock).  The kernels see the result as one fp32 value per ROW of the launch, 0 or 1 / keep for an image row,
 * 1 for a text row; how the host fills the table (one draw per image, or per token position as the reference's sequence-first
 * layout makes timm do) is train.drop_path_table's business.
 */
#ifndef MSCLIP_EXT2_H
#define MSCLIP_EXT2_H

#include "msclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* msclip_gemm with a per-row scale on the branch in front of an fp32 residual add (out_proj / c_proj of a vision block, forward):
 *     out[row(m)][n] = resid[m][n] + row_scale[m] * (alpha * acc + bias[n]),
 * row_scale fp32 [M], indexed by the launch's row m BEFORE any row scatter (M = desc->M, the upper bound under M_dev).
 * Accepted: dense X (mode 0), resid_kind 1, fp32 output, act 0, on the dense ping-pong kernel ("pp": whole tiles and its guarded
 * edge tiles, M_dev included) and on the generic 128 x 128 / 256 x 192 kernels (vectorised and element-wise tail epilogues); a
 * descriptor for which msclip_gemm would pick the streaming kernel runs on the 128 x 128 kernel here (tile 0) or is rejected
 * (tile 5).  Everything else -- the LayerNorm fold's producer / consumer forms (xb, rowstat, W2), out2, bn_mode, part, the other
 * resid_kinds, bf16 output, an activation, implicit convolutions -- returns MSCLIP_EINVAL: the scale is never silently ignored.
 * (Split-K and fp8 launches have entry points of their own, which take no such argument.)  row_scale == NULL: msclip_gemm(desc).
 * A row with scale 1.0f is bitwise the row msclip_gemm writes, a row with scale 0.0f is bitwise resid (the branch value is not
 * read for it: a non-finite product does not leak into a dropped row).  The kernels of msclip_gemm itself are untouched: the
 * ping-pong kernel's row-scaled epilogue is an instantiation of its own. */
int msclip_gemm_rowscale(const msclip_gemm_desc* desc, const float* row_scale, void* stream);

/* msclip_layernorm_bwd whose bf16 copy and column sums carry a per-row scale: dxb[m] = bf16(row_scale[m] * dX_new[m]) and
 * sum_part sums the same scaled fp32 values; dx itself is written unscaled (the residual path).  In the training step the new
 * residual-stream gradient is the output gradient of the projection in front of this LayerNorm point; behind a DropPath that
 * projection's dgrad operand, weight gradient and bias gradient all see row_scale[m] * dX[m].  row_scale fp32 [M] needs dxb /
 * sum_part (MSCLIP_EINVAL without them); NULL: msclip_layernorm_bwd, bit for bit. */
int msclip_layernorm_bwd_rowscale(const float* x, int ldx, const int* row_idx, int row_mul, const void* dy, int lddy, int dy_is_f32,
                                  const float* gamma, float* dx, int lddx, int accumulate, float* part, int part_blocks, int M,
                                  int C, float eps, void* dxb, int lddxb, float* sum_part, int sum_accumulate,
                                  const float* row_scale, void* stream);

/* msclip_cast_bf16_colsum of row_scale[m] * x[src(m)]: y[m] = bf16(row_scale[m] * x row), part = the block sums of the same scaled
 * fp32 values; x is not written.  row_scale fp32 [M] is indexed by the OUTPUT row m (skip_group as in msclip_cast_bf16_colsum).
 * NULL: msclip_cast_bf16_colsum, bit for bit. */
int msclip_cast_bf16_colsum_rowscale(const float* x, int ldx, void* y, int ldy, int M, int C, float* part, int part_blocks,
                                     int skip_group, const float* row_scale, void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_EXT2_ABI_VERSION 1
int msclip_ext2_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
