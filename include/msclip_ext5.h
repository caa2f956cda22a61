/* msclip_ext5.h -- linear probing (msclip_amd/linear_probe.py): the row pass of a softmax classifier's objective on frozen
 * features, the fold of its loss partials, and the one-pass bf16 hi/lo split of an fp32 matrix.  Newer than ABI version 9 of
 * msclip_hip.h and than version 1 of msclip_ext.h ... msclip_ext4.h.
 *
 * A fifth extension header, for the reason msclip_ext.h gives: the five older headers and everything that is pinned to them stay
 * as they are; the declarations below are versioned on their own (MSCLIP_EXT5_ABI_VERSION, msclip_ext5_abi_version) and bound
 * as a sixth table (msclip_amd/hip.py: EXT5_EXPORTS).
 *
 * Conventions and declaration style: those of msclip_hip.h (device pointers owned by the caller, ordered on `stream`, 0 = launched,
 * -1 = rejected arguments, -2 = HIP launch error; msclip_amd/abi.py reads this text with the same rules).  Every pointer is checked
 * for NULL (where it is not optional) and for 4-byte alignment (8-byte where it points to doubles) before anything is launched.
 *
 * The objective, for features X [N, E] fp32, labels y in [0, C) and parameters P = [W | b] of shape [C, E + 1] fp32:
 *     f(P) = (1/N) * sum_i ( logsumexp_c(x_i . W_c + b_c) - (x_i . W_{y_i} + b_{y_i}) )  +  (l2/2) * ||W||_F^2      (b is not penalised)
 * One evaluation, per chunk of R rows, in stream order (linear_probe.ProbeObjective.value_and_grad):
 *     msclip_gemm (S = X W^T, K = 3E split operands, fp32) -> msclip_probe_ce_rows -> msclip_gemm_splitk_tn x 2 (dW = G^T X)
 *     -> msclip_colsum (bias gradient);  msclip_probe_loss_fold once behind the last chunk. */
#ifndef MSCLIP_EXT5_H
#define MSCLIP_EXT5_H

#include "msclip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of a workgroup of msclip_probe_ce_rows: the call launches (R + 31) / 32 workgroups, and the partial arrays below hold one
 * entry (loss_part, bad_part) or one row (colsum_part) per workgroup. */
#define MSCLIP_PROBE_ROWS 32

/* The classifier's row pass over an fp32 logits block S [R, lds] = x . W (without the bias).  Row r, with v[c] = S[r][c] + bias[c]
 * for c < C (bias NULL: zero) and label l = labels[r]:
 *     lse[r]  = logsumexp_c v[c]                    max-subtracted, fp32 statistics; optional (NULL: not stored)
 *     G[r][c] = w * (exp(v[c] - lse) - [c == l])    fp32, stored as two bf16 matrices [R, ldg]: G_hi = bf16(G),
 *               G_lo = bf16(G - float(G_hi)); columns [C, Cpad) of both are written as zero -- GEMM operands as they stand
 *     pred[r] = argmax_c v[c], the lowest index on ties;  rank[r] = the number of c with v[c] > v[l] (top-k hit: rank < k)
 * Columns [C, Cpad) of S are never read as classes.  Per workgroup b (rows [32 b, 32 b + 32)):
 *     loss_part[b]      DOUBLE: sum over its rows of (lse - v[l]), each term fp32, added in double in a fixed order
 *     colsum_part[b][c] fp32 [.., ldp]: sum over its rows of the fp32 G[r][c] for c < Cpad (zero for c >= C): folded over b
 *                       (msclip_colsum) it is the bias gradient
 *     bad_part[b]       int: the number of its rows whose label was outside [0, C); such a label is clamped into the range before
 *                       anything is indexed with it.  Optional
 * Every slot of every output is written by exactly one thread: no atomics, no zero-fill pass in front, fixed addition order --
 * bitwise repeatable.  w is 1/N of the WHOLE set, not of the block.
 * Forms: G_hi == NULL (then G_lo, colsum_part must be NULL too): statistics only -- the predict-only form of held-out sets;
 * labels == NULL (then G_hi, loss_part, rank, bad_part must be NULL): pred / lse only.
 * Rules: R > 0, C >= 2, Cpad >= C, lds >= Cpad, ldg >= Cpad, ldp >= Cpad; loss_part 8-byte aligned.  Any C >= 2 runs on the scalar
 * path; 16-byte loads of S and 8-byte stores of G are used where S is 16-byte and G_hi, G_lo are 8-byte aligned and lds, ldg, Cpad
 * are multiples of 4.  Device pointers only: recordable in a launch plan. */
int msclip_probe_ce_rows(const float* S, int lds, const float* bias, const int* labels, int R, int C, int Cpad, float w,
                         float* lse, void* G_hi, void* G_lo, int ldg, void* loss_part, float* colsum_part, int ldp,
                         int* pred, int* rank, int* bad_part, void* stream);

/* out[0] (DOUBLE) = (sum_b loss_part[b]) / denom: one workgroup, thread t adds entries t, t + 256, ... in double, then a fixed
 * tree (msclip_clip_coef's fold).  n > 0, denom > 0; both pointers 8-byte aligned. */
int msclip_probe_loss_fold(const void* loss_part, long long n, long long denom, void* out, void* stream);

/* hi = bf16(x), lo = bf16(x - float(hi)) for an fp32 matrix x [M, ldx] in ONE pass, in the "hi | lo" layout of the training head's
 * split features: out is bf16 [M, ldo], out[m][c] = hi, out[m][C + c] = lo (c < C); columns past 2 C are not touched.
 * M > 0, C > 0, ldx >= C, ldo >= 2 C; 16-byte loads / 8-byte stores where x is 16-byte and out 8-byte aligned and C, ldx, ldo are
 * multiples of 4, element by element otherwise. */
int msclip_split_bf16(const float* x, int ldx, void* out, int ldo, long long M, int C, void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_EXT5_ABI_VERSION 1
int msclip_ext5_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
