/* msclip_metrics.h -- the ranking counts behind the zero-shot metrics 11point_mAP and roc_auc (msclip_amd/metrics.py,
 * msclip_amd/metrics_hip.py; the reference hands every logit to scikit-learn on the host, tools/zero_shot.py:136-147, 280-300).
 *
 * A header of its own, versioned on its own (MSCLIP_METRICS_ABI_VERSION, msclip_metrics_abi_version) and bound by a module of its
 * own (msclip_amd/metrics_hip.py, which opens the same libmsclip_hip.so): msclip_hip.h, the msclip_ext*.h headers, msclip_input.h,
 * msclip_color.h and the binding table of msclip_amd/hip.py stay as they are.
 *
 * Conventions and declaration style: those of msclip_hip.h (device pointers owned by the caller, ordered on `stream`, 0 = launched,
 * -1 = rejected arguments, -2 = HIP launch error; msclip_amd/abi.py reads this text with the same rules).  Every pointer is checked
 * for NULL (where it is not optional) and for 4-byte alignment (Y: bytes, any address) before anything is launched.
 *
 * THE COUNTS.  Scores S fp32 [N, lds], row = sample, column = class; labels Y uint8 [N, ldy], "not 0" = positive.  For every
 * column c < C and sample i < N, with x = S[i][c]:
 *     ge_pos[c][i] = #{ j : Y[j][c] != 0 and S[j][c] >= x }
 *     ge_neg[c][i] = #{ j : Y[j][c] == 0 and S[j][c] >= x }
 *     gt_neg[c][i] = #{ j : Y[j][c] == 0 and S[j][c] >  x }
 *     npos[c]      = #{ j : Y[j][c] != 0 },   nbad[c] = #{ j : S[j][c] is not a number }
 * The comparisons are IEEE's: a NaN compares false both ways (it counts nowhere and sees nothing; the host refuses a column whose
 * nbad is not 0, as scikit-learn refuses NaN), +0.0 == -0.0, denormals keep their value, +-Inf order like numbers.  Sample i is one
 * of the j: ge_pos + ge_neg >= 1 wherever x is a number.
 * These are the numbers of true and false positives at the threshold x (the precision-recall curve's point of sample i) and, for a
 * positive i, the negatives it beats (N - npos - ge_neg) and ties with (ge_neg - gt_neg): Mann-Whitney's statistic.  Ties are exact:
 * there is no sort and no rank to break. */
#ifndef MSCLIP_METRICS_H
#define MSCLIP_METRICS_H

#ifdef __cplusplus
extern "C" {
#endif

/* A workgroup owns MSCLIP_RANK_ROWS samples of one column (one thread each) and stages that column MSCLIP_RANK_STAGE samples at a
 * time in LDS: 2 x 4 bytes per staged sample, 8 KiB, beside 2 KiB for the fold of npos / nbad: 10 KiB per workgroup. */
#define MSCLIP_RANK_ROWS 256
#define MSCLIP_RANK_STAGE 1024
/* The comparisons of one call, N * N * C, at most 2^MSCLIP_RANK_LOG2_MAX_PAIRS (so N <= 2^21).  The Python binding
 * (msclip_amd/metrics_hip.py) is stricter: it cuts the class range so that one launch compares at most 2^40 pairs, cannot cut a
 * single column, and therefore stops at N = 2^20. */
#define MSCLIP_RANK_LOG2_MAX_PAIRS 42

/* The counts above, over columns [0, C) of S and Y.
 *   S       fp32 [N, lds]                        Y       uint8 [N, ldy]
 *   ge_pos, ge_neg, gt_neg    int32 [C, ldn]: entry [c][i]; columns [N, ldn) of a row are not touched.  gt_neg is optional (NULL: not
 *           stored)
 *   npos, nbad                int32 [C]
 * An all-pairs count: ceil(N / MSCLIP_RANK_ROWS) x C workgroups.  A workgroup writes the staged scores twice, as "the score where
 * the label is positive, NaN elsewhere" and the reverse, so that the inner loop is three compares and three adds per pair and every
 * thread reads the same LDS address (a broadcast: no bank conflicts).  The first workgroup of a column also counts npos and nbad
 * while it stages (an integer tree in LDS).  No atomics and no zero-fill pass: every output slot, npos[c] and nbad[c] is written by
 * exactly one thread -- bitwise repeatable.
 * A column view is a call of its own: S + c, Y + c, C = 1, the leading dimensions unchanged.
 * Rejected: S, Y, ge_pos, ge_neg, npos or nbad NULL; S, ge_pos, ge_neg, gt_neg, npos or nbad not 4-byte aligned; N < 1, C < 1,
 * lds < C, ldy < C, ldn < N; N * N * C > 2^42.
 * Device pointers only: recordable in a launch plan. */
int msclip_rank_counts(const float* S, int lds, const void* Y, int ldy, int N, int C, int* ge_pos, int* ge_neg, int* gt_neg,
                       int ldn, int* npos, int* nbad, void* stream);

/* Bumped whenever a declaration of this file changes; the binding refuses a library built from another version. */
#define MSCLIP_METRICS_ABI_VERSION 1
int msclip_metrics_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
