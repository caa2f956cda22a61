// The ranking counts of the zero-shot metrics (include/msclip_metrics.h, msclip_amd/metrics_hip.py): for every sample and column,
// how many positives and negatives score at least as high, in one launch and without a sort.
//
// rank_counts_kernel: one workgroup of four waves owns MSCLIP_RANK_ROWS samples of one column, a thread per sample with its score in
// a register.  The column passes through LDS MSCLIP_RANK_STAGE samples at a time, written twice: the score where the label is
// positive and NaN elsewhere, and the reverse -- a NaN compares false, so the label costs the inner loop nothing: three compares and
// three adds per pair.  Every thread reads the same LDS address (16 bytes at a time: a broadcast, no bank conflicts), so the loop
// is bound by the vector ALU; the staging loads (one column of a row-major matrix: a cache line per sample, served by L2 after the
// first workgroup) are 4 per thread against 6 144 ALU operations, and 10 KiB of LDS (two staged arrays of 4 KiB, 2 KiB for the fold of the totals)
// leaves the CU full of workgroups to hide them.
// The first workgroup of a column folds the threads' shares of npos and nbad by a fixed tree (integers: any order gives the same
// sum) and thread 0 writes them.  No atomics, nothing to zero.
// The counting is rank_body.h, which a host program compiles too.  build.sh compiles this file without fast-math and with
// -ffp-contract=off (probe.hip's and color.hip's flags): the comparisons must see NaN, +-0 and denormals as IEEE does.
#include "common.h"
#include "plan.h"
#include "rank_body.h"
#include "../../include/msclip_hip.h"
#include "../../include/msclip_metrics.h"

static_assert(msclip_rank::ROWS == MSCLIP_RANK_ROWS && msclip_rank::STAGE == MSCLIP_RANK_STAGE &&
              msclip_rank::LOG2_MAX_PAIRS == MSCLIP_RANK_LOG2_MAX_PAIRS, "msclip_metrics.h");
static_assert(msclip_rank::STAGE % msclip_rank::ROWS == 0 && msclip_rank::STAGE % 4 == 0 &&
              (msclip_rank::ROWS & (msclip_rank::ROWS - 1)) == 0, "rank_body.h");

namespace {

__global__ __launch_bounds__(msclip_rank::ROWS) void rank_counts_kernel(msclip_rank::Args a, int c0, int nblk) {
  __shared__ msclip_rank::Quad sp[msclip_rank::STAGE / 4];
  __shared__ msclip_rank::Quad sn[msclip_rank::STAGE / 4];
  __shared__ int red[2 * msclip_rank::ROWS];
  const int col = (int)(blockIdx.x / (unsigned)nblk), blk = (int)(blockIdx.x - (unsigned)col * (unsigned)nblk), c = c0 + col;
  const int tid = threadIdx.x;
  const long long i = (long long)blk * msclip_rank::ROWS + tid;
  msclip_rank::Lane l;
  msclip_rank::begin(a, c, i, &l);
  for (int j0 = 0; j0 < a.N; j0 += msclip_rank::STAGE) {
    if (j0) __syncthreads();                       // everybody is done with the previous stage
    msclip_rank::stage(a, c, j0, sp, sn, tid, msclip_rank::ROWS, &l);
    __syncthreads();
    const int left = a.N - j0;
    msclip_rank::count(sp, sn, left < msclip_rank::STAGE ? left : msclip_rank::STAGE, &l);
  }
  msclip_rank::store(a, c, i, l);
  if (blk != 0) return;                            // (uniform over the workgroup)
  red[tid] = l.npos;
  red[msclip_rank::ROWS + tid] = l.nbad;
  __syncthreads();
  for (int s = msclip_rank::ROWS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red[msclip_rank::ROWS + tid] += red[msclip_rank::ROWS + tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.npos[c] = red[0];
    a.nbad[c] = red[msclip_rank::ROWS];
  }
}

}  // namespace

extern "C" int msclip_rank_counts(const float* S, int lds, const void* Y, int ldy, int N, int C, int* ge_pos, int* ge_neg,
                                  int* gt_neg, int ldn, int* npos, int* nbad, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_rank_counts, stream, S, lds, Y, ldy, N, C, ge_pos, ge_neg, gt_neg, ldn, npos, nbad);
  if (!S || !Y || !ge_pos || !ge_neg || !npos || !nbad) return MSCLIP_EINVAL;
  if (((size_t)S | (size_t)ge_pos | (size_t)ge_neg | (size_t)gt_neg | (size_t)npos | (size_t)nbad) & 3) return MSCLIP_EINVAL;
  if (!msclip_rank::shape_ok(lds, ldy, N, C, ldn)) return MSCLIP_EINVAL;
  msclip_rank::Args a;
  a.S = S;
  a.lds = lds;
  a.Y = (const unsigned char*)Y;
  a.ldy = ldy;
  a.N = N;
  a.C = C;
  a.ge_pos = ge_pos;
  a.ge_neg = ge_neg;
  a.gt_neg = gt_neg;
  a.ldn = ldn;
  a.npos = npos;
  a.nbad = nbad;
  const int nblk = (N + msclip_rank::ROWS - 1) / msclip_rank::ROWS;          // <= 2^13: shape_ok caps N at 2^21
  const int per = 0x7fffffff / nblk;                                         // columns of one grid
  for (int c0 = 0; c0 < C; c0 += per) {
    const int cols = C - c0 < per ? C - c0 : per;
    hipLaunchKernelGGL(rank_counts_kernel, dim3((unsigned)cols * (unsigned)nblk), dim3(msclip_rank::ROWS), 0, (hipStream_t)stream,
                       a, c0, nblk);
  }
  return msclip_launch_status();
}

extern "C" int msclip_metrics_abi_version(void) { return MSCLIP_METRICS_ABI_VERSION; }
