// msclip_rank_counts' counting (msclip_amd/csrc/rank_body.h) built for the host: the same begin / stage / count / store, every
// workgroup in turn and its threads one after the other.  tests/test_metrics_cpu.py compiles this file with the host C++ compiler
// (-ffp-contract=off, no fast-math: the flags metrics.hip gets) into a shared object and compares it with the numpy restatement
// (tests/metrics_ref.py) exactly; the stand-alone program (-DMETRICS_HOST_MAIN) is for a sanitizer build: ragged shapes, NaN and
// +-Inf scores, label bytes 0 / 1 / 255, leading dimensions with slack, checked against a plain double loop.
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "../msclip_amd/csrc/rank_body.h"

// host pointers throughout; returns 0, or -1 for what msclip_rank_counts rejects
extern "C" int host_rank_counts(const float* S, int lds, const unsigned char* Y, int ldy, int N, int C, int* ge_pos, int* ge_neg,
                                int* gt_neg, int ldn, int* npos, int* nbad) {
  using namespace msclip_rank;
  if (!S || !Y || !ge_pos || !ge_neg || !npos || !nbad) return -1;
  if (((size_t)S | (size_t)ge_pos | (size_t)ge_neg | (size_t)gt_neg | (size_t)npos | (size_t)nbad) & 3) return -1;
  if (!shape_ok(lds, ldy, N, C, ldn)) return -1;
  Args a = {S, lds, Y, ldy, N, C, ge_pos, ge_neg, gt_neg, ldn, npos, nbad};
  std::vector<Quad> sp(STAGE / 4), sn(STAGE / 4);                   // exactly the device's allocation: a sanitizer sees an overrun
  std::vector<Lane> lane(ROWS);
  const int nblk = (N + ROWS - 1) / ROWS;
  for (int c = 0; c < C; ++c)
    for (int blk = 0; blk < nblk; ++blk) {
      for (int t = 0; t < ROWS; ++t) begin(a, c, (long long)blk * ROWS + t, &lane[t]);
      for (int j0 = 0; j0 < N; j0 += STAGE) {
        for (int t = 0; t < ROWS; ++t) stage(a, c, j0, sp.data(), sn.data(), t, ROWS, &lane[t]);
        const int left = N - j0;
        for (int t = 0; t < ROWS; ++t) count(sp.data(), sn.data(), left < STAGE ? left : STAGE, &lane[t]);
      }
      for (int t = 0; t < ROWS; ++t) store(a, c, (long long)blk * ROWS + t, lane[t]);
      if (blk == 0) {
        int p = 0, b = 0;
        for (int t = 0; t < ROWS; ++t) p += lane[t].npos, b += lane[t].nbad;
        npos[c] = p;
        nbad[c] = b;
      }
    }
  return 0;
}

extern "C" int host_rank_rows(void) { return msclip_rank::ROWS; }
extern "C" int host_rank_stage(void) { return msclip_rank::STAGE; }

#ifdef METRICS_HOST_MAIN
int main() {
  using namespace msclip_rank;
  unsigned long long sum = 0;
  unsigned seed = 9876u;
  auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (int)(seed >> 8); };
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const int SENT = -77;
  const int shapes[][2] = {{1, 1}, {2, 3}, {7, 2}, {ROWS - 1, 1}, {ROWS + 1, 3}, {STAGE - 1, 2}, {STAGE + 1, 1}, {2 * STAGE + 3, 2}};
  for (const auto& s : shapes)
    for (int with_gt = 0; with_gt < 2; ++with_gt) {
      const int N = s[0], C = s[1], lds = C + 3, ldy = C + 1, ldn = N + 5;
      // the matrices end with their last row's C entries: a read of the slack behind it is an overrun the sanitizer sees
      std::vector<float> S((size_t)(N - 1) * lds + C);
      std::vector<unsigned char> Y((size_t)(N - 1) * ldy + C);
      for (auto& v : S) {
        const int k = rnd() % 16;
        v = k == 0 ? nan : k == 1 ? inf : k == 2 ? -inf : k == 3 ? 0.f : k == 4 ? -0.f : (float)(rnd() % 9) * 0.25f - 1.f;
      }
      for (auto& v : Y) {
        const int k = rnd() % 4;
        v = k == 0 ? 1 : k == 1 ? 255 : 0;
      }
      std::vector<int> gp((size_t)C * ldn, SENT), gn((size_t)C * ldn, SENT), tn((size_t)C * ldn, SENT), np(C, SENT), nb(C, SENT);
      if (host_rank_counts(S.data(), lds, Y.data(), ldy, N, C, gp.data(), gn.data(), with_gt ? tn.data() : nullptr, ldn, np.data(),
                           nb.data()) != 0) {
        printf("rejected %d x %d\n", N, C);
        return 1;
      }
      for (int c = 0; c < C; ++c) {
        int p = 0, b = 0;
        for (int j = 0; j < N; ++j) p += Y[(size_t)j * ldy + c] != 0, b += S[(size_t)j * lds + c] != S[(size_t)j * lds + c];
        if (np[c] != p || nb[c] != b) return 2;
        for (int i = 0; i < ldn; ++i) {
          const size_t o = (size_t)c * ldn + i;
          if (i >= N) {
            if (gp[o] != SENT || gn[o] != SENT || tn[o] != SENT) return 3;          // the slack is not touched
            continue;
          }
          int a0 = 0, a1 = 0, a2 = 0;
          const float x = S[(size_t)i * lds + c];
          for (int j = 0; j < N; ++j) {
            const float v = S[(size_t)j * lds + c];
            const bool pos = Y[(size_t)j * ldy + c] != 0;
            a0 += pos && v >= x, a1 += !pos && v >= x, a2 += !pos && v > x;
          }
          if (gp[o] != a0 || gn[o] != a1 || tn[o] != (with_gt ? a2 : SENT)) return 4;
          sum = sum * 31 + (unsigned)(a0 + 3 * a1 + 7 * a2);
        }
      }
    }
  int one = 0;
  float f = 0.f;
  unsigned char y = 0;
  if (host_rank_counts(&f, 1, &y, 1, 0, 1, &one, &one, nullptr, 1, &one, &one) != -1) return 5;       // N = 0
  if (host_rank_counts(&f, 1, &y, 1, 1, 2, &one, &one, nullptr, 1, &one, &one) != -1) return 5;       // lds < C
  if (host_rank_counts(&f, 1 << 30, &y, 1 << 30, 1 << 21, 2, &one, &one, nullptr, 1 << 21, &one, &one) != -1) return 5;   // N N C
  printf("metrics_host: checksum %llu\n", sum);
  return 0;
}
#endif
