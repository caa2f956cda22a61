// msclip_color_augment's kernel body (msclip_amd/csrc/color_body.h) built for the host: the same mean pass and the same three band
// phases, every workgroup in turn, one "thread" each.  tests/test_color_cpu.py compiles this file with the host C++ compiler
// (-ffp-contract=off, no fast-math: the flags color.hip gets) into a shared object and compares it with the numpy restatement
// (tests/color_ref.py) bitwise; the stand-alone program (-DCOLOR_HOST_MAIN) is for a sanitizer build: it runs ragged shapes with
// hostile ops / coef (NaN factors, order entries and shifts out of range) and prints a checksum.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "../msclip_amd/csrc/color_body.h"

// host pointers throughout; returns 0, or -1 for what msclip_color_augment rejects
extern "C" int host_color_augment(const unsigned char* src, const int* ops, const float* coef, const float* lut, int B, int H, int W,
                                  int stages, int* work, void* out, int out_bf16, unsigned char* out_u8) {
  msclip_color::Plan p;
  if (!src || !ops || !coef || !lut || !out || B <= 0 || stages < 0 || stages > 7) return -1;
  if (((stages & 1) && !work) || out_u8 == src) return -1;
  if (!msclip_color::make_plan(H, W, &p)) return -1;
  msclip_color::Args a = {src, ops, coef, lut, B, H, W, stages, work, out, out_bf16, out_u8, p.band};
  std::vector<uint32_t> lds((size_t)p.lds_bytes / 4);          // exactly the device's allocation: a sanitizer sees an overrun
  for (int b = 0; b < B; ++b) {
    msclip_color::Rec rec;
    msclip_color::read_rec(a, b, &rec);
    if (stages & 1) work[b] = msclip_color::mean_of(msclip_color::partial_sum(a, b, rec, 0, 1), H, W);
    const int m = (stages & 1) ? work[b] : 0;
    for (int band0 = 0; band0 < H; band0 += p.band)
      for (int ph = 0; ph < 3; ++ph) msclip_color::phase(a, b, band0, rec, m, (stages & 4) ? lds.data() : nullptr, 0, 1, ph);
  }
  return 0;
}

extern "C" int host_color_augment_band(int H, int W) {
  msclip_color::Plan p;
  return msclip_color::make_plan(H, W, &p) ? p.band : -1;
}

#ifdef COLOR_HOST_MAIN
int main() {
  unsigned long long sum = 0;
  unsigned seed = 4321u;
  auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (int)(seed >> 8); };
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const int shapes[][2] = {{1, 4}, {3, 9}, {7, 5}, {16, 16}, {33, 20}, {1, 1}, {5, 630}, {70, 41}, {224, 224}};
  for (const auto& s : shapes)
    for (int stages = 0; stages <= 7; ++stages) {
      const int H = s[0], W = s[1], B = 6;
      std::vector<unsigned char> src((size_t)B * H * W * 3), u8((size_t)B * H * W * 3);
      for (auto& v : src) v = (unsigned char)rnd();
      std::vector<float> lut(768), out((size_t)B * 3 * H * W);
      for (int i = 0; i < 768; ++i) lut[i] = (float)(i % 256) / 255.f - 0.5f;
      // image 0: a plain record; 1: another order, gray; 2: nonsense codes; 3: extreme integers; 4: NaN / Inf factors and weights;
      // 5: huge weights (the sums overflow)
      std::vector<int> ops = {1, 0, 2, 3, 26, 0, 1, 0,      0, 3, 1, 2, 231, 1, 1, 0,      7, 1, 1, -9, 296, 5, -2, 99,
                              INT_MIN, INT_MAX, 3, 3, INT_MIN, INT_MAX, INT_MIN, INT_MAX,  2, 3, 0, 1, -30, 1, 1, 0,
                              3, 2, 1, 0, INT_MAX, 0, 1, 0};
      std::vector<float> coef = {0.83f, 1.4f, 0.6f, 0.f, 0.4f, 0.2f, 0.1f, 0.f, 0.f, 0.f, 0.f, 0.f,
                                 1.17f, 0.6f, 2.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                                 9.f, -3.f, nan, nan, 0.2f, 0.1f, 0.1f, 0.05f, 0.05f, 0.05f, 0.05f, nan,
                                 4.f, 0.f, 4.f, inf, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, -inf,
                                 nan, inf, -inf, 0.f, nan, inf, -inf, 0.3f, nan, 0.1f, inf, 0.f,
                                 1e30f, 1e-30f, -1e30f, 0.f, 3e38f, -3e38f, 3e38f, 3e38f, -3e38f, 1.f, -1.f, 0.f};
      std::vector<int> work(B);
      if (host_color_augment(src.data(), ops.data(), coef.data(), lut.data(), B, H, W, stages, work.data(), out.data(), 0,
                             u8.data()) != 0) {
        printf("rejected %d x %d\n", H, W);
        return 1;
      }
      for (auto v : u8) sum = sum * 31 + v;
    }
  if (host_color_augment_band(5, 631) != -1 || host_color_augment_band(0, 4) != -1) return 1;
  printf("color_host: checksum %llu\n", sum);
  return 0;
}
#endif
