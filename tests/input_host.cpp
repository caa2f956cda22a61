// msclip_resized_crop's kernel body (msclip_amd/csrc/input_body.h) built for the host: the same three phases, every workgroup in
// turn, one "thread" each.  tests/test_input_cpu.py compiles this file with the host C++ compiler (-ffp-contract=off, no fast-math:
// the flags input.hip gets) into a shared object and compares it with the fp64 restatement and with PIL; the stand-alone program
// (-DINPUT_HOST_MAIN) is for a sanitizer build: it runs ragged cases, boxes outside their images included, and prints a checksum.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#undef NDEBUG
#include <vector>

#define MSCLIP_CROP_CHECK_GUARDS 1        // the plan's guards abort here instead of clamping silently
#include "../msclip_amd/csrc/input_body.h"

// host pointers throughout; returns 0, or -1 for what msclip_resized_crop rejects
extern "C" int host_resized_crop(const unsigned char* src, int slot_h, int slot_w, const int* dims, const int* boxes, const int* flip,
                                 const float* lut, int B, int filter, int out_h, int out_w, void* out, int out_bf16,
                                 unsigned char* out_u8) {
  msclip_crop::Plan p;
  if (!src || !dims || !boxes || !lut || !out || B <= 0) return -1;
  if (!msclip_crop::make_plan(slot_h, slot_w, out_h, out_w, filter, &p)) return -1;
  msclip_crop::Args a = {src, slot_h, slot_w, dims, boxes, flip, lut, B, filter, out_h, out_w, out, out_bf16, out_u8,
                         p.band, p.kx, p.ky, p.rows};
  std::vector<uint32_t> lds((size_t)p.lds_bytes / 4);          // exactly the device's allocation: a sanitizer sees an overrun
  for (int b = 0; b < B; ++b)
    for (int band0 = 0; band0 < out_h; band0 += p.band)
      for (int ph = 0; ph < 3; ++ph) msclip_crop::phase(a, b, band0, lds.data(), 0, 1, ph);
  return 0;
}

extern "C" int host_resized_crop_band(int slot_h, int slot_w, int out_h, int out_w, int filter) {
  msclip_crop::Plan p;
  return msclip_crop::make_plan(slot_h, slot_w, out_h, out_w, filter, &p) ? p.band : -1;
}

#ifdef INPUT_HOST_MAIN
int main() {
  unsigned long long sum = 0;
  unsigned seed = 12345u;
  auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (int)(seed >> 8); };
  const int shapes[][4] = {{23, 17, 7, 5}, {12, 12, 16, 16}, {64, 64, 16, 12}, {56, 40, 7, 5}, {400, 256, 224, 224},
                           {512, 512, 224, 224}, {8, 8, 1, 1}, {5, 300, 3, 38}};
  for (const auto& s : shapes)
    for (int filter = 2; filter <= 3; ++filter) {
      const int sh = s[0], sw = s[1], oh = s[2], ow = s[3], B = 5;
      std::vector<unsigned char> src((size_t)B * sh * sw * 3), u8((size_t)B * oh * ow * 3);
      for (auto& v : src) v = (unsigned char)rnd();
      std::vector<float> lut(768), out((size_t)B * 3 * oh * ow);
      for (int i = 0; i < 768; ++i) lut[i] = (float)(i % 256) / 255.f - 0.5f;
      // sample 0: the whole slot; 1: a random box inside; 2: a box outside its image; 3: nonsense values; 4: a 1 x 1 box
      std::vector<int> dims = {sh, sw, sh, sw, sh / 2 + 1, sw / 2 + 1, -7, 1 << 30, sh, sw};
      std::vector<int> boxes = {0, 0, sh, sw, rnd() % sh, rnd() % sw, 1 + rnd() % sh, 1 + rnd() % sw, sh - 1, sw - 1, sh, sw,
                                INT_MIN, INT_MAX, INT_MAX, -5, sh - 1, sw - 1, 1, 1};
      std::vector<int> flip = {0, 1, 0, 1, 0};
      if (host_resized_crop(src.data(), sh, sw, dims.data(), boxes.data(), flip.data(), lut.data(), B, filter, oh, ow, out.data(), 0,
                            u8.data()) != 0) {
        printf("rejected %d x %d -> %d x %d\n", sh, sw, oh, ow);
        return 1;
      }
      for (auto v : u8) sum = sum * 31 + v;
    }
  printf("input_host: checksum %llu\n", sum);
  return 0;
}
#endif
