// The training input path (include/msclip_input.h, msclip_amd/input_hip.py): crop + antialiased resize + flip + normalisation of a
// staged batch of decoded images in one launch.
//
// resized_crop_kernel: one workgroup of four waves owns one sample and one band of output rows.  Phase 0 writes the taps of every
// output column and of the band's rows into LDS (a thread per column / row); phase 1 runs the horizontal pass over the source rows
// the band needs, a thread per (row, column), reading the source bytes from HBM (neighbouring columns share their cache lines) and
// storing the three rounded channels as ONE dword of LDS (ds_write_b32, no sub-dword LDS traffic); phase 2 runs the vertical pass
// out of LDS, a thread per (row, column) with the column fastest, so that the fp32 stores of a wave are 256 contiguous bytes per
// channel.  The arithmetic is input_body.h, which a host program compiles too.  build.sh compiles this file without fast-math
// (pack.hip's flags): floor(x + 0.5), the division of the weights by their sum and the unfused multiply-adds must stay IEEE.
#include "common.h"
#include "plan.h"
#include "input_body.h"
#include "../../include/msclip_hip.h"
#include "../../include/msclip_input.h"

static_assert(msclip_crop::MAX_SCALE == MSCLIP_CROP_MAX_SCALE && msclip_crop::LDS_BYTES == MSCLIP_CROP_LDS_BYTES, "msclip_input.h");

namespace {

__global__ __launch_bounds__(256) void resized_crop_kernel(msclip_crop::Args a, int nbands) {
  extern __shared__ uint32_t crop_lds[];
  const int b = blockIdx.x / nbands, band0 = (blockIdx.x - b * nbands) * a.band;
#pragma unroll
  for (int ph = 0; ph < 3; ++ph) {
    msclip_crop::phase(a, b, band0, crop_lds, threadIdx.x, 256, ph);
    if (ph < 2) __syncthreads();
  }
}

}  // namespace

extern "C" int msclip_resized_crop_band(int slot_h, int slot_w, int out_h, int out_w, int filter) {
  msclip_crop::Plan p;
  return msclip_crop::make_plan(slot_h, slot_w, out_h, out_w, filter, &p) ? p.band : -1;
}

extern "C" int msclip_resized_crop_lds(int slot_h, int slot_w, int out_h, int out_w, int filter) {
  msclip_crop::Plan p;
  return msclip_crop::make_plan(slot_h, slot_w, out_h, out_w, filter, &p) ? p.lds_bytes : -1;
}

extern "C" int msclip_resized_crop(const void* src, int slot_h, int slot_w, const int* dims, const int* boxes, const int* flip,
                                   const float* lut, int B, int filter, int out_h, int out_w, void* out, int out_bf16, void* out_u8,
                                   void* stream) {
  MSCLIP_PLAN_HOOK(msclip_resized_crop, stream, src, slot_h, slot_w, dims, boxes, flip, lut, B, filter, out_h, out_w, out, out_bf16,
                   out_u8);
  if (!src || !dims || !boxes || !lut || !out || B <= 0) return MSCLIP_EINVAL;
  if ((((size_t)dims | (size_t)boxes | (size_t)flip | (size_t)lut) & 3) || ((size_t)out & (out_bf16 ? 1 : 3))) return MSCLIP_EINVAL;
  msclip_crop::Plan p;
  if (!msclip_crop::make_plan(slot_h, slot_w, out_h, out_w, filter, &p)) return MSCLIP_EINVAL;
  const long long nbands = (out_h + p.band - 1) / p.band;
  if (nbands * B > 0x7fffffffll) return MSCLIP_EINVAL;
  msclip_crop::Args a;
  a.src = (const unsigned char*)src;
  a.slot_h = slot_h;
  a.slot_w = slot_w;
  a.dims = dims;
  a.boxes = boxes;
  a.flip = flip;
  a.lut = lut;
  a.B = B;
  a.filter = filter;
  a.out_h = out_h;
  a.out_w = out_w;
  a.out = out;
  a.out_bf16 = out_bf16;
  a.out_u8 = (unsigned char*)out_u8;
  a.band = p.band;
  a.kx = p.kx;
  a.ky = p.ky;
  a.rows = p.rows;
  hipLaunchKernelGGL(resized_crop_kernel, dim3((unsigned)(nbands * B)), dim3(256), (size_t)p.lds_bytes, (hipStream_t)stream, a,
                     (int)nbands);
  return msclip_launch_status();
}

extern "C" int msclip_input_abi_version(void) { return MSCLIP_INPUT_ABI_VERSION; }
