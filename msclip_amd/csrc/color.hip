// The colour stage of the training input path (include/msclip_color.h, msclip_amd/color_hip.py): colour jitter, grayscale, Gaussian
// blur and the table look-up of a batch of uint8 images, in two launches (one without jitter).
//
// color_mean_kernel: one workgroup of four waves per image.  Contrast blends with the mean gray value of the image as it stands
// when contrast's turn comes, so every thread applies the ops that precede contrast to its pixels in registers and sums L as 64-bit
// integers; the 256 partial sums are folded in LDS by a fixed tree (integers: any order gives the same sum) and thread 0 writes the
// mean to work[b].  No atomics, nothing to zero.
// color_band_kernel: one workgroup owns one image and one band of rows.  Phase 0 runs the whole pointwise chain over the band's rows
// and 6 mirrored halo rows on each side and stores the three channels as ONE dword of LDS; phase 1 runs the horizontal pass out of
// that buffer into a second one; phase 2 runs the vertical pass and stores.  A thread per pixel with the column fastest: the lanes of
// a wave read consecutive LDS dwords in both passes (no bank conflicts), and the fp32 stores of a wave are 256 contiguous bytes per
// channel.  An image whose blur flag is clear skips phases 0 and 1 and runs the chain straight into the stores; the flag is the same
// for the whole workgroup, so the barriers stay uniform.
// The arithmetic is color_body.h, which a host program compiles too.  build.sh compiles this file without fast-math and with
// -ffp-contract=off (input.hip's flags): the blend's two roundings, the IEEE divisions of the HSV conversions and the unfused
// multiply-adds of the blur are the definition.
#include "common.h"
#include "plan.h"
#include "color_body.h"
#include "../../include/msclip_hip.h"
#include "../../include/msclip_color.h"

static_assert(msclip_color::RADIUS == MSCLIP_COLOR_RADIUS && msclip_color::LDS_BYTES == MSCLIP_COLOR_LDS_BYTES, "msclip_color.h");

namespace {

__global__ __launch_bounds__(256) void color_mean_kernel(msclip_color::Args a) {
  __shared__ unsigned long long part[256];
  const int b = blockIdx.x;
  msclip_color::Rec rec;
  msclip_color::read_rec(a, b, &rec);
  part[threadIdx.x] = msclip_color::partial_sum(a, b, rec, threadIdx.x, 256);
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.work[b] = msclip_color::mean_of(part[0], a.H, a.W);
}

// Eight waves per workgroup: at the full LDS budget two workgroups share a CU, and the three phases are latency bound (LDS reads
// and barriers), so the band kernel brings 16 waves per CU rather than 8.
constexpr int BAND_THREADS = 512;

__global__ __launch_bounds__(BAND_THREADS) void color_band_kernel(msclip_color::Args a, int nbands) {
  extern __shared__ uint32_t color_lds[];
  const int b = blockIdx.x / nbands, band0 = (blockIdx.x - b * nbands) * a.band;
  msclip_color::Rec rec;
  msclip_color::read_rec(a, b, &rec);
  const int m = (a.stages & 1) ? a.work[b] : 0;
#pragma unroll
  for (int ph = 0; ph < 3; ++ph) {
    msclip_color::phase(a, b, band0, rec, m, color_lds, threadIdx.x, BAND_THREADS, ph);
    if (ph < 2) __syncthreads();
  }
}

}  // namespace

extern "C" int msclip_color_augment_band(int H, int W) {
  msclip_color::Plan p;
  return msclip_color::make_plan(H, W, &p) ? p.band : -1;
}

extern "C" int msclip_color_augment_lds(int H, int W) {
  msclip_color::Plan p;
  return msclip_color::make_plan(H, W, &p) ? p.lds_bytes : -1;
}

extern "C" int msclip_color_augment(const void* src_u8, const int* ops, const float* coef, const float* lut, int B, int H, int W,
                                    int stages, void* work, void* out, int out_bf16, void* out_u8, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_color_augment, stream, src_u8, ops, coef, lut, B, H, W, stages, work, out, out_bf16, out_u8);
  if (!src_u8 || !ops || !coef || !lut || !out || B <= 0 || stages < 0 || stages > 7) return MSCLIP_EINVAL;
  if ((stages & 1) && !work) return MSCLIP_EINVAL;
  if ((((size_t)ops | (size_t)coef | (size_t)lut | (size_t)work) & 3) || ((size_t)out & (out_bf16 ? 1 : 3))) return MSCLIP_EINVAL;
  if (out_u8 == src_u8) return MSCLIP_EINVAL;
  msclip_color::Plan p;
  if (!msclip_color::make_plan(H, W, &p)) return MSCLIP_EINVAL;
  const long long nbands = (H + p.band - 1) / p.band;
  if (nbands * B > 0x7fffffffll) return MSCLIP_EINVAL;
  msclip_color::Args a;
  a.src = (const unsigned char*)src_u8;
  a.ops = ops;
  a.coef = coef;
  a.lut = lut;
  a.B = B;
  a.H = H;
  a.W = W;
  a.stages = stages;
  a.work = (int*)work;
  a.out = out;
  a.out_bf16 = out_bf16;
  a.out_u8 = (unsigned char*)out_u8;
  a.band = p.band;
  if (stages & 1) hipLaunchKernelGGL(color_mean_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(color_band_kernel, dim3((unsigned)(nbands * B)), dim3(BAND_THREADS), (size_t)((stages & 4) ? p.lds_bytes : 0),
                     (hipStream_t)stream, a, (int)nbands);
  return msclip_launch_status();
}

extern "C" int msclip_color_abi_version(void) { return MSCLIP_COLOR_ABI_VERSION; }
