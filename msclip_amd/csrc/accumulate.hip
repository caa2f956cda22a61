// Gradient accumulation over the chunks of TrainStep.accumulate (train.py): every gradient tensor of a backward added into
// its persistent fp32 accumulator, all 325-406 tensors in a handful of launches.  Streaming, bound by HBM: 8 B per element
// in mode 0 (acc = g), 12 B in mode 1 (acc += g).  One IEEE add per element in call order, no atomics: bitwise torch's
// acc + g and bitwise repeatable.
#include "common.h"
#include "plan.h"
#include "../../include/msclip_hip_train.h"

namespace {

// block b works on piece (map[b] >> 8) of tensor (map[b] & 255): the table travels in the kernel arguments like
// msclip_adamw_multi's (backward.hip) -- the gradients' addresses change with every backward, a device-resident table would
// need an upload per chunk.  36 x 24 B + 768 x 4 B of kernel arguments (< 4 KiB).
constexpr int AC_TENSORS = 36, AC_BLOCKS = 768, AC_CHUNK = 32768;
struct AccumBatch {
  msclip_accum_tensor t[AC_TENSORS];
  unsigned map[AC_BLOCKS];
};
static_assert(sizeof(AccumBatch) <= 4000, "the tensor table travels in the kernel arguments");

template <int MODE>
__global__ __launch_bounds__(256) void accumulate_kernel(const AccumBatch a) {
  const unsigned e = a.map[blockIdx.x];
  const msclip_accum_tensor& t = a.t[e & 255u];
  const size_t lo = (size_t)(e >> 8) * AC_CHUNK;
  const size_t left = (size_t)t.n - lo;
  const int cnt = left < (size_t)AC_CHUNK ? (int)left : AC_CHUNK;
  float* __restrict__ acc = t.acc + lo;
  const float* __restrict__ g = t.g + lo;
  // 16-byte body [v0, v1) where acc and g sit at the same offset within 16 bytes (a piece starts a multiple of 128 KiB behind
  // its tensor, so that holds for every piece of a tensor or for none); scalar head [0, v0) and tail [v1, cnt)
  int v0 = 0, v1 = 0;
  if (!(((size_t)acc ^ (size_t)g) & 15)) {
    v0 = (int)(((16 - ((size_t)acc & 15)) & 15) >> 2);
    if (v0 > cnt) v0 = cnt;
    v1 = v0 + ((cnt - v0) & ~3);
  }
  const int edge = v0 + (cnt - v1);
  for (int i = threadIdx.x; i < edge; i += 256) {
    const int j = i < v0 ? i : v1 + (i - v0);
    acc[j] = MODE ? acc[j] + g[j] : g[j];
  }
  const int n4 = (v1 - v0) >> 2;
  float4* __restrict__ a4 = (float4*)(acc + v0);
  const float4* __restrict__ g4 = (const float4*)(g + v0);
  for (int i = threadIdx.x; i < n4; i += 1024) {           // four independent 16-byte loads per operand in flight per lane
    float4 gv[4], av[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 256;
      if (j < n4) {
        gv[u] = g4[j];
        if (MODE) av[u] = a4[j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 256;
      if (j < n4) {
        if (MODE) gv[u] = make_float4(av[u].x + gv[u].x, av[u].y + gv[u].y, av[u].z + gv[u].z, av[u].w + gv[u].w);
        a4[j] = gv[u];
      }
    }
  }
}

}  // namespace

extern "C" int msclip_train_abi_version(void) { return MSCLIP_TRAIN_ABI_VERSION; }

extern "C" int msclip_grad_accumulate(const msclip_accum_tensor* tensors, int count, int mode, void* stream) {
  MSCLIP_PLAN_UNSUPPORTED(msclip_grad_accumulate);
  if (!tensors || count < 0 || mode < 0 || mode > 1) return MSCLIP_EINVAL;
  for (int i = 0; i < count; ++i)
    if (!tensors[i].acc || !tensors[i].g || tensors[i].n <= 0 || (((size_t)tensors[i].acc | (size_t)tensors[i].g) & 3))
      return MSCLIP_EINVAL;
  AccumBatch b;
  int nt = 0, nb = 0;
  auto flush = [&]() {
    if (nb) {
      if (mode) hipLaunchKernelGGL(accumulate_kernel<1>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b);
      else hipLaunchKernelGGL(accumulate_kernel<0>, dim3(nb), dim3(256), 0, (hipStream_t)stream, b);
    }
    nt = nb = 0;
  };
  for (int i = 0; i < count; ++i) {
    const long long chunks = (tensors[i].n + AC_CHUNK - 1) / AC_CHUNK;
    long long c = 0;
    while (c < chunks) {
      if (nt == AC_TENSORS || nb == AC_BLOCKS) flush();
      // a tensor that continues in the next launch restarts there at piece c: shift its base instead of carrying an offset
      b.t[nt].acc = tensors[i].acc + c * AC_CHUNK;
      b.t[nt].g = tensors[i].g + c * AC_CHUNK;
      b.t[nt].n = tensors[i].n - c * AC_CHUNK;
      long long local = 0;
      while (c < chunks && nb < AC_BLOCKS) {
        b.map[nb++] = (unsigned)nt | ((unsigned)local << 8);
        ++local;
        ++c;
      }
      ++nt;
    }
  }
  flush();
  return msclip_launch_status();
}
