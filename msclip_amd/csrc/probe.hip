// Linear probing (include/msclip_ext5.h, msclip_amd/linear_probe.py): the row pass of a softmax classifier's objective over an
// fp32 logits block, the fold of its loss partials, and the one-pass bf16 hi/lo split of an fp32 matrix.
//
// probe_rows_kernel: one workgroup of four waves owns 32 consecutive rows, wave w the rows w, w + 4, ... of them; a lane owns the
// columns 1024 t + 256 j + 4 lane + k (tile t, j < 4, k < 4) of every row.  Phase 1, row by row: max / argmax / rank in one sweep,
// the sum of exponentials in a second one (the row is 4 KB at 1000 classes: the second sweep is served by the cache), statistics
// into LDS.  Phase 2, column tile by column tile: G of the wave's rows, a lane adding its 16 columns' values over the rows in row
// order, then the four waves' sums as (w0 + w1) + (w2 + w3).  Streaming: R Cpad (4 + 2 + 2) bytes of HBM traffic.  Every output
// slot has one writer and every sum a fixed order: no atomics, no zero-fill, bitwise repeatable.  build.sh compiles this file without
// fast-math (pack.hip's flags): G - float(hi) must stay that subtraction, exp(-inf) must be 0, and expf / logf are the accurate ones.
#include "common.h"
#include "plan.h"
#include "../../include/msclip_hip.h"
#include "../../include/msclip_ext5.h"

namespace {

constexpr int RB = MSCLIP_PROBE_ROWS;     // rows of a workgroup
constexpr int TILE = 1024;                // columns of a tile: 64 lanes x 4 groups x 4 columns

// v[k] = S[c + k] + bias[c + k] for c + k < C, -inf beyond (the padding columns are never classes)
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ row, const float* __restrict__ bias, int c, int C, float (&v)[4]) {
  if constexpr (VEC) {                    // c % 4 == 0 and c + 3 < Cpad <= lds: inside the row
    const float4 a = *(const float4*)(row + c);
    const float s[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)                  // bias holds C entries, not Cpad: element by element (a few KB, cached)
      v[k] = c + k < C ? s[k] + (bias ? bias[c + k] : 0.f) : -INFINITY;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c + k < C ? row[c + k] + (bias ? bias[c + k] : 0.f) : -INFINITY;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void probe_rows_kernel(const float* __restrict__ S, int lds, const float* __restrict__ bias,
                                                         const int* __restrict__ labels, int R, int C, int Cpad, float w,
                                                         float* __restrict__ lse_out, bf16_t* __restrict__ Ghi,
                                                         bf16_t* __restrict__ Glo, int ldg, double* __restrict__ loss_part,
                                                         float* __restrict__ colsum_part, int ldp, int* __restrict__ pred,
                                                         int* __restrict__ rank_out, int* __restrict__ bad_part) {
  __shared__ float sm_lse[RB];
  __shared__ int sm_lab[RB];
  __shared__ double sm_loss[4];
  __shared__ int sm_bad[4];
  __shared__ float sm_col[4][TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * RB;
  const int ntile = (Cpad + TILE - 1) / TILE;

  // ---- phase 1: the statistics of the wave's rows
  double loss = 0.0;
  int bad = 0;
  for (int i = wave; i < RB; i += 4) {
    const int r = r0 + i;
    if (r >= R) break;
    const float* __restrict__ row = S + (size_t)r * lds;
    int lab = -1;
    float vl = 0.f;
    if (labels) {
      lab = labels[r];
      if (lab < 0 || lab >= C) {
        ++bad;
        lab = lab < 0 ? 0 : C - 1;
      }
      vl = row[lab] + (bias ? bias[lab] : 0.f);
    }
    float mx = -INFINITY;
    int arg = 0x7fffffff, rank = 0;
    for (int t = 0; t < ntile; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = t * TILE + j * 256 + lane * 4;
        if (c >= C) continue;
        float v[4];
        load4<VEC>(row, bias, c, C, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) {             // a lane's columns ascend: strict > keeps its lowest index
          if (v[k] > mx) { mx = v[k]; arg = c + k; }
          rank += (labels && v[k] > vl) ? 1 : 0;
        }
      }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float omx = __shfl_xor(mx, o, 64);
      const int oarg = __shfl_xor(arg, o, 64);
      rank += __shfl_xor(rank, o, 64);
      if (omx > mx || (omx == mx && oarg < arg)) { mx = omx; arg = oarg; }
    }
    float s = 0.f;
    for (int t = 0; t < ntile; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = t * TILE + j * 256 + lane * 4;
        if (c >= C) continue;
        float v[4];
        load4<VEC>(row, bias, c, C, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) s += c + k < C ? expf(v[k] - mx) : 0.f;
      }
    s = wave_sum(s);
    const float lse = mx + logf(s);
    if (lane == 0) {
      sm_lse[i] = lse;
      sm_lab[i] = lab;
      if (lse_out) lse_out[r] = lse;
      if (pred) pred[r] = arg;
      if (rank_out) rank_out[r] = rank;
      loss += (double)(lse - vl);
    }
  }
  if (lane == 0) {
    sm_loss[wave] = loss;
    sm_bad[wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (loss_part) loss_part[blockIdx.x] = (sm_loss[0] + sm_loss[1]) + (sm_loss[2] + sm_loss[3]);
    if (bad_part) bad_part[blockIdx.x] = (sm_bad[0] + sm_bad[1]) + (sm_bad[2] + sm_bad[3]);
  }
  if (!Ghi) return;

  // ---- phase 2: G = w (softmax - onehot) as bf16 hi + lo, and the workgroup's column sums of the fp32 G
  for (int t = 0; t < ntile; ++t) {
    float acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int i = wave; i < RB; i += 4) {
      const int r = r0 + i;
      if (r >= R) break;
      const float* __restrict__ row = S + (size_t)r * lds;
      const float lse = sm_lse[i];
      const int lab = sm_lab[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = t * TILE + j * 256 + lane * 4;
        if (c >= Cpad) continue;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
          float v[4];
          load4<VEC>(row, bias, c, C, v);
#pragma unroll
          for (int k = 0; k < 4; ++k) g[k] = c + k < C ? w * (expf(v[k] - lse) - (c + k == lab ? 1.f : 0.f)) : 0.f;
        }
        bf16_t hi[4], lo[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          hi[k] = f32_to_bf16(g[k]);
          lo[k] = f32_to_bf16(g[k] - bf16_to_f32(hi[k]));
          acc[j * 4 + k] += g[k];
        }
        bf16_t* __restrict__ ph = Ghi + (size_t)r * ldg + c;
        bf16_t* __restrict__ pl = Glo + (size_t)r * ldg + c;
        if constexpr (VEC) {
          *(uint2*)ph = make_uint2((uint32_t)hi[0] | ((uint32_t)hi[1] << 16), (uint32_t)hi[2] | ((uint32_t)hi[3] << 16));
          *(uint2*)pl = make_uint2((uint32_t)lo[0] | ((uint32_t)lo[1] << 16), (uint32_t)lo[2] | ((uint32_t)lo[3] << 16));
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (c + k < Cpad) { ph[k] = hi[k]; pl[k] = lo[k]; }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) sm_col[wave][j * 256 + lane * 4 + k] = acc[j * 4 + k];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cl = q * 256 + (int)threadIdx.x, c = t * TILE + cl;
      if (c < Cpad) colsum_part[(size_t)blockIdx.x * ldp + c] = (sm_col[0][cl] + sm_col[1][cl]) + (sm_col[2][cl] + sm_col[3][cl]);
    }
    __syncthreads();
  }
}

// One workgroup: thread t adds entries t, t + 256, ... in double, six xor-shuffle steps, (w0 + w1) + (w2 + w3) (clip.hip's fold).
__global__ __launch_bounds__(256) void probe_loss_fold_kernel(const double* __restrict__ part, long long n, long long denom,
                                                              double* __restrict__ out) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) s += part[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + (red[2] + red[3])) / (double)denom;
}

template <bool VEC>
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* __restrict__ x, int ldx, bf16_t* __restrict__ out, int ldo,
                                                         long long M, int C) {
  const int c4 = (C + 3) >> 2;                                   // groups of four columns per row
  const long long total = M * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long m = i / c4;
    const int c = (int)(i - m * c4) * 4;
    const float* __restrict__ px = x + (size_t)m * ldx + c;
    bf16_t* __restrict__ ph = out + (size_t)m * ldo + c;
    bf16_t* __restrict__ pl = ph + C;
    if constexpr (VEC) {
      const float4 a = *(const float4*)px;
      const float v[4] = {a.x, a.y, a.z, a.w};
      bf16_t hi[4], lo[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hi[k] = f32_to_bf16(v[k]);
        lo[k] = f32_to_bf16(v[k] - bf16_to_f32(hi[k]));
      }
      *(uint2*)ph = make_uint2((uint32_t)hi[0] | ((uint32_t)hi[1] << 16), (uint32_t)hi[2] | ((uint32_t)hi[3] << 16));
      *(uint2*)pl = make_uint2((uint32_t)lo[0] | ((uint32_t)lo[1] << 16), (uint32_t)lo[2] | ((uint32_t)lo[3] << 16));
    } else {
      for (int k = 0; k < 4 && c + k < C; ++k) {
        const bf16_t hi = f32_to_bf16(px[k]);
        ph[k] = hi;
        pl[k] = f32_to_bf16(px[k] - bf16_to_f32(hi));
      }
    }
  }
}

}  // namespace

extern "C" int msclip_probe_ce_rows(const float* S, int lds, const float* bias, const int* labels, int R, int C, int Cpad, float w,
                                    float* lse, void* G_hi, void* G_lo, int ldg, void* loss_part, float* colsum_part, int ldp,
                                    int* pred, int* rank, int* bad_part, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_probe_ce_rows, stream, S, lds, bias, labels, R, C, Cpad, w, lse, G_hi, G_lo, ldg, loss_part, colsum_part,
                   ldp, pred, rank, bad_part);
  if (!S || R <= 0 || C < 2 || Cpad < C || lds < Cpad) return MSCLIP_EINVAL;
  const size_t all = (size_t)S | (size_t)bias | (size_t)labels | (size_t)lse | (size_t)G_hi | (size_t)G_lo | (size_t)loss_part |
                     (size_t)colsum_part | (size_t)pred | (size_t)rank | (size_t)bad_part;
  if ((all & 3) || ((size_t)loss_part & 7)) return MSCLIP_EINVAL;
  if (G_hi) {
    if (!G_lo || !colsum_part || !labels || ldg < Cpad || ldp < Cpad) return MSCLIP_EINVAL;
  } else if (G_lo || colsum_part) {
    return MSCLIP_EINVAL;
  }
  if (!labels && (loss_part || rank || bad_part)) return MSCLIP_EINVAL;
  const bool vec = !((lds | Cpad) & 3) && !((size_t)S & 15) &&
                   (!G_hi || (!(ldg & 3) && !(((size_t)G_hi | (size_t)G_lo) & 7)));
  const dim3 grid((R + RB - 1) / RB);
  if (vec)
    hipLaunchKernelGGL(probe_rows_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, S, lds, bias, labels, R, C, Cpad, w, lse,
                       (bf16_t*)G_hi, (bf16_t*)G_lo, ldg, (double*)loss_part, colsum_part, ldp, pred, rank, bad_part);
  else
    hipLaunchKernelGGL(probe_rows_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, S, lds, bias, labels, R, C, Cpad, w, lse,
                       (bf16_t*)G_hi, (bf16_t*)G_lo, ldg, (double*)loss_part, colsum_part, ldp, pred, rank, bad_part);
  return msclip_launch_status();
}

extern "C" int msclip_probe_loss_fold(const void* loss_part, long long n, long long denom, void* out, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_probe_loss_fold, stream, loss_part, n, denom, out);
  if (!loss_part || !out || n <= 0 || denom <= 0 || (((size_t)loss_part | (size_t)out) & 7)) return MSCLIP_EINVAL;
  hipLaunchKernelGGL(probe_loss_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)loss_part, n, denom,
                     (double*)out);
  return msclip_launch_status();
}

extern "C" int msclip_split_bf16(const float* x, int ldx, void* out, int ldo, long long M, int C, void* stream) {
  MSCLIP_PLAN_HOOK(msclip_split_bf16, stream, x, ldx, out, ldo, M, C);
  if (!x || !out || M <= 0 || C <= 0 || ldx < C || (long long)ldo < 2ll * C || (((size_t)x | (size_t)out) & 3)) return MSCLIP_EINVAL;
  const bool vec = !((C | ldx | ldo) & 3) && !((size_t)x & 15) && !((size_t)out & 7);
  const long long groups = M * ((C + 3) / 4);
  const int grid = grid_for((size_t)groups, 256, msclip_device_cus() * 16);
  if (vec)
    hipLaunchKernelGGL(split_bf16_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ldx, (bf16_t*)out, ldo, M, C);
  else
    hipLaunchKernelGGL(split_bf16_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ldx, (bf16_t*)out, ldo, M, C);
  return msclip_launch_status();
}

extern "C" int msclip_ext5_abi_version(void) { return MSCLIP_EXT5_ABI_VERSION; }
