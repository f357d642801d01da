// encode_f32.hip -- exact f32 encoder GEMM: out[T][N] = relu((x - b_dec) W_enc^T + b_enc), over all N features or over a
// feature list (msae_pre_acts_features_f32: the AuxK selection reads the dead latents only).
//
// Replaces Sae.pre_acts (reference sae/sae.py:172-177: nn.Linear in f32 + ReLU).
// Roofline: f32 MFMA (157 TFLOP/s dense on gfx950; there is no TF32/xf32).  2*d*N FLOP per token.
//
// v_mfma_f32_32x32x2_f32 computes, per output element, fma(a_k1, b_k1, fma(a_k0, b_k0, c)) with
// lanes 0-31 carrying k0 and lanes 32-63 carrying k1.  The K loop walks k in ascending order
// with ONE accumulator per output, so every pre-activation is the same ascending-k f32 fma chain
// as oracle/sae_oracle.c:msae_oracle_pre_acts -- compared bit-exactly in tests/.
//
// Tiling: 128 (tokens) x 128 (features) x 32 (k) per workgroup, 4 waves as 2x2, each wave a
// 64x64 tile = 2x2 MFMA blocks (64 accumulator VGPRs).  Operands are staged global -> registers
// -> LDS (x is up-cast and b_dec subtracted on the way), double-buffered, one barrier per k-tile.
// LDS rows: 36 floats, the k of a tile permuted (f_kpos): fragment reads are one ds_read_b128 per four k-steps, bank-conflict-free.  MFMA issue is the bound: 4 MFMAs (256 cycles/SIMD) per
// 4 ds_read_b32.
#include "f32_tile.h"
#include "tuning.h"

namespace {

template <int DT, bool VEC>
__global__ __launch_bounds__(F_THREADS, 2) void pre_acts_f32_kernel(
    const void *__restrict__ x, const float *__restrict__ W, const float *__restrict__ b_enc,
    const float *__restrict__ b_dec, const int *__restrict__ rows, const int *__restrict__ n_rows,
    int T, int d, int N, int relu, float *__restrict__ out, int ld_out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (n_rows) T = min(T, *n_rows);
  // row tiles blockIdx.y, +gridDim.y, ... and column tiles blockIdx.x, +gridDim.x, ...: with a device-side row count the
  // launch is sized for a few tiles only and a workgroup walks as many as the count needs (none -> it leaves at once: the
  // empty launch of the in-call exact fallback is 512 workgroups, not N / 128 * 2)
  for (int n0 = blockIdx.x * F_BN; n0 < N; n0 += gridDim.x * F_BN)
  for (int m0 = blockIdx.y * F_BM; m0 < T; m0 += gridDim.y * F_BM) {

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, khalf = lane >> 5;
  f32x16 acc[2][2];
  f32_tile_mma<DT, VEC>(acc, x, W, b_dec, rows, T, d, N, m0, n0, smem);

  // epilogue: C[row][col], col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wc * 64 + j * 32 + l31;
    if (n >= N) continue;
    const float bn = b_enc ? b_enc[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int t = m0 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * khalf;
        if (t < T) {
          float v = acc[i][j][e] + bn;
          if (relu && !(v > 0.f)) v = 0.f;
          out[(size_t)t * ld_out + n] = v;
        }
      }
    }
  }
  __syncthreads();   // LDS stages are rewritten by the next row tile
  }
}

// The same tile over a FEATURE list: column m of the output is feature cols[m] of W[N][d] (clamped into [0, N)), M columns.
// out[t][m] is bit for bit what pre_acts_f32_kernel writes at [t][cols[m]]: the same tile body, the bias of the gathered
// feature, the same ReLU rule.  A kernel of its own so that the dense one keeps its arguments and registers.
template <int DT, bool VEC>
__global__ __launch_bounds__(F_THREADS, 2) void pre_acts_cols_f32_kernel(
    const void *__restrict__ x, const float *__restrict__ W, const float *__restrict__ b_enc,
    const float *__restrict__ b_dec, const int *__restrict__ cols, int M, int T, int d, int N, int relu,
    float *__restrict__ out, int ld_out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n0 = blockIdx.x * F_BN, m0 = blockIdx.y * F_BM;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, khalf = lane >> 5;
  f32x16 acc[2][2];
  f32_tile_mma<DT, VEC, true>(acc, x, W, b_dec, nullptr, T, d, M, m0, n0, smem, cols, N);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = n0 + wc * 64 + j * 32 + l31;
    if (m >= M) continue;
    const float bn = b_enc ? b_enc[clamp_col(cols[m], N)] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int t = m0 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * khalf;
        if (t < T) {
          float v = acc[i][j][e] + bn;
          if (relu && !(v > 0.f)) v = 0.f;
          out[(size_t)t * ld_out + m] = v;
        }
      }
    }
  }
}

template <int DT>
int launch_cols_dt(const void *x, const float *W, const float *b_enc, const float *b_dec, const int *cols, int M, int T,
                   int d, int N, int relu, float *out, int ld_out, hipStream_t s) {
  const size_t xb = (DT == MSAE_F32) ? 16 : 8;
  const bool vec = (d % 4 == 0) && msae_aligned(x, xb) && msae_aligned(W, 16) && (!b_dec || msae_aligned(b_dec, 16));
  dim3 grid((M + F_BN - 1) / F_BN, (T + F_BM - 1) / F_BM);
  const size_t smem = F_LDS_FLOATS * sizeof(float);
  if (vec) {
    auto kern = pre_acts_cols_f32_kernel<DT, true>;
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, x, W, b_enc, b_dec, cols, M, T, d, N, relu, out, ld_out);
  } else {
    auto kern = pre_acts_cols_f32_kernel<DT, false>;
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, x, W, b_enc, b_dec, cols, M, T, d, N, relu, out, ld_out);
  }
  return msae_launch_status();
}

template <int DT>
int launch_dt(const void *x, const float *W, const float *b_enc, const float *b_dec, const int *rows,
              const int *n_rows, int T, int d, int N, int relu, float *out, int ld_out,
              hipStream_t s) {
  const size_t xb = (DT == MSAE_F32) ? 16 : 8;
  const bool vec = (d % 4 == 0) && msae_aligned(x, xb) && msae_aligned(W, 16) &&
                   (!b_dec || msae_aligned(b_dec, 16));
  int tiles_m = (T + F_BM - 1) / F_BM;
  int tiles_n = (N + F_BN - 1) / F_BN;
  if (n_rows && tiles_m > 2) tiles_m = 2;   // device-side count: workgroups loop over the row tiles ...
  if (n_rows && tiles_n > 256) tiles_n = 256;   // ... and over the column tiles
  if (n_rows) {                                  // (tuning.h MSAE_GRID_CAP: no cap in the product)
    tiles_n = msae_tuning::grid_cap(tiles_n);
    if (msae_tuning::GRID_CAP > 0) tiles_m = 1;
  }
  dim3 grid(tiles_n, tiles_m);
  const size_t smem = F_LDS_FLOATS * sizeof(float);
  if (vec) {
    auto kern = pre_acts_f32_kernel<DT, true>;
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)smem));
    hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, x, W, b_enc, b_dec, rows, n_rows, T, d,
                       N, relu, out, ld_out);
  } else {
    auto kern = pre_acts_f32_kernel<DT, false>;
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)smem));
    hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, x, W, b_enc, b_dec, rows, n_rows, T, d,
                       N, relu, out, ld_out);
  }
  return msae_launch_status();
}

}  // namespace

// Shared with encode_fused.hip (exact recompute of flagged tokens through a row list).
int msae_pre_acts_launch(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                         const float *b_dec, const int *rows, const int *n_rows, int T, int d, int N,
                         int relu, float *out, int ld_out, hipStream_t s) {
  if (T < 0 || d <= 0 || N <= 0 || ld_out < N) return MSAE_EINVAL;
  if (T == 0) return 0;
  if (!n_rows && (T + F_BM - 1) / F_BM > 65535) return MSAE_ENOTIMPL;
  switch (x_dtype) {
    case MSAE_F32: return launch_dt<MSAE_F32>(x, W_enc, b_enc, b_dec, rows, n_rows, T, d, N, relu, out, ld_out, s);
    case MSAE_BF16: return launch_dt<MSAE_BF16>(x, W_enc, b_enc, b_dec, rows, n_rows, T, d, N, relu, out, ld_out, s);
    case MSAE_F16: return launch_dt<MSAE_F16>(x, W_enc, b_enc, b_dec, rows, n_rows, T, d, N, relu, out, ld_out, s);
    default: return MSAE_EINVAL;
  }
}

extern "C" int msae_pre_acts_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                 const float *b_dec, int T, int d, int N, int relu, float *out,
                                 void *stream) {
  return msae_pre_acts_launch(x, x_dtype, W_enc, b_enc, b_dec, nullptr, nullptr, T, d, N, relu, out,
                              N, (hipStream_t)stream);
}

extern "C" int msae_pre_acts_features_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                          const float *b_dec, const int32_t *features, int M, int T, int d, int N,
                                          int relu, float *out, int ld_out, void *stream) {
  if (T < 0 || M < 0 || d <= 0 || N <= 0 || ld_out < M) return MSAE_EINVAL;
  if (T == 0 || M == 0) return 0;
  if (!x || !W_enc || !features || !out) return MSAE_EINVAL;
  if ((T + F_BM - 1) / F_BM > 65535) return MSAE_ENOTIMPL;
  hipStream_t s = (hipStream_t)stream;
  switch (x_dtype) {
    case MSAE_F32: return launch_cols_dt<MSAE_F32>(x, W_enc, b_enc, b_dec, features, M, T, d, N, relu, out, ld_out, s);
    case MSAE_BF16: return launch_cols_dt<MSAE_BF16>(x, W_enc, b_enc, b_dec, features, M, T, d, N, relu, out, ld_out, s);
    case MSAE_F16: return launch_cols_dt<MSAE_F16>(x, W_enc, b_enc, b_dec, features, M, T, d, N, relu, out, ld_out, s);
    default: return MSAE_EINVAL;
  }
}
