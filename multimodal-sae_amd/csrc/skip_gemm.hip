// skip_gemm.hip -- the accumulating NT GEMM of a skip transcoder: C[M][ld_c] (+)= a[M][K] B[P][K]^T, exact f32.
//
// Two uses: the forward skip term yhat += x W_skip^T, accumulated in place into the decode's output,
// and the weight gradient dW_skip (+)= g^T x, accumulated into an existing .grad under gradient accumulation.
// Roofline: f32 MFMA (157 TFLOP/s dense on gfx950), 2*M*K*P FLOP; the epilogue reads C once more when it accumulates.
//
// The tile body is f32_tile.h's, as in pre_acts_f32_kernel: s[m][p] is the ascending-j f32 fma chain from +0, one accumulator
// per output.  The epilogue is a read-modify-write by the one thread that owns the element: C = C_in + s, one rounded f32 add.
// No atomics, no split-K: the bits do not depend on the grid or on timing.  A kernel of its own so that the dense encoder
// kernel keeps its arguments and registers (pre_acts_cols_f32_kernel was split off the same way).
#include "f32_tile.h"

namespace {

template <int DT, bool VEC>
__global__ __launch_bounds__(F_THREADS, 2) void gemm_nt_acc_f32_kernel(
    const void *__restrict__ a, const float *__restrict__ B, int M, int K, int P, float *C, size_t ld_c, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n0 = blockIdx.x * F_BN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, khalf = lane >> 5;
  // row tiles blockIdx.y, +gridDim.y, ...: the launch caps gridDim.y at the grid limit, so any M is served
  for (int m0 = blockIdx.y * F_BM; m0 < M; m0 += gridDim.y * F_BM) {
    f32x16 acc[2][2];
    f32_tile_mma<DT, VEC>(acc, a, B, nullptr, nullptr, M, K, P, m0, n0, smem);
    // epilogue: C[row][col], col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5); columns [P, ld_c) are never touched
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = n0 + wc * 64 + j * 32 + l31;
      if (p >= P) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * khalf;
          if (m < M) {
            float *c = C + (size_t)m * ld_c + p;
            *c = accumulate ? *c + acc[i][j][e] : acc[i][j][e];
          }
        }
      }
    }
    __syncthreads();   // LDS stages are rewritten by the next row tile
  }
}

template <int DT>
int launch_acc_dt(const void *a, const float *B, int M, int K, int P, float *C, size_t ld_c, int accumulate, hipStream_t s) {
  const size_t ab = (DT == MSAE_F32) ? 16 : 8;
  const bool vec = (K % 4 == 0) && msae_aligned(a, ab) && msae_aligned(B, 16);
  const int tiles_m = (M + F_BM - 1) / F_BM;
  dim3 grid((P + F_BN - 1) / F_BN, tiles_m < 65535 ? tiles_m : 65535);
  const size_t smem = F_LDS_FLOATS * sizeof(float);
  if (vec) {
    auto kern = gemm_nt_acc_f32_kernel<DT, true>;
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, a, B, M, K, P, C, ld_c, accumulate);
  } else {
    auto kern = gemm_nt_acc_f32_kernel<DT, false>;
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, a, B, M, K, P, C, ld_c, accumulate);
  }
  return msae_launch_status();
}

}  // namespace

extern "C" int msae_gemm_nt_acc_f32(const void *a, int a_dtype, const float *B, int M, int K, int P, float *C, int ld_c,
                                    int accumulate, void *stream) {
  if (M < 0 || K < 1 || P < 1 || ld_c < P) return MSAE_EINVAL;
  if (a_dtype != MSAE_F32 && a_dtype != MSAE_BF16 && a_dtype != MSAE_F16) return MSAE_EINVAL;
  if (M == 0) return 0;
  if (!a || !B || !C) return MSAE_EINVAL;
  // (the tile origins n0 = blockIdx.x * 128 and m0 + gridDim.y * 128 stay ints)
  if (P > 0x7fffffff - F_BN || M > 0x7fffffff - 65535 * F_BM) return MSAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  switch (a_dtype) {
    case MSAE_F32: return launch_acc_dt<MSAE_F32>(a, B, M, K, P, C, (size_t)ld_c, accumulate, s);
    case MSAE_BF16: return launch_acc_dt<MSAE_BF16>(a, B, M, K, P, C, (size_t)ld_c, accumulate, s);
    default: return launch_acc_dt<MSAE_F16>(a, B, M, K, P, C, (size_t)ld_c, accumulate, s);
  }
}
