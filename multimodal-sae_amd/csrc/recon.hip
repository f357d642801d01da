// recon.hip -- reconstruction error against sparsity: for a token's canonical top-k list and up to 16
// checkpoints kappa_0 < kappa_1 < ... <= k, the moments (|r - x|^2, x . r, |r|^2) of the kappa-sparse reconstruction
// r_kappa = decode(first kappa entries) + b_dec, and |x|^2 -- in ONE pass over the k decoder rows, without writing a [T, d]
// reconstruction.  The list is value-descending, so its first kappa columns ARE the top-kappa list, and msae_decode_f32 is a
// slot-ordered fma chain from +0 with + b_dec behind it: the chain's partial sum after kappa slots, + b_dec, is bit for bit
// what msae_decode_f32 returns for the truncated list.  The statement the kernel is held to is in include/msae.h
// ("reconstruction error against sparsity").
//
// recon_curve_kernel: ONE WORKGROUP PER TOKEN, 256 threads.  The list goes to LDS once (value 0 / row 0 for an entry that is
// skipped, as decode.hip does).  The d columns are walked in slabs of 1024 (16 B per lane; 256, one column per lane, when
// d % 4 != 0 or a pointer is unaligned): a lane holds its x values and its chain accumulators in registers, walks the rows
// from checkpoint to checkpoint (RC_UNROLL loads in flight), and at a checkpoint forms r, e and its three partial sums.
// Summation order of a moment (fixed by d and the load path alone):
//   lane:      fmaf over the lane's columns in ascending order, from +0 (a lane past d contributes +0)
//   wave:      wave_sum's xor butterfly, partner distance 32 down to 1
//   workgroup: ((w0 + w1) + w2) + w3 over the four waves
//   token:     the slab sums added in slab order, from +0
// No floating-point atomics, nothing shared between tokens: a token's outputs are the same bits in any batch.
// LDS: 8 k bytes of list (32 KiB at the envelope k = 4096) + 800 bytes of wave partials.
#include "common.h"
#include "wave_ops.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_WAVES = RC_THREADS / MSAE_WAVE;
constexpr int RC_UNROLL = 8;
constexpr int RC_MAX_K = 4096;
constexpr int RC_MAX_C = MSAE_RECON_MAX_CHECKPOINTS;

struct ReconKs {
  int k[RC_MAX_C];
};

// one row into the chain: decode.hip's step, a zero value leaves the accumulator's bits alone
template <int W>
__device__ __forceinline__ void rc_step(float (&acc)[W], float v, const float (&w)[W]) {
#pragma unroll
  for (int e = 0; e < W; ++e) {
    const float f = __builtin_fmaf(v, w[e], acc[e]);
    acc[e] = (v == 0.f) ? acc[e] : f;
  }
}

template <int W>
__device__ __forceinline__ void rc_load(float (&o)[W], const float *p) {
  if constexpr (W == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
  } else {
    o[0] = *p;
  }
}

// rows [j, j1) of the list into acc, U at a time with U loads in flight; returns the first row not taken
template <int W, int U>
__device__ __forceinline__ int rc_walk(float (&acc)[W], const float *l_val, const int *l_row, int j, int j1,
                                       const float *__restrict__ W_col, int d) {
  for (; j + U <= j1; j += U) {
    float w[U][W];
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = l_val[j + u];
      const int row = __builtin_amdgcn_readfirstlane(l_row[j + u]);      // the list is the workgroup's: uniform
      rc_load<W>(w[u], W_col + (size_t)row * d);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) rc_step<W>(acc, v[u], w[u]);
  }
  return j;
}

// grid: (T)
template <typename IT, int DT, bool VEC>
__global__ __launch_bounds__(RC_THREADS) void recon_curve_kernel(
    const void *__restrict__ x, const float *__restrict__ vals, const IT *__restrict__ idx, int ld,
    const float *__restrict__ W_dec, const float *__restrict__ b_dec, int k, int N, int d, ReconKs ks, int C,
    float *__restrict__ mom, float *__restrict__ xx, int32_t *__restrict__ status) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int SLAB = RC_THREADS * W;
  extern __shared__ __attribute__((aligned(16))) unsigned rc_smem[];     // 2 k words
  float *l_val = reinterpret_cast<float *>(rc_smem);                     // [k] 0 for a skipped entry
  int *l_row = reinterpret_cast<int *>(rc_smem + k);                     // [k] 0 for a skipped entry
  __shared__ float red[RC_WAVES][RC_MAX_C * 3 + 1];                      // a wave's partials of one slab; [..][3 C]: x . x

  const size_t t = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (MSAE_WAVE - 1), wave = tid >> 6;

  for (int j = tid; j < k; j += RC_THREADS) {
    const IT iw = idx[t * (size_t)ld + j];
    float v = vals[t * (size_t)ld + j];
    int row = (int)iw;
    if (iw < 0 || iw >= (IT)N) {
      v = 0.f;
      row = 0;
      if (status) atomicOr(status, 1);
    }
    l_val[j] = v;
    l_row[j] = row;
  }
  __syncthreads();

  float tot = 0.f;                                   // thread o < 3 C + 1 owns output o of this token
  const int n_out = 3 * C + 1;
  for (int c0 = 0; c0 < d; c0 += SLAB) {
    const int col = c0 + tid * W;
    const bool live = col < d;                       // (d % W == 0 on the vector path: a lane is whole or empty)
    float xv[W], bv[W], acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) xv[e] = bv[e] = acc[e] = 0.f;
    if (live) {
      if constexpr (VEC) {
        const f32x4 q = load_x4<DT>(x, t * (size_t)d + col);
        xv[0] = q[0]; xv[1] = q[1]; xv[2] = q[2]; xv[3] = q[3];
      } else {
        xv[0] = load_x1<DT>(x, t * (size_t)d + col);
      }
      rc_load<W>(bv, b_dec + col);
    }
    float sxx = 0.f;
#pragma unroll
    for (int e = 0; e < W; ++e) sxx = __builtin_fmaf(xv[e], xv[e], sxx);
    sxx = wave_sum(sxx);
    if (lane == 0) red[wave][3 * C] = sxx;

    int j = 0;
    for (int c = 0; c < C; ++c) {
      const int j1 = ks.k[c];
      if (live) {
        const float *W_col = W_dec + col;
        j = rc_walk<W, RC_UNROLL>(acc, l_val, l_row, j, j1, W_col, d);
        j = rc_walk<W, 4>(acc, l_val, l_row, j, j1, W_col, d);
        j = rc_walk<W, 1>(acc, l_val, l_row, j, j1, W_col, d);
      }
      float s_ee = 0.f, s_xr = 0.f, s_rr = 0.f;
#pragma unroll
      for (int e = 0; e < W; ++e) {
        const float xe = xv[e];
        const float r = acc[e] + bv[e];
        const float err = r - xe;
        s_ee = __builtin_fmaf(err, err, s_ee);
        s_xr = __builtin_fmaf(xe, r, s_xr);
        s_rr = __builtin_fmaf(r, r, s_rr);
      }
      s_ee = wave_sum(s_ee);
      s_xr = wave_sum(s_xr);
      s_rr = wave_sum(s_rr);
      if (lane == 0) {
        red[wave][3 * c + 0] = s_ee;
        red[wave][3 * c + 1] = s_xr;
        red[wave][3 * c + 2] = s_rr;
      }
    }
    __syncthreads();
    if (tid < n_out) tot += ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();                                 // the next slab writes `red` again
  }
  if (tid < 3 * C) mom[t * (size_t)(3 * C) + tid] = tot;
  else if (tid == 3 * C) xx[t] = tot;
}

template <typename IT, int DT>
int recon_curve_dtype(const void *x, const float *vals, const IT *idx, int ld, const float *W_dec, const float *b_dec, int T,
                      int k, int N, int d, const ReconKs &ks, int C, float *mom, float *xx, int32_t *status, hipStream_t st) {
  const size_t el = DT == MSAE_F32 ? 4 : 2;
  const bool vec = (d % 4 == 0) && msae_aligned(W_dec, 16) && msae_aligned(b_dec, 16) && msae_aligned(x, 4 * el);
  const size_t smem = (size_t)k * 2 * sizeof(unsigned);
  if (vec)
    hipLaunchKernelGGL((recon_curve_kernel<IT, DT, true>), dim3((unsigned)T), dim3(RC_THREADS), smem, st, x, vals, idx, ld,
                       W_dec, b_dec, k, N, d, ks, C, mom, xx, status);
  else
    hipLaunchKernelGGL((recon_curve_kernel<IT, DT, false>), dim3((unsigned)T), dim3(RC_THREADS), smem, st, x, vals, idx, ld,
                       W_dec, b_dec, k, N, d, ks, C, mom, xx, status);
  return msae_launch_status();
}

template <typename IT>
int recon_curve_impl(const void *x, int x_dtype, const float *vals, const IT *idx, int ld, const float *W_dec,
                     const float *b_dec, int T, int k, int N, int d, const int32_t *ks_host, int C, float *mom, float *xx,
                     int32_t *status, void *stream) {
  if (T < 0 || k < 1 || k > RC_MAX_K || N <= 0 || d <= 0 || ld < k || C < 1 || C > RC_MAX_C) return MSAE_EINVAL;
  if (x_dtype != MSAE_F32 && x_dtype != MSAE_BF16 && x_dtype != MSAE_F16) return MSAE_EINVAL;
  if (!x || !vals || !idx || !W_dec || !b_dec || !ks_host || !mom || !xx) return MSAE_EINVAL;
  ReconKs ks;
  for (int c = 0; c < RC_MAX_C; ++c) ks.k[c] = 0;
  for (int c = 0; c < C; ++c) {
    const int kc = ks_host[c];
    if (kc < 0 || kc > k || (c > 0 && kc <= ks_host[c - 1])) return MSAE_EINVAL;
    ks.k[c] = kc;
  }
  if (T == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (x_dtype) {
    case MSAE_F32: return recon_curve_dtype<IT, MSAE_F32>(x, vals, idx, ld, W_dec, b_dec, T, k, N, d, ks, C, mom, xx, status, st);
    case MSAE_BF16: return recon_curve_dtype<IT, MSAE_BF16>(x, vals, idx, ld, W_dec, b_dec, T, k, N, d, ks, C, mom, xx, status, st);
    default: return recon_curve_dtype<IT, MSAE_F16>(x, vals, idx, ld, W_dec, b_dec, T, k, N, d, ks, C, mom, xx, status, st);
  }
}

}  // namespace

extern "C" int msae_recon_curve_f32(const void *x, int x_dtype, const float *vals, const int32_t *idx, int ld,
                                    const float *W_dec, const float *b_dec, int T, int k, int N, int d, const int32_t *ks,
                                    int C, float *mom, float *xx, int32_t *status, void *stream) {
  return recon_curve_impl<int32_t>(x, x_dtype, vals, idx, ld, W_dec, b_dec, T, k, N, d, ks, C, mom, xx, status, stream);
}

extern "C" int msae_recon_curve_i64_f32(const void *x, int x_dtype, const float *vals, const int64_t *idx, int ld,
                                        const float *W_dec, const float *b_dec, int T, int k, int N, int d, const int32_t *ks,
                                        int C, float *mom, float *xx, int32_t *status, void *stream) {
  return recon_curve_impl<int64_t>(x, x_dtype, vals, idx, ld, W_dec, b_dec, T, k, N, d, ks, C, mom, xx, status, stream);
}
