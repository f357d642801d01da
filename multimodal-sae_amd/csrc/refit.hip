// refit.hip -- least-squares refit on the encoder's support: keep the features a token's top-k list
// chose, solve for their best coefficients against the fixed decoder, and report the optimal error next to the encoder's own.
// The list is value-descending, so the top-kappa support is the first kappa slots; the Gram matrix, its Cholesky factor and
// the forward substitution of a prefix are leading blocks of the full ones: ONE Gram matrix, ONE factorisation and ONE forward
// solve per token give the optimal error at every sparsity kappa <= s (gain[j] = z_j^2).  The statement the kernel is held
// to is in include/msae.h ("support refit").
//
// support_refit_kernel: ONE WORKGROUP PER TOKEN, 256 threads, five phases.
//   1. Gram.  The d columns are walked in slabs of 128.  The live rows W_dec[idx[j]] and y = x - b_dec go to LDS (rows of 132
//      floats, each 32-column chunk k-permuted as f32_tile.h does, so a lane fetches four k-steps with one 16-byte read);
//      wave w multiplies chunk w of every slab with v_mfma_f32_32x32x2_f32: the 32 x 32 tiles of the lower triangle
//      (one for s <= 32, three above) and, per 32-row block, one tile against "y in column 0" for h = D y.  A fragment is read
//      once and used as the A and the B operand of up to four MFMAs.  The next slab's loads fly behind the MFMAs.
//      y . y is a plain fma chain in the 32 lanes that stage y.
//   2. Combine.  The four waves' partial tiles are added in LDS as ((w0 + w1) + w2) + w3.
//   3. Cholesky, right-looking over the (s + 1) x (s + 1) matrix [G h; h^T .] in LDS: row s carries h, so the forward solve is
//      the factorisation's own last row.  A pivot at or below tau * G_jj drops its slot.
//   4. Back solve in wave 0, z in registers, one lane per slot.
//   5. Second walk: recon.hip's slot-ordered chain, two accumulators per lane (the refit and the encoder's coefficients), and
//      its reduction order for the two squared errors.
// No floating-point atomics, nothing shared between tokens: a token's outputs are the same bits in any batch.
// LDS: (32 B + 1) * 132 * 4 bytes of slab (B = 1, 2 row blocks: 17.0 / 33.5 KiB) + 17.7 KiB of matrix and lists.
#include <type_traits>

#include "common.h"
#include "wave_ops.h"

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_WAVES = RF_THREADS / MSAE_WAVE;
constexpr int RF_MAX_S = MSAE_REFIT_MAX_S;
constexpr int RF_SLAB = 128;                       // columns per Gram slab: 32 per wave
constexpr int RF_PITCH = 132;                      // floats per LDS row: 16-byte reads of 16 rows hit every bank once
constexpr int RF_GP = RF_MAX_S + 1;                // pitch and order of the augmented matrix
constexpr int RF_UNROLL = 4;
constexpr int RF_MAX_D = 1 << 22;                  // tau's gamma_{d+s} needs (d + s) u well below 1

typedef float f32x2 __attribute__((ext_vector_type(2)));

// everything behind the slab in LDS (the slab comes first: the dynamic region's base is 16-byte aligned)
struct RefitLds {
  float G[RF_GP * RF_GP];       // lower triangle of [G h; h^T .]; L in place below the diagonal
  float diag0[RF_MAX_S];        // G_jj before the factorisation
  float ldiag[RF_MAX_S];        // L_jj
  float val[RF_MAX_S];          // the encoder's value, 0 for a dead slot
  float coef[RF_MAX_S];
  int row[RF_MAX_S];            // decoder row, -1 for a dead slot
  int ok[RF_MAX_S];             // the slot stayed in the support
  float red[RF_WAVES][2];
};

// raw staging registers of one slab: converted and centred when they are stored, behind the MFMAs
template <int DT, int NB>
struct RefitStage {
  f32x4 w[4 * NB];
  typename std::conditional<DT == MSAE_F32, f32x4, u16x4>::type x;
  f32x4 b;
};

template <int DT>
__device__ __forceinline__ f32x4 rf_cvt(const typename std::conditional<DT == MSAE_F32, f32x4, u16x4>::type &r) {
  if constexpr (DT == MSAE_F32) return r;
  else if constexpr (DT == MSAE_BF16) return f32x4{bf16_bits_to_f32(r[0]), bf16_bits_to_f32(r[1]), bf16_bits_to_f32(r[2]), bf16_bits_to_f32(r[3])};
  else return f32x4{f16_bits_to_f32(r[0]), f16_bits_to_f32(r[1]), f16_bits_to_f32(r[2]), f16_bits_to_f32(r[3])};
}

// four consecutive f32 at p[col .. col + 3], zeros at and beyond d (VEC: d % 4 == 0, so a quad is whole or empty)
template <bool VEC>
__device__ __forceinline__ f32x4 rf_load_w4(const float *p, int col, int d) {
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) {
    if (col < d) o = *reinterpret_cast<const f32x4 *>(p + col);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (col + e < d) o[e] = p[col + e];
  }
  return o;
}

// one quad into its k-permuted place of an LDS row: column 4 q + e of the slab lies in chunk q >> 3 at f_kpos(4 (q & 7) + e)
__device__ __forceinline__ void rf_store_quad(float *row, int q, const f32x4 &v) {
  float *p = row + 32 * (q >> 3) + 2 * (q & 7);
  *reinterpret_cast<f32x2 *>(p) = f32x2{v[0], v[2]};
  *reinterpret_cast<f32x2 *>(p + 16) = f32x2{v[1], v[3]};
}

template <int W>
__device__ __forceinline__ void rf_load(float (&o)[W], const float *p) {
  if constexpr (W == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
  } else {
    o[0] = *p;
  }
}

// recon.hip's step: a zero coefficient leaves the accumulator's bits alone
template <int W>
__device__ __forceinline__ void rf_step(float (&acc)[W], float v, const float (&w)[W]) {
#pragma unroll
  for (int e = 0; e < W; ++e) {
    const float f = __builtin_fmaf(v, w[e], acc[e]);
    acc[e] = (v == 0.f) ? acc[e] : f;
  }
}

// slots [j, j1) into both chains, U rows in flight
template <int W, int U>
__device__ __forceinline__ int rf_walk(float (&fit)[W], float (&enc)[W], const RefitLds &L, int j, int j1,
                                       const float *__restrict__ W_col, int d) {
  for (; j + U <= j1; j += U) {
    float w[U][W];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = __builtin_amdgcn_readfirstlane(L.row[j + u]);       // the list is the workgroup's: uniform
      rf_load<W>(w[u], W_col + (size_t)(row < 0 ? 0 : row) * d);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      rf_step<W>(fit, L.coef[j + u], w[u]);
      rf_step<W>(enc, L.val[j + u], w[u]);
    }
  }
  return j;
}

// grid: (T).  NB: 32-row blocks of the support (1: s <= 32, 2: s <= 64)
template <typename IT, int DT, bool VEC, int NB>
__global__ __launch_bounds__(RF_THREADS) void support_refit_kernel(
    const void *__restrict__ x, const float *__restrict__ vals, const IT *__restrict__ idx, int ld,
    const float *__restrict__ W_dec, const float *__restrict__ b_dec, int s, int N, int d, float tau,
    float *__restrict__ coef, float *__restrict__ gain, float *__restrict__ err_fit, float *__restrict__ err_enc,
    float *__restrict__ yy, int32_t *__restrict__ n_dep, int32_t *__restrict__ status) {
  constexpr int ROWS = 32 * NB;                                           // LDS row ROWS of the slab is y
  constexpr int NT = NB * (NB + 1) / 2;                                   // Gram tiles of the lower triangle
  extern __shared__ __attribute__((aligned(16))) float rf_smem[];
  float *slab = rf_smem;                                                  // [(ROWS + 1)][RF_PITCH]
  RefitLds &L = *reinterpret_cast<RefitLds *>(rf_smem + (ROWS + 1) * RF_PITCH);

  const size_t t = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (MSAE_WAVE - 1), wave = tid >> 6;
  const int l31 = lane & 31, khalf = lane >> 5;

  // ---- the list; dead rows of the slab are zeros for the whole walk ----
  if (tid < s) {
    const IT iw = idx[t * (size_t)ld + tid];
    float v = vals[t * (size_t)ld + tid];
    int row = (int)iw;
    if (iw < 0 || iw >= (IT)N) {
      v = 0.f;
      if (status) atomicOr(status, 1);
    }
    if (v == 0.f) row = -1;
    L.val[tid] = v;
    L.row[tid] = row;
  }
  for (int i = tid; i < (ROWS + 1) * RF_PITCH; i += RF_THREADS) slab[i] = 0.f;
  __syncthreads();

  // ---- phase 1: Gram ----
  // staging: thread (r0 = tid >> 5, q = tid & 31) owns quad q of rows r0 + 8 it; threads 0..31 also own quad q of y
  const int q = tid & 31, r0 = tid >> 5;
  const float *wrow[4 * NB];
#pragma unroll
  for (int it = 0; it < 4 * NB; ++it) {
    const int r = r0 + 8 * it;
    const int row = r < s ? L.row[r] : -1;
    wrow[it] = row < 0 ? nullptr : W_dec + (size_t)row * d;
  }
  RefitStage<DT, NB> st;
  auto load = [&](int c0) {
    const int col = c0 + 4 * q;
#pragma unroll
    for (int it = 0; it < 4 * NB; ++it)
      if (wrow[it]) st.w[it] = rf_load_w4<VEC>(wrow[it], col, d);
    if (tid < 32) {
      if constexpr (VEC) {
        const int cc = col < d ? col : 0;                                 // past d: any valid quad, zeroed at the store
        if constexpr (DT == MSAE_F32) st.x = *reinterpret_cast<const f32x4 *>(static_cast<const float *>(x) + t * (size_t)d + cc);
        else st.x = *reinterpret_cast<const u16x4 *>(static_cast<const unsigned short *>(x) + t * (size_t)d + cc);
        st.b = *reinterpret_cast<const f32x4 *>(b_dec + cc);
      } else {
        f32x4 xv = {0.f, 0.f, 0.f, 0.f}, bv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col + e < d) {
            xv[e] = load_x1<DT>(x, t * (size_t)d + col + e);
            bv[e] = b_dec[col + e];
          }
        st.b = xv - bv;                                                   // (scalar path: converted at the load, st.b carries y)
      }
    }
  };
  float yy_acc = 0.f;
  auto store = [&](int c0) {
#pragma unroll
    for (int it = 0; it < 4 * NB; ++it)
      if (wrow[it]) rf_store_quad(slab + (r0 + 8 * it) * RF_PITCH, q, st.w[it]);
    if (tid < 32) {
      f32x4 yv;
      if constexpr (VEC) {
        yv = rf_cvt<DT>(st.x) - st.b;
        if (c0 + 4 * q >= d) yv = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        yv = st.b;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) yy_acc = __builtin_fmaf(yv[e], yv[e], yy_acc);
      rf_store_quad(slab + ROWS * RF_PITCH, q, yv);
    }
  };

  f32x16 accG[NT], accH[NB];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) accG[i][e] = 0.f;
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) accH[i][e] = 0.f;

  load(0);
  for (int c0 = 0; c0 < d; c0 += RF_SLAB) {
    store(c0);
    __syncthreads();
    if (c0 + RF_SLAB < d) load(c0 + RF_SLAB);
    // wave w takes chunk w: k-step e of group g multiplies column 32 w + 8 g + 2 e (lanes 0-31) and + 1 (lanes 32-63)
    const float *a_base = slab + l31 * RF_PITCH + 32 * wave + 16 * khalf;
    const float *y_base = slab + ROWS * RF_PITCH + 32 * wave + 16 * khalf;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 a[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) a[b] = *reinterpret_cast<const f32x4 *>(a_base + 32 * b * RF_PITCH + 4 * g);
      f32x4 yv = *reinterpret_cast<const f32x4 *>(y_base + 4 * g);
      if (l31 != 0) yv = f32x4{0.f, 0.f, 0.f, 0.f};                       // the B operand "y in column 0"
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        accG[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0][e], a[0][e], accG[0], 0, 0, 0);
        accH[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0][e], yv[e], accH[0], 0, 0, 0);
        if constexpr (NB == 2) {
          accG[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1][e], a[0][e], accG[1], 0, 0, 0);
          accG[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1][e], a[1][e], accG[2], 0, 0, 0);
          accH[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1][e], yv[e], accH[1], 0, 0, 0);
        }
      }
    }
    __syncthreads();                                                      // the next slab overwrites the rows
  }

  // ---- phase 2: ((w0 + w1) + w2) + w3 into the lower triangle; h into row s ----
  for (int w = 0; w < RF_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ti = 0; ti < NT; ++ti) {
        const int bi = ti == 0 ? 0 : 1, bj = ti == 2 ? 1 : 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = 32 * bi + (e & 3) + 8 * (e >> 2) + 4 * khalf, j = 32 * bj + l31;
          if (i < s && j <= i) L.G[i * RF_GP + j] = w == 0 ? accG[ti][e] : L.G[i * RF_GP + j] + accG[ti][e];
        }
      }
      if (l31 == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int i = 32 * b + (e & 3) + 8 * (e >> 2) + 4 * khalf;
            if (i < s) L.G[s * RF_GP + i] = w == 0 ? accH[b][e] : L.G[s * RF_GP + i] + accH[b][e];
          }
      }
    }
    __syncthreads();
  }
  if (tid < s) L.diag0[tid] = L.G[tid * RF_GP + tid];
  if (wave == 0) {
    const float tot = wave_sum(yy_acc);                                   // lanes 32..63 hold +0
    if (lane == 0) yy[t] = tot;
  }

  // ---- phase 3: Cholesky of [G h; h^T .], column by column; row s becomes z ----
  int ndep = 0;
  for (int j = 0; j < s; ++j) {
    __syncthreads();
    const float p = L.G[j * RF_GP + j];
    const bool alive = L.row[j] >= 0;
    const bool ok = alive && p > tau * L.diag0[j];
    if (tid == 0) L.ok[j] = ok;
    if (!ok) {                                                            // uniform: dropped, its row and column are skipped
      ndep += alive;
      continue;
    }
    const float r = __builtin_sqrtf(p);
    if (tid == 0) L.ldiag[j] = r;
    const int ic = j + 1 + tid;
    if (ic <= s) L.G[ic * RF_GP + j] = L.G[ic * RF_GP + j] / r;
    __syncthreads();
    const int m = j + 1 + lane;
    if (m < s) {
      const float lm = L.G[m * RF_GP + j];
      for (int i = j + 1 + wave; i <= s; i += RF_WAVES)
        if (m <= i) L.G[i * RF_GP + m] = __builtin_fmaf(-L.G[i * RF_GP + j], lm, L.G[i * RF_GP + m]);
    }
  }
  __syncthreads();

  // ---- phase 4: gain and the back solve, wave 0, lane = slot ----
  if (wave == 0) {
    const bool mine = lane < s && L.ok[lane];
    float z = mine ? L.G[s * RF_GP + lane] : 0.f;
    if (lane < s) gain[t * (size_t)s + lane] = z * z;
    float c = 0.f;
    for (int j = s - 1; j >= 0; --j) {
      if (!L.ok[j]) continue;
      const float cj = __shfl(z, j, 64) / L.ldiag[j];
      if (lane == j) c = cj;
      if (lane < j) z = __builtin_fmaf(-L.G[j * RF_GP + lane], cj, z);
    }
    if (lane < s) {
      L.coef[lane] = c;
      coef[t * (size_t)s + lane] = c;
    }
    if (lane == 0) n_dep[t] = ndep;
  }
  __syncthreads();

  // ---- phase 5: the two reconstructions, directly ----
  constexpr int W = VEC ? 4 : 1;
  constexpr int SLAB2 = RF_THREADS * W;
  float tot = 0.f;                                                        // thread 0: err_fit, thread 1: err_enc
  for (int c0 = 0; c0 < d; c0 += SLAB2) {
    const int col = c0 + tid * W;
    const bool live = col < d;
    float yv[W], fit[W], enc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) yv[e] = fit[e] = enc[e] = 0.f;
    if (live) {
      float bv[W];
      if constexpr (VEC) {
        const f32x4 xq = load_x4<DT>(x, t * (size_t)d + col);
        yv[0] = xq[0]; yv[1] = xq[1]; yv[2] = xq[2]; yv[3] = xq[3];
      } else {
        yv[0] = load_x1<DT>(x, t * (size_t)d + col);
      }
      rf_load<W>(bv, b_dec + col);
#pragma unroll
      for (int e = 0; e < W; ++e) yv[e] = yv[e] - bv[e];
      const float *W_col = W_dec + col;
      int j = rf_walk<W, RF_UNROLL>(fit, enc, L, 0, s, W_col, d);
      rf_walk<W, 1>(fit, enc, L, j, s, W_col, d);
    }
    float s_fit = 0.f, s_enc = 0.f;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float ef = yv[e] - fit[e], ee = yv[e] - enc[e];
      s_fit = __builtin_fmaf(ef, ef, s_fit);
      s_enc = __builtin_fmaf(ee, ee, s_enc);
    }
    s_fit = wave_sum(s_fit);
    s_enc = wave_sum(s_enc);
    if (lane == 0) {
      L.red[wave][0] = s_fit;
      L.red[wave][1] = s_enc;
    }
    __syncthreads();
    if (tid < 2) tot += ((L.red[0][tid] + L.red[1][tid]) + L.red[2][tid]) + L.red[3][tid];
    __syncthreads();                                                      // the next slab writes `red` again
  }
  if (tid == 0) err_fit[t] = tot;
  else if (tid == 1) err_enc[t] = tot;
}

// tau = 2 gamma_{d+s}, gamma_n = n u / (1 - n u), u = 2^-24 (include/msae.h, "support refit", step 4)
float refit_tau(int d, int s) {
  const double nu = (double)(d + s) * 0x1p-24;
  return (float)(2.0 * nu / (1.0 - nu));
}

template <typename IT, int DT, bool VEC, int NB>
void refit_launch(const void *x, const float *vals, const IT *idx, int ld, const float *W_dec, const float *b_dec, int T,
                  int s, int N, int d, float *coef, float *gain, float *err_fit, float *err_enc, float *yy, int32_t *n_dep,
                  int32_t *status, hipStream_t st) {
  const size_t smem = (size_t)(32 * NB + 1) * RF_PITCH * sizeof(float) + sizeof(RefitLds);
  hipLaunchKernelGGL((support_refit_kernel<IT, DT, VEC, NB>), dim3((unsigned)T), dim3(RF_THREADS), smem, st, x, vals, idx,
                     ld, W_dec, b_dec, s, N, d, refit_tau(d, s), coef, gain, err_fit, err_enc, yy, n_dep, status);
}

template <typename IT, int DT>
int refit_dtype(const void *x, const float *vals, const IT *idx, int ld, const float *W_dec, const float *b_dec, int T, int s,
                int N, int d, float *coef, float *gain, float *err_fit, float *err_enc, float *yy, int32_t *n_dep,
                int32_t *status, hipStream_t st) {
  const size_t el = DT == MSAE_F32 ? 4 : 2;
  const bool vec = (d % 4 == 0) && msae_aligned(W_dec, 16) && msae_aligned(b_dec, 16) && msae_aligned(x, 4 * el);
#define RF_GO(VEC, NB) \
  refit_launch<IT, DT, VEC, NB>(x, vals, idx, ld, W_dec, b_dec, T, s, N, d, coef, gain, err_fit, err_enc, yy, n_dep, status, st)
  if (vec) {
    if (s <= 32) RF_GO(true, 1);
    else RF_GO(true, 2);
  } else {
    if (s <= 32) RF_GO(false, 1);
    else RF_GO(false, 2);
  }
#undef RF_GO
  return msae_launch_status();
}

template <typename IT>
int refit_impl(const void *x, int x_dtype, const float *vals, const IT *idx, int ld, const float *W_dec, const float *b_dec,
               int T, int s, int N, int d, float *coef, float *gain, float *err_fit, float *err_enc, float *yy,
               int32_t *n_dep, int32_t *status, void *stream) {
  if (T < 0 || s < 1 || s > RF_MAX_S || N <= 0 || d <= 0 || d > RF_MAX_D || ld < s) return MSAE_EINVAL;
  if (x_dtype != MSAE_F32 && x_dtype != MSAE_BF16 && x_dtype != MSAE_F16) return MSAE_EINVAL;
  if (!x || !vals || !idx || !W_dec || !b_dec || !coef || !gain || !err_fit || !err_enc || !yy || !n_dep) return MSAE_EINVAL;
  if (T == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (x_dtype) {
    case MSAE_F32: return refit_dtype<IT, MSAE_F32>(x, vals, idx, ld, W_dec, b_dec, T, s, N, d, coef, gain, err_fit, err_enc, yy, n_dep, status, st);
    case MSAE_BF16: return refit_dtype<IT, MSAE_BF16>(x, vals, idx, ld, W_dec, b_dec, T, s, N, d, coef, gain, err_fit, err_enc, yy, n_dep, status, st);
    default: return refit_dtype<IT, MSAE_F16>(x, vals, idx, ld, W_dec, b_dec, T, s, N, d, coef, gain, err_fit, err_enc, yy, n_dep, status, st);
  }
}

}  // namespace

extern "C" int msae_support_refit_f32(const void *x, int x_dtype, const float *vals, const int32_t *idx, int ld,
                                      const float *W_dec, const float *b_dec, int T, int s, int N, int d, float *coef,
                                      float *gain, float *err_fit, float *err_enc, float *yy, int32_t *n_dependent,
                                      int32_t *status, void *stream) {
  return refit_impl<int32_t>(x, x_dtype, vals, idx, ld, W_dec, b_dec, T, s, N, d, coef, gain, err_fit, err_enc, yy,
                             n_dependent, status, stream);
}

extern "C" int msae_support_refit_i64_f32(const void *x, int x_dtype, const float *vals, const int64_t *idx, int ld,
                                          const float *W_dec, const float *b_dec, int T, int s, int N, int d, float *coef,
                                          float *gain, float *err_fit, float *err_enc, float *yy, int32_t *n_dependent,
                                          int32_t *status, void *stream) {
  return refit_impl<int64_t>(x, x_dtype, vals, idx, ld, W_dec, b_dec, T, s, N, d, coef, gain, err_fit, err_enc, yy,
                             n_dependent, status, stream);
}
