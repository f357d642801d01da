// nested_decode.hip -- nested-prefix ("Matryoshka") decode: for bounds m_0 < m_1 < ... < m_{G-1} = N the
// reconstructions r_g of a token from the entries of its list whose feature lies below m_g, the residuals e_g = r_g - x and
// the squared errors |e_g|^2 -- in ONE pass over the token's decoder rows.  The statement the kernels are held to is in
// include/msae.h ("nested decode").
//
// nested_decode_kernel: ONE WORKGROUP PER TOKEN, 256 threads, after recon.hip's recon_curve_kernel.  The live entries of the
// list (slot < len, feature in [0, N), value != 0) go to LDS in GROUP-MAJOR order, a stable partition by group(feature): a
// thread owns a run of consecutive slots, one block_excl_scan of the threads' counts per group places them.  A dead entry is
// not stored at all: msae_decode_f32 leaves the accumulator's bits alone for it.  The checkpoints of the row walk are the
// cumulative group counts; the walk, the slabs and the summation order of sq are recon.hip's:
//   lane:      fmaf over the lane's columns in ascending order, from +0 (a lane past d contributes +0)
//   wave:      wave_sum's xor butterfly, partner distance 32 down to 1
//   workgroup: ((w0 + w1) + w2) + w3 over the four waves
//   token:     the slab sums added in slab order, from +0
// A lane holds one chain accumulator per column; at the end of group g it forms r_g and e_g, writes E[g] (and out behind the
// last group) and folds e_g^2 into its partial sum -- no residual outlives its checkpoint.  No floating-point atomics.
// LDS: 9 k bytes (list + group keys; 36 KiB at the envelope k = 4096) + the scan's and the reduction's few words.
//
// nested_combine_kernel: S[g] = coef[g] E[g] + S[g + 1] (S[G] = grad_full or +0), from the last plane down, in place on E.
#include "common.h"
#include "wave_ops.h"

namespace {

constexpr int ND_THREADS = 256;
constexpr int ND_WAVES = ND_THREADS / MSAE_WAVE;
constexpr int ND_UNROLL = 8;
constexpr int ND_MAX_K = 4096;
constexpr int ND_MAX_G = MSAE_NESTED_MAX_GROUPS;

struct NestedBounds {
  int m[ND_MAX_G];
};

// the number of g with m[g] <= n: 0 .. G - 1 for 0 <= n < N = m[G - 1]
__device__ __forceinline__ int nd_group(const NestedBounds &b, int G, int n) {
  int g = 0;
#pragma unroll
  for (int i = 0; i < ND_MAX_G; ++i) g += (i < G && b.m[i] <= n) ? 1 : 0;
  return g;
}

template <int W>
__device__ __forceinline__ void nd_load(float (&o)[W], const float *p) {
  if constexpr (W == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
  } else {
    o[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void nd_store(float *p, const float (&o)[W]) {
  if constexpr (W == 4) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{o[0], o[1], o[2], o[3]};
  } else {
    *p = o[0];
  }
}

// rows [j, j1) of the grouped list into acc, U at a time with U loads in flight; returns the first row not taken.  Every
// stored entry is live (value != 0): the step is decode.hip's fmaf.
template <int W, int U>
__device__ __forceinline__ int nd_walk(float (&acc)[W], const float *l_val, const int *l_row, int j, int j1,
                                       const float *__restrict__ W_col, int d) {
  for (; j + U <= j1; j += U) {
    float w[U][W];
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = l_val[j + u];
      const int row = __builtin_amdgcn_readfirstlane(l_row[j + u]);      // the list is the workgroup's: uniform
      nd_load<W>(w[u], W_col + (size_t)row * d);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] = __builtin_fmaf(v[u], w[u][e], acc[e]);
  }
  return j;
}

// grid: (T)
template <typename IT, int DT, bool VEC>
__global__ __launch_bounds__(ND_THREADS) void nested_decode_kernel(
    const void *__restrict__ x, const float *__restrict__ vals, const IT *__restrict__ idx, int ld,
    const int32_t *__restrict__ lengths, NestedBounds bounds, int G, const float *__restrict__ W_dec,
    const float *__restrict__ b_dec, int T, int k, int N, int d, float *__restrict__ out, float *__restrict__ E,
    float *__restrict__ sq, int32_t *__restrict__ status) {
  constexpr int W = VEC ? 4 : 1;
  constexpr int SLAB = ND_THREADS * W;
  extern __shared__ __attribute__((aligned(16))) unsigned nd_smem[];     // 2 k words + k bytes
  float *l_val = reinterpret_cast<float *>(nd_smem);                     // [k] the live entries, group-major
  int *l_row = reinterpret_cast<int *>(nd_smem + k);                     // [k]
  unsigned char *l_key = reinterpret_cast<unsigned char *>(nd_smem + 2 * (size_t)k);   // [k] group of slot j, 0xFF: dead
  __shared__ int wave_tot[ND_WAVES];
  __shared__ int s_ck[ND_MAX_G];                                         // live entries in the groups 0 .. g
  __shared__ float red[ND_WAVES][ND_MAX_G];                              // a wave's partials of one slab

  const size_t t = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (MSAE_WAVE - 1), wave = tid >> 6;
  const float *vp = vals + t * (size_t)ld;
  const IT *ip = idx + t * (size_t)ld;
  int len = k;
  if (lengths) {
    len = lengths[t];
    len = len < 0 ? 0 : (len > k ? k : len);
  }

  // ---- the group of every slot (the slots behind len are not read) ----
  for (int j = tid; j < len; j += ND_THREADS) {
    const IT iw = ip[j];
    const float v = vp[j];
    unsigned char key = 0xFF;
    if (iw < 0 || iw >= (IT)N) {
      if (status) atomicOr(status, 1);
    } else if (v != 0.f) {
      key = (unsigned char)nd_group(bounds, G, (int)iw);
    }
    l_key[j] = key;
  }
  // ---- stable partition: thread `tid` owns the slots [j0, j1), the scan runs in thread order = slot order ----
  const int per = (k + ND_THREADS - 1) / ND_THREADS;
  const int j0 = min(tid * per, len), j1 = min(j0 + per, len);
  int base = 0;
  __syncthreads();                                     // l_key is written
  for (int g = 0; g < G; ++g) {
    int c = 0;
    for (int j = j0; j < j1; ++j) c += l_key[j] == g ? 1 : 0;
    int total;
    int at = base + block_excl_scan<ND_WAVES>(c, wave_tot, &total);
    for (int j = j0; j < j1; ++j)
      if (l_key[j] == g) {
        l_val[at] = vp[j];
        l_row[at] = (int)ip[j];
        ++at;
      }
    base += total;
    if (tid == 0) s_ck[g] = base;
  }
  __syncthreads();

  float tot = 0.f;                                     // thread g < G owns sq[t][g]
  const size_t plane = (size_t)T * d;
  for (int c0 = 0; c0 < d; c0 += SLAB) {
    const int col = c0 + tid * W;
    const bool live = col < d;                         // (d % W == 0 on the vector path: a lane is whole or empty)
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
      nd_load<W>(bv, b_dec + col);
    }
    int j = 0;
    for (int g = 0; g < G; ++g) {
      const int jg = s_ck[g];
      float s_ee = 0.f;
      if (live) {
        const float *W_col = W_dec + col;
        j = nd_walk<W, ND_UNROLL>(acc, l_val, l_row, j, jg, W_col, d);
        j = nd_walk<W, 4>(acc, l_val, l_row, j, jg, W_col, d);
        j = nd_walk<W, 1>(acc, l_val, l_row, j, jg, W_col, d);
        float r[W], err[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
          r[e] = acc[e] + bv[e];
          err[e] = r[e] - xv[e];
          s_ee = __builtin_fmaf(err[e], err[e], s_ee);
        }
        if (E) nd_store<W>(E + (size_t)g * plane + t * (size_t)d + col, err);
        if (g == G - 1) nd_store<W>(out + t * (size_t)d + col, r);
      }
      s_ee = wave_sum(s_ee);
      if (lane == 0) red[wave][g] = s_ee;
    }
    __syncthreads();
    if (tid < G) tot += ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();                                   // the next slab writes `red` again
  }
  if (tid < G) sq[t * (size_t)G + tid] = tot;
}

template <typename IT, int DT>
int nested_decode_dtype(const void *x, const float *vals, const IT *idx, int ld, const int32_t *lengths,
                        const NestedBounds &b, int G, const float *W_dec, const float *b_dec, int T, int k, int N, int d,
                        float *out, float *E, float *sq, int32_t *status, hipStream_t st) {
  const size_t el = DT == MSAE_F32 ? 4 : 2;
  const bool vec = (d % 4 == 0) && msae_aligned(W_dec, 16) && msae_aligned(b_dec, 16) && msae_aligned(x, 4 * el) &&
                   msae_aligned(out, 16) && msae_aligned(E, 16);
  const size_t smem = msae_align_up((size_t)k * 9, 16);
  if (vec)
    hipLaunchKernelGGL((nested_decode_kernel<IT, DT, true>), dim3((unsigned)T), dim3(ND_THREADS), smem, st, x, vals, idx, ld,
                       lengths, b, G, W_dec, b_dec, T, k, N, d, out, E, sq, status);
  else
    hipLaunchKernelGGL((nested_decode_kernel<IT, DT, false>), dim3((unsigned)T), dim3(ND_THREADS), smem, st, x, vals, idx, ld,
                       lengths, b, G, W_dec, b_dec, T, k, N, d, out, E, sq, status);
  return msae_launch_status();
}

template <typename IT>
int nested_decode_impl(const void *x, int x_dtype, const float *vals, const IT *idx, int ld, const int32_t *lengths,
                       const int32_t *bounds_host, int G, const float *W_dec, const float *b_dec, int T, int k, int N, int d,
                       float *out, float *E, float *sq, int32_t *status, void *stream) {
  if (T < 0 || k < 1 || k > ND_MAX_K || N <= 0 || d <= 0 || ld < k || G < 1 || G > ND_MAX_G) return MSAE_EINVAL;
  if (x_dtype != MSAE_F32 && x_dtype != MSAE_BF16 && x_dtype != MSAE_F16) return MSAE_EINVAL;
  if (!x || !vals || !idx || !W_dec || !b_dec || !bounds_host || !out || !sq) return MSAE_EINVAL;
  NestedBounds b;
  for (int g = 0; g < ND_MAX_G; ++g) b.m[g] = 0x7FFFFFFF;
  for (int g = 0; g < G; ++g) {
    const int m = bounds_host[g];
    if (m < 1 || (g > 0 && m <= bounds_host[g - 1])) return MSAE_EINVAL;
    b.m[g] = m;
  }
  if (bounds_host[G - 1] != N) return MSAE_EINVAL;
  if (T == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (x_dtype) {
    case MSAE_F32:
      return nested_decode_dtype<IT, MSAE_F32>(x, vals, idx, ld, lengths, b, G, W_dec, b_dec, T, k, N, d, out, E, sq, status, st);
    case MSAE_BF16:
      return nested_decode_dtype<IT, MSAE_BF16>(x, vals, idx, ld, lengths, b, G, W_dec, b_dec, T, k, N, d, out, E, sq, status, st);
    default:
      return nested_decode_dtype<IT, MSAE_F16>(x, vals, idx, ld, lengths, b, G, W_dec, b_dec, T, k, N, d, out, E, sq, status, st);
  }
}

// one thread per W consecutive elements of a plane, grid-stride; n = T d elements per plane
template <bool VEC>
__global__ __launch_bounds__(256) void nested_combine_kernel(float *__restrict__ E, const float *__restrict__ coef,
                                                             const float *__restrict__ grad_full, size_t n, int G) {
  constexpr int W = VEC ? 4 : 1;
  float cf[ND_MAX_G];
#pragma unroll
  for (int g = 0; g < ND_MAX_G; ++g) cf[g] = g < G ? coef[g] : 0.f;
  const size_t nw = n / W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += (size_t)gridDim.x * 256) {
    float s[W];
#pragma unroll
    for (int e = 0; e < W; ++e) s[e] = 0.f;
    if (grad_full) nd_load<W>(s, grad_full + i * W);
#pragma unroll
    for (int g = ND_MAX_G - 1; g >= 0; --g) {
      if (g < G) {
        float ev[W];
        nd_load<W>(ev, E + (size_t)g * n + i * W);
#pragma unroll
        for (int e = 0; e < W; ++e) s[e] = __builtin_fmaf(cf[g], ev[e], s[e]);
        nd_store<W>(E + (size_t)g * n + i * W, s);
      }
    }
  }
}

}  // namespace

extern "C" int msae_nested_decode_f32(const void *x, int x_dtype, const float *vals, const int32_t *idx, int ld,
                                      const int32_t *lengths, const int32_t *bounds, int G, const float *W_dec,
                                      const float *b_dec, int T, int k, int N, int d, float *out, float *E, float *sq,
                                      int32_t *status, void *stream) {
  return nested_decode_impl<int32_t>(x, x_dtype, vals, idx, ld, lengths, bounds, G, W_dec, b_dec, T, k, N, d, out, E, sq,
                                     status, stream);
}

extern "C" int msae_nested_decode_i64_f32(const void *x, int x_dtype, const float *vals, const int64_t *idx, int ld,
                                          const int32_t *lengths, const int32_t *bounds, int G, const float *W_dec,
                                          const float *b_dec, int T, int k, int N, int d, float *out, float *E, float *sq,
                                          int32_t *status, void *stream) {
  return nested_decode_impl<int64_t>(x, x_dtype, vals, idx, ld, lengths, bounds, G, W_dec, b_dec, T, k, N, d, out, E, sq,
                                     status, stream);
}

extern "C" int msae_nested_combine_f32(float *E, const float *coef, const float *grad_full, int T, int d, int G,
                                       void *stream) {
  if (T < 0 || d <= 0 || G < 1 || G > ND_MAX_G) return MSAE_EINVAL;
  if (!E || !coef) return MSAE_EINVAL;
  if (T == 0) return 0;
  const size_t n = (size_t)T * d;
  // the planes lie n floats apart: 16-byte accesses need n % 4 == 0 as well as aligned bases
  const bool vec = (n % 4 == 0) && msae_aligned(E, 16) && msae_aligned(grad_full, 16);
  const size_t work = vec ? n / 4 : n;
  const unsigned grid = (unsigned)((work + 255) / 256 < 16384 ? (work + 255) / 256 : 16384);
  if (vec)
    hipLaunchKernelGGL(nested_combine_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, E, coef, grad_full, n, G);
  else
    hipLaunchKernelGGL(nested_combine_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, E, coef, grad_full, n, G);
  return msae_launch_status();
}
