// delta_decode.hip -- error-preserving interventions: out = x + (decode(Q) - decode(P)) for a token's plain
// top-k list P and its edited list Q, WITHOUT decoding either list: the entries the two lists share cancel, so only the
// entries that differ -- about 2 E of them after an edit of E features -- are gathered.  Where nothing was edited the token
// keeps x's own bits.  The statement the kernel is held to is in include/msae.h ("error-preserving interventions").
//
// delta_decode_kernel: ONE WORKGROUP PER (token, column slab), 256 threads, the slab 1024 columns (16 B per lane) or, for
// d % 4 != 0 or unaligned rows, 256 columns (one per lane) -- decode.hip's two layouts.
//   1. both lists go to LDS as 64-bit (feature, value bits) words with a feature outside [0, N) stored as -1 (and flagged)
//   2. entry j of a list survives when its value is not +-0, its feature is valid and the OTHER list holds no entry with the
//      same feature and the same value bits.  The search walks outwards from slot j: after an edit an entry sits at most E
//      slots from where it was, so the common entry is found in O(E) LDS reads and only the ~2 E real survivors scan the list
//      (16 independent reads per step: the scan of a survivor is what a workgroup waits for).
//   3. survivors are compacted in slot order (ballot + prefix count per wave, block_wave_offset across the waves) into the
//      difference sequence D = Q's survivors with +value, then P's with -value
//   4. |D| = 0: the slab of x is copied (or left alone when out aliases x) before any W_dec row is touched; else the rows of D
//      are gathered, DD_UNROLL loads in flight, through the explicit fma chain in D's order, and out = rne(f32(x) + delta).
// Every feature that indexes W_dec passed the range check of step 1: a hostile list can be wrong, not out of bounds.
// LDS: 32 k bytes (two lists of k (bits, feature) pairs + 2 k (coefficient, feature) pairs): 1 KiB at k = 32, 128 KiB at the
// envelope k = 4096 (one workgroup per CU there; the 64 KiB of the two lists alone is what the C ABI promises to fit).
#include "common.h"
#include "wave_ops.h"

namespace {

constexpr int DD_THREADS = 256;
constexpr int DD_WAVES = DD_THREADS / MSAE_WAVE;
constexpr int DD_UNROLL = 8;
constexpr int DD_MAX_K = 4096;            // msae_encode_topk's own limit on k (+ E)

// An entry as one 64-bit word: the feature (-1: out of range) above the value's bits, so "same feature, same bits" is one compare.
__device__ __forceinline__ unsigned long long dd_key(int feat, unsigned bits) {
  return ((unsigned long long)(unsigned)feat << 32) | bits;
}

// does keys[0 .. k) hold `key`?  Slots j, j -+ 1, j -+ 2, ... : nearest first, DD_SCAN distances (2 DD_SCAN independent LDS
// reads) per step.  A slot past either end is clamped onto the end: that entry IS a member of the list, so the answer stands.
constexpr int DD_SCAN = 8;
__device__ __forceinline__ bool dd_holds(const unsigned long long *keys, int k, int j, unsigned long long key) {
  for (int s0 = 0; s0 < k; s0 += DD_SCAN) {
    bool hit = false;
#pragma unroll
    for (int u = 0; u < DD_SCAN; ++u) {
      const int lo = max(j - s0 - u, 0), hi = min(j + s0 + u, k - 1);
      hit |= keys[lo] == key;
      hit |= keys[hi] == key;
    }
    if (hit) return true;
    if (j - s0 - (DD_SCAN - 1) <= 0 && j + s0 + (DD_SCAN - 1) >= k - 1) break;      // both ends reached
  }
  return false;
}

template <int DT>
__device__ __forceinline__ void store_x1(void *out, size_t i, float v) {
  if constexpr (DT == MSAE_F32) static_cast<float *>(out)[i] = v;
  else if constexpr (DT == MSAE_BF16) {
    const unsigned u = __float_as_uint(v);
    static_cast<unsigned short *>(out)[i] =
        (v != v) ? (unsigned short)((u >> 16) | 0x40u) : f32_to_bf16_bits(v);      // a NaN stays one (quiet bit set)
  } else {
    static_cast<unsigned short *>(out)[i] = __builtin_bit_cast(unsigned short, (_Float16)v);   // v_cvt_f16_f32: RNE
  }
}

// grid: (T, ceil(d / (VEC ? 1024 : 256)))
template <typename IT, int DT, bool VEC>
__global__ __launch_bounds__(DD_THREADS) void delta_decode_kernel(
    const void *x, const float *__restrict__ pv, const IT *__restrict__ pi, int ld_p,
    const float *__restrict__ qv, const IT *__restrict__ qi, int ld_q, const float *__restrict__ W_dec, int k, int N, int d,
    void *out, int32_t *__restrict__ status) {           // (out may alias x: neither is __restrict__)
  extern __shared__ __attribute__((aligned(16))) unsigned dd_smem[];     // 8 k words
  unsigned long long *q_key = reinterpret_cast<unsigned long long *>(dd_smem);     // [k]
  unsigned long long *p_key = q_key + k;                                            // [k]
  float *d_coef = reinterpret_cast<float *>(dd_smem + 4 * (size_t)k);   // [2 k]
  int *d_feat = reinterpret_cast<int *>(dd_smem + 6 * (size_t)k);       // [2 k]
  __shared__ int wave_tot[DD_WAVES];

  const size_t t = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (MSAE_WAVE - 1);

  // 1. the two lists
  for (int j = tid; j < 2 * k; j += DD_THREADS) {
    const bool edited = j < k;
    const int jj = edited ? j : j - k;
    const IT iw = edited ? qi[t * ld_q + jj] : pi[t * ld_p + jj];
    const float v = edited ? qv[t * ld_q + jj] : pv[t * ld_p + jj];
    const bool bad = iw < 0 || iw >= (IT)N;
    if (bad && status && blockIdx.y == 0) atomicOr(status, 1);
    (edited ? q_key : p_key)[jj] = dd_key(bad ? -1 : (int)iw, __float_as_uint(v));
  }
  __syncthreads();

  // 2. + 3. survivors, compacted in the order Q[0 .. k), P[0 .. k)
  int n = 0;                                                    // |D| so far (uniform over the workgroup)
  for (int base = 0; base < 2 * k; base += DD_THREADS) {
    const int j = base + tid;
    bool keep = false;
    unsigned b = 0;
    int f = -1;
    bool edited = true;
    if (j < 2 * k) {
      edited = j < k;
      const int jj = edited ? j : j - k;
      const unsigned long long key = (edited ? q_key : p_key)[jj];
      b = (unsigned)key;
      f = (int)(unsigned)(key >> 32);
      if ((b << 1) != 0u && f >= 0) keep = !dd_holds(edited ? p_key : q_key, k, jj, key);
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    int total;
    const int wbase = block_wave_offset<DD_WAVES>((int)__popcll(m), wave_tot, &total);
    if (keep) {
      const float v = __uint_as_float(b);
      d_coef[n + wbase + before] = edited ? v : -v;
      d_feat[n + wbase + before] = f;
    }
    n += total;
  }
  __syncthreads();

  // 4. the slab
  constexpr int W = VEC ? 4 : 1;
  const int col = (blockIdx.y * DD_THREADS + tid) * W;
  if (col >= d) return;
  const size_t xo = t * (size_t)d + col;
  if (n == 0) {                                                 // nothing differs: x's own bits
    if (out == x) return;
    if constexpr (DT == MSAE_F32) {
      if constexpr (VEC) *reinterpret_cast<u32x4 *>(static_cast<unsigned *>(out) + xo) =
          *reinterpret_cast<const u32x4 *>(static_cast<const unsigned *>(x) + xo);
      else static_cast<unsigned *>(out)[xo] = static_cast<const unsigned *>(x)[xo];
    } else {
      if constexpr (VEC) *reinterpret_cast<u16x4 *>(static_cast<unsigned short *>(out) + xo) =
          *reinterpret_cast<const u16x4 *>(static_cast<const unsigned short *>(x) + xo);
      else static_cast<unsigned short *>(out)[xo] = static_cast<const unsigned short *>(x)[xo];
    }
    return;
  }
  if constexpr (VEC) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int j = 0;
    for (; j + DD_UNROLL <= n; j += DD_UNROLL) {
      f32x4 w[DD_UNROLL];
      float c[DD_UNROLL];
#pragma unroll
      for (int u = 0; u < DD_UNROLL; ++u) {
        c[u] = d_coef[j + u];
        w[u] = *reinterpret_cast<const f32x4 *>(W_dec + (size_t)d_feat[j + u] * d + col);
      }
#pragma unroll
      for (int u = 0; u < DD_UNROLL; ++u) {
        acc[0] = __builtin_fmaf(c[u], w[u][0], acc[0]);
        acc[1] = __builtin_fmaf(c[u], w[u][1], acc[1]);
        acc[2] = __builtin_fmaf(c[u], w[u][2], acc[2]);
        acc[3] = __builtin_fmaf(c[u], w[u][3], acc[3]);
      }
    }
    for (; j < n; ++j) {
      const float c = d_coef[j];
      const f32x4 w = *reinterpret_cast<const f32x4 *>(W_dec + (size_t)d_feat[j] * d + col);
      acc[0] = __builtin_fmaf(c, w[0], acc[0]);
      acc[1] = __builtin_fmaf(c, w[1], acc[1]);
      acc[2] = __builtin_fmaf(c, w[2], acc[2]);
      acc[3] = __builtin_fmaf(c, w[3], acc[3]);
    }
    const f32x4 xv = load_x4<DT>(x, xo);
    f32x4 o;
    o[0] = xv[0] + acc[0]; o[1] = xv[1] + acc[1]; o[2] = xv[2] + acc[2]; o[3] = xv[3] + acc[3];
    if constexpr (DT == MSAE_F32) {
      *reinterpret_cast<f32x4 *>(static_cast<float *>(out) + xo) = o;
    } else {
      unsigned short r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) store_x1<DT>(r, e, o[e]);
      const u16x4 pk = {r[0], r[1], r[2], r[3]};
      *reinterpret_cast<u16x4 *>(static_cast<unsigned short *>(out) + xo) = pk;
    }
  } else {
    float acc = 0.f;
    for (int j = 0; j < n; ++j) acc = __builtin_fmaf(d_coef[j], W_dec[(size_t)d_feat[j] * d + col], acc);
    store_x1<DT>(out, xo, load_x1<DT>(x, xo) + acc);
  }
}

template <typename IT, int DT>
int delta_decode_dtype(const void *x, const float *pv, const IT *pi, int ld_p, const float *qv, const IT *qi, int ld_q,
                       const float *W_dec, int T, int k, int N, int d, void *out, int32_t *status, hipStream_t st) {
  const size_t el = DT == MSAE_F32 ? 4 : 2;
  const bool vec = (d % 4 == 0) && msae_aligned(W_dec, 16) && msae_aligned(x, 4 * el) && msae_aligned(out, 4 * el);
  const size_t smem = (size_t)k * 8 * sizeof(unsigned);
  const int per = DD_THREADS * (vec ? 4 : 1);
  const dim3 grid((unsigned)T, (unsigned)((d + per - 1) / per));
#define DD_LAUNCH(V)                                                                                                      \
  do {                                                                                                                    \
    auto kern = delta_decode_kernel<IT, DT, V>;                                                                           \
    if (smem > 64 * 1024)                                                                                                 \
      MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));       \
    hipLaunchKernelGGL(kern, grid, dim3(DD_THREADS), smem, st, x, pv, pi, ld_p, qv, qi, ld_q, W_dec, k, N, d, out, status); \
  } while (0)
  if (vec) DD_LAUNCH(true); else DD_LAUNCH(false);
#undef DD_LAUNCH
  return msae_launch_status();
}

template <typename IT>
int delta_decode_impl(const void *x, int x_dtype, const float *pv, const IT *pi, int ld_p, const float *qv, const IT *qi,
                      int ld_q, const float *W_dec, int T, int k, int N, int d, void *out, int32_t *status, void *stream) {
  if (T < 0 || k < 1 || k > DD_MAX_K || N <= 0 || d <= 0 || ld_p < k || ld_q < k) return MSAE_EINVAL;
  if (x_dtype != MSAE_F32 && x_dtype != MSAE_BF16 && x_dtype != MSAE_F16) return MSAE_EINVAL;
  if (!x || !pv || !pi || !qv || !qi || !W_dec || !out) return MSAE_EINVAL;
  if (T == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (x_dtype) {
    case MSAE_F32: return delta_decode_dtype<IT, MSAE_F32>(x, pv, pi, ld_p, qv, qi, ld_q, W_dec, T, k, N, d, out, status, st);
    case MSAE_BF16: return delta_decode_dtype<IT, MSAE_BF16>(x, pv, pi, ld_p, qv, qi, ld_q, W_dec, T, k, N, d, out, status, st);
    default: return delta_decode_dtype<IT, MSAE_F16>(x, pv, pi, ld_p, qv, qi, ld_q, W_dec, T, k, N, d, out, status, st);
  }
}

}  // namespace

extern "C" int msae_delta_decode_f32(const void *x, int x_dtype, const float *plain_vals, const int32_t *plain_idx,
                                     int ld_plain, const float *edit_vals, const int32_t *edit_idx, int ld_edit,
                                     const float *W_dec, int T, int k, int N, int d, void *out, int32_t *status,
                                     void *stream) {
  return delta_decode_impl<int32_t>(x, x_dtype, plain_vals, plain_idx, ld_plain, edit_vals, edit_idx, ld_edit, W_dec, T, k, N,
                                    d, out, status, stream);
}

extern "C" int msae_delta_decode_i64_f32(const void *x, int x_dtype, const float *plain_vals, const int64_t *plain_idx,
                                         int ld_plain, const float *edit_vals, const int64_t *edit_idx, int ld_edit,
                                         const float *W_dec, int T, int k, int N, int d, void *out, int32_t *status,
                                         void *stream) {
  return delta_decode_impl<int64_t>(x, x_dtype, plain_vals, plain_idx, ld_plain, edit_vals, edit_idx, ld_edit, W_dec, T, k, N,
                                    d, out, status, stream);
}
