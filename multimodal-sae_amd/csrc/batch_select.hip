// batch_select.hip -- capped BatchTopK on top-C lists (include/msae.h, "batch-level selection").
//
//   msae_batch_kth_f32     theta = the K-th largest positive value of a [T, C] list: an exact radix select on the float bits,
//                          four 8-bit passes, integer histograms only (bit-reproducible), one launch per pass.
//   msae_list_filter_f32   keep v > 0 && v >= theta (or theta_feat[idx]): stable partition of every row, lengths, saturation.
//   msae_decode_prefix_f32 decode.hip's forward with a row length: the slots behind len[a] are never read.
//
// Nothing here hands data between the workgroups of one launch: a pass's 256-bin histogram is complete when its launch ends,
// and every workgroup of the NEXT launch redoes the (tiny) digit picks from the global histograms.  No flag, no spin.
#include "common.h"
#include "sortsel.h"
#include "wave_ops.h"

namespace {

constexpr int KTH_THREADS = 256;          // = the 256 bins of a pass: thread t owns bin 255 - t in the picks
constexpr int KTH_MAX_BLOCKS = 1024;
constexpr long KTH_MAX_VALUES = 1l << 24;

struct KthLds {
  unsigned hist[256];
  unsigned wave_tot[4];
  unsigned pick[2];                        // the chosen digit, the rank left inside its bin
};

// The digit pick of one pass: hist = that pass's 256 global bins (complete: written by an earlier launch), r = the 1-based
// rank (from the top) wanted among the values counted there, 1 <= r <= their number.  Returns the digit whose bin holds that
// rank and leaves the rank inside the bin in r.  All 256 threads call; barriers inside (block_excl_scan's two in front of
// the write of pick[], one behind it: calls may follow each other).
__device__ __forceinline__ unsigned kth_pick_digit(const unsigned *__restrict__ hist, unsigned &r, KthLds &s) {
  const int tid = threadIdx.x;
  const unsigned h = hist[255 - tid];      // descending digit order: the scan counts the values above the thread's bin
  unsigned tot;
  const unsigned above = block_excl_scan<4>(h, s.wave_tot, &tot);
  if (above < r && r <= above + h) { s.pick[0] = 255u - tid; s.pick[1] = r - above; }
  __syncthreads();
  r = s.pick[1];
  return s.pick[0];
}

// |P| and the picks of the passes [0, passes): -> the prefix they fix (passes * 8 bits) and the rank left, false when P is empty
__device__ __forceinline__ bool kth_prefix(const unsigned *__restrict__ hist, long long K, int passes, KthLds &s, unsigned &prefix,
                                           unsigned &r, unsigned &n_pos) {
  if (threadIdx.x == 0) { s.pick[0] = 0u; s.pick[1] = 1u; }      // (published by the scan's barriers; never read unwritten)
  unsigned tot;
  block_excl_scan<4>(hist[threadIdx.x], s.wave_tot, &tot);
  n_pos = tot;
  prefix = 0u;
  if (tot == 0u) return false;                                   // uniform: every thread holds the same total
  r = K < (long long)tot ? (unsigned)K : tot;                    // |P| < K: the smallest member of P
  for (int q = 0; q < passes; ++q) prefix = (prefix << 8) | kth_pick_digit(hist + 256 * q, r, s);
  return true;
}

__device__ __forceinline__ void kth_count(float v, int pass, unsigned prefix, unsigned *hist) {
  const unsigned b = __float_as_uint(v);
  const int shift = 24 - 8 * pass;
  if (v > 0.f && (pass == 0 || (b >> (shift + 8)) == prefix)) atomicAdd(hist + ((b >> shift) & 255u), 1u);
}

// pass p of the select: the histogram of byte 3 - p over the positive values whose higher bytes equal the picks so far.
// A positive float's bits order like the value (+inf above every finite one; NaN fails v > 0), so no key transform is needed.
__global__ __launch_bounds__(KTH_THREADS) void kth_hist_kernel(const float *__restrict__ vals, int T, int C, size_t ld,
                                                               long long K, unsigned *__restrict__ hist, int pass, int vec4) {
  __shared__ KthLds s;
  const int tid = threadIdx.x;
  unsigned prefix = 0u, r = 0u, n_pos = 0u;
  if (pass > 0 && !kth_prefix(hist, K, pass, s, prefix, r, n_pos)) return;
  s.hist[tid] = 0u;
  __syncthreads();
  const long n = (long)T * C;
  const long stride = (long)gridDim.x * KTH_THREADS;
  if (vec4) {                                // ld == C, 16-byte aligned: the list is one flat array
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * KTH_THREADS + tid; i < n4; i += stride) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(vals + 4 * i);
      kth_count(v[0], pass, prefix, s.hist); kth_count(v[1], pass, prefix, s.hist);
      kth_count(v[2], pass, prefix, s.hist); kth_count(v[3], pass, prefix, s.hist);
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) kth_count(vals[4 * n4 + tid], pass, prefix, s.hist);
  } else {
    for (long i = (long)blockIdx.x * KTH_THREADS + tid; i < n; i += stride)
      kth_count(vals[(size_t)(i / C) * ld + (size_t)(i % C)], pass, prefix, s.hist);
  }
  __syncthreads();
  const unsigned c = s.hist[tid];
  if (c) atomicAdd(hist + 256 * pass + tid, c);                  // one integer atomic per bin and workgroup
}

__global__ __launch_bounds__(KTH_THREADS) void kth_zero_kernel(unsigned *__restrict__ hist) {
  hist[blockIdx.x * KTH_THREADS + threadIdx.x] = 0u;
}

__global__ __launch_bounds__(KTH_THREADS) void kth_final_kernel(const unsigned *__restrict__ hist, long long K,
                                                                float *__restrict__ theta, int32_t *__restrict__ n_pos_out) {
  __shared__ KthLds s;
  unsigned prefix, r, n_pos;
  const bool any = kth_prefix(hist, K, 4, s, prefix, r, n_pos);
  if (threadIdx.x == 0) {
    *theta = any ? __uint_as_float(prefix) : __uint_as_float(0x7F800000u);   // P empty: +inf keeps nothing
    if (n_pos_out) *n_pos_out = (int32_t)n_pos;
  }
}

// ---- list filter ------------------------------------------------------------------------------------------------------------
constexpr int FILTER_WAVE_C = 256;         // rows up to here: one wave per token, the row in 4 registers per lane
constexpr int FILTER_MAX_C = 4096;

template <typename IT>
__device__ __forceinline__ bool filter_keep(float v, IT ix, float th, const float *__restrict__ theta_feat, int N) {
  if (!(v > 0.f)) return false;            // NaN, -0.0, negatives
  if (!theta_feat) return v >= th;
  if (ix < 0 || ix >= (IT)N) return false; // the table is never read out of bounds
  return v >= theta_feat[(int)ix];
}

// One wave per token.  Slot i = j * 64 + lane sits in key[j] as (value bits << 32 | keep << 31 | i + 1); 0 = behind the row.
// Two ballot compactions (sortsel.h): the kept entries to the front in list order, the dropped ones behind them in theirs.
template <typename IT>
__global__ __launch_bounds__(256) void list_filter_wave_kernel(const float *__restrict__ vals_in, const IT *__restrict__ idx_in,
                                                               int T, int C, size_t ld, const float *__restrict__ theta,
                                                               const float *__restrict__ theta_feat, int N,
                                                               float *__restrict__ vals_out, IT *__restrict__ idx_out,
                                                               int32_t *__restrict__ len, int32_t *__restrict__ n_saturated) {
  constexpr int PK = FILTER_WAVE_C / 64;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;                      // wave-uniform
  const float th = *theta;
  const float *vp = vals_in + (size_t)t * ld;
  const IT *ip = idx_in + (size_t)t * ld;
  float *vo = vals_out + (size_t)t * C;
  IT *io = idx_out + (size_t)t * C;
  const int nj = (C + 63) >> 6;
  unsigned long long key[PK];
#pragma unroll
  for (int j = 0; j < PK; ++j) {
    const int i = j * 64 + lane;
    key[j] = 0ull;
    if (j < nj && i < C) {
      const float v = vp[i];
      const bool keep = filter_keep<IT>(v, theta_feat ? ip[i] : (IT)0, th, theta_feat, N);
      key[j] = ((unsigned long long)__float_as_uint(v) << 32) | (keep ? 0x80000000u : 0u) | (unsigned)(i + 1);
    }
  }
  const auto slot = [](unsigned long long k) { return (int)((unsigned)k & 0x7FFFFFFFu) - 1; };
  const int kept = wave_compact_if<PK>(
      key, nj, lane, [](unsigned long long k) { return ((unsigned)k >> 31) != 0u; },
      [&](unsigned long long k, bool take, int pos) {
        if (take) { vo[pos] = __uint_as_float((unsigned)(k >> 32)); io[pos] = ip[slot(k)]; }
      });
  wave_compact_if<PK>(
      key, nj, lane, [](unsigned long long k) { return k != 0ull && ((unsigned)k >> 31) == 0u; },
      [&](unsigned long long k, bool take, int pos) {
        if (take) { vo[kept + pos] = 0.f; io[kept + pos] = ip[slot(k)]; }
      });
  if (lane == 0) {
    len[t] = kept;
    const float last = vp[C - 1];
    if (n_saturated && last > 0.f && last >= th) atomicAdd(n_saturated, 1);
  }
}

// One workgroup per token, rows up to 4096: chunks of 256 slots in list order, a workgroup scan of the keep flags per chunk.
template <typename IT>
__global__ __launch_bounds__(256) void list_filter_wg_kernel(const float *__restrict__ vals_in, const IT *__restrict__ idx_in,
                                                             int C, size_t ld, const float *__restrict__ theta,
                                                             const float *__restrict__ theta_feat, int N,
                                                             float *__restrict__ vals_out, IT *__restrict__ idx_out,
                                                             int32_t *__restrict__ len, int32_t *__restrict__ n_saturated) {
  __shared__ int wave_tot[4];
  const int t = blockIdx.x, tid = threadIdx.x;
  const float th = *theta;
  const float *vp = vals_in + (size_t)t * ld;
  const IT *ip = idx_in + (size_t)t * ld;
  float *vo = vals_out + (size_t)t * C;
  IT *io = idx_out + (size_t)t * C;
  int mine = 0;
  for (int i = tid; i < C; i += 256) mine += filter_keep<IT>(vp[i], theta_feat ? ip[i] : (IT)0, th, theta_feat, N) ? 1 : 0;
  int kept;
  block_excl_scan<4>(mine, wave_tot, &kept);
  int kbase = 0, dbase = kept;
  for (int c0 = 0; c0 < C; c0 += 256) {    // uniform trip count: the scan's barriers are met by every thread
    const int i = c0 + tid;
    const bool valid = i < C;
    const float v = valid ? vp[i] : 0.f;
    const IT ix = valid ? ip[i] : (IT)0;
    const bool keep = valid && filter_keep<IT>(v, ix, th, theta_feat, N);
    int tot;
    const int before = block_excl_scan<4>(keep ? 1 : 0, wave_tot, &tot);
    if (valid) {
      const int pos = keep ? kbase + before : dbase + (tid - before);
      vo[pos] = keep ? v : 0.f;
      io[pos] = ix;
    }
    const int n_valid = C - c0 < 256 ? C - c0 : 256;
    kbase += tot;
    dbase += n_valid - tot;
  }
  if (tid == 0) {
    len[t] = kept;
    const float last = vp[C - 1];
    if (n_saturated && last > 0.f && last >= th) atomicAdd(n_saturated, 1);
  }
}

// ---- decode with a row length -----------------------------------------------------------------------------------------------
// decode.hip's two forward kernels (same column slabs, same unroll, same fma chain in j order) with the loop bound
// clamp(len[a], 0, k) in place of k: index, activation and decoder row of a slot behind it are not touched.
constexpr int DEC_THREADS = 256;
constexpr int DEC_UNROLL = 8;

__device__ __forceinline__ int prefix_len(const int32_t *__restrict__ len, int a, int k) {
  const int l = len[a];
  return l < 0 ? 0 : (l > k ? k : l);
}

// grid: (A, ceil(d / 1024))
template <typename IT>
__global__ __launch_bounds__(DEC_THREADS) void decode_prefix_v4_kernel(
    const IT *__restrict__ idx, const float *__restrict__ acts, const int32_t *__restrict__ len,
    const float *__restrict__ W_dec, const float *__restrict__ b_dec, float *__restrict__ out,
    int k, int N, int d, int32_t *status) {
  const int a = blockIdx.x;
  const int col = (blockIdx.y * DEC_THREADS + threadIdx.x) * 4;
  const IT *ip = idx + (size_t)a * k;
  const float *vp = acts + (size_t)a * k;
  if (col >= d) return;
  const int L = prefix_len(len, a, k);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int j = 0;
  for (; j + DEC_UNROLL <= L; j += DEC_UNROLL) {
    f32x4 w[DEC_UNROLL];
    float v[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      const IT iw = ip[j + u];
      int i = (int)iw;
      v[u] = vp[j + u];
      const bool bad = iw < 0 || iw >= (IT)N;
      if (bad) {
        v[u] = 0.f;
        i = 0;
        if (status && threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, 1);
      }
      w[u] = *reinterpret_cast<const f32x4 *>(W_dec + (size_t)i * d + col);
    }
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      f32x4 f;
      f[0] = __builtin_fmaf(v[u], w[u][0], acc[0]);
      f[1] = __builtin_fmaf(v[u], w[u][1], acc[1]);
      f[2] = __builtin_fmaf(v[u], w[u][2], acc[2]);
      f[3] = __builtin_fmaf(v[u], w[u][3], acc[3]);
      acc = (v[u] == 0.f) ? acc : f;
    }
  }
  for (; j < L; ++j) {
    const IT iw = ip[j];
    int i = (int)iw;
    float v = vp[j];
    if (iw < 0 || iw >= (IT)N) {
      v = 0.f;
      i = 0;
      if (status && threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, 1);
    }
    f32x4 w = *reinterpret_cast<const f32x4 *>(W_dec + (size_t)i * d + col);
    f32x4 f;
    f[0] = __builtin_fmaf(v, w[0], acc[0]);
    f[1] = __builtin_fmaf(v, w[1], acc[1]);
    f[2] = __builtin_fmaf(v, w[2], acc[2]);
    f[3] = __builtin_fmaf(v, w[3], acc[3]);
    acc = (v == 0.f) ? acc : f;
  }
  if (b_dec) {
    f32x4 b = *reinterpret_cast<const f32x4 *>(b_dec + col);
    acc[0] += b[0]; acc[1] += b[1]; acc[2] += b[2]; acc[3] += b[3];
  }
  *reinterpret_cast<f32x4 *>(out + (size_t)a * d + col) = acc;
}

// any d / alignment: one column per lane.  grid: (A, ceil(d / 256))
template <typename IT>
__global__ __launch_bounds__(DEC_THREADS) void decode_prefix_scalar_kernel(
    const IT *__restrict__ idx, const float *__restrict__ acts, const int32_t *__restrict__ len,
    const float *__restrict__ W_dec, const float *__restrict__ b_dec, float *__restrict__ out,
    int k, int N, int d, int32_t *status) {
  const int a = blockIdx.x;
  const int col = blockIdx.y * DEC_THREADS + threadIdx.x;
  if (col >= d) return;
  const int L = prefix_len(len, a, k);
  float acc = 0.f;
  for (int j = 0; j < L; ++j) {
    const IT iw = idx[(size_t)a * k + j];
    int i = (int)iw;
    float v = acts[(size_t)a * k + j];
    if (iw < 0 || iw >= (IT)N) {
      v = 0.f;
      i = 0;
      if (status && threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, 1);
    }
    float f = __builtin_fmaf(v, W_dec[(size_t)i * d + col], acc);
    acc = (v == 0.f) ? acc : f;
  }
  if (b_dec) acc += b_dec[col];
  out[(size_t)a * d + col] = acc;
}

}  // namespace

extern "C" size_t msae_batch_kth_ws_bytes(int T, int C) {
  if (T < 1 || C < 1 || (long)T * C > KTH_MAX_VALUES) return 0;
  return 4 * 256 * sizeof(unsigned);       // one 256-bin histogram per pass
}

extern "C" int msae_batch_kth_f32(const float *vals, int T, int C, int ld, long long K, float *theta, int32_t *n_pos,
                                  void *ws, size_t ws_bytes, void *stream) {
  if (T < 1 || C < 1 || (long)T * C > KTH_MAX_VALUES || ld < C || K < 1 || !vals || !theta) return MSAE_EINVAL;
  if (!ws || ws_bytes < msae_batch_kth_ws_bytes(T, C)) return MSAE_EWS;
  if (!msae_aligned(ws, 4) || !msae_aligned(vals, 4)) return MSAE_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  unsigned *hist = reinterpret_cast<unsigned *>(ws);
  const long n = (long)T * C;
  const int vec4 = (ld == C && msae_aligned(vals, 16)) ? 1 : 0;
  const long work = vec4 ? (n + 3) / 4 : n;
  long blocks = (work + KTH_THREADS - 1) / KTH_THREADS;
  if (blocks > KTH_MAX_BLOCKS) blocks = KTH_MAX_BLOCKS;
  hipLaunchKernelGGL(kth_zero_kernel, dim3(4), dim3(KTH_THREADS), 0, s, hist);
  for (int pass = 0; pass < 4; ++pass)
    hipLaunchKernelGGL(kth_hist_kernel, dim3((unsigned)blocks), dim3(KTH_THREADS), 0, s, vals, T, C, (size_t)ld, K, hist, pass,
                       vec4);
  hipLaunchKernelGGL(kth_final_kernel, dim3(1), dim3(KTH_THREADS), 0, s, hist, K, theta, n_pos);
  return msae_launch_status();
}

template <typename IT>
static int list_filter_launch(const float *vals_in, const IT *idx_in, int T, int C, int ld, const float *theta,
                              const float *theta_feat, int N, float *vals_out, IT *idx_out, int32_t *len,
                              int32_t *n_saturated, void *stream) {
  if (T < 0 || C < 1 || C > FILTER_MAX_C || ld < C || !theta || (theta_feat && N < 1)) return MSAE_EINVAL;
  if (T == 0) return 0;
  if (!vals_in || !idx_in || !vals_out || !idx_out || !len) return MSAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (C <= FILTER_WAVE_C)
    hipLaunchKernelGGL(list_filter_wave_kernel<IT>, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, vals_in, idx_in, T, C,
                       (size_t)ld, theta, theta_feat, N, vals_out, idx_out, len, n_saturated);
  else
    hipLaunchKernelGGL(list_filter_wg_kernel<IT>, dim3((unsigned)T), dim3(256), 0, s, vals_in, idx_in, C, (size_t)ld, theta,
                       theta_feat, N, vals_out, idx_out, len, n_saturated);
  return msae_launch_status();
}

extern "C" int msae_list_filter_f32(const float *vals_in, const int32_t *idx_in, int T, int C, int ld, const float *theta,
                                    const float *theta_feat, int N, float *vals_out, int32_t *idx_out, int32_t *len,
                                    int32_t *n_saturated, void *stream) {
  return list_filter_launch<int32_t>(vals_in, idx_in, T, C, ld, theta, theta_feat, N, vals_out, idx_out, len, n_saturated,
                                     stream);
}

extern "C" int msae_list_filter_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int C, int ld, const float *theta,
                                        const float *theta_feat, int N, float *vals_out, int64_t *idx_out, int32_t *len,
                                        int32_t *n_saturated, void *stream) {
  return list_filter_launch<int64_t>(vals_in, idx_in, T, C, ld, theta, theta_feat, N, vals_out, idx_out, len, n_saturated,
                                     stream);
}

template <typename IT>
static int decode_prefix_launch(const IT *idx, const float *acts, const int32_t *len, const float *W_dec, const float *b_dec,
                                int A, int k, int N, int d, float *out, int32_t *status, void *stream) {
  if (A < 0 || k <= 0 || N <= 0 || d <= 0) return MSAE_EINVAL;
  if (A == 0) return 0;
  if (!len) return MSAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (d % 4 == 0) && msae_aligned(W_dec, 16) && msae_aligned(out, 16) &&
                   (!b_dec || msae_aligned(b_dec, 16));
  if (vec) {
    dim3 grid(A, (d + DEC_THREADS * 4 - 1) / (DEC_THREADS * 4));
    hipLaunchKernelGGL(decode_prefix_v4_kernel<IT>, grid, dim3(DEC_THREADS), 0, s, idx, acts, len, W_dec, b_dec,
                       out, k, N, d, status);
  } else {
    dim3 grid(A, (d + DEC_THREADS - 1) / DEC_THREADS);
    hipLaunchKernelGGL(decode_prefix_scalar_kernel<IT>, grid, dim3(DEC_THREADS), 0, s, idx, acts, len, W_dec,
                       b_dec, out, k, N, d, status);
  }
  return msae_launch_status();
}

extern "C" int msae_decode_prefix_f32(const int32_t *idx, const float *acts, const int32_t *len, const float *W_dec,
                                      const float *b_dec, int A, int k, int N, int d, float *out, int32_t *status,
                                      void *stream) {
  return decode_prefix_launch<int32_t>(idx, acts, len, W_dec, b_dec, A, k, N, d, out, status, stream);
}

extern "C" int msae_decode_prefix_i64_f32(const int64_t *idx, const float *acts, const int32_t *len, const float *W_dec,
                                          const float *b_dec, int A, int k, int N, int d, float *out, int32_t *status,
                                          void *stream) {
  return decode_prefix_launch<int64_t>(idx, acts, len, W_dec, b_dec, A, k, N, d, out, status, stream);
}
