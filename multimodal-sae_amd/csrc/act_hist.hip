// act_hist.hip -- per-feature histograms of activation strength, updated from the cache loop's top-k, and the quantile
// bins read from them (include/msae.h: msae_act_hist_*).
//
// The BIN of a value c > 0 is a function of its float32 bits alone (ah_bin): 2^sub_bits bins per octave from 2^e_lo up,
// both ends clamped.  A SEGMENT VALUE is a kept entry itself (token mode: |v| > thresh, 0 <= index < N, fs_keys_kernel's
// rule) or the pooled candidate the feature statistics rank (window / image mode: fs_group_kernel's value, bit for bit);
// it is counted iff it is > 0:
//   hist[f][bin(c)] += 1                                                                               int32 atomics
// Integer adds commute: the state is the same bits whatever the order of the adds, the cut into calls or their order.
//
// Token mode (ah_token_kernel): no sort.  A workgroup takes AH_TOK_ENTRIES consecutive entries (32 tokens at k = 32), one
// lane per entry and round, and first counts its (feature, bin) pairs in an LDS table (open addressing, at most half full);
// then every used slot issues ONE global atomic.  A feature that fires on every token with one value costs T * k /
// AH_TOK_ENTRIES adds on its address instead of T.  Measured at T = 8192, k = 32, N = 131072 (kernel alone): one atomic per
// entry 0.014 ms on lists without a repeat but 0.101 ms with one such feature; combining equal pairs inside a wave -- a wave
// holds 64 / k tokens, and a token names a feature once, so at most 64 / k of them meet -- 0.016 / 0.059 ms; the table
// 0.017 / 0.017 ms.
// Window / image mode: feature_stats.hip's pipeline, restated.
//   1. ah_keys_kernel    every kept entry -> key (feature << tb | t) with its value; dropped entries get feature = N.
//   2. rocPRIM radix sort (pairs) over the used key bits: grouped by feature, inside a feature in token order; the sort
//                        is stable, so a caller's repeat of (token, feature) keeps its list order, as it does there.
//   3. ah_group_kernel   the thread on a group's first entry walks it in ascending position, forms the pooled value in
//                        fs_group_kernel's order of operations and issues one atomic for the group.
//
// ah_quantile_kernel: one wave per feature (grid-stride).  Lane l holds bins [l * per, (l + 1) * per), per = ceil(n_bins / 64)
// <= 8, in registers; a wave prefix scan of the lane totals gives every lane its running count; per probability the first
// lane whose inclusive count reaches the rank finds the bin among its own.
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "wave_ops.h"

namespace {

constexpr int AH_MAX_K = 256, AH_MAX_N = 262144, AH_MAX_BINS = 512, AH_MAX_Q = 64;
constexpr int AH_PER_LANE = AH_MAX_BINS / 64;

struct AhBins {      // the bin rule: raw = (bits >> shift) - base, clamped to [0, n_bins)
  int shift, base, n_bins;
};

__device__ __forceinline__ int ah_bin(float c, const AhBins &b) {      // c > 0 (the sign bit is clear)
  const int raw = (int)(__float_as_uint(c) >> b.shift) - b.base;
  return raw < 0 ? 0 : raw >= b.n_bins ? b.n_bins - 1 : raw;
}

__device__ __forceinline__ bool ah_keep(float v, int f, float thresh, int N) {
  return fabsf(v) > thresh && (unsigned)f < (unsigned)N;
}

// ---- token mode ------------------------------------------------------------------------------------------------------
constexpr int AH_TOK_ENTRIES = 1024;                 // entries per workgroup
constexpr int AH_TOK_SLOTS = 2 * AH_TOK_ENTRIES;     // table slots: a power of two, never more than half full
constexpr int AH_TOK_SLOT_BITS = 11;
static_assert(1 << AH_TOK_SLOT_BITS == AH_TOK_SLOTS && AH_TOK_ENTRIES % 256 == 0, "table size");

__global__ __launch_bounds__(256) void ah_token_kernel(const float *__restrict__ vals, const int32_t *__restrict__ idx,
                                                       long M, float thresh, int N, AhBins bins, int *__restrict__ hist) {
  __shared__ int s_key[AH_TOK_SLOTS];               // f * n_bins + bin (< 2^27), -1 = free
  __shared__ int s_cnt[AH_TOK_SLOTS];
  for (int s = threadIdx.x; s < AH_TOK_SLOTS; s += 256) {
    s_key[s] = -1;
    s_cnt[s] = 0;
  }
  __syncthreads();
  const long base = (long)blockIdx.x * AH_TOK_ENTRIES;
  for (int e = 0; e < AH_TOK_ENTRIES; e += 256) {
    const long i = base + e + threadIdx.x;
    if (i >= M) break;
    const float v = vals[i];
    const int f = idx[i];
    if (ah_keep(v, f, thresh, N) && v > 0.f) {
      const int key = f * bins.n_bins + ah_bin(v, bins);
      unsigned slot = ((unsigned)key * 2654435761u) >> (32 - AH_TOK_SLOT_BITS);
      for (;;) {                                    // linear probing; a free slot exists: <= AH_TOK_ENTRIES keys
        const int prev = atomicCAS(&s_key[slot], -1, key);
        if (prev == -1 || prev == key) break;
        slot = (slot + 1) & (AH_TOK_SLOTS - 1);
      }
      atomicAdd(&s_cnt[slot], 1);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < AH_TOK_SLOTS; s += 256) {
    const int c = s_cnt[s];
    if (c) atomicAdd(hist + s_key[s], c);
  }
}

// ---- window / image mode ---------------------------------------------------------------------------------------------
struct AhGeom {      // where token t = b*S + s belongs (FsGeom without the ids)
  int S, mode, P, W, nw, tb;
};

__device__ __forceinline__ int ah_group(const AhGeom &g, int s) { return g.mode == MSAE_POOL_WINDOW ? s / g.W : 0; }

__global__ __launch_bounds__(256) void ah_keys_kernel(const float *__restrict__ vals, const int32_t *__restrict__ idx,
                                                      long M, int k, float thresh, int N, int tb,
                                                      unsigned long long *__restrict__ keys, float *__restrict__ kv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const float v = vals[i];
  const int f = idx[i];
  const unsigned long long t = (unsigned long long)(i / k);
  keys[i] = ((unsigned long long)(ah_keep(v, f, thresh, N) ? f : N) << tb) | t;
  kv[i] = v;
}

// one thread per sorted entry; the thread on a group's first entry walks the group (fs_group_kernel's walk and arithmetic)
__global__ __launch_bounds__(256) void ah_group_kernel(const unsigned long long *__restrict__ keys,
                                                       const float *__restrict__ kv, long M, int N, AhGeom g, AhBins bins,
                                                       int *__restrict__ hist) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const unsigned long long tmask = (1ull << g.tb) - 1ull;
  const unsigned long long key = keys[i];
  const int f = (int)(key >> g.tb);
  if (f >= N) return;                               // dropped entries: sorted behind every kept one
  const int t = (int)(key & tmask), b = t / g.S, s = t - b * g.S, grp = ah_group(g, s);
  if (i > 0 && (int)(keys[i - 1] >> g.tb) == f) {
    const int pt = (int)(keys[i - 1] & tmask), pb = pt / g.S;
    if (pb == b && ah_group(g, pt - pb * g.S) == grp) return;      // not the group's first entry
  }
  if (g.mode == MSAE_POOL_WINDOW && grp >= g.nw) return;           // the ragged tail is not pooled
  int cnt = 0, pooled_n = 0;
  float pool = 0.f;                                 // window: max; image: f32 sum in ascending s
  for (long j = i; j < M; ++j) {
    const unsigned long long kj = keys[j];
    if ((int)(kj >> g.tb) != f) break;
    const int tj = (int)(kj & tmask), bj = tj / g.S, sj = tj - bj * g.S;
    if (bj != b || ah_group(g, sj) != grp) break;
    const float v = kv[j];
    ++cnt;
    if (g.mode == MSAE_POOL_WINDOW) {
      pool = pooled_n ? fmaxf(pool, v) : v;
      ++pooled_n;
    } else if (sj < g.P) {
      pool += v;
      ++pooled_n;
    }
  }
  float c = 0.f;
  if (g.mode == MSAE_POOL_WINDOW) {
    c = cnt < g.W ? fmaxf(pool, 0.f) : pool;        // a window with a position the feature did not fire on also holds a 0
  } else if (pooled_n) {
    c = pool / (float)g.P;
  }
  if (c > 0.f) atomicAdd(hist + (size_t)f * bins.n_bins + ah_bin(c, bins), 1);      // NaN, 0 and negatives: nowhere
}

// ---- quantiles -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ah_quantile_kernel(const int *__restrict__ hist, int N, int n_bins,
                                                          const double *__restrict__ qs, int Q, long long n_segments,
                                                          int zeros, int *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), waves = (int)(gridDim.x * 4u);
  const int per = (n_bins + 63) >> 6, b0 = lane * per;
  const double q = lane < Q ? qs[lane] : 0.0;
  for (int f = wave; f < N; f += waves) {
    const int *row = hist + (size_t)f * n_bins;
    int c[AH_PER_LANE];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < AH_PER_LANE; ++j) {
      c[j] = (j < per && b0 + j < n_bins) ? row[b0 + j] : 0;
      mine += c[j];
    }
    const long long incl = wave_incl_scan(mine, lane);
    const long long n = __shfl(incl, 63, 64);
    const long long z = (zeros && n_segments > n) ? n_segments - n : 0;
    const long long tot = n + z;
    // this lane's probability -> rank: one f64 multiply, ceil, clamp to [1, tot]
    long long r = (long long)ceil(q * (double)tot);
    r = r < 1 ? 1 : r > tot ? tot : r;
    for (int i = 0; i < Q; ++i) {
      const long long ri = __shfl(r, i, 64);
      int res;
      if (tot == 0) {
        res = -2;
      } else if (ri <= z) {
        res = -1;
      } else {
        const unsigned long long hit = __ballot(incl + z >= ri);   // lane 63 always hits: ri <= tot
        const int src = __builtin_ctzll(hit);
        long long run = incl - mine + z;
        int bin = b0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < AH_PER_LANE; ++j) {
          run += c[j];
          if (!found && run >= ri) { bin = b0 + j; found = true; }
        }
        res = __shfl(bin, src, 64);
      }
      if (lane == 0) out[(size_t)f * Q + i] = res;
    }
  }
}

int ah_bit_width(unsigned long long v) { return v ? 64 - __builtin_clzll(v) : 0; }

struct AhLayout {
  size_t keys0, keys1, vals0, vals1, sort, total;
};

size_t ah_sort_bound(long M) { return (size_t)M * 8 + (1u << 20); }

AhLayout ah_layout(long M) {
  AhLayout L;
  size_t o = 0;
  auto take = [&](size_t b) { size_t r = o; o = msae_align_up(o + b, 256); return r; };
  L.keys0 = take((size_t)M * 8);
  L.keys1 = take((size_t)M * 8);
  L.vals0 = take((size_t)M * 4);
  L.vals1 = take((size_t)M * 4);
  L.sort = take(ah_sort_bound(M));
  L.total = o;
  return L;
}

bool ah_shape_ok(int T, int k, int N) {
  return T >= 0 && T <= MSAE_STATS_MAX_T && k > 0 && k <= AH_MAX_K && N > 0 && N <= AH_MAX_N;
}

// sub_bits in [0, 4], 127 + e_lo in [1, 254], e_lo + octaves <= 128 (the top edge is at most +inf), 1 <= n_bins <= 512
bool ah_bins_ok(int sub_bits, int e_lo, int octaves, AhBins *out) {
  if (sub_bits < 0 || sub_bits > 4 || e_lo < -126 || e_lo > 127 || octaves < 1 || e_lo + octaves > 128) return false;
  const int n_bins = octaves << sub_bits;
  if (n_bins > AH_MAX_BINS) return false;
  out->shift = 23 - sub_bits;
  out->base = (127 + e_lo) << sub_bits;
  out->n_bins = n_bins;
  return true;
}

}  // namespace

extern "C" size_t msae_act_hist_ws_bytes(int T, int k, int N) {
  if (!ah_shape_ok(T, k, N)) return 0;
  return ah_layout((long)T * k).total;
}

extern "C" int msae_act_hist_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N,
                                    int mode, int pool_len, int window, int sub_bits, int e_lo, int octaves,
                                    int32_t *hist, void *ws, size_t ws_bytes, void *stream) {
  if (B < 0 || S < 0 || (B > 0 && S > MSAE_STATS_MAX_T / B)) return MSAE_EINVAL;
  const int T = B * S;
  AhBins bins;
  if (!ah_shape_ok(T, k, N) || !ah_bins_ok(sub_bits, e_lo, octaves, &bins)) return MSAE_EINVAL;
  if (mode == MSAE_POOL_IMAGE) {
    if (pool_len <= 0 || pool_len > 2880) return MSAE_EINVAL;
  } else if (mode == MSAE_POOL_WINDOW) {
    if (window <= 0 || window > 4096) return MSAE_EINVAL;
  } else if (mode != MSAE_POOL_TOKEN) {
    return MSAE_EINVAL;
  }
  if (T == 0) return 0;
  if (!vals || !idx || !hist) return MSAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long M = (long)T * k;
  const unsigned blocks = (unsigned)((M + 255) / 256);
  if (mode == MSAE_POOL_TOKEN) {
    const unsigned tblocks = (unsigned)((M + AH_TOK_ENTRIES - 1) / AH_TOK_ENTRIES);
    hipLaunchKernelGGL(ah_token_kernel, dim3(tblocks), dim3(256), 0, st, vals, idx, M, thresh, N, bins, hist);
    return msae_launch_status();
  }
  const AhLayout L = ah_layout(M);
  if (!ws || ws_bytes < L.total) return MSAE_EWS;
  char *w = (char *)ws;
  unsigned long long *k0 = (unsigned long long *)(w + L.keys0), *k1 = (unsigned long long *)(w + L.keys1);
  float *v0 = (float *)(w + L.vals0), *v1 = (float *)(w + L.vals1);
  AhGeom g;
  g.S = S;
  g.mode = mode;
  g.P = pool_len;
  g.W = window;
  g.nw = mode == MSAE_POOL_WINDOW ? S / window : 1;
  g.tb = ah_bit_width((unsigned long long)(T - 1));
  hipLaunchKernelGGL(ah_keys_kernel, dim3(blocks), dim3(256), 0, st, vals, idx, M, k, thresh, N, g.tb, k0, v0);
  rocprim::double_buffer<unsigned long long> kb(k0, k1);
  rocprim::double_buffer<float> vb(v0, v1);
  const unsigned end_bit = (unsigned)(g.tb + ah_bit_width((unsigned long long)N));
  size_t sort_bytes = 0;
  MSAE_HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, kb, vb, (size_t)M, 0u, end_bit, st));
  if (sort_bytes > ah_sort_bound(M)) return MSAE_EWS;
  MSAE_HIP_TRY(rocprim::radix_sort_pairs((void *)(w + L.sort), sort_bytes, kb, vb, (size_t)M, 0u, end_bit, st));
  hipLaunchKernelGGL(ah_group_kernel, dim3(blocks), dim3(256), 0, st, kb.current(), vb.current(), M, N, g, bins, hist);
  return msae_launch_status();
}

extern "C" int msae_act_hist_quantiles(const int32_t *hist, int N, int n_bins, const double *qs, int Q,
                                       int64_t n_segments, int zeros, int32_t *bins, void *stream) {
  if (N <= 0 || N > AH_MAX_N || n_bins < 1 || n_bins > AH_MAX_BINS || Q < 1 || Q > AH_MAX_Q || n_segments < 0)
    return MSAE_EINVAL;
  if (!hist || !qs || !bins) return MSAE_EINVAL;
  const unsigned need = (unsigned)((N + 3) / 4);
  hipLaunchKernelGGL(ah_quantile_kernel, dim3(need < 4096u ? need : 4096u), dim3(256), 0, (hipStream_t)stream, hist, N,
                     n_bins, qs, Q, (long long)n_segments, zeros, bins);
  return msae_launch_status();
}
