// act_hist.hip -- per-feature histograms of activation strength, updated from the cache loop's top-k, and the quantile
// bins read from them (include/msae.h: msae_act_hist_*).
//
// The BIN of a value c > 0 is a function of its float32 bits alone (ah_bin): 2^sub_bits bins per octave from 2^e_lo up,
// both ends clamped.  A SEGMENT VALUE is a kept entry itself (token mode: |v| > thresh, 0 <= index < N, pool_keep) or the
// pooled candidate the feature statistics rank (window / image mode: pool_walk_run's value, the one copy of that arithmetic,
// in pool_segments.h); it is counted iff it is > 0:
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
// Window / image mode: feature_stats.hip's pipeline through the same code (pool_segments.h).
//   1. pool_keys_kernel  every kept entry -> key (feature << tb | t) with its value; dropped entries get feature = N.
//   2. pool_sort         rocPRIM radix sort (pairs) over the used key bits: grouped by feature, inside a feature in token
//                        order; the sort is stable, so a caller's repeat of (token, feature) keeps its list order.
//   3. ah_group_kernel   the thread on a group's first entry walks it (pool_walk_run) and issues one atomic for the group.
//
// ah_quantile_kernel: one wave per feature (grid-stride).  Lane l holds bins [l * per, (l + 1) * per), per = ceil(n_bins / 64)
// <= 8, in registers; a wave prefix scan of the lane totals gives every lane its running count; per probability the first
// lane whose inclusive count reaches the rank finds the bin among its own.
#include "pool_segments.h"
#include "wave_ops.h"

namespace {

constexpr int AH_MAX_BINS = 512, AH_MAX_Q = 64;
constexpr int AH_PER_LANE = AH_MAX_BINS / 64;

struct AhBins {      // the bin rule: raw = (bits >> shift) - base, clamped to [0, n_bins)
  int shift, base, n_bins;
};

__device__ __forceinline__ int ah_bin(float c, const AhBins &b) {      // c > 0 (the sign bit is clear)
  const int raw = (int)(__float_as_uint(c) >> b.shift) - b.base;
  return raw < 0 ? 0 : raw >= b.n_bins ? b.n_bins - 1 : raw;
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
    if (pool_keep(v, f, thresh, N) && v > 0.f) {
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
// one thread per sorted entry; the thread on a group's first entry walks the group
__global__ __launch_bounds__(256) void ah_group_kernel(const unsigned long long *__restrict__ keys,
                                                       const float *__restrict__ kv, long M, int N, PoolGeom g, AhBins bins,
                                                       int *__restrict__ hist) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const PoolEntry e = pool_entry(keys[i], g);
  if (e.f >= N) return;                             // dropped entries: sorted behind every kept one
  if (!pool_run_head(keys, i, e, g)) return;
  if (g.mode == MSAE_POOL_WINDOW && e.grp >= g.nw) return;         // the ragged tail is not pooled
  const float c = pool_walk_run<false>(keys, kv, M, i, e, g).cand;
  if (c > 0.f) atomicAdd(hist + (size_t)e.f * bins.n_bins + ah_bin(c, bins), 1);    // NaN, 0 and negatives: nowhere
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
  if (!pool_shape_ok(T, k, N)) return 0;
  return pool_layout((long)T * k, true, 0).total;
}

extern "C" int msae_act_hist_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N,
                                    int mode, int pool_len, int window, int sub_bits, int e_lo, int octaves,
                                    int32_t *hist, void *ws, size_t ws_bytes, void *stream) {
  int T;
  AhBins bins;
  if (!pool_tokens(B, S, &T) || !pool_shape_ok(T, k, N) || !ah_bins_ok(sub_bits, e_lo, octaves, &bins)) return MSAE_EINVAL;
  if (!pool_mode_ok(mode, pool_len, window, true)) return MSAE_EINVAL;
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
  const PoolLayout L = pool_layout(M, true, 0);
  if (!ws || ws_bytes < L.total) return MSAE_EWS;
  char *w = (char *)ws;
  const PoolGeom g = pool_geom(T, S, mode, pool_len, window);
  hipLaunchKernelGGL(pool_keys_kernel, dim3(blocks), dim3(256), 0, st, vals, idx, M, k, thresh, N, g.tb,
                     (unsigned long long *)(w + L.keys0), (float *)(w + L.vals0));
  PoolSorted sorted;
  const unsigned end_bit = (unsigned)(g.tb + pool_bit_width((unsigned long long)N));
  if (const int rc = pool_sort(w, L, M, end_bit, true, st, &sorted)) return rc;
  hipLaunchKernelGGL(ah_group_kernel, dim3(blocks), dim3(256), 0, st, sorted.keys, sorted.vals, M, N, g, bins, hist);
  return msae_launch_status();
}

extern "C" int msae_act_hist_quantiles(const int32_t *hist, int N, int n_bins, const double *qs, int Q,
                                       int64_t n_segments, int zeros, int32_t *bins, void *stream) {
  if (N <= 0 || N > POOL_MAX_N || n_bins < 1 || n_bins > AH_MAX_BINS || Q < 1 || Q > AH_MAX_Q || n_segments < 0)
    return MSAE_EINVAL;
  if (!hist || !qs || !bins) return MSAE_EINVAL;
  const unsigned need = (unsigned)((N + 3) / 4);
  hipLaunchKernelGGL(ah_quantile_kernel, dim3(need < 4096u ? need : 4096u), dim3(256), 0, (hipStream_t)stream, hist, N,
                     n_bins, qs, Q, (long long)n_segments, zeros, bins);
  return msae_launch_status();
}
