// pool_segments.h -- what the cache-loop statistics share (feature_stats.hip, coact.hip, act_hist.hip): the keep rule and the
// limits of a call, the pooling geometry, the feature-major key kernel, the walk over one sorted (feature, row, group) run
// with its pooled candidate, and the sort scratch.  One copy of each: include/msae.h promises that the histograms' window
// and image values are the candidates the feature statistics rank, bit for bit, and pool_walk_run is that promise.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace {

// ---- keep rule and limits ---------------------------------------------------------------------------------------------
constexpr int POOL_MAX_K = 256, POOL_MAX_N = 262144, POOL_MAX_LEN = 2880, POOL_MAX_WINDOW = 4096;

// an entry counts iff |v| > thresh (sparsify_count_kernel's rule, no filter bitmap) and its index names a feature
__device__ __forceinline__ bool pool_keep(float v, int f, float thresh, int N) {
  return fabsf(v) > thresh && (unsigned)f < (unsigned)N;
}

inline bool pool_shape_ok(int T, int k, int N) {
  return T >= 0 && T <= MSAE_STATS_MAX_T && k > 0 && k <= POOL_MAX_K && N > 0 && N <= POOL_MAX_N;
}

inline bool pool_mode_ok(int mode, int pool_len, int window, bool allow_token) {
  if (mode == MSAE_POOL_IMAGE) return pool_len > 0 && pool_len <= POOL_MAX_LEN;
  if (mode == MSAE_POOL_WINDOW) return window > 0 && window <= POOL_MAX_WINDOW;
  return allow_token && mode == MSAE_POOL_TOKEN;
}

// *T = B * S, or false where a size is negative or the product passes MSAE_STATS_MAX_T (no int overflow on the way)
inline bool pool_tokens(int B, int S, int *T) {
  if (B < 0 || S < 0 || (B > 0 && S > MSAE_STATS_MAX_T / B)) return false;
  *T = B * S;
  return true;
}

inline int pool_bit_width(unsigned long long v) { return v ? 64 - __builtin_clzll(v) : 0; }

// ---- geometry ---------------------------------------------------------------------------------------------------------
struct PoolGeom {      // where token t = b*S + s belongs; tb = the bits of t in a feature-major key
  int S, mode, P, W, nw, tb;
  __device__ __forceinline__ int group(int s) const { return mode == MSAE_POOL_WINDOW ? s / W : 0; }
};

inline PoolGeom pool_geom(int T, int S, int mode, int pool_len, int window) {
  return PoolGeom{S, mode, pool_len, window, mode == MSAE_POOL_WINDOW ? S / window : 1,
                  pool_bit_width((unsigned long long)(T - 1))};
}

// ---- feature-major keys -----------------------------------------------------------------------------------------------
// every kept entry -> key (feature << tb | t) with its value; dropped entries get feature = N and sort last
__global__ __launch_bounds__(256) void pool_keys_kernel(const float *__restrict__ vals, const int32_t *__restrict__ idx,
                                                        long M, int k, float thresh, int N, int tb,
                                                        unsigned long long *__restrict__ keys, float *__restrict__ kv) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const float v = vals[i];
  const int f = idx[i];
  const unsigned long long t = (unsigned long long)(i / k);
  keys[i] = ((unsigned long long)(pool_keep(v, f, thresh, N) ? f : N) << tb) | t;
  kv[i] = v;
}

struct PoolEntry {     // a feature-major key taken apart
  int f, b, s, grp;
};

__device__ __forceinline__ int pool_key_feature(unsigned long long key, const PoolGeom &g) { return (int)(key >> g.tb); }

__device__ __forceinline__ PoolEntry pool_entry(unsigned long long key, const PoolGeom &g) {
  const int t = (int)(key & ((1ull << g.tb) - 1ull)), b = t / g.S, s = t - b * g.S;
  return PoolEntry{pool_key_feature(key, g), b, s, g.group(s)};
}

// ---- the walk ---------------------------------------------------------------------------------------------------------
// A RUN is the sorted entries of one feature inside one pooling segment (window mode: [w*W, (w+1)*W) of a row, the ragged
// tail its own group; image mode: the row).  Does sorted entry i (kept, e = pool_entry(keys[i])) head its run?
__device__ __forceinline__ bool pool_run_head(const unsigned long long *__restrict__ keys, long i, const PoolEntry &e,
                                              const PoolGeom &g) {
  if (i == 0 || pool_key_feature(keys[i - 1], g) != e.f) return true;
  const PoolEntry p = pool_entry(keys[i - 1], g);
  return !(p.b == e.b && p.grp == e.grp);
}

struct PoolRun {
  int cnt;             // entries of the run
  float cand;          // the pooled candidate; 0 = none
  float mx;            // STATS only: max and f64 sum of the run's values
  double sum;
};

// Walks the run headed by sorted entry i in ascending position (the sort is stable: a repeated (token, feature) keeps its list
// order).  The candidate:
//   window   the max of the values; a window with a position the feature did not fire on also holds a 0 (max_pool1d over the
//            dense row): cnt < W gives fmaxf(pool, 0).  Groups at or beyond nw (the ragged tail) give none.
//   image    the f32 sum of the values at s < P, added in this order, divided by (float)P (avg_pool1d over the first P
//            positions); none without such a value.
// The order of the operations is the contract (built with -ffp-contract=off); do not reorder.
template <bool STATS>
__device__ __forceinline__ PoolRun pool_walk_run(const unsigned long long *__restrict__ keys, const float *__restrict__ kv,
                                                 long M, long i, const PoolEntry &e, const PoolGeom &g) {
  PoolRun r;
  r.cnt = 0;
  r.mx = -INFINITY;
  r.sum = 0.0;
  int pooled_n = 0;
  float pool = 0.f;                                 // window: max; image: f32 sum in ascending s
  for (long j = i; j < M; ++j) {
    const unsigned long long kj = keys[j];
    if (pool_key_feature(kj, g) != e.f) break;
    const PoolEntry x = pool_entry(kj, g);
    if (x.b != e.b || x.grp != e.grp) break;
    const float v = kv[j];
    ++r.cnt;
    if constexpr (STATS) {
      r.mx = fmaxf(r.mx, v);
      r.sum += (double)v;
    }
    if (g.mode == MSAE_POOL_WINDOW) {
      pool = pooled_n ? fmaxf(pool, v) : v;
      ++pooled_n;
    } else if (x.s < g.P) {
      pool += v;
      ++pooled_n;
    }
  }
  r.cand = 0.f;
  if (g.mode == MSAE_POOL_WINDOW) {
    if (e.grp < g.nw) r.cand = r.cnt < g.W ? fmaxf(pool, 0.f) : pool;
  } else if (pooled_n) {
    r.cand = pool / (float)g.P;
  }
  return r;
}

// ---- sort scratch -----------------------------------------------------------------------------------------------------
// 256-byte aligned regions, in this order: two key buffers, two value buffers (pairs), the starts / ends of `runs` runs, the
// sort's temporary storage.  A region of no bytes takes no room.
struct PoolLayout {
  size_t keys0, keys1, vals0, vals1, starts, ends, sort, total;
};

inline size_t pool_sort_bound(long M) { return (size_t)M * 8 + (1u << 20); }

inline PoolLayout pool_layout(long M, bool pairs, long runs) {
  PoolLayout L;
  size_t o = 0;
  auto take = [&](size_t b) { size_t r = o; o = msae_align_up(o + b, 256); return r; };
  L.keys0 = take((size_t)M * 8);
  L.keys1 = take((size_t)M * 8);
  L.vals0 = take(pairs ? (size_t)M * 4 : 0);
  L.vals1 = take(pairs ? (size_t)M * 4 : 0);
  L.starts = take((size_t)runs * 4);
  L.ends = take((size_t)runs * 4);
  L.sort = take(pool_sort_bound(M));
  L.total = o;
  return L;
}

struct PoolSorted {    // where the sort left its result: the other value buffer is free for the caller
  unsigned long long *keys;
  float *vals, *spare;
};

// rocPRIM's radix sort of the M keys in keys0 (with the values in vals0: `pairs`) over the bits [0, end_bit): the size query,
// its check against the layout's bound, the sort
inline int pool_sort(char *w, const PoolLayout &L, long M, unsigned end_bit, bool pairs, hipStream_t st, PoolSorted *out) {
  rocprim::double_buffer<unsigned long long> kb((unsigned long long *)(w + L.keys0), (unsigned long long *)(w + L.keys1));
  rocprim::double_buffer<float> vb((float *)(w + L.vals0), (float *)(w + L.vals1));
  size_t bytes = 0;
  for (void *tmp : {(void *)nullptr, (void *)(w + L.sort)}) {
    if (pairs) MSAE_HIP_TRY(rocprim::radix_sort_pairs(tmp, bytes, kb, vb, (size_t)M, 0u, end_bit, st));
    else MSAE_HIP_TRY(rocprim::radix_sort_keys(tmp, bytes, kb, (size_t)M, 0u, end_bit, st));
    if (bytes > pool_sort_bound(M)) return MSAE_EWS;
  }
  *out = PoolSorted{kb.current(), vb.current(), vb.alternate()};
  return 0;
}

}  // namespace
