// feature_stats.hip -- per-feature statistics and top-example tables, updated from the cache loop's top-k.
//
// Answers, for every feature as the tokens stream by, the two questions the reference's explain side re-derives
// from the COO split files afterwards: how often a feature fires (loader.py:103-106, min_examples) and which rows
// / windows activate it most (features/constructors.py:28-85 pool_max_activation_windows, 88-141
// pool_max_activations_windows_image -- there a dense [rows, seq] tensor per feature on the CPU).
//
// One update per batch of [B*S][k] top-k pairs:
//   1. key build      pool_segments.h's pool_keys_kernel: every kept entry (|v| > thresh, sparsify's rule; no filter bitmap)
//                     becomes the key (feature << tb | t) with its value; dropped entries get feature = N and sort last.
//   2. radix sort     rocPRIM's device radix sort over the used key bits: entries grouped by feature, and inside a
//                     feature in token order (t is unique per feature: a token's top-k indices are distinct).
//   3. group pass     a GROUP is the run of one feature inside one pooling segment (window mode: [w*W, (w+1)*W) of
//                     a row, the ragged tail its own group; image mode: the row).  The thread on a group's first
//                     entry walks it in ascending position (pool_segments.h's pool_walk_run, the walk the activation
//                     histograms share): count / max / f64 sum -> ONE atomic each per (group,
//                     feature), not one per token (a feature that fires on every token costs B*S/W atomics, not
//                     B*S); the pooled value of the segment -> cand[i] (0 = no candidate).
//   4. table merge    one wave per feature with records in this batch: the candidates of its run are ranked
//                     against its sorted top-n table (value descending, id ascending: a total order) and merged.
//                     The table after a batch is the top-n of every candidate seen, whatever the cut into calls.
//                     With a sample (msae_feature_stats_update_sampled) the same wave, while the chunk of candidates is
//                     in LDS, also merges it into the feature's uniform sample table: the same rank-and-scatter body
//                     under another order (FsSampleOrder: a hash of (seed, feature, id) ascending), and counts the
//                     feature's candidates.
// No host synchronisation, no allocation (workspace: msae_feature_stats_ws_bytes).
#include "pool_segments.h"
#include "wave_ops.h"

namespace {

constexpr int FS_MAX_TOP = 256;

struct FsGeom : PoolGeom {      // ... and the global row of the call's first row
  long long row_base;
};

// the pooled candidate's id: image = global row, window = global row * (S / W) + w
__device__ __forceinline__ long long fs_id(const FsGeom &g, int b, int grp) {
  return g.mode == MSAE_POOL_WINDOW ? (g.row_base + b) * (long long)g.nw + grp : g.row_base + b;
}

__device__ __forceinline__ void atomic_max_f32(float *p, float v) {
  if (v >= 0.f)
    atomicMax((int *)p, __float_as_int(v));
  else
    atomicMin((unsigned *)p, __float_as_uint(v));
}

// ---- table orders --------------------------------------------------------------------------------------------------
// A table is one feature's list of (value, id) entries, sorted under a strict total order of (key, id).  The key is derived
// from the entry (and the feature), never stored in HBM: `feature(f)` is the per-feature part of it, `key(h, v, id)` the rest.
struct FsTopOrder {      // top examples: value descending, then id ascending; the key is the value itself
  using Key = float;
  static constexpr bool kKeyIsValue = true;
  __device__ __forceinline__ unsigned long long feature(int) const { return 0ull; }
  __device__ __forceinline__ Key key(unsigned long long, float v, long long) const { return v; }
  static __device__ __forceinline__ bool before(Key ak, long long ai, Key bk, long long bi) {
    return ak > bk || (ak == bk && ai < bi);
  }
};
// uniform sample: prio(seed, f, id) = mix64(mix64(seed + 0x9E3779B97F4A7C15 * (f + 1)) ^ (uint64)id) ascending, then id
// ascending.  For fixed (seed, f) a bijection of id: distinct ids never tie.  Pinned (include/msae.h, tests):
//   prio(22, 0, 0) = 0xbe5264ad2aa020f4   prio(1, 5, 7) = 0xb2e6c178b81a5c56   prio(22, 7, 2^33) = 0x27044a0765e2616f
//   prio(22, 131071, 12345) = 0x45984866898b23bf   prio(2^64 - 1, 262143, 2^40 + 3) = 0xaf8ee0a530541d25
struct FsSampleOrder {
  using Key = unsigned long long;
  static constexpr bool kKeyIsValue = false;
  unsigned long long seed;
  __device__ __forceinline__ unsigned long long feature(int f) const {
    return mix64(seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)f + 1ull));
  }
  __device__ __forceinline__ Key key(unsigned long long h, float, long long id) const {
    return mix64(h ^ (unsigned long long)id);
  }
  static __device__ __forceinline__ bool before(Key ak, long long ai, Key bk, long long bi) {
    return ak < bk || (ak == bk && ai < bi);
  }
};

// Two sorted lists of one feature, of up to CAP entries each, in LDS (the merge kernel's double buffer; dst and src of the
// table-to-table merge).  An order whose key is the value keeps no value array.
template <class O, int CAP, bool = O::kKeyIsValue>
struct FsTableVal {
  float val[2][CAP];
};
template <class O, int CAP>
struct FsTableVal<O, CAP, true> {};
template <class O, int CAP = FS_MAX_TOP>
struct FsTable : FsTableVal<O, CAP> {
  typename O::Key key[2][CAP];
  long long id[2][CAP];
  __device__ __forceinline__ float value(int b, int j) const {
    if constexpr (O::kKeyIsValue) return key[b][j]; else return this->val[b][j];
  }
  __device__ __forceinline__ void put(int b, int j, typename O::Key k, float v, long long i) {
    key[b][j] = k;
    id[b][j] = i;
    if constexpr (!O::kKeyIsValue) this->val[b][j] = v;
  }
};

// HBM table of n slots -> list b, keys derived on the way; returns the number of valid entries (they sit at the front)
template <class O, int CAP>
__device__ __forceinline__ int fs_table_load(FsTable<O, CAP> &T, int b, const O &o, unsigned long long h,
                                             const float *__restrict__ tv, const long long *__restrict__ ti, int n,
                                             int lane) {
  int tn = 0;
  for (int j = lane; j < n; j += 64) {
    const float v = tv[j];
    const long long i = ti[j];
    T.put(b, j, o.key(h, v, i), v, i);
    tn += i >= 0;
  }
  return wave_sum(tn);
}

// One chunk of up to 64 candidates (key ck / value cv / id ci per lane of `mask`, in LDS; this lane's own in k, v, id) into
// list `cur` of tn entries -> list cur ^ 1 of min(n, tn + candidates) entries: every candidate and every entry computes its
// rank in the merged list and scatters itself there.  Equal (key, id) pairs (a caller that repeats an id) rank by lane.
template <class O, int CAP>
__device__ __forceinline__ void fs_table_merge_chunk(FsTable<O, CAP> &T, int cur, int &tn, int n, unsigned long long mask,
                                                     bool is_c, int lane, const typename O::Key *ck,
                                                     const long long *ci, typename O::Key k, float v, long long id) {
  using Key = typename O::Key;
  const Key *A = T.key[cur];
  const long long *AI = T.id[cur];
  if (is_c) {
    int r = 0;                                      // candidates of this chunk ranked before this one
    for (unsigned long long m = mask; m; m &= m - 1) {
      const int o = __builtin_ctzll(m);
      r += O::before(ck[o], ci[o], k, id) || (ck[o] == k && ci[o] == id && o < lane);
    }
    int lo = 0, hi = tn;                            // table entries ranked before or equal: upper bound
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (O::before(k, id, A[mid], AI[mid])) hi = mid; else lo = mid + 1;
    }
    r += lo;
    if (r < n) T.put(cur ^ 1, r, k, v, id);
  }
  for (int j = lane; j < tn; j += 64) {
    const Key ak = A[j];
    const long long aid = AI[j];
    int r = j;
    for (unsigned long long m = mask; m; m &= m - 1) {
      const int o = __builtin_ctzll(m);
      r += O::before(ck[o], ci[o], ak, aid);
    }
    if (r < n) T.put(cur ^ 1, r, ak, T.value(cur, j), aid);
  }
  tn = min(n, tn + __popcll(mask));
}

template <class O, int CAP>
__device__ __forceinline__ void fs_table_store(const FsTable<O, CAP> &T, int b, int tn, float *__restrict__ tv,
                                               long long *__restrict__ ti, int n, int lane) {
  for (int j = lane; j < n; j += 64) {
    tv[j] = j < tn ? T.value(b, j) : 0.f;
    ti[j] = j < tn ? T.id[b][j] : -1ll;
  }
}

struct FsSampleArgs {    // msae_feature_sample on the device side
  int n;
  unsigned long long seed;
  unsigned long long *seg_count;
  float *val;
  long long *id;
};

template <bool SAMPLE, int CAP>
struct FsMergeLds {
  FsTable<FsTopOrder, CAP> top;
  float cv[64];
  long long ci[64];
};
template <int CAP>
struct FsMergeLds<true, CAP> : FsMergeLds<false, CAP> {
  FsTable<FsSampleOrder, CAP> smp;
  unsigned long long cp[64];
};

// one thread per sorted entry: run boundaries of every feature, and the walk of every group from its first entry
__global__ __launch_bounds__(256) void fs_group_kernel(const unsigned long long *__restrict__ keys,
                                                       const float *__restrict__ kv, long M, int N, FsGeom g,
                                                       int *__restrict__ run_start, int *__restrict__ run_end,
                                                       float *__restrict__ cand, unsigned long long *__restrict__ count,
                                                       float *__restrict__ act_max, double *__restrict__ act_sum) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const PoolEntry e = pool_entry(keys[i], g);
  const int f = e.f;
  if (f >= N) return;                               // dropped entries: sorted behind every kept one
  if (i == 0 || pool_key_feature(keys[i - 1], g) != f) run_start[f] = (int)i;
  if (i == M - 1 || pool_key_feature(keys[i + 1], g) != f) run_end[f] = (int)i + 1;
  if (!pool_run_head(keys, i, e, g)) {
    cand[i] = 0.f;
    return;
  }
  const PoolRun r = pool_walk_run<true>(keys, kv, M, i, e, g);
  atomicAdd(count + f, (unsigned long long)r.cnt);    // the ragged tail has no candidate but counts here
  atomic_max_f32(act_max + f, r.mx);
  atomicAdd(act_sum + f, r.sum);
  cand[i] = (r.cand == r.cand) ? r.cand : 0.f;      // NaN never enters a table
}

// one single-wave workgroup per feature (grid-stride): rank this batch's candidates against the feature's table(s), merge.
// SAMPLE: the same chunk of candidates, while it is in LDS, also goes into the feature's sample table under FsSampleOrder, and
// the feature's candidates are counted (the popcount of the ballots: this wave owns the feature, no atomics).
// CAP >= n (and >= sa.n) sizes the tables in LDS.  The kernel waits on HBM, one wave per workgroup, so the workgroups a CU
// holds -- LDS-bound -- set its speed: tables of <= 64 entries on both sides take the CAP = 64 instantiation (5.4 KB against
// 17.3 KB).
template <bool SAMPLE, int CAP>
__global__ __launch_bounds__(64) void fs_merge_kernel(const unsigned long long *__restrict__ keys,
                                                      const float *__restrict__ cand, int N, int n, FsGeom g,
                                                      const int *__restrict__ run_start, const int *__restrict__ run_end,
                                                      float *__restrict__ top_val, long long *__restrict__ top_id,
                                                      FsSampleArgs sa) {
  __shared__ FsMergeLds<SAMPLE, CAP> L;
  const int lane = threadIdx.x;
  const unsigned long long tmask = (1ull << g.tb) - 1ull;
  const FsTopOrder top_order{};
  const FsSampleOrder smp_order{sa.seed};
  for (int f = blockIdx.x; f < N; f += gridDim.x) {
    const int e = run_end[f];
    if (e == 0) continue;                           // no record of f in this batch
    const int s0 = run_start[f];
    float *tv = top_val + (size_t)f * n;
    long long *ti = top_id + (size_t)f * n;
    int tn = fs_table_load(L.top, 0, top_order, 0ull, tv, ti, n, lane);
    unsigned long long h = 0ull;
    int sn = 0, nseg = 0;
    if constexpr (SAMPLE) {
      h = smp_order.feature(f);
      sn = fs_table_load(L.smp, 0, smp_order, h, sa.val + (size_t)f * sa.n, sa.id + (size_t)f * sa.n, sa.n, lane);
    }
    int cur = 0;
    bool changed = false;
    __syncthreads();
    for (int base = s0; base < e; base += 64) {
      const int i = base + lane;
      const float c = i < e ? cand[i] : 0.f;
      const bool is_c = c != 0.f;
      const unsigned long long mask = __ballot(is_c);
      if (mask == 0ull) continue;
      changed = true;
      long long id = 0;
      if (is_c) {
        const int t = (int)(keys[i] & tmask), b = t / g.S;
        id = fs_id(g, b, g.group(t - b * g.S));
      }
      L.cv[lane] = c;
      L.ci[lane] = id;
      unsigned long long p = 0ull;
      if constexpr (SAMPLE) {
        p = smp_order.key(h, c, id);
        L.cp[lane] = p;
        nseg += __popcll(mask);
      }
      __syncthreads();
      fs_table_merge_chunk(L.top, cur, tn, n, mask, is_c, lane, L.cv, L.ci, c, c, id);
      if constexpr (SAMPLE)
        fs_table_merge_chunk(L.smp, cur, sn, sa.n, mask, is_c, lane, L.cp, L.ci, p, c, id);
      cur ^= 1;
      __syncthreads();
    }
    if (changed) {
      fs_table_store(L.top, cur, tn, tv, ti, n, lane);
      if constexpr (SAMPLE) {
        fs_table_store(L.smp, cur, sn, sa.val + (size_t)f * sa.n, sa.id + (size_t)f * sa.n, sa.n, lane);
        if (lane == 0) sa.seg_count[f] += (unsigned long long)nseg;
      }
    }
    __syncthreads();
  }
}

// dst += src, feature by feature, for the tables of order O: counts add (and, with the top table's statistics, maxima max and
// sums add: act_max != null), tables merge in O's total order
template <class O>
__global__ __launch_bounds__(64) void fs_merge_tables_kernel(
    int N, int n, O order, unsigned long long *__restrict__ count, float *__restrict__ act_max,
    double *__restrict__ act_sum, float *__restrict__ dst_val, long long *__restrict__ dst_id,
    const unsigned long long *__restrict__ s_count, const float *__restrict__ s_max, const double *__restrict__ s_sum,
    const float *__restrict__ s_val, const long long *__restrict__ s_id) {
  __shared__ FsTable<O> T;                          // list 0: dst, list 1: src
  const int lane = threadIdx.x;
  for (int f = blockIdx.x; f < N; f += gridDim.x) {
    if (lane == 0) {
      count[f] += s_count[f];
      if (act_max) {
        act_max[f] = fmaxf(act_max[f], s_max[f]);
        act_sum[f] += s_sum[f];
      }
    }
    float *tv = dst_val + (size_t)f * n;
    long long *ti = dst_id + (size_t)f * n;
    const unsigned long long h = order.feature(f);
    const int na = fs_table_load(T, 0, order, h, tv, ti, n, lane);
    const int nb = fs_table_load(T, 1, order, h, s_val + (size_t)f * n, s_id + (size_t)f * n, n, lane);
    __syncthreads();
    if (nb) {
      for (int j = lane; j < na; j += 64) {         // dst entries: after the src entries strictly before them
        int lo = 0, hi = nb;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (O::before(T.key[1][mid], T.id[1][mid], T.key[0][j], T.id[0][j])) lo = mid + 1; else hi = mid;
        }
        if (j + lo < n) {
          tv[j + lo] = T.value(0, j);
          ti[j + lo] = T.id[0][j];
        }
      }
      for (int j = lane; j < nb; j += 64) {         // src entries: after the dst entries before or equal
        int lo = 0, hi = na;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (O::before(T.key[1][j], T.id[1][j], T.key[0][mid], T.id[0][mid])) hi = mid; else lo = mid + 1;
        }
        if (j + lo < n) {
          tv[j + lo] = T.value(1, j);
          ti[j + lo] = T.id[1][j];
        }
      }
    }
    __syncthreads();
  }
}

PoolLayout fs_layout(long M, int N) { return pool_layout(M, true, N); }

bool fs_args_ok(int T, int k, int N, int n_top, int mode, int pool_len, int window) {
  return pool_shape_ok(T, k, N) && n_top > 0 && n_top <= FS_MAX_TOP && pool_mode_ok(mode, pool_len, window, false);
}

}  // namespace

extern "C" size_t msae_feature_stats_ws_bytes(int T, int k, int N) {
  if (!pool_shape_ok(T, k, N)) return 0;
  return fs_layout((long)T * k, N).total;
}

namespace {

bool fs_sample_ok(const msae_feature_sample *sm) {
  if (sm->size < sizeof(msae_feature_sample)) return false;
  if (sm->n_sample <= 0 || sm->n_sample > FS_MAX_TOP) return false;
  return sm->seg_count && sm->smp_val && sm->smp_id;
}

int fs_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N, int mode, int pool_len,
              int window, int64_t row_base, int n_top, uint64_t *count, float *act_max, double *act_sum, float *top_val,
              int64_t *top_id, const msae_feature_sample *sample, void *ws, size_t ws_bytes, void *stream) {
  int T;
  if (!pool_tokens(B, S, &T)) return MSAE_EINVAL;
  if (!fs_args_ok(T, k, N, n_top, mode, pool_len, window) || row_base < 0) return MSAE_EINVAL;
  if (sample && !fs_sample_ok(sample)) return MSAE_EINVAL;
  if (T == 0) return 0;
  const long M = (long)T * k;
  const PoolLayout L = fs_layout(M, N);
  if (!ws || ws_bytes < L.total) return MSAE_EWS;
  hipStream_t st = (hipStream_t)stream;
  char *w = (char *)ws;
  int *starts = (int *)(w + L.starts), *ends = (int *)(w + L.ends);
  const FsGeom g{pool_geom(T, S, mode, pool_len, window), row_base};
  const unsigned blocks = (unsigned)((M + 255) / 256);
  hipLaunchKernelGGL(pool_keys_kernel, dim3(blocks), dim3(256), 0, st, vals, idx, M, k, thresh, N, g.tb,
                     (unsigned long long *)(w + L.keys0), (float *)(w + L.vals0));
  MSAE_HIP_TRY(hipMemsetAsync(ends, 0, (size_t)N * 4, st));
  PoolSorted sorted;
  const unsigned end_bit = (unsigned)(g.tb + pool_bit_width((unsigned long long)N));
  if (const int rc = pool_sort(w, L, M, end_bit, true, st, &sorted)) return rc;
  // the group pass writes the candidates over the sort's other value buffer (dead after the sort)
  float *cand = sorted.spare;
  hipLaunchKernelGGL(fs_group_kernel, dim3(blocks), dim3(256), 0, st, sorted.keys, sorted.vals, M, N, g, starts, ends,
                     cand, (unsigned long long *)count, act_max, act_sum);
  const unsigned mblocks = (unsigned)(N < 8192 ? N : 8192);
  FsSampleArgs sa{};
  if (sample) {
    sa = FsSampleArgs{sample->n_sample, (unsigned long long)sample->seed, (unsigned long long *)sample->seg_count,
                      sample->smp_val, (long long *)sample->smp_id};
    auto kern = n_top <= 64 && sa.n <= 64 ? fs_merge_kernel<true, 64> : fs_merge_kernel<true, FS_MAX_TOP>;
    hipLaunchKernelGGL(kern, dim3(mblocks), dim3(64), 0, st, sorted.keys, cand, N, n_top, g, starts, ends, top_val,
                       (long long *)top_id, sa);
  } else {
    hipLaunchKernelGGL((fs_merge_kernel<false, FS_MAX_TOP>), dim3(mblocks), dim3(64), 0, st, sorted.keys, cand, N, n_top, g, starts,
                       ends, top_val, (long long *)top_id, sa);
  }
  return msae_launch_status();
}

}  // namespace

extern "C" int msae_feature_stats_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh,
                                         int N, int mode, int pool_len, int window, int64_t row_base, int n_top,
                                         uint64_t *count, float *act_max, double *act_sum, float *top_val,
                                         int64_t *top_id, void *ws, size_t ws_bytes, void *stream) {
  return fs_update(vals, idx, B, S, k, thresh, N, mode, pool_len, window, row_base, n_top, count, act_max, act_sum,
                   top_val, top_id, nullptr, ws, ws_bytes, stream);
}

extern "C" int msae_feature_stats_update_sampled(const float *vals, const int32_t *idx, int B, int S, int k,
                                                 float thresh, int N, int mode, int pool_len, int window,
                                                 int64_t row_base, int n_top, uint64_t *count, float *act_max,
                                                 double *act_sum, float *top_val, int64_t *top_id,
                                                 const msae_feature_sample *sample, void *ws, size_t ws_bytes,
                                                 void *stream) {
  return fs_update(vals, idx, B, S, k, thresh, N, mode, pool_len, window, row_base, n_top, count, act_max, act_sum,
                   top_val, top_id, sample, ws, ws_bytes, stream);
}

extern "C" int msae_feature_stats_merge(int N, int n_top, uint64_t *count, float *act_max, double *act_sum,
                                        float *top_val, int64_t *top_id, const uint64_t *src_count,
                                        const float *src_max, const double *src_sum, const float *src_val,
                                        const int64_t *src_id, void *stream) {
  if (N <= 0 || N > POOL_MAX_N || n_top <= 0 || n_top > FS_MAX_TOP) return MSAE_EINVAL;
  const unsigned blocks = (unsigned)(N < 8192 ? N : 8192);
  hipLaunchKernelGGL(fs_merge_tables_kernel<FsTopOrder>, dim3(blocks), dim3(64), 0, (hipStream_t)stream, N, n_top,
                     FsTopOrder{}, (unsigned long long *)count, act_max, act_sum, top_val, (long long *)top_id,
                     (const unsigned long long *)src_count, src_max, src_sum, src_val, (const long long *)src_id);
  return msae_launch_status();
}

extern "C" int msae_feature_sample_merge(int N, int n_sample, uint64_t seed, uint64_t *seg_count, float *smp_val,
                                         int64_t *smp_id, const uint64_t *src_seg_count, const float *src_val,
                                         const int64_t *src_id, void *stream) {
  if (N <= 0 || N > POOL_MAX_N || n_sample <= 0 || n_sample > FS_MAX_TOP) return MSAE_EINVAL;
  if (!seg_count || !smp_val || !smp_id || !src_seg_count || !src_val || !src_id) return MSAE_EINVAL;
  const unsigned blocks = (unsigned)(N < 8192 ? N : 8192);
  hipLaunchKernelGGL(fs_merge_tables_kernel<FsSampleOrder>, dim3(blocks), dim3(64), 0, (hipStream_t)stream, N,
                     n_sample, FsSampleOrder{(unsigned long long)seed}, (unsigned long long *)seg_count,
                     (float *)nullptr, (double *)nullptr, smp_val, (long long *)smp_id,
                     (const unsigned long long *)src_seg_count, (const float *)nullptr, (const double *)nullptr, src_val,
                     (const long long *)src_id);
  return msae_launch_status();
}
