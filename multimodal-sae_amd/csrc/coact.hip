// coact.hip -- co-activation counters of a list of query features, updated from the cache loop's top-k, and the
// neighbour lists read from them (include/msae.h: msae_coact_*).
//
// A SEGMENT is a token, a window of W positions or the first P positions of a row (pool mode); a feature is ACTIVE in a
// segment that holds a kept entry of it (|v| > thresh, 0 <= index < N: pool_segments.h's pool_keep).  Per update:
//   counts[slot][g]  += 1 for every segment in which query `slot` and feature g are both active      int32 atomics
//   seg_count[g]     += 1 for every segment in which g is active                                      u64 atomics
// Integer adds commute: the state is the same bits whatever the order of the adds, the cut into calls or their order.
//
// Token mode (coact_token_kernel): one wave (a workgroup of its own) per token, no sort.  The kept entries are compacted into LDS by ballot
// prefix, a repeated index is struck out (the top-k of a token is distinct; a caller's repeat still counts once), the
// query members among them are compacted into a second list, and the lanes stride over the (query member, member)
// product.
// Window / image mode: the distinct members of a segment come from a sort.
//   1. coact_keys_kernel   kept entries of pooled positions -> key (segment << fb | feature); others -> segment = nseg.
//   2. pool_sort           rocPRIM radix sort (keys) over the used key bits, in pool_segments.h's scratch layout.
//   3. coact_heads_kernel  one thread per sorted key: the first key of a run is a distinct member (one add into
//                          seg_count); the first / last key of a segment records its range.
//   4. coact_pairs_kernel  one workgroup per (segment, slice of its range).  The segment's range is walked in chunks of
//                          CO_CHUNK keys: the query members of a chunk go into an LDS list (at most CO_CHUNK of them, so a
//                          segment with any number of query members takes ceil(range / CO_CHUNK) rounds), then the threads
//                          stride over the run heads of the workgroup's slice and add one per listed query.  Consecutive
//                          threads hold ascending features: the adds of a query land along its row.
// Inside one segment every (query, member) pair is distinct, so no two adds of a wave share an address; equal
// destinations meet only across segments (a feature that fires everywhere), where they are separate atomics.
//
// coact_topk_kernel: one workgroup per query row streams the counters (16-byte loads where the row is aligned), turns
// every nonzero one into a rank key (common.h: score descending, feature ascending) and appends the keys that beat the
// current m-th best to an LDS buffer; a full buffer is sorted (sortsel.h) and cut back to its first m.  Rank keys are
// distinct, so the list is a function of the set of candidates alone.
#include "pool_segments.h"
#include "sortsel.h"
#include "wave_ops.h"

namespace {

constexpr int CO_MAX_F = 16384, CO_MAX_M = 64;
constexpr int CO_CHUNK = 1024;              // keys per round of the pairs kernel = capacity of its query list
constexpr int CO_PAIR_THREADS = 256;
constexpr int CO_TOPK_THREADS = 256, CO_TOPK_BUF = 2048, CO_TOPK_TILE = CO_TOPK_THREADS * 4;
static_assert(CO_MAX_M + CO_TOPK_TILE <= CO_TOPK_BUF, "one tile of candidates fits behind a trimmed list");

// ---- token mode ------------------------------------------------------------------------------------------------------
// one single-wave workgroup per token: __syncthreads() orders the wave's LDS traffic
__global__ __launch_bounds__(64) void coact_token_kernel(
    const float *__restrict__ vals, const int32_t *__restrict__ idx, int k, float thresh, int N,
    const int32_t *__restrict__ slot_of, int F, int *__restrict__ counts, unsigned long long *__restrict__ seg_count) {
  __shared__ int feat[POOL_MAX_K];
  __shared__ int slot[POOL_MAX_K];
  const int lane = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * k;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n = 0;                                                // kept entries, in list order
  for (int j0 = 0; j0 < k; j0 += 64) {
    const int j = j0 + lane;
    int f = -1;
    bool keep = false;
    if (j < k) {
      f = idx[base + j];
      keep = pool_keep(vals[base + j], f, thresh, N);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) feat[n + __popcll(m & below)] = f;
    n += __popcll(m);
  }
  __syncthreads();
  // strike out repeats (entry p repeats an earlier one), count the members, list the query members.  A mark of an
  // earlier round reads as -1, which no entry equals: a later repeat is then caught by the FIRST occurrence, never marked.
  int nq = 0;
  for (int p0 = 0; p0 < n; p0 += 64) {
    const int p = p0 + lane;
    const int f = p < n ? feat[p] : -1;
    bool first = p < n;
    const int lim = min(n, p0 + 64);
    for (int i = 0; i < lim; ++i) first = first && !(i < p && feat[i] == f);
    int s = -1;
    if (first) {
      atomicAdd(seg_count + f, 1ull);
      s = slot_of[f];
      if ((unsigned)s >= (unsigned)F) s = -1;
    }
    const unsigned long long m = __ballot(s >= 0);
    if (s >= 0) slot[nq + __popcll(m & below)] = s;
    nq += __popcll(m);
    __syncthreads();                                        // every lane has read feat[] of this round before the marks
    if (p < n && !first) feat[p] = -1;
    __syncthreads();
  }
  const int pairs = nq * n;
  for (int i = lane; i < pairs; i += 64) {
    const int q = i / n, p = i - q * n;
    const int g = feat[p];
    if (g >= 0) atomicAdd(counts + (size_t)slot[q] * N + g, 1);
  }
}

// ---- window / image mode ---------------------------------------------------------------------------------------------
struct CoGeom : PoolGeom {      // ... and the segment-major key: (segment << fb | feature), nseg segments in the call
  int k, fb, nseg;
};

// segment of token (b, s), or -1
__device__ __forceinline__ int co_segment(const CoGeom &g, int b, int s) {
  if (g.mode == MSAE_POOL_WINDOW) return s < g.nw * g.W ? b * g.nw + s / g.W : -1;
  return s < g.P ? b : -1;
}

__global__ __launch_bounds__(256) void coact_keys_kernel(const float *__restrict__ vals, const int32_t *__restrict__ idx,
                                                         long M, float thresh, int N, CoGeom g,
                                                         unsigned long long *__restrict__ keys) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const int f = idx[i];
  const int t = (int)(i / g.k), b = t / g.S, s = t - b * g.S;
  const int seg = pool_keep(vals[i], f, thresh, N) ? co_segment(g, b, s) : -1;
  keys[i] = seg >= 0 ? ((unsigned long long)seg << g.fb) | (unsigned)f : (unsigned long long)g.nseg << g.fb;
}

__global__ __launch_bounds__(256) void coact_heads_kernel(const unsigned long long *__restrict__ keys, long M, CoGeom g,
                                                          int *__restrict__ seg_start, int *__restrict__ seg_end,
                                                          unsigned long long *__restrict__ seg_count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const unsigned long long key = keys[i];
  const int seg = (int)(key >> g.fb);
  if (seg >= g.nseg) return;                                // dropped entries: sorted behind every kept one
  const unsigned long long prev = i ? keys[i - 1] : ~0ull;
  if (prev != key) atomicAdd(seg_count + (int)(key & ((1ull << g.fb) - 1ull)), 1ull);
  if (i == 0 || (int)(prev >> g.fb) != seg) seg_start[seg] = (int)i;
  if (i == M - 1 || (int)(keys[i + 1] >> g.fb) != seg) seg_end[seg] = (int)i + 1;
}

__global__ __launch_bounds__(CO_PAIR_THREADS) void coact_pairs_kernel(
    const unsigned long long *__restrict__ keys, CoGeom g, int N, const int *__restrict__ seg_start,
    const int *__restrict__ seg_end, const int32_t *__restrict__ slot_of, int F, int *__restrict__ counts) {
  __shared__ int s_slot[CO_CHUNK];
  __shared__ int s_nq;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int e = seg_end[seg];
  if (e == 0) return;                                       // empty segment (uniform over the workgroup)
  const int s0 = seg_start[seg];
  const unsigned long long fmask = (1ull << g.fb) - 1ull;
  // this workgroup's slice of the member side
  const int len = e - s0, per = (len + (int)gridDim.y - 1) / (int)gridDim.y;
  const int m0 = s0 + (int)blockIdx.y * per, m1 = min(e, m0 + per);
  if (m0 >= m1) return;
  for (int c0 = s0; c0 < e; c0 += CO_CHUNK) {
    if (tid == 0) s_nq = 0;
    __syncthreads();
    for (int i = c0 + tid; i < min(e, c0 + CO_CHUNK); i += CO_PAIR_THREADS) {
      const unsigned long long key = keys[i];
      if (i == s0 || keys[i - 1] != key) {
        const int s = slot_of[(int)(key & fmask)];
        if ((unsigned)s < (unsigned)F) s_slot[atomicAdd(&s_nq, 1)] = s;
      }
    }
    __syncthreads();
    const int nq = s_nq;
    if (nq) {
      for (int i = m0 + tid; i < m1; i += CO_PAIR_THREADS) {
        const unsigned long long key = keys[i];
        if (i != s0 && keys[i - 1] == key) continue;
        int *col = counts + (int)(key & fmask);
        for (int q = 0; q < nq; ++q) atomicAdd(col + (size_t)s_slot[q] * N, 1);
      }
    }
    __syncthreads();                                        // the next round rewrites the list
  }
}

// ---- neighbour lists -------------------------------------------------------------------------------------------------
__device__ __forceinline__ float co_score(int c, long long sq, long long sg, int metric) {
  if (metric == MSAE_COACT_COUNT) return (float)c;
  const long long u = sq + sg - (long long)c;
  return (float)((double)c / (double)u);
}

template <bool WIDE>
__global__ __launch_bounds__(CO_TOPK_THREADS) void coact_topk_kernel(
    const int *__restrict__ counts, const long long *__restrict__ seg_count, const int32_t *__restrict__ queries, int N,
    int m, int metric, int exclude_self, float *__restrict__ out_val, void *__restrict__ out_idx) {
  __shared__ unsigned long long buf[CO_TOPK_BUF];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, row = blockIdx.x;
  const int q = queries[row];
  const bool q_ok = (unsigned)q < (unsigned)N;
  const long long sq = q_ok ? seg_count[q] : 0;
  const int ex = (exclude_self && q_ok) ? q : -1;
  const int *crow = counts + (size_t)row * N;
  const bool vec = ((uintptr_t)crow & 15) == 0;
  if (tid == 0) s_cnt = 0;
  unsigned long long thr = 0ull;                            // the m-th best key so far (0: fewer than m)
  __syncthreads();
  for (int n0 = 0; n0 < N; n0 += CO_TOPK_TILE) {
    const int g0 = n0 + tid * 4;
    int c[4] = {0, 0, 0, 0};
    if (vec && g0 + 3 < N) {
      const i32x4 v = *reinterpret_cast<const i32x4 *>(crow + g0);
      c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = g0 + j < N ? crow[g0 + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int gi = g0 + j;
      if (c[j] > 0 && gi != ex) {
        const unsigned long long key = rank_key(co_score(c[j], sq, seg_count[gi], metric), gi);
        if (key > thr) buf[atomicAdd(&s_cnt, 1)] = key;
      }
    }
    __syncthreads();
    const int cnt = s_cnt;                                  // uniform; at most CO_TOPK_BUF, by the trim below
    __syncthreads();                                        // ... and read by all before the next tile appends
    if (cnt > CO_TOPK_BUF - CO_TOPK_TILE) {
      lds_sort_desc_u64<4, 8>(buf, cnt, CO_TOPK_BUF, tid);
      if (cnt >= m) thr = buf[m - 1];
      __syncthreads();
      if (tid == 0) s_cnt = min(cnt, m);
      __syncthreads();
    }
  }
  const int cnt = s_cnt;
  lds_sort_desc_u64<4, 8>(buf, cnt, CO_TOPK_BUF, tid);
  if (tid < m) {
    const bool has = tid < cnt;
    const unsigned long long key = has ? buf[tid] : 0ull;
    const size_t o = (size_t)row * m + tid;
    out_val[o] = has ? rank_key_value(key) : 0.f;
    if constexpr (WIDE) static_cast<long long *>(out_idx)[o] = has ? (long long)rank_key_index(key) : -1ll;
    else static_cast<int *>(out_idx)[o] = has ? rank_key_index(key) : -1;
  }
}

PoolLayout co_layout(long T, long M) { return pool_layout(M, false, T > 0 ? T : 1); }

}  // namespace

extern "C" size_t msae_coact_ws_bytes(int T, int k, int N) {
  if (!pool_shape_ok(T, k, N)) return 0;
  return co_layout(T, (long)T * k).total;
}

extern "C" int msae_coact_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N, int mode,
                                 int pool_len, int window, const int32_t *slot_of, int F, int32_t *counts,
                                 uint64_t *seg_count, void *ws, size_t ws_bytes, void *stream) {
  int T;
  if (!pool_tokens(B, S, &T) || !pool_shape_ok(T, k, N) || F < 1 || F > CO_MAX_F) return MSAE_EINVAL;
  if (!pool_mode_ok(mode, pool_len, window, true)) return MSAE_EINVAL;
  if (T == 0) return 0;
  if (!vals || !idx || !slot_of || !counts || !seg_count) return MSAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (mode == MSAE_POOL_TOKEN) {
    hipLaunchKernelGGL(coact_token_kernel, dim3((unsigned)T), dim3(64), 0, st, vals, idx, k, thresh, N, slot_of, F, counts,
                       (unsigned long long *)seg_count);
    return msae_launch_status();
  }
  const PoolGeom pg = pool_geom(T, S, mode, pool_len, window);
  const CoGeom g{pg, k, pool_bit_width((unsigned long long)(N - 1)), mode == MSAE_POOL_WINDOW ? B * pg.nw : B};
  if (g.nseg == 0) return 0;                                // rows shorter than one window: nothing is pooled
  const long M = (long)T * k;
  const PoolLayout L = co_layout(T, M);
  if (!ws || ws_bytes < L.total) return MSAE_EWS;
  char *w = (char *)ws;
  int *starts = (int *)(w + L.starts), *ends = (int *)(w + L.ends);
  const unsigned blocks = (unsigned)((M + 255) / 256);
  hipLaunchKernelGGL(coact_keys_kernel, dim3(blocks), dim3(256), 0, st, vals, idx, M, thresh, N, g,
                     (unsigned long long *)(w + L.keys0));
  MSAE_HIP_TRY(hipMemsetAsync(ends, 0, (size_t)g.nseg * 4, st));
  PoolSorted sorted;
  const unsigned end_bit = (unsigned)(g.fb + pool_bit_width((unsigned long long)g.nseg));
  if (const int rc = pool_sort(w, L, M, end_bit, false, st, &sorted)) return rc;
  hipLaunchKernelGGL(coact_heads_kernel, dim3(blocks), dim3(256), 0, st, sorted.keys, M, g, starts, ends,
                     (unsigned long long *)seg_count);
  // slices of a segment's member side: enough workgroups for the chip when the segments are few (image mode)
  int slices = (1024 + g.nseg - 1) / g.nseg;
  const int max_slices = (int)(((long)(mode == MSAE_POOL_WINDOW ? window : pool_len) * k + 255) / 256);
  slices = slices < 1 ? 1 : slices > 64 ? 64 : slices;
  if (slices > max_slices) slices = max_slices;
  hipLaunchKernelGGL(coact_pairs_kernel, dim3((unsigned)g.nseg, (unsigned)slices), dim3(CO_PAIR_THREADS), 0, st,
                     sorted.keys, g, N, starts, ends, slot_of, F, counts);
  return msae_launch_status();
}

static int coact_topk_impl(const int32_t *counts, const int64_t *seg_count, const int32_t *queries, int F, int N, int m,
                           int metric, int exclude_self, float *out_val, void *out_idx, bool wide, void *stream) {
  if (F < 1 || F > CO_MAX_F || N <= 0 || N > POOL_MAX_N || m < 1 || m > CO_MAX_M) return MSAE_EINVAL;
  if (metric != MSAE_COACT_JACCARD && metric != MSAE_COACT_COUNT) return MSAE_EINVAL;
  if (!counts || !seg_count || !queries || !out_val || !out_idx) return MSAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (wide)
    hipLaunchKernelGGL(coact_topk_kernel<true>, dim3((unsigned)F), dim3(CO_TOPK_THREADS), 0, st, counts,
                       (const long long *)seg_count, queries, N, m, metric, exclude_self, out_val, out_idx);
  else
    hipLaunchKernelGGL(coact_topk_kernel<false>, dim3((unsigned)F), dim3(CO_TOPK_THREADS), 0, st, counts,
                       (const long long *)seg_count, queries, N, m, metric, exclude_self, out_val, out_idx);
  return msae_launch_status();
}

extern "C" int msae_coact_topk(const int32_t *counts, const int64_t *seg_count, const int32_t *queries, int F, int N,
                               int m, int metric, int exclude_self, float *out_val, int32_t *out_idx, void *stream) {
  return coact_topk_impl(counts, seg_count, queries, F, N, m, metric, exclude_self, out_val, out_idx, false, stream);
}

extern "C" int msae_coact_topk_i64(const int32_t *counts, const int64_t *seg_count, const int32_t *queries, int F, int N,
                                   int m, int metric, int exclude_self, float *out_val, int64_t *out_idx, void *stream) {
  return coact_topk_impl(counts, seg_count, queries, F, N, m, metric, exclude_self, out_val, out_idx, true, stream);
}
