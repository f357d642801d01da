// token_profile.hip -- token profiles of a list of query features, updated from the cache loop's top-k and the batch's token
// ids, and the top-token lists read from them (include/msae.h: msae_token_profile_*).
//
// For F query features, a vocabulary of V tokens and O offsets o_a: an entry (v, f) at position (b, s) that is kept (|v| >
// thresh, 0 <= f < N: the cache's rule) and positive (v > 0: the position profiles' rule), with f the query of slot i, adds
//   counts[a][i][t] += 1,  mass[a][i][t] += q(v)      for every a with 0 <= s + o_a < S and t = ids[b][s + o_a] in [0, V)
// and every position (b, s') adds tok_count[a][ids[b][s']] += 1 for every a with 0 <= s' - o_a < S.  Integer adds commute: the
// state is the same bits whatever the order of the adds, the cut into calls or their order.
//
// tp_update_kernel: pos_profile.hip's update kernel with the slot_of lookup in front, so that most entries leave after one
// load.  Workgroup (x, a) takes TP_ENTRIES consecutive entries for offset plane a, one lane per entry and round, and adds its
// (cell, 1, q) triples into an LDS table (open addressing, at most TP_ENTRIES keys in 2 * TP_ENTRIES slots: every probe
// sequence ends); then every used slot issues ONE global atomic, or a pair with mass.  A padding token under a feature that
// fires everywhere costs T * k / TP_ENTRIES adds on its cell instead of T.  tp_tok_kernel is the same table over the positions,
// keyed by the token id alone.  No workgroup waits for another: no flags, no hand-over.
//
// tp_topk_kernel: coact.hip's coact_topk_kernel over a row of tokens: one workgroup per query row of ONE offset plane streams
// the counters, turns every token with count >= min_count into a rank key (common.h: score descending, token ascending) and
// appends the keys that beat the current m-th best to an LDS buffer; a full buffer is sorted (sortsel.h) and cut back to its
// first m.  The row total of the counters comes out of the same pass.
//
// Nothing is indexed by a list entry's feature, by a slot or by a token id that was not range-checked first.
#include "pool_segments.h"
#include "pos_q.h"
#include "sortsel.h"
#include "token_profile_args.h"
#include "wave_ops.h"

namespace {

using tp_args::Offsets;
constexpr int TP_ENTRIES = tp_args::ENTRIES;        // entries (positions) per workgroup
constexpr int TP_SLOTS = 2 * TP_ENTRIES;            // table slots: a power of two, never more than half full
constexpr int TP_SLOT_BITS = 11;
static_assert(1 << TP_SLOT_BITS == TP_SLOTS && TP_ENTRIES % 256 == 0, "table size");
static_assert(tp_args::MAX_T == MSAE_STATS_MAX_T && tp_args::MAX_K == POOL_MAX_K && tp_args::MAX_N == POOL_MAX_N,
              "the envelope of the other cache-loop updates");
constexpr int TP_TOPK_THREADS = 256, TP_TOPK_BUF = 2048, TP_TOPK_TILE = TP_TOPK_THREADS * 4;
static_assert(tp_args::MAX_M + TP_TOPK_TILE <= TP_TOPK_BUF, "one tile of candidates fits behind a trimmed list");

// the slot of `key` (>= 0) in the table: linear probing; a free slot exists, there are at most TP_ENTRIES keys
__device__ __forceinline__ int tp_slot(int *s_key, int key) {
  unsigned slot = ((unsigned)key * 2654435761u) >> (32 - TP_SLOT_BITS);
  for (;;) {
    const int prev = atomicCAS(&s_key[slot], -1, key);
    if (prev == -1 || prev == key) return (int)slot;
    slot = (slot + 1) & (TP_SLOTS - 1);
  }
}

// token id p of the batch (0 <= p < T), 32 or 64 bits wide
__device__ __forceinline__ long long tp_id(const void *__restrict__ ids, int ids64, long p) {
  return ids64 ? static_cast<const long long *>(ids)[p] : (long long)static_cast<const int *>(ids)[p];
}

template <typename IdxT, bool MASS>
__global__ __launch_bounds__(256) void tp_update_kernel(const float *__restrict__ vals, const IdxT *__restrict__ idx, long M,
                                                        int k, int S, float thresh, int N, const int32_t *__restrict__ slot_of,
                                                        int F, int V, const void *__restrict__ ids, int ids64, Offsets off,
                                                        int *__restrict__ counts, unsigned long long *__restrict__ mass) {
  __shared__ int s_key[TP_SLOTS];                   // slot * V + token (< 2^31), -1 = free
  __shared__ int s_cnt[TP_SLOTS];
  __shared__ unsigned long long s_mass[MASS ? TP_SLOTS : 1];
  for (int s = threadIdx.x; s < TP_SLOTS; s += 256) {
    s_key[s] = -1;
    s_cnt[s] = 0;
    if constexpr (MASS) s_mass[s] = 0ull;
  }
  __syncthreads();
  const int a = blockIdx.y, o = off.o[a];
  const long base = (long)blockIdx.x * TP_ENTRIES;
  for (int e = 0; e < TP_ENTRIES; e += 256) {
    const long i = base + e + threadIdx.x;
    if (i >= M) break;
    const float v = vals[i];
    const IdxT f = idx[i];
    // the keep rule (pool_keep) on an index of either width, and the count rule v > 0 (a NaN fails both comparisons)
    if (!(fabsf(v) > thresh && v > 0.f) || (unsigned long long)(long long)f >= (unsigned long long)N) continue;
    const int slot = slot_of[(int)f];
    if ((unsigned)slot >= (unsigned)F) continue;    // no query: most entries leave here
    const long t = i / k;
    const int s2 = (int)(t % S) + o;
    if ((unsigned)s2 >= (unsigned)S) continue;      // offsets never cross a row
    const long long id = tp_id(ids, ids64, t + o);  // t + o = b * S + s2, inside the batch
    if ((unsigned long long)id >= (unsigned long long)V) continue;
    const int w = tp_slot(s_key, slot * V + (int)id);
    atomicAdd(&s_cnt[w], 1);
    if constexpr (MASS) atomicAdd(&s_mass[w], pp_q(v));
  }
  __syncthreads();
  const size_t plane = (size_t)a * F * V;
  for (int s = threadIdx.x; s < TP_SLOTS; s += 256) {
    const int c = s_cnt[s];
    if (c) {
      atomicAdd(counts + plane + s_key[s], c);
      if constexpr (MASS) atomicAdd(mass + plane + s_key[s], s_mass[s]);
    }
  }
}

__global__ __launch_bounds__(256) void tp_tok_kernel(const void *__restrict__ ids, int ids64, int T, int S, int V, Offsets off,
                                                     unsigned long long *__restrict__ tok_count) {
  __shared__ int s_key[TP_SLOTS];                   // the token, -1 = free
  __shared__ int s_cnt[TP_SLOTS];
  for (int s = threadIdx.x; s < TP_SLOTS; s += 256) {
    s_key[s] = -1;
    s_cnt[s] = 0;
  }
  __syncthreads();
  const int a = blockIdx.y, o = off.o[a];
  const long base = (long)blockIdx.x * TP_ENTRIES;
  for (int e = 0; e < TP_ENTRIES; e += 256) {
    const long p = base + e + threadIdx.x;
    if (p >= T) break;
    if ((unsigned)((int)(p % S) - o) >= (unsigned)S) continue;     // no position s of the row has s + o here
    const long long id = tp_id(ids, ids64, p);
    if ((unsigned long long)id >= (unsigned long long)V) continue;
    atomicAdd(&s_cnt[tp_slot(s_key, (int)id)], 1);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < TP_SLOTS; s += 256) {
    const int c = s_cnt[s];
    if (c) atomicAdd(tok_count + (size_t)a * V + s_key[s], (unsigned long long)c);
  }
}

// ---- top tokens ------------------------------------------------------------------------------------------------------
// one fixed operation sequence per metric (include/msae.h); c >= 1
__device__ __forceinline__ float tp_score(int c, long long tc, unsigned long long ms, int metric) {
  if (metric == MSAE_TOKEN_COUNT) return (float)c;
  if (metric == MSAE_TOKEN_PRECISION) return (float)((double)c / (double)tc);
  return (float)((double)ms / (double)c * 0x1p-20);
}

__global__ __launch_bounds__(TP_TOPK_THREADS) void tp_topk_kernel(
    const int *__restrict__ counts, const unsigned long long *__restrict__ mass, const long long *__restrict__ tok_count, int V,
    int m, int metric, int min_count, float *__restrict__ out_val, int *__restrict__ out_tok, long long *__restrict__ out_total) {
  __shared__ unsigned long long buf[TP_TOPK_BUF];
  __shared__ long long s_tot[TP_TOPK_THREADS / 64];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, row = blockIdx.x;
  const int *crow = counts + (size_t)row * V;
  const unsigned long long *mrow = metric == MSAE_TOKEN_MEAN ? mass + (size_t)row * V : nullptr;
  const bool vec = ((uintptr_t)crow & 15) == 0;
  if (tid == 0) s_cnt = 0;
  unsigned long long thr = 0ull;                            // the m-th best key so far (0: fewer than m)
  long long tot = 0;
  __syncthreads();
  for (int n0 = 0; n0 < V; n0 += TP_TOPK_TILE) {
    const int g0 = n0 + tid * 4;
    int c[4] = {0, 0, 0, 0};
    if (vec && g0 + 3 < V) {
      const i32x4 v = *reinterpret_cast<const i32x4 *>(crow + g0);
      c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = g0 + j < V ? crow[g0 + j] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = g0 + j;
      tot += c[j];
      if (c[j] >= min_count) {                              // min_count >= 1: t < V here
        const long long tc = metric == MSAE_TOKEN_PRECISION ? tok_count[t] : 0;
        const unsigned long long key = rank_key(tp_score(c[j], tc, mrow ? mrow[t] : 0ull, metric), t);
        if (key > thr) buf[atomicAdd(&s_cnt, 1)] = key;
      }
    }
    __syncthreads();
    const int cnt = s_cnt;                                  // uniform; at most TP_TOPK_BUF, by the trim below
    __syncthreads();                                        // ... and read by all before the next tile appends
    if (cnt > TP_TOPK_BUF - TP_TOPK_TILE) {
      lds_sort_desc_u64<4, 8>(buf, cnt, TP_TOPK_BUF, tid);
      if (cnt >= m) thr = buf[m - 1];
      __syncthreads();
      if (tid == 0) s_cnt = min(cnt, m);
      __syncthreads();
    }
  }
  const int cnt = s_cnt;
  lds_sort_desc_u64<4, 8>(buf, cnt, TP_TOPK_BUF, tid);
  if (tid < m) {
    const bool has = tid < cnt;
    const unsigned long long key = has ? buf[tid] : 0ull;
    const size_t o = (size_t)row * m + tid;
    out_val[o] = has ? rank_key_value(key) : 0.f;
    out_tok[o] = has ? rank_key_index(key) : -1;
  }
  tot = wave_sum(tot);
  if ((tid & 63) == 0) s_tot[tid >> 6] = tot;
  __syncthreads();
  if (tid == 0) {
    long long all = 0;
#pragma unroll
    for (int w = 0; w < TP_TOPK_THREADS / 64; ++w) all += s_tot[w];
    out_total[row] = all;
  }
}

template <typename IdxT>
int tp_update(const float *vals, const IdxT *idx, const void *ids, int ids_bits, int B, int S, int k, float thresh, int N,
              const int32_t *slot_of, int F, int V, const int32_t *offsets, int O, int32_t *counts, uint64_t *mass,
              uint64_t *tok_count, void *stream) {
  int T;
  Offsets off;
  if (!tp_args::update_shape_ok(B, S, k, N, F, V, O, ids_bits, &T) || !tp_args::offsets_ok(offsets, O, &off)) return MSAE_EINVAL;
  if (T == 0) return 0;
  if (!vals || !idx || !ids || !slot_of || !counts || !tok_count) return MSAE_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long M = (long)T * k;
  const int ids64 = ids_bits == 64;
  const dim3 grid(tp_args::chunks(M), (unsigned)O);
  if (mass)
    hipLaunchKernelGGL((tp_update_kernel<IdxT, true>), grid, dim3(256), 0, st, vals, idx, M, k, S, thresh, N, slot_of, F, V, ids,
                       ids64, off, counts, (unsigned long long *)mass);
  else
    hipLaunchKernelGGL((tp_update_kernel<IdxT, false>), grid, dim3(256), 0, st, vals, idx, M, k, S, thresh, N, slot_of, F, V, ids,
                       ids64, off, counts, (unsigned long long *)nullptr);
  hipLaunchKernelGGL(tp_tok_kernel, dim3(tp_args::chunks(T), (unsigned)O), dim3(256), 0, st, ids, ids64, T, S, V, off,
                     (unsigned long long *)tok_count);
  return msae_launch_status();
}

}  // namespace

extern "C" int msae_token_profile_update(const float *vals, const int32_t *idx, const void *ids, int ids_bits, int B, int S,
                                         int k, float thresh, int N, const int32_t *slot_of, int F, int V,
                                         const int32_t *offsets, int O, int32_t *counts, uint64_t *mass, uint64_t *tok_count,
                                         void *stream) {
  return tp_update(vals, idx, ids, ids_bits, B, S, k, thresh, N, slot_of, F, V, offsets, O, counts, mass, tok_count, stream);
}

extern "C" int msae_token_profile_update_i64(const float *vals, const int64_t *idx, const void *ids, int ids_bits, int B, int S,
                                             int k, float thresh, int N, const int32_t *slot_of, int F, int V,
                                             const int32_t *offsets, int O, int32_t *counts, uint64_t *mass,
                                             uint64_t *tok_count, void *stream) {
  return tp_update(vals, (const long long *)idx, ids, ids_bits, B, S, k, thresh, N, slot_of, F, V, offsets, O, counts, mass,
                   tok_count, stream);
}

extern "C" int msae_token_profile_topk(const int32_t *counts, const uint64_t *mass, const int64_t *tok_count, int F, int V, int m,
                                       int metric, int min_count, float *out_val, int32_t *out_tok, int64_t *out_total,
                                       void *stream) {
  if (!tp_args::topk_shape_ok(F, V, m, metric, min_count, mass != nullptr)) return MSAE_EINVAL;
  if (!counts || !tok_count || !out_val || !out_tok || !out_total) return MSAE_EINVAL;
  hipLaunchKernelGGL(tp_topk_kernel, dim3((unsigned)F), dim3(TP_TOPK_THREADS), 0, (hipStream_t)stream, counts,
                     (const unsigned long long *)mass, (const long long *)tok_count, V, m, metric, min_count, out_val, out_tok,
                     (long long *)out_total);
  return msae_launch_status();
}
