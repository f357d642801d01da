// pos_profile.hip -- per-feature position profiles, updated from the cache loop's top-k, and the peak bin read from them
// (include/msae.h: msae_pos_profile_*).
//
// Position s of a row falls into bin pos_bin[s] (s < L) or tail_bin (s >= L); a bin outside [0, P) is counted nowhere.  A kept
// entry (v, f) (|v| > thresh, 0 <= f < N: pool_keep, the cache's rule) at a position with bin b is counted iff v > 0:
//   count[f][b] += 1                                                                                   int32 atomics
//   mass[f][b]  += q(v), q = the value in units of 2^-20, rounded half to even, at most 2^60           u64 atomics (mod 2^64)
// Integer adds commute: the state is the same bits whatever the order of the adds, the cut into calls or their order.
//
// pp_update_kernel: act_hist.hip's token kernel with a second payload.  A workgroup takes PP_ENTRIES consecutive entries (32
// tokens at k = 32), one lane per entry and round, and first adds its (feature, bin) pairs into an LDS table (open addressing,
// at most half full; ds_add_u32 / ds_add_u64); then every used slot issues ONE global atomic pair.  A feature that fires on
// every token of one bin (a BOS feature) costs T * k / PP_ENTRIES adds on its two addresses instead of T.
//
// pp_summary_kernel: one wave per feature (grid-stride).  Lane l walks the bins l, l + 64, .. in ascending order and keeps the
// first one of the highest RATE count[f][b] / bin_positions[b], compared by cross-multiplication in int64 (both factors below
// 2^31); a wave reduction joins the lanes (equal rates: the lower bin).
#include "pool_segments.h"
#include "pos_q.h"
#include "wave_ops.h"

namespace {

constexpr int PP_MAX_L = 65536, PP_MAX_P = 1024;

// q(v): pp_q of pos_q.h, shared with the token profiles

struct PpTable {       // where a position falls
  const int32_t *pos_bin;
  int L, tail_bin, P, S;
  __device__ __forceinline__ int bin(int s) const {
    const int b = s < L ? pos_bin[s] : tail_bin;
    return (unsigned)b < (unsigned)P ? b : -1;
  }
};

constexpr int PP_ENTRIES = 1024;                    // entries per workgroup
constexpr int PP_SLOTS = 2 * PP_ENTRIES;            // table slots: a power of two, never more than half full
constexpr int PP_SLOT_BITS = 11;
static_assert(1 << PP_SLOT_BITS == PP_SLOTS && PP_ENTRIES % 256 == 0, "table size");
static_assert((long)POOL_MAX_N * PP_MAX_P <= (1l << 30), "a key f * P + bin is a non-negative int");

__global__ __launch_bounds__(256) void pp_update_kernel(const float *__restrict__ vals, const int32_t *__restrict__ idx, long M,
                                                        int k, float thresh, int N, PpTable tab, int *__restrict__ count,
                                                        unsigned long long *__restrict__ mass) {
  __shared__ int s_key[PP_SLOTS];                   // f * P + bin (< 2^28), -1 = free
  __shared__ int s_cnt[PP_SLOTS];
  __shared__ unsigned long long s_mass[PP_SLOTS];
  for (int s = threadIdx.x; s < PP_SLOTS; s += 256) {
    s_key[s] = -1;
    s_cnt[s] = 0;
    s_mass[s] = 0ull;
  }
  __syncthreads();
  const long base = (long)blockIdx.x * PP_ENTRIES;
  for (int e = 0; e < PP_ENTRIES; e += 256) {
    const long i = base + e + threadIdx.x;
    if (i >= M) break;
    const float v = vals[i];
    const int f = idx[i];
    if (pool_keep(v, f, thresh, N) && v > 0.f) {
      const int b = tab.bin((int)((i / k) % tab.S));
      if (b >= 0) {
        const int key = f * tab.P + b;
        unsigned slot = ((unsigned)key * 2654435761u) >> (32 - PP_SLOT_BITS);
        for (;;) {                                  // linear probing; a free slot exists: <= PP_ENTRIES keys
          const int prev = atomicCAS(&s_key[slot], -1, key);
          if (prev == -1 || prev == key) break;
          slot = (slot + 1) & (PP_SLOTS - 1);
        }
        atomicAdd(&s_cnt[slot], 1);
        atomicAdd(&s_mass[slot], pp_q(v));
      }
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < PP_SLOTS; s += 256) {
    const int c = s_cnt[s];
    if (c) {
      atomicAdd(count + s_key[s], c);
      atomicAdd(mass + s_key[s], s_mass[s]);
    }
  }
}

struct PpPeak {        // a bin and its rate c / n; (-1, 0, 1): none yet, rate 0
  int bin;
  long long c, n;
};

// is a's rate higher than b's, or equal with the lower bin?
__device__ __forceinline__ bool pp_better(const PpPeak &a, const PpPeak &b) {
  const long long l = a.c * b.n, r = b.c * a.n;
  return l > r || (l == r && a.bin < b.bin);
}

__global__ __launch_bounds__(256) void pp_summary_kernel(const int *__restrict__ count, const long long *__restrict__ bin_positions,
                                                         int N, int P, long long *__restrict__ fired, int *__restrict__ peak) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), waves = (int)(gridDim.x * 4u);
  for (int f = wave; f < N; f += waves) {
    const int *row = count + (size_t)f * P;
    PpPeak best{-1, 0, 1};
    long long tot = 0;
    for (int b = lane; b < P; b += 64) {
      const long long c = row[b], n = bin_positions[b];
      tot += c;
      if (n > 0 && c * best.n > best.c * n) best = PpPeak{b, c, n};      // strictly higher: the first bin of a rate stays
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      tot += __shfl_xor(tot, o, 64);
      const PpPeak other{__shfl_xor(best.bin, o, 64), __shfl_xor(best.c, o, 64), __shfl_xor(best.n, o, 64)};
      if (other.bin >= 0 && (best.bin < 0 || pp_better(other, best))) best = other;
    }
    if (lane == 0) {
      fired[f] = tot;
      peak[2 * (size_t)f] = best.bin;
      peak[2 * (size_t)f + 1] = (int)best.c;
    }
  }
}

inline bool pp_table_ok(int L, int tail_bin, int P) {
  return L >= 1 && L <= PP_MAX_L && P >= 1 && P <= PP_MAX_P && tail_bin >= -1 && tail_bin < P;
}

}  // namespace

extern "C" size_t msae_pos_profile_ws_bytes(int T, int k, int N) {
  (void)T, (void)k, (void)N;
  return 0;                                         // the table lives in LDS: no scratch for any shape
}

extern "C" int msae_pos_profile_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N,
                                       const int32_t *pos_bin, int L, int tail_bin, int P, int32_t *count, uint64_t *mass,
                                       void *ws, size_t ws_bytes, void *stream) {
  int T;
  if (!pool_tokens(B, S, &T) || !pool_shape_ok(T, k, N) || !pp_table_ok(L, tail_bin, P)) return MSAE_EINVAL;
  (void)ws, (void)ws_bytes;                         // none is needed, so none can be short: MSAE_EWS is never returned
  if (T == 0) return 0;
  if (!vals || !idx || !pos_bin || !count || !mass) return MSAE_EINVAL;
  const long M = (long)T * k;
  const unsigned blocks = (unsigned)((M + PP_ENTRIES - 1) / PP_ENTRIES);
  hipLaunchKernelGGL(pp_update_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, vals, idx, M, k, thresh, N,
                     PpTable{pos_bin, L, tail_bin, P, S}, count, (unsigned long long *)mass);
  return msae_launch_status();
}

extern "C" int msae_pos_profile_summary(const int32_t *count, const int64_t *bin_positions, int N, int P, int64_t *fired,
                                        int32_t *peak, void *stream) {
  if (N <= 0 || N > POOL_MAX_N || P < 1 || P > PP_MAX_P) return MSAE_EINVAL;
  if (!count || !bin_positions || !fired || !peak) return MSAE_EINVAL;
  const unsigned need = (unsigned)((N + 3) / 4);
  hipLaunchKernelGGL(pp_summary_kernel, dim3(need < 4096u ? need : 4096u), dim3(256), 0, (hipStream_t)stream, count,
                     (const long long *)bin_positions, N, P, (long long *)fired, peak);
  return msae_launch_status();
}
