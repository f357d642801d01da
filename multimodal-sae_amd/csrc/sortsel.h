// sortsel.h -- sort and select primitives on 64-bit keys that rank by descending value (common.h's rank keys: value word above,
// index word below; 0 = empty, the smallest key) for every kernel that orders a list: the stages behind the candidate GEMM
// (encode_rescore.h, encode_small.h), the row top-k and the shard merge (topk.hip), the cache records (sparsify.hip) and the
// list edits (edit_topk.hip).  Bitonic sorts of an LDS array by one wave or one workgroup, in LDS or in registers; a lookup in
// a sorted array; ballot counts and compaction of keys held in registers.
#pragma once
#include "common.h"

namespace {

// Bitonic sort (descending) of the n = power-of-two u64 keys of the LDS array s by ALL threads of the workgroup: NT of them, or
// blockDim.x where NT = 0 (a launch that sizes the workgroup at run time); tid = the caller's index among them.  The one LDS
// compare-exchange loop of the library.  Barriers: one in front of every step -- so whoever filled s[] needs none of their own
// -- and one behind the last: the sorted keys are visible to every thread.  n must be uniform over the workgroup.
template <int NT>
__device__ __forceinline__ void bitonic_sort_desc_u64(unsigned long long *s, int n, int tid) {
  const int nt = NT ? NT : (int)blockDim.x;
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (n >> 1); i += nt) {
        const int lo = (i / stride) * (stride << 1) + (i % stride), hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const unsigned long long x = s[lo], y = s[hi];
        if ((x < y) == desc) { s[lo] = y; s[hi] = x; }
      }
    }
  __syncthreads();
}

// The same order for <= 64 R keys by ONE wave in registers: key i = r * 64 + lane sits in v[r]; partners 64 or more apart are
// the lane's own registers, closer ones another lane's (two 32-bit shuffles).  No LDS traffic, no barriers: a 64-key sort is
// 21 compare-exchange steps of ~10 instructions (the LDS version: 21 barriers, ~10 k cycles for a wave that is alone).
template <int R>
__device__ __forceinline__ void wave_sort_desc_u64_regs(unsigned long long (&v)[R], int lane) {
#pragma unroll
  for (int size = 2; size <= 64 * R; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride >= 64) {
        const int rs = stride >> 6;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if ((r & rs) == 0) {
            const bool desc = (((r * 64 + lane) & size) == 0);
            const unsigned long long a = v[r], b = v[r | rs];
            if ((a < b) == desc) { v[r] = b; v[r | rs] = a; }
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = r * 64 + lane;
          const unsigned lo = __shfl_xor((unsigned)v[r], stride, 64), hi = __shfl_xor((unsigned)(v[r] >> 32), stride, 64);
          const unsigned long long o = ((unsigned long long)hi << 32) | lo;
          // the lower index of a pair keeps the larger key where the block sorts descending
          const bool lower = (lane & stride) == 0, desc = ((i & size) == 0);
          const bool take_max = lower == desc;
          v[r] = take_max ? (v[r] > o ? v[r] : o) : (v[r] < o ? v[r] : o);
        }
      }
    }
}

// ... and for 64 NW R keys by a WORKGROUP of NW waves: key i = tid * R + r sits in v[r] of thread tid.  Partners closer than R
// are the thread's own registers, up to 32 R apart another lane's (shuffles), farther another wave's: those few steps
// (3 of 66 for 2048 keys) go through `xch` (LDS, 64 NW R keys) behind barriers.  All threads call.
template <int NW, int R>
__device__ __forceinline__ void wg_sort_desc_u64_regs(unsigned long long (&v)[R], int tid, unsigned long long *xch) {
  constexpr int M = 64 * NW * R;
#pragma unroll
  for (int size = 2; size <= M; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (stride < R) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if ((r & stride) == 0) {
            const bool desc = (((tid * R + r) & size) == 0);
            const unsigned long long a = v[r], b = v[r | stride];
            if ((a < b) == desc) { v[r] = b; v[r | stride] = a; }
          }
        }
      } else {
        const int pt = stride / R;                         // partner thread = tid ^ pt
        const bool lower = (tid & pt) == 0;
        if (pt >= 64) {
          __syncthreads();
#pragma unroll
          for (int r = 0; r < R; ++r) xch[tid * R + r] = v[r];
          __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          unsigned long long o;
          if (pt >= 64) o = xch[(tid ^ pt) * R + r];
          else o = ((unsigned long long)__shfl_xor((unsigned)(v[r] >> 32), pt, 64) << 32) | __shfl_xor((unsigned)v[r], pt, 64);
          const bool desc = (((tid * R + r) & size) == 0);
          const bool take_max = lower == desc;
          v[r] = take_max ? (v[r] > o ? v[r] : o) : (v[r] < o ? v[r] : o);
        }
      }
    }
}

// s[0, 64 NW R) sorted descending through R registers per thread: the keys at and behind n count as empty and come back as 0.
// Barriers: one in front (whoever wrote s[] is done), one behind (the sorted keys are published); all threads call.
template <int NW, int R>
__device__ __forceinline__ void lds_sort_desc_u64_regs(unsigned long long *s, int n, int tid) {
  __syncthreads();
  unsigned long long v[R];
  // one wave: key r * 64 + lane, a lane reads and writes its own slots only; a workgroup: key tid * R + r, s[] = the exchange buffer
  const auto at = [tid](int r) { return NW == 1 ? r * 64 + tid : tid * R + r; };
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = at(r) < n ? s[at(r)] : 0ull;
  if constexpr (NW == 1) wave_sort_desc_u64_regs<R>(v, tid);
  else { wg_sort_desc_u64_regs<NW, R>(v, tid, s); __syncthreads(); }
#pragma unroll
  for (int r = 0; r < R; ++r) s[at(r)] = v[r];
  __syncthreads();
}

// The first n (a power of two) keys of the LDS array s[0, slots) sorted descending by the workgroup of NW waves that calls it,
// barriers included (see lds_sort_desc_u64_regs).  In registers where the keys fit into RMAX per thread and the array has the
// slots a register sort writes back -- one wave: 64 keys (RMAX >= 1) or 128 (RMAX >= 2); four waves: 1024 keys (RMAX >= 4: 55
// stages instead of the 66 of 2048) or 2048 (RMAX >= 8) --, else in LDS.  RMAX = 0: always in LDS.
// n, slots are wave-uniform at every call site, so the barriers are not in divergent code.  Precondition: n <= slots (the LDS
// sort takes the smaller of the two only so that a caller's mistake stays inside the array: the result is then not a sort).
template <int NW, int RMAX>
__device__ __forceinline__ void lds_sort_desc_u64(unsigned long long *s, int n, int slots, int tid) {
  if constexpr (NW == 1 && RMAX >= 1) { if (n <= 64 && slots >= 64) { lds_sort_desc_u64_regs<1, 1>(s, n, tid); return; } }
  if constexpr (NW == 1 && RMAX >= 2) { if (n <= 128 && slots >= 128) { lds_sort_desc_u64_regs<1, 2>(s, n, tid); return; } }
  if constexpr (NW == 4 && RMAX >= 4) { if (n <= 1024 && slots >= 1024) { lds_sort_desc_u64_regs<4, 4>(s, n, tid); return; } }
  if constexpr (NW == 4 && RMAX >= 8) { if (n <= 2048 && slots >= 2048) { lds_sort_desc_u64_regs<4, 8>(s, n, tid); return; } }
  bitonic_sort_desc_u64<64 * NW>(s, n < slots ? n : slots, tid);
}

// number of keys (sorted descending, value in the upper 32 bits as an order key) whose value is >= v
__device__ __forceinline__ int count_ge(const unsigned long long *keys, int n, float v) {
  const unsigned tk = f32_order_key(v);
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned)(keys[mid] >> 32) >= tk) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- a list of <= 64 PK keys in the registers of ONE wave: key i = j * 64 + lane in kreg[j] ----------------------------------
// The first nj = ceil(n / 64) slots are in use (wave-uniform); empty places hold 0.
template <int PK>
__device__ __forceinline__ void wave_load_keys(unsigned long long (&kreg)[PK], const unsigned long long *__restrict__ src, int n,
                                               int nj, int lane) {
#pragma unroll
  for (int j = 0; j < PK; ++j) kreg[j] = (j < nj && j * 64 + lane < n) ? src[j * 64 + lane] : 0ull;
}
// how many of them satisfy pred (which must be false for 0): one ballot per key slot, one branch per eight slots
template <int PK, class Pred>
__device__ __forceinline__ int wave_count_if(const unsigned long long (&kreg)[PK], int nj, Pred pred) {
  static_assert(PK % 8 == 0, "eight key slots per branch");
  int c = 0;
#pragma unroll
  for (int jb = 0; jb < PK; jb += 8) {
    if (jb < nj) {
#pragma unroll
      for (int j = jb; j < jb + 8; ++j) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(pred(kreg[j])));
    }
  }
  return c;
}
// compaction by ballot prefix: visit(key, take, pos) for every key of the slots in use; the keys with take = pred(key) get the
// positions 0, 1, ... in list order.  Returns how many were taken.
template <int PK, class Pred, class Visit>
__device__ __forceinline__ int wave_compact_if(const unsigned long long (&kreg)[PK], int nj, int lane, Pred pred, Visit visit) {
  int base = 0;
#pragma unroll
  for (int j = 0; j < PK; ++j) {
    if (j < nj) {
      const bool take = pred(kreg[j]);
      const unsigned long long m = __builtin_amdgcn_ballot_w64(take);
      visit(kreg[j], take, base + __builtin_popcountll(m & ((1ull << lane) - 1ull)));
      base += __builtin_popcountll(m);
    }
  }
  return base;
}

}  // namespace
