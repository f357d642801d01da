// jump_select.hip -- JumpReLU on top-C lists with learned per-feature thresholds (include/msae.h, "JumpReLU selection";
// DESIGN.md section 7s).
//
//   msae_jump_filter_f32   stable three-way partition of every row: kept (a >= theta_f), near (dropped, inside the STE band),
//                          rest; len, reach, the slot map src; integer counters l0 and n_saturated.
//   msae_jump_bwd_f32      the backward of that selection: the routing copy g -> g_in through src, and g_theta[f], the sum
//                          over the band entries of feature f of c = -fmaf(theta_f, g, s) / eps in a fixed order.
//
// No floating-point atomics anywhere.  The band entries are grouped by feature with a counting sort whose fill order is not
// fixed (an integer cursor per feature); every feature's run is then SORTED by (t, input slot) before it is summed, so the
// bits of g_theta are a function of the inputs alone.
#include "common.h"
#include "sortsel.h"
#include "wave_ops.h"

namespace {

constexpr int JUMP_MAX_C = 256;            // one wave per token, the row in 4 registers per lane
constexpr int JUMP_PK = JUMP_MAX_C / 64;

// the three classes of an entry (include/msae.h): 2 = kept, 1 = near, 0 = rest
template <typename IT>
__device__ __forceinline__ unsigned jump_class(float a, IT ix, const float *__restrict__ theta, int N, float h) {
  if (!(a > 0.f)) return 0u;               // NaN, -0.0, negatives
  if (ix < 0 || ix >= (IT)N) return 0u;    // the table is never read out of bounds
  const float th = theta[(int)ix];
  if (a >= th) return 2u;
  return (th - a < h) ? 1u : 0u;
}

// One wave per token.  Slot i = j * 64 + lane sits in key[j] as (value bits << 32 | class << 30 | i + 1); 0 = behind the row.
// Three ballot compactions (sortsel.h), each in list order: kept, near, rest.
template <typename IT>
__global__ __launch_bounds__(256) void jump_filter_kernel(const float *__restrict__ vals_in, const IT *__restrict__ idx_in, int T,
                                                          int C, size_t ld, const float *__restrict__ theta, int N, float h,
                                                          const float *__restrict__ floor_p, float *__restrict__ vals_out,
                                                          IT *__restrict__ idx_out, int32_t *__restrict__ len,
                                                          int32_t *__restrict__ reach, uint8_t *__restrict__ src,
                                                          unsigned long long *__restrict__ l0, int32_t *__restrict__ n_saturated) {
  __shared__ int s_kept[4], s_sat[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wave;
  int kept = 0, sat = 0;
  if (t < T) {                             // wave-uniform
    const float *vp = vals_in + (size_t)t * ld;
    const IT *ip = idx_in + (size_t)t * ld;
    float *vo = vals_out + (size_t)t * C;
    IT *io = idx_out + (size_t)t * C;
    uint8_t *so = src + (size_t)t * C;
    const int nj = (C + 63) >> 6;
    unsigned long long key[JUMP_PK];
#pragma unroll
    for (int j = 0; j < JUMP_PK; ++j) {
      const int i = j * 64 + lane;
      key[j] = 0ull;
      if (j < nj && i < C) {
        const float v = vp[i];
        const unsigned cls = jump_class<IT>(v, ip[i], theta, N, h);
        key[j] = ((unsigned long long)__float_as_uint(v) << 32) | (cls << 30) | (unsigned)(i + 1);
      }
    }
    const auto slot = [](unsigned long long k) { return (int)((unsigned)k & 0x3FFFFFFFu) - 1; };
    const auto cls_of = [](unsigned long long k) { return ((unsigned)k >> 30) & 3u; };
    kept = wave_compact_if<JUMP_PK>(
        key, nj, lane, [&](unsigned long long k) { return cls_of(k) == 2u; },
        [&](unsigned long long k, bool take, int pos) {
          if (take) { vo[pos] = __uint_as_float((unsigned)(k >> 32)); io[pos] = ip[slot(k)]; so[pos] = (uint8_t)slot(k); }
        });
    const int near = wave_compact_if<JUMP_PK>(
        key, nj, lane, [&](unsigned long long k) { return cls_of(k) == 1u; },
        [&](unsigned long long k, bool take, int pos) {
          if (take) { vo[kept + pos] = 0.f; io[kept + pos] = ip[slot(k)]; so[kept + pos] = (uint8_t)slot(k); }
        });
    const int front = kept + near;
    wave_compact_if<JUMP_PK>(
        key, nj, lane, [&](unsigned long long k) { return k != 0ull && cls_of(k) == 0u; },
        [&](unsigned long long k, bool take, int pos) {
          if (take) { vo[front + pos] = 0.f; io[front + pos] = ip[slot(k)]; so[front + pos] = (uint8_t)slot(k); }
        });
    if (lane == 0) {
      len[t] = kept;
      reach[t] = front;
      const float last = vp[C - 1];
      sat = (last > 0.f && last >= *floor_p) ? 1 : 0;
    }
  }
  // one integer atomic per workgroup and counter
  if (lane == 0) { s_kept[wave] = kept; s_sat[wave] = sat; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int k4 = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
    const int s4 = s_sat[0] + s_sat[1] + s_sat[2] + s_sat[3];
    if (l0 && k4) atomicAdd(l0, (unsigned long long)k4);
    if (n_saturated && s4) atomicAdd(n_saturated, s4);
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// Workspace layout (msae_jump_bwd_ws_bytes): counts int [N + 1] | offsets int [N + 1] | cursor int [N + 1] | pad to 8 bytes |
// ent u64 [T * C].  An entry of `ent` is ((t * C + input slot) << 32 | bits of c).
struct JumpWs {
  int *counts, *offsets, *cursor;
  unsigned long long *ent;
};

__host__ __device__ inline size_t jump_ints(int N) { return ((size_t)3 * ((size_t)N + 1) + 1) / 2 * 2; }

// One wave per token.  FILL = false: the routing copy and the per-feature band counts.  FILL = true: every band entry goes
// to its feature's run (integer cursor; the run is sorted afterwards).  Both walk the OUTPUT slots p < reach[t]: those are
// the valid entries (kept, then near), so the band test is fabsf(a - theta_f) < h alone.
template <typename IT, bool FILL>
__global__ __launch_bounds__(256) void jump_bwd_rows_kernel(const float *__restrict__ vals_in, const IT *__restrict__ idx_in,
                                                            int T, int C, size_t ld, const float *__restrict__ theta, int N,
                                                            float h, float eps, const uint8_t *__restrict__ src,
                                                            const int32_t *__restrict__ len, const int32_t *__restrict__ reach,
                                                            const float *__restrict__ g, const float *__restrict__ s_p,
                                                            float *__restrict__ g_in, int *__restrict__ counts,
                                                            int *__restrict__ cursor, unsigned long long *__restrict__ ent) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;                      // wave-uniform
  int L = len[t], R = reach[t];
  L = L < 0 ? 0 : (L > C ? C : L);
  R = R < L ? L : (R > C ? C : R);
  const float s = FILL ? *s_p : 0.f;
  for (int p = lane; p < C; p += 64) {
    const int i = (int)src[(size_t)t * C + p];
    if (i >= C) continue;                  // (a slot map that is none: nothing is read or written outside the row)
    const float gp = g[(size_t)t * C + p];
    if (!FILL) g_in[(size_t)t * C + i] = p < L ? gp : 0.f;
    if (p >= R) continue;
    const float a = vals_in[(size_t)t * ld + i];
    const IT ix = idx_in[(size_t)t * ld + i];
    if (!(a > 0.f) || ix < 0 || ix >= (IT)N) continue;
    const float th = theta[(int)ix];
    if (!(fabsf(a - th) < h)) continue;
    if (!FILL) {
      atomicAdd(counts + (int)ix, 1);
    } else {
      // one fused multiply-add, one division: a separately rounded product would leave an error of u |theta g|, which no
      // bound relative to |c| covers where theta g and s cancel
      const float c = -__builtin_fmaf(th, gp, s) / eps;
      const int pos = atomicAdd(cursor + (int)ix, 1);
      ent[pos] = ((unsigned long long)(unsigned)(t * C + i) << 32) | __float_as_uint(c);
    }
  }
}

__global__ __launch_bounds__(256) void jump_zero_kernel(int *p, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = 0;
}

// single workgroup: offsets[n] = exclusive prefix of counts[0, N), cursor = its copy, offsets[N] = the total.  A thread owns 8
// consecutive counts of a tile of 8192 (decode.hip's wgrad_scan_kernel pattern).
__global__ __launch_bounds__(1024) void jump_scan_kernel(const int *__restrict__ counts, int N, int *__restrict__ offsets,
                                                         int *__restrict__ cursor) {
  __shared__ int wave_tot[16];
  int carry = 0;
  for (int base = 0; base < N; base += 8192) {
    const int i0 = base + threadIdx.x * 8;
    int v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = i0 + e < N ? counts[i0 + e] : 0;
    int tot = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { const int c = v[e]; v[e] = tot; tot += c; }
    int all;
    const int excl = carry + block_excl_scan<16>(tot, wave_tot, &all);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (i0 + e < N) { offsets[i0 + e] = excl + v[e]; cursor[i0 + e] = excl + v[e]; }
    carry += all;
  }
  if (threadIdx.x == 0) offsets[N] = carry;
}

// Ascending sort of a[0, L) by ONE wave: a network whose comparators all point the same way (the first step of a merge stage
// mirrors the block, the rest are half-cleaners), so the slots >= L act as +inf without being stored.  sync() orders one
// step's writes before the next step's reads.
template <class Sync>
__device__ __forceinline__ void jump_sort_asc(unsigned long long *a, int L, int lane, Sync &&sync) {
  const int np = next_pow2(L);
  for (int size = 2; size <= np; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const bool flip = stride == (size >> 1);
      for (int i = lane; i < (np >> 1); i += 64) {
        const int blk = i / stride, off = i % stride;
        const int lo = blk * (stride << 1) + off;
        const int hi = flip ? blk * size + size - 1 - off : lo + stride;
        if (hi < L) {
          const unsigned long long x = a[lo], y = a[hi];
          if (x > y) { a[lo] = y; a[hi] = x; }
        }
      }
      sync();
    }
  }
}

constexpr int JUMP_LDS_SEG = 1024;         // entries a wave sorts in its LDS slice

// One wave per feature: the run sorted by (t, input slot) -- the upper word of an entry, unique --, then lane l adds the
// entries l, l + 64, ... in that order from +0 and the fixed xor butterfly of wave_sum joins the 64 partial sums.
__global__ __launch_bounds__(256) void jump_reduce_kernel(const int *__restrict__ offsets, unsigned long long *ent,
                                                          int N, float *__restrict__ g_theta) {
  __shared__ unsigned long long s_seg[4][JUMP_LDS_SEG];
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= N) return;                      // wave-uniform; no workgroup barrier below
  const int beg = offsets[f], L = offsets[f + 1] - beg;
  float acc = 0.f;
  if (L > 0 && L <= JUMP_LDS_SEG) {
    unsigned long long *seg = s_seg[threadIdx.x >> 6];
    for (int i = lane; i < L; i += 64) seg[i] = ent[beg + i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (L > 1)
      jump_sort_asc(seg, L, lane, [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); });
    for (int i = lane; i < L; i += 64) acc += __uint_as_float((unsigned)seg[i]);
  } else if (L > JUMP_LDS_SEG) {            // a feature inside the band on more than 1024 entries of the call: in place
    unsigned long long *seg = ent + beg;
    jump_sort_asc(seg, L, lane, [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent"); __builtin_amdgcn_wave_barrier(); });
    for (int i = lane; i < L; i += 64) acc += __uint_as_float((unsigned)seg[i]);
  }
  acc = wave_sum(acc);
  if (lane == 0) g_theta[f] = acc;
}

}  // namespace

template <typename IT>
static int jump_filter_launch(const float *vals_in, const IT *idx_in, int T, int C, int ld, const float *theta, int N, float h,
                              const float *floor_p, float *vals_out, IT *idx_out, int32_t *len, int32_t *reach, uint8_t *src,
                              int64_t *l0, int32_t *n_saturated, void *stream) {
  if (T < 0 || C < 1 || C > JUMP_MAX_C || ld < C || N < 1 || !theta || !floor_p || !(h > 0.f)) return MSAE_EINVAL;
  if (T == 0) return 0;
  if (!vals_in || !idx_in || !vals_out || !idx_out || !len || !reach || !src) return MSAE_EINVAL;
  hipLaunchKernelGGL(jump_filter_kernel<IT>, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, vals_in, idx_in,
                     T, C, (size_t)ld, theta, N, h, floor_p, vals_out, idx_out, len, reach, src,
                     reinterpret_cast<unsigned long long *>(l0), n_saturated);
  return msae_launch_status();
}

extern "C" int msae_jump_filter_f32(const float *vals_in, const int32_t *idx_in, int T, int C, int ld, const float *theta, int N,
                                    float h, const float *floor, float *vals_out, int32_t *idx_out, int32_t *len,
                                    int32_t *reach, uint8_t *src, int64_t *l0, int32_t *n_saturated, void *stream) {
  return jump_filter_launch<int32_t>(vals_in, idx_in, T, C, ld, theta, N, h, floor, vals_out, idx_out, len, reach, src, l0,
                                     n_saturated, stream);
}

extern "C" int msae_jump_filter_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int C, int ld, const float *theta,
                                        int N, float h, const float *floor, float *vals_out, int64_t *idx_out, int32_t *len,
                                        int32_t *reach, uint8_t *src, int64_t *l0, int32_t *n_saturated, void *stream) {
  return jump_filter_launch<int64_t>(vals_in, idx_in, T, C, ld, theta, N, h, floor, vals_out, idx_out, len, reach, src, l0,
                                     n_saturated, stream);
}

static bool jump_bwd_shape_ok(int T, int C, int N) {
  return T >= 1 && C >= 1 && C <= JUMP_MAX_C && N >= 1 && N < (1 << 30) && (long)T * C < (1l << 31);
}

extern "C" size_t msae_jump_bwd_ws_bytes(int T, int C, int N) {
  if (!jump_bwd_shape_ok(T, C, N)) return 0;
  return jump_ints(N) * sizeof(int) + (size_t)T * C * sizeof(unsigned long long);
}

template <typename IT>
static int jump_bwd_launch(const float *vals_in, const IT *idx_in, int T, int C, int ld, const float *theta, int N, float h,
                           float eps, const uint8_t *src, const int32_t *len, const int32_t *reach, const float *g,
                           const float *s, float *g_in, float *g_theta, void *ws, size_t ws_bytes, void *stream) {
  if (T == 0 && C >= 1 && C <= JUMP_MAX_C && N >= 1 && g_theta) {            // no entries: every feature gets +0.0
    hipLaunchKernelGGL(jump_zero_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<int *>(g_theta), N);
    return msae_launch_status();
  }
  if (!jump_bwd_shape_ok(T, C, N) || ld < C || !(h > 0.f) || !(eps > 0.f)) return MSAE_EINVAL;
  if (!vals_in || !idx_in || !theta || !src || !len || !reach || !g || !s || !g_in || !g_theta) return MSAE_EINVAL;
  if (!ws || ws_bytes < msae_jump_bwd_ws_bytes(T, C, N)) return MSAE_EWS;
  if (!msae_aligned(ws, 8)) return MSAE_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  JumpWs w;
  w.counts = reinterpret_cast<int *>(ws);
  w.offsets = w.counts + (N + 1);
  w.cursor = w.offsets + (N + 1);
  w.ent = reinterpret_cast<unsigned long long *>(w.counts + jump_ints(N));
  const dim3 rows((unsigned)((T + 3) / 4));
  hipLaunchKernelGGL(jump_zero_kernel, dim3(256), dim3(256), 0, st, w.counts, N + 1);
  hipLaunchKernelGGL((jump_bwd_rows_kernel<IT, false>), rows, dim3(256), 0, st, vals_in, idx_in, T, C, (size_t)ld, theta, N, h,
                     eps, src, len, reach, g, s, g_in, w.counts, w.cursor, w.ent);
  hipLaunchKernelGGL(jump_scan_kernel, dim3(1), dim3(1024), 0, st, w.counts, N, w.offsets, w.cursor);
  hipLaunchKernelGGL((jump_bwd_rows_kernel<IT, true>), rows, dim3(256), 0, st, vals_in, idx_in, T, C, (size_t)ld, theta, N, h,
                     eps, src, len, reach, g, s, g_in, w.counts, w.cursor, w.ent);
  hipLaunchKernelGGL(jump_reduce_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, w.offsets, w.ent, N, g_theta);
  return msae_launch_status();
}

extern "C" int msae_jump_bwd_f32(const float *vals_in, const int32_t *idx_in, int T, int C, int ld, const float *theta, int N,
                                 float h, float eps, const uint8_t *src, const int32_t *len, const int32_t *reach,
                                 const float *g, const float *s, float *g_in, float *g_theta, void *ws, size_t ws_bytes,
                                 void *stream) {
  return jump_bwd_launch<int32_t>(vals_in, idx_in, T, C, ld, theta, N, h, eps, src, len, reach, g, s, g_in, g_theta, ws,
                                  ws_bytes, stream);
}

extern "C" int msae_jump_bwd_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int C, int ld, const float *theta, int N,
                                     float h, float eps, const uint8_t *src, const int32_t *len, const int32_t *reach,
                                     const float *g, const float *s, float *g_in, float *g_theta, void *ws, size_t ws_bytes,
                                     void *stream) {
  return jump_bwd_launch<int64_t>(vals_in, idx_in, T, C, ld, theta, N, h, eps, src, len, reach, g, s, g_in, g_theta, ws,
                                  ws_bytes, stream);
}
