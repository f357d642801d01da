// train.hip -- the parameter-sized passes of one SAE optimisation step, fused.
//
// The reference trainer (train/sae/sae/trainer.py:347-414) runs, per step and per [N, d] matrix,
//   set_decoder_norm_to_unit_norm          sae.py:249-255   norm, +eps, div            3 passes
//   clip_grad_norm_(params, 1.0)           trainer.py:390   norm over all grads, g *= c 3 passes
//   remove_gradient_parallel_to_decoder... sae.py:257-271   (g*W).sum, g -= along*W     ~9 passes
//   Adam                                   trainer.py:395   p, g, m, v -> p, m, v       7 passes
// as separate torch ops: ~67 GB of HBM traffic at d=4096, N=131072.  Here:
//   unit_norm_rows   one read + one write of W_dec (the row is re-read from L2 for the scale)
//   grad_sumsq       one read of each gradient -> a device scalar (no host sync)
//   adam_rows        one pass: clip coefficient from the device scalar, optional removal of the
//                    row-parallel component, Adam moments and parameter update.  g is not written.
// ~38 GB.  All HBM-bound streaming kernels: 16-B accesses, one workgroup per row so the row's
// second touch (projection / scale) is an L2 hit.
#include "common.h"
#include "encode_defs.h"
#include "encode_prep.h"
#include "wave_ops.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float *red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();                 // red[] may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

// W[r][:] /= (||W[r][:]||_2 + eps)      (sae.py:252-255)
__global__ __launch_bounds__(256) void unit_norm_rows_kernel(float *__restrict__ W, int d, float eps) {
  __shared__ float red[4];
  float *row = W + (size_t)blockIdx.x * d;
  float ss = 0.f;
  if ((d & 3) == 0) {
    for (int c = threadIdx.x * 4; c < d; c += 1024) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(row + c);
      ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
  } else {
    for (int c = threadIdx.x; c < d; c += 256) ss += row[c] * row[c];
  }
  const float inv = 1.f / (sqrtf(block_sum(ss, red)) + eps);
  if ((d & 3) == 0) {
    for (int c = threadIdx.x * 4; c < d; c += 1024) {
      f32x4 v = *reinterpret_cast<const f32x4 *>(row + c);
      v[0] *= inv; v[1] *= inv; v[2] *= inv; v[3] *= inv;
      *reinterpret_cast<f32x4 *>(row + c) = v;
    }
  } else {
    for (int c = threadIdx.x; c < d; c += 256) row[c] *= inv;
  }
}

// *accum += sum(g[i]^2)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float *__restrict__ g, size_t n,
                                                         float *__restrict__ accum) {
  __shared__ float red[4];
  float ss = 0.f;
  const size_t n4 = n / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4 v = reinterpret_cast<const f32x4 *>(g)[i];
    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) ss += g[i] * g[i];
  const float s = block_sum(ss, red);
  if (threadIdx.x == 0) atomicAdd(accum, s);
}

struct AdamArgs {
  float lr, beta1, beta2, eps, max_norm;
  float bc1, bc2_sqrt;     // 1 - beta1^t, sqrt(1 - beta2^t)
  int project;
};

// torch's fused Adam arithmetic (aten/native/cuda/fused_adam_utils.cuh, no weight decay / amsgrad)
__device__ __forceinline__ void adam_update(float &w, float g, float &m, float &v, const AdamArgs &a) {
  m = m + (g - m) * (1.f - a.beta1);                 // lerp(m, g, 1 - beta1)
  v = a.beta2 * v + (1.f - a.beta2) * g * g;
  const float step_size = a.lr / a.bc1;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  w -= step_size * (m / denom);                      // addcdiv_(m, denom, -step_size)
}

// *accum += sum(v[0 .. n)) in a FIXED order (one workgroup: per-thread strided partial sums, then block_sum): the total of
// the per-row squared gradient norms the weight-gradient kernel wrote (msae_decode_bwd_wdec_f32: row_sumsq)
__global__ __launch_bounds__(1024) void sum_fixed_kernel(const float *__restrict__ v, size_t n, float *__restrict__ accum) {
  __shared__ float red[16];
  float ss = 0.f;
  const size_t n4 = n / 4;                               // (v comes from the caching allocator: 16-B aligned)
  for (size_t i = threadIdx.x; i < n4; i += 1024) {
    const f32x4 q = reinterpret_cast<const f32x4 *>(v)[i];
    ss += (q[0] + q[1]) + (q[2] + q[3]);
  }
  for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 1024) ss += v[i];
  const float t = block_sum(ss, red);
  if (threadIdx.x == 0) *accum += t;
}

// out[c] = scale * sum_n s[n] W[n][c]: the b_dec gradient of the sparse encoder backward, -sum_t sum_j g[t,j] W_enc[n_tj] =
// -(s^T W_enc) with s[n] = the summed latent gradients of feature n (msae_decode_bwd_wdec_f32: row_act_sum) -- ONE streaming read
// of W_enc instead of a k-row gather per token plus a sum over tokens.  Stage 1: workgroup b sums its 64 consecutive rows (ascending)
// into part[b][:]; stage 2 adds the partial rows up in a fixed order.  Bit-reproducible.
constexpr int WRS_ROWS = 64;       // rows per workgroup of stage 1
__global__ __launch_bounds__(256) void weighted_rows_part_kernel(const float *__restrict__ W, const float *__restrict__ sv, int N,
                                                                 int d, float *__restrict__ part) {
  __shared__ float s_w[WRS_ROWS];
  const int n0 = blockIdx.x * WRS_ROWS;
  if (threadIdx.x < WRS_ROWS) s_w[threadIdx.x] = n0 + (int)threadIdx.x < N ? sv[n0 + threadIdx.x] : 0.f;
  __syncthreads();
  const int rows = min(WRS_ROWS, N - n0);
  for (int c = threadIdx.x * 4; c < d; c += 1024) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float *base = W + (size_t)n0 * d + c;
    for (int r0 = 0; r0 < rows; r0 += 8) {            // eight rows' loads in flight per thread; rows with s == 0 are not read
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool live = r0 + u < rows && s_w[r0 + u] != 0.f;           // workgroup-uniform
        v[u] = live ? *reinterpret_cast<const f32x4 *>(base + (size_t)(r0 + u) * d) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {                    // ascending row order: a fixed summation order
        const float w = r0 + u < rows ? s_w[r0 + u] : 0.f;
        acc[0] = __builtin_fmaf(w, v[u][0], acc[0]); acc[1] = __builtin_fmaf(w, v[u][1], acc[1]);
        acc[2] = __builtin_fmaf(w, v[u][2], acc[2]); acc[3] = __builtin_fmaf(w, v[u][3], acc[3]);
      }
    }
    *reinterpret_cast<f32x4 *>(part + (size_t)blockIdx.x * d + c) = acc;
  }
}
// out[y][c] = scale * sum of part rows [y per, (y + 1) per) (blockIdx.y = y): run twice -- 2048 partial rows -> 64 -> 1 -- so that
// no thread walks more than 64 rows (one 16-block launch over 2048 rows took 0.22 ms)
__global__ __launch_bounds__(256) void weighted_rows_sum_kernel(const float *__restrict__ part, int groups, int per, int d,
                                                                float scale, float *__restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  const int b0 = blockIdx.y * per, b1 = min(groups, b0 + per);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;       // four interleaved partial sums (fixed assignment), then a fixed combine
  int b = b0;
  for (; b + 4 <= b1; b += 4) {
    a0 += part[(size_t)b * d + c]; a1 += part[(size_t)(b + 1) * d + c];
    a2 += part[(size_t)(b + 2) * d + c]; a3 += part[(size_t)(b + 3) * d + c];
  }
  for (; b < b1; ++b) a0 += part[(size_t)b * d + c];
  out[(size_t)blockIdx.y * d + c] = scale * ((a0 + a1) + (a2 + a3));
}

// ---- the optimiser row passes ------------------------------------------------------------------------------------------------
// One workgroup per row r of W, G and the moments [rows][d]:
//   c     = min(1, max_norm / (sqrt(*total_sumsq) + 1e-6))        (clip_grad_norm_)
//   g     = c * G[r][:]
//   g    -= <g, W[r][:]> * W[r][:]      if project                (sae.py:266-271, after clipping)
//   the optimiser's update of W[r] and its moments from g         (the update policies below)
// opt_rows_kernel is that pass alone, for any d.  opt_rows_fused_kernel (d % 4 == 0; the updated row stays in registers for
// d <= 8192) folds the NEXT step's passes over the same matrix in:
//   renorm_eps >= 0  W[r] /= |W[r]| + eps after the update: the trainer's set_decoder_norm_to_unit_norm at the top of the next
//                     step (sae.py:249-255, trainer.py:352) -- same arithmetic, reduction order and bits as unit_norm_rows_kernel,
//                     without its read + write of the 2 GiB matrix
//   REFRESH 1 / 2     the coarse-pass operands of the updated encoder row (int8: row statistics + quantised copies, as
//                     row_stats_quant_kernel<true>; bf16: statistics + the bf16 copy) into the prepared buffer -- what
//                     msae_encoder_refresh_for would rebuild with another sweep over W_enc before the next encode
struct FusedTail {
  float renorm_eps;
  RowQuantOut rq;
  unsigned short *wb, *ws;      // REFRESH 2: bf16 copy + bf16 sample rows
};

// ---- the steps of a row pass, one copy each ---------------------------------------------------------------------------------
// c = min(1, max_norm / (sqrt(*total_sumsq) + 1e-6)), 1 without a total
__device__ __forceinline__ float clip_coef(const float *__restrict__ total_sumsq, float max_norm) {
  float clip = 1.f;
  if (total_sumsq) {
    const float c = max_norm / (sqrtf(*total_sumsq) + 1e-6f);
    clip = c < 1.f ? c : 1.f;
  }
  return clip;
}
// <clip * G[r], W[r]> of the workgroup's row; vec4: d % 4 == 0, read 16 bytes at a time
__device__ __forceinline__ float row_along(const float *__restrict__ G, const float *__restrict__ W, size_t base, int d,
                                           float clip, bool vec4, float *red) {
  float dot = 0.f;
  if (vec4) {
    for (int c = threadIdx.x * 4; c < d; c += 1024) {
      const f32x4 g = *reinterpret_cast<const f32x4 *>(G + base + c);
      const f32x4 w = *reinterpret_cast<const f32x4 *>(W + base + c);
      dot += (g[0] * clip) * w[0] + (g[1] * clip) * w[1] + (g[2] * clip) * w[2] + (g[3] * clip) * w[3];
    }
  } else {
    for (int c = threadIdx.x; c < d; c += 256) dot += (G[base + c] * clip) * W[base + c];
  }
  return block_sum(dot, red);
}
// the updated row waits in registers for its norm: trip `it` of a thread is keep[it] (d <= 8192, checked by the host)
constexpr int KEEP = 8;
__device__ __forceinline__ void keep_put(f32x4 (&keep)[KEEP], int it, const f32x4 w) {
#pragma unroll
  for (int q = 0; q < KEEP; ++q) if (q == it) keep[q] = w;
}
__device__ __forceinline__ void renorm_store(float *__restrict__ W, size_t base, int d, const f32x4 (&keep)[KEEP], float inv) {
  int it = 0;
  for (int c = threadIdx.x * 4; c < d; c += 1024, ++it) {
    f32x4 v = keep[0];
#pragma unroll
    for (int q = 1; q < KEEP; ++q) if (q == it) v = keep[q];
    v[0] *= inv; v[1] *= inv; v[2] *= inv; v[3] *= inv;
    *reinterpret_cast<f32x4 *>(W + base + c) = v;
  }
}
// REFRESH 1 / 2: the coarse-pass operands of the row the workgroup has just written
template <int REFRESH>
__device__ __forceinline__ void refresh_row(float *__restrict__ W, size_t base, int d, const FusedTail &ft,
                                            float (&red3)[3][4]) {
  __threadfence_block();
  __syncthreads();                              // the whole updated row is visible to the workgroup (same CU, same L1)
  const int n = blockIdx.x;
  if constexpr (REFRESH == 1) {
    row_stats_quant_row<true>(W, n, d, ft.rq, red3);
  } else {
    row_stats_quant_row<false>(W, n, d, ft.rq, red3);
    const bool samp = (n % SAMPLE_STRIDE) == SAMPLE_OFF;
    for (int c = threadIdx.x * 4; c < d; c += 1024) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(W + base + c);
      u16x4 o;
      o[0] = f32_to_bf16_bits(v[0]); o[1] = f32_to_bf16_bits(v[1]); o[2] = f32_to_bf16_bits(v[2]); o[3] = f32_to_bf16_bits(v[3]);
      *reinterpret_cast<u16x4 *>(ft.wb + base + c) = o;
      if (samp) *reinterpret_cast<u16x4 *>(ft.ws + (size_t)(n / SAMPLE_STRIDE) * d + c) = o;
    }
  }
}

// ---- sign momentum ("lion" / "signum", include/msae.h) ----------------------------------------------------------
struct LionArgs {
  float lr, omb1, omb2, max_norm;      // omb = 1.f - beta, rounded once on the host's float32 values as the device would
  int project;
};

// u = lerp(m, g, 1 - beta1) is signed, m' = lerp(m, g, 1 - beta2) is carried: one subtraction and one explicit fma each, so
// that every variant of the kernel takes the same sign from the same g.  beta1 == beta2: u and m' are the same bits.
__device__ __forceinline__ void lion_update(float &w, float g, float &m, const LionArgs &a) {
  const float dgm = g - m;
  const float u = __builtin_fmaf(dgm, a.omb1, m);
  const float s = (float)((u > 0.f) - (u < 0.f));          // 0 for u == 0 and for NaN
  w = w - a.lr * s;
  m = __builtin_fmaf(dgm, a.omb2, m);
}

// ---- 8-bit moments ("adam8", include/msae.h) -------------------------------------------------------------------
// M8 = e4m3 codes of m, R8 = e4m3 codes of sqrt(v), one float32 scale (absmax / 448) per block of ADAM8_BLOCK consecutive
// elements of a row.  With one workgroup per row and one f32x4 per thread per trip, a block is what ONE WAVE holds in ONE TRIP:
// its absmax is a wave_max, its codes are one 32-bit word per lane, lane 0 writes the scales.
constexpr int ADAM8_BLOCK = 256;
constexpr float E4M3_MAX = 448.f;
struct Adam8Ptrs {
  unsigned *M8, *R8;            // the code arrays, addressed as words of four codes
  float *SM, *SR;
};
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ f32x4 unpack4_fp8(unsigned w) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  return f32x4{lo[0], lo[1], hi[0], hi[1]};
}
// codes of x * (448 / absmax), clamped to +-448 in float32, rounded to nearest even by the conversion instruction
__device__ __forceinline__ unsigned adam8_codes(const f32x4 x, float absmax) {
  const float inv = absmax > 0.f ? E4M3_MAX / absmax : 0.f;
  f32x4 q;
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] = fminf(fmaxf(x[e] * inv, -E4M3_MAX), E4M3_MAX);
  return (unsigned)pack4_fp8(q);
}
// One wave, one block: word `word` of the code arrays is this lane's (live lanes only; the others pass m = r = 0), block `blk`
// the wave's.  A positive r never becomes code 0 (it would turn a still-nonzero m / sqrt(v) into m / eps): code 1 instead.
__device__ __forceinline__ void adam8_store_block(const Adam8Ptrs &st, size_t word, size_t blk, bool live, const f32x4 m,
                                                  const f32x4 r) {
  const float am = wave_max(fmaxf(fmaxf(fabsf(m[0]), fabsf(m[1])), fmaxf(fabsf(m[2]), fabsf(m[3]))));
  const float ar = wave_max(fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])));
  if (live) {
    const unsigned cm = adam8_codes(m, am);
    unsigned cr = adam8_codes(r, ar);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (r[e] > 0.f && ((cr >> (8 * e)) & 0xFFu) == 0u) cr |= 1u << (8 * e);
    MSAE_ADAM_STORE(cm, st.M8 + word);
    MSAE_ADAM_STORE(cr, st.R8 + word);
  }
  if ((threadIdx.x & 63) == 0) {
    st.SM[blk] = am / E4M3_MAX;
    st.SR[blk] = ar / E4M3_MAX;
  }
}
// m = dec(M8) * SM, r = dec(R8) * SR, v = r * r: three separate float32 multiplications (the build has -ffp-contract=off)
__device__ __forceinline__ void adam8_load(const Adam8Ptrs &st, size_t word, size_t blk, f32x4 &m, f32x4 &v) {
  const float sm = st.SM[blk], sr = st.SR[blk];
  m = unpack4_fp8(MSAE_ADAM_LOAD(st.M8 + word)) * sm;
  const f32x4 r = unpack4_fp8(MSAE_ADAM_LOAD(st.R8 + word)) * sr;
  v = r * r;
}

// ---- update policies -------------------------------------------------------------------------------------------------------
// A policy names what differs between the optimisers: State (its moment pointers), Args (max_norm, project and its own
// constants), NMOM float32 moments per element in registers and update() of one element; for the fused kernel also trip(c, d)
// (does the thread whose columns start at c run this trip), at() (where that thread's moments lie, worked out once per trip)
// and load() / store() of one f32x4 of each moment, streaming.
template <int N>
struct F32Moments {               // N float32 moments stored as they are
  static constexpr int NMOM = N;
  struct State { float *mom[N]; };
  typedef size_t At;
  static __device__ __forceinline__ bool trip(int c, int d) { return c < d; }
  static __device__ __forceinline__ At at(size_t base, int c, int) { return base + c; }
  static __device__ __forceinline__ void load(const State &st, At p, f32x4 (&mo)[N]) {
    // the moments are touched exactly once per step: streaming accesses, kept out of the caches' way (MSAE_ADAM_PLAIN_LOADS
    // in a tuning build switches the hint off)
#pragma unroll
    for (int i = 0; i < N; ++i) mo[i] = MSAE_ADAM_LOAD(reinterpret_cast<const f32x4 *>(st.mom[i] + p));
  }
  static __device__ __forceinline__ void store(const State &st, At p, bool, const f32x4 (&mo)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) MSAE_ADAM_STORE(mo[i], reinterpret_cast<f32x4 *>(st.mom[i] + p));
  }
};
struct AdamOpt : F32Moments<2> {  // m, v.  28 bytes per element
  using Args = AdamArgs;
  static __device__ __forceinline__ void update(float &w, float g, float (&mo)[2], const Args &a) {
    adam_update(w, g, mo[0], mo[1], a);
  }
};
struct LionOpt : F32Moments<1> {  // one moment, no second-moment stream.  20 bytes per element
  using Args = LionArgs;
  static __device__ __forceinline__ void update(float &w, float g, float (&mo)[1], const Args &a) { lion_update(w, g, mo[0], a); }
};
// Adam with the moments carried in the adam8 format: decoded on the way in, the update computed from the float32 m', v' of this
// step, m' and sqrt(v') encoded on the way out.  A trip runs a whole wave at a time (the wave_max needs all 64 lanes): a wave
// whose block lies past d skips the trip, lanes past d inside a block contribute 0.
struct Adam8Opt {
  static constexpr int NMOM = 2;  // m, and v on the way in / sqrt(v') on the way out
  using State = Adam8Ptrs;
  using Args = AdamArgs;
  struct At { size_t word, blk; };  // the lane's word of the code arrays, the wave's block
  static __device__ __forceinline__ bool trip(int c, int d) { return (c & ~(ADAM8_BLOCK - 1)) < d; }
  static __device__ __forceinline__ At at(size_t base, int c, int d) {
    return At{(base + c) >> 2, (size_t)blockIdx.x * ((d + ADAM8_BLOCK - 1) / ADAM8_BLOCK) + (c >> 8)};
  }
  static __device__ __forceinline__ void load(const State &st, const At &p, f32x4 (&mo)[2]) {
    adam8_load(st, p.word, p.blk, mo[0], mo[1]);
  }
  static __device__ __forceinline__ void update(float &w, float g, float (&mo)[2], const Args &a) {
    adam_update(w, g, mo[0], mo[1], a);
    mo[1] = sqrtf(mo[1]);
  }
  static __device__ __forceinline__ void store(const State &st, const At &p, bool live, const f32x4 (&mo)[2]) {
    adam8_store_block(st, p.word, p.blk, live, mo[0], mo[1]);
  }
};

// one element: clip, projection, the policy's update
template <class Opt>
__device__ __forceinline__ void update_elem(float &w, float g, float (&mo)[Opt::NMOM], float clip, float along,
                                            const typename Opt::Args &a) {
  float ge = g * clip;
  if (a.project) ge -= along * w;
  Opt::update(w, ge, mo, a);
}
template <class Opt>
__device__ __forceinline__ void update_vec(f32x4 &w, const f32x4 g, f32x4 (&mo)[Opt::NMOM], float clip, float along,
                                           const typename Opt::Args &a) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float we = w[e], me[Opt::NMOM];
#pragma unroll
    for (int i = 0; i < Opt::NMOM; ++i) me[i] = mo[i][e];
    update_elem<Opt>(we, g[e], me, clip, along, a);
    w[e] = we;
#pragma unroll
    for (int i = 0; i < Opt::NMOM; ++i) mo[i][e] = me[i];
  }
}

// the pass alone, float32 moments: any d (d % 4 != 0: scalar loop), what the fused kernel does not take included
template <class Opt>
__global__ __launch_bounds__(256) void opt_rows_kernel(float *__restrict__ W, const float *__restrict__ G, typename Opt::State st,
                                                       int d, const float *__restrict__ total_sumsq, typename Opt::Args a) {
  __shared__ float red[4];
  const size_t base = (size_t)blockIdx.x * d;
  const float clip = clip_coef(total_sumsq, a.max_norm);
  const bool vec4 = (d & 3) == 0;
  const float along = a.project ? row_along(G, W, base, d, clip, vec4, red) : 0.f;
  if (vec4) {
    for (int c = threadIdx.x * 4; c < d; c += 1024) {
      const f32x4 g = *reinterpret_cast<const f32x4 *>(G + base + c);     // L2 hit when projecting
      f32x4 w = *reinterpret_cast<const f32x4 *>(W + base + c), mo[Opt::NMOM];
#pragma unroll
      for (int i = 0; i < Opt::NMOM; ++i) mo[i] = *reinterpret_cast<const f32x4 *>(st.mom[i] + base + c);
      update_vec<Opt>(w, g, mo, clip, along, a);
      *reinterpret_cast<f32x4 *>(W + base + c) = w;
#pragma unroll
      for (int i = 0; i < Opt::NMOM; ++i) *reinterpret_cast<f32x4 *>(st.mom[i] + base + c) = mo[i];
    }
  } else {
    for (int c = threadIdx.x; c < d; c += 256) {
      float w = W[base + c], mo[Opt::NMOM];
#pragma unroll
      for (int i = 0; i < Opt::NMOM; ++i) mo[i] = st.mom[i][base + c];
      update_elem<Opt>(w, G[base + c], mo, clip, along, a);
      W[base + c] = w;
#pragma unroll
      for (int i = 0; i < Opt::NMOM; ++i) st.mom[i][base + c] = mo[i];
    }
  }
}

template <class Opt, int REFRESH>
__global__ __launch_bounds__(256) void opt_rows_fused_kernel(float *__restrict__ W, const float *__restrict__ G,
                                                             typename Opt::State st, int d,
                                                             const float *__restrict__ total_sumsq, typename Opt::Args a,
                                                             FusedTail ft) {
  __shared__ float red[4];
  __shared__ float red3[3][4];
  const size_t base = (size_t)blockIdx.x * d;
  const float clip = clip_coef(total_sumsq, a.max_norm);
  const float along = a.project ? row_along(G, W, base, d, clip, true, red) : 0.f;
  const bool renorm = ft.renorm_eps >= 0.f;
  f32x4 keep[KEEP];
  float ss = 0.f;
  int it = 0;
  for (int c = threadIdx.x * 4; Opt::trip(c, d); c += 1024, ++it) {
    const bool live = c < d;                        // (always, where the trip is c < d)
    const typename Opt::At at = Opt::at(base, c, d);
    f32x4 w = {0.f, 0.f, 0.f, 0.f}, mo[Opt::NMOM] = {};
    if (live) {
      // the gradient is read once too, unless the projection has just read it
      const f32x4 g = a.project ? *reinterpret_cast<const f32x4 *>(G + base + c)     // L2 hit when projecting
                                : MSAE_ADAM_LOAD(reinterpret_cast<const f32x4 *>(G + base + c));
      w = *reinterpret_cast<const f32x4 *>(W + base + c);
      Opt::load(st, at, mo);
      update_vec<Opt>(w, g, mo, clip, along, a);
    }
    Opt::store(st, at, live, mo);
    if (live) {
      if (renorm) {
        keep_put(keep, it, w);
        ss += w[0] * w[0] + w[1] * w[1] + w[2] * w[2] + w[3] * w[3];
      } else {
        *reinterpret_cast<f32x4 *>(W + base + c) = w;
      }
    }
  }
  if (renorm) renorm_store(W, base, d, keep, 1.f / (sqrtf(block_sum(ss, red)) + ft.renorm_eps));
  if constexpr (REFRESH != 0) refresh_row<REFRESH>(W, base, d, ft, red3);
}

// float32 moments -> the adam8 format (checkpoints, switching precision on resume): one workgroup per row, as above
__global__ __launch_bounds__(256) void adam8_quantize_kernel(const float *__restrict__ M, const float *__restrict__ V,
                                                             Adam8Ptrs st, int d) {
  const size_t base = (size_t)blockIdx.x * d;
  const int bpr = (d + ADAM8_BLOCK - 1) / ADAM8_BLOCK;
  for (int c = threadIdx.x * 4; (c & ~(ADAM8_BLOCK - 1)) < d; c += 1024) {
    const bool live = c < d;
    f32x4 m = {0.f, 0.f, 0.f, 0.f}, r = m;
    if (live) {
      m = *reinterpret_cast<const f32x4 *>(M + base + c);
      const f32x4 v = *reinterpret_cast<const f32x4 *>(V + base + c);
      r = f32x4{sqrtf(v[0]), sqrtf(v[1]), sqrtf(v[2]), sqrtf(v[3])};
    }
    adam8_store_block(st, (base + c) >> 2, (size_t)blockIdx.x * bpr + (c >> 8), live, m, r);
  }
}
// ... and back: the values Adam8Opt computes with
__global__ __launch_bounds__(256) void adam8_dequantize_kernel(Adam8Ptrs st, float *__restrict__ M, float *__restrict__ V, int d) {
  const size_t base = (size_t)blockIdx.x * d;
  const int bpr = (d + ADAM8_BLOCK - 1) / ADAM8_BLOCK;
  for (int c = threadIdx.x * 4; c < d; c += 1024) {
    f32x4 m, v;
    adam8_load(st, (base + c) >> 2, (size_t)blockIdx.x * bpr + (c >> 8), m, v);
    *reinterpret_cast<f32x4 *>(M + base + c) = m;
    *reinterpret_cast<f32x4 *>(V + base + c) = v;
  }
}

}  // namespace

constexpr int WRS_MID = 64;        // partial rows after the first summation level
extern "C" size_t msae_weighted_row_sum_ws_bytes(int N, int d) {
  return (N > 0 && d > 0 && (d & 3) == 0) ? (size_t)((N + WRS_ROWS - 1) / WRS_ROWS + WRS_MID) * d * 4 : 0;
}

extern "C" int msae_weighted_row_sum_f32(const float *W, const float *s, int N, int d, float scale, float *out, void *ws,
                                         size_t ws_bytes, void *stream) {
  if (!W || !s || !out || N <= 0 || d <= 0 || (d & 3) != 0) return MSAE_EINVAL;
  if (!ws || ws_bytes < msae_weighted_row_sum_ws_bytes(N, d)) return MSAE_EWS;
  if (!msae_aligned(W, 16) || !msae_aligned(ws, 16)) return MSAE_EALIGN;
  float *part = static_cast<float *>(ws);
  const int groups = (N + WRS_ROWS - 1) / WRS_ROWS;
  hipLaunchKernelGGL(weighted_rows_part_kernel, dim3(groups), dim3(256), 0, (hipStream_t)stream, W, s, N, d, part);
  float *mid = part + (size_t)groups * d;
  const int per = (groups + WRS_MID - 1) / WRS_MID, n_mid = (groups + per - 1) / per;
  hipLaunchKernelGGL(weighted_rows_sum_kernel, dim3((d + 255) / 256, n_mid), dim3(256), 0, (hipStream_t)stream, part, groups, per, d,
                     1.f, mid);
  hipLaunchKernelGGL(weighted_rows_sum_kernel, dim3((d + 255) / 256, 1), dim3(256), 0, (hipStream_t)stream, mid, n_mid, n_mid, d,
                     scale, out);
  return msae_launch_status();
}

extern "C" int msae_sum_f32(const float *v, size_t n, float *accum, void *stream) {
  if (!v || !accum) return MSAE_EINVAL;
  if (!msae_aligned(v, 16)) return MSAE_EALIGN;
  if (n == 0) return 0;
  hipLaunchKernelGGL(sum_fixed_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, v, n, accum);
  return msae_launch_status();
}

extern "C" int msae_unit_norm_rows_f32(float *W, int N, int d, float eps, void *stream) {
  if (!W || N <= 0 || d <= 0) return MSAE_EINVAL;
  if ((d & 3) == 0 && !msae_aligned(W, 16)) return MSAE_EALIGN;
  hipLaunchKernelGGL(unit_norm_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, W, d, eps);
  return msae_launch_status();
}

extern "C" int msae_grad_sumsq_f32(const float *g, size_t n, float *accum, void *stream) {
  if (!g || !accum) return MSAE_EINVAL;
  if (!msae_aligned(g, 16)) return MSAE_EALIGN;
  if (n == 0) return 0;
  const size_t want = (n / 4 + 255) / 256;
  const int grid = (int)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, accum);
  return msae_launch_status();
}

// the host half the optimiser entry points share: Adam's constants ...
static AdamArgs adam_args(float max_norm, int project, float lr, float beta1, float beta2, float eps, int step) {
  AdamArgs a{};
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.max_norm = max_norm;
  a.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  a.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  a.project = project ? 1 : 0;
  return a;
}
// ... and the tail: the renorm switch, and for an encoder weight the header of its prepared buffer, the dither table and the
// kernel's output pointers.  *refresh = the kernel's REFRESH (0: no operands to build).
static int fused_tail(int rows, int d, float renorm_eps, void *prepared, int T_next, const msae_options *opts, hipStream_t s,
                      FusedTail *ft, int *refresh) {
  *ft = FusedTail{};
  ft->renorm_eps = renorm_eps >= 0.f ? renorm_eps : -1.f;
  *refresh = 0;
  if (!prepared) return 0;
  CallOpts co;
  if (!resolve_opts(opts, co)) return MSAE_EINVAL;
  if (!msae_aligned(prepared, 256)) return MSAE_EALIGN;
  const int N = rows;
  Prepared p = make_prepared(N, d);
  if (!p.S) {
    MSAE_HIP_TRY(hipMemcpyAsync(prepared, &p, sizeof(p), hipMemcpyHostToDevice, s));   // no fused path for this shape: header only
    return 0;
  }
  const bool i8 = co.mode == 1 && i8_shape_ok(N, d);
  const int modes = (i8 ? 2 : 1) | (T_next > 256 ? 4 : 0);     // as msae_encoder_refresh[_for]
  p.valid = prep_valid_bits(modes, N, d);
  p.dseed = i8 ? co.seed : 0ull;                                // (the shared dither of the int8 operands, encode_defs.h)
  MSAE_HIP_TRY(hipMemcpyAsync(prepared, &p, sizeof(p), hipMemcpyHostToDevice, s));
  unsigned char *base = static_cast<unsigned char *>(prepared);
  ft->rq = row_quant_out(base, p, modes, i8);
  ft->rq.seed = co.seed;                                        // msae_options::dither: this refresh's own seed
  if (p.dseed != 0ull)
    hipLaunchKernelGGL(sd_table_kernel, dim3(1), dim3(1024), 0, s, co.seed, d, reinterpret_cast<int *>(base + p.off_sdtab));
  ft->wb = reinterpret_cast<unsigned short *>(base + p.off_wb);
  ft->ws = reinterpret_cast<unsigned short *>(base + p.off_ws);
  *refresh = i8 ? 1 : 2;
  return 0;
}

// ... the fused pass: the tail, then the kernel of its REFRESH ...
template <class Opt>
static int fused_rows(float *W, const float *G, typename Opt::State st, int rows, int d, const float *total_sumsq,
                      const typename Opt::Args &a, float renorm_eps, void *prepared, int T_next, const msae_options *opts,
                      void *stream) {
  hipStream_t s = (hipStream_t)stream;
  FusedTail ft;
  int refresh;
  if (int rc = fused_tail(rows, d, renorm_eps, prepared, T_next, opts, s, &ft, &refresh)) return rc;
  const auto kernel = refresh == 1 ? opt_rows_fused_kernel<Opt, 1> : refresh == 2 ? opt_rows_fused_kernel<Opt, 2>
                                                                                    : opt_rows_fused_kernel<Opt, 0>;
  hipLaunchKernelGGL(kernel, dim3(rows), dim3(256), 0, s, W, G, st, d, total_sumsq, a, ft);
  return msae_launch_status();
}
// ... and the separate passes, for the shapes the fused kernel does not take (d % 4 != 0, d > 8192)
template <class Opt>
static int separate_passes(float *W, const float *G, typename Opt::State st, int rows, int d, const float *total_sumsq,
                           const typename Opt::Args &a, float renorm_eps, void *prepared, int T_next, const msae_options *opts,
                           void *stream) {
  hipLaunchKernelGGL(opt_rows_kernel<Opt>, dim3(rows), dim3(256), 0, (hipStream_t)stream, W, G, st, d, total_sumsq, a);
  if (int rc = msae_launch_status()) return rc;
  if (renorm_eps >= 0.f) { if (int rc = msae_unit_norm_rows_f32(W, rows, d, renorm_eps, stream)) return rc; }
  if (prepared) return T_next > 0 ? msae_encoder_refresh_for(W, rows, d, prepared, T_next, opts, stream)
                                  : msae_encoder_refresh(W, rows, d, prepared, opts, stream);
  return 0;
}
// the choice between the two
template <class Opt>
static int opt_rows(float *W, const float *G, typename Opt::State st, int rows, int d, const float *total_sumsq,
                    const typename Opt::Args &a, float renorm_eps, void *prepared, int T_next, const msae_options *opts,
                    void *stream) {
  return ((d & 3) == 0 && d <= 8192 ? fused_rows<Opt> : separate_passes<Opt>)(W, G, st, rows, d, total_sumsq, a, renorm_eps,
                                                                              prepared, T_next, opts, stream);
}

// always the plain kernel, whatever the shape
extern "C" int msae_adam_rows_f32(float *W, const float *G, float *M, float *V, int rows, int d,
                                  const float *total_sumsq, float max_norm, int project, float lr,
                                  float beta1, float beta2, float eps, int step, void *stream) {
  if (!W || !G || !M || !V || rows <= 0 || d <= 0 || step < 1) return MSAE_EINVAL;
  if ((d & 3) == 0 && !(msae_aligned(W, 16) && msae_aligned(G, 16) && msae_aligned(M, 16) && msae_aligned(V, 16)))
    return MSAE_EALIGN;
  return separate_passes<AdamOpt>(W, G, {{M, V}}, rows, d, total_sumsq, adam_args(max_norm, project, lr, beta1, beta2, eps, step),
                                  -1.f, nullptr, 0, nullptr, stream);
}

extern "C" int msae_adam_rows_fused_f32(float *W, const float *G, float *M, float *V, int rows, int d,
                                        const float *total_sumsq, float max_norm, int project, float lr,
                                        float beta1, float beta2, float eps, int step, float renorm_eps,
                                        void *prepared, int T_next, const msae_options *opts, void *stream) {
  if (!W || !G || !M || !V || rows <= 0 || d <= 0 || step < 1) return MSAE_EINVAL;
  if ((d & 3) == 0 && !(msae_aligned(W, 16) && msae_aligned(G, 16) && msae_aligned(M, 16) && msae_aligned(V, 16)))
    return MSAE_EALIGN;
  const AdamArgs a = adam_args(max_norm, project, lr, beta1, beta2, eps, step);
  return opt_rows<AdamOpt>(W, G, {{M, V}}, rows, d, total_sumsq, a, renorm_eps, prepared, T_next, opts, stream);
}

// ---- sign momentum --------------------------------------------------------------------------------------------------------------
// ONE entry, with or without tails: on a fused shape a call without tails and a call with them run the same kernel and compute
// the same W before the renorm and the same M.
extern "C" int msae_lion_rows_f32(float *W, const float *G, float *M, int rows, int d, const float *total_sumsq,
                                  float max_norm, int project, float lr, float beta1, float beta2, float renorm_eps,
                                  void *prepared, int T_next, const msae_options *opts, void *stream) {
  if (!W || !G || !M || rows <= 0 || d <= 0) return MSAE_EINVAL;
  if ((d & 3) == 0 && !(msae_aligned(W, 16) && msae_aligned(G, 16) && msae_aligned(M, 16))) return MSAE_EALIGN;
  LionArgs a{};
  a.lr = lr; a.omb1 = 1.f - beta1; a.omb2 = 1.f - beta2; a.max_norm = max_norm;
  a.project = project ? 1 : 0;
  return opt_rows<LionOpt>(W, G, {{M}}, rows, d, total_sumsq, a, renorm_eps, prepared, T_next, opts, stream);
}

// ---- 8-bit moments -------------------------------------------------------------------------------------------------------------
// what the kernels take: f32x4 rows inside the KEEP window.  A one-row view that is no multiple of 1024 long is what a vector gets
// whose length does not divide (ops.adam_rows_): the whole parameter would be ONE workgroup's -- such a parameter keeps float32
// moments.
static bool adam8_kernel_shape(int rows, int d) {
  return rows > 0 && d > 0 && (d & 3) == 0 && d <= 8192 && !(rows == 1 && (d & 1023) != 0);
}
static size_t adam8_nb(int rows, int d) { return (size_t)rows * ((d + ADAM8_BLOCK - 1) / ADAM8_BLOCK); }

extern "C" size_t msae_adam8_blocks(int rows, int d) {
  if (!adam8_kernel_shape(rows, d) || (size_t)rows * d < 4096) return 0;      // (the floor is policy: small parameters stay float32)
  return adam8_nb(rows, d);
}

static int adam8_check(const void *M8, const void *R8, const void *SM, const void *SR, int rows, int d) {
  if (!M8 || !R8 || !SM || !SR || rows <= 0 || d <= 0) return MSAE_EINVAL;
  if (!adam8_kernel_shape(rows, d)) return MSAE_ENOTIMPL;
  if (!(msae_aligned(M8, 16) && msae_aligned(R8, 16) && msae_aligned(SM, 4) && msae_aligned(SR, 4))) return MSAE_EALIGN;
  return 0;
}

extern "C" int msae_adam8_rows_f32(float *W, const float *G, uint8_t *M8, uint8_t *R8, float *SM, float *SR, int rows, int d,
                                   const float *total_sumsq, float max_norm, int project, float lr, float beta1,
                                   float beta2, float eps, int step, float renorm_eps, void *prepared, int T_next,
                                   const msae_options *opts, void *stream) {
  if (!W || !G || step < 1) return MSAE_EINVAL;
  if (int rc = adam8_check(M8, R8, SM, SR, rows, d)) return rc;
  if (!(msae_aligned(W, 16) && msae_aligned(G, 16))) return MSAE_EALIGN;
  const Adam8Ptrs st{reinterpret_cast<unsigned *>(M8), reinterpret_cast<unsigned *>(R8), SM, SR};
  return fused_rows<Adam8Opt>(W, G, st, rows, d, total_sumsq, adam_args(max_norm, project, lr, beta1, beta2, eps, step),
                              renorm_eps, prepared, T_next, opts, stream);
}

extern "C" int msae_adam8_quantize_f32(const float *M, const float *V, uint8_t *M8, uint8_t *R8, float *SM, float *SR, int rows,
                                       int d, void *stream) {
  if (!M || !V) return MSAE_EINVAL;
  if (int rc = adam8_check(M8, R8, SM, SR, rows, d)) return rc;
  if (!(msae_aligned(M, 16) && msae_aligned(V, 16))) return MSAE_EALIGN;
  const Adam8Ptrs st{reinterpret_cast<unsigned *>(M8), reinterpret_cast<unsigned *>(R8), SM, SR};
  hipLaunchKernelGGL(adam8_quantize_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, M, V, st, d);
  return msae_launch_status();
}

extern "C" int msae_adam8_dequantize_f32(const uint8_t *M8, const uint8_t *R8, const float *SM, const float *SR, float *M,
                                         float *V, int rows, int d, void *stream) {
  if (!M || !V) return MSAE_EINVAL;
  if (int rc = adam8_check(M8, R8, SM, SR, rows, d)) return rc;
  if (!(msae_aligned(M, 16) && msae_aligned(V, 16))) return MSAE_EALIGN;
  const Adam8Ptrs st{reinterpret_cast<unsigned *>(const_cast<uint8_t *>(M8)), reinterpret_cast<unsigned *>(const_cast<uint8_t *>(R8)),
                     const_cast<float *>(SM), const_cast<float *>(SR)};
  hipLaunchKernelGGL(adam8_dequantize_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, st, M, V, d);
  return msae_launch_status();
}
