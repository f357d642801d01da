// probe.hip -- fused segment-pooled feature ranking and activation maps (Sae.probe; reference
// tools/probe_activations.py:109-126: latents = pre_acts(h); latents.mean(0).topk(k); latents[:, :, idx]).
//
// pooled_f32_kernel: out[s][n] = mean (or max) over the tokens of segment s of v[t][n] = relu((x[t] - b_dec) W_enc[n]^T + b_enc[n]).
// The tile is pre_acts_f32_kernel's (f32_tile.h: same staging, same ascending-k v_mfma_f32_32x32x2_f32 chain, same `+ b_enc`
// and ReLU), so every v[t][n] is bit-identical to msae_pre_acts_f32's output; only the epilogue differs: the ReLU'd 128 x 128
// tile goes into the (then free) staging LDS and 128 threads, one per feature column, walk its rows in ascending token order,
// each adding into an f64 register that lives across the tiles of the workgroup's chunk and is written out at every segment
// end.  The dense [T][N] latents never reach HBM.
//
// Work split: a workgroup owns one 128-feature strip and one CHUNK, a run of consecutive segments whose tokens it walks in
// 128-token tiles (tiles are packed across the segment boundaries inside a chunk: 8 x 576 tokens are 36 tiles, not 40).  A
// segment is never split between chunks, so every segment's sum is ONE ascending-token f64 chain whatever the chunking: the
// result of a segment does not depend on the chunk plan, on the tile packing or on the other segments of the batch.
// Chunks are planned on the host (msae/sae/probe.py: balanced by token count, cut at gaps) or, with device-side segments and
// no plan, one per segment.  Tokens outside every segment are never loaded.
//
// probe_maps_kernel: maps[t][j] = v[t][idx[s][j]] for the tokens t of segment s, recomputed as ONE sequential ascending-k fmaf
// chain per (token, j) -- one lane per j, the token's centred row wave-uniform (encode_rescore.h's chain) -- which is the
// MFMA chain's arithmetic step for step, so the maps equal pre_acts's values bit for bit.  Tokens outside every segment: 0.
#include <algorithm>

#include "f32_tile.h"

namespace {

constexpr int P_PITCH = F_BN + 1;     // the ReLU'd tile in LDS: [128 tokens][129 floats] (66 KB of the 73.7 KB staging area)
static_assert(F_BM * P_PITCH <= F_LDS_FLOATS, "the pooled tile must fit the staging LDS");

// segment s clamped to [0, T); an empty (or inverted) segment becomes [e, e)
__device__ __forceinline__ int2 seg_clamped(const int32_t *seg, int s, int T) {
  int b = seg[2 * s], e = seg[2 * s + 1];
  b = b < 0 ? 0 : (b > T ? T : b);
  e = e < b ? b : (e > T ? T : e);
  return make_int2(b, e);
}

template <int DT, bool VEC>
__global__ __launch_bounds__(F_THREADS, 2) void pooled_f32_kernel(
    const void *__restrict__ x, const float *__restrict__ W, const float *__restrict__ b_enc,
    const float *__restrict__ b_dec, int T, int d, int N, const int32_t *__restrict__ seg, int S,
    const int32_t *__restrict__ chunks, int C, int reduce_max, float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, khalf = lane >> 5;
  for (int n0 = blockIdx.x * F_BN; n0 < N; n0 += gridDim.x * F_BN)
  for (int c = blockIdx.y; c < C; c += gridDim.y) {
    // chunk c = segments [s_lo, s_hi); its tokens run from the first segment's start to the last one's end
    int s_lo = c, s_hi = c + 1;
    if (chunks) {
      s_lo = min(max(chunks[2 * c], 0), S);
      s_hi = min(max(chunks[2 * c + 1], s_lo), S);
    }
    if (s_lo >= s_hi) continue;
    const int t_lo = seg_clamped(seg, s_lo, T).x, t_hi = max(seg_clamped(seg, s_hi - 1, T).y, t_lo);

    // per-column state of the epilogue (threads 0..127; the segment walk is the same for every column)
    const int col = threadIdx.x;
    const int n = n0 + col;
    const bool owner = col < F_BN && n < N;
    int s = s_lo;
    int2 cur = seg_clamped(seg, s, T);
    double sum = 0.0;
    float mx = 0.f;
    // closes segment s (writes its pooled value) and every empty segment behind it; leaves `cur` on the next non-empty one
    auto flush_empty = [&]() {
      while (s < s_hi && cur.x >= cur.y) {
        if (owner) out[(size_t)s * N + n] = 0.f;
        ++s;
        if (s < s_hi) cur = seg_clamped(seg, s, T);
      }
    };
    flush_empty();

    for (int m0 = t_lo; m0 < t_hi; m0 += F_BM) {
      f32x16 acc[2][2];
      f32_tile_mma<DT, VEC>(acc, x, W, b_dec, nullptr, t_hi, d, N, m0, n0, smem);
      // tile -> LDS, + b_enc and ReLU as pre_acts_f32_kernel's epilogue (the staging area is free: the k-loop ended on a barrier)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cc = wc * 64 + j * 32 + l31;
        const float be = (b_enc && n0 + cc < N) ? b_enc[n0 + cc] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int r = wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * khalf;
            float v = acc[i][j][e] + be;
            if (!(v > 0.f)) v = 0.f;
            smem[r * P_PITCH + cc] = v;
          }
      }
      __syncthreads();
      if (col < F_BN) {
        const int rows = min(F_BM, t_hi - m0);
        for (int r = 0; r < rows && s < s_hi; ++r) {
          const int t = m0 + r;
          if (t < cur.x) continue;                     // a gap between two segments of a chunk (not in a planned chunk)
          const float v = smem[r * P_PITCH + col];
          if (reduce_max) mx = fmaxf(mx, v);
          else sum += (double)v;
          if (t == cur.y - 1) {                        // segment end: write, reset, move on
            if (owner) out[(size_t)s * N + n] = reduce_max ? mx : (float)(sum / (double)(cur.y - cur.x));
            sum = 0.0;
            mx = 0.f;
            ++s;
            if (s < s_hi) cur = seg_clamped(seg, s, T);
            flush_empty();
          }
        }
      }
      __syncthreads();                                 // the next tile's staging rewrites the LDS
    }
  }
}

template <int DT>
int pooled_launch(const void *x, const float *W, const float *b_enc, const float *b_dec, int T, int d, int N,
                  const int32_t *seg, int S, const int32_t *chunks, int C, int reduce, float *out, hipStream_t s) {
  const size_t xb = (DT == MSAE_F32) ? 16 : 8;
  const bool vec = (d % 4 == 0) && msae_aligned(x, xb) && msae_aligned(W, 16) && (!b_dec || msae_aligned(b_dec, 16));
  const int strips = (N + F_BN - 1) / F_BN;
  dim3 grid(min(strips, 65535), min(C, 65535));
  const size_t smem = F_LDS_FLOATS * sizeof(float);
  auto kern = vec ? pooled_f32_kernel<DT, true> : pooled_f32_kernel<DT, false>;
  MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, x, W, b_enc, b_dec, T, d, N, seg, S, chunks, C, reduce, out);
  return msae_launch_status();
}

// ---- maps -----------------------------------------------------------------------------------------------------------
constexpr int M_THREADS = 256, M_WAVES = M_THREADS / 64;

// One wave per token, one lane per j: the chain walks k in 64-wide steps; the token's centred row arrives one element per
// lane and is broadcast with readlane (wave-uniform), the lane's 64 W_enc values of a step are loaded together (the chain
// itself stays one sequential ascending-k fmaf sequence per lane).
template <int DT, bool VEC>
__global__ __launch_bounds__(M_THREADS) void probe_maps_kernel(
    const void *__restrict__ x, const float *__restrict__ W, const float *__restrict__ b_enc,
    const float *__restrict__ b_dec, int T, int d, int N, const int32_t *__restrict__ seg, int S,
    const int32_t *__restrict__ idx, int k, float *__restrict__ maps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int2 sg = seg_clamped(seg, s, T);
    for (int t = sg.x + blockIdx.y * M_WAVES + wave; t < sg.y; t += gridDim.y * M_WAVES) {
      for (int j0 = 0; j0 < k; j0 += 64) {             // every lane runs every step (readlane needs the whole wave)
        const int j = j0 + lane;
        int f = j < k ? idx[(size_t)s * k + j] : -1;
        const bool live = f >= 0 && f < N;             // (top-k indices always are; a hostile idx gives 0, never a fault)
        f = live ? f : 0;
        const float *w = W + (size_t)f * d;
        float acc = 0.f;
        for (int k0 = 0; k0 < d; k0 += 64) {
          const int kk = k0 + lane;
          const float a_l = kk < d ? load_x1<DT>(x, (size_t)t * d + kk) - (b_dec ? b_dec[kk] : 0.f) : 0.f;
          const int a_bits = __float_as_int(a_l);
          if (k0 + 64 <= d) {
            float wv[64];
            if constexpr (VEC) {
#pragma unroll
              for (int q = 0; q < 16; ++q) {
                const f32x4 v4 = *reinterpret_cast<const f32x4 *>(w + k0 + 4 * q);
                wv[4 * q] = v4[0]; wv[4 * q + 1] = v4[1]; wv[4 * q + 2] = v4[2]; wv[4 * q + 3] = v4[3];
              }
            } else {
#pragma unroll
              for (int e = 0; e < 64; ++e) wv[e] = w[k0 + e];
            }
#pragma unroll
            for (int e = 0; e < 64; ++e)
              acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(a_bits, e)), wv[e], acc);
          } else {
            for (int e = 0; e < d - k0; ++e)
              acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(a_bits, e)), w[k0 + e], acc);
          }
        }
        float v = acc + (b_enc ? b_enc[f] : 0.f);
        if (!(v > 0.f) || !live) v = 0.f;
        if (j < k) maps[(size_t)t * k + j] = v;
      }
    }
  }
}

}  // namespace

extern "C" int msae_pooled_acts_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                    const float *b_dec, int T, int d, int N, const int32_t *seg, int S,
                                    const int32_t *chunks, int C, int reduce, float *out, void *stream) {
  if (T < 0 || d <= 0 || N <= 0 || S < 0 || (reduce != MSAE_REDUCE_MEAN && reduce != MSAE_REDUCE_MAX)) return MSAE_EINVAL;
  if (chunks ? C < 0 : false) return MSAE_EINVAL;
  if (!chunks) C = S;
  if (S == 0) return 0;
  if (!seg || !out || !x || !W_enc) return MSAE_EINVAL;
  if (T == 0) return (int)hipMemsetAsync(out, 0, (size_t)S * N * sizeof(float), (hipStream_t)stream);
  const hipStream_t s = (hipStream_t)stream;
  if (chunks) {   // segments no chunk names must still read 0: clear first (a planned chunk list names every segment)
    MSAE_HIP_TRY(hipMemsetAsync(out, 0, (size_t)S * N * sizeof(float), s));
    if (C == 0) return 0;
  }
  switch (x_dtype) {
    case MSAE_F32: return pooled_launch<MSAE_F32>(x, W_enc, b_enc, b_dec, T, d, N, seg, S, chunks, C, reduce, out, s);
    case MSAE_BF16: return pooled_launch<MSAE_BF16>(x, W_enc, b_enc, b_dec, T, d, N, seg, S, chunks, C, reduce, out, s);
    case MSAE_F16: return pooled_launch<MSAE_F16>(x, W_enc, b_enc, b_dec, T, d, N, seg, S, chunks, C, reduce, out, s);
    default: return MSAE_EINVAL;
  }
}

extern "C" int msae_probe_maps_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                   const float *b_dec, int T, int d, int N, const int32_t *seg, int S,
                                   const int32_t *idx, int k, float *maps, void *stream) {
  if (T < 0 || d <= 0 || N <= 0 || S < 0 || k <= 0 || k > MSAE_PROBE_MAX_K) return MSAE_EINVAL;
  if (T == 0) return 0;
  if (!maps || !x || !W_enc || (S > 0 && (!seg || !idx))) return MSAE_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  MSAE_HIP_TRY(hipMemsetAsync(maps, 0, (size_t)T * k * sizeof(float), s));
  if (S == 0) return 0;
  // blocks: segments x token groups; a block's four waves take every (4 * gridDim.y)-th token of its segment
  const long per_seg = ((long)T + S - 1) / S;
  const int gy = (int)std::min<long>(std::max<long>((per_seg + M_WAVES - 1) / M_WAVES, 1), 256);
  dim3 grid(std::min(S, 65535), gy);
  const bool vec = d % 4 == 0 && msae_aligned(W_enc, 16);
  switch (x_dtype) {
#define MAPS_CASE(DT) case DT: \
    if (vec) hipLaunchKernelGGL((probe_maps_kernel<DT, true>), grid, dim3(M_THREADS), 0, s, x, W_enc, b_enc, b_dec, T, d, N, seg, \
                                S, idx, k, maps); \
    else hipLaunchKernelGGL((probe_maps_kernel<DT, false>), grid, dim3(M_THREADS), 0, s, x, W_enc, b_enc, b_dec, T, d, N, seg, \
                            S, idx, k, maps); \
    break;
    MAPS_CASE(MSAE_F32) MAPS_CASE(MSAE_BF16) MAPS_CASE(MSAE_F16)
#undef MAPS_CASE
    default: return MSAE_EINVAL;
  }
  return msae_launch_status();
}
