// neighbors.hip -- fused f32 GEMM + per-row top-k: the k nearest features of a feature by decoder cosine similarity
// (reference sae_auto_interp/features/stats.py:76-120, cos + get_neighbors) and the top logits of a feature by direct logit
// attribution (stats.py:12-47, logits).  Both are "Q K^T, then the top-k of every row"; the [M][N] product never reaches HBM.
//
// rows_topk_kernel: the tile is pre_acts_f32_kernel's (f32_tile.h with b_dec = NULL and the query rows as the gather list:
// the same staging, the same ascending-k v_mfma_f32_32x32x2_f32 chain), so every dot is bit-identical to msae_pre_acts_f32's
// value without bias and ReLU; only the epilogue differs.  The 128 x 128 tile goes into the (then free) staging LDS at pitch
// 129 and TWO threads per query row walk it, 64 columns each: the value is scaled (two separate f32 multiplies), turned into
// the project's 64-bit rank key (common.h: value descending, index ascending) and compared with the k-th key of the thread's
// running list.  The list -- the KMAX best keys of the thread's columns so far, sorted -- lives in REGISTERS across the
// strips of the workgroup's chunk: it costs no LDS, so the k <= 16 variant keeps pre_acts_f32_kernel's two workgroups per CU
// (a 128 x k x 8 B list in LDS beside the 73.7 KB staging area would not).  Rank keys are distinct (they carry the index), so
// the result is a pure function of the SET of (value, index) pairs: it cannot depend on the walk order, the split of a row
// between two threads, the chunking or the grid.  After the first strips a hit is rare (about k / keys seen per column); the
// insert is a KMAX-step compare-exchange chain.
//
// Work split: one workgroup per (128-query tile, chunk); a chunk is a contiguous run of 128-key strips.  At the end of the
// chunk the row's two half lists are merged through LDS and written as plane 0 = value bits, plane 1 = key index into
// ws[chunks][2][M][k] -- msae_merge_topk's `gathered` layout, so ONE merge call with G = chunks, kl = k finishes; with one
// chunk the list goes straight to vals / idx.  A list shorter than k (few keys, the exclusion) is padded with the key that
// ranks last (rank key 0: value bits 0xFFFFFFFF, index 0x7FFFFFFF), which no real (value, index) pair can produce.
//
// row_inv_norms_kernel: one wave per row; lane l adds the f64 squares of elements l, l + 64, ... in ascending order, the 64
// partial sums are added in a fixed xor tree; no atomics -> bit-reproducible.
#include <algorithm>

#include "f32_tile.h"
#include "wave_ops.h"

namespace {

constexpr int NB_PITCH = F_BN + 1;             // the tile in LDS: [128 queries][129 floats]
constexpr int NB_KS_OFF = F_BM * NB_PITCH;     // the strip's 128 key scales behind it
static_assert(NB_KS_OFF + F_BN <= F_LDS_FLOATS, "tile + key scales must fit the staging LDS");
constexpr int NB_K_SMALL = 16, NB_K_MAX = 64;
static_assert((size_t)F_BM * NB_K_MAX * sizeof(unsigned long long) <= F_LDS_FLOATS * sizeof(float),
              "the half lists must fit the staging LDS at the end of a chunk");

// q_rows -> ws: entries clamped to [0, Qn) (a hostile index reads a valid row, never faults); ones[m] = 1 (the mask of the
// 64-bit-index merge)
__global__ __launch_bounds__(256) void clamp_rows_kernel(const int32_t *__restrict__ q_rows, int M, int Qn,
                                                         int32_t *__restrict__ out, int32_t *__restrict__ ones) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  if (q_rows) out[m] = min(max(q_rows[m], 0), Qn - 1);
  if (ones) ones[m] = 1;
}

// sorted (descending) insert of `key` into list[0 .. KMAX): the smallest entry falls out
template <int KMAX>
__device__ __forceinline__ void list_insert(unsigned long long (&list)[KMAX], unsigned long long key) {
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    const unsigned long long cur = list[j];
    const bool up = key > cur;
    list[j] = up ? key : cur;
    key = up ? cur : key;
  }
}
template <int KMAX>
__device__ __forceinline__ unsigned long long list_at(const unsigned long long (&list)[KMAX], int i) {
  unsigned long long v = 0ull;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) v = (j == i) ? list[j] : v;
  return v;
}

template <bool VEC, int KMAX>
__global__ __launch_bounds__(F_THREADS, KMAX <= NB_K_SMALL ? 2 : 1) void rows_topk_kernel(
    const float *__restrict__ Q, const int32_t *__restrict__ rows, int M, const float *__restrict__ K, int N, int d,
    const float *__restrict__ q_scale, const float *__restrict__ k_scale, const int32_t *__restrict__ exclude, int k,
    int chunks, int32_t *__restrict__ plane0, int32_t *__restrict__ plane1, int wide) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, khalf = lane >> 5;
  const int m0 = blockIdx.x * F_BM, c = blockIdx.y;
  const int strips = (N + F_BN - 1) / F_BN;
  const int s_lo = (int)((long long)c * strips / chunks), s_hi = (int)((long long)(c + 1) * strips / chunks);

  // epilogue state: thread (row, half) owns columns [64 half, 64 half + 64) of query row m0 + row in every strip
  const int row = threadIdx.x & (F_BM - 1), half = threadIdx.x >> 7;
  const int m = m0 + row;
  const bool live = m < M;
  const float qs = (live && q_scale) ? q_scale[m] : 1.f;
  const int ex = (live && exclude) ? exclude[m] : -1;
  unsigned long long list[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) list[j] = 0ull;
  unsigned long long thr = 0ull;                       // list[k - 1]: a key must beat it to enter

  for (int s = s_lo; s < s_hi; ++s) {
    const int n0 = s * F_BN;
    f32x16 acc[2][2];
    f32_tile_mma<MSAE_F32, VEC>(acc, Q, K, nullptr, rows, M, d, N, m0, n0, smem);
    // tile -> LDS (the staging area is free: the k-loop ended on a barrier)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cc = wc * 64 + j * 32 + l31;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * khalf;
          smem[r * NB_PITCH + cc] = acc[i][j][e];
        }
    }
    if (k_scale && threadIdx.x < F_BN) smem[NB_KS_OFF + threadIdx.x] = (n0 + (int)threadIdx.x < N) ? k_scale[n0 + threadIdx.x] : 0.f;
    __syncthreads();
    if (live) {
      const float *trow = smem + row * NB_PITCH + half * 64;   // bank (row + column) % 64: a wave's 64 rows never collide
      const float *ks = smem + NB_KS_OFF + half * 64;          // one address per wave: broadcast
      const int nb = n0 + half * 64;
#pragma unroll 8
      for (int col = 0; col < 64; ++col) {
        float v = trow[col];
        if (q_scale) v = v * qs;                               // two separately rounded multiplies (-ffp-contract=off)
        if (k_scale) v = v * ks[col];
        const int n = nb + col;
        const unsigned long long key = rank_key(v, n);
        if (n < N && n != ex && key > thr) {
          list_insert<KMAX>(list, key);
          thr = list_at<KMAX>(list, k - 1);
        }
      }
    }
    __syncthreads();                                           // the next strip's staging rewrites the LDS
  }

  // the row's two half lists -> one: half 1 hands its (sorted) list over through LDS, half 0 inserts what beats its own
  unsigned long long *hand = reinterpret_cast<unsigned long long *>(smem);   // [KMAX][128]: consecutive rows, no conflicts
  if (half == 1) {
#pragma unroll
    for (int j = 0; j < KMAX; ++j) hand[j * F_BM + row] = list[j];
  }
  __syncthreads();
  if (half == 0 && live) {
#pragma unroll 1
    for (int j = 0; j < k; ++j) {
      const unsigned long long key = hand[j * F_BM + row];
      if (!(key > thr)) break;                                 // sorted: nothing further down beats the list either
      list_insert<KMAX>(list, key);
      thr = list_at<KMAX>(list, k - 1);
    }
    const size_t base0 = (((size_t)c * 2 + 0) * M + m) * k, base1 = (((size_t)c * 2 + 1) * M + m) * k;
    const size_t off0 = chunks > 1 ? base0 : (size_t)m * k, off1 = chunks > 1 ? base1 : (size_t)m * k;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < k) {
        plane0[off0 + j] = (int32_t)__float_as_uint(rank_key_value(list[j]));
        if (wide) reinterpret_cast<int64_t *>(plane1)[off1 + j] = rank_key_index(list[j]);   // (one chunk, int64 output)
        else plane1[off1 + j] = rank_key_index(list[j]);
      }
  }
}

constexpr int IN_THREADS = 256, IN_WAVES = IN_THREADS / 64;
__global__ __launch_bounds__(IN_THREADS) void row_inv_norms_kernel(const float *__restrict__ W, int N, int d,
                                                                   float *__restrict__ inv) {
  const int lane = threadIdx.x & 63;
  for (long long n = (long long)blockIdx.x * IN_WAVES + (threadIdx.x >> 6); n < N; n += (long long)gridDim.x * IN_WAVES) {
    const float *w = W + (size_t)n * d;
    double s = 0.0;
    for (int i = lane; i < d; i += 64) {
      const double v = (double)w[i];
      s = __builtin_fma(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) {
      const double nrm = __builtin_sqrt(s);
      inv[n] = (float)(1.0 / (nrm > 1e-12 ? nrm : 1e-12));    // F.normalize's clamp (stats.py:80-81)
    }
  }
}

int cu_count() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus > 0 ? cus : 256;
}

// chunks of a call: forced (> 0) or the smallest count that gives >= 2 workgroups per CU over the query tiles; never more
// than the strips, never more than msae_merge_topk takes (G * kl <= 8192).  0: the forced count is out of range.
int plan_chunks(int M, int N, int k, int chunks) {
  const int strips = (N + F_BN - 1) / F_BN, cap = std::max(1, std::min(strips, 8192 / k));
  if (chunks > 0) return (long long)std::min(chunks, strips) * k > 8192 ? 0 : std::min(chunks, strips);
  const long long tiles = std::max(1LL, ((long long)M + F_BM - 1) / F_BM), want = 2LL * cu_count();
  return (int)std::min<long long>(cap, std::max(1LL, (want + tiles - 1) / tiles));
}

bool shape_ok(int M, int N, int k, int chunks) { return M >= 0 && N > 0 && k >= 1 && k <= NB_K_MAX && chunks >= 0; }

// workspace: the clamped row list [M], the all-ones mask [M], then the chunks' lists
size_t rows_bytes(int M) { return msae_align_up((size_t)std::max(M, 1) * sizeof(int32_t), 256); }
size_t head_bytes(int M) { return 2 * rows_bytes(M); }

}  // namespace

extern "C" int msae_row_inv_norms_f32(const float *W, int N, int d, float *inv, void *stream) {
  if (N < 0 || d <= 0) return MSAE_EINVAL;
  if (N == 0) return 0;
  if (!W || !inv) return MSAE_EINVAL;
  const int grid = (int)std::min<long long>(((long long)N + IN_WAVES - 1) / IN_WAVES, 1 << 20);
  hipLaunchKernelGGL(row_inv_norms_kernel, dim3(grid), dim3(IN_THREADS), 0, (hipStream_t)stream, W, N, d, inv);
  return msae_launch_status();
}

extern "C" size_t msae_rows_topk_ws_bytes(int M, int N, int k, int chunks) {
  if (!shape_ok(M, N, k, chunks) || k > N) return 0;
  const int C = plan_chunks(M, N, k, chunks);
  if (C == 0) return 0;
  return head_bytes(M) + (C > 1 ? (size_t)C * 2 * M * k * sizeof(int32_t) : 0);
}

static int rows_topk_impl(const float *Q, int Qn, const int32_t *q_rows, int M, const float *K, int N, int d,
                          const float *q_scale, const float *k_scale, const int32_t *exclude, int k, int chunks,
                          float *vals, int32_t *idx, int64_t *idx64, void *ws, size_t ws_bytes, void *stream) {
  if (!shape_ok(M, N, k, chunks) || d <= 0 || Qn <= 0 || k > N - (exclude ? 1 : 0)) return MSAE_EINVAL;
  if (!q_rows && M > Qn) return MSAE_EINVAL;
  if (M == 0) return 0;
  if (!Q || !K || !vals || (!idx && !idx64)) return MSAE_EINVAL;
  const int C = plan_chunks(M, N, k, chunks);
  if (C == 0) return MSAE_EINVAL;
  const size_t need = head_bytes(M) + (C > 1 ? (size_t)C * 2 * M * k * sizeof(int32_t) : 0);
  if ((q_rows || C > 1) && (!ws || ws_bytes < need)) return MSAE_EWS;
  if (C > 65535) return MSAE_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  int32_t *rows = q_rows ? static_cast<int32_t *>(ws) : nullptr;
  int32_t *ones = (C > 1 && idx64) ? reinterpret_cast<int32_t *>(static_cast<char *>(ws) + rows_bytes(M)) : nullptr;
  if (rows || ones) hipLaunchKernelGGL(clamp_rows_kernel, dim3((M + 255) / 256), dim3(256), 0, s, q_rows, M, Qn, rows, ones);
  int32_t *lists = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + head_bytes(M));
  const int wide = (C == 1 && idx64) ? 1 : 0;
  int32_t *plane0 = C > 1 ? lists : reinterpret_cast<int32_t *>(vals);
  int32_t *plane1 = C > 1 ? lists : (idx64 ? reinterpret_cast<int32_t *>(idx64) : idx);
  const bool vec = (d % 4 == 0) && msae_aligned(Q, 16) && msae_aligned(K, 16);
  const size_t smem = F_LDS_FLOATS * sizeof(float);
  const dim3 grid((M + F_BM - 1) / F_BM, C);
#define NB_LAUNCH(VEC, KM)                                                                                              \
  do {                                                                                                                  \
    auto kern = rows_topk_kernel<VEC, KM>;                                                                              \
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));       \
    hipLaunchKernelGGL(kern, grid, dim3(F_THREADS), smem, s, Q, rows, M, K, N, d, q_scale, k_scale, exclude, k, C,      \
                       plane0, plane1, wide);                                                                              \
  } while (0)
  if (k <= NB_K_SMALL) {
    if (vec) NB_LAUNCH(true, NB_K_SMALL); else NB_LAUNCH(false, NB_K_SMALL);
  } else {
    if (vec) NB_LAUNCH(true, NB_K_MAX); else NB_LAUNCH(false, NB_K_MAX);
  }
#undef NB_LAUNCH
  int st = msae_launch_status();
  if (st != 0 || C == 1) return st;
  if (idx64) return msae_merge_topk_masked(lists, M, C, k, k, ones, vals, nullptr, idx64, stream);
  return msae_merge_topk(lists, M, C, k, k, vals, idx, nullptr, stream);
}

extern "C" int msae_rows_topk_f32(const float *Q, int Qn, const int32_t *q_rows, int M, const float *K, int N, int d,
                                  const float *q_scale, const float *k_scale, const int32_t *exclude, int k, int chunks,
                                  float *vals, int32_t *idx, void *ws, size_t ws_bytes, void *stream) {
  return rows_topk_impl(Q, Qn, q_rows, M, K, N, d, q_scale, k_scale, exclude, k, chunks, vals, idx, nullptr, ws, ws_bytes,
                        stream);
}

extern "C" int msae_rows_topk_i64_f32(const float *Q, int Qn, const int32_t *q_rows, int M, const float *K, int N, int d,
                                      const float *q_scale, const float *k_scale, const int32_t *exclude, int k,
                                      int chunks, float *vals, int64_t *idx, void *ws, size_t ws_bytes, void *stream) {
  return rows_topk_impl(Q, Qn, q_rows, M, K, N, d, q_scale, k_scale, exclude, k, chunks, vals, nullptr, idx, ws, ws_bytes,
                        stream);
}
