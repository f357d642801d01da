// edit_topk.hip -- set-valued hook edits on a per-token top-k LIST: the steering / attribution hooks'
// `latents[:, features] = values` and `latents[:, off_features] = 0` (reference features/steering.py:113-114,
// features/patching/utils.py:43-48 with a list or tensor of features) without the dense [T][N] latents and without a
// change to the fused encoder.  The caller runs the UNEDITED encode with kk >= k + E entries per token; this kernel turns
// each token's list into the canonical top-k of the edited latents.
//
// Why the list is enough: the canonical order (value descending, index ascending) is a total order on (value, index)
// pairs and the unedited list is its top-(k + E), zero fill by ascending index included.  At most E of the first k + E
// entries belong to edited features, so at least k unedited entries remain, and each of them precedes every unedited
// feature outside the list.  The top-k of the edited latents is therefore the top-k of
//     {list entries whose feature is not edited}  u  {(set value, f): SET edits}  u  {(+0, f): ZERO edits}.
// Only the first k + E entries of a row are read, so the result cannot depend on kk beyond kk >= k + E.
//
// edit_topk_kernel: ONE WORKGROUP PER TOKEN, min(1024, max(64, n_sort / 2)) threads -- a single wave up to 128 keys.
//   1. the edit table's features [E] go to LDS (they are the same for every token: L2 hits)
//   2. list entry j < k + E binary-searches them; a hit drops the entry (its feature's value is the edit's)
//   3. survivors and the E edit entries become 64-bit rank keys (common.h: msae_topk_f32's / msae_merge_topk's key)
//   4. the n_sort = next_pow2(k + 2 E) keys (padding: key 0, which no (value, index) pair produces) are sorted in LDS,
//      bitonic, descending (sortsel.h)
//   5. the first k are decoded: value from the order key (a value of -0 comes back as +0, as msae_merge_topk's does), index
// LDS per workgroup: 8 n_sort + 4 E bytes (2.2 KiB at k = 32, E = 50; 80 KiB at the envelope k + E = 4096, E = 4095).
// The kernel never indexes memory by a list entry's feature, so a hostile index cannot fault it.
//
// PER-TOKEN TABLES (msae_edit_topk_rows_f32): token t applies the slice
// [group_off[g], group_off[g + 1]) of the concatenated edit arrays, g = group_of[t]; a g outside [0, G) or an empty slice
// copies the first k entries.  The argument above is a statement about ONE token and its table, so it holds unchanged.  Both
// device arrays are clamped (slice into [0, E_total], length into [0, E_max]) before anything is indexed by them.
//   edit_topk_rows_wave_kernel<R>: next_pow2(k + 2 E_max) <= 64 R <= 256.  ONE WAVE PER TOKEN, ET_ROWS_WAVES waves per
//     workgroup, the 64 R keys in R registers per lane (sortsel.h wave_sort_desc_u64_regs), the slice read from global memory
//     (the same few lines for every token of a group: L2 hits; a linear scan up to ET_SCAN_MAX entries, else edit_find).
//     No LDS, no barriers; a wave whose token is unedited copies its row and leaves.
//   edit_topk_rows_wg_kernel: above 256 keys, edit_topk_kernel's layout with the token's slice in LDS and the token's own
//     n_sort = next_pow2(k + 2 E_g) <= the launch's; LDS 8 n_sort + 4 E_max bytes, 80 KiB at the envelope as above.
// `edited` (optional) marks the output slots whose feature is in the token's table: every surviving list entry's is not, so
// those are exactly the slots that came from an edit entry.
//
// VALUE-DEPENDENT EDITS (msae_edit_topk_valued_f32 / msae_edit_topk_rows_valued_f32): SCALE, ADD, FLOOR
// and CAP are functions of the feature's own latent c = L[t][f].  The list cannot supply c -- a feature outside the first
// k + E entries has an unknown value, and an increasing edit may lift it into the top-k -- so the caller passes the edited
// features' exact latents `cur` (msae_pre_acts_features_f32's columns).  With them the set above becomes
//     {list entries whose feature is not edited}  u  {(L'[t][f], f): every table entry},
// the same k + 2 E keys, and the argument stands word for word: it never used what an edit's value IS, only that every
// edited feature's value is known.  The three kernels are templated on VALUED; <false> is the code above, <true> reads
// `cur` at the entries whose kind depends on it and (optionally) writes each slot's gain dL'/dL * [c > 0], 1 for a slot that
// came from the list.
#include <algorithm>

#include "common.h"
#include "sortsel.h"

namespace {

constexpr int ET_MAX_SEL = 4096;            // k + E: msae_encode_topk's own limit on k
constexpr int ET_MAX_THREADS = 1024;

// position of f in the strictly ascending feat[0 .. E), or -1
__device__ __forceinline__ int edit_find(const int32_t *feat, int E, int f) {
  int lo = 0, hi = E;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (feat[mid] < f) lo = mid + 1; else hi = mid;
  }
  return (lo < E && feat[lo] == f) ? lo : -1;
}

// the valued forms' extra arguments; the <false> instantiations get an empty one and never look at it
struct EditCur {
  const float *cur = nullptr;          // [T][ld_cur] the edited features' exact latents
  int ld_cur = 0;
  const int32_t *col = nullptr;        // [E] / [E_total] the column of `cur` entry e reads; null: column e
  float *gain = nullptr;               // [T][k] or null
};

__device__ __forceinline__ bool edit_kind_valued(int kind) {
  return (unsigned)(kind - MSAE_EDIT_SCALE) <= (unsigned)(MSAE_EDIT_CAP - MSAE_EDIT_SCALE);
}

// c = L[t][feature of table entry e] for a kind that depends on it (the column clamped into [0, ld_cur)); other kinds
// read nothing
template <bool VALUED>
__device__ __forceinline__ float edit_current(const EditCur &a, size_t t, int e, int kind) {
  if (!VALUED || !edit_kind_valued(kind)) return 0.f;
  const int c = min(max(a.col ? a.col[e] : e, 0), a.ld_cur - 1);
  return a.cur[t * (size_t)a.ld_cur + c];
}

// L'[t][f] of a table entry: one f32 operation on c (include/msae.h); a kind outside the known ones reads as SET
template <bool VALUED>
__device__ __forceinline__ float edit_value(int kind, float v, float c) {
  if (kind == MSAE_EDIT_ZERO) return 0.f;
  if (VALUED) {
    if (kind == MSAE_EDIT_SCALE) return c * v;
    if (kind == MSAE_EDIT_ADD) return c + v;
    if (kind == MSAE_EDIT_FLOOR) return fmaxf(c, v);
    if (kind == MSAE_EDIT_CAP) return fminf(c, v);
  }
  return v;
}

// dL'/dL * [c > 0] of a table entry (torch.clamp's convention at the tie)
__device__ __forceinline__ float edit_gain(int kind, float v, float c) {
  const bool on = c > 0.f;
  if (kind == MSAE_EDIT_SCALE) return on ? v : 0.f;
  if (kind == MSAE_EDIT_ADD) return on ? 1.f : 0.f;
  if (kind == MSAE_EDIT_FLOOR) return (on && c >= v) ? 1.f : 0.f;
  if (kind == MSAE_EDIT_CAP) return (on && c <= v) ? 1.f : 0.f;
  return 0.f;
}

template <typename IDX, bool VALUED>
__global__ __launch_bounds__(ET_MAX_THREADS) void edit_topk_kernel(
    const float *__restrict__ vals_in, const IDX *__restrict__ idx_in, int kk, const int32_t *__restrict__ edit_feat,
    const float *__restrict__ edit_val, const int32_t *__restrict__ edit_kind, int E, int k, int n_sort,
    float *__restrict__ vals, IDX *__restrict__ idx, EditCur ec) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long et_smem[];
  unsigned long long *keys = et_smem;                               // [n_sort]
  int32_t *feat = reinterpret_cast<int32_t *>(keys + n_sort);       // [E]
  const size_t t = blockIdx.x;
  const int L = k + E;                                              // the entries of the row that matter

  for (int e = threadIdx.x; e < E; e += blockDim.x) feat[e] = edit_feat[e];
  __syncthreads();
  for (int j = threadIdx.x; j < n_sort; j += blockDim.x) {
    unsigned long long key = 0ull;
    if (j < L) {
      const int f = (int)idx_in[t * kk + j];
      if (edit_find(feat, E, f) < 0) key = rank_key(vals_in[t * kk + j], f);
    } else if (j < L + E) {
      const int e = j - L, kind = edit_kind[e];
      key = rank_key(edit_value<VALUED>(kind, edit_val[e], edit_current<VALUED>(ec, t, e, kind)), feat[e]);
    }
    keys[j] = key;
  }
  bitonic_sort_desc_u64<0>(keys, n_sort, threadIdx.x);              // run-time thread count (barriers before and after)
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const unsigned long long key = keys[j];
    const int f = rank_key_index(key);
    vals[t * k + j] = rank_key_value(key);
    idx[t * k + j] = (IDX)f;
    if (VALUED && ec.gain) {
      const int e = edit_find(feat, E, f);
      const int kind = e < 0 ? 0 : edit_kind[e];
      ec.gain[t * k + j] = e < 0 ? 1.f : edit_gain(kind, edit_val[e], edit_current<VALUED>(ec, t, e, kind));
    }
  }
}

template <typename IDX, bool VALUED>
int edit_topk_impl(const float *vals_in, const IDX *idx_in, int T, int kk, const int32_t *edit_feat, const float *edit_val,
                   const int32_t *edit_kind, int E, int N, int k, float *vals, IDX *idx, const EditCur &ec, void *stream) {
  if (T < 0 || N <= 0 || k < 1 || E < 1) return MSAE_EINVAL;
  if (VALUED && (!ec.cur || ec.ld_cur < 1)) return MSAE_EINVAL;
  if ((long long)k + E > ET_MAX_SEL || (long long)k + E > N || kk < k + E) return MSAE_EINVAL;
  if (!vals_in || !idx_in || !edit_feat || !edit_val || !edit_kind || !vals || !idx) return MSAE_EINVAL;
  if (T == 0) return 0;
  const int n_sort = next_pow2(k + 2 * E);                          // <= 8192
  const int threads = std::min(ET_MAX_THREADS, std::max(MSAE_WAVE, n_sort / 2));
  const size_t smem = (size_t)n_sort * sizeof(unsigned long long) + (size_t)E * sizeof(int32_t);
  auto kern = edit_topk_kernel<IDX, VALUED>;
  if (smem > 64 * 1024)
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(kern, dim3(T), dim3(threads), smem, (hipStream_t)stream, vals_in, idx_in, kk, edit_feat, edit_val,
                     edit_kind, E, k, n_sort, vals, idx, ec);
  return msae_launch_status();
}

// ---- per-token tables -----------------------------------------------------------------------------------------------------
constexpr int ET_ROWS_WAVES = 4;            // tokens per workgroup of the wave layout
constexpr int ET_SCAN_MAX = 8;              // slices up to this length are scanned, longer ones searched

// the token's slice of the edit arrays -> (first entry, length), both clamped: nothing read from the device is trusted
__device__ __forceinline__ int edit_slice(const int32_t *__restrict__ group_of, const int32_t *__restrict__ group_off, size_t t,
                                          int G, int E_total, int E_max, int &first) {
  const int g = group_of[t];
  first = 0;
  if (g < 0 || g >= G) return 0;
  const int a = min(max(group_off[g], 0), E_total), b = min(max(group_off[g + 1], 0), E_total);
  first = a;
  return min(max(b - a, 0), E_max);
}

// is f one of feat[0 .. E) (strictly ascending)?
__device__ __forceinline__ bool edit_has(const int32_t *feat, int E, int f) {
  if (E <= ET_SCAN_MAX) {
    bool hit = false;
    for (int e = 0; e < E; ++e) hit |= (feat[e] == f);
    return hit;
  }
  return edit_find(feat, E, f) >= 0;
}

// position of f in feat[0 .. E) (strictly ascending), or -1: edit_has's two routes
__device__ __forceinline__ int edit_pos(const int32_t *feat, int E, int f) {
  if (E <= ET_SCAN_MAX) {
    int pos = -1;
    for (int e = 0; e < E; ++e) pos = (feat[e] == f) ? e : pos;
    return pos;
  }
  return edit_find(feat, E, f);
}

template <typename IDX>
__device__ __forceinline__ void edit_copy_row(const float *__restrict__ vals_in, const IDX *__restrict__ idx_in, size_t t, int kk,
                                              int k, float *__restrict__ vals, IDX *__restrict__ idx,
                                              uint8_t *__restrict__ edited, float *__restrict__ gain, int tid, int nt) {
  for (int j = tid; j < k; j += nt) {
    vals[t * k + j] = vals_in[t * kk + j];
    idx[t * k + j] = idx_in[t * kk + j];
    if (edited) edited[t * k + j] = 0;
    if (gain) gain[t * k + j] = 1.f;
  }
}

template <typename IDX, int R, bool VALUED>
__global__ __launch_bounds__(ET_ROWS_WAVES * MSAE_WAVE) void edit_topk_rows_wave_kernel(
    const float *__restrict__ vals_in, const IDX *__restrict__ idx_in, int T, int kk, const int32_t *__restrict__ group_of,
    const int32_t *__restrict__ group_off, int G, const int32_t *__restrict__ edit_feat, const float *__restrict__ edit_val,
    const int32_t *__restrict__ edit_kind, int E_total, int E_max, int k, float *__restrict__ vals, IDX *__restrict__ idx,
    uint8_t *__restrict__ edited, EditCur ec) {
  const int lane = threadIdx.x & (MSAE_WAVE - 1);
  const size_t t = (size_t)blockIdx.x * ET_ROWS_WAVES + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / MSAE_WAVE));
  if (t >= (size_t)T) return;                                       // (no barrier anywhere in this kernel)
  int first;
  const int E = __builtin_amdgcn_readfirstlane(edit_slice(group_of, group_off, t, G, E_total, E_max, first));
  if (E == 0) {
    edit_copy_row(vals_in, idx_in, t, kk, k, vals, idx, edited, VALUED ? ec.gain : nullptr, lane, MSAE_WAVE);
    return;
  }
  first = __builtin_amdgcn_readfirstlane(first);
  const int32_t *feat = edit_feat + first;
  const int L = k + E;                                              // k + 2 E <= 64 R: the host chose R for E_max
  unsigned long long v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = r * MSAE_WAVE + lane;
    unsigned long long key = 0ull;
    if (j < L) {
      const int f = (int)idx_in[t * kk + j];
      if (!edit_has(feat, E, f)) key = rank_key(vals_in[t * kk + j], f);
    } else if (j < L + E) {
      const int e = first + (j - L), kind = edit_kind[e];
      key = rank_key(edit_value<VALUED>(kind, edit_val[e], edit_current<VALUED>(ec, t, e, kind)), edit_feat[e]);
    }
    v[r] = key;
  }
  wave_sort_desc_u64_regs<R>(v, lane);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = r * MSAE_WAVE + lane;
    if (j < k) {
      const int f = rank_key_index(v[r]);
      vals[t * k + j] = rank_key_value(v[r]);
      idx[t * k + j] = (IDX)f;
      if (edited) edited[t * k + j] = edit_has(feat, E, f) ? 1 : 0;
      if (VALUED && ec.gain) {
        const int p = edit_pos(feat, E, f), e = first + max(p, 0);
        const int kind = p < 0 ? 0 : edit_kind[e];
        ec.gain[t * k + j] = p < 0 ? 1.f : edit_gain(kind, edit_val[e], edit_current<VALUED>(ec, t, e, kind));
      }
    }
  }
}

template <typename IDX, bool VALUED>
__global__ __launch_bounds__(ET_MAX_THREADS) void edit_topk_rows_wg_kernel(
    const float *__restrict__ vals_in, const IDX *__restrict__ idx_in, int kk, const int32_t *__restrict__ group_of,
    const int32_t *__restrict__ group_off, int G, const int32_t *__restrict__ edit_feat, const float *__restrict__ edit_val,
    const int32_t *__restrict__ edit_kind, int E_total, int E_max, int k, int n_sort, float *__restrict__ vals,
    IDX *__restrict__ idx, uint8_t *__restrict__ edited, EditCur ec) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long et_smem[];
  unsigned long long *keys = et_smem;                               // [n_sort]
  int32_t *feat = reinterpret_cast<int32_t *>(keys + n_sort);       // [E_max]
  const size_t t = blockIdx.x;
  int first;
  const int E = edit_slice(group_of, group_off, t, G, E_total, E_max, first);   // uniform over the workgroup
  if (E == 0) {
    edit_copy_row(vals_in, idx_in, t, kk, k, vals, idx, edited, VALUED ? ec.gain : nullptr, threadIdx.x, blockDim.x);
    return;
  }
  const int L = k + E;
  const int n = min(next_pow2(k + 2 * E), n_sort);                  // the token's own key count (E <= E_max: n <= n_sort)
  for (int e = threadIdx.x; e < E; e += blockDim.x) feat[e] = edit_feat[first + e];
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    unsigned long long key = 0ull;
    if (j < L) {
      const int f = (int)idx_in[t * kk + j];
      if (edit_find(feat, E, f) < 0) key = rank_key(vals_in[t * kk + j], f);
    } else if (j < L + E) {
      const int e = j - L, kind = edit_kind[first + e];
      key = rank_key(edit_value<VALUED>(kind, edit_val[first + e], edit_current<VALUED>(ec, t, first + e, kind)), feat[e]);
    }
    keys[j] = key;
  }
  bitonic_sort_desc_u64<0>(keys, n, threadIdx.x);
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const unsigned long long key = keys[j];
    const int f = rank_key_index(key);
    vals[t * k + j] = rank_key_value(key);
    idx[t * k + j] = (IDX)f;
    const int p = edit_find(feat, E, f);
    if (edited) edited[t * k + j] = p >= 0 ? 1 : 0;
    if (VALUED && ec.gain) {
      const int e = first + max(p, 0);
      const int kind = p < 0 ? 0 : edit_kind[e];
      ec.gain[t * k + j] = p < 0 ? 1.f : edit_gain(kind, edit_val[e], edit_current<VALUED>(ec, t, e, kind));
    }
  }
}

template <typename IDX, bool VALUED>
int edit_topk_rows_impl(const float *vals_in, const IDX *idx_in, int T, int kk, const int32_t *group_of,
                        const int32_t *group_off, int G, const int32_t *edit_feat, const float *edit_val,
                        const int32_t *edit_kind, int E_total, int E_max, int N, int k, float *vals, IDX *idx, uint8_t *edited,
                        const EditCur &ec, void *stream) {
  if (T < 0 || G < 1 || k < 1 || E_max < 1 || E_total < 0) return MSAE_EINVAL;
  if (VALUED && (!ec.cur || ec.ld_cur < 1)) return MSAE_EINVAL;
  if ((long long)k + E_max > ET_MAX_SEL || (long long)k + E_max > N || kk < k + E_max) return MSAE_EINVAL;
  if (!vals_in || !idx_in || !group_of || !group_off || !edit_feat || !edit_val || !edit_kind || !vals || !idx)
    return MSAE_EINVAL;
  if (T == 0) return 0;
  const int n_sort = next_pow2(k + 2 * E_max);                      // <= 8192
  hipStream_t st = (hipStream_t)stream;
  if (n_sort <= 256) {
    const dim3 grid((unsigned)(((long long)T + ET_ROWS_WAVES - 1) / ET_ROWS_WAVES)), block(ET_ROWS_WAVES * MSAE_WAVE);
#define ET_ROWS_LAUNCH(R)                                                                                                 \
  hipLaunchKernelGGL((edit_topk_rows_wave_kernel<IDX, R, VALUED>), grid, block, 0, st, vals_in, idx_in, T, kk, group_of,   \
                     group_off, G, edit_feat, edit_val, edit_kind, E_total, E_max, k, vals, idx, edited, ec)
    if (n_sort <= 64) ET_ROWS_LAUNCH(1);
    else if (n_sort <= 128) ET_ROWS_LAUNCH(2);
    else ET_ROWS_LAUNCH(4);
#undef ET_ROWS_LAUNCH
    return msae_launch_status();
  }
  const int threads = std::min(ET_MAX_THREADS, std::max(MSAE_WAVE, n_sort / 2));
  const size_t smem = (size_t)n_sort * sizeof(unsigned long long) + (size_t)E_max * sizeof(int32_t);
  auto kern = edit_topk_rows_wg_kernel<IDX, VALUED>;
  if (smem > 64 * 1024)
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(kern, dim3(T), dim3(threads), smem, st, vals_in, idx_in, kk, group_of, group_off, G, edit_feat, edit_val,
                     edit_kind, E_total, E_max, k, n_sort, vals, idx, edited, ec);
  return msae_launch_status();
}

}  // namespace

extern "C" int msae_edit_topk_rows_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *group_of,
                                       const int32_t *group_off, int G, const int32_t *edit_feat, const float *edit_val,
                                       const int32_t *edit_kind, int E_total, int E_max, int N, int k, float *vals,
                                       int32_t *idx, uint8_t *edited, void *stream) {
  return edit_topk_rows_impl<int32_t, false>(vals_in, idx_in, T, kk, group_of, group_off, G, edit_feat, edit_val, edit_kind,
                                             E_total, E_max, N, k, vals, idx, edited, EditCur{}, stream);
}

extern "C" int msae_edit_topk_rows_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk, const int32_t *group_of,
                                           const int32_t *group_off, int G, const int32_t *edit_feat, const float *edit_val,
                                           const int32_t *edit_kind, int E_total, int E_max, int N, int k, float *vals,
                                           int64_t *idx, uint8_t *edited, void *stream) {
  return edit_topk_rows_impl<int64_t, false>(vals_in, idx_in, T, kk, group_of, group_off, G, edit_feat, edit_val, edit_kind,
                                             E_total, E_max, N, k, vals, idx, edited, EditCur{}, stream);
}

extern "C" int msae_edit_topk_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *edit_feat,
                                  const float *edit_val, const int32_t *edit_kind, int E, int N, int k, float *vals,
                                  int32_t *idx, void *stream) {
  return edit_topk_impl<int32_t, false>(vals_in, idx_in, T, kk, edit_feat, edit_val, edit_kind, E, N, k, vals, idx, EditCur{},
                                        stream);
}

extern "C" int msae_edit_topk_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk, const int32_t *edit_feat,
                                      const float *edit_val, const int32_t *edit_kind, int E, int N, int k, float *vals,
                                      int64_t *idx, void *stream) {
  return edit_topk_impl<int64_t, false>(vals_in, idx_in, T, kk, edit_feat, edit_val, edit_kind, E, N, k, vals, idx, EditCur{},
                                        stream);
}

// ---- value-dependent edits: the same kernels with the edited features' exact latents ---------------------------------------
extern "C" int msae_edit_topk_valued_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *edit_feat,
                                         const float *edit_val, const int32_t *edit_kind, int E, int N, int k,
                                         const float *cur, int ld_cur, const int32_t *edit_col, float *vals, int32_t *idx,
                                         float *gain, void *stream) {
  return edit_topk_impl<int32_t, true>(vals_in, idx_in, T, kk, edit_feat, edit_val, edit_kind, E, N, k, vals, idx,
                                       EditCur{cur, ld_cur, edit_col, gain}, stream);
}

extern "C" int msae_edit_topk_valued_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk,
                                             const int32_t *edit_feat, const float *edit_val, const int32_t *edit_kind, int E,
                                             int N, int k, const float *cur, int ld_cur, const int32_t *edit_col, float *vals,
                                             int64_t *idx, float *gain, void *stream) {
  return edit_topk_impl<int64_t, true>(vals_in, idx_in, T, kk, edit_feat, edit_val, edit_kind, E, N, k, vals, idx,
                                       EditCur{cur, ld_cur, edit_col, gain}, stream);
}

extern "C" int msae_edit_topk_rows_valued_f32(const float *vals_in, const int32_t *idx_in, int T, int kk,
                                              const int32_t *group_of, const int32_t *group_off, int G,
                                              const int32_t *edit_feat, const float *edit_val, const int32_t *edit_kind,
                                              int E_total, int E_max, int N, int k, const float *cur, int ld_cur,
                                              const int32_t *edit_col, float *vals, int32_t *idx, uint8_t *edited, float *gain,
                                              void *stream) {
  return edit_topk_rows_impl<int32_t, true>(vals_in, idx_in, T, kk, group_of, group_off, G, edit_feat, edit_val, edit_kind,
                                            E_total, E_max, N, k, vals, idx, edited, EditCur{cur, ld_cur, edit_col, gain},
                                            stream);
}

extern "C" int msae_edit_topk_rows_valued_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk,
                                                  const int32_t *group_of, const int32_t *group_off, int G,
                                                  const int32_t *edit_feat, const float *edit_val, const int32_t *edit_kind,
                                                  int E_total, int E_max, int N, int k, const float *cur, int ld_cur,
                                                  const int32_t *edit_col, float *vals, int64_t *idx, uint8_t *edited,
                                                  float *gain, void *stream) {
  return edit_topk_rows_impl<int64_t, true>(vals_in, idx_in, T, kk, group_of, group_off, G, edit_feat, edit_val, edit_kind,
                                            E_total, E_max, N, k, vals, idx, edited, EditCur{cur, ld_cur, edit_col, gain},
                                            stream);
}
