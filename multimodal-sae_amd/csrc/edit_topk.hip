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

template <typename IDX>
__global__ __launch_bounds__(ET_MAX_THREADS) void edit_topk_kernel(
    const float *__restrict__ vals_in, const IDX *__restrict__ idx_in, int kk, const int32_t *__restrict__ edit_feat,
    const float *__restrict__ edit_val, const int32_t *__restrict__ edit_kind, int E, int k, int n_sort,
    float *__restrict__ vals, IDX *__restrict__ idx) {
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
      const int e = j - L;
      key = rank_key(edit_kind[e] == MSAE_EDIT_ZERO ? 0.f : edit_val[e], feat[e]);
    }
    keys[j] = key;
  }
  bitonic_sort_desc_u64<0>(keys, n_sort, threadIdx.x);              // run-time thread count (barriers before and after)
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const unsigned long long key = keys[j];
    vals[t * k + j] = rank_key_value(key);
    idx[t * k + j] = (IDX)rank_key_index(key);
  }
}

template <typename IDX>
int edit_topk_impl(const float *vals_in, const IDX *idx_in, int T, int kk, const int32_t *edit_feat, const float *edit_val,
                   const int32_t *edit_kind, int E, int N, int k, float *vals, IDX *idx, void *stream) {
  if (T < 0 || N <= 0 || k < 1 || E < 1) return MSAE_EINVAL;
  if ((long long)k + E > ET_MAX_SEL || (long long)k + E > N || kk < k + E) return MSAE_EINVAL;
  if (!vals_in || !idx_in || !edit_feat || !edit_val || !edit_kind || !vals || !idx) return MSAE_EINVAL;
  if (T == 0) return 0;
  const int n_sort = next_pow2(k + 2 * E);                          // <= 8192
  const int threads = std::min(ET_MAX_THREADS, std::max(MSAE_WAVE, n_sort / 2));
  const size_t smem = (size_t)n_sort * sizeof(unsigned long long) + (size_t)E * sizeof(int32_t);
  auto kern = edit_topk_kernel<IDX>;
  if (smem > 64 * 1024)
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL(kern, dim3(T), dim3(threads), smem, (hipStream_t)stream, vals_in, idx_in, kk, edit_feat, edit_val,
                     edit_kind, E, k, n_sort, vals, idx);
  return msae_launch_status();
}

}  // namespace

extern "C" int msae_edit_topk_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *edit_feat,
                                  const float *edit_val, const int32_t *edit_kind, int E, int N, int k, float *vals,
                                  int32_t *idx, void *stream) {
  return edit_topk_impl<int32_t>(vals_in, idx_in, T, kk, edit_feat, edit_val, edit_kind, E, N, k, vals, idx, stream);
}

extern "C" int msae_edit_topk_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk, const int32_t *edit_feat,
                                      const float *edit_val, const int32_t *edit_kind, int E, int N, int k, float *vals,
                                      int64_t *idx, void *stream) {
  return edit_topk_impl<int64_t>(vals_in, idx_in, T, kk, edit_feat, edit_val, edit_kind, E, N, k, vals, idx, stream);
}
