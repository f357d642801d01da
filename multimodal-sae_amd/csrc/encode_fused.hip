// encode_fused.hip -- fused Sae.encode: MFMA candidate pass (int8 or bf16) + exact f32 re-score + TopK.  This file is the HOST
// side.  Kernels: encode_prep.h (operand preparation), gemm_mfma.h / gemm_skinny.h (candidate passes), encode_rescore.h (select +
// exact re-score, shard records), encode_small.h (T <= 16), encode_cert.h (certified pass), topk.hip / encode_f32.hip (exact path);
// shared layout / options: encode_defs.h; build-time knobs and probes: tuning.h.
//
// Structure.  An entry point validates, fills ONE EncodeCall (the arguments nothing below it changes), builds its plan and
// dispatches once on x_dtype (with_x_dtype).  Plans: FusedPlan (make_plan), ExtPlan, RowsPlan -- byte offsets read through at<T>();
// all three embed one FallbackPlan, the exact fallback's flag list + dense scratch.  Launch sequences: run_small (T <= 16);
// run_candidate_pipeline, stages 2 to 6 below, driven by a CandidatePass that run_fast's operand preparations (prep_i8, prep_f8,
// prep_bf16) or run_cert fill in; run_rescore_ext (owner side of a feature-sharded group); run_exact_fallback / run_exact_rows.
// prepare_impl rebuilds the operand groups a REQ_* request names (prepare_request).
//
// Replaces Sae.encode = select_topk(pre_acts(x)) (reference sae/sae.py:172-185) without ever
// writing the dense [T][N] latents (512 KiB/token at N = 131072) to HBM.
//
// Pipeline per call (all on one stream, no host synchronisation):
//   1. prep_x        a32[T][d] = f32(x) - b_dec  (the exact SAE input)
//      int8 pass:    column max over the batch -> outlier dims -> per-token scale sx[t], int8 rows xq,
//                    outlier dims in their own 128-wide k-tile at scale m[t]*sx[t]; the matching
//                    columns of Wq are gathered into an outlier tile.  (bf16 pass: xb = bf16(a32).)
//   2. gemm<DENSE>   coarse pre-acts of a 1/32 strided SAMPLE of the features -> [T][S] f32
//   3. kth value     tau[t] = r-th largest sample value: ~32*r features of the full width exceed it; the sample
//                    features above tau start the token's candidate list (KthPush / sample_push_kernel)
//   4. gemm<THRESH>  THE DOMINANT KERNEL (gemm_mfma.h): [T][d] x [d][N] on the matrix cores -- for batches of more
//                    than 256 tokens over the 31/32 of the features the sample pass has not scored (main_row);
//                    epilogue: scales, +b_enc, compare with tau[t], append (feature, coarse) of the
//                    rare survivors to a per-token candidate list.  Roofline: MFMA, 2*d*N op/token (in practice the
//                    package power limit: DESIGN.md section 5).
//   5. select_rescore per token: order candidates by their UPPER value u, re-score the best ones
//                    with the exact ascending-k f32 fma chain over the f32 W_enc rows, take the
//                    canonical top-k, and verify that EVERY feature whose u reaches the exact
//                    k-th value v_k has been re-scored (at most one extension round).  Tokens
//                    that fail (list overflow, tau <= 0, model violation ...) are flagged.
//   6. exact path    flagged tokens (normally none) are recomputed by encode_f32 + topk through a
//                    device-side row list; their results overwrite step 5's.
//
// Verification model.  The coarse value c(t,n) of the candidate pass differs from the exact
// pre-activation p(t,n) by rounding noise whose variance is known per (token, feature) PAIR:
//   int8:  p - c = sum_c [ a_c sw_n eps_c + sx_t delta_c w_c ],  eps, delta = rounding residuals in
//          (-1/2, 1/2] steps (delta in m_t steps on the outlier dims), so
//          sigma^2(t,n) = sw_n^2 |a_t|^2 / 12 + sx_t^2 (|W_n[in]|^2 + m_t^2 |W_n[out]|^2) / 12
//   bf16:  p - c = -sum_c a_c w_c (da_c + dw_c), relative roundings of variance 2.75e-6 each, so
//          sigma^2(t,n) <= 5.5e-6 |a_t|_4^2 |W_n|_4^2   (Cauchy-Schwarz on sum a_c^2 w_c^2)
// both of the separable form  z^2 sigma^2 = P_t Q_n + R_t (Si_n + M_t So_n).  Every stage works on
// u = c + z sigma (z = 7 by default): the sample threshold tau is a rank statistic of u, the GEMM
// emits u > tau, and a token is verified when all features with u >= v_k were re-scored exactly --
// a feature is then missed only if its own error exceeds z of ITS sigma (heterogeneous rows: spiky,
// large-norm or near-dead encoder rows carry their own band).  Rows whose bulk lies below one int8
// step (max > 127 rms) are rounded stochastically (hash dither), which keeps the residual unbiased
// whatever direction the activations have, at variance sw^2/4.  The model is CHECKED on every
// re-scored pair: |p - c| > 6 sigma flags the token (reason 64) and it goes to the exact path.
// DESIGN.md section 4 gives the failure-probability arithmetic.
//
// Outputs are therefore bit-identical to msae_pre_acts_f32 + msae_topk_f32 whenever the token
// verifies, and ARE that path's outputs when it does not -- whichever operand type ran step 4.
#include <new>
#include <cstddef>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "gemm_mfma.h"
#include "gemm_skinny.h"
#include "encode_defs.h"
#include "encode_prep.h"
#include "encode_rescore.h"
#include "encode_small.h"
#include "encode_cert.h"

int msae_pre_acts_launch(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                         const float *b_dec, const int *rows, const int *n_rows, int T, int d, int N,
                         int relu, float *out, int ld_out, hipStream_t s);
int msae_topk_launch(const float *latents, int T, int N, int k, int ld, const int *n_rows,
                     float *vals, int32_t *idx, hipStream_t s, const TopkExtra &ex = TopkExtra());
bool msae_kth_value_launch(const float *rows, int T, int S, int ld, int r, float *out, int out_ld,
                           int out_col, hipStream_t s, const KthPush &push = KthPush());

namespace {

// ---- MFMA GEMM: gemm_mfma.h.  Tile choice from tools/gemm_sweep on MI355X (T=8192, d=4096,
// N=131072): 256x256 tiles of 128-B k-rows, 2-slot ring, 8 waves as 2x4.
using GemmBf16 = GemmCfg<256, 256, 2, 2, 4, false>;
constexpr int kGemmI8Shape = MSAE_GEMM_MF == 16 ? 128 : 0;  // GemmCfg bit 7: 16x16x64 int8 MFMAs (tuning.h)
using GemmI8 = GemmCfg<256, 256, 2, 2, 4, true, kGemmI8Shape>;
using GemmI8Cert = GemmCfg<256, 256, 2, 2, 4, true, 32 | kGemmI8Shape>;   // msae_options::certified (encode_cert.h)
using GemmF8 = GemmCfg<256, 256, 2, 2, 4, false, 64>;      // MSAE_COARSE_FP8: e4m3 operands (BASELINE configs[4])
constexpr int G_BM = GemmBf16::BM;

// the scratch ranges of a call in one launch (candidate counters, flag list, column maxima; with the feature-major re-score its
// pair counters and defer flags): (pointer, count) pairs by value, unused ones empty
constexpr int ZERO_RANGES = 5;
struct ZeroRanges { int *p[ZERO_RANGES]; size_t n[ZERO_RANGES]; };
__global__ void zero_ranges_i32_kernel(ZeroRanges z) {
#pragma unroll
  for (int r = 0; r < ZERO_RANGES; ++r)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < z.n[r]; i += (size_t)gridDim.x * 256) z.p[r][i] = 0;
}

__global__ void zero_i32_kernel(int *p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0;
}

// hook edits on dense rows (exact path): latents[:, set_feature] = set_value; [:, zero_feature] = 0
__global__ void edit_dense_kernel(float *dense, int ld, int rows, const int *n_rows, int set_feature,
                                  float set_value, int zero_feature) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int R = n_rows ? min(rows, *n_rows) : rows;
  if (r >= R) return;
  if (set_feature >= 0) dense[(size_t)r * ld + set_feature] = set_value;
  if (zero_feature >= 0) dense[(size_t)r * ld + zero_feature] = 0.f;
}

// list[0 .. T) = 0 .. T - 1, list[T] = T (the count), the words behind it 0: "every token is flagged" (msae_options::exact)
__global__ void iota_list_kernel(int *list, int T, int n_total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_total) list[i] = i < T ? i : (i == T ? T : 0);
}

// counts[c] = number of flagged tokens in pass c of the exact fallback
__global__ void fallback_counts_kernel(const int *n_flagged, int fb_cap, int chunks, int *counts) {
  const int nf = *n_flagged;
  for (int c = threadIdx.x; c < chunks; c += blockDim.x) {
    const int left = nf - c * fb_cap;
    counts[c] = left < 0 ? 0 : (left > fb_cap ? fb_cap : left);
  }
}

// msae_shard_candidates: where this shard's records go
struct ShardOut { unsigned char *recs; int C; int row_offset; };

// ---- stage profiling (bench.py roofline): HIP events recorded on the launch stream ------------------
constexpr int PROF_MARKS = 7;  // boundaries of: prep | sample gemm | tau topk | main gemm | rescore | fallback
struct ProfState {
  unsigned magic = 0x50524F46u;   // "PROF"
  int max_steps = 0, step = 0;
  hipEvent_t *ev = nullptr;
};

inline void prof_mark(ProfState *pf, int i, hipStream_t s) {
  if (pf && pf->step < pf->max_steps) (void)hipEventRecord(pf->ev[pf->step * PROF_MARKS + i], s);
}
inline void prof_step(ProfState *pf) {
  if (pf && pf->step < pf->max_steps) ++pf->step;
}

// ---- one call ------------------------------------------------------------------------------------
// What an entry point was given and nothing below it changes.  (msae_shard_candidates: W_enc, vals, idx, status null, the hook
// features local to the shard; msae_encode_topk_rows: T = max_rows; msae_rescore_candidates: T = token rows of the records.)
struct EncodeCall {
  const void *x; int x_dtype;
  const float *W_enc, *b_enc, *b_dec;
  int T, d, N, k;
  int set_feature; float set_value; int zero_feature;
  float *vals; IdxOut idx; int32_t *status;
  hipStream_t s;
  // the hook features as the candidate passes leave them out (-1: none)
  int skip_a() const { return set_feature >= 0 ? set_feature : -1; }
  int skip_b() const { return zero_feature >= 0 ? zero_feature : -1; }
};

// THE switch over x_dtype: f(std::integral_constant<int, MSAE_F32 | MSAE_BF16 | MSAE_F16>) for the paths whose kernels read x
template <class F>
inline int with_x_dtype(int x_dtype, F &&f) {
  switch (x_dtype) {
    case MSAE_F32: return f(std::integral_constant<int, MSAE_F32>{});
    case MSAE_BF16: return f(std::integral_constant<int, MSAE_BF16>{});
    default: return f(std::integral_constant<int, MSAE_F16>{});
  }
}

// ---- workspace carving -------------------------------------------------------------------------
// a region of the workspace (or of a prepared buffer) as the type stored there
template <class E> inline E *at(unsigned char *base, size_t off) { return reinterpret_cast<E *>(base + off); }
template <class E> inline const E *at(const unsigned char *base, size_t off) { return reinterpret_cast<const E *>(base + off); }
using u64 = unsigned long long;

// The in-call exact fallback's share of a workspace: the token list [listed] | its count (64 words) | per-pass counts [fb_chunks],
// and the dense f32 [fb_cap][N] scratch of one pass.  (listed = 0: the caller brings the list, msae_encode_topk_rows.)
struct FallbackPlan {
  size_t off_flag, off_fbdense;
  int fb_cap, fb_chunks;
  size_t flag_words(int listed) const { return (size_t)listed + 64 + fb_chunks; }
  int *flagged(unsigned char *ws) const { return at<int>(ws, off_flag); }
  int *n_flagged(unsigned char *ws, int listed) const { return flagged(ws) + listed; }
  int *pass_counts(unsigned char *ws, int listed) const { return flagged(ws) + listed + 64; }
  float *dense(unsigned char *ws) const { return at<float>(ws, off_fbdense); }
};
template <class Take>
inline FallbackPlan make_fallback_plan(int T, int N, int listed, Take &&take) {
  FallbackPlan f{};
  f.fb_cap = fallback_capacity(T, N);
  f.fb_chunks = (T + f.fb_cap - 1) / f.fb_cap;
  f.off_flag = take(f.flag_words(listed) * 4);
  f.off_fbdense = take((size_t)f.fb_cap * N * 4);
  return f;
}

// most rows one token may read before it is handed to the exact path (the needed set is ~k + 10:
// reaching this means the band is not separating anything); at least k + 4 (first-round minimum)
inline int rescore_row_budget(int k, int cap) {
  int r_max = k <= 64 ? 8 * k : 3 * k;
  if (r_max < k + 4) r_max = k + 4;
  return r_max > cap ? cap : r_max;
}

struct FusedPlan {
  bool fast, i8, small, fm, f8;
  size_t off_fmcount, off_fmtarget, off_fmkeys, off_fmpairs, off_fmpre, off_fmdefer;
  size_t off_xhi, off_xlo, off_skeys, off_sviol, off_surv, off_sbound, off_scand, off_stau;
  int Tp, S, r, cap, r_max;
  size_t off_rowe, off_cds, off_cds_s, off_cds_p;   // subtractive dither: (E, m) per token, Ds per column in the three column orders
  size_t off_xq, off_xqo, off_rowc, off_refs, off_colc, off_colc_s, off_colc_p, off_colmax, off_odims, off_isout, off_wqo, off_wqos;
  size_t off_xb, off_a32, off_sample, off_tauv, off_taui, off_cnt, off_cand, off_segcnt, off_segcand, off_dense, bytes;
  FallbackPlan fb;
  int segs;   // > 1: the candidate passes append to segmented lists (compact_candidates_kernel joins them)
};

inline FusedPlan make_plan(int T, int d, int N, int k, int mode, int shard_C = 0, bool cert = false) {
  FusedPlan p{};
  p.fast = fast_shape_ok(N, d) && T > EXACT_T_MAX && k <= 256 && k >= 1;
  if (cert && !cert_shape_ok(N, d)) p.fast = false;      // shapes without the certified pass: the exact path (certainly certified)
  if (cert) mode = 1;
  size_t o = 0;
  auto take = [&](size_t b) { size_t at = o; o += msae_align_up(b, 256); return at; };
  if (p.fast) {
    p.Tp = (T + G_BM - 1) / G_BM * G_BM;
    p.S = N / SAMPLE_STRIDE;
    // tau = r-th largest of the 1/32 sample: ~32*r survivors, Gamma(r)-distributed.  r = 16 keeps
    // P(fewer than ~2k survivors) and P(overflow) below 1e-9 per token (r = 8 flagged 3 of 8192)
    p.r = k / 8 > 16 ? k / 8 : 16;         // k = 256: r = 32 -> ~1024 survivors, capacity 4096
    if (k < 32) p.r = k / 2 > 8 ? k / 2 : 8;   // small k (a shard's k_loc): ~k + band rows are needed, 256+ survive
    // A shard of a feature-sharded group only has to deliver its C best: 256+ survivors are plenty (its share of
    // the needed set is below C / 1.5 by construction of C, P(Gamma(8) x 32 below that) ~ 1e-5), and the default
    // would put 512 survivors per token into 1/G of the columns -- at G = 8 that is 2048 per output tile, the
    // size of the epilogue's LDS queue.
    if (shard_C > 0) { const int rs = shard_C / 8 > 8 ? shard_C / 8 : 8; if (rs < p.r) p.r = rs; }
    p.cap = next_pow2(128 * p.r);           // 4x the expected count
    p.i8 = mode == 1 && i8_shape_ok(N, d);
    p.f8 = mode == 2 && i8_shape_ok(N, d);     // (other shapes: the bf16 pass, whose operands an fp8 prepare builds as well)
    p.small = !cert && p.i8 && small_shape_ok(T, d, N, k) && getenv("MSAE_NO_SMALL_PATH") == nullptr;
    p.r_max = rescore_row_budget(k, p.cap);
    if (p.i8 || p.f8) {   // the batch's massive-activation dims and the per-call column constants of the band
      p.off_colc = take((size_t)N * 16);
      p.off_colc_s = take((size_t)p.S * 16);
      p.off_colc_p = take(p.i8 ? (size_t)N * 16 : 0);
      p.off_colmax = take((size_t)d * 4 * COLMAX_PARTS);
      p.off_odims = take((size_t)(MAX_OUT + 1) * 4);
      p.off_isout = take((size_t)d);
    }
    if (p.i8) {
      p.off_xq = take((size_t)p.Tp * d * (cert ? 2 : 1));   // (certified: two planes per token row)
      p.off_xqo = take((size_t)p.Tp * MAX_OUT);
      p.off_wqo = take((size_t)N * MAX_OUT);
      p.off_wqos = take((size_t)p.S * MAX_OUT);
    }
    p.off_rowc = take((size_t)p.Tp * 16);
    p.off_rowe = take(p.i8 ? (size_t)p.Tp * 8 : 0);
    p.off_cds = take(p.i8 ? (size_t)N * 4 : 0);
    p.off_cds_s = take(p.i8 ? (size_t)p.S * 4 : 0);
    p.off_cds_p = take(p.i8 ? (size_t)N * 4 : 0);
    p.off_refs = take(256);
    if (p.small) {
      p.off_xhi = take((size_t)T * d);
      p.off_xlo = take((size_t)T * d);
      p.off_skeys = take((size_t)T * 128 * 8);
      p.off_surv = take((size_t)T * SMALL_SURV * 8);
      p.off_sbound = take((size_t)T * SMALL_GRID * 4);
      p.off_scand = take((size_t)T * 128 * 8);
      p.off_stau = take((size_t)T * 4);
      p.off_sviol = take((size_t)T * 2 * 4);            // model-check flags [T] | finished-wave counters [T]
    }
    p.off_xb = take(p.i8 ? 256 : (size_t)p.Tp * d * (p.f8 ? 1 : 2));
    p.off_a32 = take((size_t)T * d * 4);
    p.off_sample = take((size_t)T * p.S * 4);
    const size_t tau_n = (size_t)T * p.r;
    p.off_tauv = take(tau_n * 4);
    p.off_taui = take(tau_n * 4);
    p.off_cnt = take((size_t)T * 4);
    p.segs = (T <= 256 && p.cap >= 1024) ? 8 : 1;      // few tokens: hundreds of appends per list counter (GemmEpilogue::segs)
    p.off_segcnt = take(p.segs > 1 ? (size_t)T * p.segs * 4 : 0);   // right behind cnt: zeroed with it
    p.off_cand = take((size_t)T * p.cap * 8);
    p.off_segcand = take(p.segs > 1 ? (size_t)T * p.cap * 8 : 0);
    p.fb = make_fallback_plan(T, N, T, take);
    p.fm = shard_C == 0 && fm_shape_ok(T, k, N, d, p.r_max);    // feature-major first round of the re-score (encode_rescore.h)
    if (p.fm) {
      p.off_fmcount = take(((size_t)N + 64 + (N + FM_SCAN_BLOCK - 1) / FM_SCAN_BLOCK) * 4);   // counts [N] | total | block sums
      p.off_fmtarget = take((size_t)T * 4);
      p.off_fmkeys = take((size_t)T * p.r_max * 8);
      p.off_fmpairs = take(((size_t)T * p.r_max + (size_t)N * 16) * 8);   // slots: the pairs + every feature's padding to whole groups
      p.off_fmpre = take((size_t)T * p.r_max * 4);
      p.off_fmdefer = take((size_t)T * 2 * 4);              // tokens the LEAN launch of PHASE 1 / 2 left to the full-size one
    }
  } else {
    p.off_dense = take((size_t)T * N * 4);
  }
  p.bytes = o;
  return p;
}

// the buffers, plan and options of one fused call (run_small, run_fast and its operand preparations)
struct FusedCtx {
  const Prepared &pp; const unsigned char *prepared;
  unsigned char *ws; const FusedPlan &pl; const CallOpts &co;
  const unsigned *valid() const { return at<unsigned>(prepared, offsetof(Prepared, valid)); }
};

// exact recompute of a device-side list of tokens, fb_cap at a time (device-side counts; passes without work exit
// immediately): list[0 .. *n_list) of token rows, pass_counts[fb_chunks] scratch, dense f32[fb_cap][N] scratch
int run_exact_rows(const EncodeCall &c, const int *list, const int *n_list, int *pass_counts, float *dense,
                   const FallbackPlan &fb, int detail) {
  const int N = c.N, fb_cap = fb.fb_cap, fb_chunks = fb.fb_chunks;
  hipStream_t s = c.s;
  if (fb_chunks > 1)
    hipLaunchKernelGGL(fallback_counts_kernel, dim3(1), dim3(64), 0, s, n_list, fb_cap, fb_chunks, pass_counts);
  for (int p = 0; p < fb_chunks; ++p) {
    // one pass covers every token (T <= fb_cap): the list's count itself is the pass's row count
    const int *rows = list + (size_t)p * fb_cap, *n_rows = fb_chunks > 1 ? pass_counts + p : n_list;
    int rc = msae_pre_acts_launch(c.x, c.x_dtype, c.W_enc, c.b_enc, c.b_dec, rows, n_rows, fb_cap, c.d, N, 1, dense, N, s);
    if (rc) return rc;
    if (c.set_feature >= 0 || c.zero_feature >= 0)
      hipLaunchKernelGGL(edit_dense_kernel, dim3((fb_cap + 255) / 256), dim3(256), 0, s, dense, N, fb_cap, n_rows,
                         c.set_feature, c.set_value, c.zero_feature);
    // the exact results go straight to the listed tokens' rows of the outputs (row map = the list)
    TopkExtra ex;
    ex.idx64 = c.idx.i64; ex.row_map = rows; ex.status = c.status; ex.detail = detail;
    rc = msae_topk_launch(dense, fb_cap, N, c.k, N, n_rows, c.vals, c.idx.i32, s, ex);
    if (rc) return rc;
  }
  return 0;
}

// ... of the tokens the fused path flagged
int run_exact_fallback(const EncodeCall &c, unsigned char *ws, const FallbackPlan &fb, int detail) {
  return run_exact_rows(c, fb.flagged(ws), fb.n_flagged(ws, c.T), fb.pass_counts(ws, c.T), fb.dense(ws), fb, detail);
}

inline int dot4_max_small() {   // largest T of the dot4 weight stream (tuning knob; the MFMA stream takes the rest of the small path)
  // (at most SMALL_T_DOT4: gemv_small_kernel is instantiated for 1, 2 and 4 tokens)
  static const int v = [] {
    const char *e = getenv("MSAE_SMALL_DOT4_MAX");
    const int m = e ? atoi(e) : SMALL_DOT4_PREF;
    return m < SMALL_T_DOT4 ? m : SMALL_T_DOT4;
  }();
  return v;
}

template <int DT>
int run_small(const EncodeCall &c, const FusedCtx &fx) {
  const Prepared &pp = fx.pp; const FusedPlan &pl = fx.pl; const CallOpts &co = fx.co;
  const unsigned char *prepared = fx.prepared; unsigned char *ws = fx.ws;
  const int T = c.T, d = c.d, N = c.N;
  const float *b_enc = c.b_enc;
  hipStream_t s = c.s;
  // zz12: z^2 x the W-side variance of one rounding inside P_t (the dither's factor 3 is in Q_n); zzx: ... of the x side
  const float z = co.z, zz12 = z * z / 12.f, zzx = z * z * x_round_var(co.seed != 0ull);
  float *a32 = at<float>(ws, pl.off_a32);
  signed char *xhi = at<signed char>(ws, pl.off_xhi), *xlo = at<signed char>(ws, pl.off_xlo);
  f32x4 *rowc = at<f32x4>(ws, pl.off_rowc);
  u64 *surv = at<u64>(ws, pl.off_surv), *cand = at<u64>(ws, pl.off_scand), *exact = at<u64>(ws, pl.off_skeys);
  unsigned *bound = at<unsigned>(ws, pl.off_sbound);
  float *tau = at<float>(ws, pl.off_stau);
  int *viol = at<int>(ws, pl.off_sviol), *done = viol + T;
  int *flagged = pl.fb.flagged(ws), *n_flagged = pl.fb.n_flagged(ws, T);
  const signed char *wq = at<signed char>(prepared, pp.off_wq);
  const signed char *wqf = at<signed char>(prepared, pp.off_wqf), *wqsf = at<signed char>(prepared, pp.off_wqsf);   // fragment-major copies (MFMA stream)
  const f32x4 *wstat = at<f32x4>(prepared, pp.off_wstat);
  const unsigned *valid = fx.valid();
  const bool mfma_stream = T > dot4_max_small() && d <= 4096;
  prof_mark(co.prof, 0, s);
  hipLaunchKernelGGL(prep_small_kernel<DT>, dim3(T), dim3(256), 0, s, c.x, c.b_dec, d, a32, xhi, xlo, rowc, zz12, viol, 2 * T,
                     flagged, (int)pl.fb.flag_words(T), valid, mfma_stream ? (PREP_I8 | PREP_FRAG) : PREP_I8, T, co.seed);
  prof_mark(co.prof, 1, s);
  prof_mark(co.prof, 2, s);
  prof_mark(co.prof, 3, s);
  const int skip_a = c.skip_a(), skip_b = c.skip_b();
  // every case below is a member of small_kernel_for (encode_small.h), which is what the plan asked; `default` is a defence
#define MSAE_GEMV(DSEG, TT)                                                                                        \
  static_assert(small_kernel_for(DSEG, TT), "a dot4 stream kernel outside the small path's shape set");            \
  hipLaunchKernelGGL((gemv_small_kernel<DSEG, TT>), dim3(SMALL_GRID), dim3(256), 0, s, wq, wstat, b_enc, N, T, xhi, xlo, \
                     rowc, zzx, skip_a, skip_b, surv, bound)
  const int dseg = d / 1024;
  int n_surv = SMALL_SURV, n_bound = SMALL_GRID;
  if (mfma_stream) {
    static int n_cu = [] {
      int dev = 0, cus = 256;
      if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
      return cus > 0 ? cus : 256;
    }();
    const int grid_m = n_cu < SMALL_GRID ? n_cu : SMALL_GRID;
    n_surv = grid_m * SMALL_MF_EMIT; n_bound = grid_m;
    const size_t smem_m = (size_t)2 * 16 * (d + 16) + (size_t)16 * 8 * (SMALL_MF_EMIT + 1) * 8;
#define MSAE_GEMV_M(DSEG)                                                                                          \
  do {                                                                                                             \
    static_assert(small_kernel_for(DSEG, SMALL_T_MAX), "an MFMA stream kernel outside the small path's shape set"); \
    MSAE_HIP_TRY(hipFuncSetAttribute((const void *)gemv_mfma_kernel<DSEG>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                     (int)smem_m));                                                                \
    hipLaunchKernelGGL(gemv_mfma_kernel<DSEG>, dim3(grid_m), dim3(512), smem_m, s, wqf, wqsf, wstat, b_enc, N, T, xhi, xlo, rowc, \
                       zzx, skip_a, skip_b, surv, bound);                                                          \
  } while (0)
    switch (dseg) { case 1: MSAE_GEMV_M(1); break; case 2: MSAE_GEMV_M(2); break; case 4: MSAE_GEMV_M(4); break;
                    default: return MSAE_ENOTIMPL; }
#undef MSAE_GEMV_M
  } else if (T == 1) {
    switch (dseg) { case 1: MSAE_GEMV(1, 1); break; case 2: MSAE_GEMV(2, 1); break; case 4: MSAE_GEMV(4, 1); break;
                    case 8: MSAE_GEMV(8, 1); break; default: return MSAE_ENOTIMPL; }
  } else if (T == 2) {
    switch (dseg) { case 1: MSAE_GEMV(1, 2); break; case 2: MSAE_GEMV(2, 2); break; case 4: MSAE_GEMV(4, 2); break;
                    case 8: MSAE_GEMV(8, 2); break; default: return MSAE_ENOTIMPL; }
  } else {
    switch (dseg) { case 1: MSAE_GEMV(1, 4); break; case 2: MSAE_GEMV(2, 4); break; case 4: MSAE_GEMV(4, 4); break;
                    default: return MSAE_ENOTIMPL; }
  }
#undef MSAE_GEMV
  hipLaunchKernelGGL(select_small_kernel, dim3(T), dim3(1024), 0, s, surv, bound, cand, tau, n_surv, n_bound);
  prof_mark(co.prof, 4, s);
#define MSAE_RESCORE(DSEG)                                                                                         \
  static_assert(small_kernel_for(DSEG, 1), "a re-score kernel outside the small path's shape set");                \
  hipLaunchKernelGGL(rescore_small_kernel<DSEG>, dim3(SMALL_RMAX, T), dim3(64), 0, s, a32, c.W_enc, b_enc, c.k, cand, tau, wstat, \
                     rowc, zzx, z * z, guard_z_check2(co.seed != 0ull), c.set_feature, c.set_value, exact, viol, done, c.vals, \
                     c.idx, c.status, flagged, n_flagged)
  switch (dseg) { case 1: MSAE_RESCORE(1); break; case 2: MSAE_RESCORE(2); break; case 4: MSAE_RESCORE(4); break;
                  case 8: MSAE_RESCORE(8); break; default: return MSAE_ENOTIMPL; }
#undef MSAE_RESCORE
  prof_mark(co.prof, 5, s);
  const int rc = run_exact_fallback(c, ws, pl.fb, co.detail);
  if (rc) return rc;
  prof_mark(co.prof, 6, s);
  prof_step(co.prof);
  return msae_launch_status();
}

// select + exact re-score of the candidate lists (RescoreArgs filled by the caller): token-major, or with the FEATURE-major first
// round where the plan has it and the cost model says it pays (encode_rescore.h)
template <int DT>
int rescore_stage(RescoreArgs &ra, const float *a32, const EncodeCall &c, unsigned char *ws, const FusedPlan &pl) {
  const int T = c.T, d = c.d, N = c.N, k = c.k;
  hipStream_t s = c.s;
  // (fm_dot_kernel reads x in 16-B pieces; the entry points ask 8 B of a 16-bit x)
  if (!(pl.fm && msae_aligned(c.x, 16) && fm_pays(T, k, N, d, DT == MSAE_F32 ? 4 : 2)))
    return launch_select_rescore<false>(ra, a32, c.W_enc, s);
  int *fcount = at<int>(ws, pl.off_fmcount);
  int2 *pairs = at<int2>(ws, pl.off_fmpairs);
  float *fpre = at<float>(ws, pl.off_fmpre);
  RescoreFm &fm = ra.fm;
  fm.count = fcount; fm.target = at<int>(ws, pl.off_fmtarget);
  fm.keys = at<u64>(ws, pl.off_fmkeys); fm.pre = fpre; fm.rcap = pl.r_max; fm.cand = at<u64>(ws, pl.off_cand);
  fm.rank = reinterpret_cast<int *>(fpre);
  fm.defer = at<int>(ws, pl.off_fmdefer);             // (defer and fcount[0 .. N]: zeroed at the start of the call, zero_call_scratch)
  const int lrc = launch_select_rescore<false, 1>(ra, a32, c.W_enc, s);
  if (lrc) return lrc;
  const int scan_blocks = (N + FM_SCAN_BLOCK - 1) / FM_SCAN_BLOCK, G = fm_group_lanes(T, k, N);
  hipLaunchKernelGGL(fm_blocksum_kernel, dim3(scan_blocks), dim3(256), 0, s, fcount, N, G, fcount + N + 64);
  hipLaunchKernelGGL(fm_scan_kernel, dim3(scan_blocks), dim3(256), 0, s, fcount, N, G, fcount + N + 64, pairs);
  hipLaunchKernelGGL(fm_scatter_kernel, dim3(T), dim3(256), 0, s, fm.target, fm.keys, fm.rank, pl.r_max, fcount, pairs);
  const long max_slots = (long)T * pl.r_max + (long)N * (G - 1);
  const dim3 dgrid((unsigned)((max_slots + 63) / 64));
  if (G == 16) hipLaunchKernelGGL((fm_dot_kernel<DT, 16>), dgrid, dim3(64), 0, s, c.x, c.b_dec, c.W_enc, c.b_enc, pairs, fcount + N, d, pl.r_max, fpre);
  else hipLaunchKernelGGL((fm_dot_kernel<DT, 4>), dgrid, dim3(64), 0, s, c.x, c.b_dec, c.W_enc, c.b_enc, pairs, fcount + N, d, pl.r_max, fpre);
  return launch_select_rescore<false, 2>(ra, a32, c.W_enc, s);
}

// ---- the candidate pipeline (stages 2 to 6 of the header) ------------------------------------------------------------------
// What one operand preparation hands to it: everything in which the int8, fp8, bf16 and certified passes differ.
enum CandidateGemm { GEMM_BF16, GEMM_I8, GEMM_F8, GEMM_I8_CERT };
struct CandidatePass {
  GemmOperands op_main, op_samp;
  CandidateGemm gemm;
  int skinny;                  // 64 / 128 / 256: token rows of the weight-stream kernel's tile (gemm_skinny.h) runs both passes; 0: gemm_mfma.h
  bool skip_sample;            // the main pass leaves the sample features out (MAIN_SKIPS_SAMPLE: its operand holds the other rows only)
  const float *bias;           // b_enc (certified: its upper bias)
  // error-band column constants: of the sample pass, of the main pass in ITS column order, and by feature (records, re-score)
  const f32x4 *colc_s, *colc_main, *colc;
  float zzx;                   // z^2 x the x-side variance of one rounding (fp8: of the absolute grid; certified: CERT_ZZX)
  const int2 *row_e;           // subtractive dither (encode_defs.h) or null: (E, m) per token, Ds per column of the main / sample pass
  const float *cds_main, *cds_s;
  float z2, zc2;               // the re-score's z^2 and its model check
  int i8;                      // the three-term band (int8, fp8, certified)
};

// zeroes the call's scratch: candidate counters (+ segment counters), flag list, for the passes that pick outlier dims the
// column maxima, and where the plan has the feature-major re-score its pair counters [N + 1] and defer flags [2 T] -- nothing
// in front of rescore_stage touches those two (their only user), so they need no launches of their own there
void zero_call_scratch(const EncodeCall &c, unsigned char *ws, const FusedPlan &pl, bool colmax) {
  const size_t n_cnt = pl.segs > 1 ? (pl.off_segcnt - pl.off_cnt) / 4 + (size_t)c.T * pl.segs : (size_t)c.T;
  ZeroRanges z{};
  z.p[0] = at<int>(ws, pl.off_cnt); z.n[0] = n_cnt;
  z.p[1] = pl.fb.flagged(ws); z.n[1] = pl.fb.flag_words(c.T);
  if (colmax) { z.p[2] = at<int>(ws, pl.off_colmax); z.n[2] = (size_t)c.d * COLMAX_PARTS; }
  if (pl.fm) {
    z.p[3] = at<int>(ws, pl.off_fmcount); z.n[3] = (size_t)c.N + 1;
    z.p[4] = at<int>(ws, pl.off_fmdefer); z.n[4] = (size_t)c.T * 2;
  }
  hipLaunchKernelGGL(zero_ranges_i32_kernel, dim3(pl.fm ? 256 : 64), dim3(256), 0, c.s, z);
}

// the sample (DENSE) or main pass of `cp` over n_cols columns
template <bool DENSE>
int launch_candidate_gemm(const CandidatePass &cp, const EncodeCall &c, const FusedPlan &pl, int n_cols, const GemmEpilogue &ep) {
  const GemmOperands &op = DENSE ? cp.op_samp : cp.op_main;
  switch (cp.skinny) {
    case 64: return gemm_skinny_launch<64, DENSE>(op, c.T, c.d, n_cols, ep, c.s);
    case 128: return gemm_skinny_launch<128, DENSE>(op, c.T, c.d, n_cols, ep, c.s);
    case 256: return gemm_skinny_launch<256, DENSE>(op, c.T, c.d, n_cols, ep, c.s);
  }
  switch (cp.gemm) {
    case GEMM_I8: return gemm_launch<GemmI8, DENSE>(op, c.T, pl.Tp, n_cols, ep, c.s);
    case GEMM_F8: return gemm_launch<GemmF8, DENSE>(op, c.T, pl.Tp, n_cols, ep, c.s);
    case GEMM_I8_CERT: return gemm_launch<GemmI8Cert, DENSE>(op, c.T, pl.Tp, n_cols, ep, c.s);
    default: return gemm_launch<GemmBf16, DENSE>(op, c.T, pl.Tp, n_cols, ep, c.s);
  }
}

// band_refs -> sample GEMM -> threshold (+ the sample features' own candidates) -> main GEMM -> compact -> shard: pack the records |
// select + exact re-score -> exact fallback.  The caller has recorded mark 0, zeroed the scratch and prepared the operands.
template <int DT>
int run_candidate_pipeline(const EncodeCall &c, unsigned char *ws, const FusedPlan &pl, const CallOpts &co, const CandidatePass &cp,
                           const ShardOut *shard) {
  const int T = c.T, N = c.N;
  hipStream_t s = c.s;
  float *a32 = at<float>(ws, pl.off_a32), *sample = at<float>(ws, pl.off_sample), *tauv = at<float>(ws, pl.off_tauv);
  float *refs = at<float>(ws, pl.off_refs);
  const f32x4 *rowc = at<f32x4>(ws, pl.off_rowc);
  int *cnt = at<int>(ws, pl.off_cnt);
  u64 *cand = at<u64>(ws, pl.off_cand);
  // producers of the candidate lists write the segmented lists when the plan has them (compact_candidates_kernel joins them)
  int *pcnt = pl.segs > 1 ? at<int>(ws, pl.off_segcnt) : cnt;
  u64 *pcand = pl.segs > 1 ? at<u64>(ws, pl.off_segcand) : cand;
  const int seg_cap = pl.cap / pl.segs;
  const int skip_a = c.skip_a(), skip_b = c.skip_b();
  hipLaunchKernelGGL(band_refs_kernel, dim3(1), dim3(1024), 0, s, cp.colc_s, pl.S, refs);
  prof_mark(co.prof, 1, s);
  {  // sample pass -> dense [T][S]
    GemmEpilogue ep{};
    ep.bias = cp.bias; ep.bias_stride = SAMPLE_STRIDE; ep.bias_off = SAMPLE_OFF;
    ep.dense = sample; ep.ld_dense = pl.S;
    ep.rowc = rowc; ep.colc = cp.colc_s; ep.refs = refs; ep.zz12 = cp.zzx;
    ep.row_e = cp.row_e; ep.col_ds = cp.cds_s;
    const int grc = launch_candidate_gemm<true>(cp, c, pl, pl.S, ep);
    if (grc) return grc;
  }
  prof_mark(co.prof, 2, s);
  // the sample features' own candidates, when the main pass leaves them out: from the threshold select itself (it holds
  // the row in registers), or by sample_push_kernel for the shapes / calls it does not cover (hook edits: features to skip)
  KthPush push{};
  bool pushed = false;
  if (cp.skip_sample && skip_a < 0 && skip_b < 0) {
    push.cnt = pcnt; push.cand = pcand; push.cap = seg_cap; push.stride = SAMPLE_STRIDE; push.off = SAMPLE_OFF;
    push.cnt_stride = pl.segs; push.row_stride = pl.cap;
    pushed = true;
  }
  if (!msae_kth_value_launch(sample, T, pl.S, pl.S, pl.r, tauv, pl.r, pl.r - 1, s, push)) {
    const int rc = msae_topk_launch(sample, T, pl.S, pl.r, pl.S, nullptr, tauv, at<int32_t>(ws, pl.off_taui), s);  // generic shapes
    if (rc) return rc;
    pushed = false;
  }
  if (cp.skip_sample && !pushed)
    hipLaunchKernelGGL(sample_push_kernel, dim3(T), dim3(256), 0, s, sample, pl.S, tauv, pl.r, pl.r - 1, skip_a, skip_b, pcnt,
                       pcand, seg_cap, pl.segs, pl.cap);
  prof_mark(co.prof, 3, s);
  {  // full pass with the threshold epilogue
    GemmEpilogue ep{};
    ep.bias = cp.bias; ep.bias_stride = 1; ep.bias_off = 0;
    if (cp.skip_sample) { ep.skip_stride = SAMPLE_STRIDE; ep.skip_off = SAMPLE_OFF; }
    ep.tau_vals = tauv; ep.tau_ld = pl.r; ep.tau_col = pl.r - 1;
    ep.cnt = pcnt; ep.cand = pcand; ep.cap = pl.cap; ep.segs = pl.segs;
    ep.skip_a = skip_a; ep.skip_b = skip_b;
    ep.rowc = rowc; ep.colc = cp.colc_main; ep.refs = refs; ep.zz12 = cp.zzx;
    ep.row_e = cp.row_e; ep.col_ds = cp.cds_main;
    if constexpr (msae_tuning::GEMM_TIMELINE != 0) {
      if (!g_timeline) (void)hipMalloc(&g_timeline, 64 * 8 * 8);
      (void)hipMemsetAsync(g_timeline, 0, 64 * 8 * 8, s);
      ep.timeline = g_timeline;
    }
    const int grc = launch_candidate_gemm<false>(cp, c, pl, cp.skip_sample ? N - pl.S : N, ep);
    if (grc) return grc;
  }
  if (pl.segs > 1)
    hipLaunchKernelGGL(compact_candidates_kernel, dim3(T), dim3(64), 0, s, pcnt, pcand, pl.segs, pl.cap, cnt, cand);
  prof_mark(co.prof, 4, s);
  if (shard) {   // feature-sharded group: this shard's best candidates travel, the owner of the token re-scores
    PackArgs pa{};
    pa.cnt = cnt; pa.cand = cand; pa.cap = pl.cap;
    pa.tau_vals = tauv; pa.tau_ld = pl.r; pa.tau_col = pl.r - 1;
    pa.rowc = rowc; pa.colc = cp.colc; pa.zz12 = cp.zzx; pa.i8 = cp.i8;
    pa.C = shard->C; pa.row_offset = shard->row_offset; pa.stride = shard_record_bytes(shard->C);
    pa.recs = shard->recs;
    if (pl.cap <= 64 * 32) hipLaunchKernelGGL(pack_candidates_kernel<32>, dim3(T), dim3(64), 0, s, pa);
    else if (pl.cap <= 64 * 64) hipLaunchKernelGGL(pack_candidates_kernel<64>, dim3(T), dim3(64), 0, s, pa);
    else return MSAE_ENOTIMPL;
    prof_mark(co.prof, 5, s);
    prof_mark(co.prof, 6, s);
    prof_step(co.prof);
    return msae_launch_status();
  }
  {
    RescoreArgs ra{};
    ra.b_enc = c.b_enc;
    ra.tau_vals = tauv; ra.tau_ld = pl.r; ra.tau_col = pl.r - 1;
    ra.cnt = cnt; ra.cand = cand; ra.cap = pl.cap;
    ra.T = T; ra.d = c.d; ra.k = c.k; ra.r_max = pl.r_max;
    ra.rowc = rowc; ra.colc = cp.colc; ra.zz12 = cp.zzx; ra.z2 = cp.z2; ra.i8 = cp.i8; ra.zc2 = cp.zc2;
    ra.set_feature = c.set_feature; ra.set_value = c.set_value;
    ra.vals = c.vals; ra.idx = c.idx.i32; ra.idx64 = c.idx.i64; ra.status = c.status;
    ra.flagged = pl.fb.flagged(ws); ra.n_flagged = pl.fb.n_flagged(ws, T);
    ra.fb_cap = T;
    ra.rows_out = co.rows_out;
    const int lrc = rescore_stage<DT>(ra, a32, c, ws, pl);
    if (lrc) return lrc;
  }
  prof_mark(co.prof, 5, s);
  if constexpr (!msae_tuning::ABL_NOFALLBACK) {
    const int rc = run_exact_fallback(c, ws, pl.fb, co.detail);
    if (rc) return rc;
  }
  prof_mark(co.prof, 6, s);
  prof_step(co.prof);
  return msae_launch_status();
}

// ---- operand preparation (stage 1): each launches its kernels and describes its pass -------------------------------------------
// a thread owns four columns, ~16 rows per thread: 2048 workgroups at T = 8192
inline dim3 colmax_grid(int T, int d) { return dim3((d / 4 + 255) / 256, T >= 32 ? (T / 16 < 512 ? T / 16 : 512) : 1); }

// int8: column max over the batch -> outlier dims -> per-token scale, int8 rows, the outlier tile of both operands, the per-call
// column constants.  shard: no re-score on this rank -- quantise straight from x - b_dec, a32 is never written.
template <int DT>
CandidatePass prep_i8(const EncodeCall &c, const FusedCtx &fx, bool shard) {
  const Prepared &pp = fx.pp; const FusedPlan &pl = fx.pl; const CallOpts &co = fx.co;
  const unsigned char *prepared = fx.prepared; unsigned char *ws = fx.ws;
  const int T = c.T, d = c.d, N = c.N;
  hipStream_t s = c.s;
  float *a32 = at<float>(ws, pl.off_a32);
  signed char *xq = at<signed char>(ws, pl.off_xq), *xqo = at<signed char>(ws, pl.off_xqo);
  signed char *wqo = at<signed char>(ws, pl.off_wqo), *wqos = at<signed char>(ws, pl.off_wqos);
  f32x4 *rowc = at<f32x4>(ws, pl.off_rowc);
  f32x4 *cc_main = at<f32x4>(ws, pl.off_colc), *cc_samp = at<f32x4>(ws, pl.off_colc_s), *cc_perm = at<f32x4>(ws, pl.off_colc_p);
  unsigned *colmax = at<unsigned>(ws, pl.off_colmax);
  int *odims = at<int>(ws, pl.off_odims);
  unsigned char *is_out = ws + pl.off_isout;
  int2 *rowe = at<int2>(ws, pl.off_rowe);
  const signed char *wq = at<signed char>(prepared, pp.off_wq), *wqs = at<signed char>(prepared, pp.off_wqs);
  // tile-major operands for the candidate GEMM (MSAE_GEMM_ROWMAJOR=1: the row-major copies, for A/B runs)
  // one row of output tiles (T <= 256) streams Wq from HBM once and keeps round 2's row-major operands + unstaggered
  // issue: tile-major + stagger measured 2-3 % slower there (profiles/r03_ab_small_T.txt)
  const int tile_major = pl.Tp > G_BM ? gemm_layout() : 0;
  // up to 256 tokens: the weight-stream kernel (gemm_skinny.h) runs both candidate passes: xq row-major, Wq fragment-major
  int skinny = 0;
  if (T <= 256 && tile_major == 0 && gemm_layout() == 1 && d % 1024 == 0 && N % (SAMPLE_STRIDE * 256) == 0 &&
      getenv("MSAE_NO_SKINNY") == nullptr)
    skinny = T <= 64 ? 64 : (T <= 128 ? 128 : 256);
  const bool w_packed = tile_major == 1 || skinny != 0;   // the W side of the candidate passes reads the tile-major copies
  if (shard)
    hipLaunchKernelGGL((prep_colmax_kernel<DT, false>), colmax_grid(T, d), dim3(256), 0, s, c.x, c.b_dec, T, d, (float *)nullptr,
                       colmax);
  else
    hipLaunchKernelGGL((prep_colmax_kernel<DT, true>), colmax_grid(T, d), dim3(256), 0, s, c.x, c.b_dec, T, d, a32, colmax);
  hipLaunchKernelGGL(pick_outliers_kernel, dim3(1), dim3(1024), 0, s, colmax, d, odims, is_out);
  const unsigned need = skinny ? (PREP_I8 | PREP_FRAG) : PREP_I8;   // operands this call's candidate passes read
  // the candidate passes (gemm_mfma.h, gemm_skinny.h) subtract the shared dither again: both roundings uniform with variance 1/12, for every input
  const bool sd = co.seed != 0ull && getenv("MSAE_NO_SUBTRACT") == nullptr;
  // (see run_small) zz12: the W side inside P_t, zzx: the x side
  const float z = co.z, zz12 = sd ? z * z / 12.f * sd_slack(z, d) : z * z / 12.f, zzx = sd ? zz12 : z * z * x_round_var(co.seed != 0ull);
  const u64 *dseed_p = at<u64>(prepared, offsetof(Prepared, dseed));
  const int *sdtab = sd ? at<int>(prepared, pp.off_sdtab) : nullptr;
  auto quant = [&](auto kernel, const void *src, const float *sub) {
    hipLaunchKernelGGL(kernel, dim3(pl.Tp), dim3(256), 0, s, src, sub, T, d, (const int *)odims, (const unsigned char *)is_out, xq, xqo,
                       rowc, zz12, tile_major, fx.valid(), need, co.seed, dseed_p, rowe, sdtab);
  };
  // (not a shard: from a32 -- reading the caller's 16-bit x + b_dec instead measured +0.016 ms, the kernel is bound by its
  // instructions, not its bytes)
  if (shard && sd) quant(quant_x_kernel<DT, true, true>, c.x, c.b_dec);
  else if (shard) quant(quant_x_kernel<DT, true, false>, c.x, c.b_dec);
  else if (sd) quant(quant_x_kernel<MSAE_F32, false, true>, a32, nullptr);
  else quant(quant_x_kernel<MSAE_F32, false, false>, a32, nullptr);
  const bool skip_sample = MAIN_SKIPS_SAMPLE && w_packed;   // the tile-major main operand holds the non-sample rows only
  hipLaunchKernelGGL(gather_wo_kernel, dim3(N / 32), dim3(256), 0, s, wq, N, d, odims, at<f32x4>(prepared, pp.off_wstat), wqo, wqos,
                     cc_main, cc_samp, cc_perm, skip_sample ? 1 : 0, sd ? at<float>(prepared, pp.off_ds) : (const float *)nullptr,
                     at<float>(ws, pl.off_cds), at<float>(ws, pl.off_cds_s), at<float>(ws, pl.off_cds_p));
  CandidatePass cp{};
  cp.gemm = GEMM_I8; cp.skinny = skinny; cp.skip_sample = skip_sample;
  cp.bias = c.b_enc;
  cp.colc = cc_main; cp.colc_s = cc_samp; cp.colc_main = skip_sample ? cc_perm : cc_main;
  cp.zzx = zzx;
  if (sd) {
    cp.row_e = rowe; cp.cds_s = at<float>(ws, pl.off_cds_s);
    cp.cds_main = at<float>(ws, skip_sample ? pl.off_cds_p : pl.off_cds);
  }
  // (subtractive dither: the band's sigma is the residuals' actual one again -- 6 sigma, as for round to nearest)
  cp.z2 = z * z; cp.zc2 = guard_z_check2(co.seed != 0ull && !sd); cp.i8 = 1;
  GemmOperands &om = cp.op_main;
  om.A = reinterpret_cast<const unsigned char *>(xq); om.ldA = d;
  om.B = skinny ? prepared + pp.off_wqf : tile_major ? prepared + pp.off_wqp : reinterpret_cast<const unsigned char *>(wq);
  om.ldB = d;
  om.nk = tile_major == 2 ? d / 64 : d / 128;
  om.packed = skinny ? 3 : tile_major;
  om.Ao = reinterpret_cast<const unsigned char *>(xqo);
  om.Bo = reinterpret_cast<const unsigned char *>(wqo);
  om.n_out = odims + MAX_OUT;
  cp.op_samp = om;
  cp.op_samp.B = skinny ? prepared + pp.off_wqsf : tile_major ? prepared + pp.off_wqsp : reinterpret_cast<const unsigned char *>(wqs);
  cp.op_samp.Bo = reinterpret_cast<const unsigned char *>(wqos);
  if constexpr (msae_tuning::ABL_NOLEAD) { om.Ao = nullptr; om.Bo = nullptr; }   // (tuning builds; results invalid)
  return cp;
}

// fp8: e4m3 operands, x scaled per token, W per feature (prepared), both tile-major like the int8 operands; no outlier tile (the
// format's own dynamic range takes the massive-activation dims), the main pass over ALL features like the bf16 pass
template <int DT>
CandidatePass prep_f8(const EncodeCall &c, const FusedCtx &fx) {
  const Prepared &pp = fx.pp; const FusedPlan &pl = fx.pl;
  unsigned char *ws = fx.ws;
  const int T = c.T, d = c.d, N = c.N;
  hipStream_t s = c.s;
  const float z = fx.co.z;
  float *a32 = at<float>(ws, pl.off_a32);
  signed char *x8 = at<signed char>(ws, pl.off_xb);
  unsigned *colmax = at<unsigned>(ws, pl.off_colmax);
  int *odims = at<int>(ws, pl.off_odims);
  unsigned char *is_out = ws + pl.off_isout;
  f32x4 *cc_main = at<f32x4>(ws, pl.off_colc), *cc_samp = at<f32x4>(ws, pl.off_colc_s);
  hipLaunchKernelGGL((prep_colmax_kernel<DT, true>), colmax_grid(T, d), dim3(256), 0, s, c.x, c.b_dec, T, d, a32, colmax);
  hipLaunchKernelGGL(pick_outliers_kernel, dim3(1), dim3(1024), 0, s, colmax, d, odims, is_out);
  hipLaunchKernelGGL(quant_x_fp8_kernel, dim3(pl.Tp), dim3(256), 0, s, (const float *)a32, T, d, (const unsigned char *)is_out, x8,
                     at<f32x4>(ws, pl.off_rowc), z * z, fx.valid());
  hipLaunchKernelGGL(gather_wo_fp8_kernel, dim3(N / 32), dim3(256), 0, s, c.W_enc, N, d, (const int *)odims,
                     at<f32x4>(fx.prepared, pp.off_colbf), cc_main, cc_samp);
  CandidatePass cp{};
  cp.gemm = GEMM_F8;
  cp.bias = c.b_enc;
  cp.colc = cc_main; cp.colc_s = cc_samp; cp.colc_main = cc_main;
  cp.zzx = z * z * FP8_ABS_VAR;   // the band's absolute-grid terms (encode_defs.h)
  cp.z2 = z * z; cp.zc2 = guard_z_check2(false); cp.i8 = 1;   // (the three-term band as well)
  GemmOperands &om = cp.op_main;
  om.A = reinterpret_cast<const unsigned char *>(x8); om.ldA = d;
  om.B = fx.prepared + pp.off_wq; om.ldB = d;
  om.nk = d / 128;
  om.packed = 1;
  cp.op_samp = om;
  cp.op_samp.B = fx.prepared + pp.off_wqsp;
  return cp;
}

// bf16: xb = bf16(x - b_dec), the column constants are the prepared buffer's
template <int DT>
CandidatePass prep_bf16(const EncodeCall &c, const FusedCtx &fx) {
  const Prepared &pp = fx.pp; const FusedPlan &pl = fx.pl;
  const int T = c.T, d = c.d;
  const float z = fx.co.z;
  unsigned short *xb = at<unsigned short>(fx.ws, pl.off_xb);
  float *a32 = at<float>(fx.ws, pl.off_a32);
  hipLaunchKernelGGL(prep_x_kernel<DT>, dim3(2048), dim3(256), 0, c.s, c.x, c.b_dec, T, pl.Tp, d, xb, a32);
  hipLaunchKernelGGL(row_p4_kernel, dim3(T), dim3(256), 0, c.s, a32, T, d, at<f32x4>(fx.ws, pl.off_rowc), z * z, fx.valid());
  CandidatePass cp{};
  cp.gemm = GEMM_BF16;
  cp.bias = c.b_enc;
  cp.colc = at<f32x4>(fx.prepared, pp.off_colbf); cp.colc_s = at<f32x4>(fx.prepared, pp.off_colbf_s); cp.colc_main = cp.colc;
  cp.zzx = z * z * x_round_var(false);
  cp.z2 = z * z; cp.zc2 = guard_z_check2(false); cp.i8 = 0;
  GemmOperands &om = cp.op_main;
  om.A = reinterpret_cast<const unsigned char *>(xb); om.ldA = (size_t)d * 2;
  om.B = fx.prepared + pp.off_wb; om.ldB = (size_t)d * 2;
  om.nk = d / 64;
  cp.op_samp = om;
  cp.op_samp.B = fx.prepared + pp.off_ws;
  return cp;
}

// the fused path of more than 16 tokens; with `shard` the body of msae_shard_candidates (no a32, no W_enc, no outputs but the records)
template <int DT>
int run_fast(const EncodeCall &c, const FusedCtx &fx, const ShardOut *shard = nullptr) {
  const FusedPlan &pl = fx.pl;
  prof_mark(fx.co.prof, 0, c.s);
  zero_call_scratch(c, fx.ws, pl, pl.i8 || pl.f8);
  const CandidatePass cp = pl.i8 ? prep_i8<DT>(c, fx, shard != nullptr) : pl.f8 ? prep_f8<DT>(c, fx) : prep_bf16<DT>(c, fx);
  return run_candidate_pipeline<DT>(c, fx.ws, pl, fx.co, cp, shard);
}

// msae_options::certified: the same pipeline with the certified candidate pass (encode_cert.h) in front of the unchanged select +
// exact re-score -- two planes per operand, no outlier tile, static column constants, z = 1 (the band IS the bound) and a model
// check at exactly the band (a violation can only mean operands that do not belong to the weights).
template <int DT>
int run_cert(const EncodeCall &c, const unsigned char *cprep, unsigned char *ws, const FusedPlan &pl, const CallOpts &co) {
  const CertPrepared cq = make_cert_prepared(c.N, c.d);
  const int T = c.T, d = c.d;
  float *a32 = at<float>(ws, pl.off_a32);
  signed char *xp = at<signed char>(ws, pl.off_xq);
  prof_mark(co.prof, 0, c.s);
  zero_call_scratch(c, ws, pl, false);
  // (this path has always given prep_x_kernel T, not the plan's Tp, as the padded row count: no xb rows to zero)
  hipLaunchKernelGGL(prep_x_kernel<DT>, dim3(2048), dim3(256), 0, c.s, c.x, c.b_dec, T, T, d, (unsigned short *)nullptr, a32);
  hipLaunchKernelGGL(cert_quant_x_kernel, dim3(pl.Tp), dim3(256), 0, c.s, (const float *)a32, T, d, xp, at<f32x4>(ws, pl.off_rowc),
                     at<unsigned>(cprep, 0), c.N);
  CandidatePass cp{};
  cp.gemm = GEMM_I8_CERT; cp.skip_sample = true;
  cp.bias = at<float>(cprep, cq.off_bup);
  cp.colc = at<f32x4>(cprep, cq.off_colc); cp.colc_s = at<f32x4>(cprep, cq.off_colc_s); cp.colc_main = at<f32x4>(cprep, cq.off_colc_p);
  cp.zzx = CERT_ZZX;
  cp.z2 = 1.f; cp.i8 = 1;
  cp.zc2 = 1.f;                       // |p - c| <= band, always: the check can only trip on foreign operands
  GemmOperands &om = cp.op_main;
  om.A = reinterpret_cast<const unsigned char *>(xp); om.ldA = d; om.ldB = d;
  om.B = cprep + cq.off_w;
  om.cert = d / 128; om.nk = 3 * om.cert; om.packed = 1;
  cp.op_samp = om;
  cp.op_samp.B = cprep + cq.off_ws;
  return run_candidate_pipeline<DT>(c, ws, pl, co, cp, nullptr);
}

}  // namespace

#ifdef MSAE_GEMM_TIMELINE   // entry points of instrumented builds only (tools/gemm_timeline.py, tools/rescore_timeline.py): not in include/msae.h
extern "C" int msae_debug_timeline(unsigned long long *host_out) {
  if (!g_timeline) return MSAE_EINVAL;
  return (int)hipMemcpy(host_out, g_timeline, 64 * 8 * 8, hipMemcpyDeviceToHost);
}
#endif

#ifdef MSAE_RESCORE_TL
extern "C" int msae_debug_rescore_timeline(unsigned long long *host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_rs_tl), 64 * 16 * 8);
}
#endif

extern "C" void msae_options_init(msae_options *opts) {
  if (!opts) return;
  opts->size = (uint32_t)sizeof(msae_options);
  opts->coarse_mode = MSAE_COARSE_DEFAULT;
  opts->guard_z = 0.f;
  opts->status_detail = 0;
  opts->profile = nullptr;
  opts->exact = 0;
  opts->dither = MSAE_DITHER_DEFAULT;
  opts->rows_rescored = nullptr;
  opts->dither_seed = 0;
  opts->certified = 0;
  opts->reserved2 = 0;
  opts->certified_operands = nullptr;
}

extern "C" int msae_profile_create(int max_steps, void **handle) {
  if (max_steps <= 0 || max_steps > 4096 || !handle) return MSAE_EINVAL;
  ProfState *pf = new (std::nothrow) ProfState();       // (no exception may cross the C ABI)
  if (!pf) return (int)hipErrorOutOfMemory;
  pf->ev = new (std::nothrow) hipEvent_t[(size_t)max_steps * PROF_MARKS];
  if (!pf->ev) { delete pf; return (int)hipErrorOutOfMemory; }
  for (int i = 0; i < max_steps * PROF_MARKS; ++i) {
    const hipError_t e = hipEventCreate(&pf->ev[i]);
    if (e != hipSuccess) {
      for (int j = 0; j < i; ++j) (void)hipEventDestroy(pf->ev[j]);
      delete[] pf->ev;
      delete pf;
      return (int)e;
    }
  }
  pf->max_steps = max_steps;
  *handle = pf;
  return 0;
}

extern "C" int msae_profile_read(void *handle, float *stage_ms, int *n_steps) {
  ProfState *pf = static_cast<ProfState *>(handle);
  if (!pf || pf->magic != 0x50524F46u || !stage_ms) return MSAE_EINVAL;
  const int n = pf->step;
  if (n_steps) *n_steps = n;
  for (int st = 0; st < n; ++st) {
    MSAE_HIP_TRY(hipEventSynchronize(pf->ev[st * PROF_MARKS + PROF_MARKS - 1]));
    for (int i = 0; i + 1 < PROF_MARKS; ++i)
      MSAE_HIP_TRY(hipEventElapsedTime(&stage_ms[st * (PROF_MARKS - 1) + i], pf->ev[st * PROF_MARKS + i],
                                       pf->ev[st * PROF_MARKS + i + 1]));
  }
  pf->step = 0;
  return 0;
}

extern "C" int msae_profile_destroy(void *handle) {
  ProfState *pf = static_cast<ProfState *>(handle);
  if (!pf || pf->magic != 0x50524F46u) return MSAE_EINVAL;
  for (int i = 0; i < pf->max_steps * PROF_MARKS; ++i) (void)hipEventDestroy(pf->ev[i]);
  delete[] pf->ev;
  pf->magic = 0;
  delete pf;
  return 0;
}

extern "C" size_t msae_encoder_prepared_bytes(int N, int d) {
  if (N <= 0 || d <= 0) return 0;
  return make_prepared(N, d).bytes;
}


namespace {
// req: REQ_* bits (encode_defs.h)
int prepare_impl(const float *W_enc, int N, int d, void *prepared, int req, unsigned long long seed, hipStream_t s) {
  if (N <= 0 || d <= 0 || !prepared) return MSAE_EINVAL;
  if (!msae_aligned(prepared, 256)) return MSAE_EALIGN;
  Prepared p = make_prepared(N, d);
  const bool i8 = i8_shape_ok(N, d);
  const bool rebuild_i8 = (req & REQ_I8) && !(req & REQ_F8) && i8;
  // what this call rebuilds is valid, everything else is stale from now on (the weights have changed)
  p.valid = prep_valid_bits(req, N, d);
  p.dseed = rebuild_i8 ? seed : 0ull;   // the int8 operands' shared dither (encode_defs.h)
  MSAE_HIP_TRY(hipMemcpyAsync(prepared, &p, sizeof(p), hipMemcpyHostToDevice, s));
  if (p.S) {
    if (!msae_aligned(W_enc, 16)) return MSAE_EALIGN;
    unsigned char *base = static_cast<unsigned char *>(prepared);
    if (req & REQ_BF16)
      hipLaunchKernelGGL(prepare_weights_kernel, dim3(4096), dim3(256), 0, s, W_enc, N, d, at<unsigned short>(base, p.off_wb),
                         at<unsigned short>(base, p.off_ws));
    RowQuantOut ro = row_quant_out(base, p, req, i8);
    ro.seed = seed;
    if (p.dseed != 0ull)
      hipLaunchKernelGGL(sd_table_kernel, dim3(1), dim3(1024), 0, s, seed, d, at<int>(base, p.off_sdtab));
    if (rebuild_i8)   // row statistics (both passes' error bands) + int8 operands
      hipLaunchKernelGGL(row_stats_quant_kernel<true>, dim3(N), dim3(256), 0, s, W_enc, N, d, ro);
    else
      hipLaunchKernelGGL(row_stats_quant_kernel<false>, dim3(N), dim3(256), 0, s, W_enc, N, d, ro);
    if ((req & REQ_F8) && i8)                    // fp8 operands where the int8 ones would be (PREP_F8)
      hipLaunchKernelGGL(quant_w_fp8_kernel, dim3(N), dim3(256), 0, s, W_enc, N, d, at<f32x4>(base, p.off_colbf),
                         at<signed char>(base, p.off_wq), at<signed char>(base, p.off_wqsp));
  }
  return msae_launch_status();
}

// What the operands of `co`'s coarse mode ask of prepare_impl.  A prepare builds bf16 + int8 (either pass can run); fp8 operands
// take the int8 operands' place (bf16 + fp8, always).  A refresh rebuilds only what the mode in force reads; T_next > 0: for an
// encode of that many tokens -- more than 256 do not read the fragment-major copies.
int prepare_request(const CallOpts &co, int N, int d, bool refresh, int T_next) {
  if (co.mode == 2) return REQ_BF16 | REQ_F8;
  if (!refresh) return REQ_BF16 | REQ_I8;
  return ((co.mode == 1 && i8_shape_ok(N, d)) ? REQ_I8 : REQ_BF16) | (T_next > 256 ? REQ_NO_FRAG : 0);
}
}  // namespace

extern "C" int msae_encoder_prepare_opts(const float *W_enc, int N, int d, void *prepared, const msae_options *opts,
                                         void *stream) {
  CallOpts co;
  if (!resolve_opts(opts, co)) return MSAE_EINVAL;
  return prepare_impl(W_enc, N, d, prepared, prepare_request(co, N, d, false, 0), co.seed, (hipStream_t)stream);
}
extern "C" int msae_encoder_prepare(const float *W_enc, int N, int d, void *prepared, void *stream) {
  return msae_encoder_prepare_opts(W_enc, N, d, prepared, nullptr, stream);
}

// After a weight update (training): rebuild only the operands the coarse mode in force reads.
extern "C" int msae_encoder_refresh(const float *W_enc, int N, int d, void *prepared, const msae_options *opts,
                                    void *stream) {
  CallOpts co;
  if (!resolve_opts(opts, co)) return MSAE_EINVAL;
  return prepare_impl(W_enc, N, d, prepared, prepare_request(co, N, d, true, 0), co.seed, (hipStream_t)stream);
}

// ... for an encode of T_next tokens that follows: a batch of more than 256 tokens does not read the fragment-major copies (0.5 GB
// of scattered 16-byte stores per refresh at C2).  The buffer must be refreshed again before an encode of fewer tokens.
extern "C" int msae_encoder_refresh_for(const float *W_enc, int N, int d, void *prepared, int T_next, const msae_options *opts,
                                        void *stream) {
  CallOpts co;
  if (!resolve_opts(opts, co) || T_next <= 0) return MSAE_EINVAL;
  return prepare_impl(W_enc, N, d, prepared, prepare_request(co, N, d, true, T_next), co.seed, (hipStream_t)stream);
}

extern "C" size_t msae_encode_topk_ws_bytes(int T, int d, int N, int k, const msae_options *opts) {
  if (T <= 0 || d <= 0 || N <= 0 || k <= 0 || k > N || k > 4096) return 0;   // (what encode_topk_impl refuses)
  CallOpts co;
  if (!resolve_opts(opts, co)) return 0;
  const FusedPlan pl = make_plan(T, d, N, k, co.mode, 0, co.cert != 0);
  return pl.bytes;
}

extern "C" size_t msae_encoder_certified_bytes(int N, int d) {
  if (N <= 0 || d <= 0 || !cert_shape_ok(N, d)) return 0;
  return make_cert_prepared(N, d).bytes;
}

extern "C" int msae_encoder_prepare_certified(const float *W_enc, const float *b_enc, int N, int d, void *operands, void *stream) {
  if (N <= 0 || d <= 0 || !operands || !W_enc) return MSAE_EINVAL;
  if (!cert_shape_ok(N, d)) return MSAE_ENOTIMPL;
  if (!msae_aligned(operands, 256) || !msae_aligned(W_enc, 16)) return MSAE_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const CertPrepared cp = make_cert_prepared(N, d);
  MSAE_HIP_TRY(hipMemcpyAsync(operands, &cp, sizeof(cp), hipMemcpyHostToDevice, s));
  unsigned char *base = static_cast<unsigned char *>(operands);
  hipLaunchKernelGGL(cert_prepare_rows_kernel, dim3(N), dim3(256), 0, s, W_enc, b_enc, N, d, at<float>(base, cp.off_bup),
                     at<f32x4>(base, cp.off_colc), at<f32x4>(base, cp.off_colc_p), at<f32x4>(base, cp.off_colc_s),
                     at<signed char>(base, cp.off_w), at<signed char>(base, cp.off_ws));
  return msae_launch_status();
}

static bool x_dtype_ok(int x_dtype) { return x_dtype == MSAE_F32 || x_dtype == MSAE_BF16 || x_dtype == MSAE_F16; }
// alignment the kernels ask of the call's inputs (W_enc null: a shard, which does not read it)
static bool inputs_aligned(const EncodeCall &c) {
  return msae_aligned(c.x, c.x_dtype == MSAE_F32 ? 16 : 8) && msae_aligned(c.W_enc, 16) && (!c.b_dec || msae_aligned(c.b_dec, 16));
}

static int encode_topk_impl(const EncodeCall &c, const void *prepared, void *ws, size_t ws_bytes, const msae_options *opts) {
  const int T = c.T, d = c.d, N = c.N, k = c.k;
  hipStream_t s = c.s;
  CallOpts co;
  if (!resolve_opts(opts, co)) return MSAE_EINVAL;
  if (T < 0 || d <= 0 || N <= 0 || k <= 0 || k > N || k > 4096) return MSAE_EINVAL;
  if (!x_dtype_ok(c.x_dtype)) return MSAE_EINVAL;
  if (c.set_feature >= N || c.zero_feature >= N) return MSAE_EINVAL;
  if (T == 0) return 0;
  const FusedPlan pl = make_plan(T, d, N, k, co.mode, 0, co.cert != 0);
  if (co.cert) {
    if (pl.fast && !co.cert_ops) return MSAE_EINVAL;   // msae_options::certified needs msae_encoder_prepare_certified()'s buffer
  } else if (!prepared && pl.fast) return MSAE_EINVAL;  // the fast path needs msae_encoder_prepare()
  if (ws_bytes < pl.bytes || !ws) return MSAE_EWS;
  if (!msae_aligned(ws, 256)) return MSAE_EALIGN;
  unsigned char *wsb = static_cast<unsigned char *>(ws);
  if (!pl.fast) {
    float *dense = at<float>(wsb, pl.off_dense);
    int rc = msae_pre_acts_launch(c.x, c.x_dtype, c.W_enc, c.b_enc, c.b_dec, nullptr, nullptr, T, d, N, 1, dense, N, s);
    if (rc) return rc;
    if (c.set_feature >= 0 || c.zero_feature >= 0)
      hipLaunchKernelGGL(edit_dense_kernel, dim3((T + 255) / 256), dim3(256), 0, s, dense, N, T,
                         (const int *)nullptr, c.set_feature, c.set_value, c.zero_feature);
    TopkExtra ex;
    ex.idx64 = c.idx.i64;
    rc = msae_topk_launch(dense, T, N, k, N, nullptr, c.vals, c.idx.i32, s, ex);
    if (rc) return rc;
    if (c.status) hipLaunchKernelGGL(zero_i32_kernel, dim3(64), dim3(256), 0, s, c.status, (size_t)T);
    return msae_launch_status();
  }
  if (!inputs_aligned(c)) return MSAE_EALIGN;
  if (co.rows_out && (co.exact || (pl.small && !co.cert)))   // paths without the large-batch re-score kernel report 0 rows
    hipLaunchKernelGGL(zero_i32_kernel, dim3(8), dim3(256), 0, s, co.rows_out, (size_t)T);
  if (co.exact) {   // msae_options::exact: every token through the in-call exact path (bounded scratch, status 1)
    const int n_list = (int)pl.fb.flag_words(T);
    hipLaunchKernelGGL(iota_list_kernel, dim3((n_list + 255) / 256), dim3(256), 0, s, pl.fb.flagged(wsb), T, n_list);
    const int rc = run_exact_fallback(c, wsb, pl.fb, 0);
    return rc ? rc : msae_launch_status();
  }
  if (co.cert) {
    const unsigned char *cb = static_cast<const unsigned char *>(co.cert_ops);
    if (!msae_aligned(cb, 256)) return MSAE_EALIGN;
    return with_x_dtype(c.x_dtype, [&](auto dt) { return run_cert<decltype(dt)::value>(c, cb, wsb, pl, co); });
  }
  const Prepared pp = make_prepared(N, d);  // layout is a pure function of (N, d)
  const FusedCtx fx{pp, static_cast<const unsigned char *>(prepared), wsb, pl, co};
  return with_x_dtype(c.x_dtype, [&](auto dt) { return pl.small ? run_small<decltype(dt)::value>(c, fx) : run_fast<decltype(dt)::value>(c, fx); });
}

extern "C" int msae_encode_topk(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                const float *b_dec, const void *prepared, int T, int d, int N, int k,
                                int set_feature, float set_value, int zero_feature, float *vals,
                                int32_t *idx, int32_t *status, void *ws, size_t ws_bytes,
                                const msae_options *opts, void *stream) {
  if (!idx) return MSAE_EINVAL;
  const EncodeCall c{x, x_dtype, W_enc, b_enc, b_dec, T, d, N, k, set_feature, set_value, zero_feature, vals,
                     IdxOut{idx, nullptr}, status, (hipStream_t)stream};
  return encode_topk_impl(c, prepared, ws, ws_bytes, opts);
}

extern "C" int msae_encode_topk_i64(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                    const float *b_dec, const void *prepared, int T, int d, int N, int k,
                                    int set_feature, float set_value, int zero_feature, float *vals,
                                    int64_t *idx, int32_t *status, void *ws, size_t ws_bytes,
                                    const msae_options *opts, void *stream) {
  if (!idx) return MSAE_EINVAL;
  const EncodeCall c{x, x_dtype, W_enc, b_enc, b_dec, T, d, N, k, set_feature, set_value, zero_feature, vals,
                     IdxOut{nullptr, idx}, status, (hipStream_t)stream};
  return encode_topk_impl(c, prepared, ws, ws_bytes, opts);
}

// ---- exact encode of a device-side token list (second round of the feature-sharded engine's per-shard top-k scheme) ----
namespace {
// the fallback's plan without a token list of its own: the caller's `rows` are the list, the counts sit at word 64
struct RowsPlan { FallbackPlan fb; size_t bytes; };
inline RowsPlan make_plan_rows(int max_rows, int N) {
  RowsPlan p{};
  size_t o = 0;
  auto take = [&](size_t b) { size_t at = o; o += msae_align_up(b, 256); return at; };
  p.fb = make_fallback_plan(max_rows, N, 0, take);
  p.bytes = o;
  return p;
}
}  // namespace

extern "C" size_t msae_encode_topk_rows_ws_bytes(int max_rows, int N) {
  if (max_rows <= 0 || N <= 0) return 0;
  return make_plan_rows(max_rows, N).bytes;
}

extern "C" int msae_encode_topk_rows(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                     const float *b_dec, const int32_t *rows, const int32_t *n_rows, int max_rows,
                                     int d, int N, int k, int set_feature, float set_value, int zero_feature,
                                     float *vals, int64_t *idx, int32_t *status, void *ws, size_t ws_bytes,
                                     void *stream) {
  if (max_rows < 0 || d <= 0 || N <= 0 || k <= 0 || k > N || k > 16384 || !rows || !n_rows || !vals || !idx) return MSAE_EINVAL;
  if (!x_dtype_ok(x_dtype)) return MSAE_EINVAL;
  if (set_feature >= N || zero_feature >= N) return MSAE_EINVAL;
  if (max_rows == 0) return 0;
  const EncodeCall c{x, x_dtype, W_enc, b_enc, b_dec, max_rows, d, N, k, set_feature, set_value, zero_feature, vals,
                     IdxOut{nullptr, idx}, status, (hipStream_t)stream};
  const RowsPlan rp = make_plan_rows(max_rows, N);
  if (ws_bytes < rp.bytes || !ws) return MSAE_EWS;
  if (!msae_aligned(ws, 256) || !inputs_aligned(c)) return MSAE_EALIGN;
  unsigned char *wsb = static_cast<unsigned char *>(ws);
  const int rc = run_exact_rows(c, rows, n_rows, rp.fb.pass_counts(wsb, 0), rp.fb.dense(wsb), rp.fb, 0);
  return rc ? rc : msae_launch_status();
}

// ---- feature-sharded group: per-shard candidates, owner-side exact re-score ----------------------------
namespace {
struct ExtPlan { size_t off_a32, bytes; FallbackPlan fb; int cap, r_max; };
inline ExtPlan make_plan_ext(int T, int d, int N, int k, int M) {
  ExtPlan p{};
  size_t o = 0;
  auto take = [&](size_t b) { size_t at = o; o += msae_align_up(b, 256); return at; };
  p.cap = next_pow2(M > 2 ? M : 2);
  p.r_max = rescore_row_budget(k, p.cap);
  p.off_a32 = take((size_t)T * d * 4);
  p.fb = make_fallback_plan(T, N, T, take);
  p.bytes = o;
  return p;
}

// the records of G shards, C per token: c.T token rows of them, the first T_valid hold tokens
struct ShardRecords { const unsigned char *recs; int G, C, T_valid; };

template <int DT>
int run_rescore_ext(const EncodeCall &c, const ShardRecords &sr, unsigned char *ws, const ExtPlan &xp, const CallOpts &co) {
  const int T = c.T, T_valid = sr.T_valid;
  float *a32 = at<float>(ws, xp.off_a32);
  int *flagged = xp.fb.flagged(ws);
  const float z = co.z;
  hipLaunchKernelGGL(zero_i32_kernel, dim3(8), dim3(256), 0, c.s, flagged, xp.fb.flag_words(T));
  hipLaunchKernelGGL(prep_x_kernel<DT>, dim3(2048), dim3(256), 0, c.s, c.x, c.b_dec, T_valid, T_valid, c.d,
                     (unsigned short *)nullptr, a32);
  RescoreArgs ra{};
  ra.b_enc = c.b_enc;
  ra.cap = xp.cap;
  ra.T = T_valid; ra.d = c.d; ra.k = c.k; ra.r_max = xp.r_max;
  ra.zz12 = z * z / 12.f; ra.z2 = z * z; ra.i8 = 0;
  // (the records' z sigma came from shards running with the same options; large batches subtract the dither there -- actual
  // sigma --, small ones carry Hoeffding's proxy: 6 of either is the net under operands edited behind the API)
  ra.zc2 = guard_z_check2(false);
  ra.set_feature = c.set_feature; ra.set_value = c.set_value;
  ra.vals = c.vals; ra.idx = nullptr; ra.idx64 = c.idx.i64; ra.status = c.status;
  ra.flagged = flagged; ra.n_flagged = xp.fb.n_flagged(ws, T);
  ra.fb_cap = T;
  ra.ext = RescoreExt{sr.recs, sr.G, sr.C, T, shard_record_bytes(sr.C), T_valid};
  const int lrc = launch_select_rescore<true>(ra, a32, c.W_enc, c.s);
  if (lrc) return lrc;
  const int rc = run_exact_fallback(c, ws, xp.fb, co.detail);
  return rc ? rc : msae_launch_status();
}
}  // namespace

extern "C" size_t msae_shard_record_bytes(int C) { return C > 0 ? (size_t)shard_record_bytes(C) : 0; }

extern "C" int msae_shard_candidates(const void *x, int x_dtype, const float *b_enc, const float *b_dec,
                                     const void *prepared, int T, int d, int N, int k, int row_offset, int C,
                                     int set_feature, int zero_feature, void *records, void *ws, size_t ws_bytes,
                                     const msae_options *opts, void *stream) {
  CallOpts co;
  if (!resolve_opts(opts, co)) return MSAE_EINVAL;
  if (T < 0 || d <= 0 || N <= 0 || k <= 0 || C <= 0 || row_offset < 0 || !records) return MSAE_EINVAL;
  if (!x_dtype_ok(x_dtype)) return MSAE_EINVAL;
  if (T == 0) return 0;
  FusedPlan pl = make_plan(T, d, N, k, co.mode, C);
  if (!pl.fast || !prepared || C > pl.cap || pl.f8) return MSAE_ENOTIMPL;   // shapes / modes without the candidate exchange: msae_encode_topk per shard
  pl.small = false;
  // the hooks' features are global ids: only the owning shard leaves them out of its candidates
  const int sf = (set_feature >= row_offset && set_feature < row_offset + N) ? set_feature - row_offset : -1;
  const int zf = (zero_feature >= row_offset && zero_feature < row_offset + N) ? zero_feature - row_offset : -1;
  const EncodeCall c{x, x_dtype, nullptr, b_enc, b_dec, T, d, N, k, sf, 0.f, zf, nullptr, IdxOut{nullptr, nullptr}, nullptr,
                     (hipStream_t)stream};
  // the contract is msae_encode_topk_ws_bytes (include/msae.h): the shard's own plan never exceeds it -- C only lowers r, cap and
  // the segment count, and there is no feature-major re-score -- and a caller that brings less than the contract is told so
  const size_t contract = make_plan(T, d, N, k, co.mode).bytes;
  if (ws_bytes < (contract > pl.bytes ? contract : pl.bytes) || !ws) return MSAE_EWS;
  if (!msae_aligned(ws, 256) || !msae_aligned(records, 8)) return MSAE_EALIGN;
  if (!inputs_aligned(c)) return MSAE_EALIGN;
  const Prepared pp = make_prepared(N, d);
  const FusedCtx fx{pp, static_cast<const unsigned char *>(prepared), static_cast<unsigned char *>(ws), pl, co};
  const ShardOut so{static_cast<unsigned char *>(records), C, row_offset};
  return with_x_dtype(x_dtype, [&](auto dt) { return run_fast<decltype(dt)::value>(c, fx, &so); });
}

extern "C" size_t msae_rescore_candidates_ws_bytes(int T, int d, int N, int k, int G, int C) {
  if (T <= 0 || d <= 0 || N <= 0 || k <= 0 || G <= 0 || C <= 0) return 0;
  if (k > N || k > 256 || (long)G * C < k || (long)G * C > 8192 || d % 64 != 0) return 0;   // (what msae_rescore_candidates refuses)
  return make_plan_ext(T, d, N, k, G * C).bytes;
}

extern "C" int msae_rescore_candidates(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                                       const float *b_dec, int T, int T_valid, int d, int N, int k, int G, int C,
                                       const void *records, int set_feature, float set_value, int zero_feature,
                                       float *vals, int64_t *idx, int32_t *status, void *ws, size_t ws_bytes,
                                       const msae_options *opts, void *stream) {
  CallOpts co;
  if (!resolve_opts(opts, co)) return MSAE_EINVAL;
  if (T < 0 || T_valid < 0 || T_valid > T || d <= 0 || N <= 0 || k <= 0 || k > N || k > 256 || G <= 0 || C <= 0 ||
      (long)G * C < k || (long)G * C > 8192 || d % 64 != 0)
    return MSAE_EINVAL;
  if (!x_dtype_ok(x_dtype)) return MSAE_EINVAL;
  if (set_feature >= N || zero_feature >= N || !records || !vals || !idx) return MSAE_EINVAL;
  if (T_valid == 0) return 0;
  const EncodeCall c{x, x_dtype, W_enc, b_enc, b_dec, T, d, N, k, set_feature, set_value, zero_feature, vals,
                     IdxOut{nullptr, idx}, status, (hipStream_t)stream};
  const ExtPlan xp = make_plan_ext(T, d, N, k, G * C);
  if (ws_bytes < xp.bytes || !ws) return MSAE_EWS;
  if (!msae_aligned(ws, 256) || !msae_aligned(records, 8) || !inputs_aligned(c)) return MSAE_EALIGN;
  const ShardRecords sr{static_cast<const unsigned char *>(records), G, C, T_valid};
  unsigned char *wsb = static_cast<unsigned char *>(ws);
  return with_x_dtype(x_dtype, [&](auto dt) { return run_rescore_ext<decltype(dt)::value>(c, sr, wsb, xp, co); });
}
