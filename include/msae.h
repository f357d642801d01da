/*
 * msae.h -- C ABI of libmsae_hip.so: the MI355X (gfx950) native SAE encode / TopK / decode /
 * cache-sparsify path.  Plain pointers and sizes only; no torch types.
 *
 * Every pointer is a DEVICE pointer unless stated otherwise.  Every call is asynchronous on
 * `stream` (a hipStream_t passed as void*; NULL = the default stream), never synchronises the
 * device, and allocates nothing: workspaces are sized by the *_ws_bytes() helpers and owned by the
 * caller (the reference calls this path inside an HF forward hook on the model's stream,
 * features/cache.py:187-204, so ops must be stream-ordered).
 *
 * WORKSPACE CONTRACT (every entry that takes `void *ws, size_t ws_bytes`; tests/test_gpu_workspace_contract.py holds each of
 * them to it with exact-size, guarded and dirty buffers; tests/test_gpu_pos_profile.py does so for msae_pos_profile_update,
 * whose helper asks for no bytes, tests/test_gpu_batch_select.py for msae_batch_kth_f32):
 *   - the contents of [ws, ws + ws_bytes) are UNSPECIFIED on entry and on return: a caller may hand over a fresh block, the
 *     block a different entry has just used, or one it shares between all entries of a stream; nothing is kept in it
 *     between calls;
 *   - no entry reads a byte of the workspace that the same call has not written before;
 *   - no entry reads or writes outside [ws, ws + ws_bytes), and ws_bytes equal to what the entry's *_ws_bytes() helper
 *     returns for the same shape (and options) always suffices;
 *   - a workspace the entry needs and that is missing (NULL) or smaller than that is refused with MSAE_EWS before anything
 *     is launched or written: outputs and workspace are untouched;
 *   - a *_ws_bytes() helper returns 0 for every shape its entry refuses with MSAE_EINVAL because of the sizes the helper
 *     sees (zero or negative sizes, k or N beyond the entry's envelope).
 *
 * Return value: 0 on success, a positive hipError_t from the HIP runtime, or a negative
 * MSAE_E* code for argument errors (the reference raises Python AssertionError on the same
 * conditions: sae/kernels.py:28-36,194-197,303-309; the Python host layer turns any non-zero
 * code into RuntimeError).  msae_error_string() describes a code.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference):
 *   msae_pre_acts_f32        Sae.pre_acts                  sae_auto_interp/sae/sae.py:172-177
 *   msae_topk_f32            Sae.select_topk / torch.topk  sae_auto_interp/sae/sae.py:179-181,
 *                                                          features/cache.py:210-212
 *   msae_encode_topk         Sae.encode (fused)            sae_auto_interp/sae/sae.py:183-185
 *                            + hook edits                  features/steering.py:113-114,
 *                                                          features/patching/utils.py:43-48
 *   msae_decode_f32          Sae.decode / decoder_impl     sae_auto_interp/sae/sae.py:187-191,
 *                            TritonDecoder.forward         sae/utils.py:115-129, sae/kernels.py:178-284
 *   msae_decode_bwd_acts_f32 TritonDecoder.backward (acts) sae/kernels.py:421-425,287-400
 *   msae_decode_bwd_wdec_f32 TritonDecoder.backward (W)    sae/kernels.py:417-419,10-175
 *   msae_sparsify_*          scatter_ + Cache.add/get_nonzeros  features/cache.py:214-217,42-92
 *   msae_feature_stats_*     per-feature counts + top examples  features/loader.py:103-106, constructors.py:28-141
 *   msae_coact_*             co-activation counters + neighbours (no reference counterpart)
 *   msae_act_hist_*          per-feature activation histograms + quantiles (no reference counterpart)
 *   msae_pos_profile_*       per-feature position profiles + peak bins (no reference counterpart)
 *   msae_token_profile_*     which tokens a feature fires on: unigram  features/stats.py:50-73
 *   msae_rows_topk_f32       cos + get_neighbors; logits   features/stats.py:76-120; stats.py:12-47
 *   msae_row_inv_norms_f32   F.normalize's norms in cos    features/stats.py:80-81
 *   msae_edit_topk_f32       hook edits with a feature LIST features/steering.py:113-114, patching/utils.py:43-48
 *   msae_edit_topk_rows_f32  the same with one table per token (a feature per batch row of one generate)
 *   msae_delta_decode_f32    x + decode(edited) - decode(plain): error-preserving hooks (no reference counterpart)
 *   msae_recon_curve_f32     reconstruction error at several sparsities in one pass (sae.py:190-202 per checkpoint)
 *   msae_support_refit_f32   least-squares refit on the encoder's support: optimal error at every sparsity (no reference
 *                            counterpart)
 *   msae_batch_kth_f32, msae_list_filter_f32, msae_decode_prefix_f32   BatchTopK on top-C lists: the batch threshold, the
 *                            threshold filter, the decode with a row length (no reference counterpart)
 *   msae_jump_filter_f32, msae_jump_bwd_f32   JumpReLU with learned per-feature thresholds on top-C lists: the three-way
 *                            partition and its straight-through backward (no reference counterpart)
 *   msae_nested_decode_f32, msae_nested_combine_f32, msae_decode_bwd_*_grouped_f32   Matryoshka prefixes: every prefix's
 *                            reconstruction error in one decode pass, and its backward (no reference counterpart)
 *
 * Numerics contract: all dot products are ascending-k f32 fused
 * multiply-add chains (v_mfma_f32_32x32x2_f32 / v_fma_f32), bit-identical to oracle/sae_oracle.c.
 * msae_encode_topk selects candidates with an int8 (or bf16) MFMA pass and re-scores them with the exact f32
 * chain, so its outputs are bit-identical to msae_pre_acts_f32 + msae_topk_f32 for every token it
 * VERIFIES: all features whose coarse value plus the error band of the pair (token, feature) reaches the exact
 * k-th value were re-scored.  Tokens it cannot verify are reported in `status` and recomputed by the exact path
 * inside the same call.  WHAT THE BAND GUARANTEES depends on the mode (msae_options):
 *   default    int8 operands rounded STOCHASTICALLY with seeds drawn by the library (`dither`): for EVERY input a
 *              member of the true top-k is missed with probability <= k exp(-z^2 / 2) over the library's own randomness
 *              (a Chernoff bound of a sum of independent bounded residuals; 7e-10 per token at z = 7, k = 32; guard_z = 8:
 *              4e-13).  No assumption about the data.  The probability is over the seed of the PREPARE / refresh for the
 *              weights' residuals and, for every batch that runs an MFMA candidate pass (more than 16 tokens), for the
 *              activations' as well (the subtractive dither below: both operands are rounded against per-dim vectors fixed
 *              when the operands are prepared); the weight-stream path of <= 16 tokens rounds the activations with a seed
 *              drawn per call.  A long-running job that wants fresh randomness
 *              re-prepares (msae_encoder_refresh: one sweep over W_enc).
 *   certified  two int8 planes per operand, three MFMA segments, a DETERMINISTIC Cauchy-Schwarz band: no probability
 *              left; ~2.5x the default's step time on large batches (`certified`).
 *   exact      every token through the f32 MFMA path (`exact`); ~20x.
 *   dither off / bf16 pass: the statistical contract of ABI <= 3 (z = 7 of the rounding-noise MODEL, < 3e-13 per token under
 *              it; the model is checked on every re-scored pair) -- kept for A/B runs and for callers pinned to ABI 3.
 * Non-finite activations (+-inf / NaN, e.g. an overflowed bf16 residual stream): in every mode a token that holds one is
 * recomputed by the exact path inside the call (status 1) -- its outputs are msae_pre_acts_f32 + msae_topk_f32's -- and the
 * other tokens of the batch are unaffected (tests/test_gpu_hostile.py::test_non_finite_activations_stay_with_their_token).
 */
#ifndef MSAE_H_
#define MSAE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSAE_ABI_VERSION 4

/* element type of the activation tensor x handed over by the LLM hook (sae.py:174 up-casts) */
enum { MSAE_F32 = 0, MSAE_BF16 = 1, MSAE_F16 = 2 };

/* argument errors */
enum {
  MSAE_EINVAL = -1,   /* bad shape / k / dtype code */
  MSAE_EALIGN = -2,   /* pointer or leading dimension not aligned as required */
  MSAE_EWS = -3,      /* workspace too small */
  MSAE_ENOTIMPL = -4  /* shape outside what this build supports */
};

/* ---- per-call options of the fused encoder ---------------------------------------------------------
 * The library keeps NO mutable process state: what used to be msae_set_coarse_mode / msae_set_guard_z /
 * msae_set_status_detail / msae_profile_begin (ABI 1) travels with the call.  Zero-initialise, set `size`,
 * fill what you need; NULL wherever a `const msae_options *` is taken means "all defaults".  Calls with
 * different options may run concurrently from different threads / streams.
 *   coarse_mode   operand type of the candidate pass: MSAE_COARSE_INT8 (per-token / per-feature scales, massive-
 *                 activation dims in a separately scaled k-tile), MSAE_COARSE_BF16, MSAE_COARSE_FP8 (ABI 4; OCP e4m3
 *                 operands with per-token / per-feature scales through v_mfma_f32_32x32x16_fp8_fp8, f32 accumulate --
 *                 the "fp8 MFMA encoder path" of BASELINE configs[4]; batches of any size run the 256-row tile kernel;
 *                 its prepared operands take the int8 operands' place in the buffer, so msae_encoder_prepare_opts /
 *                 _refresh with the SAME mode must precede the encode -- an encode in a mode whose operands the buffer
 *                 does not hold computes every token by the exact path; statistical contract like the bf16 pass, and
 *                 ~2x the rows to re-score: slower than int8) or MSAE_COARSE_DEFAULT
 *                 (environment MSAE_COARSE=bf16|int8|fp8, else int8).  Either way the candidates are re-scored with
 *                 the exact f32 chain, so outputs do not depend on it; the workspace size does (pass the same
 *                 options to the *_ws_bytes helper).
 *   guard_z       width z of the candidate pass's error band in standard deviations of its per-(token, feature)
 *                 rounding noise; 0 = default (environment MSAE_GUARD_Z, else 7); 0.25 <= z <= 64.  A larger z
 *                 re-scores more rows per token; results of verified tokens do not depend on it.
 *   status_detail diagnostics (tools/soak_fused.py): a token recomputed inside the call reports
 *                 status = 1 | reason << 8 (reason bits below) instead of 1, so `status & 0xFF` is the code.
 *   profile       a handle from msae_profile_create (stage timing, below) or NULL.
 *   rows_rescored (ABI 3) optional DEVICE int32[T]: per token, rounds (6 bits) << 24 | first-round rows << 12 | rows of W_enc
 *                 the exact re-score read for it (0 for tokens the large-batch re-score did not verify / paths without it) --
 *                 the measurement behind bench.py's rows_rescored_per_token; costs one store per token.  Bit 30: the first
 *                 round ran FEATURE-major (batches in which a feature is a candidate of >= ~4 tokens, e.g. k = 256 at 8192
 *                 tokens: the pairs are counting-sorted by feature, every row of W_enc comes from HBM once and the
 *                 activation rows out of the Infinity Cache -- same chains, same bits).
 *   exact         (ABI 3) != 0: msae_encode_topk[_i64] computes EVERY token by the exact path (msae_pre_acts_f32 +
 *                 msae_topk_f32 semantics through the in-call fallback: <= 1 GiB of dense scratch whatever T; status 1
 *                 for every token).  The switch for callers that cannot accept the fused path's statistical contract:
 *                 "bit-identical for every verified token, a member of the true top-k missed with probability < 3e-13
 *                 per token UNDER THE NOISE MODEL" -- the model assumes the rounding residuals of one operand are not
 *                 aligned with the other operand.  Encoder rows constructed from a token's own int8 rounding residual
 *                 (W_n ~ sign(x/sx - rint(x/sx))) violate it by construction: such a row's coarse value is low by
 *                 ~0.25 sqrt(12 d) = 55 sigma at d = 4096, it is never re-scored, no check sees it, and the int8 pass
 *                 returns status 0 with that feature missing (tests/test_gpu_hostile.py::test_row_aligned_with_a_
 *                 token_s_rounding_residual pins exactly this; the bf16 pass, whose residuals are relative roundings of
 *                 other bits, and exact = 1 return the right answer).  Trained weights cannot know a future token's
 *                 residual; weights under an adversary's control can.  Slower by ~20x on large batches.
 *                 (That paragraph describes dither = MSAE_DITHER_OFF, the behaviour of ABI <= 3.  With the dither -- the
 *                 default since ABI 4 -- the same row is found: see `dither`.)
 *   dither        (ABI 4; the word ABI 3 called `reserved`) MSAE_DITHER_DEFAULT (0: environment MSAE_DITHER=0|1, else ON),
 *                 MSAE_DITHER_ON, MSAE_DITHER_OFF.  ON: the int8 operands are rounded STOCHASTICALLY -- q = floor(v / step + r),
 *                 r uniform in [0, 1) from a counter hash of (seed, token or row, dim) -- instead of to nearest: the
 *                 activations with a fresh seed in every encode call, the weights with a fresh seed in every prepare /
 *                 refresh.  The rounding residuals are then the LIBRARY's randomness, not a property of the data: for EVERY
 *                 input (chosen without knowledge of the seeds) the error of a coarse value is a sum of independent,
 *                 zero-mean terms bounded by one step each, so by Hoeffding's inequality it exceeds z sigma' with
 *                 probability <= exp(-z^2 / 2), sigma'^2 = sw_n^2 |a_t|^2 / 4 + sx_t^2 (|W_n[in]|^2 + m_t^2 |W_n[out]|^2) / 4
 *                 (the variance PROXY of a bounded term, 3x the variance of round-to-nearest on fine data; the band the
 *                 kernels use).  A member of the true top-k is therefore missed with probability <= k exp(-z^2 / 2) per token
 *                 -- 7.3e-10 at z = 7, k = 32; 4e-13 at guard_z = 8 -- whatever the weights and activations are, including
 *                 rows built from a token's round-to-nearest residual (the pinned test now asserts the RIGHT answer).
 *                 Outputs of verified tokens do not depend on the seeds (they are the exact path's bits); which tokens fall
 *                 back may.  Costs ~sqrt(3) of band width: measured rows re-scored per token and step time in DESIGN.md
 *                 section 5.  Applies to the int8 pass (all batch sizes); the bf16 pass keeps its statistical model.
 *                 The proxy includes the cross term of the two roundings: the weights' residuals multiply the DEQUANTISED
 *                 activation, so |a_t| above reads |a_t| + sx_t sqrt(d) (ABI 4 builds before round 6 left it out).
 *                 SUBTRACTIVE DITHER (round 6; batches of more than 16 tokens: the MFMA candidate passes of csrc/gemm_mfma.h and
 *                 csrc/gemm_skinny.h; the <= 16-token weight stream keeps the band above).  The
 *                 sqrt(3) is the price of a residual whose variance f (1 - f) depends on the input.  When the dither is
 *                 subtracted again -- the operand element is taken as q - (r - 1/2) -- the residual is EXACTLY uniform on
 *                 (-1/2, 1/2] step for every input, and a uniform variable is sub-Gaussian with its own variance 1/12 as proxy:
 *                 the same bound k exp(-z^2 / 2) holds with sigma^2 = sw_n^2 (|a_t| + sx_t sqrt(d) / 2)^2 / 12 + sx_t^2 |W_n|^2 / 12,
 *                 the round-to-nearest band, now a theorem.  Subtracting is affordable because the dither is SHARED: one
 *                 vector r_x(c) for all tokens, one r_w(c) for all features (independence is needed across the dims of ONE
 *                 pair only), both derived from the seed of the prepare / refresh.  The corrections are a per-feature constant
 *                 D_n = sum_c (r_x(c) - 1/2) Wq[n][c] stored with the operands and a per-token integer E_t out of the
 *                 activation quantiser; the MFMA pass applies both at no cost (E in the multiply-add that scales the outlier
 *                 tile, D inside the epilogue's fma nesting).  Massive-activation dims keep an exact integer quotient in the
 *                 outlier tile and their remainder in their own column, so they carry the same one-step residual as every
 *                 other dim.  Measured: 45 rows re-scored per token instead of 58, re-score 0.88 -> 0.75 ms (DESIGN.md
 *                 section 5); tests/test_gpu_band.py checks the coarse value, the band and the residuals' variance pair by
 *                 pair against a numpy restatement.  A buffer prepared with dither OFF and encoded with dither ON has no
 *                 D_n: such a call computes its tokens by the exact path (status 1) -- prepare and encode with the same mode.
 *                 Environment MSAE_NO_SUBTRACT=1 keeps the non-subtractive band (A/B runs).
 *   certified     (ABI 4) != 0: msae_encode_topk[_i64] runs the CERTIFIED candidate pass: both operands as two int8 planes
 *                 (15 bits; x_lo.W_hi + x_hi.W_lo, a rounded shift by 7, then x_hi.W_hi in one int32 accumulator -- three
 *                 times the MFMA work of the default pass) and a DETERMINISTIC error band: Cauchy-Schwarz bounds of every
 *                 dropped term (the planes' rounding residuals, the lo.lo product, the shift's rounding, the f32 chain's own
 *                 gamma_d, the f32 evaluation of the bound), evaluated per (token, feature) from exact norms
 *                 (csrc/encode_cert.h derives it).  No probability and no assumption about the data is left: for EVERY input a
 *                 token reported status 0 carries exactly the exact path's top-k.  ~3x the default's step time on the bench
 *                 batch, ~9x faster than `exact`.  Needs `certified_operands` = the buffer of
 *                 msae_encoder_prepare_certified (2 d bytes per feature); `prepared` may be NULL.  Massive-activation dims have
 *                 no separate tile here: a token whose largest dim dwarfs the rest by > ~100x gets a wide band and ends in the
 *                 in-call exact path (time, never a wrong answer).  Shapes without the pass (d % 128, N % 8192) run the exact path.
 *   dither_seed   (ABI 4) 0: the library draws a seed per call (process-random base + atomic counter through a 64-bit
 *                 mixer -- the one piece of process state the library keeps); != 0: the seed of THIS call (reproducible
 *                 candidate sets: tests, A/B runs).  In a prepare / refresh it seeds the weights' rounding and the shared
 *                 dither vectors of the MFMA candidate passes; in an encode, the activations' rounding of the <= 16-token path
 *                 (and of every batch under MSAE_NO_SUBTRACT=1). */
enum { MSAE_COARSE_DEFAULT = -1, MSAE_COARSE_BF16 = 0, MSAE_COARSE_INT8 = 1, MSAE_COARSE_FP8 = 2 };
enum { MSAE_DITHER_DEFAULT = 0, MSAE_DITHER_ON = 1, MSAE_DITHER_OFF = 2 };
typedef struct msae_options {
  uint32_t size;          /* sizeof(msae_options) of the caller's header (ABI 2's 24-byte and ABI 3's 40-byte structs are
                             accepted: exact = 0 / dither_seed = 0) */
  int32_t coarse_mode;    /* MSAE_COARSE_* */
  float guard_z;          /* 0 = default */
  int32_t status_detail;  /* 0 / 1 */
  void *profile;          /* msae_profile_create handle or NULL */
  int32_t exact;          /* 0 / 1 */
  int32_t dither;         /* MSAE_DITHER_* (ABI 3: reserved, 0) */
  int32_t *rows_rescored; /* device int32[T] or NULL */
  uint64_t dither_seed;   /* 0 = drawn by the library */
  int32_t certified;      /* 0 / 1 (ABI 4) */
  int32_t reserved2;      /* 0 */
  const void *certified_operands;   /* device buffer of msae_encoder_prepare_certified, or NULL */
} msae_options;
/* Fills *opts with the defaults (coarse_mode MSAE_COARSE_DEFAULT, guard_z 0, no detail, no profile). */
void msae_options_init(msae_options *opts);

int msae_abi_version(void);
const char *msae_error_string(int code);
/* Name of the device architecture the kernels were compiled for ("gfx950"). */
const char *msae_target_arch(void);

/* ---- exact f32 path ------------------------------------------------------------------ */

/* out[T][N] = relu((x[T][d] - b_dec[d]) @ W_enc[N][d]^T + b_enc[N]), f32, row-major, dense.
 * x is row-major with element type x_dtype.  b_enc / b_dec may be NULL (treated as zeros).
 * relu != 0 applies the ReLU (Sae.pre_acts always does). */
int msae_pre_acts_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                      const float *b_dec, int T, int d, int N, int relu, float *out, void *stream);

/* The accumulating NT GEMM of a skip transcoder: C[m][p] (+)= sum_j a[m][j] B[p][j].
 * a is [M][K] row-major with element type a_dtype (MSAE_F32 / MSAE_BF16 / MSAE_F16, up-cast exactly), B is f32 [P][K], C is
 * f32 with row stride ld_c >= P; columns [P, ld_c) of C are neither read nor written.  C must not overlap a or B.
 *   1. s[m][p] is the ascending-j f32 fma chain from +0, one accumulator per output: the bits of msae_pre_acts_f32 with no
 *      biases and relu = 0.
 *   2. accumulate == 0: C = s.  accumulate != 0: C = C_in + s, ONE rounded f32 add per element, C_in read in the epilogue by
 *      the thread that writes the element (inf and NaN in C_in propagate as that add propagates them).  No atomics and no
 *      split-K: the result does not depend on the grid or on timing, and two runs give the same bits.
 *   3. Any M, K, P >= 1 (M <= 2^31 - 2^23, P <= 2^31 - 129).  K % 4 != 0 or a base that is not aligned to four elements
 *      takes the tile's generic staging (element loads), with the same bits.  M == 0 returns 0 and touches nothing.  A null
 *      pointer, a dtype code outside the three, K < 1, P < 1, M < 0 or ld_c < P: MSAE_EINVAL before any launch.
 *      Asynchronous on `stream`; allocates nothing, never synchronises, needs no workspace.
 * Uses: the forward skip term accumulated in place into the decode's output (a = x [T][d_in], B = W_skip [d_out][d_in],
 * C = yhat), and the weight gradient dW_skip (+)= g^T x as a = g^T [d_out][T], B = x^T [d_in][T]. */
int msae_gemm_nt_acc_f32(const void *a, int a_dtype, const float *B, int M, int K, int P, float *C, int ld_c,
                         int accumulate, void *stream);

/* Canonical top-k of each row of latents[T][N]: vals[T][k] descending, ties by ascending index.
 * idx is int32 (the host layer widens to int64 where the reference API returns int64). */
size_t msae_topk_ws_bytes(int T, int N, int k);
int msae_topk_f32(const float *latents, int T, int N, int k, float *vals, int32_t *idx, void *ws,
                  size_t ws_bytes, void *stream);

/* ---- fused encoder: bf16 MFMA candidate pass + exact f32 re-score ------------------------ */

/* One-time preparation of the encoder weights (bf16 copy of W_enc + a strided sample of its rows
 * used to set the per-token candidate threshold).  `prepared` must hold
 * msae_encoder_prepared_bytes(N, d) bytes and stay valid while the encoder is used. */
size_t msae_encoder_prepared_bytes(int N, int d);
int msae_encoder_prepare(const float *W_enc, int N, int d, void *prepared, void *stream);
/* The same with options (ABI 4): `dither` / `dither_seed` choose how the int8 operands are rounded (msae_options above;
 * msae_encoder_prepare = NULL options = the defaults: dithered with a drawn seed).  Two prepares with the same non-zero seed
 * build identical operands. */
int msae_encoder_prepare_opts(const float *W_enc, int N, int d, void *prepared, const msae_options *opts, void *stream);
/* Operands of the certified pass (msae_options::certified): two int8 planes of every row of W_enc (tile-major), the rows'
 * exact norms for the deterministic band, and the biases rounded up by 2^-20 |b| (b_enc may be NULL = zeros).  Once per weight
 * (and bias) load; msae_encoder_certified_bytes(N, d) bytes (0: the shape has no certified pass -- MSAE_ENOTIMPL here). */
size_t msae_encoder_certified_bytes(int N, int d);
int msae_encoder_prepare_certified(const float *W_enc, const float *b_enc, int N, int d, void *operands, void *stream);
/* Same buffer after a weight update (one training step): rebuilds only the operands that the coarse
 * mode of `opts` reads -- the other mode's operands go stale, so call msae_encoder_prepare again before
 * encoding in the other mode. */
int msae_encoder_refresh(const float *W_enc, int N, int d, void *prepared, const msae_options *opts,
                         void *stream);
/* The buffer records which operand groups hold the current weights (bf16 | int8 | fragment-major int8); a refresh clears
 * the record of everything it does not rebuild, and an encode whose candidate pass would read a stale group computes all
 * its tokens by the exact path instead (status 1; reason 128 with status_detail) -- stale operands cost time, never a
 * wrong top-k.
 * The same for ONE following encode of T_next tokens (the training loop, train/sae/sae/trainer.py:347-401: the weights change
 * before the buffer is read again): a batch of more than 256 tokens does not read the copies the small-batch kernels use,
 * and they are left stale (a later encode of <= 256 tokens falls back to the exact path until the next refresh / prepare). */
int msae_encoder_refresh_for(const float *W_enc, int N, int d, void *prepared, int T_next, const msae_options *opts,
                             void *stream);

/* Fused Sae.encode: vals/idx[T][k] = canonical top-k of relu((x - b_dec) W_enc^T + b_enc), with
 * the reference hooks' edits of the dense latents applied before TopK:
 *   set_feature >= 0 : latents[:, set_feature] = set_value       (steering.py:113-114)
 *   zero_feature >= 0: latents[:, zero_feature] = 0               (patching/utils.py:43-48)
 * status (optional, int32[T]): 0 = fast path verified; 1 = token recomputed by the exact path
 * inside the call (every flagged token is: the fallback runs ceil(T / rows) passes over a 1 GiB
 * scratch of f32[rows][N], 2048 rows at N = 131072, sized on the device -- no host round trip).
 * Values >= 2 exist only between the kernels of one call: 2 | reason bits (4 list overflow, 8
 * threshold <= 0, 16 fewer than k candidates, 32 too many rows inside the band, 64 a re-scored pair
 * was more than 6 sigma from its coarse value: the error model does not describe this token, 128 the token's
 * shape is outside the model by a deterministic test -- the dims its int8 scale rounds to zero carry more than 4
 * bands of energy).
 * Alignment: x 16 bytes for f32, 8 bytes for the 16-bit types; large batches of a 16-BYTE-aligned x additionally take the
 * feature-major route of the exact re-score (rows_rescored bit 30; same results, less time) -- torch allocations are. */
size_t msae_encode_topk_ws_bytes(int T, int d, int N, int k, const msae_options *opts);
int msae_encode_topk(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                     const float *b_dec, const void *prepared, int T, int d, int N, int k,
                     int set_feature, float set_value, int zero_feature, float *vals, int32_t *idx,
                     int32_t *status, void *ws, size_t ws_bytes, const msae_options *opts, void *stream);
/* The same call writing 64-bit indices (EncoderOutput.top_indices is int64 in the reference: Tensor.topk,
 * sae.py:179-181); saves the widening pass on the latency path (one decode step of steering). */
int msae_encode_topk_i64(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                         const float *b_dec, const void *prepared, int T, int d, int N, int k,
                         int set_feature, float set_value, int zero_feature, float *vals, int64_t *idx,
                         int32_t *status, void *ws, size_t ws_bytes, const msae_options *opts, void *stream);

/* Exact Sae.encode of a DEVICE-SIDE LIST of tokens: for i < min(*n_rows, max_rows), t = rows[i]:
 * vals[t][k] / idx[t][k] (/ status[t] = 1, optional) = the canonical top-k of token t by msae_pre_acts_f32 +
 * msae_topk_f32 -- what msae_encode_topk returns for t, bit for bit; rows of unlisted tokens are left untouched.
 * rows / n_rows are device pointers: the work is sized on the device (ceil(max_rows / capacity) passes over a
 * <= 1 GiB dense scratch are enqueued, passes without rows exit at once), so a caller can enqueue "redo whatever the
 * previous kernel flagged" without reading the count back -- the second round of the feature-sharded engine
 * (msae/parallel.py: shards whose truncated top-k_loc list may have lost a member), inside the same forward hook
 * (features/cache.py:187-204: no host synchronisation).  No reference counterpart. */
size_t msae_encode_topk_rows_ws_bytes(int max_rows, int N);
int msae_encode_topk_rows(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                          const float *b_dec, const int32_t *rows, const int32_t *n_rows, int max_rows,
                          int d, int N, int k, int set_feature, float set_value, int zero_feature,
                          float *vals, int64_t *idx, int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* ---- feature-sharded group (BASELINE configs[2]: "per-shard TopK + RCCL merge over xGMI") ------
 * The encoder's feature axis is split over G ranks; every rank sees the same T tokens.  Re-scoring a local top-k
 * exactly on every rank would multiply the HBM-bound re-score work by G, so the shards exchange CANDIDATES:
 *   msae_shard_candidates    rank g, all T tokens: candidate pass over its N/G features, then per token the C best
 *                            by upper value u as one record of msae_shard_record_bytes(C) bytes:
 *                            uint64 key[C] (order key of u << 32 | 0x7FFFFFFF - GLOBAL feature id, 0 = empty),
 *                            float z_sigma[C], float tau (largest u any OTHER feature of the shard can have; +inf when
 *                            the shard cannot bound it), float 0.  ws: msae_encode_topk_ws_bytes(T, d, N/G, k, opts) with the
 *                            same options, for every C >= 1 (the shard plans the same regions as the encode with a
 *                            threshold rank, list capacity and segment count that C can only lower, and without the
 *                            feature-major re-score: no region grows; less than the helper's size is MSAE_EWS all the
 *                            same).  MSAE_ENOTIMPL for shapes without the fused pass and for MSAE_COARSE_FP8 (its
 *                            band reads the f32 weights of the batch's massive-activation dims, which a shard call does
 *                            not receive): the caller runs msae_encode_topk per shard instead.
 *   (all-to-all / all-gather of the records: rank r needs the records of its tokens from every shard)
 *   msae_rescore_candidates  rank r, its T tokens (T_valid of them real): records[G][T] -> exact top-k against the
 *                            FULL W_enc / b_enc (replicated, 2 GiB of 288 GB), same verification rule as
 *                            msae_encode_topk (every feature with u >= v_k re-scored, v_k above every shard's tau,
 *                            model check), unverifiable tokens recomputed exactly in the call.  Bit-identical to the
 *                            single-GPU msae_encode_topk.  set_feature / zero_feature are global ids (both calls). */
size_t msae_shard_record_bytes(int C);
int msae_shard_candidates(const void *x, int x_dtype, const float *b_enc_shard, const float *b_dec,
                          const void *prepared_shard, int T, int d, int N_shard, int k, int row_offset, int C,
                          int set_feature, int zero_feature, void *records, void *ws, size_t ws_bytes,
                          const msae_options *opts, void *stream);
size_t msae_rescore_candidates_ws_bytes(int T, int d, int N, int k, int G, int C);
int msae_rescore_candidates(const void *x, int x_dtype, const float *W_enc, const float *b_enc,
                            const float *b_dec, int T, int T_valid, int d, int N, int k, int G, int C,
                            const void *records, int set_feature, float set_value, int zero_feature,
                            float *vals, int64_t *idx, int32_t *status, void *ws, size_t ws_bytes,
                            const msae_options *opts, void *stream);

/* ---- k-sparse decoder -------------------------------------------------------------------- */

/* out[A][d] = sum_j acts[A][j] * W_dec[idx[A][j]][:] + b_dec  (j-ordered f32 fma chain, entries
 * with acts == 0 skipped, kernels.py:277).  Indices outside [0, N) are skipped and, when
 * `status` (int32[1], optional) is given, flagged there (kernels.py:276 device_assert). */
int msae_decode_f32(const int32_t *idx, const float *acts, const float *W_dec, const float *b_dec,
                    int A, int k, int N, int d, float *out, int32_t *status, void *stream);
/* The same with 64-bit indices: the dtype Tensor.topk returns and the reference hands to decoder_impl
 * (sae.py:179-181,187-191) -- no narrowing copy between the encoder and the decoder. */
int msae_decode_i64_f32(const int64_t *idx, const float *acts, const float *W_dec, const float *b_dec,
                        int A, int k, int N, int d, float *out, int32_t *status, void *stream);

/* g_acts[A][k] = grad_out[A][:] . W_dec[idx[A][j]][:]   (dense-dense-sparse-out matmul).  An index outside
 * [0, N) yields g_acts = 0 for that pair and, when `status` (int32[1], optional) is given, is flagged there
 * like the forward does (kernels.py:389 device_assert). */
int msae_decode_bwd_acts_f32(const int32_t *idx, const float *grad_out, const float *W_dec, int A,
                             int k, int N, int d, float *g_acts, int32_t *status, void *stream);

/* g_W_dec[n][:] = sum over (a, j) with idx[a][j] == n of acts[a][j] * grad_out[a][:], written to
 * the WHOLE dense [N][d] buffer (the layout autograd expects for Sae.W_dec.grad; rows without a
 * pair are zero; no pre-zeroing needed).  Pairs are grouped by feature with a counting sort and
 * summed in ascending pair order (segments are sorted whatever their length), so the result is bit-reproducible.
 * Pairs whose index lies outside [0, N) contribute nothing and are flagged in `status` (int32[1], optional).
 * d % 4 == 0.  row_sumsq (optional, f32[N]) receives |g_W_dec[n][:]|^2 per row while the row is in registers: the
 * gradient-norm pass of clip_grad_norm_ (train/sae/sae/trainer.py:390) without re-reading the 2 GiB gradient
 * (msae_sum_f32 adds the rows up in a fixed order).  row_act_sum (optional, f32[N]) receives the sum of acts over the
 * row's pairs in ascending pair order: with acts = the latents' gradients (the sparse encoder backward, msae/ops.py) that is
 * the encoder-bias gradient, without index_add_'s atomics. */
size_t msae_decode_bwd_wdec_ws_bytes(int A, int k, int N);
int msae_decode_bwd_wdec_f32(const int32_t *idx, const float *acts, const float *grad_out, int A,
                             int k, int N, int d, float *g_W_dec, float *row_sumsq, float *row_act_sum,
                             int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* ---- feature-cache sparsify ------------------------------------------------------------------
 * From the per-token top-k (vals/idx[B*S][k], any order) produce the reference cache's COO
 * records in its order (row, pos, feature ascending):
 *     keep (|v| > thresh) and (filter_bitmap == NULL or filter_bitmap[feature] != 0)
 *     locations[n] = (row_base + b, s, feature) int64 ; activations[n] = v
 * Two calls: _count fills counts[B*S+1] (exclusive prefix sum, counts[B*S] = nnz) on the device;
 * the caller reads nnz, allocates, then _write emits the records. */
int msae_sparsify_count(const float *vals, const int32_t *idx, int B, int S, int k, float thresh,
                        const uint8_t *filter_bitmap, int N, int64_t *counts, void *stream);
int msae_sparsify_write(const float *vals, const int32_t *idx, int B, int S, int k, float thresh,
                        const uint8_t *filter_bitmap, int N, int64_t row_base,
                        const int64_t *counts, int64_t *locations, float *activations,
                        void *stream);

/* ---- per-feature statistics and top-example tables (opt-in part of the cache loop) ----------------
 * What the reference's explain side re-derives per feature from the split files afterwards, kept for ALL N
 * features as the batches stream by:
 *   how often it fires   the loader's min_examples cut       sae_auto_interp/features/loader.py:103-106
 *   its top examples     pool_max_activation_windows          features/constructors.py:28-85 (window mode)
 *                        pool_max_activations_windows_image   features/constructors.py:88-141 (image mode)
 * Input: one batch's top-k vals/idx[B*S][k] (any order inside a token; a token's indices distinct).  An entry is
 * kept when |v| > thresh and 0 <= idx < N (msae_sparsify's rule; there is no filter bitmap: the statistics cover
 * every feature, so filters can be chosen from them).  Per feature f, accumulated in place:
 *   count[f]    u64  kept (token, f) records                                         exact
 *   act_max[f]  f32  maximum kept value (initialise to -inf)                          exact
 *   act_sum[f]  f64  sum of kept values, one f64 atomic per (segment, f)             order-dependent at rounding level
 *   top_val[f][n_top] f32, top_id[f][n_top] i64: the n_top largest NONZERO pooled values of f seen so far, sorted by
 *               value descending then id ascending (a total order: the table is the same however the rows are cut
 *               into calls); free slots (0, -1) at the tail (initialise so).
 * Pooling segments (a row never spans two calls, so each segment is complete in one call):
 *   MSAE_POOL_IMAGE   one per row b: pooled = (f32 sum of the values at s < pool_len, ascending s) / pool_len
 *                     (avg_pool1d over the first num_image_tokens positions); id = row_base + b.
 *   MSAE_POOL_WINDOW  [w*W, (w+1)*W) of a row, W = window, w < S / W (positions >= (S / W) * W are not pooled, as
 *                     unfold / max_pool1d drop them); pooled = max over the window's dense values, i.e. a window
 *                     where f did not fire on every position also holds a 0; id = (row_base + b) * (S / W) + w.
 * Envelope: B*S <= 65536, k <= 256, N <= 262144, n_top <= 256, pool_len <= 2880, window <= 4096 (else
 * MSAE_EINVAL).  No host synchronisation, no allocation: the workspace is msae_feature_stats_ws_bytes(B*S, k, N).
 * _merge: dst += src for two sets of statistics of the same N and n_top (ranks, modules): counts add, maxima max,
 * sums add, tables merge in the same total order. */
enum { MSAE_POOL_IMAGE = 0, MSAE_POOL_WINDOW = 1, MSAE_STATS_MAX_T = 65536 };
size_t msae_feature_stats_ws_bytes(int T, int k, int N);
int msae_feature_stats_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N,
                              int mode, int pool_len, int window, int64_t row_base, int n_top, uint64_t *count,
                              float *act_max, double *act_sum, float *top_val, int64_t *top_id, void *ws,
                              size_t ws_bytes, void *stream);
int msae_feature_stats_merge(int N, int n_top, uint64_t *count, float *act_max, double *act_sum, float *top_val,
                             int64_t *top_id, const uint64_t *src_count, const float *src_max,
                             const double *src_sum, const float *src_val, const int64_t *src_id, void *stream);

/* ---- per-feature uniform example sample (opt-in part of the statistics update) ----------------------------------
 * The top tables answer the reference's train_type "top" (sae_auto_interp/features/samplers.py); "random" and
 * "quantile" (and detection-style scoring) need examples from a feature's whole activation range.  A CANDIDATE is what
 * it is for the top tables: one pooling segment of one feature with a nonzero pooled value c and its id.  Per
 * feature f, updated in place by the same call that updates the top tables:
 *   seg_count[f]          u64  candidates of f seen so far (the population the sample is drawn from)         exact
 *   smp_val[f][n_sample]  f32, smp_id[f][n_sample] i64: the n_sample candidates of f with the SMALLEST priority
 *                         prio(seed, f, id) = mix64( mix64(seed + 0x9E3779B97F4A7C15 * (f + 1)) ^ (uint64)id )
 *                         (arithmetic mod 2^64; mix64 = the splitmix64 finaliser: z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9,
 *                         z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^ z >> 31), sorted by priority ascending, then id
 *                         ascending; free slots (0, -1) at the tail (initialise so, and seg_count to 0).
 *                         1 <= n_sample <= 256.  Only val and id are stored: priorities are recomputed from (f, id).
 * For fixed (seed, f) the priority is a bijection of id, so distinct ids never tie; f is mixed in so that two features'
 * samples do not prefer the same rows.  Pinned:
 *   prio(22, 0, 0) = 0xbe5264ad2aa020f4          prio(1, 5, 7) = 0xb2e6c178b81a5c56
 *   prio(22, 7, 2^33) = 0x27044a0765e2616f       prio(22, 131071, 12345) = 0x45984866898b23bf
 *   prio(2^64 - 1, 262143, 2^40 + 3) = 0xaf8ee0a530541d25
 * Consequences:
 *   - the table is a uniform sample without replacement of the feature's candidates (bottom-n of a hash of the id);
 *   - it is independent of the candidates' values;
 *   - it is bit-identical however the rows are cut into calls, in whatever order the calls arrive, and however the rows
 *     are split over ranks (msae_feature_sample_merge);
 *   - the first m entries of a table are the table one would get with n_sample = m and the same seed.
 * Ids are unique per feature over a table's life because a row never spans two calls.  A caller that breaks that may
 * see the id twice in a table, as in the top table; nothing else is promised, and nothing faults.
 * msae_feature_stats_update_sampled: msae_feature_stats_update with `sample` (NULL: exactly that call); the workspace
 * is the same msae_feature_stats_ws_bytes.  `sample->size` is sizeof(msae_feature_sample) of the caller.  n_sample
 * outside 1..256, a short struct or a null table pointer: MSAE_EINVAL before any launch.
 * msae_feature_sample_merge: dst += src for two samples of the same N, n_sample and seed: counts add, tables merge in
 * the same (priority, id) order.  Neither call allocates or synchronises with the host. */
typedef struct msae_feature_sample {
  uint32_t size;        /* sizeof(msae_feature_sample) */
  int32_t n_sample;     /* 1..256 */
  uint64_t seed;
  uint64_t *seg_count;  /* [N] */
  float *smp_val;       /* [N][n_sample] */
  int64_t *smp_id;      /* [N][n_sample] */
} msae_feature_sample;
int msae_feature_stats_update_sampled(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N,
                                      int mode, int pool_len, int window, int64_t row_base, int n_top,
                                      uint64_t *count, float *act_max, double *act_sum, float *top_val,
                                      int64_t *top_id, const msae_feature_sample *sample, void *ws, size_t ws_bytes,
                                      void *stream);
int msae_feature_sample_merge(int N, int n_sample, uint64_t seed, uint64_t *seg_count, float *smp_val,
                              int64_t *smp_id, const uint64_t *src_seg_count, const float *src_val,
                              const int64_t *src_id, void *stream);

/* ---- co-activation counters of a query list, and neighbour lists from them (msae.features.CoactStats) ---------------
 * Which features fire together, counted while the cache runs, for F query features (no reference counterpart; the
 * decoder-geometry neighbours are msae_rows_topk_f32).  Input: one batch's top-k vals/idx[B*S][k], as the feature
 * statistics take it; an entry is kept when |v| > thresh and 0 <= idx < N (no filter bitmap on the member side).
 * Segments (a row never spans two calls, so each segment is complete in one call):
 *   MSAE_POOL_TOKEN   every position its own segment: B*S per call
 *   MSAE_POOL_WINDOW  positions s < (S / W) * W belong to b * (S / W) + s / W (the ragged tail is not pooled): B * (S / W)
 *   MSAE_POOL_IMAGE   positions s < pool_len belong to segment b, later ones to none: B
 * A feature is ACTIVE in a segment that holds at least one kept entry of it; a repeat inside a segment counts once.
 * State, updated in place (initialise to 0):
 *   counts[F][N]  i32  counts[i][g] = segments in which the query of slot i and g are both active; the entry at the
 *                      query's own column is the query's count
 *   seg_count[N]  u64  segments in which g is active
 * slot_of[N] i32: the slot of a query feature, -1 for every other feature (a value outside [0, F) counts as -1).
 * Every update is an integer atomic add: the state is bit-identical however the rows are cut into calls, in whatever
 * order the calls arrive, and adds over ranks.  A counter wraps at 2^31 segments: the caller keeps the total below.
 * Envelope: B*S <= 65536, k <= 256, N <= 262144, 1 <= F <= 16384, pool_len <= 2880, window <= 4096 (else MSAE_EINVAL).
 * No host synchronisation, no allocation: the workspace is msae_coact_ws_bytes(B*S, k, N) (token mode uses none of it),
 * whatever F and however many entries are queries.
 * msae_coact_topk: for slot i with query q = queries[i] and every g with c = counts[i][g] > 0 (g != q with exclude_self)
 *   MSAE_COACT_JACCARD  score = (float)((double)c / (double)(seg_count[q] + seg_count[g] - c))   integers, one f64
 *                       quotient (IEEE, correctly rounded), one rounding to f32
 *   MSAE_COACT_COUNT    score = (float)c
 *   out_val[F][m] / out_idx[F][m]: the best m in (score descending, g ascending) order -- the library's rank key --,
 *   free slots (0.0, -1) at the tail.  1 <= m <= 64.  A pure function of the state; no scratch. */
enum { MSAE_POOL_TOKEN = 2 };
enum { MSAE_COACT_JACCARD = 0, MSAE_COACT_COUNT = 1 };
size_t msae_coact_ws_bytes(int T, int k, int N);
int msae_coact_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N, int mode,
                      int pool_len, int window, const int32_t *slot_of, int F, int32_t *counts, uint64_t *seg_count,
                      void *ws, size_t ws_bytes, void *stream);
int msae_coact_topk(const int32_t *counts, const int64_t *seg_count, const int32_t *queries, int F, int N, int m,
                    int metric, int exclude_self, float *out_val, int32_t *out_idx, void *stream);
int msae_coact_topk_i64(const int32_t *counts, const int64_t *seg_count, const int32_t *queries, int F, int N, int m,
                        int metric, int exclude_self, float *out_val, int64_t *out_idx, void *stream);

/* ---- per-feature activation histograms, and quantile bins from them (msae.features.ActHist) --------------------------
 * HOW STRONGLY every feature fires, counted while the cache runs (no reference counterpart: the reference rebuilds dense
 * per-feature tensors on the CPU for a handful of features).  Input: one batch's top-k vals/idx[B*S][k], as the feature
 * statistics take it; an entry is kept when |v| > thresh and 0 <= idx < N (no filter bitmap).
 * The bin rule is defined on the float32 bits, with no transcendental function and no tolerance.  Parameters: sub_bits s in
 * [0, 4], e_lo (the exponent of the lowest octave, -126 <= e_lo, e_lo + octaves <= 128), octaves E >= 1,
 * n_bins = E << s in [1, 512].  For a value c > 0 with bit pattern u:
 *   raw     = (u >> (23 - s)) - ((127 + e_lo) << s)
 *   bin     = clamp(raw, 0, n_bins - 1)
 *   edge(b) = the float with bits ((b + ((127 + e_lo) << s)) << (23 - s)),  b = 0 .. n_bins
 * so values below 2^e_lo (subnormals included) land in bin 0, values >= 2^(e_lo + E) and +inf in the last bin, and an
 * unclamped value satisfies edge(bin) <= c < edge(bin + 1).  With s = 3, e_lo = -16, E = 32 (256 bins over [2^-16, 2^16),
 * 8 per octave): 1e-5 -> 0, 1.0 -> 128, 1.125 -> 129, 65536 and +inf -> 255.
 * A SEGMENT VALUE c of feature f (a row never spans two calls, so each segment is complete in one call):
 *   MSAE_POOL_TOKEN   every kept entry is its own value, c = v; nothing is de-duplicated (a caller's repeat counts twice)
 *   MSAE_POOL_WINDOW  exactly the candidate msae_feature_stats_update ranks, bit for bit: the maximum of f's kept values in
 *                     the window, joined with 0 unless f has W kept entries there (positions >= (S / W) * W are not pooled)
 *   MSAE_POOL_IMAGE   likewise: the f32 sum of f's kept values at s < pool_len, added in ascending s (list order inside a
 *                     token) from +0, divided by (float)pool_len
 * State, updated in place (initialise to 0):
 *   hist[N][n_bins]  i32  hist[f][bin(c)] += 1 for every segment value c > 0 of f.  NaN, zero and negative values are
 *                         counted nowhere.
 * Every update is an integer atomic add: the state is bit-identical however the rows are cut into calls, in whatever
 * order the calls arrive, and adds over ranks.  A counter wraps at 2^31: the caller keeps the number of segments below.
 * Envelope: B*S <= 65536, k <= 256, N <= 262144, pool_len <= 2880, window <= 4096, the bin parameters as above (else
 * MSAE_EINVAL).  No host synchronisation, no allocation: the workspace is msae_act_hist_ws_bytes(B*S, k, N) (token mode
 * uses none of it).
 * msae_act_hist_quantiles: bins[N][Q] i32 from hist, Q probabilities qs[Q] (f64, device; 1 <= Q <= 64; each in [0, 1]),
 *   n_segments (segments seen, empty ones included) and the `zeros` flag.  Per feature, with n = the row total and
 *   z = max(n_segments - n, 0) if zeros else 0 (the segments in which the feature's value was not > 0):
 *     rank r = clamp(ceil(q * (double)(n + z)), 1, n + z)       one IEEE f64 multiply, then ceil
 *     bin    = the first b with hist[f][0] + .. + hist[f][b] + z >= r;  -1 when r <= z (the quantile is a zero);
 *              -2 when n + z = 0 (nothing to rank)
 *   A pure function of its arguments; no scratch, no host synchronisation, no allocation. */
size_t msae_act_hist_ws_bytes(int T, int k, int N);
int msae_act_hist_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N, int mode,
                         int pool_len, int window, int sub_bits, int e_lo, int octaves, int32_t *hist, void *ws,
                         size_t ws_bytes, void *stream);
int msae_act_hist_quantiles(const int32_t *hist, int N, int n_bins, const double *qs, int Q, int64_t n_segments,
                            int zeros, int32_t *bins, void *stream);

/* ---- per-feature position profiles, and the peak bin read from them (msae.features.PosProfile) -----------------------
 * WHERE IN A ROW every feature fires, counted while the cache runs (no reference counterpart: the reference's only defence
 * against positional features is a hard-coded window offset, features/constructors.py:204).  Input: one batch's top-k
 * vals/idx[B*S][k], as the feature statistics take it; an entry is kept when |v| > thresh and 0 <= idx < N (no filter
 * bitmap).  Per token: there are no pooling modes.
 * The position table pos_bin[L] (i32, device; 1 <= L <= 65536) and tail_bin name the BIN of a position s of a row:
 *   bin(s) = pos_bin[s] for s < L, tail_bin for s >= L;  bins are 0 .. P - 1 (1 <= P <= 1024), -1 = counted nowhere.
 * tail_bin outside [-1, P) is MSAE_EINVAL; a table value outside [0, P) counts as -1 (the table is on the device and is
 * not read back: nothing faults).
 * A kept entry (v, f) at a position with bin b >= 0 is COUNTED iff v > 0 -- the histograms' rule: NaN, zero and negative
 * values are counted nowhere; nothing is de-duplicated (a caller's repeat counts twice).  State, updated in place
 * (initialise to 0):
 *   count[N][P]  i32  count[f][b] += 1
 *   mass[N][P]   u64  mass[f][b]  += q(v),  q(v) = llrint((double)v * 2^20) in round-half-to-even, saturated at 2^60 for
 *                     v >= 2^40 (+inf included): the value in fixed point, 20 fractional bits.  The sum is mod 2^64.
 *                     q(2^-21) = 0 (a tie, to even), q(3 * 2^-21) = 2, q(1.0) = 2^20, q(any subnormal) = 0.
 * Every update is an integer atomic add: the state is bit-identical however the rows are cut into calls, in whatever
 * order the calls arrive, and adds over ranks.  A counter wraps at 2^31: the caller keeps the number of positions below.
 * Envelope: B*S <= 65536, k <= 256, N <= 262144, L and P as above (else MSAE_EINVAL).  No host synchronisation, no
 * allocation.  msae_pos_profile_ws_bytes(B*S, k, N) is 0 for every shape: the update needs no workspace, ws / ws_bytes are
 * not looked at, and MSAE_EWS is never returned.
 * msae_pos_profile_summary: from count and bin_positions[P] (i64, device: positions seen per bin, each below 2^31)
 *   fired[N]    i64  the row total of count
 *   peak[N][2]  i32  (b, count[f][b]) of the bin with the highest firing RATE count[f][b] / bin_positions[b] among the bins
 *                    with bin_positions[b] > 0, rates compared exactly (c1 * n2 against c2 * n1 in int64); equal rates:
 *                    the lowest bin; (-1, 0) when no such bin has a count (fired = 0 for a state the update produced).
 *   Envelope: N <= 262144, P <= 1024.  A pure function of its arguments; no scratch, no host synchronisation, no
 *   allocation. */
size_t msae_pos_profile_ws_bytes(int T, int k, int N);
int msae_pos_profile_update(const float *vals, const int32_t *idx, int B, int S, int k, float thresh, int N,
                            const int32_t *pos_bin, int L, int tail_bin, int P, int32_t *count, uint64_t *mass, void *ws,
                            size_t ws_bytes, void *stream);
int msae_pos_profile_summary(const int32_t *count, const int64_t *bin_positions, int N, int P, int64_t *fired,
                             int32_t *peak, void *stream);

/* ---- token profiles of a query list, and the top tokens read from them (msae.features.TokenProfile) -------------------
 * ON WHICH TOKENS a feature fires, counted while the cache runs, for F query features (the reference's
 * features/stats.py::unigram, which joins every record with the token stream on the host).  Input: one batch's top-k
 * vals/idx[B*S][k], as the feature statistics take it, and the batch's token ids[B*S] (i32 or i64: ids_bits = 32 / 64).
 * Parameters: slot_of[N] i32, the slot of a query feature and -1 for every other feature (a value outside [0, F) counts as
 * -1); a vocabulary size V; O offsets o_0 .. o_{O-1} (a HOST array, read during the call: distinct, each in [-64, 64],
 * 1 <= O <= 4).
 * An entry (v, f) at position (b, s) is COUNTED iff it is kept (|v| > thresh and 0 <= f < N, no filter bitmap) and v > 0 --
 * the position profiles' rule: NaN, zero and negative values are counted nowhere; nothing is de-duplicated (a caller's
 * repeat counts twice).  State, updated in place (initialise to 0), for the query of slot i = slot_of[f]:
 *   counts[O][F][V]  i32  counts[a][i][t] += 1      for every a with 0 <= s + o_a < S and t = ids[b][s + o_a]
 *   mass[O][F][V]    u64  mass[a][i][t]   += q(v)   likewise; q is the position profiles' q (above), bit for bit; the sum
 *                         is mod 2^64.  Optional: NULL keeps no mass.
 *   tok_count[O][V]  u64  tok_count[a][t] = positions (b, s) with 0 <= s + o_a < S and ids[b][s + o_a] == t, whether or not
 *                         anything fired there: counts / tok_count is P(the query fires at s | token t at s + o_a).
 * A token id outside [0, V) is counted nowhere (counts, mass and tok_count alike); offsets never cross a row.  Nothing is
 * indexed by a list entry's feature, a slot or a token id before its range check: a hostile value costs its own entry's count
 * at most.
 * Every update is an integer atomic add: the state is bit-identical however the rows are cut into calls, in whatever order
 * the calls arrive, and adds over ranks.  A counter wraps at 2^31: the caller keeps the number of positions below.
 * Envelope: B*S <= 65536, k <= 256, N <= 262144, 1 <= F <= 16384, V >= 1, O * F * V < 2^31 (else MSAE_EINVAL, as are bad
 * offsets and an ids_bits other than 32 / 64).  Asynchronous on `stream`; no host synchronisation, no allocation, no
 * workspace.
 * msae_token_profile_topk: over ONE offset plane (counts[F][V], mass[F][V] or NULL, tok_count[V]), for every row i and
 * every token t with c = counts[i][t] >= min_count (min_count >= 1):
 *   MSAE_TOKEN_COUNT      score = (float)c
 *   MSAE_TOKEN_PRECISION  score = (float)((double)c / (double)tok_count[t])           one f64 quotient, one rounding to f32
 *   MSAE_TOKEN_MEAN       score = (float)((double)mass[i][t] / (double)c * 2^-20)     mass read as UNSIGNED; one conversion
 *                         (correctly rounded), one f64 quotient, an exact scaling, one rounding to f32.  MSAE_EINVAL without mass.
 *   out_val[F][m] f32 / out_tok[F][m] i32: the best m in (score descending, token ascending) order -- the library's rank
 *   key --, free slots (0.0, -1) at the tail.  The order is that of the f32 SCORE: counts above 2^24 that round to one float
 *   tie, and the lower token comes first.  out_total[F] i64: the row total of counts (every token, whatever min_count).
 *   1 <= m <= 64.  A pure function of the state; no scratch, no host synchronisation, no allocation. */
enum { MSAE_TOKEN_COUNT = 0, MSAE_TOKEN_PRECISION = 1, MSAE_TOKEN_MEAN = 2 };
int msae_token_profile_update(const float *vals, const int32_t *idx, const void *ids, int ids_bits, int B, int S, int k,
                              float thresh, int N, const int32_t *slot_of, int F, int V, const int32_t *offsets, int O,
                              int32_t *counts, uint64_t *mass, uint64_t *tok_count, void *stream);
int msae_token_profile_update_i64(const float *vals, const int64_t *idx, const void *ids, int ids_bits, int B, int S, int k,
                                  float thresh, int N, const int32_t *slot_of, int F, int V, const int32_t *offsets, int O,
                                  int32_t *counts, uint64_t *mass, uint64_t *tok_count, void *stream);
int msae_token_profile_topk(const int32_t *counts, const uint64_t *mass, const int64_t *tok_count, int F, int V, int m,
                            int metric, int min_count, float *out_val, int32_t *out_tok, int64_t *out_total, void *stream);

/* ---- probe: segment-pooled feature ranking and activation maps (Sae.probe) ---------------------------------------
 * Replaces the dense probe of tools/probe_activations.py:109-126 (latents = pre_acts(h); latents.mean(0).topk(k);
 * latents[:, :, idx]) without materialising the [T][N] latents.  x[T][d] (element type x_dtype) as msae_pre_acts_f32;
 * seg: int32 [S][2] device array of token ranges [start, end) over the T rows.  Segments are trusted but never fault: each
 * is clamped to [0, T), an empty (or inverted) one pools to 0.  Neither call reads anything back to the host, allocates,
 * or needs scratch.
 * Numerics contract (v[t][f] = relu((x[t] - b_dec) W_enc[f]^T + b_enc[f]) as msae_pre_acts_f32 computes it, bit for bit):
 *   MSAE_REDUCE_MEAN  out[s][f] = (float)(S_f / n): S_f the f64 sum of (double)v[t][f] over the segment's tokens, added one
 *                     by one in ascending t from +0.0; n the segment length as a double.  Independent of the chunk plan, the
 *                     tile packing and the other segments: a segment gives the same bits alone or in any batch.
 *   MSAE_REDUCE_MAX   out[s][f] = max_t v[t][f], exact; 0 for an all-zero column.
 *   ranking           msae_topk_f32 on out[S][N] (canonical: value desc, index asc).
 *   maps              maps[t][j] = v[t][idx[s][j]] bit for bit for t in segment s; 0 for a t outside every segment and for
 *                     an idx outside [0, N).  (Overlapping segments: a token of two takes either one's map.)
 * msae_pooled_acts_f32: out[S][N].  chunks (optional, int32 [C][2] device array: segment ranges [first, last) in ascending
 *   order, each a run of ADJACENT segments -- no token between them -- and every segment in exactly one; msae/sae/probe.py
 *   plans them) groups short segments so that one workgroup walks them as packed 128-token tiles; NULL = one chunk per
 *   segment (what device-side segments use).  A segment no chunk names pools to 0.
 *   Envelope: any d, N (N % 128 != 0 included), S <= 65535 * 65535; reduce MSAE_REDUCE_MEAN or MSAE_REDUCE_MAX.
 * msae_probe_maps_f32: maps[T][k], idx int32 [S][k] (the ranking's indices).  Envelope: 1 <= k <= MSAE_PROBE_MAX_K. */
enum { MSAE_REDUCE_MEAN = 0, MSAE_REDUCE_MAX = 1, MSAE_PROBE_MAX_K = 256 };
int msae_pooled_acts_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc, const float *b_dec, int T,
                         int d, int N, const int32_t *seg, int S, const int32_t *chunks, int C, int reduce, float *out,
                         void *stream);
int msae_probe_maps_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc, const float *b_dec, int T,
                        int d, int N, const int32_t *seg, int S, const int32_t *idx, int k, float *maps, void *stream);

/* ---- neighbours and top logits: fused f32 GEMM + per-row top-k (Sae.neighbors, Sae.top_logits) ----------------------
 * Replaces sae_auto_interp/features/stats.py:76-120 (cos + get_neighbors: normalise, torch.mm, torch.topk) and
 * stats.py:12-47 (logits: torch.matmul, torch.topk) without materialising the [M][N] product.  Both calls are asynchronous
 * on `stream`; neither allocates nor reads anything back to the host.
 * msae_rows_topk_f32: queries are the rows q_rows[m] of Q[Qn][d] (q_rows NULL: row m, M <= Qn), keys K[N][d];
 *   vals[M][k] f32, idx[M][k] int32 key indices.  Numerics contract:
 *   1. dot[m][n] is the ascending-k f32 fma chain from +0 of Q[q_rows[m]][c] * K[n][c] -- msae_pre_acts_f32's tile with
 *      b_dec = NULL and rows = q_rows, bit-identical to oracle.pre_acts(Q[q_rows], K, 0, 0, relu=False).
 *   2. value = dot, then * q_scale[m] if given, then * k_scale[n] if given: each its own rounded f32 multiply.
 *   3. Ranking: the canonical top-k of row m over all n -- value descending, index ascending, by the library's rank key, so
 *      +-0 and non-finite values rank exactly as msae_topk_f32 ranks them.  n == exclude[m] is left out (exclude[m] < 0:
 *      nothing).  k > N - (exclude != NULL ? 1 : 0) returns MSAE_EINVAL.  Values are decoded from the rank key, as
 *      msae_merge_topk's are: a value of -0 is returned as +0.
 *   4. The result does not depend on `chunks`, on the grid, or on which other queries are in the call.
 *   Envelope: any d (d % 4 != 0 and unaligned pointers take the tile's generic staging path), any N (N % 128 != 0
 *   included), any M >= 0, 1 <= k <= 64.  q_rows may be unsorted and hold repeats; an entry outside [0, Qn) is clamped
 *   into it, never faults.  chunks: 0 = chosen by the library (the smallest count that gives two workgroups per CU over
 *   the 128-query tiles, at most the 128-key strips and 8192 / k), > 0 = forced (tests; capped at the strips,
 *   MSAE_EINVAL beyond 8192 / k).  ws: msae_rows_topk_ws_bytes(M, N, k, chunks) bytes, read when q_rows is given or more than
 *   one chunk runs -- then a missing or smaller one is MSAE_EWS -- (the clamped row list, the merge
 *   mask of the int64 variant, then the per-chunk lists [chunks][2][M][k] in msae_merge_topk's `gathered` layout, merged by one msae_merge_topk call).
 * msae_row_inv_norms_f32: inv[n] = the f32 nearest to 1 / max(||W_n||_2, 1e-12) (F.normalize's clamp) evaluated in f64
 *   (fixed summation order, no atomics: bit-reproducible; <= 1 f32 ulp from numpy f64).  The cosine is defined from the
 *   arrays the caller passes as q_scale / k_scale, so points 1-4 hold whatever order the norms were summed in. */
int msae_row_inv_norms_f32(const float *W, int N, int d, float *inv, void *stream);
size_t msae_rows_topk_ws_bytes(int M, int N, int k, int chunks);
int msae_rows_topk_f32(const float *Q, int Qn, const int32_t *q_rows, int M, const float *K, int N, int d,
                       const float *q_scale, const float *k_scale, const int32_t *exclude, int k, int chunks,
                       float *vals, int32_t *idx, void *ws, size_t ws_bytes, void *stream);
/* the same with int64 indices (Tensor.topk's index type) written directly: no widening pass, no int32 copy */
int msae_rows_topk_i64_f32(const float *Q, int Qn, const int32_t *q_rows, int M, const float *K, int N, int d,
                           const float *q_scale, const float *k_scale, const int32_t *exclude, int k, int chunks,
                           float *vals, int64_t *idx, void *ws, size_t ws_bytes, void *stream);

/* ---- exact encode over a feature subset (AuxK without the dense latents; Sae.pre_acts(x, features=...)) ----------------
 * Replaces the AuxK selection of sae_auto_interp/sae/sae.py:207-225, where(dead_mask, pre_acts, -inf).topk(k_aux), without
 * the two dense [T][N] tensors: pre-activations of the M listed features only, then the canonical top-k of rows of width M.
 * Both calls are asynchronous on `stream`; neither allocates, needs scratch, nor reads anything back to the host.
 * msae_pre_acts_features_f32: features int32 [M] (device), out[T][ld_out] with ld_out >= M; columns [M, ld_out) are not
 *   written.  Numerics contract: out[t][m] is bit for bit the value msae_pre_acts_f32 writes at [t][features[m]] -- the same
 *   ascending-k single-accumulator f32 fma chain of (x[t][c] - b_dec[c]) * W_enc[f][c] from +0, then + b_enc[f], then the
 *   same ReLU rule (relu != 0: a value that is not > 0 becomes +0).  It does not depend on M, on the order of the list or
 *   on its other entries.  The list may be unsorted and may repeat entries; an entry outside [0, N) is clamped into it,
 *   never faults (as q_rows in msae_rows_topk_f32).
 *   Envelope: any d (d % 4 != 0 and unaligned pointers take the tile's generic staging path), any M >= 0 (M == 0 returns 0
 *   without a launch), T as msae_pre_acts_f32 (T <= 65535 * 128, else MSAE_ENOTIMPL), x in f32, bf16 or f16.
 * msae_topk_map_i64_f32: msae_topk_f32 on latents[T][ld] rows of width M (ld >= M), with idx[t][j] = col_map[p] (int64) for
 *   the winner at position p.  Selection, values and tie order are msae_topk_f32's: value descending, then ascending
 *   POSITION -- with an ascending col_map that is ascending feature index, i.e. exactly the dense where(...).topk()
 *   result restricted to the listed features.  1 <= k <= min(M, 16384).  Rows with M % 4 == 0, ld % 4 == 0 and a 16-byte
 *   aligned base take the vector loads. */
int msae_pre_acts_features_f32(const void *x, int x_dtype, const float *W_enc, const float *b_enc, const float *b_dec,
                               const int32_t *features, int M, int T, int d, int N, int relu,
                               float *out, int ld_out, void *stream);
int msae_topk_map_i64_f32(const float *latents, int T, int M, int k, int ld, const int32_t *col_map,
                          float *vals, int64_t *idx, void *stream);

/* ---- set-valued hook edits on a top-k list (Sae.encode(edits=...)) -------------------------------
 * The reference's hooks edit the dense latents with torch indexing, so the edited feature may be a LIST or tensor:
 * latents[:, :, f] = clamp (features/steering.py:113-114), mask[:, off_features] = 0 (features/patching/utils.py:43-48).
 * msae_encode_topk takes one feature of each kind; a set of E distinct features is applied AFTER an unedited encode that
 * over-fetched kk >= k + E entries per token:
 *   vals_in / idx_in [T][kk]  msae_encode_topk's output for k' = kk with no edit (canonical order; idx in [0, N))
 *   edit_feat int32 [E]       the edited features, STRICTLY ASCENDING, each in [0, N)
 *   edit_val f32 [E]          the value of a SET edit (ignored for a ZERO edit)
 *   edit_kind int32 [E]       MSAE_EDIT_SET or MSAE_EDIT_ZERO
 *   vals / idx [T][k]         outputs; must not overlap the inputs
 * Asynchronous on `stream`; allocates nothing, never synchronises, needs no workspace (the sort of a token's at most
 * 8192 keys is LDS-resident, one workgroup per token).  MSAE_EINVAL: E < 1, k < 1, kk < k + E, k + E > N,
 * k + E > 4096 (msae_encode_topk's own limit on k), T < 0, a null pointer.  T == 0 does nothing.
 * Contract (L = msae_pre_acts_f32's latents of the encode that produced the list):
 *   1. The output is the canonical top-k (value descending, index ascending) of L' with L'[:, f] = edit_val for a SET
 *      edit and L'[:, f] = +0 for a ZERO edit -- bit-identical to msae_topk_f32 on the edited dense latents for finite
 *      pre-activations.  A feature has ONE entry in the table: the host layer (msae.features.FeatureEdits) gives ZERO
 *      precedence where a feature is named in both lists (the oracle applies set, then zero).
 *   2. With E = 1 it is bit-identical to msae_encode_topk's scalar set_feature / zero_feature arguments.
 *   3. A SET value <= 0 ranks by the same key rule as msae_topk_f32 (+-0 tie with the zero fill by index, negatives below
 *      every zero); because k + E <= N a negative value is never selected.  Values are decoded from the rank key: a
 *      value of -0 is returned as +0.
 *   4. A non-finite pre-activation AT AN EDITED FEATURE: the result holds the set value or +0, where the reference's
 *      mask multiply would produce NaN from NaN * 0 (a flagged quirk).
 *   5. Only the first k + E entries of a row are read: the result does not depend on kk beyond kk >= k + E, nor on T or
 *      on the other tokens of the call.
 *   6. The `status` of the underlying encode describes the result unchanged (the kernel does not touch it). */
enum { MSAE_EDIT_SET = 0, MSAE_EDIT_ZERO = 1,
       MSAE_EDIT_SCALE = 2, MSAE_EDIT_ADD = 3, MSAE_EDIT_FLOOR = 4, MSAE_EDIT_CAP = 5 };   /* the valued forms below only */
int msae_edit_topk_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *edit_feat,
                       const float *edit_val, const int32_t *edit_kind, int E, int N, int k, float *vals, int32_t *idx,
                       void *stream);
/* the same reading and writing 64-bit indices (msae_encode_topk_i64's output type) */
int msae_edit_topk_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk, const int32_t *edit_feat,
                           const float *edit_val, const int32_t *edit_kind, int E, int N, int k, float *vals,
                           int64_t *idx, void *stream);

/* ---- per-token edit tables (Sae.encode(edits=RowEdits, edit_group=...)) ---------------------------
 * The same edit with a table that is a function of the token: B features steered in the B rows of one generate, G
 * ablations in the G copies of one attribution batch.  The tables of G groups are concatenated:
 *   group_of int32 [T]        the group of token t; any value outside [0, G) (-1 by convention): the token is unedited
 *   group_off int32 [G + 1]   ascending offsets into the edit arrays: group g owns [group_off[g], group_off[g + 1])
 *   edit_feat / edit_val / edit_kind [E_total]   as above; edit_feat STRICTLY ASCENDING inside each group
 *   E_max                     >= every group's length; it sizes the sort (and the kernel layout) of the whole call
 *   edited uint8 [T][k] or NULL   1 where the output slot came from an edit entry (the differentiable encode masks those)
 * Asynchronous on `stream`; allocates nothing, never synchronises, needs no workspace.
 * MSAE_EINVAL: T < 0, G < 1, k < 1, E_max < 1, E_total < 0, k + E_max > min(N, 4096), kk < k + E_max, a null pointer
 * (`edited` may be null).  T == 0 does nothing and returns 0.
 * Contract:
 *   1. Edited tokens.  For g = group_of[t] in [0, G) with E_g > 0 entries the output row is the canonical top-k (value
 *      descending, index ascending) of the latents edited with group g's table -- bit-identical to what msae_edit_topk_f32
 *      returns for that token with that table alone (so points 1-4 and 6 above hold per token).
 *   2. Entries read.  Only the first k + E_g entries of the row are read: the result does not depend on kk beyond
 *      kk >= k + E_max, nor on the other tokens or groups of the call.
 *   3. Unedited tokens.  A token whose group id lies outside [0, G), and a token of an empty group (E_g = 0), gets the
 *      first k input entries copied bit for bit, `edited` all 0: a batch carries its unedited baseline row this way.
 *   4. Device data.  group_of and group_off are never trusted: a slice is clamped into [0, E_total], its length into
 *      [0, E_max].  Like msae_edit_topk_f32 the kernels never index memory by a list entry's feature.  A hostile id or
 *      offset can give a wrong row for that token; it cannot give an out-of-bounds access.
 *   5. Layout.  next_pow2(k + 2 E_max) <= 256: one wave per token, keys in registers, no LDS, no barriers; above: one
 *      workgroup per token with the token's slice and keys in LDS (8 next_pow2(k + 2 E_max) + 4 E_max bytes <= 80 KiB). */
int msae_edit_topk_rows_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *group_of,
                            const int32_t *group_off, int G, const int32_t *edit_feat, const float *edit_val,
                            const int32_t *edit_kind, int E_total, int E_max, int N, int k, float *vals, int32_t *idx,
                            uint8_t *edited, void *stream);
/* the same reading and writing 64-bit indices */
int msae_edit_topk_rows_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk, const int32_t *group_of,
                                const int32_t *group_off, int G, const int32_t *edit_feat, const float *edit_val,
                                const int32_t *edit_kind, int E_total, int E_max, int N, int k, float *vals, int64_t *idx,
                                uint8_t *edited, void *stream);

/* ---- value-dependent edits (FeatureEdits(scale=, add=, floor=, cap=)) ------------------------------
 * SET and ZERO ignore the feature's activation.  The four kinds below are functions of it: amplify a feature where it
 * fires, add to it, keep it above or below a bound.  With c = L[t][f] the exact post-ReLU latent (msae_pre_acts_f32's bits)
 * and v = edit_val[e]:
 *   kind               L'[t][f]                      gain = dL'/dL * [c > 0]
 *   MSAE_EDIT_SET      v                             0
 *   MSAE_EDIT_ZERO     +0                            0
 *   MSAE_EDIT_SCALE    c * v   (one f32 multiply)    v * [c > 0]
 *   MSAE_EDIT_ADD      c + v   (one f32 add)         [c > 0]
 *   MSAE_EDIT_FLOOR    fmaxf(c, v)                   [c > 0 && c >= v]
 *   MSAE_EDIT_CAP      fminf(c, v)                   [c > 0 && c <= v]      (torch.clamp's convention at the tie)
 * The list alone cannot supply c: a feature outside a token's first k + E entries has an unknown value <= the last entry's,
 * and an increasing edit can lift it into the top-k.  The valued forms therefore take, beside the arguments of
 * msae_edit_topk_f32 / msae_edit_topk_rows_f32 (same meaning, same MSAE_EINVAL cases):
 *   cur f32 [T][ld_cur]           the edited features' exact latents: msae_pre_acts_features_f32's output (relu = 1) over
 *                                 the table's features; ld_cur >= 1
 *   edit_col int32 [E] / [E_total] or NULL   the column of `cur` that table entry e reads (rows form: e counts through the
 *                                 concatenated arrays); NULL: entry e reads column e.  Clamped into [0, ld_cur) before use.
 *   gain f32 [T][k] or NULL       per output slot: 1.0 for a slot that came from an unedited list entry, the table's gain
 *                                 (above) for a slot that came from a table entry
 * Asynchronous on `stream`; allocates nothing, never synchronises, needs no workspace.  MSAE_EINVAL in addition: cur null,
 * ld_cur < 1.
 * Contract:
 *   1. The output is the canonical top-k (value descending, index ascending) of L' -- bit-identical to msae_topk_f32 on
 *      the edited dense latents for finite pre-activations.  A result <= 0 follows point 3 of "set-valued hook edits": it
 *      ranks by the key rule and a negative one is never selected, so a negative ADD or SCALE ablates the feature wherever
 *      it drives the value to 0 or below.
 *   2. A table holding only SET / ZERO entries gives msae_edit_topk_f32's / msae_edit_topk_rows_f32's bits; `cur` is then
 *      not read (gain: 0 at the table's slots, 1 elsewhere).
 *   3. Only the first k + E (k + E_g) entries of a row are read.  Of `cur`, only row t's columns named by the
 *      value-dependent entries of token t's own table are read: other columns, and the padding up to ld_cur, may hold
 *      anything.
 *   4. Nothing is indexed by a list entry's feature.  No device id, offset or column is trusted: a hostile one can give a
 *      wrong row for that token, not an out-of-bounds access.
 *   5. A kind outside [0, 5] reads as SET, as the unvalued kernels read any kind but ZERO.
 *   6. Rows form: an unedited token (group id outside [0, G), or an empty group) copies its first k entries, gain 1.
 *   7. Layout, LDS and launch shapes are the unvalued kernels': the same three kernels instantiated with VALUED = true. */
int msae_edit_topk_valued_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *edit_feat,
                              const float *edit_val, const int32_t *edit_kind, int E, int N, int k, const float *cur,
                              int ld_cur, const int32_t *edit_col, float *vals, int32_t *idx, float *gain, void *stream);
int msae_edit_topk_valued_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk, const int32_t *edit_feat,
                                  const float *edit_val, const int32_t *edit_kind, int E, int N, int k, const float *cur,
                                  int ld_cur, const int32_t *edit_col, float *vals, int64_t *idx, float *gain, void *stream);
int msae_edit_topk_rows_valued_f32(const float *vals_in, const int32_t *idx_in, int T, int kk, const int32_t *group_of,
                                   const int32_t *group_off, int G, const int32_t *edit_feat, const float *edit_val,
                                   const int32_t *edit_kind, int E_total, int E_max, int N, int k, const float *cur,
                                   int ld_cur, const int32_t *edit_col, float *vals, int32_t *idx, uint8_t *edited,
                                   float *gain, void *stream);
int msae_edit_topk_rows_valued_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int kk, const int32_t *group_of,
                                       const int32_t *group_off, int G, const int32_t *edit_feat, const float *edit_val,
                                       const int32_t *edit_kind, int E_total, int E_max, int N, int k, const float *cur,
                                       int ld_cur, const int32_t *edit_col, float *vals, int64_t *idx, uint8_t *edited,
                                       float *gain, void *stream);

/* ---- error-preserving interventions (Sae.intervene) ------------------------------------------------
 * out = x + (decode(edited list) - decode(plain list)): the hidden state keeps the SAE's reconstruction error and moves by
 * the decoded EDIT alone.  Entries the two lists share cancel, so only the entries that differ are gathered.
 *   x [T][d]                          the hidden states, x_dtype MSAE_F32 / MSAE_BF16 / MSAE_F16
 *   plain_vals / plain_idx [T][ld_plain]   P: the canonical top-k of the UNEDITED latents in the first k columns of each row
 *                                     (the over-fetched encode's output is passed as it is, ld_plain = kk)
 *   edit_vals / edit_idx [T][ld_edit]      Q: the edited list (msae_edit_topk_f32 / msae_edit_topk_rows_f32), first k columns
 *   W_dec f32 [N][d]
 *   out [T][d]                        x's dtype; may be x itself (no other overlap)
 *   status int32 [1] or NULL          bit 0 is ORed in when an entry's feature lies outside [0, N), as msae_decode_f32 does
 * Asynchronous on `stream`; allocates nothing, needs no workspace, never synchronises.  MSAE_EINVAL: a null pointer
 * (`status` may be null), k < 1, k > 4096, ld_plain < k, ld_edit < k, T < 0, N < 1, d < 1, a bad dtype code.  T == 0 returns 0.
 * Contract, per token t (nothing depends on T or on the other tokens):
 *   1. Surviving entries.  An entry (value, feature) of one list SURVIVES when its value is not +-0 and the other list
 *      holds no entry with the same feature and the bit-identical value (values compared as 32-bit patterns).  A feature in
 *      both lists with different values survives twice, once from each list.
 *   2. Difference sequence D_t: the surviving entries of Q in slot order, each with coefficient +value, then the surviving
 *      entries of P in slot order, each with coefficient -value.
 *   3. delta[t][c] is the f32 chain acc = fmaf(coef_j, W_dec[f_j][c], acc) over D_t in that order, from acc = +0.
 *   4. out[t][c] = convert(f32(x[t][c]) + delta[t][c]): one f32 add, one round-to-nearest-even conversion to x's dtype
 *      (a NaN sum stays a NaN).  b_dec is in both reconstructions and cancels: it is not an argument.
 *   5. Empty D_t: out[t][:] holds x[t][:]'s own bits -- nothing is added, so -0 and NaN payloads pass through; with
 *      out == x the row is not touched at all.
 *   6. A surviving entry whose feature lies outside [0, N) is skipped (and flagged in `status`, like every out-of-range
 *      entry of either list).  No memory is indexed by a feature that was not range-checked: a hostile list -- repeated
 *      features, any order -- follows the same survival rule; it can give a wrong row, not an out-of-bounds access.
 *   7. f32(x) + (msae_decode_f32(Q) - msae_decode_f32(P)) is the MEANING of this definition, not its bits: the two differ by
 *      the rounding of the cancelled entries.
 * Layout: one workgroup per (token, slab of 1024 columns), both lists and D_t in LDS (32 k bytes; the two lists alone are
 * 16 k <= 64 KiB); 16-byte loads per lane when d % 4 == 0 and W_dec, x, out are aligned to 4 elements, one column per lane
 * otherwise. */
int msae_delta_decode_f32(const void *x, int x_dtype, const float *plain_vals, const int32_t *plain_idx, int ld_plain,
                          const float *edit_vals, const int32_t *edit_idx, int ld_edit, const float *W_dec, int T, int k,
                          int N, int d, void *out, int32_t *status, void *stream);
/* the same reading 64-bit indices (msae_encode_topk_i64's and msae_edit_topk_i64_f32's output type) */
int msae_delta_decode_i64_f32(const void *x, int x_dtype, const float *plain_vals, const int64_t *plain_idx, int ld_plain,
                              const float *edit_vals, const int64_t *edit_idx, int ld_edit, const float *W_dec, int T,
                              int k, int N, int d, void *out, int32_t *status, void *stream);

/* ---- reconstruction error against sparsity (Sae.recon_error, msae.features.ReconStats) ------------
 * The canonical top-k list is value descending, index ascending, so its first kappa columns are the top-kappa list, and
 * msae_decode_f32 is a slot-ordered fma chain from +0: ONE pass over the k decoder rows that stops at C checkpoints gives the
 * error of the kappa-sparse reconstruction at every checkpoint.  x is read once and no [T][d] reconstruction is written.
 *   x [T][d]                          the hidden states, x_dtype MSAE_F32 / MSAE_BF16 / MSAE_F16
 *   vals / idx [T][ld]                the list in the first k columns of each row (an over-fetched list is passed as it
 *                                     is, ld = kk)
 *   W_dec f32 [N][d], b_dec f32 [d]   both required
 *   ks int32 [C]                      the checkpoints, a HOST array: copied into the launch arguments during the call
 *   mom f32 [T][C][3]                 (|e|^2, x . r, |r|^2) per token and checkpoint
 *   xx f32 [T]                        |x|^2 per token
 *   status int32 [1] or NULL          bit 0 is ORed in when an entry's feature lies outside [0, N), as msae_decode_f32 does
 * Asynchronous on `stream`; allocates nothing, needs no workspace, never synchronises.  MSAE_EINVAL: a null pointer
 * (`status` may be null), k < 1, k > 4096, ld < k, T < 0, N < 1, d < 1, C outside [1, MSAE_RECON_MAX_CHECKPOINTS], ks not
 * strictly ascending or outside [0, k], a bad dtype code.  T == 0 returns 0.
 * Contract, per token t (nothing depends on T or on the other tokens):
 *   1. Checkpoints.  0 <= ks[0] < ks[1] < ... < ks[C-1] <= k.  kappa = 0 is the reconstruction by b_dec alone.
 *   2. Reconstruction.  r_kappa[c] = (the f32 chain acc = fmaf(v_j, W_dec[f_j][c], acc) over the slots j < kappa in slot
 *      order, from acc = +0) + b_dec[c], one f32 add behind the chain.  An entry with v_j == +-0 is skipped; an entry whose
 *      f_j lies outside [0, N) is skipped and flagged in `status`.  This is msae_decode_f32's own rule, so r_kappa is
 *      BIT-IDENTICAL to msae_decode_f32 over the first kappa columns.  No memory is indexed by a feature that was not
 *      range-checked: a hostile list -- repeated features, any order -- follows the same rule.
 *   3. Error.  e_kappa[c] = r_kappa[c] - f32(x[t][c]), one f32 subtract (the up-cast of bf16 / f16 is exact).
 *   4. Moments.  mom[t][i] = (sum_c e^2, sum_c x r, sum_c r^2) at ks[i] and xx[t] = sum_c x^2, f32 sums over the d columns
 *      of products formed by fmaf, in this order: a lane owns 4 consecutive columns (1 on the scalar path) of a slab of 1024
 *      (256) columns and chains them in ascending order from +0; the 64 lanes of a wave are added by an xor butterfly,
 *      partner distance 32, 16, ..., 1 (a lane past d holds +0); the four waves as ((w0 + w1) + w2) + w3; the slabs in
 *      ascending order from +0.  The order depends on d and on which load path ran, never on T, the grid or timing: no
 *      floating-point atomics.  Token t's outputs are the same bits alone or in any batch, in any call.
 *   5. A non-finite x[t][c] makes token t's moments non-finite and touches no other token.
 * Layout: one workgroup of 256 threads per token, the list in LDS (8 k bytes); 16-byte loads per lane when d % 4 == 0 and
 * W_dec, b_dec, x are aligned to 4 elements, one column per lane otherwise. */
#define MSAE_RECON_MAX_CHECKPOINTS 16
int msae_recon_curve_f32(const void *x, int x_dtype, const float *vals, const int32_t *idx, int ld, const float *W_dec,
                         const float *b_dec, int T, int k, int N, int d, const int32_t *ks, int C, float *mom, float *xx,
                         int32_t *status, void *stream);
/* the same reading 64-bit indices (msae_encode_topk_i64's output type) */
int msae_recon_curve_i64_f32(const void *x, int x_dtype, const float *vals, const int64_t *idx, int ld, const float *W_dec,
                             const float *b_dec, int T, int k, int N, int d, const int32_t *ks, int C, float *mom, float *xx,
                             int32_t *status, void *stream);

/* ---- support refit (Sae.refit, msae.features.ReconStats(refit=True)) -------------------------------
 * Keep the support the encoder chose -- the first s slots of a token's canonical list -- and refit its coefficients by
 * least squares against the fixed decoder: min_c |y - D^T c|^2, y = x - b_dec, D = the listed rows of W_dec.  err_enc -
 * err_fit is what the encoder loses by its magnitudes alone (the amortisation gap); err_fit is what the dictionary cannot
 * express on that support.  The list is value descending, so the support of the top-kappa list is the first kappa slots;
 * the Gram matrix of a prefix is a leading block of G, its Cholesky factor a leading block of L, and the forward solve
 * nests too: yy - sum_{j < kappa} gain[j] is the optimal squared error at EVERY kappa <= s from one factorisation.
 *   x [T][d]                          the hidden states, x_dtype MSAE_F32 / MSAE_BF16 / MSAE_F16
 *   vals / idx [T][ld]                the list in the first s columns of each row (ld >= s: a longer list is refit on its
 *                                     first s slots in place)
 *   W_dec f32 [N][d], b_dec f32 [d]   both required
 *   coef f32 [T][s]                   the least-squares coefficients on the full live support, signs as they come
 *   gain f32 [T][s]                   z_j^2: what slot j takes off the optimal error when it joins the slots before it
 *   err_fit, err_enc, yy f32 [T]      |y - D^T coef|^2, |y - D^T vals|^2, |y|^2
 *   n_dependent int32 [T]             live slots dropped as linearly dependent on the slots before them
 *   status int32 [1] or NULL          bit 0 is ORed in when a slot's feature lies outside [0, N), as msae_recon_curve_f32 does
 * Asynchronous on `stream`; allocates nothing, needs no workspace, never synchronises.  MSAE_EINVAL: a null pointer
 * (`status` may be null), s < 1, s > MSAE_REFIT_MAX_S, ld < s, T < 0, N < 1, d < 1, d > 2^22, a bad dtype code.  T == 0
 * returns 0.
 * Contract, per token t (nothing depends on T or on the other tokens); u = 2^-24, gamma_n = n u / (1 - n u):
 *   1. Support.  Slot j is live iff vals[j] != 0 and 0 <= idx[j] < N; an index outside sets `status`.  A dead slot has
 *      coef = gain = 0 and keeps its place; it is not counted in n_dependent.  Its row of D is zero below.
 *   2. y[c] = f32(x[t][c]) - b_dec[c], one f32 subtract.
 *   3. Gram.  G = D D^T (lower triangle), h = D y: each entry is the sum of four f32 fma chains, one per c mod 128 in
 *      [0, 32), [32, 64), [64, 96), [96, 128), each over its columns in ascending order from +0 (two columns per
 *      v_mfma_f32_32x32x2_f32, fma(a_c1, b_c1, fma(a_c0, b_c0, acc))), added as ((p0 + p1) + p2) + p3.  yy: a lane owns the
 *      columns with (c mod 128) / 4 == lane, lane < 32, and chains them in ascending order from +0; the 64 lanes (32 of them
 *      +0) are added by an xor butterfly, partner distance 32, 16, ..., 1.  Neither order depends on the load path.
 *   4. Cholesky, G = L L^T in slot order, right-looking: at column j the pivot p is G_jj after the updates of the columns
 *      before it.  p <= tau G_jj (G_jj as formed in step 3), tau = f32(2 gamma_{d+s}): the slot is dependent -- counted,
 *      coef = gain = 0, its row and column skipped from then on.  (gamma_{d+s} bounds the relative error of a Gram entry
 *      plus its at most s pivot updates against sum |terms| <= 2 G_jj: a pivot below tau G_jj is not told from zero.  A
 *      repeated index leaves |p| <= 3 u G_jj; a row at angle theta to the span before it leaves sin^2 theta G_jj.)
 *      Otherwise L_jj = sqrt(p), L_ij = G_ij / L_jj, G_im = fma(-L_ij, L_mj, G_im) for j < m <= i: every entry takes its
 *      updates in ascending j.  sqrt and / are correctly rounded.
 *   5. Forward solve.  h rides as row s of the same factorisation: z_j = h_j after the same updates, / L_jj.
 *      gain[j] = z_j * z_j.
 *   6. Back solve over the slots kept, j descending: coef_j = z_j / L_jj, then z_m = fma(-L_jm, coef_j, z_m) for m < j.
 *   7. Second walk.  fit[c] and enc[c] are msae_recon_curve_f32's slot-ordered chains over the s slots (from +0, a zero
 *      coefficient skipped) with coef and with vals (0 for a dead slot; a dependent slot keeps its value);
 *      err_fit = sum_c (y[c] - fit[c])^2 and err_enc likewise, in the order of msae_recon_curve_f32's moments (step 4 there).
 *      Neither is taken from yy - sum gain: a wrong solve cannot hide behind its own algebra.
 * No floating-point atomics: token t's outputs are the same bits alone or in any batch, in any call.
 * Layout: one workgroup of 256 threads per token; 128-column slabs of the rows through LDS, the matrix (at most 65 x 65)
 * factored in LDS.  16-byte loads when d % 4 == 0 and W_dec, b_dec, x are aligned to 4 elements, element loads otherwise. */
#define MSAE_REFIT_MAX_S 64
int msae_support_refit_f32(const void *x, int x_dtype, const float *vals, const int32_t *idx, int ld, const float *W_dec,
                           const float *b_dec, int T, int s, int N, int d, float *coef, float *gain, float *err_fit,
                           float *err_enc, float *yy, int32_t *n_dependent, int32_t *status, void *stream);
/* the same reading 64-bit indices (msae_encode_topk_i64's output type) */
int msae_support_refit_i64_f32(const void *x, int x_dtype, const float *vals, const int64_t *idx, int ld, const float *W_dec,
                               const float *b_dec, int T, int s, int N, int d, float *coef, float *gain, float *err_fit,
                               float *err_enc, float *yy, int32_t *n_dependent, int32_t *status, void *stream);

/* ---- batch-level selection: capped BatchTopK, threshold filter, length-aware decode -------------
 * BatchTopK keeps the T*k largest pre-activations of a whole batch instead of k per token; inference replaces the batch's
 * threshold by a learned one.  Here it is defined on LISTS, so it is exact by construction and needs no fallback and no
 * host read.  T tokens, a target k, a cap C with k <= C:
 *   1. L_t = the canonical top-C list of token t (msae_encode_topk with k = C: value descending, index ascending).
 *   2. P = the multiset of list entries with v > 0 (false for NaN, -0.0 and negatives; +inf is the largest value), K = T*k.
 *      theta = the K-th largest value of P; |P| < K: theta = min P; P empty: theta = +inf.
 *   3. An entry is kept iff v > 0 && v >= theta: ALL ties at theta are kept, so the result does not depend on the order of
 *      the tokens, and sum(len) >= min(K, |P|) with equality unless floats tie at theta.
 *   4. On a value-descending row the kept entries are a prefix; len[t] is its length.  Dropped slots come out with
 *      activation +0.0 and their own index (the indices of a row stay valid and distinct).
 *   5. saturated[t] = (len[t] == C): the token may have had more latents at or above theta than the cap admits.  With no
 *      saturated row the result equals uncapped BatchTopK over the dense [T, N] latents (an entry outside a list is at most
 *      the list's last entry, which is below theta: no outside entry can enter the top K, and theta is the dense one).
 *   6. Thresholded inference: the same keep rule with a given theta; with a per-feature table theta_feat[N] an entry is kept
 *      iff its index lies in [0, N) && v > 0 && v >= theta_feat[idx] (the table is never read out of bounds).
 *
 * msae_batch_kth_f32: step 2.  vals [T][ld >= C] f32 (the [:, :C] view of a wider list is read in place), K >= 1;
 *   *theta (f32) and *n_pos (int32, optional: |P|) are DEVICE scalars.  An exact radix select on the float bits (a positive
 *   float's bits order like its value): four 8-bit passes over all T*C entries, one launch per pass, integer histograms
 *   only -- per-workgroup LDS bins, one integer atomic per bin and workgroup -- so the result is bit-reproducible.  No data
 *   is handed between the workgroups of a launch and nothing waits on a flag: every workgroup of a launch redoes the
 *   earlier passes' digit picks from their complete 256-bin histograms.  Envelope: T, C >= 1, T*C <= 2^24 (else MSAE_EINVAL;
 *   the helper returns 0).  ws: msae_batch_kth_ws_bytes(T, C) bytes under the workspace contract above (the call zeroes the
 *   histograms itself; a short or missing workspace is MSAE_EWS before any launch).
 * msae_list_filter_f32 / _i64_f32: steps 3-6.  vals_in / idx_in [T][ld >= C], *theta a DEVICE scalar, theta_feat f32 [N] or
 *   NULL (then N is not looked at and indices are not checked); vals_out / idx_out [T][C] (not the inputs), len int32 [T].
 *   Every row is partitioned STABLY: the kept entries first in list order, then the dropped ones in theirs with activation
 *   +0.0 -- on a value-descending row in scalar mode that is the row itself with its tail zeroed.  *n_saturated (int32
 *   device counter, optional) is ADDED to by the number of rows with v_last > 0 && v_last >= *theta, v_last the row's last
 *   INPUT entry: in scalar mode on a descending row that is len == C; in table mode the host passes theta_feat's minimum as
 *   *theta (the floor below which no feature keeps anything).  1 <= C <= 4096 (else MSAE_EINVAL); T == 0 returns 0.  One wave
 *   per token for C <= 256 (ballot compaction in registers), one workgroup per token above.  No workspace.
 * msae_decode_prefix_f32 / _i64_f32: msae_decode_f32 over the first clamp(len[a], 0, k) entries of every row.  The slots
 *   behind that are not read at all -- neither index, nor activation, nor decoder row (they may hold anything) -- so the
 *   cost follows sum(len), not A*k.  Same column slabs and the same fma chain in j order: on a filtered list the output is
 *   bit-identical to msae_decode_f32's, which lets a zero activation contribute nothing. */
size_t msae_batch_kth_ws_bytes(int T, int C);
int msae_batch_kth_f32(const float *vals, int T, int C, int ld, long long K, float *theta, int32_t *n_pos, void *ws,
                       size_t ws_bytes, void *stream);
int msae_list_filter_f32(const float *vals_in, const int32_t *idx_in, int T, int C, int ld, const float *theta,
                         const float *theta_feat, int N, float *vals_out, int32_t *idx_out, int32_t *len,
                         int32_t *n_saturated, void *stream);
int msae_list_filter_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int C, int ld, const float *theta,
                             const float *theta_feat, int N, float *vals_out, int64_t *idx_out, int32_t *len,
                             int32_t *n_saturated, void *stream);
int msae_decode_prefix_f32(const int32_t *idx, const float *acts, const int32_t *len, const float *W_dec,
                           const float *b_dec, int A, int k, int N, int d, float *out, int32_t *status, void *stream);
int msae_decode_prefix_i64_f32(const int64_t *idx, const float *acts, const int32_t *len, const float *W_dec,
                               const float *b_dec, int A, int k, int N, int d, float *out, int32_t *status, void *stream);

/* ---- JumpReLU selection: learned per-feature thresholds on top-C lists (ops.jump_select) -----------
 * z = a * H(a - theta_f) with a threshold theta_f > 0 per feature, trained through straight-through estimators with the
 * rectangle kernel K(u) = [|u| < 1/2] of bandwidth eps.  Like the batch-level selection it is defined on LISTS.
 *   Inputs.  vals_in / idx_in [T][ld >= C]: a canonical top-C list; theta f32 [N]; eps > 0; h = 0.5f * eps, rounded once on
 *     the host and passed as f32.  For an entry with value a and index f every operation is a single f32 operation:
 *       valid  0 <= f < N && a > 0            (false for NaN, -0.0 and negatives; the table is never read out of bounds)
 *       kept   valid && a >= theta_f          (msae_list_filter_f32's table rule: inference and training agree)
 *       near   valid && !kept && theta_f - a < h
 *       band   valid && fabsf(a - theta_f) < h   (the kept entries within h of theta_f, and every near entry)
 *   Partition.  Every row is partitioned STABLY into three parts, each in list order: kept, near, rest.  The dropped slots
 *     (near and rest) come out with activation +0.0 and their own index.  len[t] = the number kept, reach[t] = kept + near,
 *     src[t][p] = the input slot of output slot p (uint8: C <= 256).
 *   Counters.  *l0 (int64 device counter) is ADDED to by sum_t len[t]; *n_saturated (int32 device counter) by the number of
 *     rows with v_last > 0 && v_last >= *floor, v_last the row's last INPUT entry and *floor a device f32 scalar -- the host
 *     passes min(theta) - h.  With no saturated row every (t, f) outside a list lies below theta_f - h for every f, so the
 *     kept set and the band equal those of the dense [T, N] latents.
 *   Pseudo-derivatives.  dz/da = kept; dz/dtheta_f = -(theta_f / eps) * band; dH/dtheta_f = -(1 / eps) * band.
 *   Backward.  g [T][C] = the gradient of vals_out, *s (device f32 scalar) = the gradient of the float l0.
 *       g_in[t][src[t][p]] = p < len[t] ? g[t][p] : +0.0                       (a routing copy)
 *       g_theta[f] = sum over the band entries of feature f of c,  c = -fmaf(theta_f, g[t][p], s) / eps
 *     c is two f32 operations, one fused multiply-add and one division (the negation is exact): its error is relative to |c|
 *     even where theta_f g and s cancel, which a separately rounded product would not give.  Every feature is written; one
 *     without band entries gets +0.0.  Order of the sum, a function of the inputs alone: the feature's band entries e_0, e_1,
 *     ... in ascending (t, input slot) order; lane l of a wave adds e_l, e_{l + 64}, ... in that order starting from +0.0, and
 *     the 64 partial sums are joined by the xor butterfly with partner distance 32, 16, ..., 1 (v += shfl_xor(v, off)).  No
 *     floating-point atomics: two runs give the same bits.
 * msae_jump_filter_f32 / _i64_f32: one wave per token, the row in registers, three ballot compactions; one integer atomic per
 *   workgroup and counter.  1 <= C <= 256, ld >= C, N >= 1, h > 0 (else MSAE_EINVAL; a null pointer too -- l0 and n_saturated
 *   may be null); T == 0 returns 0.  vals_out / idx_out [T][C] are not the inputs.  No workspace.
 * msae_jump_bwd_f32 / _i64_f32: vals_in / idx_in / theta / h as the filter got them, src / len / reach as it wrote them.
 *   Two passes of one wave per token (routing and per-feature counts; fill), a one-workgroup scan, one wave per feature that
 *   sorts its run by (t, slot) and sums it.  ws: msae_jump_bwd_ws_bytes(T, C, N) bytes under the workspace contract above
 *   (3 (N + 1) ints and T * C 8-byte entries; 0 for a shape the entry refuses).  Envelope: T >= 1, 1 <= C <= 256,
 *   1 <= N < 2^30, T * C < 2^31, eps > 0, h > 0.  T == 0 writes +0.0 to every g_theta[f] and needs no workspace. */
int msae_jump_filter_f32(const float *vals_in, const int32_t *idx_in, int T, int C, int ld, const float *theta, int N, float h,
                         const float *floor, float *vals_out, int32_t *idx_out, int32_t *len, int32_t *reach, uint8_t *src,
                         int64_t *l0, int32_t *n_saturated, void *stream);
int msae_jump_filter_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int C, int ld, const float *theta, int N,
                             float h, const float *floor, float *vals_out, int64_t *idx_out, int32_t *len, int32_t *reach,
                             uint8_t *src, int64_t *l0, int32_t *n_saturated, void *stream);
size_t msae_jump_bwd_ws_bytes(int T, int C, int N);
int msae_jump_bwd_f32(const float *vals_in, const int32_t *idx_in, int T, int C, int ld, const float *theta, int N, float h,
                      float eps, const uint8_t *src, const int32_t *len, const int32_t *reach, const float *g, const float *s,
                      float *g_in, float *g_theta, void *ws, size_t ws_bytes, void *stream);
int msae_jump_bwd_i64_f32(const float *vals_in, const int64_t *idx_in, int T, int C, int ld, const float *theta, int N, float h,
                          float eps, const uint8_t *src, const int32_t *len, const int32_t *reach, const float *g,
                          const float *s, float *g_in, float *g_theta, void *ws, size_t ws_bytes, void *stream);

/* ---- nested decode: Matryoshka prefixes of the dictionary (ops.nested_reconstruct) ----------------
 * A Matryoshka SAE asks the first m_0 features to reconstruct x alone, the first m_1 too, ... up to m_{G-1} = N, under ONE
 * sparse selection over all N features.  Forward: every prefix's reconstruction error from one pass over a token's decoder
 * rows.  Backward: the per-prefix loss gradients folded into G planes, and the two decoder backward kernels reading the
 * plane of each feature's group.
 *   Bounds and groups.  m[0] < m[1] < ... < m[G-1] = N, 1 <= G <= MSAE_NESTED_MAX_GROUPS, m[0] >= 1.  group(n) = the number
 *     of g with m[g] <= n: 0 .. G-1 for 0 <= n < N.
 *   Live entries.  Token t has the list (v_j, i_j), j < k; with `lengths`, j < clamp(len[t], 0, k) and the slots behind
 *     are not read.  An entry is live iff 0 <= i_j < N and v_j != 0.  An out-of-range index ORs 1 into `status`, as
 *     msae_decode_f32 does, and the entry is dead.
 *   Group-major order.  The live entries ordered by (group(i_j), j): a stable partition of the list by group.
 *   The chain, per column c.  acc = +0; for the live entries in group-major order acc = fmaf(v, W_dec[i][c], acc); after the
 *     last entry of group g -- at once if the group has none -- r_g[c] = acc + b_dec[c] and e_g[c] = r_g[c] - (float)x[t][c].
 *   Outputs.  out[t] = r_{G-1}.  E[g][t][c] = e_g[c], f32 [G][T][d]; E may be NULL, then nothing is written.
 *     sq[t][g] = sum_c e_g[c]^2 in msae_recon_curve_f32's order of a moment (step 4 there): lane fmaf chain over its
 *     ascending columns from +0, xor butterfly over the wave, ((w0 + w1) + w2) + w3, slabs in ascending order.  No
 *     floating-point atomics: token t's outputs are the same bits alone or in any batch.
 *   Consequences.  G = 1: out is bit-identical to msae_decode_f32 on the same list.  r_g is bit-identical to msae_decode_f32
 *     on the group-major list with the entries of the groups above g set to 0.
 * msae_nested_decode_f32 / _i64_f32: x [T][d] (MSAE_F32 / MSAE_BF16 / MSAE_F16), vals / idx [T][ld >= k], lengths int32 [T]
 *   or NULL, bounds a HOST int32 [G] (copied into the launch arguments), W_dec f32 [N][d], b_dec f32 [d], out f32 [T][d],
 *   E f32 [G][T][d] or NULL, sq f32 [T][G], status int32 [1] or NULL.  One workgroup of 256 threads per token; the live
 *   entries in LDS (9 k bytes), partitioned by one workgroup scan per group; slabs of 1024 columns (256, one column per lane,
 *   when d % 4 != 0 or a pointer is not aligned to 4 elements).  MSAE_EINVAL before any launch: a null pointer (lengths, E,
 *   status may be null), k < 1, k > 4096, ld < k, T < 0, N < 1, d < 1, G outside [1, MSAE_NESTED_MAX_GROUPS], bounds not
 *   strictly ascending, below 1 or not ending at N, a bad dtype code.  T == 0 returns 0.  No workspace, never synchronises.
 * msae_nested_combine_f32: elementwise and in place on E (16-byte accesses when T*d % 4 == 0 and the pointers are aligned --
 *   the planes lie T*d floats apart --, one element per lane otherwise; the same bits either way).  s = grad_full[t][c] (+0 when grad_full is NULL); for g = G-1
 *   down to 0: s = fmaf(coef[g], E[g][t][c], s), S[g][t][c] = s (stored over E[g]).  coef: a DEVICE f32 [G].  With
 *   coef[g] = 2 dL/d(sum_t sq[t][g]) and grad_full = dL/d(out), S[g] is the gradient that reaches r_g and everything the
 *   chain added before it: the gradient of every decoder row and activation of group g.
 * msae_decode_bwd_acts_grouped_f32 / msae_decode_bwd_wdec_grouped_f32: msae_decode_bwd_acts_f32 / msae_decode_bwd_wdec_f32
 *   -- the same kernels, chains, reductions, pair order, row_sumsq / row_act_sum outputs and workspace
 *   (msae_decode_bwd_wdec_ws_bytes(A, k, N)) -- with the gradient row of a pair or feature row taken from plane group(i) of
 *   grad_planes f32 [G][A][d]:
 *     g_acts[t][j] = S[group(i_j)][t] . W_dec[i_j]                          (0 and flagged for an out-of-range index)
 *     g_W[n]       = sum over the pairs with i = n and v != 0, in ascending pair order, of v * S[group(n)][t]
 *   bounds: a DEVICE int32 [G] (the caller passes N = bounds[G-1]; a group count past G-1 is clamped, so no bounds array
 *   can index outside the planes).  The choice of plane is uniform over a wave. */
#define MSAE_NESTED_MAX_GROUPS 8
int msae_nested_decode_f32(const void *x, int x_dtype, const float *vals, const int32_t *idx, int ld, const int32_t *lengths,
                           const int32_t *bounds, int G, const float *W_dec, const float *b_dec, int T, int k, int N, int d,
                           float *out, float *E, float *sq, int32_t *status, void *stream);
int msae_nested_decode_i64_f32(const void *x, int x_dtype, const float *vals, const int64_t *idx, int ld,
                               const int32_t *lengths, const int32_t *bounds, int G, const float *W_dec, const float *b_dec,
                               int T, int k, int N, int d, float *out, float *E, float *sq, int32_t *status, void *stream);
int msae_nested_combine_f32(float *E, const float *coef, const float *grad_full, int T, int d, int G, void *stream);
int msae_decode_bwd_acts_grouped_f32(const int32_t *idx, const float *grad_planes, const int32_t *bounds, int G,
                                     const float *W_dec, int A, int k, int N, int d, float *g_acts, int32_t *status,
                                     void *stream);
int msae_decode_bwd_wdec_grouped_f32(const int32_t *idx, const float *acts, const float *grad_planes, const int32_t *bounds,
                                     int G, int A, int k, int N, int d, float *g_W_dec, float *row_sumsq, float *row_act_sum,
                                     int32_t *status, void *ws, size_t ws_bytes, void *stream);

/* ---- merge of per-shard results (feature-sharded encode; no reference counterpart) ----
 * gathered: int32 [G][2][T][kl], the all-gather of each rank's packed block [2][T][kl]
 * (plane 0 = f32 activation bits, plane 1 = GLOBAL feature index).  Writes the canonical top-k of
 * the G*kl candidates per token; flagged[t] (optional) = 1 when kl < k and some shard's last
 * candidate ranks inside the merged top-k (that shard may hold more members than it sent). */
int msae_merge_topk(const int32_t *gathered, int T, int G, int kl, int k, float *vals, int32_t *idx,
                    int32_t *flagged, void *stream);
/* rows[0 .. n) = the t with flags[t] != 0 in ascending order, *n_rows = n (device pointers; one small kernel): the
 * redo list msae_encode_topk_rows takes, derived identically on every rank from the same gathered data. */
int msae_compact_flags(const int32_t *flags, int T, int32_t *rows, int32_t *n_rows, void *stream);
/* msae_merge_topk for the tokens with mask[t] != 0 only, in place: the others' vals / idx rows are left as they are
 * (second round: the redone tokens' full local lists, kl = k, replace round 1's merge).  idx or idx64 may be NULL. */
int msae_merge_topk_masked(const int32_t *gathered, int T, int G, int kl, int k, const int32_t *mask,
                           float *vals, int32_t *idx, int64_t *idx64, void *stream);

/* ---- debug entry: the threshold select of the fused encoder on its own (csrc/topk.hip) ----
 * out[t] = the float whose order key is the r-th largest order key of rows[t][0 .. S) with its low 14 bits cleared (the
 * r-th largest rounded down by < 0.2 %: at least r values of the row are at or above it).  With cnt != NULL and out[t] > 0
 * every value of the row ABOVE out[t] is appended to the row's list: cnt[t] advances by their number in one atomic add
 * and cand[t * cap + slot] = (order key << 32) | (0x7FFFFFFF - (j * stride + off)) for column j, slots at or past cap
 * dropped; the order inside a list is unspecified.  rows 16-byte aligned, ld % 4 == 0, ld >= S, S % 256 == 0 and
 * S <= 8192 or S % 1024 == 0; other shapes return MSAE_ENOTIMPL.  MSAE_KTH_STREAM=0 in the environment (read at every
 * call) keeps the register-resident kernel where the streaming one would run; both return the same values. */
int msae_kth_value_f32(const float *rows, int T, int S, int ld, int r, float *out, int32_t *cnt,
                       unsigned long long *cand, int cap, int stride, int off, void *stream);

/* ---- parameter-sized passes of one optimisation step (training) ----
 * msae_unit_norm_rows_f32: W[r][:] /= ||W[r][:]||_2 + eps, in place
 *                          (Sae.set_decoder_norm_to_unit_norm, sae_auto_interp/sae/sae.py:249-255).
 * msae_grad_sumsq_f32:     *accum += sum(g^2) (device scalar; the total-norm half of
 *                          clip_grad_norm_, train/sae/sae/trainer.py:390).
 * msae_adam_rows_f32:      one pass over a [rows][d] parameter: g = G * min(1, max_norm /
 *                          (sqrt(*total_sumsq) + 1e-6)) (total_sumsq NULL: no clipping); if `project`,
 *                          g -= <g, W[r]> W[r] per row (Sae.remove_gradient_parallel_to_decoder_
 *                          directions, sae.py:257-271); then Adam (torch.optim.Adam arithmetic, no
 *                          weight decay, trainer.py:139-146,395) on W, M, V in place, `step` >= 1.
 *                          G is read only. */
int msae_unit_norm_rows_f32(float *W, int N, int d, float eps, void *stream);
/* out[d] = scale * sum_n s[n] * W[n][:] in a fixed order (rows with s[n] == 0 are not read): the b_dec gradient of the sparse
 * encoder backward, -(s^T W_enc) with s = row_act_sum, as ONE streaming read of W_enc (the reference back-propagates a dense
 * [T, N] gradient through nn.Linear, sae.py:172-177; a k-row gather per token is the sparse alternative).  d % 4 == 0. */
size_t msae_weighted_row_sum_ws_bytes(int N, int d);
int msae_weighted_row_sum_f32(const float *W, const float *s, int N, int d, float scale, float *out, void *ws,
                              size_t ws_bytes, void *stream);
/* *accum += v[0] + ... + v[n - 1], summed in a fixed order (bit-reproducible): the total of row_sumsq. */
int msae_sum_f32(const float *v, size_t n, float *accum, void *stream);
/* msae_adam_rows_f32 with the NEXT step's passes over the same matrix folded into the one sweep:
 *   renorm_eps >= 0  rows of W are divided by their norm + renorm_eps after the update -- the trainer's
 *                    set_decoder_norm_to_unit_norm at the top of the next step (sae.py:249-255, trainer.py:352), bit for
 *                    bit what msae_unit_norm_rows_f32 would produce from the updated matrix; < 0: off
 *   prepared != NULL W is the ENCODER weight [N = rows][d]: its coarse-pass operands for the next encode of T_next
 *                    tokens (T_next <= 0: any batch size) are rebuilt from the updated rows, bit for bit what
 *                    msae_encoder_refresh_for / msae_encoder_refresh would build (opts: the coarse mode)
 * Both save a read (+ write) of the 2 GiB matrix per step.  Shapes the fused kernel does not take (d % 4 != 0, d > 8192)
 * run the separate passes. */
int msae_adam_rows_fused_f32(float *W, const float *G, float *M, float *V, int rows, int d,
                             const float *total_sumsq, float max_norm, int project, float lr, float beta1,
                             float beta2, float eps, int step, float renorm_eps, void *prepared, int T_next,
                             const msae_options *opts, void *stream);
int msae_grad_sumsq_f32(const float *g, size_t n, float *accum, void *stream);
int msae_adam_rows_f32(float *W, const float *G, float *M, float *V, int rows, int d,
                       const float *total_sumsq, float max_norm, int project, float lr, float beta1,
                       float beta2, float eps, int step, void *stream);

/* ---- sign momentum: Lion (Chen et al. 2023, arXiv:2302.06675), and Signum (Bernstein et al. 2018) as its beta1 == beta2
 * case.  One moment M, no second moment, no bias correction, no step count, no weight decay.  Per row r of the [rows][d]
 * view msae_adam_rows_f32 takes, one workgroup:
 *   c  = min(1, max_norm / (sqrtf(*total_sumsq) + 1e-6f))          (total_sumsq NULL: 1)   as msae_adam_rows_f32
 *   g  = c * G[r][j];   if project: g -= <g, W[r]> * W[r][j]                                as msae_adam_rows_f32
 *   u  = fmaf(g - m, 1.f - beta1, m)        the interpolated momentum that is signed
 *   s  = (u > 0) - (u < 0)                  0 for u == 0, and for a NaN
 *   w' = w - lr * s                         one float32 multiplication (exact: s is -1, 0 or 1), one float32 subtraction
 *   m' = fmaf(g - m, 1.f - beta2, m)        the carried momentum
 * Bit-level rules: g - m and 1.f - beta are float32 operations, u and m' are each ONE fused multiply-add of them (no other
 * contraction anywhere), so given g the sign and the momentum are defined bit for bit, and with beta1 == beta2 u == m'.
 * An element with s == 0 keeps its bits.  G is read only.
 * renorm_eps (>= 0: on) and prepared / T_next / opts are the tails of msae_adam_rows_fused_f32, with its bits: a call with
 * tails leaves the M, and before the renorm the W, of a call without.  d % 4 == 0 and d <= 8192 is one kernel (W, G, M
 * 16-byte aligned, else MSAE_EALIGN); other shapes run a plain pass and then the separate tail passes.  Null W / G / M or a
 * non-positive shape: MSAE_EINVAL.  No atomics, no workspace: two runs give the same bits.  20 bytes moved per element. */
int msae_lion_rows_f32(float *W, const float *G, float *M, int rows, int d, const float *total_sumsq, float max_norm,
                       int project, float lr, float beta1, float beta2, float renorm_eps, void *prepared, int T_next,
                       const msae_options *opts, void *stream);

/* ---- blockwise 8-bit Adam moments ("adam8"; the role of bitsandbytes' Adam8bit in train/sae/sae/trainer.py:139-147,
 * a format of this project's own: checkpoints are NOT interchangeable with bitsandbytes') ----
 * A parameter is the [rows][d] view msae_adam_rows_f32 takes.  A BLOCK is 256 consecutive elements of one row, the last
 * block of a row may be partial: nb = rows * ceil(d / 256) blocks, block b of row r is number r * ceil(d / 256) + b.
 *   M8 uint8 [rows*d]   codes of the first moment m
 *   R8 uint8 [rows*d]   codes of r = sqrt(v), the SQUARE ROOT of the second moment (v spans twice the binades of r)
 *   SM, SR float32 [nb] one scale per block
 * A code is OCP e4m3fn (gfx950's conversion instructions); stored value = decode(code) * scale, scale = absmax_block / 448.f
 * (an all-zero block: scale 0, codes 0).
 *   encode   q = x * (448.f / absmax), clamped to +-448 in float32, rounded to nearest, ties to even, subnormals included.
 *            The NaN codes 0x7F / 0xFF are never written; 0x80 (-0) and 0x00 are the same value, either is valid.
 *            R8 never loses a positive value: r > 0 that would round to 0 is stored as code 1 (the smallest subnormal) --
 *            else an element whose v underflows inside a block with a large absmax would divide its still-nonzero m by eps.
 *   decode   m = dec(M8) * SM[b];  r = dec(R8) * SR[b];  v = r * r -- three separate float32 multiplications, none of them
 *            contracted into an fma.
 * Shapes: d % 4 == 0, d <= 8192, and not one row of a length that is no multiple of 1024 (the view of a vector whose
 * length 1024 does not divide: one workgroup would own the whole parameter); others return MSAE_ENOTIMPL and keep
 * float32 moments.  msae_adam8_blocks adds the caller's policy floor rows * d >= 4096 (bitsandbytes' min_8bit_size): it
 * returns nb, or 0 for a parameter that stays float32 (pure host code).  W, G, M, V, M8, R8 16-byte aligned.
 *
 * msae_adam8_rows_f32:       msae_adam_rows_fused_f32 (same clip, projection, Adam arithmetic, renorm_eps and prepared /
 *                            T_next / opts tails, same bits of those tails given the same updated W) with the moments read
 *                            from and written to the format above.  The update of W uses the float32 m', v' of this step;
 *                            only the carried state is quantised.  No atomics: two runs give the same bits.
 * msae_adam8_quantize_f32:   M, V (float32, V >= 0) -> M8, R8, SM, SR.
 * msae_adam8_dequantize_f32: the inverse: exactly the m and v msae_adam8_rows_f32 computes with. */
size_t msae_adam8_blocks(int rows, int d);
int msae_adam8_rows_f32(float *W, const float *G, uint8_t *M8, uint8_t *R8, float *SM, float *SR, int rows, int d,
                        const float *total_sumsq, float max_norm, int project, float lr, float beta1, float beta2,
                        float eps, int step, float renorm_eps, void *prepared, int T_next, const msae_options *opts,
                        void *stream);
int msae_adam8_quantize_f32(const float *M, const float *V, uint8_t *M8, uint8_t *R8, float *SM, float *SR, int rows,
                            int d, void *stream);
int msae_adam8_dequantize_f32(const uint8_t *M8, const uint8_t *R8, const float *SM, const float *SR, float *M, float *V,
                              int rows, int d, void *stream);

/* ---- stage timing of msae_encode_topk's fused path (measurement aid for bench.py) --------------
 * A profile handle passed in msae_options::profile makes every fused msae_encode_topk call made with it
 * record HIP events, on the stream it launches on, at the boundaries of its 6 stages:
 *   0 prep (zero + quantise x) 1 sample GEMM   2 threshold TopK   3 main int8/bf16 MFMA GEMM
 *   4 select + exact re-score 5 exact fallback of flagged tokens
 * for up to max_steps calls.  _read synchronises on the recorded events and returns stage_ms[n_steps][6]
 * (HOST pointers) and restarts the handle at step 0.  One handle must not be used by two threads at once. */
int msae_profile_create(int max_steps, void **handle);
int msae_profile_read(void *handle, float *stage_ms, int *n_steps);
int msae_profile_destroy(void *handle);

#ifdef __cplusplus
}
#endif
#endif /* MSAE_H_ */
