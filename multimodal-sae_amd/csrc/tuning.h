// tuning.h -- every build-time tuning knob, ablation switch and measurement probe of libmsae_hip.so, in ONE place.
//
// The product build (csrc/build.sh) defines none of these macros: the knobs take the defaults below (each the winner of
// an A/B run recorded in NOTEBOOK.md), the ablation switches are `false`, the probes expand to nothing.  Instrumented
// builds (tools/build_dbg.sh, tools/gpu_ab*.sh) pass -D flags; the kernels test `msae_tuning::...` constants with
// `if constexpr` / plain `if`, so product sources carry no conditional compilation of their own.  Experiments that were
// measured and not kept live under tools/tuning/ (e.g. the 64-byte / 4-slot ring GEMM, gemm_mfma64.h), not here.
#pragma once

// ---- knobs (value macros, default = product) ------------------------------------------------------------------------
#ifndef MSAE_GEMM_STAGGER      // candidate GEMM: 1 = waves 4-7 issue their LDS-DMA pieces behind k-step MSAE_GEMM_STAGGER_AT
#define MSAE_GEMM_STAGGER 1    // (-4 % on the main pass with tile-major operands: profiles/r03_ab_stagger_tile_major.txt); 0 = off, 2 = odd waves
#endif
#ifndef MSAE_GEMM_STAGGER_AT   // 0 since the wave-block staging of round 5 (issue is ~100 cycles instead of ~700: the earlier the pieces leave,
#define MSAE_GEMM_STAGGER_AT 0 // the better -- 3.93-3.97 ms against 4.04-4.07 behind k-step 1, two boxes: profiles/r05_ab_stagger_at.txt)
#endif
#ifndef MSAE_GEMM_GM           // candidate GEMM: super-tile of output tiles an XCD's 32 workgroups work on together (gemm_map_tile): GM row tiles
#define MSAE_GEMM_GM 8         // x GN column tiles, GM * GN = 32.  8 x 4 fetches 12 operand blocks per k-step for 32 tiles; 4 x 8 the same with the
#define MSAE_GEMM_GN 4         // roles swapped, 16 x 2 / 2 x 16 fetch 18 (profiles/r05_ab_supertile.txt)
#endif
#ifndef MSAE_GEMM_MF           // int8 candidate GEMM (GemmI8, GemmI8Cert): MFMA shape, 16 = v_mfma_i32_16x16x64_i8, 32 = v_mfma_i32_32x32x32_i8.
#define MSAE_GEMM_MF 16        // Equal MACs per cycle; 16x16x64 holds a higher clock under the power cap (profiles/gemm_mfma_shape.txt)
#endif
static_assert(MSAE_GEMM_MF == 16 || MSAE_GEMM_MF == 32, "MSAE_GEMM_MF: 16 or 32");
#ifndef MSAE_SK_UN             // weight-stream kernel: 64-B k-steps per B batch at 64 tokens (halved per doubling of the tile)
#define MSAE_SK_UN 4
#endif
#ifndef MSAE_SK_ABL            // weight-stream kernel ablations: 1 no A chunk traffic, 2 no B loads, 4 no MFMAs (results invalid)
#define MSAE_SK_ABL 0
#endif
#ifndef MSAE_RESCORE_U         // re-score: 16-B loads per lane and batch
#define MSAE_RESCORE_U 16
#endif
#ifndef MSAE_RESCORE_LPR       // lanes that share a row of W_enc in the FIRST round's re-scoring stream: 1, or 4 (64-B pieces per
#define MSAE_RESCORE_LPR 1     // row and instruction, 16 rows per pass: measured 1.61 ms against 1.17 -- not the default)
#endif
#ifndef MSAE_GUARD_ZETA        // first re-score round reaches zeta sigma below the k-th coarse value
#define MSAE_GUARD_ZETA 1.f
#endif

// ---- load flavours of the weight streams (each row piece is read exactly once per call: non-temporal by default) -----------
#ifdef MSAE_SK_PLAIN
#define MSAE_SK_LOAD(p) (*(p))
#else
#define MSAE_SK_LOAD(p) __builtin_nontemporal_load(p)
#endif
#ifdef MSAE_SK_NOFENCE
#define MSAE_SK_FENCE() do { } while (0)
#else
#define MSAE_SK_FENCE() __builtin_amdgcn_sched_barrier(0)   // a batch of loads is issued as a batch, where it is written
#endif
// The S = 1 weight stream reads every 1-KiB row piece exactly once per call: non-temporal loads (0.141 -> 0.131 ms at T = 1).
// NOT for the re-scoring rows: a lane fetches a 128-B line in eight 16-B loads and lives on the cache holding it in between
// (non-temporal there: 1.18 -> 3.34 ms, profiles/r02_ab_nontemporal.txt).
#ifdef MSAE_GEMV_PLAIN_LOADS
#define MSAE_STREAM_LOAD(p) (*(p))
#else
#define MSAE_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#endif
#ifdef MSAE_MF_PLAIN_LOADS
#define MSAE_MF_LOAD(p) (*(p))
#else
#define MSAE_MF_LOAD(p) __builtin_nontemporal_load(p)
#endif

#ifdef MSAE_ADAM_PLAIN_LOADS
#define MSAE_ADAM_LOAD(p) (*(p))
#define MSAE_ADAM_STORE(v, p) (*(p) = (v))
#else
#define MSAE_ADAM_LOAD(p) __builtin_nontemporal_load(p)
#define MSAE_ADAM_STORE(v, p) __builtin_nontemporal_store((v), (p))
#endif

// ---- ablation switches (results are INVALID when one is set; stage clocks of the others stay comparable) ---------------------
namespace msae_tuning {
#ifdef MSAE_ABL_NOEPI
constexpr bool ABL_NOEPI = true;        // candidate GEMM: skip the threshold epilogue's element loop
#else
constexpr bool ABL_NOEPI = false;
#endif
#ifdef MSAE_ABL_NOFLUSH
constexpr bool ABL_NOFLUSH = true;      // ... drop the LDS queue instead of flushing it
#else
constexpr bool ABL_NOFLUSH = false;
#endif
#ifdef MSAE_ABL_NOLEAD
constexpr bool ABL_NOLEAD = true;       // ... no outlier k-tile and no acc * m - E pass in the MAIN pass (the round-5 verdict's A/B: what the tile costs)
#else
constexpr bool ABL_NOLEAD = false;
#endif
#ifdef MSAE_ABL_NOFALLBACK
constexpr bool ABL_NOFALLBACK = true;   // fused encode: no exact fallback launches
#else
constexpr bool ABL_NOFALLBACK = false;
#endif
#ifdef MSAE_RESCORE_NO_PRESELECT
constexpr bool RESCORE_PRESELECT = false;   // re-score: sort the whole candidate list instead of pre-selecting ~128 keys
#else
constexpr bool RESCORE_PRESELECT = true;
#endif
#ifdef MSAE_FULL_MAIN_PASS
constexpr bool MAIN_SKIPS_SAMPLE = false;   // main candidate pass over ALL rows (the sample rows twice): the round-2 layout
#else
constexpr bool MAIN_SKIPS_SAMPLE = true;
#endif
#ifdef MSAE_GEMM_TIMELINE
constexpr int GEMM_TIMELINE = MSAE_GEMM_TIMELINE + 0 == 2 ? 2 : 1;
#else
constexpr int GEMM_TIMELINE = 0;
#endif
}  // namespace msae_tuning

// ---- probes: s_memtime stamps (tools/gemm_timeline.py, tools/rescore_timeline.py) ------------------------------------------
// candidate GEMM: workgroup 0 / wave 0, 8 stamps per output tile into GemmEpilogue::timeline (null in the product)
#if defined(MSAE_GEMM_TIMELINE) && MSAE_GEMM_TIMELINE != 2
#define MSAE_TL(slot) do { if (blockIdx.x == 0 && threadIdx.x == 0 && ep.timeline && tl_tile < 64) \
    ep.timeline[tl_tile * 8 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define MSAE_TL(slot) do { } while (0)
#endif
#if defined(MSAE_GEMM_TIMELINE) && MSAE_GEMM_TIMELINE == 2   // inside k-tile 8 of every output tile (wave MSAE_TLK_WAVE)
#ifndef MSAE_TLK_WAVE
#define MSAE_TLK_WAVE 0
#endif
#define MSAE_TLK(cond, slot) do { if ((cond) && blockIdx.x == 0 && threadIdx.x == 64 * MSAE_TLK_WAVE && ep.timeline && tl_tile < 64) \
    ep.timeline[tl_tile * 8 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define MSAE_TLK(cond, slot) do { } while (0)
#endif
// re-score: thread 0 of the first 64 tokens, 16 stamps each
#ifdef MSAE_RESCORE_TL
__device__ unsigned long long g_rs_tl[64 * 16];
#define MSAE_RTL(slot) do { if (threadIdx.x == 0 && blockIdx.x < 64 && (slot) < 16) g_rs_tl[blockIdx.x * 16 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#define MSAE_RTL_VALUE(slot, v) do { if (threadIdx.x == 0 && blockIdx.x < 64) g_rs_tl[blockIdx.x * 16 + (slot)] = (v); } while (0)
#else
#define MSAE_RTL(slot) do { } while (0)
#define MSAE_RTL_VALUE(slot, v) do { } while (0)
#endif

// ---- perturbed-schedule build (csrc/build.sh: libmsae_hip_perturb.so; tests/test_gpu_perturbed_schedule.py) -------------------
// MSAE_GRID_CAP (0 = none): the looping launches run at most this many workgroups, so that each walks several tiles at a test's
// small shapes: the persistent grid of gemm_launch (a multiple of 8: gemm_map_tile's XCD super-tile), and the column-tile and row
// grids of the in-call exact fallback (encode_f32.hip: launch_dt with n_rows, topk.hip: msae_topk_launch with n_rows).
#ifndef MSAE_GRID_CAP
#define MSAE_GRID_CAP 0
#endif
static_assert(MSAE_GRID_CAP >= 0 && MSAE_GRID_CAP % 8 == 0, "MSAE_GRID_CAP: 0 or a multiple of 8");
namespace msae_tuning {
constexpr int GRID_CAP = MSAE_GRID_CAP;
constexpr int grid_cap(int grid) { return GRID_CAP > 0 && grid > GRID_CAP ? GRID_CAP : grid; }
}  // namespace msae_tuning

// MSAE_PERTURB: MSAE_PERTURB_AT(site, visit) delays the calling WAVE by a pseudo-random time on about one visit in four (per-k-tile
// sites, MSAE_PERTURB_AT_K: one in sixteen), so that the waves of a workgroup -- and the workgroups of a launch -- meet every
// hand-synchronised hand-over at relative speeds the product's one schedule never shows.  The delay is a hash of (run seed,
// workgroup, wave, site, the wave's visit counter): no clock is read, a run repeats from its seed.  Up to MSAE_PERTURB_MAX
// s_sleep units of 64 clocks: 32 (~2000 cycles) by default; build.sh builds the variant with 256, because a delay only shows a
// missing barrier when it is longer than the path it races against (epilogue exit -> next tile's side fetch -> early park is a
// global-load round trip, ~2000 cycles by itself: profiles/perturb_sensitivity.txt).  One site per hand-over; the
// comment at each MSAE_PERTURB_AT says which.  X(enum name, hand-over)
#define MSAE_PERTURB_SITES(X) \
  X(GEMM_TILE_ENTRY, "gemm_kernel: a wave enters a tile while others may be in the previous tile's epilogue") \
  X(GEMM_PARK_EARLY, "gemm_kernel: in front of GemmSide::park_early (EARLY pair vs the previous epilogue's side reads)") \
  X(GEMM_KTILE_BARRIER, "gemm_kernel: in front of the k-tile barrier (vmcnt(0) of this wave vs the others' fragment reads)") \
  X(GEMM_STAGE_EARLY, "gemm_kernel: behind the barrier, in front of stage_next() of the early waves (ring slot reuse)") \
  X(GEMM_STAGE_LATE, "gemm_kernel: in front of stage_next() of the staggered waves, inside the compute phase") \
  X(GEMM_SIDE_PARK, "gemm_kernel: behind the k-loop, in front of GemmSide::park (vs the previous epilogue's flush)") \
  X(GEMM_EPI_ENTER, "gemm_epilogue: in front of its first barrier (side buffer written, previous flush done)") \
  X(GEMM_EPI_BEHIND, "gemm_epilogue: behind its first barrier (queue count reset vs the first reservations)") \
  X(GEMM_EPI_FLUSH, "gemm_epilogue: in front of the queue flush's barrier (pushes vs the flush's reads)") \
  X(GEMM_EPI_FLUSHED, "gemm_epilogue: behind the flush loop (vs the next tile's reservations and side writes)") \
  X(GEMM_TILE_EXIT, "gemm_kernel: tile exit") \
  X(SKINNY_ENTRY, "gemm_skinny_kernel: behind park_early, in front of the first loads") \
  X(SKINNY_BATCH, "gemm_skinny_kernel: between the two B load batches of a double-batch") \
  X(SKINNY_CHUNK, "gemm_skinny_kernel: in front of the raw barrier that hands an A buffer over") \
  X(SKINNY_EPILOGUE, "gemm_skinny_kernel: in front of the accumulator image's first barrier (A buffers become the image)") \
  X(SMALL_ARRIVE, "rescore_small_kernel: in front of the token's device-scope arrival counter") \
  X(SMALL_FINAL, "rescore_small_kernel: the finalising wave, in front of its acquire") \
  X(RESCORE_LIST, "select_rescore_kernel: behind load_list (list and activations in LDS vs the sorts)") \
  X(RESCORE_SORTED, "select_rescore_kernel: behind the prefix sort, in front of first_round_target's LDS exchange") \
  X(RESCORE_TARGET, "select_rescore_kernel: behind first_round_target, in front of the round") \
  X(RESCORE_ROUND, "select_rescore_kernel: behind a round's re-score pass, in front of its result sort") \
  X(RESCORE_VERIFY, "select_rescore_kernel: behind the result sort, in front of verify") \
  X(RESCORE_FOLLOWUP, "select_rescore_kernel: in front of a follow-up round's barrier") \
  X(RESCORE_FM_SCAN, "fm_scan_kernel (feature-major first round): in front of the LDS scan of the waves' partial sums") \
  X(RESCORE_FM_DOT, "fm_dot_kernel (feature-major first round): workgroup entry (a token's pairs finish in any order)")
enum MsaePerturbSite {
#define MSAE_PS_ENUM(name, what) PS_##name,
  MSAE_PERTURB_SITES(MSAE_PS_ENUM)
#undef MSAE_PS_ENUM
  MSAE_PERTURB_NSITES
};
#ifdef MSAE_PERTURB
#ifndef MSAE_PERTURB_MAX       // longest delay in s_sleep units of 64 clocks (32: ~2000 cycles)
#define MSAE_PERTURB_MAX 32
#endif
__device__ unsigned long long g_perturb_hits[MSAE_PERTURB_NSITES];
__device__ unsigned g_perturb_seed;
__device__ __forceinline__ unsigned msae_perturb_mix(unsigned h, unsigned v) {
  h ^= v + 0x9E3779B9u + (h << 6) + (h >> 2);
  h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
// `visit` is the wave's visit counter of the site, read off the loop the site stands in (tile id, flat k-tile number, round)
// instead of being kept in memory: a counter fetched with a returning atomic costs a memory round trip per visit, as long as the
// delays themselves, on exactly the paths (epilogue exit -> next tile's early park) whose shortness the probes are there to test.
// The books are one fire-and-forget atomic of the first active lane.
__device__ __forceinline__ void msae_perturb_at(int site, unsigned visit, unsigned one_in) {
  const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (lane == (unsigned)__builtin_ctzll(__ballot(1))) atomicAdd(&g_perturb_hits[site], 1ull);
  const unsigned wg = blockIdx.x + gridDim.x * blockIdx.y, wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned seed = g_perturb_seed;   // 0 (the state until a seed is set): count the visit, never sleep
  unsigned h = msae_perturb_mix(seed, wg);
  h = msae_perturb_mix(h, wave);
  h = msae_perturb_mix(h, (unsigned)site);
  h = msae_perturb_mix(h, (unsigned)__builtin_amdgcn_readfirstlane((int)visit));
  const unsigned units = seed != 0u && h % one_in == 0u ? (h >> 8) % (unsigned)(MSAE_PERTURB_MAX + 1) : 0u;   // wave-uniform: s_sleep ignores EXEC
  for (unsigned i = 0; i < units; ++i) __builtin_amdgcn_s_sleep(1);
}
#define MSAE_PERTURB_AT(site, visit) msae_perturb_at(PS_##site, (unsigned)(visit), 4u)
#define MSAE_PERTURB_AT_K(site, visit) msae_perturb_at(PS_##site, (unsigned)(visit), 16u)
// host side: the last candidate-GEMM launches (gemm_launch), so that a test can ASSERT its tiles per workgroup
struct MsaePerturbLaunch { int kind, tiles, grid; };   // kind: 0 = sample (DENSE), 1 = main (THRESH)
constexpr int MSAE_PERTURB_NLAUNCH = 64;
inline MsaePerturbLaunch g_perturb_launches[MSAE_PERTURB_NLAUNCH];
inline int g_perturb_n_launches = 0;
#define MSAE_PERTURB_LAUNCH(kind, tiles, grid) \
  (g_perturb_launches[g_perturb_n_launches++ % MSAE_PERTURB_NLAUNCH] = MsaePerturbLaunch{(kind), (tiles), (grid)})
// Exported by the variant only (the one translation unit built with MSAE_PERTURB: encode_fused.hip); the test runner binds them
// itself.  The seed: MSAE_PERTURB_SEED in the environment, read at the first reset, or msae_perturb_set_seed; seed 0 (the
// state until one is set) switches the delays off.
extern "C" __attribute__((visibility("default"))) int msae_perturb_set_seed(unsigned seed) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_perturb_seed), &seed, sizeof(seed));
}
// zero the site counters and the launch record
extern "C" __attribute__((visibility("default"))) int msae_perturb_reset() {
  static const bool seeded = [] {
    const char *e = getenv("MSAE_PERTURB_SEED");
    if (e) (void)msae_perturb_set_seed((unsigned)strtoul(e, nullptr, 0));
    return true;
  }();
  (void)seeded;
  void *hits = nullptr;
  if (hipDeviceSynchronize() != hipSuccess) return (int)hipGetLastError();
  if (hipGetSymbolAddress(&hits, HIP_SYMBOL(g_perturb_hits)) != hipSuccess) return (int)hipGetLastError();
  if (hipMemset(hits, 0, sizeof(g_perturb_hits)) != hipSuccess) return (int)hipGetLastError();
  g_perturb_n_launches = 0;
  return (int)hipDeviceSynchronize();
}
// out[0, min(n, sites)) = visits per site since the last reset; returns the number of sites (negative: a HIP error)
extern "C" __attribute__((visibility("default"))) int msae_perturb_hits(unsigned long long *out, int n) {
  unsigned long long h[MSAE_PERTURB_NSITES];
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(h, HIP_SYMBOL(g_perturb_hits), sizeof(h)) != hipSuccess)
    return -(int)hipGetLastError() - 1;
  for (int i = 0; i < n && i < MSAE_PERTURB_NSITES; ++i) out[i] = h[i];
  return MSAE_PERTURB_NSITES;
}
extern "C" __attribute__((visibility("default"))) const char *msae_perturb_site_name(int site) {
  static const char *const names[] = {
#define MSAE_PS_NAME(name, what) #name ": " what,
    MSAE_PERTURB_SITES(MSAE_PS_NAME)
#undef MSAE_PS_NAME
  };
  return site >= 0 && site < MSAE_PERTURB_NSITES ? names[site] : nullptr;
}
// out[3 i ..] = (kind, tiles, grid) of the i-th candidate-GEMM launch since the previous call (or reset), oldest first, at most n
// of the last MSAE_PERTURB_NLAUNCH; returns how many were written and starts the record afresh
extern "C" __attribute__((visibility("default"))) int msae_perturb_launches(int *out, int n) {
  const int have = g_perturb_n_launches < MSAE_PERTURB_NLAUNCH ? g_perturb_n_launches : MSAE_PERTURB_NLAUNCH;
  const int first = g_perturb_n_launches - have, m = have < n ? have : n;
  for (int i = 0; i < m; ++i) {
    const MsaePerturbLaunch &l = g_perturb_launches[(first + i) % MSAE_PERTURB_NLAUNCH];
    out[3 * i] = l.kind; out[3 * i + 1] = l.tiles; out[3 * i + 2] = l.grid;
  }
  g_perturb_n_launches = 0;
  return m;
}
#else
#define MSAE_PERTURB_AT(site, visit) do { } while (0)
#define MSAE_PERTURB_AT_K(site, visit) do { } while (0)
#define MSAE_PERTURB_LAUNCH(kind, tiles, grid) do { } while (0)
#endif
