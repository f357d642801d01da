// gemm_mfma.h -- candidate-pass GEMM  C[T][N] = A[T][K] * B[N][K]^T  on the gfx950 matrix cores, with
// the SAE epilogues.  Two operand types share one tile / pipeline structure:
//   bf16 : v_mfma_f32_32x32x16_bf16, f32 accumulate          (2.5 PFLOP/s dense peak)
//   int8 : v_mfma_i32_16x16x64_i8 (the default; v_mfma_i32_32x32x32_i8 behind MSAE_GEMM_MF=32, tuning.h),
//          i32 accumulate, per-token x per-feature scales applied in the
//          epilogue; a leading "outlier" k-tile carries the few massive activation dims at a
//          coarser per-token scale (acc *= m[t] after it)   (~2x the bf16 rate, half the bytes)
// This is the dominant kernel of the fused encoder (encode_fused.hip): 2*d*N FLOP per token.  Both
// operands are K-contiguous, so A and B fragments are read the same way.
//
// Structure (template parameters BM, BN, STAGES, WM, WN; a k-tile is always 128 B per row):
//   * a workgroup of WM x WN waves computes a BM x BN tile; each wave owns (BM/WM) x (BN/WN) as
//     MI x NI accumulator blocks of 16 VGPRs each: one 32x32 MFMA result, or (int8 16x16x64) four 16x16
//     results stacked in rows, 64 x 16 (GemmEpiCfg);
//   * operand tiles travel L2 -> LDS by global_load_lds (16 B per lane, 1 KiB per wave instruction,
//     no VGPR round trip) into a ring of STAGES slots; counted s_waitcnt vmcnt + ONE raw s_barrier
//     per k-tile, so loads stay in flight across barriers;
//   * LDS image: row r of a tile at byte r*128 with its eight 16-B chunks XOR-permuted by
//     swz(r) = (r >> 1) & 7: every ds_read_b128 fragment read is bank-conflict-free
//     (SQ_LDS_BANK_CONFLICT = 0 measured).  global_load_lds writes lane-linear, so the permutation
//     is applied to the per-lane SOURCE address and again on the read;
//   * the fragment reads of a k-tile are inline-asm ds_read_b128 with COUNTED lgkmcnt waits (the
//     compiler waits lgkmcnt(0) after every group of reads): the reads of the next (half) k-step are in
//     flight while the MFMAs of this one execute -- 32x32: 6 reads behind 8 MFMAs, 16x16x64: 4-fragment
//     groups behind 16 (-5 % on the int8 pass; gemm_compute_asm32 / gemm_compute_asm16);
//   * workgroups are persistent (one per CU) and walk their tiles as one flat k-sequence: the last
//     k-iteration of a tile already stages the first k-tile of the next one;
//   * tile -> workgroup map is XCD-aware: the 32 workgroups resident on one XCD's 32 CUs form an
//     8 (M) x 4 (N) super-tile sharing 8 A-tiles and 4 B-tiles in that XCD's private L2.
//
// Round 2 (profiles/r02_gemm_sweep_*.txt, int8 operands, 64 k-tiles per output tile): full loop 1.67 us
// per k-tile and workgroup; LDS-DMA staging alone 1.41-1.75 us (46 GB/s per CU out of L2, the same with
// plain global_load_dwordx4 -> ds_write_b128 staging: 1.72 us, so it is the L2 -> CU delivery of this
// access pattern, not the DMA instruction); MFMA + fragment reads + barriers alone 1.35-1.40 us.  The
// two-group ping-pong loop (waves 0-3 / 4-7 half a k-tile apart, one barrier per half: commit 5ad2c1e^)
// hides the DMA issue behind the partner wave's MFMAs but pays four barriers per k-tile: 1.81-1.92 us.  Issuing part of a wave's DMA pieces behind
// its own MFMA groups (2..8 pieces after k-steps 0/1/2; profiles/r02_gemm_sweep_dma_interleave.txt): -2 % to +16 %.  Register staging: 2.6-3.3 us (32 more
// live VGPRs, spills).  What paid in round 2: wave-uniform DMA base addresses (saddr form, 1 VGPR) and
// computing the epilogue's band constants after the k-loop instead of in the prologue (4.7 -> 4.27 ms).
//
// Measured on MI355X (tools/gemm_sweep, T=8192 K=4096 N=131072, random data; profiles/):
//   256x256 tile, 2-slot ring, 8 waves (2x4): bf16 1.20 PFLOP/s (1.39 on zero-filled operands: the
//   kernel is partly DVFS-bound), int8 2x that; 128x128: 1.0.  Ablations: MFMA+barriers only
//   5.4 ms, LDS-DMA staging only 5.4 ms (~12.7 TB/s L2->LDS, independent of ring depth and row
//   pitch), both 7.3 ms.  Deeper rings (half-size k-tiles x 4 slots), a two-group ping-pong
//   schedule, s_setprio, an L2 prefetch and issuing the DMA behind the first MFMA group were all
//   measured equal or worse and are not kept.
// Round 5 (profiles/r05_ab_stagger_at.txt, r05_ab_supertile.txt, r05_gemm96_prototype.txt): a wave's eight pieces are issued as ONE
// block (gemm_stage_block: two SGPR bases, the rest immediate offsets that the instruction adds to the global AND the LDS address:
// ~100 cycles instead of ~700), after which the staggered waves issue behind k-step 0 instead of 1 (-2 %); L2 warming, pre-staging
// the next tile's second k-tile, other super-tile shapes and a 96-byte / 3-slot ring (tools/tuning/gemm_mfma96.h) all measured equal.
//
// Epilogues work on the UPPER value u = v + z*sigma(t, n) of every output, v = coarse pre-activation
// (value + bias) and z*sigma the width of the error band of the operand type (encode_fused.hip):
//     z^2 sigma^2(t, n) = P_t Q_n + R_t (Si_n + M_t So_n),  R_t = sx_t^2 z^2/12, M_t = m_t^2 (int8 only)
//   DENSE  out[t][n] = u                                                      (sample pass)
//   THRESH append (feature, u) to token t's candidate list when u > tau[t].  The hot loop tests the
//          separable upper bound  v + h_n B_t > tau[t]  (one fma more than a plain compare):
//            B_t = z sigma of token t against a REFERENCE feature (refs = typical Q, Si, So),
//            h_n^2 = max(Q_n/Qr, Si_n/Sir, So_n/Sor)  =>  h_n B_t >= z sigma(t, n) for every pair;
//          survivors are queued in LDS and the exact u of each is computed when the queue is flushed
#pragma once
#include <cstdlib>

#include "common.h"
#include "tuning.h"


struct GemmEpilogue {
  const float *bias;             // b_enc
  int bias_stride, bias_off;     // feature of column n is n*bias_stride + bias_off ...
  int skip_stride, skip_off;     // ... or, with skip_stride = S > 0, the n-th feature f with f % S != skip_off (gemm_feature)
  float *dense; int ld_dense;    // DENSE
  const float *tau_vals; int tau_ld, tau_col;   // THRESH: tau[t] = tau_vals[t*tau_ld + tau_col]
  int *cnt; unsigned long long *cand; int cap;  // candidate lists
  // A token's list can be split into `segs` (0 / 1: one) equal segments with their own counters cnt[t*segs + s]: workgroup b
  // appends to segment b % segs.  A batch of few tokens has hundreds of appends per counter (~650 per token, all of the launch's
  // workgroups on <= 256 addresses); same-address atomics serialise in L2, ~45 ns each: 0.03 ms of a 0.13 ms pass.
  int segs;
  int skip_a, skip_b;            // features never emitted (hook edits replace their latents)
  // error-band constants (encode_fused.hip): per token (sx, m as float, P, -), per COLUMN of this
  // launch (sw, Q, Si, So).  int8: value = float(acc) * sx[t] * sw[n]; bf16 ignores sx, sw, Si, So.
  const f32x4 *rowc, *colc;
  const float *refs;             // (Qr, Sir, Sor): the reference feature of the separable bound
  float zz12;                    // z^2 / 12
  // Subtractive dither (round 6; encode_defs.h): row_e[t] = (E_t, m_t) -- the token's integer correction of the weights' shared
  // dither and its outlier multiplier: acc = acc_outlier_tile * m - E in the multiply that scales the outlier tile anyway -- and
  // col_ds[n] = sw_n D_n, the feature's correction of the activations' shared dither: v = (acc sw - Ds) sx + b, the same two
  // packed instructions as (acc (sx sw) + b).  Both null: no correction (m from rowc[t][1]).  int8 only.
  const int2 *row_e;
  const float *col_ds;
  unsigned long long *timeline;  // tuning builds (tuning.h, MSAE_TL): s_memtime stamps of workgroup 0 / wave 0; null in the product
};

// Operands of one launch.  A rows are tokens, B rows are features; ld* in BYTES.
struct GemmOperands {
  const unsigned char *A, *B;
  size_t ldA, ldB;
  int nk;                        // k-tiles of 128 B per row
  // int8 only: optional leading outlier tile (one k-tile, rows 128 B apart); the accumulators are
  // multiplied by the token's integer multiplier m (GemmEpilogue::rowc[t][1]) after it
  const unsigned char *Ao, *Bo;
  const int *n_out;              // device: number of outlier dims actually present (the tile is compact from column 0)
  // Tile-major operands (round 3): A and B are stored [row tile of BM / BN rows][k-tile][row in tile][128 B] with the LDS
  // image's chunk permutation already applied (position p of row r holds the row's 16-B chunk p ^ swz(r)), so a 1-KiB
  // staging piece is ONE contiguous kilobyte -- eight consecutive 128-B lines instead of eight lines a leading
  // dimension apart -- and every lane's source offset is lane * 16.  Measured on the stream alone (tools/dma_depth,
  // profiles/r03_dma_tile_major.txt): 43.2 -> 47.7 GB/s per CU with the 2 x 128 B ring, 50.6 -> 65.9 with 4 x 64 B.
  int packed;
  // Certified pass (encode_cert.h): > 0 = k-tiles per PLANE (d / 128).  A and B are tile-major with 2 * cert k-tiles per row tile
  // (plane 0 = lo, plane 1 = hi); nk = 3 * cert; k-tile q of the walk multiplies A plane (q < cert ? lo : hi) with B plane
  // (cert <= q < 2 cert ? lo : hi), and the accumulators are divided by 128 (rounded) in front of k-tile 2 * cert:
  // acc = x_hi . W_hi + round((x_lo . W_hi + x_hi . W_lo) / 128).  The token's rowc[1] is the band's M_t (no outlier tile).
  int cert;
};

constexpr int gemm_side_bytes(int nt) { return 7 * nt * 4; }   // the LDS side buffer of nt threads (GemmSide)

// What gemm_epilogue and GemmSide require of a config C, stated once.  From this base: the operand kind (I8 / F8 / CERT -> SCALED)
// and the accumulator block shape (MF16, BR x BC, acc_row / acc_col).  From the config itself: BM, BN, NT (threads, >= BM + BN),
// the wave tile TM x TN = MI x NI blocks, and the LDS map LDS_RING_BYTES | SIDE_BYTES = gemm_side_bytes(NT) | 16 | QCAP * 8.
template <bool I8_, bool F8_, bool CERT_, bool MF16_>
struct GemmEpiCfg {
  static constexpr bool I8 = I8_, F8 = F8_, CERT = CERT_, MF16 = MF16_;
  static_assert(!(I8 && F8), "fp8 accumulates in f32");
  static_assert(!MF16 || I8, "16x16x64 is an int8 shape");
  static constexpr bool SCALED = I8 || F8;       // value = acc * sx[t] * sw[n] + bias (else: acc + bias)
  static constexpr int BR = MF16 ? 64 : 32, BC = MF16 ? 16 : 32;   // rows x columns of one accumulator block (16 VGPRs)
  // row / column inside the wave tile of register e of accumulator block (i, j) in lane `lane`:
  //   32x32: C[r][n] with n = lane & 31, r = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  //   16x16: register group e >> 2 is the 16x16 block of rows 16 (e >> 2) ..; in it n = lane & 15, r = (e & 3) + 4 (lane >> 4)
  static __device__ __forceinline__ int acc_row(int i, int e, int lane) {
    return i * BR + (MF16 ? 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3) : (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5));
  }
  static __device__ __forceinline__ int acc_col(int j, int lane) { return j * BC + (lane & (BC - 1)); }
};

// FLAGS:
//   (tuning only; results invalid when an ABL bit is set)
//   bit 2 ABL_NOSTAGE  skip the LDS-DMA staging in the loop
//   bit 3 ABL_NOREAD   read the fragments once and reuse them
//   bit 4 ABL_NOMFMA   issue no MFMA
//   bit 5 CERT         the certified three-segment pass (encode_cert.h); I8 only: its own instantiation, the product kernel is untouched
//   bit 6 F8           fp8 (e4m3) operands, f32 accumulate (I8 = false)
//   bit 7 MF16         int8 through v_mfma_i32_16x16x64_i8 instead of 32x32x32 (I8 only; tuning.h MSAE_GEMM_MF)
// fp8 candidate pass (BASELINE configs[4]: "fp8 MFMA encoder path"): one byte per operand element exactly like int8 -- the SAME
// tile-major operands, LDS image, ring and hand-scheduled fragment reads -- multiplied by v_mfma_f32_32x32x16_fp8_fp8 (two per
// 16-byte fragment pair: the low and the high 8 bytes of the lanes) into f32 accumulators; per-token / per-feature scales in
// the epilogue as on the int8 path, the error band of the bf16 path's form (relative roundings).  I8_ must be false.
// The 16x16x64 int8 shape: the same MACs per cycle as 32x32x32, but under the package power cap it holds a higher clock on the
// product's operands (tools/mfma_rate.hip: 1.14x the sustained rate, profiles/gemm_mfma_shape.txt).  Tile, waves, ring, LDS
// image and staging are unchanged; a 16-VGPR accumulator block then holds four 16x16 blocks stacked in rows (64 x 16).
template <int BM_, int BN_, int STAGES_, int WM_, int WN_, bool I8_ = false, int FLAGS_ = 0>
struct GemmCfg : GemmEpiCfg<I8_, (FLAGS_ & 64) != 0, (FLAGS_ & 32) != 0, (FLAGS_ & 128) != 0> {
  using GemmCfg::GemmEpiCfg::MF16;
  using GemmCfg::GemmEpiCfg::BR;
  using GemmCfg::GemmEpiCfg::BC;
  static constexpr int BM = BM_, BN = BN_, STAGES = STAGES_, WM = WM_, WN = WN_;
  static constexpr bool ABL_NOSTAGE = FLAGS_ & 4, ABL_NOREAD = FLAGS_ & 8, ABL_NOMFMA = FLAGS_ & 16;
  static constexpr int NWAVES = WM * WN, NT = NWAVES * 64;
  static constexpr int TM = BM / WM, TN = BN / WN, MI = TM / BR, NI = TN / BC;
  static constexpr int FA = MF16 ? TM / 16 : MI, FB = MF16 ? TN / 16 : NI;   // A / B fragments of one k-step
  static constexpr int ROWB = 128;               // bytes per tile row: 64 bf16 or 128 int8
  static constexpr int KS = MF16 ? 2 : 4;        // MFMA k-steps per tile (32 B per lane-half each; 16x16x64: 16 B per lane-quarter)
  static constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
  static constexpr int LDS_RING_BYTES = STAGES * STAGE_BYTES;
  // behind the ring: side buffer of epilogue constants (GemmSide), then the THRESH epilogue's candidate queue.
  // Neither overlaps the ring: the next tile's first k-tile is already landing in it meanwhile.
  static constexpr int SIDE_BYTES = gemm_side_bytes(NT);
  static constexpr int QCAP = 2296;              // (2304 before the dither's slot of the side buffer: the budget below is the CU's whole LDS)
  static constexpr int LDS_BYTES = LDS_RING_BYTES + SIDE_BYTES + 16 + QCAP * 8;
  static_assert(STAGES == 2, "the flat cross-tile k-sequence below is written for a 2-slot ring");
  static_assert(BM + BN <= NT, "one thread per tile row and column fetches the epilogue constants");
  static constexpr int PIECES = STAGE_BYTES / 1024, PPW = PIECES / NWAVES;  // 1-KiB pieces per wave
  static constexpr int A_PIECES = A_BYTES / 1024;
  static_assert(PIECES % NWAVES == 0, "stage must split evenly over the waves");
  static_assert(TM % BR == 0 && TN % BC == 0 && TM % 32 == 0 && TN % 16 == 0, "tile shape");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

__device__ __forceinline__ int gemm_swz(int row) { return (row >> 1) & 7; }

// LDS-DMA staging.  A piece = 8 tile rows x 128 B = one wave instruction (16 B per lane).  Its global
// address is a WAVE-UNIFORM base (operand + first row of the piece + k offset: SGPRs) plus a 32-bit
// per-lane offset (row within the piece x leading dimension + swizzled 16-B chunk) that depends only
// on the parity of the piece and on the leading dimension -- four VGPRs for the whole kernel instead
// of one 64-bit address per piece.  (Tiles are always full: Tp % BM == 0 and N % BN == 0.)
struct GemmStageLane {
  unsigned off;            // byte offset of this lane inside an EVEN piece (A and B share the leading dimension);
};                         // an odd piece flips chunk bit 2: swz(row + 8) = swz(row) ^ 4, i.e. off ^ 64
__device__ __forceinline__ GemmStageLane gemm_stage_lane(int lane, unsigned ld) {
  const unsigned r_in = lane >> 3, c_in = lane & 7;
  GemmStageLane l;
  l.off = r_in * ld + ((c_in ^ ((r_in >> 1) & 7)) << 4);   // ld % 128 == 0: bit 6 belongs to the chunk index
  return l;
}
// pieces [first, first + COUNT) of one k-tile (byte offset kbyte in each row) into ring slot `slot`.
// Branch-free on purpose: control flow between two LDS-DMA instructions makes the compiler's wait-count
// pass drain vmcnt before each of them.
template <class C, int COUNT>
__device__ __forceinline__ void gemm_stage_pieces(const unsigned char *__restrict__ A,
                                                  const unsigned char *__restrict__ B, size_t ld, int m0,
                                                  int n0, size_t kbyte, unsigned char *lds, int slot, int first,
                                                  const GemmStageLane &sl) {
  unsigned char *base = lds + slot * C::STAGE_BYTES;
#pragma unroll
  for (int i = 0; i < COUNT; ++i) {
    const int piece = first + i;                      // wave-uniform
    const bool isA = piece < C::A_PIECES;
    const int pl = isA ? piece : piece - C::A_PIECES;  // piece index inside its operand tile
    const unsigned char *op0 = isA ? A : B;
    const int r0 = (isA ? m0 : n0) + pl * 8;
    const unsigned voff = sl.off ^ ((unsigned)(pl & 1) << 6);
    const unsigned char *sbase = op0 + (size_t)r0 * ld + kbyte;         // wave-uniform: SGPR pair
    const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)(base + piece * 1024);
    // saddr + 32-bit voffset form, LDS base in M0.  Written as asm because the builtin materialises a
    // 64-bit VGPR address per piece (hoisted out of the k-loop: ~2 VGPRs per piece).  No builtin LDS-DMA
    // is left in this kernel, so the compiler never holds a value of its own in M0.
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :: "v"(voff), "s"(sbase), "s"(dst) : "memory", "m0");
  }
}
// tile-major operands: tileA / tileB = the 32-KB block of this k-tile of the A / B row tile (wave-uniform)
template <class C>
__device__ __forceinline__ void gemm_stage_packed(const unsigned char *__restrict__ tileA,
                                                  const unsigned char *__restrict__ tileB, unsigned char *lds,
                                                  int slot, int wave, int lane) {
  unsigned char *base = lds + slot * C::STAGE_BYTES;
  const unsigned voff = (unsigned)lane << 4;
#pragma unroll
  for (int i = 0; i < C::PPW; ++i) {
    const int piece = wave * C::PPW + i;               // wave-uniform
    const bool isA = piece < C::A_PIECES;
    const unsigned char *sbase = isA ? tileA + piece * 1024 : tileB + (piece - C::A_PIECES) * 1024;
    const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)(base + piece * 1024);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :: "v"(voff), "s"(sbase), "s"(dst) : "memory", "m0");
  }
}

// Tile-major operands, the wave's share as ONE block: with A_PIECES % PPW == 0 a wave's PPW pieces are PPW contiguous kilobytes of
// ONE operand's 32-KB k-tile block and land in PPW contiguous kilobytes of the ring slot, and the instruction's immediate offset
// is added to BOTH the global and the LDS address -- so four pieces share one SGPR base and one M0 (offsets 0 / 1 / 2 / 3 KiB).
// Scalar work per wave and k-tile: ~12 SALU instead of ~90 (per piece: two 64-bit candidate bases, the A / B select, the LDS
// address, M0).  `src` = the wave's first source byte, `dst` = its first LDS byte (both wave-uniform).
template <class C>
struct GemmWaveBlock {
  static constexpr bool OK = C::A_PIECES % C::PPW == 0 && C::PPW % 4 == 0;
};
template <class C>
__device__ __forceinline__ void gemm_stage_block(const unsigned char *__restrict__ src, unsigned char *dst_lds, int lane) {
  const unsigned voff = (unsigned)lane << 4;
#pragma unroll
  for (int g = 0; g < C::PPW / 4; ++g) {
    const unsigned char *sbase = src + g * 4096;
    const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)(dst_lds + g * 4096);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:3072"
                 :: "v"(voff), "s"(sbase), "s"(dst) : "memory", "m0");
  }
}

// this wave's even share (PPW pieces) of one k-tile
template <class C>
__device__ __forceinline__ void gemm_stage(const unsigned char *__restrict__ A,
                                           const unsigned char *__restrict__ B, size_t ld, int m0,
                                           int n0, size_t kbyte, unsigned char *lds, int slot, int wave,
                                           const GemmStageLane &sl) {
  gemm_stage_pieces<C, C::PPW>(A, B, ld, m0, n0, kbyte, lds, slot, wave * C::PPW, sl);
}

__device__ __forceinline__ i32x4 gemm_frag(const unsigned char *tile, int row, int chunk) {
  return *reinterpret_cast<const i32x4 *>(tile + row * 128 + ((chunk ^ gemm_swz(row)) << 4));
}

// tile id -> (tm, tn); see header.  Falls back to M-fastest order when the grid does not factor.
__device__ __forceinline__ void gemm_map_tile(int b, int nM, int nN, int &tm, int &tn) {
  constexpr int GM = MSAE_GEMM_GM, GN = MSAE_GEMM_GN;   // (tuning.h: 8 x 4)
  if (nM % GM == 0 && nN % GN == 0 && ((nM / GM) * (nN / GN)) % 8 == 0) {
    const int xcd = b & 7, slot = b >> 3;
    const int grp = slot / (GM * GN), w = slot % (GM * GN);
    const int st = grp * 8 + xcd;
    const int nSM = nM / GM;
    tm = (st % nSM) * GM + (w % GM);
    tn = (st / nSM) * GN + (w / GM);
  } else {
    tm = b % nM;
    tn = b / nM;
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// one k-tile of MFMAs out of the LDS images sA / sB
// 16x16x64 int8 on register group s (registers 4s .. 4s+3) of a 16-VGPR accumulator block
__device__ __forceinline__ void gemm_mfma16(f32x16 &acc, int s, const i32x4 &a, const i32x4 &b) {
  i32x16 v = __builtin_bit_cast(i32x16, acc);
  i32x4 c = {v[4 * s], v[4 * s + 1], v[4 * s + 2], v[4 * s + 3]};
  c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  v[4 * s] = c[0]; v[4 * s + 1] = c[1]; v[4 * s + 2] = c[2]; v[4 * s + 3] = c[3];
  acc = __builtin_bit_cast(f32x16, v);
}
template <class C>
__device__ __forceinline__ void gemm_mfma_step(f32x16 (&acc)[C::MI][C::NI], const i32x4 (&a)[C::FA],
                                               const i32x4 (&b)[C::FB]) {
  if constexpr (C::MF16) {   // A fragment f = rows 16 f .. of the wave tile: block f / 4, register group f % 4
#pragma unroll
    for (int f = 0; f < C::FA; ++f)
#pragma unroll
      for (int j = 0; j < C::FB; ++j) gemm_mfma16(acc[f >> 2][j], f & 3, a[f], b[j]);
    return;
  }
  // (issue order: i outer -- consecutive MFMAs share the A fragment; j outer, four in a row on one B fragment, measured the same:
  // 3.84-3.86 vs 3.82-3.87 ms, NOTEBOOK.md)
#pragma unroll
  for (int i = 0; i < C::MI; ++i)
#pragma unroll
    for (int j = 0; j < C::NI; ++j) {
      if constexpr (C::I8) {  // the accumulator registers hold i32 on this path
        acc[i][j] = __builtin_bit_cast(
            f32x16, __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], __builtin_bit_cast(i32x16, acc[i][j]), 0, 0, 0));
      } else if constexpr (C::F8) {
        typedef long i64x2 __attribute__((ext_vector_type(2)));
        const i64x2 a2 = __builtin_bit_cast(i64x2, a[i]), b2 = __builtin_bit_cast(i64x2, b[j]);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a2[0], b2[0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a2[1], b2[1], acc[i][j], 0, 0, 0);
      } else
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[i]),
                                                            __builtin_bit_cast(bf16x8, b[j]), acc[i][j], 0, 0, 0);
    }
}

// ---- hand-scheduled k-tile ----------------------------------------------------------------------------
// The compiler waits lgkmcnt(0) after every group of fragment reads, so a read issued for the NEXT
// k-step stalls the MFMAs of the current one.  Here the ds_read_b128 are inline asm (invisible to
// the compiler's wait-count pass) with counted waits: the 6 reads of k-step ks+1 stay in flight
// while the 8 MFMAs of ks execute.  The "+v" ties make every MFMA depend on the wait that covers
// its operands.
template <int IMM>
__device__ __forceinline__ i32x4 lds_read_b128(unsigned addr) {
  i32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(IMM) : "memory");
  return v;
}
template <int N, class C>
__device__ __forceinline__ void lgkm_wait_tied(i32x4 (&a)[C::MI], i32x4 (&b)[C::NI]) {
  static_assert(C::MI == 4 && C::NI == 2, "operand list below is written for a 128x64 wave tile");
  asm volatile("s_waitcnt lgkmcnt(%6)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1])
               : "n"(N)
               : "memory");
}
template <class C>
__device__ __forceinline__ void gemm_read_frags(i32x4 (&a)[C::MI], i32x4 (&b)[C::NI], unsigned addrA,
                                                unsigned addrB) {
  a[0] = lds_read_b128<0 * 4096>(addrA); a[1] = lds_read_b128<1 * 4096>(addrA);
  a[2] = lds_read_b128<2 * 4096>(addrA); a[3] = lds_read_b128<3 * 4096>(addrA);
  b[0] = lds_read_b128<0 * 4096>(addrB); b[1] = lds_read_b128<1 * 4096>(addrB);
}
// `mid(pos)` is called at every issue position of the k-tile: -1 behind the first fragment reads, 0 / 1 / 2 behind the MFMAs of
// that k-step (the next reads in flight across it).  The waves that issue the next k-tile's LDS-DMA inside the compute phase
// instead of before their first MFMA do it at position MSAE_GEMM_STAGGER_AT (gemm_kernel: stagger)
template <class C, class F>
__device__ __forceinline__ void gemm_compute_asm32(f32x16 (&acc)[C::MI][C::NI], const unsigned char *sA,
                                                   int wr, int wc, int lane, F &&mid) {
  static_assert(C::KS == 4, "four k-steps per tile");
  const int l31 = lane & 31, kh = lane >> 5;
  const unsigned base = (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char *)sA;
  const unsigned rowA = base + (unsigned)(wr * C::TM + l31) * 128u;
  const unsigned rowB = base + (unsigned)C::A_BYTES + (unsigned)(wc * C::TN + l31) * 128u;
  const unsigned sw = (unsigned)gemm_swz(l31);       // same swizzle for every 32-row block of A and B
  unsigned off[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) off[ks] = (((unsigned)(ks * 2 + kh)) ^ sw) << 4;
  i32x4 a0[C::MI], b0[C::NI], a1[C::MI], b1[C::NI];
  gemm_read_frags<C>(a0, b0, rowA + off[0], rowB + off[0]);
  gemm_read_frags<C>(a1, b1, rowA + off[1], rowB + off[1]);
  mid(-1);                         // (behind the first reads, in front of the first MFMA: measured worse than any other position)
  lgkm_wait_tied<6, C>(a0, b0);
  gemm_mfma_step<C>(acc, a0, b0);
  gemm_read_frags<C>(a0, b0, rowA + off[2], rowB + off[2]);
  mid(0);
  lgkm_wait_tied<6, C>(a1, b1);
  gemm_mfma_step<C>(acc, a1, b1);
  gemm_read_frags<C>(a1, b1, rowA + off[3], rowB + off[3]);
  mid(1);
  lgkm_wait_tied<6, C>(a0, b0);
  gemm_mfma_step<C>(acc, a0, b0);
  mid(2);
  lgkm_wait_tied<0, C>(a1, b1);
  gemm_mfma_step<C>(acc, a1, b1);
}

// ---- the same k-tile with 16x16x64 MFMAs (C::MF16) ----
// A k-step (64 B of k) is 8 A and 4 B fragments of 16 rows (lane l: row l % 16, 16-B chunk 4 ks + l / 16 -- with the LDS image's
// swizzle (r >> 1) & 7 every ds_read_b128 is conflict-free) and 32 MFMAs.  A whole k-step of fragments is 48 VGPRs, so the tile runs
// in half-steps: A rows 0-63 (block 0) then 64-127 (block 1), each against the 4 B fragments held in registers, B-outer (one B
// fragment across four consecutive MFMAs).  Three 16-VGPR groups: ga = A low half, gc = A high half, gb = B.  Each group is
// refilled for the next k-step as soon as its last MFMA has issued: the A high half of k-step ks in front of half-step (ks, 0), the
// A low half of ks + 1 in front of half-step (ks, 1), B of ks + 1 piecewise behind the four MFMAs of each B fragment in half-step
// (ks, 1).  lgkmcnt counts the wave's outstanding LDS reads in issue order; the "+v" ties make each MFMA depend on the wait that
// covers its operands.  They do not stop MFMAs from moving BELOW a later wait: the compiled order differs from the written one
// (the waits of a half-step come ahead of its first MFMA, and the wait for the A high half of k-step 1 ahead of half-step (1, 0)),
// so a read does not always have 16 MFMAs to land behind; the partner wave on the SIMD covers the rest.  Correctness does not
// depend on the order.
template <int N>
__device__ __forceinline__ void lgkm_wait_tie4(i32x4 (&g)[4]) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]) : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait_tie1(i32x4 &g) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(g) : "n"(N) : "memory");
}
template <int IMM>
__device__ __forceinline__ void gemm_read4(i32x4 (&g)[4], unsigned addr) {   // four fragments 16 rows (2 KiB) apart
  g[0] = lds_read_b128<IMM + 0 * 2048>(addr); g[1] = lds_read_b128<IMM + 1 * 2048>(addr);
  g[2] = lds_read_b128<IMM + 2 * 2048>(addr); g[3] = lds_read_b128<IMM + 3 * 2048>(addr);
}
// half-step on A block h (held in g) against the 4 B fragments; B fragment j is waited for right before its MFMAs
template <class C>
__device__ __forceinline__ void gemm_half_wait_b(f32x16 (&acc)[C::MI][C::NI], int h, i32x4 (&ga)[4], i32x4 (&gb)[4]) {
  lgkm_wait_tie4<7>(ga);   // outstanding in issue order: ga, gb[0..3], the next A group (4)
  lgkm_wait_tie1<7>(gb[0]);
#pragma unroll
  for (int s = 0; s < 4; ++s) gemm_mfma16(acc[h][0], s, ga[s], gb[0]);
  lgkm_wait_tie1<6>(gb[1]);
#pragma unroll
  for (int s = 0; s < 4; ++s) gemm_mfma16(acc[h][1], s, ga[s], gb[1]);
  lgkm_wait_tie1<5>(gb[2]);
#pragma unroll
  for (int s = 0; s < 4; ++s) gemm_mfma16(acc[h][2], s, ga[s], gb[2]);
  lgkm_wait_tie1<4>(gb[3]);
#pragma unroll
  for (int s = 0; s < 4; ++s) gemm_mfma16(acc[h][3], s, ga[s], gb[3]);
}
template <class C, class F>
__device__ __forceinline__ void gemm_compute_asm16(f32x16 (&acc)[C::MI][C::NI], const unsigned char *sA, int wr, int wc,
                                                   int lane, F &&mid) {
  static_assert(C::KS == 2 && C::MI == 2 && C::NI == 4 && C::FA == 8 && C::FB == 4, "written for a 128x64 wave tile");
  const int l15 = lane & 15, kq = lane >> 4;
  const unsigned base = (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char *)sA;
  const unsigned rowA = base + (unsigned)(wr * C::TM + l15) * 128u;
  const unsigned rowB = base + (unsigned)C::A_BYTES + (unsigned)(wc * C::TN + l15) * 128u;
  const unsigned sw = (unsigned)gemm_swz(l15);       // same swizzle for every 16-row block of A and B
  const unsigned off0 = ((unsigned)kq ^ sw) << 4, off1 = ((unsigned)(4 + kq) ^ sw) << 4;
  const unsigned a0 = rowA + off0, b0 = rowB + off0, a1 = rowA + off1, b1 = rowB + off1;
  i32x4 ga[4], gb[4], gc[4];
  gemm_read4<0>(ga, a0);                             // A rows 0-63, k-step 0
  gemm_read4<0>(gb, b0);                             // B, k-step 0
  mid(-1);
  gemm_read4<8192>(gc, a0);                          // A rows 64-127, k-step 0
  gemm_half_wait_b<C>(acc, 0, ga, gb);
  mid(0);
  gemm_read4<0>(ga, a1);                             // A rows 0-63, k-step 1
  lgkm_wait_tie4<4>(gc);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int s = 0; s < 4; ++s) gemm_mfma16(acc[1][j], s, gc[s], gb[j]);
    if (j == 0) gb[0] = lds_read_b128<0 * 2048>(b1);   // B fragment j of k-step 1, once its last MFMA of k-step 0 has issued
    if (j == 1) gb[1] = lds_read_b128<1 * 2048>(b1);
    if (j == 2) gb[2] = lds_read_b128<2 * 2048>(b1);
    if (j == 3) gb[3] = lds_read_b128<3 * 2048>(b1);
  }
  mid(1);
  gemm_read4<8192>(gc, a1);                          // A rows 64-127, k-step 1
  gemm_half_wait_b<C>(acc, 0, ga, gb);
  mid(2);
  lgkm_wait_tie4<0>(gc);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) gemm_mfma16(acc[1][j], s, gc[s], gb[j]);
}
template <class C, class F>
__device__ __forceinline__ void gemm_compute_asm(f32x16 (&acc)[C::MI][C::NI], const unsigned char *sA,
                                                 int wr, int wc, int lane, F &&mid) {
  if constexpr (C::MF16) gemm_compute_asm16<C>(acc, sA, wr, wc, lane, mid);
  else gemm_compute_asm32<C>(acc, sA, wr, wc, lane, mid);
}

// The fragments of k-step ks of the wave tile, compiler-scheduled (outlier tile, ablations): fragment f of A / B is FR = 16 or 32
// tile rows, lane l holds row l % FR and the 16-B chunk l / FR of the k-step's 64 / FR; frag(tile, row, chunk) reads one.
template <class C, class F>
__device__ __forceinline__ void gemm_load_frags(i32x4 (&a)[C::FA], i32x4 (&b)[C::FB], const unsigned char *tA,
                                                const unsigned char *tB, int wr, int wc, int lane, int ks, F &&frag) {
  constexpr int FR = C::MF16 ? 16 : 32;
  const int lr = lane & (FR - 1), chunk = ks * (64 / FR) + lane / FR;
#pragma unroll
  for (int f = 0; f < C::FA; ++f) a[f] = frag(tA, wr * C::TM + f * FR + lr, chunk);
#pragma unroll
  for (int f = 0; f < C::FB; ++f) b[f] = frag(tB, wc * C::TN + f * FR + lr, chunk);
}

// Compact outlier tile (at most 32 outlier dims: one k-step).  The k-loop is bound by the L2 -> LDS delivery, and a
// full 64 KB tile of which 32 B per row carry data is 3 % of an output tile's bytes for nothing: only bytes [0, 32) of
// each 128-B row are staged -- 16 pieces of 32 rows x 32 B, two per wave -- into a dense [512][32 B] image (A rows,
// then B rows) at the head of the slot.
template <class C>
__device__ __forceinline__ void gemm_stage_lead_compact(const unsigned char *__restrict__ Ao,
                                                        const unsigned char *__restrict__ Bo, int m0, int n0,
                                                        unsigned char *lds, int slot, int wave, int lane) {
  static_assert(C::BM == 256 && C::BN == 256 && C::NWAVES == 8, "16 pieces over 8 waves");
  unsigned char *base = lds + slot * C::STAGE_BYTES;
  const unsigned voff = (unsigned)(lane >> 1) * 128u + (unsigned)(lane & 1) * 16u;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int piece = wave * 2 + i;                    // 0..7: A rows 32 piece .., 8..15: B rows
    const bool isA = piece < 8;
    const int pl = isA ? piece : piece - 8;
    const unsigned char *sbase = (isA ? Ao + (size_t)m0 * 128 : Bo + (size_t)n0 * 128) + (size_t)pl * 32 * 128;
    const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)(base + piece * 1024);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :: "v"(voff), "s"(sbase), "s"(dst) : "memory", "m0");
  }
}
template <class C>
__device__ __forceinline__ void gemm_compute_lead_compact(f32x16 (&acc)[C::MI][C::NI], const unsigned char *sA,
                                                          int wr, int wc, int lane) {
  i32x4 a[C::FA], b[C::FB];   // (16x16x64: a fragment spans 64 B of k, the image 32: lanes 32-63 -- chunks 2, 3 -- feed zeros)
  gemm_load_frags<C>(a, b, sA, sA + C::BM * 32, wr, wc, lane, 0, [](const unsigned char *t, int row, int chunk) {
    return chunk < 2 ? *reinterpret_cast<const i32x4 *>(t + row * 32 + chunk * 16) : i32x4{};
  });
  gemm_mfma_step<C>(acc, a, b);
}

// the outlier k-tile: only its first `nks` k-steps of 32 B hold data (32 outlier dims each), the rest is zero
template <class C>
__device__ __forceinline__ void gemm_compute_lead(f32x16 (&acc)[C::MI][C::NI], const unsigned char *sA,
                                                  const unsigned char *sB, int wr, int wc, int lane, int nks) {
  for (int ks = 0; ks < (C::MF16 ? (nks + 1) >> 1 : nks); ++ks) {   // (16x16x64: 64 dims per k-step)
    i32x4 a[C::FA], b[C::FB];
    gemm_load_frags<C>(a, b, sA, sB, wr, wc, lane, ks, [](const unsigned char *t, int row, int chunk) { return gemm_frag(t, row, chunk); });
    gemm_mfma_step<C>(acc, a, b);
  }
}

template <class C>
__device__ __forceinline__ void gemm_compute(f32x16 (&acc)[C::MI][C::NI], const unsigned char *sA,
                                             const unsigned char *sB, int wr, int wc, int lane,
                                             i32x4 (&abl_a)[C::FA], i32x4 (&abl_b)[C::FB]) {
  if constexpr (!C::ABL_NOREAD && !C::ABL_NOMFMA) {
    gemm_compute_asm<C>(acc, sA, wr, wc, lane, [](int) {});
    return;
  }
  // ablation builds only (tools/gemm_sweep): compiler-scheduled reads / no reads / no MFMA
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
    i32x4 a[C::FA], b[C::FB];
    if constexpr (C::ABL_NOREAD) {
#pragma unroll
      for (int f = 0; f < C::FA; ++f) { a[f] = abl_a[f]; asm volatile("" : "+v"(a[f])); }
#pragma unroll
      for (int f = 0; f < C::FB; ++f) { b[f] = abl_b[f]; asm volatile("" : "+v"(b[f])); }
    } else {
      gemm_load_frags<C>(a, b, sA, sB, wr, wc, lane, ks, [](const unsigned char *t, int row, int chunk) { return gemm_frag(t, row, chunk); });
    }
    if constexpr (C::ABL_NOMFMA) {
#pragma unroll
      for (int f = 0; f < C::FA; ++f) asm volatile("" ::"v"(a[f]));
#pragma unroll
      for (int f = 0; f < C::FB; ++f) asm volatile("" ::"v"(b[f]));
    } else {
      gemm_mfma_step<C>(acc, a, b);
    }
  }
}

// append one candidate key to token t's list (segment of this workgroup)
__device__ __forceinline__ void gemm_push_candidate(const GemmEpilogue &ep, int t, unsigned long long key) {
  if (ep.segs > 1) {
    const int sg = (int)(blockIdx.x % (unsigned)ep.segs), scap = ep.cap / ep.segs;
    const int gslot = atomicAdd(ep.cnt + (size_t)t * ep.segs + sg, 1);
    if (gslot < scap) ep.cand[(size_t)t * ep.cap + (size_t)sg * scap + gslot] = key;
  } else {
    const int gslot = atomicAdd(ep.cnt + t, 1);
    if (gslot < ep.cap) ep.cand[(size_t)t * ep.cap + gslot] = key;
  }
}

// feature id of column n of this launch
__device__ __forceinline__ int gemm_feature(const GemmEpilogue &ep, int n) {
  if (ep.skip_stride) {
    const int g = n / (ep.skip_stride - 1), p = n - g * (ep.skip_stride - 1);
    return g * ep.skip_stride + p + (p >= ep.skip_off ? 1 : 0);
  }
  return n * ep.bias_stride + ep.bias_off;
}

// ---- the LDS side buffer: the epilogue constants of one output tile ----------------------------------------------------------
// Seven slots of NT floats behind the ring.  Thread tid < BM owns row tid of the tile, thread BM + c its column c, and slot s
// keeps one word for each of them: [s * NT + row] | [s * NT + BM + col].  Only these two structs know the slot numbers:
//   slot   row t (token)                      column n (feature)
//    0     tau   threshold (THRESH)           bias
//    1     sx    scale                        sw    scale
//    2     m as int             EARLY         Q  \
//    3     P   \  of the band                 Si  } of the band: z^2 sigma^2 = P Q + R (Si + M So)   (gemm_band_sq)
//    4     m as float (M = m^2) /             So /
//    5     B   = z sigma against the reference feature   h  >= sqrt of every ratio to it             (THRESH; file header)
//    6     -E as int            EARLY         Ds = sw_n D_n                                           (subtractive dither, int8)
// GemmSideView is what the epilogue gets: it can name every value above except the two EARLY ones.
template <class C>
class GemmSideView {
 public:
  __device__ __forceinline__ float tau(int row) const { return s[row]; }
  __device__ __forceinline__ float sx(int row) const { return s[C::NT + row]; }
  __device__ __forceinline__ float P(int row) const { return s[3 * C::NT + row]; }
  __device__ __forceinline__ float m(int row) const { return s[4 * C::NT + row]; }
  __device__ __forceinline__ float B(int row) const { return s[5 * C::NT + row]; }
  __device__ __forceinline__ float bias(int col) const { return s[C::BM + col]; }
  __device__ __forceinline__ float sw(int col) const { return s[C::NT + C::BM + col]; }
  __device__ __forceinline__ float Q(int col) const { return s[2 * C::NT + C::BM + col]; }
  __device__ __forceinline__ float Si(int col) const { return s[3 * C::NT + C::BM + col]; }
  __device__ __forceinline__ float So(int col) const { return s[4 * C::NT + C::BM + col]; }
  __device__ __forceinline__ float h(int col) const { return s[5 * C::NT + C::BM + col]; }
  __device__ __forceinline__ float Ds(int col) const { return s[6 * C::NT + C::BM + col]; }

 protected:
  __device__ __forceinline__ explicit GemmSideView(unsigned char *side) : s((__attribute__((address_space(3))) float *)side) {}
  __attribute__((address_space(3))) float *s;   // (typed as LDS: left to address-space inference the THRESH loop took 20 VGPRs more)
};

// The kernels' side: fetch a tile's constants into registers in front of the k-loop, park them behind it (so the epilogue
// never waits on global memory), and the EARLY pair.
template <class C>
class GemmSide : public GemmSideView<C> {
  using GemmSideView<C>::s;
  static constexpr bool DITHER = C::I8 && !C::CERT;   // GemmEpilogue::row_e / col_ds may be set
  static_assert(C::SIDE_BYTES == gemm_side_bytes(C::NT) && C::BM + C::BN <= C::NT, "row part | column part of every slot");
  static_assert(C::LDS_BYTES == C::LDS_RING_BYTES + 7 * C::NT * 4 + 16 + C::QCAP * 8, "ring | side buffer | queue count | queue");
  __device__ __forceinline__ __attribute__((address_space(3))) int *words() const { return (__attribute__((address_space(3))) int *)s; }

 public:
  __device__ __forceinline__ explicit GemmSide(unsigned char *smem) : GemmSideView<C>(smem + C::LDS_RING_BYTES) {}

  // This thread's word of slots 0-4 and 6, and the reference feature (Qr, Sir, Sor) of slot 5
  struct Regs {
    float c0 = 0.f, c1 = 0.f, c3 = 0.f, c4 = 0.f;
    int c2 = 1, c6 = 0;                             // rows: m, +E; columns: the float bits of Q, Ds
    float ref0 = 1.f, ref1 = 1.f, ref2 = 1.f;
  };
  // tile at (m0, n0); rows from T on are padding; has_out: the launch has an outlier tile (int8)
  template <bool DENSE>
  static __device__ __forceinline__ Regs fetch(const GemmEpilogue &ep, int tid, int m0, int n0, int T, bool has_out) {
    Regs r;
    if constexpr (!DENSE) { r.ref0 = ep.refs[0]; r.ref1 = ep.refs[1]; r.ref2 = ep.refs[2]; }
    if (tid < C::BM) {
      const int t = m0 + tid;
      if constexpr (!DENSE) {
        const float v = (t < T) ? ep.tau_vals[(size_t)t * ep.tau_ld + ep.tau_col] : 0.f;
        r.c0 = (v > 0.f) ? v : __builtin_inff();     // degenerate / padded token: emit nothing
      }
      if (t < T) {
        const f32x4 rc = ep.rowc[t];
        r.c1 = rc[0];
        r.c3 = rc[2];
        r.c4 = 1.f;
        if (has_out) { r.c2 = (int)rc[1]; r.c4 = rc[1]; }
        if constexpr (C::CERT || C::F8) r.c4 = rc[1];
        if constexpr (DITHER) {
          if (ep.row_e) { const int2 em = ep.row_e[t]; r.c6 = em.x; r.c2 = em.y; }
        }
      }
    } else if (tid < C::BM + C::BN) {
      const int n = n0 + tid - C::BM;
      r.c0 = ep.bias ? ep.bias[gemm_feature(ep, n)] : 0.f;
      const f32x4 cc = ep.colc[n];
      r.c1 = cc[0];
      r.c2 = __float_as_int(cc[1]);
      r.c3 = cc[2];
      r.c4 = cc[3];
      if constexpr (DITHER) {
        if (ep.col_ds) r.c6 = __float_as_int(ep.col_ds[n]);
      }
    }
    return r;
  }

  // EARLY: m and -E of the rows (acc = acc * m - E right behind the outlier tile) are parked in front of the tile's first barrier,
  // while slower waves of a persistent workgroup may still run the PREVIOUS tile's epilogue.  So they live where no epilogue
  // reads -- the row parts of slots 2 and 6, which GemmSideView cannot name -- and never beside an epilogue input (d74ff0c: as
  // int2 across slot 2 they overwrote Q_n under the slow waves' band computations; verified-and-wrong tokens at N = 262144).
  __device__ __forceinline__ void park_early(int tid, const Regs &r) const {
    if (tid < C::BM) { words()[2 * C::NT + tid] = r.c2; if constexpr (DITHER) words()[6 * C::NT + tid] = -r.c6; }
  }
  __device__ __forceinline__ int early_m(int row) const { return words()[2 * C::NT + row]; }
  __device__ __forceinline__ int early_neg_e(int row) const { return DITHER ? words()[6 * C::NT + row] : 0; }   // (0 without the dither)

  // behind the k-loop: everything the epilogue reads.  Slot 5 is computed only now: the loads it needs had the whole k-loop to land.
  template <bool DENSE>
  __device__ __forceinline__ void park(int tid, const Regs &r, float zz12) const {
    const bool col = tid >= C::BM;                  // (the row parts of slots 2 and 6 are the EARLY pair's)
    s[tid] = r.c0;
    s[C::NT + tid] = r.c1;
    if (col) words()[2 * C::NT + tid] = r.c2;
    s[3 * C::NT + tid] = r.c3;
    s[4 * C::NT + tid] = r.c4;
    if constexpr (DITHER) { if (col) words()[6 * C::NT + tid] = r.c6; }
    if constexpr (!DENSE) {
      float c5 = 0.f;
      if (tid < C::BM) {          // B_t: z sigma of this token against the reference feature
        float b2 = r.c3 * r.ref0;
        if constexpr (C::SCALED) {
          const float rz = r.c1 * r.c1 * zz12;
          b2 = __builtin_fmaf(rz * r.c4 * r.c4, r.ref2, __builtin_fmaf(rz, r.ref1, b2));
        }
        c5 = __builtin_sqrtf(b2) * 1.00001f;
      } else if (tid < C::BM + C::BN) {   // h_n >= sqrt of every ratio to the reference feature (0/0 counts as 0)
        const float q = __int_as_float(r.c2);
        float h2 = q / r.ref0;
        if constexpr (C::SCALED) {
          h2 = fmaxf(h2, r.c3 / r.ref1);
          if (r.c4 > 0.f) h2 = fmaxf(h2, r.c4 / r.ref2);
        }
        c5 = (q > 0.f || r.c3 > 0.f || r.c4 > 0.f) ? __builtin_sqrtf(h2) * 1.00001f : 0.f;
      }
      s[5 * C::NT + tid] = c5;
    }
  }
};

// z^2 sigma^2 of pair (row, col) from the side buffer (same expression as band_sq in encode_fused.hip)
template <class C>
__device__ __forceinline__ float gemm_band_sq(const GemmSideView<C> &side, int row, int col, float zz12) {
  const float pz = side.P(row);
  if constexpr (!C::SCALED) return pz * side.Q(col);
  const float rs = side.sx(row), mf = side.m(row);
  const float rz = rs * rs * zz12;
  return __builtin_fmaf(pz, side.Q(col), __builtin_fmaf(rz * mf * mf, side.So(col), rz * side.Si(col)));
}

// The coarse pre-activation v of accumulator register e (V = float) or registers e, e + 1 (V = f32x2: packed-f32 instructions) of
// one block, for the operand kind of C.  THE definition of v: the candidate audit pins it to a fraction of an f32 rounding.
//   int8            v = (acc sw_n - sw_n D_n) sx_t + b_n   two fmas; nds = -sw_n D_n (0 without the subtractive dither)
//   certified, fp8  v = acc (sx_t sw_n) + b_n
//   bf16            v = acc + b_n
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <class V>
__device__ __forceinline__ V gemm_splat(float x) {
  if constexpr (sizeof(V) == sizeof(float)) return x;
  else return V{x, x};
}
template <class C, class V>
__device__ __forceinline__ V gemm_value(const f32x16 &blk, int e, V sx, float sw, float nds, float bias) {
  V a;
  if constexpr (sizeof(V) == sizeof(float)) {
    if constexpr (C::I8) a = (float)__builtin_bit_cast(i32x16, blk)[e]; else a = blk[e];
  } else {
    if constexpr (C::I8) a = V{(float)__builtin_bit_cast(i32x16, blk)[e], (float)__builtin_bit_cast(i32x16, blk)[e + 1]};
    else a = V{blk[e], blk[e + 1]};
  }
  if constexpr (C::I8 && !C::CERT)
    return __builtin_elementwise_fma(__builtin_elementwise_fma(a, gemm_splat<V>(sw), gemm_splat<V>(nds)), sx, gemm_splat<V>(bias));
  else if constexpr (C::SCALED) return a * (sx * sw) + bias;
  else return a + bias;
}

// Epilogue.  DENSE stores every value.  THRESH compares with the per-token threshold; survivors are
// rare (~1 per 200 outputs pass the hot loop's separable bound) but each needs a slot in its token's
// candidate list, i.e. a RETURNING global atomic (~2 us round trip).  Doing that inline serialises ~30
// round trips per wave -- as long as the whole k-loop.  So survivors are first queued in LDS (its own
// region behind the ring) and then flushed, one queue entry per lane: the global atomics of the whole
// workgroup are in flight together.  The hot loop itself touches no LDS queue: hit masks per accumulator
// block first (4.5 VALU per output), then ONE queue reservation per lane and tile, then the pushes
// (round 3; 15.4k -> 7.8k cycles per tile on the tile timeline, profiles/r03_epilogue_batch.txt --
// worth 0-1 % of wall time only, because the kernel runs at the package power limit: the clock drops
// as the cycle count does, profiles/r03_power.txt).
// Called by every wave of the workgroup with its accumulators, behind GemmSide::park (its first barrier orders the two).
template <class C, bool DENSE>
__device__ __forceinline__ void gemm_epilogue(f32x16 (&acc)[C::MI][C::NI], const GemmEpilogue &ep, int T,
                                              int m0, int n0, int wr, int wc, int lane,
                                              unsigned char *smem, const GemmSideView<C> side, int tl_tile = 0) {
  constexpr int QCAP = C::QCAP;
  unsigned *q_count = reinterpret_cast<unsigned *>(smem + C::LDS_RING_BYTES + C::SIDE_BYTES);
  unsigned long long *queue = reinterpret_cast<unsigned long long *>(smem + C::LDS_RING_BYTES + C::SIDE_BYTES + 16);
  MSAE_PERTURB_AT(GEMM_EPI_ENTER, m0 * 31 + n0);   // this wave's side-buffer words are written: the barrier publishes them and ends the last k-tile's reads
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                        // side buffer written; previous tile's flush done
  MSAE_PERTURB_AT(GEMM_EPI_BEHIND, m0 * 31 + n0);   // the queue count is reset behind the barrier, in front of the first reservation
  if constexpr (!DENSE) {
    if (threadIdx.x == 0) *q_count = 0u;
    __syncthreads();
  }
  MSAE_TL(7);
  // column constants of this lane's NI columns stay in registers across the row loops
  float c_bias[C::NI], c_sw[C::NI], c_h[C::NI];
  float c_ds[C::NI];                                   // -sw_n D_n (subtractive dither; 0 otherwise)
  bool c_live[C::NI];
#pragma unroll
  for (int j = 0; j < C::NI; ++j) {
    const int col = wc * C::TN + C::acc_col(j, lane);  // column inside the tile
    c_bias[j] = side.bias(col);
    c_sw[j] = side.sw(col);
    c_ds[j] = (C::I8 && !C::CERT) ? -side.Ds(col) : 0.f;
    c_h[j] = side.h(col);
    const int feat = gemm_feature(ep, n0 + col);
    c_live[j] = (feat != ep.skip_a) && (feat != ep.skip_b);
  }
  // row / column of register e of block (i, j): C::acc_row / acc_col
  if (msae_tuning::ABL_NOEPI && !DENSE && ep.cap != -12345) { asm volatile("" ::"v"(acc[0][0][0])); } else   // (tuning builds: skip the element loop)
  // THRESH.  One pass over the wave's MI x NI blocks without any LDS round trip: the value v replaces the accumulator in its register,
  // the sign of (v + h_n B_t) - tau goes through a 1-instruction shift register (v_alignbit) into a 16-bit hit mask per block.
  // Then ONE queue reservation per lane for all its hits of this tile, then the pushes (v picked out of the 16 registers
  // by a select tree on the hit's position).
  if constexpr (!DENSE) {
    unsigned hits[C::MI][C::NI];
    // The constants of RG rows are held at a time.  32x32 blocks: all 16 rows of a block.  16x16 blocks: a lane holds 4 column
    // sets (NI = 4) instead of 2, so the 48 row constants of a whole block do not fit beside them; the rows of register group g
    // (e = 4g .. 4g+3) are the same in all four column blocks: 12 row constants at a time, with a scheduling fence per group so
    // that the compiler does not hoist the next groups' LDS loads.
    constexpr int RG = C::MF16 ? 4 : 16;
#pragma unroll
    for (int i = 0; i < C::MI; ++i) {
      unsigned mj[C::NI];
#pragma unroll
      for (int j = 0; j < C::NI; ++j) mj[j] = 0u;
#pragma unroll
      for (int g = 0; g < 16 / RG; ++g) {
        if constexpr (RG < 16) __builtin_amdgcn_sched_barrier(0);
        float tau[RG], rs[RG], bt[RG];
#pragma unroll
        for (int r = 0; r < RG; ++r) {
          const int row = wr * C::TM + C::acc_row(i, RG * g + r, lane);
          tau[r] = side.tau(row);
          rs[r] = C::SCALED ? side.sx(row) : 0.f;
          bt[r] = side.B(row);
        }
#pragma unroll
        for (int j = 0; j < C::NI; ++j) {
          unsigned m = mj[j];
#pragma unroll
          for (int r = 0; r < RG; r += 2) {                                      // two outputs per packed-f32 instruction
            const int e = RG * g + r;
            const f32x2 tau2 = {tau[r], tau[r + 1]}, rs2 = {rs[r], rs[r + 1]}, bt2 = {bt[r], bt[r + 1]};
            const f32x2 v = gemm_value<C, f32x2>(acc[i][j], e, rs2, c_sw[j], c_ds[j], c_bias[j]);
            acc[i][j][e] = v.x;
            acc[i][j][e + 1] = v.y;
            const f32x2 ch2 = {c_h[j], c_h[j]};
            const f32x2 dlt = __builtin_elementwise_fma(ch2, bt2, v) - tau2;      // >= +0 iff the bound reaches tau (NaN: either)
            m = __builtin_amdgcn_alignbit(m, __float_as_uint(dlt.x), 31);        // m = m << 1 | sign(dlt)
            m = __builtin_amdgcn_alignbit(m, __float_as_uint(dlt.y), 31);
          }
          mj[j] = m;
          // bit 15 - e: output e is a hit  (taken here, not in a loop of its own behind the groups: that form spills on 32x32 blocks)
          if (g == 16 / RG - 1) hits[i][j] = c_live[j] ? (~m & 0xFFFFu) : 0u;
        }
      }
      if constexpr (RG < 16) __builtin_amdgcn_sched_barrier(0);
    }
    unsigned total = 0;
#pragma unroll
    for (int i = 0; i < C::MI; ++i)
#pragma unroll
      for (int j = 0; j < C::NI; ++j) total += (unsigned)__builtin_popcount(hits[i][j]);
    if (total) {
      unsigned slot;
      {  // the hardware serialises the lanes of one LDS atomic on one address (asm: the compiler would turn atomicAdd into
         // a scalar loop over the active lanes)
        const unsigned qa = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned *)q_count;
        asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(slot) : "v"(qa), "v"(total) : "memory");
      }
#pragma unroll
      for (int i = 0; i < C::MI; ++i) {
#pragma unroll
        for (int j = 0; j < C::NI; ++j) {
          unsigned h = hits[i][j];
          const int col = wc * C::TN + C::acc_col(j, lane);
          while (h) {
            const int p = 31 - __builtin_clz(h);                                // highest set bit first = lowest e first
            h &= ~(1u << p);
            const int e = 15 - p;
            // v = acc[i][j][e] by a bit-select tree (a ?: tree is turned into a scratch array indexed by e)
            const unsigned b0 = 0u - (e & 1), b1 = 0u - ((e >> 1) & 1), b2 = 0u - ((e >> 2) & 1), b3 = 0u - ((e >> 3) & 1);
            auto sel = [](unsigned mk, unsigned hi, unsigned lo) { return (hi & mk) | (lo & ~mk); };
            unsigned s8[8], s4[4], s2[2];
#pragma unroll
            for (int q = 0; q < 8; ++q) s8[q] = sel(b0, __float_as_uint(acc[i][j][2 * q + 1]), __float_as_uint(acc[i][j][2 * q]));
#pragma unroll
            for (int q = 0; q < 4; ++q) s4[q] = sel(b1, s8[2 * q + 1], s8[2 * q]);
#pragma unroll
            for (int q = 0; q < 2; ++q) s2[q] = sel(b2, s4[2 * q + 1], s4[2 * q]);
            const float v = __uint_as_float(sel(b3, s2[1], s2[0]));
            const int row = wr * C::TM + C::acc_row(i, e, lane);
            if (slot < QCAP) {
              queue[slot] = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)(row << 16 | col);
            } else {                                                            // queue full: slow path
              const float u = v + __builtin_sqrtf(gemm_band_sq<C>(side, row, col, ep.zz12));
              if (u > side.tau(row)) {
                const int t = m0 + row;
                const int feat = gemm_feature(ep, n0 + col);
                gemm_push_candidate(ep, t, rank_key(u, feat));
              }
            }
            ++slot;
          }
        }
      }
    }
  } else {
    // DENSE: every value + its band (32x32 blocks: 128-B runs per 32 lanes; 16x16: 64-B runs per 16 lanes)
#pragma unroll
    for (int i = 0; i < C::MI; ++i) {
#pragma unroll
      for (int j = 0; j < C::NI; ++j) {
        const int col = wc * C::TN + C::acc_col(j, lane);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = wr * C::TM + C::acc_row(i, e, lane), t = m0 + row;
          const float v = gemm_value<C, float>(acc[i][j], e, C::SCALED ? side.sx(row) : 0.f, c_sw[j], c_ds[j], c_bias[j]);
          if (t < T) ep.dense[(size_t)t * ep.ld_dense + n0 + col] = v + __builtin_sqrtf(gemm_band_sq<C>(side, row, col, ep.zz12));
        }
      }
    }
  }
  MSAE_TL(4);
  if constexpr (!DENSE) {
    MSAE_PERTURB_AT(GEMM_EPI_FLUSH, m0 * 31 + n0);   // this wave's pushes are in the LDS queue: the barrier hands them to the flush
    __syncthreads();
    const unsigned nq = msae_tuning::ABL_NOFLUSH ? 0u : (*q_count < QCAP ? *q_count : QCAP);
    for (unsigned q = threadIdx.x; q < nq; q += C::NT) {
      const unsigned long long e = queue[q];
      const int row = (int)((e >> 16) & 0xFFFFu), col = (int)(e & 0xFFFFu);
      const float v = __uint_as_float((unsigned)(e >> 32));
      const float u = v + __builtin_sqrtf(gemm_band_sq<C>(side, row, col, ep.zz12));   // the exact upper value
      if (!(u > side.tau(row))) continue;
      const int t = m0 + row;
      const int feat = gemm_feature(ep, n0 + col);
      gemm_push_candidate(ep, t, rank_key(u, feat));
    }
    MSAE_PERTURB_AT(GEMM_EPI_FLUSHED, m0 * 31 + n0);   // a wave done flushing runs ahead into the next tile while others still read queue and side buffer
  }
  MSAE_TL(5);
}

template <class C, bool DENSE>
__global__ __launch_bounds__(C::NT) void gemm_kernel(GemmOperands op, int T, int Tp, int N, int nM, int nN,
                                                     GemmEpilogue ep) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  // persistent workgroups: the grid is one workgroup per CU (a multiple of 8, so a workgroup's
  // tiles keep its XCD's super-tile affinity) and each walks tile ids blockIdx.x, +gridDim.x, ...
  // The k-tiles of all its output tiles form ONE flat sequence through the 2-slot ring: the last
  // iteration of a tile already stages the first k-tile of the next one, whose latency is then
  // hidden behind the epilogue.
  int seq = 0;                                   // flat k-tile counter; ring slot = seq & 1
  [[maybe_unused]] int tl_tile = -1;
  for (int tile_id = blockIdx.x; tile_id < nM * nN; tile_id += gridDim.x) {
  ++tl_tile;
  MSAE_TL(0);
  MSAE_PERTURB_AT(GEMM_TILE_ENTRY, tile_id);   // a wave starts the next tile while slower ones are still in the previous epilogue
  // the thread id is made opaque per tile: otherwise every lane-dependent address of the
  // prologue and the epilogue is hoisted out of this loop and lives across the k-loop (spills)
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));
  const int lane = tid_ & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid_ >> 6);
  const int wr = wave / C::WN, wc = wave % C::WN;
  int tm, tn;
  gemm_map_tile(tile_id, nM, nN, tm, tn);
  const int m0 = tm * C::BM, n0 = tn * C::BN;
  const bool has_next = tile_id + (int)gridDim.x < nM * nN;
  int m0n = 0, n0n = 0;
  if (has_next) {
    gemm_map_tile(tile_id + gridDim.x, nM, nN, tm, tn);
    m0n = tm * C::BM, n0n = tn * C::BN;
  }

  // Row / column constants of the epilogue: fetched NOW into registers, parked in the LDS side buffer
  // after the k-loop, so the epilogue never waits on global memory.  (Issuing these loads behind the
  // tile's first barrier instead -- so that the first vmcnt(0) does not wait for them -- measured 5 %
  // SLOWER: their address arithmetic then sits between the DMA issue and the first MFMAs of the tile.)
  const bool has_out = C::I8 && op.Ao != nullptr;
  const GemmSide<C> side(smem);
  const typename GemmSide<C>::Regs side_regs = GemmSide<C>::template fetch<DENSE>(ep, tid_, m0, n0, T, has_out);
  [[maybe_unused]] const bool sub_e = C::I8 && !C::CERT && ep.row_e != nullptr;   // wave-uniform
  int lead_ks = 4;
  if (has_out && op.n_out != nullptr) lead_ks = (*op.n_out + 31) >> 5;    // wave-uniform scalar load

  f32x16 acc[C::MI][C::NI];
#pragma unroll
  for (int i = 0; i < C::MI; ++i)
#pragma unroll
    for (int j = 0; j < C::NI; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;   // all-zero bits: also i32 zero

  i32x4 abl_a[C::FA], abl_b[C::FB];
  if constexpr (C::ABL_NOREAD)   // any fragments: the first ones of the tile's rows, straight from global memory
    gemm_load_frags<C>(abl_a, abl_b, op.A + (size_t)m0 * op.ldA, op.B + (size_t)n0 * op.ldB, 0, 0, lane, 0,
                       [&](const unsigned char *t, int row, int chunk) { return *reinterpret_cast<const i32x4 *>(t + (size_t)row * op.ldA + chunk * 16); });

  // tile sequence: [outlier tile (int8, optional)] then the nk main k-tiles
  const int lead = has_out ? 1 : 0;
  const int ntiles = op.nk + lead;
  const GemmStageLane sl_main = gemm_stage_lane(lane, (unsigned)op.ldA);   // ldA == ldB (launcher)
  const GemmStageLane sl_lead = gemm_stage_lane(lane, 128u);
  const bool lead_compact = lead_ks <= 1;                  // wave-uniform (device-side count of outlier dims)
  // ONE row of output tiles (T <= BM): all workgroups read the SAME A tile, and walking its k-tiles in step they ask
  // the same few L2 lines at the same moment.  Integer accumulation does not depend on the order, so each workgroup
  // starts its k-walk at its own k-tile (the 32 workgroups of an XCD at 32 different ones) and wraps around.
  const int krot = (C::I8 && nM == 1 && !C::CERT) ? (int)(gridDim.x >= 64 ? blockIdx.x >> 3 : blockIdx.x) % op.nk : 0;   // (few tiles: the sample pass)
  auto stage = [&](int tm0, int tn0, int tile, int slot) {
    if (tile < lead) {
      if constexpr (C::I8) {
        if (lead_compact) { gemm_stage_lead_compact<C>(op.Ao, op.Bo, tm0, tn0, smem, slot, wave, lane); return; }
      }
      gemm_stage<C>(op.Ao, op.Bo, 128, tm0, tn0, 0, smem, slot, wave, sl_lead);
    } else {
      int kq = tile - lead + krot;                         // (a select, no control flow: see gemm_stage_pieces)
      kq -= kq >= op.nk ? op.nk : 0;
      // tile-major: the wave's share is one contiguous block of ONE operand (gemm_stage_block); only that operand's address is formed
      [[maybe_unused]] const bool wa = wave * C::PPW < C::A_PIECES;                 // wave-uniform
      [[maybe_unused]] const unsigned char *wop = wa ? op.A : op.B;
      [[maybe_unused]] const size_t wrt = (size_t)(wa ? tm0 / C::BM : tn0 / C::BN);
      [[maybe_unused]] const size_t wbytes = wa ? (size_t)C::A_BYTES : (size_t)C::B_BYTES;
      [[maybe_unused]] const size_t win = (size_t)(wave * C::PPW - (wa ? 0 : C::A_PIECES)) * 1024;
      [[maybe_unused]] unsigned char *wdst = smem + slot * C::STAGE_BYTES + wave * C::PPW * 1024;
      if constexpr (C::CERT) {                             // wave-uniform; scalar selects (see GemmOperands::cert)
        const int seg = kq >= 2 * op.cert ? 2 : (kq >= op.cert ? 1 : 0), kk = kq - seg * op.cert;
        const int ia = (seg == 0 ? 0 : op.cert) + kk, ib = (seg == 1 ? 0 : op.cert) + kk;
        if constexpr (GemmWaveBlock<C>::OK)
          gemm_stage_block<C>(wop + (wrt * (2 * op.cert) + (wa ? ia : ib)) * wbytes + win, wdst, lane);
        else
          gemm_stage_packed<C>(op.A + ((size_t)(tm0 / C::BM) * (2 * op.cert) + ia) * C::A_BYTES,
                               op.B + ((size_t)(tn0 / C::BN) * (2 * op.cert) + ib) * C::B_BYTES, smem, slot, wave, lane);
        return;
      }
      if (op.packed) {                                     // wave-uniform
        if constexpr (GemmWaveBlock<C>::OK)
          gemm_stage_block<C>(wop + (wrt * op.nk + kq) * wbytes + win, wdst, lane);
        else
          gemm_stage_packed<C>(op.A + ((size_t)(tm0 / C::BM) * op.nk + kq) * C::A_BYTES,
                               op.B + ((size_t)(tn0 / C::BN) * op.nk + kq) * C::B_BYTES, smem, slot, wave, lane);
      } else
        gemm_stage<C>(op.A, op.B, op.ldA, tm0, tn0, (size_t)kq * C::ROWB, smem, slot, wave, sl_main);
    }
  };
  if (tile_id == (int)blockIdx.x) {   // later tiles: staged by their predecessor
    stage(m0, n0, 0, 0);
  }

  auto iteration = [&](int kt, bool park_m = false) {
    MSAE_TLK(kt == 8, 0);
    MSAE_TLK(kt == 9, 5);
    wait_vmcnt<0>();               // this wave's pieces of k-tile kt (and the side constants) landed
    if (park_m) {                  // outlier multipliers (and -E) of the tile's rows -> LDS (read after this k-tile)
      MSAE_PERTURB_AT(GEMM_PARK_EARLY, tile_id);   // the EARLY pair is written while the previous tile's epilogue may still read the side buffer
      side.park_early(tid_, side_regs);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    MSAE_TLK(kt == 8, 1);
    MSAE_PERTURB_AT_K(GEMM_KTILE_BARRIER, seq);   // this wave's pieces have landed: the barrier is all that publishes them to the others
    __builtin_amdgcn_s_barrier();  // ... and everybody's; the other slot is free again
    MSAE_TLK(kt == 8, 2);
    if (kt == 0) MSAE_TL(1);
    if (kt == 1) MSAE_TL(2);
    auto stage_next = [&]() {
      if (kt + 1 < ntiles) stage(m0, n0, kt + 1, (seq + 1) & 1);
      else if (has_next) stage(m0n, n0n, 0, (seq + 1) & 1);
    };
    // (MSAE_GEMM_STAGGER, tuning.h: on by default since round 3 -- -4 % on the main pass together with tile-major operands, two
    // boxes: profiles/r03_ab_stagger_tile_major.txt, r03_ab_ring64_spilling_build.txt; 0 = off, 2 = odd waves)
    // Waves w and w + 4 share a SIMD.  If both issue their LDS-DMA pieces right behind the barrier the SIMD's MFMA pipe idles
    // for that long in every k-tile; so the upper four waves start with MFMAs on the data already in LDS and issue their pieces
    // behind k-step MSAE_GEMM_STAGGER_AT, while their partners -- done issuing -- keep the pipe busy.  ONE copy of the MFMA
    // code: the two roles differ only in which of the two stage_next() call sites is taken.  (Round 3, ~700 cycles of issue per
    // wave: behind k-step 1.  Round 5, one block per wave = ~100 cycles: behind k-step 0 -- the pieces' time to land is what
    // counts now; behind k-step 2 costs 9 %, everybody at the top 2 %: profiles/r05_ab_stagger_at.txt.)
    const bool late = MSAE_GEMM_STAGGER != 0 && (MSAE_GEMM_STAGGER == 2 ? (wave & 1) != 0 : wave >= C::NWAVES / 2) && !park_m && nM > 1;
    if constexpr (!C::ABL_NOSTAGE) {
      if (!late) {
        MSAE_PERTURB_AT_K(GEMM_STAGE_EARLY, seq);   // the slot staged into was read in the previous k-tile: only the barrier frees it
        stage_next();
      }
    }
    MSAE_TLK(kt == 8, 3);
    const unsigned char *sA = smem + (seq & 1) * C::STAGE_BYTES;
    if (park_m) {
      if (lead_compact) { if (lead_ks > 0) { if constexpr (C::I8) gemm_compute_lead_compact<C>(acc, sA, wr, wc, lane); } }
      else gemm_compute_lead<C>(acc, sA, sA + C::A_BYTES, wr, wc, lane, lead_ks);
    }
    else if constexpr (!C::ABL_NOREAD && !C::ABL_NOMFMA && !C::ABL_NOSTAGE)
      gemm_compute_asm<C>(acc, sA, wr, wc, lane, [&](int pos) {
        if (late && pos == MSAE_GEMM_STAGGER_AT) {
          MSAE_PERTURB_AT_K(GEMM_STAGE_LATE, seq);   // the staggered waves stage into the free slot from inside the compute phase
          stage_next();
        }
      });
    else gemm_compute<C>(acc, sA, sA + C::A_BYTES, wr, wc, lane, abl_a, abl_b);
    MSAE_TLK(kt == 8, 4);
    ++seq;
  };
  auto scale_by_m = [&]() {
    // |acc| <= 128 * 127 * 127 < 2^21 here and m <= 1040 (quant_x_kernel clamps and hands larger multipliers' tokens to the exact
    // path): the full-rate 24-bit multiply is exact and the product fits int32
    // (v_mul_lo_u32 is quarter rate: 128 of them per lane cost ~2 us per tile)
#pragma unroll
    for (int i = 0; i < C::MI; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wr * C::TM + C::acc_row(i, e, tid_ & 63);
        const int m = side.early_m(row), ee = side.early_neg_e(row);   // one v_mad_i32_i24 per accumulator with or without -E
#pragma unroll
        for (int j = 0; j < C::NI; ++j) {
          i32x16 v = __builtin_bit_cast(i32x16, acc[i][j]);
          v[e] = __mul24(v[e], m) + ee;
          acc[i][j] = __builtin_bit_cast(f32x16, v);
        }
      }
  };
  int kt0 = 0;
  if constexpr (C::I8) {
    if (has_out) {   // peeled: the outlier dims were quantised at scale m[t]*sx[t]
      iteration(0, true);
      kt0 = 1;
      if (lead_ks > 0 || sub_e) scale_by_m();   // no outlier dim in this batch: the accumulators are still zero (sub_e: they become -E)
    }
  }
  if constexpr (C::CERT) {
    const int cut = 2 * op.cert;                     // (no outlier tile in this mode: kt0 == 0)
    for (int kt = kt0; kt < cut; ++kt) iteration(kt);
    // the low-order segments are done: acc = round(acc / 128), an arithmetic shift (|acc| < 2^31: encode_cert.h)
#pragma unroll
    for (int i = 0; i < C::MI; ++i)
#pragma unroll
      for (int j = 0; j < C::NI; ++j) {
        i32x16 v = __builtin_bit_cast(i32x16, acc[i][j]);
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = (v[e] + 64) >> 7;
        acc[i][j] = __builtin_bit_cast(f32x16, v);
      }
    for (int kt = cut; kt < ntiles; ++kt) iteration(kt);
  } else {
    for (int kt = kt0; kt < ntiles; ++kt) iteration(kt);
  }

  MSAE_TL(3);
  MSAE_PERTURB_AT(GEMM_SIDE_PARK, tile_id);   // the side buffer is rewritten: every wave has left the previous epilogue's flush (k-tile barriers)
  side.template park<DENSE>(tid_, side_regs, ep.zz12);
  // behind the epilogue's first barrier every wave is done with the last k-tile's slot: the next tile's first main
  // k-tile lands there while the epilogue runs (its outlier tile is already in the other slot)
  gemm_epilogue<C, DENSE>(acc, ep, T, m0, n0, wr, wc, lane, smem, side, tl_tile);
  MSAE_TL(6);
  MSAE_PERTURB_AT(GEMM_TILE_EXIT, tile_id);   // the waves leave a tile apart: the next tile's entry and EARLY park meet this one's flush
  }
}

// Host launcher.  Requires Tp % BM == 0 and N % BN == 0 (checked by the caller's plan).
template <class C, bool DENSE>
inline int gemm_launch(const GemmOperands &op, int T, int Tp, int N, const GemmEpilogue &ep, hipStream_t s) {
  if (Tp % C::BM || N % C::BN || op.nk <= 0 || op.ldA != op.ldB || op.ldA % 128 || op.packed > 1) return MSAE_EINVAL;
  if ((op.cert != 0) != C::CERT) return MSAE_EINVAL;
  if (C::CERT && (!C::I8 || op.cert < 0 || op.nk != 3 * op.cert || op.packed != 1 || op.Ao != nullptr)) return MSAE_EINVAL;
  const int nM = Tp / C::BM, nN = N / C::BN;
  auto kern = gemm_kernel<C, DENSE>;
  MSAE_HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
  static int n_cu = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus > 8 ? cus / 8 * 8 : 8;
  }();
  const char *np_env = getenv("MSAE_GEMM_NONPERSISTENT");
  const int per_cu = C::LDS_BYTES > 80 * 1024 ? 1 : 2;
  const int grid = msae_tuning::grid_cap((np_env || nM * nN <= n_cu * per_cu) ? nM * nN : n_cu * per_cu);
  MSAE_PERTURB_LAUNCH(DENSE ? 0 : 1, nM * nN, grid);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(C::NT), C::LDS_BYTES, s, op, T, Tp, N, nM, nN, ep);
  return (int)hipGetLastError();
}
