// gemm4w.hip -- standalone prototype (not part of the product): the candidate GEMM's k-loop with FOUR waves per CU
// (2 x 2, 128 x 128 per wave, 256 accumulator registers each) and REGISTER staging (global_load_dwordx4 -> VGPR ->
// ds_write_b128) instead of LDS-DMA.  tools/dma_depth.hip measured the register path delivering 58 GB/s per CU against
// 43.5 for LDS-DMA at the same depth; this asks what a full k-loop makes of it.  int8, 256 x 256 x 128-byte k-tiles,
// 2-slot LDS ring, T=8192 N=131072 d=4096; prints us per k-tile and checks a few outputs against a naive reference.
// Variants 7-11 (gemm4w_dma_kernel) are the same four waves with the PRODUCT's LDS-DMA staging and 16x16x64 MFMAs
// (profiles/gemm_wave_tile.txt).  G4W_ONLY=<variant> runs one of them G4W_REPS times, G4W_N sets N, G4W_SIGMA the operands,
// G4W_READY=1 prints "ready" in front of the timed launches (tools/smi_sample.sh).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/gemm4w.hip -o tools/bin/gemm4w
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "../multimodal-sae_amd/csrc/gemm_mfma.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

template <int SETS>
__global__ __launch_bounds__(256) void gemm4w_kernel(const unsigned char *__restrict__ A, const unsigned char *__restrict__ B,
                                                     size_t ld, int nM, int nN, int nk, int *__restrict__ out, int N) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  constexpr int SLOT = 512 * 128, PPW = 16;            // 64 pieces of 8 rows x 128 B per k-tile, 16 per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, kh = lane >> 5;
  const int r_in = lane >> 3, c_in = lane & 7;
  auto fetch = [&](int tm, int tn, int kt, v4i (&r)[PPW]) {
#pragma unroll
    for (int p = 0; p < PPW; ++p) {
      const int piece = wave * PPW + p;                  // 0..31 A rows, 32..63 B rows
      const bool isA = piece < 32;
      const int row = (isA ? tm * 256 : tn * 256) + (piece & 31) * 8 + r_in;
      r[p] = *reinterpret_cast<const v4i *>((isA ? A : B) + (size_t)row * ld + (size_t)kt * 128 + c_in * 16);
    }
  };
  auto put = [&](int slot, const v4i (&r)[PPW]) {
#pragma unroll
    for (int p = 0; p < PPW; ++p) {
      const int piece = wave * PPW + p;
      const int row = (piece & 31) * 8 + r_in;         // row inside its operand tile
      unsigned char *tile = smem + slot * SLOT + (piece < 32 ? 0 : 256 * 128);
      *reinterpret_cast<v4i *>(tile + row * 128 + ((c_in ^ gemm_swz(row)) << 4)) = r[p];
    }
  };
  for (int tile_id = blockIdx.x; tile_id < nM * nN; tile_id += gridDim.x) {
    int tm, tn;
    gemm_map_tile(tile_id, nM, nN, tm, tn);
    v16i acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
    v4i ra[PPW], rb[PPW];
    fetch(tm, tn, 0, ra);
    put(0, ra);
    if (nk > 1) fetch(tm, tn, 1, ra);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      if (SETS == 2 && kt + 2 < nk) fetch(tm, tn, kt + 2, (kt & 1) ? ra : rb);     // two k-tiles in flight
      const unsigned char *sA = smem + (kt & 1) * SLOT, *sB = sA + 256 * 128;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        v4i a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = gemm_frag(sA, wr * 128 + i * 32 + l31, ks * 2 + kh);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = gemm_frag(sB, wc * 128 + j * 32 + l31, ks * 2 + kh);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      if (kt + 1 < nk) {
        if (SETS == 2) put((kt + 1) & 1, (kt & 1) ? rb : ra);
        else { put((kt + 1) & 1, ra); if (kt + 2 < nk) fetch(tm, tn, kt + 2, ra); }
      }
      __syncthreads();
    }
    // checksum of the tile's accumulators (keeps them live) + a few outputs for the correctness check
    int s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) s ^= acc[i][j][e];
    if (s == 0x7fffffff) out[0] = s;
    if (tile_id < 2 && lane == 0) {   // C[row][col]: col = l31, row = (e&3) + 8*(e>>2) + 4*kh  -> row 0 col 0 of block (i, j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[16 + tile_id * 64 + wave * 16 + i * 4 + j] = acc[i][j][0];
    }
  }
}

// ---- hand-scheduled variant: asm ds_read / ds_write / waits with counted lgkmcnt and vmcnt ---------------------------
template <int IMM> __device__ __forceinline__ v4i ldsr(unsigned addr) {
  v4i v; asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(IMM) : "memory"); return v;
}
__device__ __forceinline__ void ldsw(unsigned addr, const v4i &v) {
  asm volatile("ds_write_b128 %0, %1" :: "v"(addr), "v"(v) : "memory");
}
template <int N> __device__ __forceinline__ void lgkm_tied(v4i (&a)[4], v4i (&b)[4]) {
  asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void vm_tied8(v4i *r) {
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "n"(N) : "memory");
}
__device__ __forceinline__ void rd8(v4i (&a)[4], v4i (&b)[4], unsigned ra, unsigned rb) {
  a[0] = ldsr<0>(ra); a[1] = ldsr<4096>(ra); a[2] = ldsr<8192>(ra); a[3] = ldsr<12288>(ra);
  b[0] = ldsr<0>(rb); b[1] = ldsr<4096>(rb); b[2] = ldsr<8192>(rb); b[3] = ldsr<12288>(rb);
}
__device__ __forceinline__ void mfma16(v16i (&acc)[4][4], const v4i (&a)[4], const v4i (&b)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
}

__global__ __launch_bounds__(256) void gemm4w_sched_kernel(const unsigned char *__restrict__ A, const unsigned char *__restrict__ B,
                                                           size_t ld, int nM, int nN, int nk, int *__restrict__ out, int N) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  constexpr int SLOT = 512 * 128, PPW = 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, kh = lane >> 5;
  const int r_in = lane >> 3, c_in = lane & 7;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  // fragment read addresses (slot 0): row base + swizzled chunk of k-step ks
  const unsigned sw = (unsigned)gemm_swz(l31);
  unsigned offk[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) offk[ks] = (((unsigned)(ks * 2 + kh)) ^ sw) << 4;
  const unsigned rowA = lds0 + (unsigned)(wr * 128 + l31) * 128u, rowB = lds0 + 256u * 128u + (unsigned)(wc * 128 + l31) * 128u;
  // staging: piece p of this wave = rows (piece & 31) * 8 + r_in of A (piece < 32) or B
  unsigned wdst[PPW];
#pragma unroll
  for (int p = 0; p < PPW; ++p) {
    const int piece = wave * PPW + p, row = (piece & 31) * 8 + r_in;
    wdst[p] = lds0 + (piece < 32 ? 0u : 256u * 128u) + (unsigned)row * 128u + (unsigned)((c_in ^ gemm_swz(row)) << 4);
  }
  const bool stA = wave < 2;                              // waves 0,1 stage A rows, waves 2,3 B rows (16 pieces = 128 rows each)
  for (int tile_id = blockIdx.x; tile_id < nM * nN; tile_id += gridDim.x) {
    int tm, tn;
    gemm_map_tile(tile_id, nM, nN, tm, tn);
    const unsigned char *src0 = (stA ? A + (size_t)(tm * 256 + (wave & 1) * 128 + r_in) * ld
                                     : B + (size_t)(tn * 256 + (wave & 1) * 128 + r_in) * ld) + c_in * 16;
    v16i acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
    v4i rg[PPW];
    auto fetch8 = [&](int kt, int half) {
#pragma unroll
      for (int p = 0; p < 8; ++p)
        rg[half * 8 + p] = *reinterpret_cast<const v4i *>(src0 + (size_t)(half * 8 + p) * 8 * ld + (size_t)kt * 128);
    };
    // prologue: tile 0 -> slot 0, tile 1 in flight
    fetch8(0, 0); fetch8(0, 1);
#pragma unroll
    for (int p = 0; p < PPW; ++p) ldsw(wdst[p], rg[p]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (nk > 1) { fetch8(1, 0); fetch8(1, 1); }
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nk; ++kt) {
      const unsigned so = (unsigned)(kt & 1) * SLOT, sn = (unsigned)((kt + 1) & 1) * SLOT;
      const bool more = kt + 1 < nk, more2 = kt + 2 < nk;
      v4i a0[4], b0[4], a1[4], b1[4];
      rd8(a0, b0, rowA + so + offk[0], rowB + so + offk[0]);
      rd8(a1, b1, rowA + so + offk[1], rowB + so + offk[1]);
      lgkm_tied<8>(a0, b0);
      mfma16(acc, a0, b0);
      if (more) {                                          // first half of the next tile -> LDS
        vm_tied8<8>(rg);
#pragma unroll
        for (int p = 0; p < 8; ++p) ldsw(wdst[p] + sn, rg[p]);
      }
      rd8(a0, b0, rowA + so + offk[2], rowB + so + offk[2]);
      if (more) lgkm_tied<15>(a1, b1); else lgkm_tied<8>(a1, b1);
      mfma16(acc, a1, b1);
      if (more) {
        vm_tied8<0>(rg + 8);
#pragma unroll
        for (int p = 8; p < PPW; ++p) ldsw(wdst[p] + sn, rg[p]);
      }
      rd8(a1, b1, rowA + so + offk[3], rowB + so + offk[3]);
      if (more) lgkm_tied<15>(a0, b0); else lgkm_tied<8>(a0, b0);     // (first 8 writes and) k-step 2 fragments landed
      if (more2) fetch8(kt + 2, 0);                        // their registers are free: the first 8 writes have completed
      mfma16(acc, a0, b0);
      lgkm_tied<0>(a1, b1);
      if (more2) fetch8(kt + 2, 1);
      mfma16(acc, a1, b1);
      __builtin_amdgcn_s_barrier();
    }
    int s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) s ^= acc[i][j][e];
    if (s == 0x7fffffff) out[0] = s;
    if (tile_id < 2 && lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[16 + tile_id * 64 + wave * 16 + i * 4 + j] = acc[i][j][0];
    }
    __builtin_amdgcn_s_barrier();
  }
}

// ---- v2: accumulators pinned to physical AGPRs (tools/gemm4w_asm.inc), every memory op and wait in inline asm, two
// staging sets (two k-tiles of loads in flight), branch-free steady state (the loop is unrolled by two) ----------------
#include "gemm4w_asm.inc"
__device__ __forceinline__ v4i gld(const unsigned char *p) {
  v4i v; asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory"); return v;
}
__device__ __forceinline__ void vm_wait16_tied(v4i (&r)[16]) {
  asm volatile("s_waitcnt vmcnt(16)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]),
               "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15]) :: "memory");
}
__device__ __forceinline__ void vm_wait0_tied(v4i (&r)[16]) {
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]),
               "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15]) :: "memory");
}
template <int IMM> __device__ __forceinline__ void ldsw_i(unsigned addr, const v4i &v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(addr), "v"(v), "n"(IMM) : "memory");
}

template <int MODE>   // 0: the kernel; 1: no staging in the loop (timing only: stale data); 2: no loads, writes only (timing only)
__global__ __launch_bounds__(256) void gemm4w_v2_kernel(const unsigned char *__restrict__ A, const unsigned char *__restrict__ B,
                                                        size_t ld, int nM, int nN, int nk, int *__restrict__ out, int N) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  constexpr unsigned SLOT = 512 * 128;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, kh = lane >> 5;
  const int r_in = lane >> 3, c_in = lane & 7;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  const unsigned sw = (unsigned)gemm_swz(l31);
  unsigned offk[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) offk[ks] = (((unsigned)(ks * 2 + kh)) ^ sw) << 4;
  const unsigned rowA = lds0 + (unsigned)(wr * 128 + l31) * 128u, rowB = lds0 + 256u * 128u + (unsigned)(wc * 128 + l31) * 128u;
  // this wave stages 128 consecutive rows of one operand: waves 0,1 -> A rows 0-127 / 128-255, waves 2,3 -> B.  Piece p
  // = rows 8 p .. 8 p + 7 of that range; its LDS image: row * 128 + swizzled chunk.  swz(row + 8) = swz(row) ^ 4, so odd
  // pieces flip chunk bit 2 (two write addresses, immediate offsets p * 1024 for the rest)
  const unsigned wbase = lds0 + (wave >= 2 ? 256u * 128u : 0u) + (unsigned)((wave & 1) * 128 + r_in) * 128u;
  const unsigned wev = wbase + (unsigned)((c_in ^ gemm_swz(r_in)) << 4), wod = wbase + (unsigned)((c_in ^ gemm_swz(r_in + 8)) << 4);
  for (int tile_id = blockIdx.x; tile_id < nM * nN; tile_id += gridDim.x) {
    int tm, tn;
    gemm_map_tile(tile_id, nM, nN, tm, tn);
    const unsigned char *src = (wave < 2 ? A + (size_t)(tm * 256 + (wave & 1) * 128 + r_in) * ld
                                         : B + (size_t)(tn * 256 + (wave & 1) * 128 + r_in) * ld) + c_in * 16;
    const size_t pstride = 8 * ld;
    g4w_zero();
    v4i sa[16], sb[16];
    auto fetch = [&](v4i (&r)[16], int kt) {
      const unsigned char *p = src + (size_t)kt * 128;
#pragma unroll
      for (int q = 0; q < 16; ++q) r[q] = gld(p + q * pstride);
    };
    auto put4 = [&](const v4i (&r)[16], unsigned so, auto grp) {       // pieces 4 g .. 4 g + 3 of the set -> slot at so
      constexpr int g = decltype(grp)::value;
      ldsw_i<(4 * g + 0) * 1024>(wev + so, r[4 * g + 0]); ldsw_i<(4 * g + 1) * 1024>(wod + so, r[4 * g + 1]);
      ldsw_i<(4 * g + 2) * 1024>(wev + so, r[4 * g + 2]); ldsw_i<(4 * g + 3) * 1024>(wod + so, r[4 * g + 3]);
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
    // Software-pipelined body of one k-tile.  On entry the fragments of k-steps 0 and 1 of slot `so` are in flight in
    // (a0, b0) / (a1, b1).  Six groups of 8 MFMAs carry the staging (3 pieces each: wait for them in `ws` -- vmcnt(13):
    // 13 - 3g older loads of the set + the 3g of this iteration are younger --, write them to slot `sn`, issue the
    // same pieces' loads of the k-tile after next into `fs`); then every LDS op of the wave is waited for, the
    // barrier publishes slot `sn`, and the NEXT k-tile's first fragments are read while the last 16 MFMAs run.
    // STAGE 2: write + fetch, 1: write only, 0: neither; LAST: no next k-tile to read ahead
    v4i a0[4], b0[4], a1[4], b1[4];
    auto body = [&](unsigned so, unsigned sn, v4i (&ws)[16], v4i (&fs)[16], int kt, auto stage_tag, auto last_tag) {
      constexpr int STAGE = decltype(stage_tag)::value;
      constexpr bool LAST = decltype(last_tag)::value != 0;
      const unsigned char *fp = src + (size_t)(kt + 2) * 128;
      auto piece = [&](auto qtag) {
        constexpr int q = decltype(qtag)::value;
        if constexpr (STAGE >= 1) ldsw_i<q * 1024>((q & 1 ? wod : wev) + sn, ws[q]);
        if constexpr (STAGE == 2) fs[q] = gld(fp + (size_t)q * pstride);
      };
      auto stage3 = [&](auto gtag) {
        constexpr int g = decltype(gtag)::value;
        if constexpr (g < 5) {
          if constexpr (STAGE == 2) asm volatile("s_waitcnt vmcnt(13)" : "+v"(ws[3 * g]), "+v"(ws[3 * g + 1]), "+v"(ws[3 * g + 2]) :: "memory");
          else if constexpr (STAGE == 1) asm volatile("s_waitcnt vmcnt(0)" : "+v"(ws[3 * g]), "+v"(ws[3 * g + 1]), "+v"(ws[3 * g + 2]) :: "memory");
          piece(std::integral_constant<int, 3 * g>()); piece(std::integral_constant<int, 3 * g + 1>());
          piece(std::integral_constant<int, 3 * g + 2>());
        } else {
          if constexpr (STAGE == 2) asm volatile("s_waitcnt vmcnt(15)" : "+v"(ws[15]) :: "memory");
          else if constexpr (STAGE == 1) asm volatile("s_waitcnt vmcnt(0)" : "+v"(ws[15]) :: "memory");
          piece(std::integral_constant<int, 15>());
        }
      };
      using G0 = std::integral_constant<int, 0>; using G1 = std::integral_constant<int, 1>; using G2 = std::integral_constant<int, 2>;
      using G3 = std::integral_constant<int, 3>; using G4 = std::integral_constant<int, 4>; using G5 = std::integral_constant<int, 5>;
      // younger than the k-step-0 fragments at this point: the 8 reads of k-step 1
      lgkm_tied<8>(a0, b0);
      g4w_mfma8_0(a0[0], a0[1], b0); stage3(G0());
      g4w_mfma8_1(a0[2], a0[3], b0); stage3(G1());
      rd8(a0, b0, rowA + so + offk[2], rowB + so + offk[2]);
      if constexpr (STAGE >= 1) lgkm_tied<14>(a1, b1); else lgkm_tied<8>(a1, b1);     // younger: 6 writes + 8 reads
      g4w_mfma8_0(a1[0], a1[1], b1); stage3(G2());
      g4w_mfma8_1(a1[2], a1[3], b1); stage3(G3());
      rd8(a1, b1, rowA + so + offk[3], rowB + so + offk[3]);
      if constexpr (STAGE >= 1) lgkm_tied<14>(a0, b0); else lgkm_tied<8>(a0, b0);
      g4w_mfma8_0(a0[0], a0[1], b0); stage3(G4());
      g4w_mfma8_1(a0[2], a0[3], b0); stage3(G5());
      lgkm_tied<0>(a1, b1);                              // k-step 3 fragments AND every write of this wave
      __builtin_amdgcn_s_barrier();                      // slot sn complete; nobody reads slot so any more after k-step 3's reads
      if constexpr (!LAST) rd8(a0, b0, rowA + sn + offk[0], rowB + sn + offk[0]);
      g4w_mfma8_0(a1[0], a1[1], b1);
      g4w_mfma8_1(a1[2], a1[3], b1);
      if constexpr (!LAST) rd8(a1, b1, rowA + sn + offk[1], rowB + sn + offk[1]);
    };
    using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>; using S2 = std::integral_constant<int, 2>;
    // prologue: k-tile 0 -> slot 0, k-tile 1 in flight in sa, k-steps 0 / 1 of slot 0 in flight
    fetch(sa, 0);
    vm_wait0_tied(sa);
    put4(sa, 0u, I0()); put4(sa, 0u, I1()); put4(sa, 0u, I2()); put4(sa, 0u, I3());
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    fetch(sa, 1);
    __builtin_amdgcn_s_barrier();
    rd8(a0, b0, rowA + offk[0], rowB + offk[0]);
    rd8(a1, b1, rowA + offk[1], rowB + offk[1]);
    int kt = 0;
    using SM = std::integral_constant<int, MODE == 0 ? 2 : (MODE == 1 ? 0 : 1)>;
    if constexpr (MODE == 3) {                         // MFMAs only: no fragment reads, no barrier, no staging (timing only)
      lgkm_tied<0>(a0, b0); lgkm_tied<0>(a1, b1);
      for (; kt + 3 < nk; kt += 2) {
#pragma unroll
        for (int rep = 0; rep < 4; ++rep) {
          g4w_mfma8_0(a0[0], a0[1], b0); g4w_mfma8_1(a0[2], a0[3], b0);
          g4w_mfma8_0(a1[0], a1[1], b1); g4w_mfma8_1(a1[2], a1[3], b1);
        }
      }
    } else
    for (; kt + 3 < nk; kt += 2) {                     // nk even: pairs (sa = next, sb = after next), then swapped
      body(0u, SLOT, sa, sb, kt, SM(), S0());
      body(SLOT, 0u, sb, sa, kt + 1, SM(), S0());
    }
    body(0u, SLOT, sa, sb, kt, S1(), S0());             // kt = nk - 2: write the last k-tile, nothing left to fetch
    body(SLOT, 0u, sb, sa, kt + 1, S0(), S1());         // kt = nk - 1
    if (tile_id < 2 && lane == 0) {
      int r[16];
#define G4W_OUT(B) g4w_read_##B(r); out[16 + tile_id * 64 + wave * 16 + B] = r[0];
      G4W_OUT(0) G4W_OUT(1) G4W_OUT(2) G4W_OUT(3) G4W_OUT(4) G4W_OUT(5) G4W_OUT(6) G4W_OUT(7)
      G4W_OUT(8) G4W_OUT(9) G4W_OUT(10) G4W_OUT(11) G4W_OUT(12) G4W_OUT(13) G4W_OUT(14) G4W_OUT(15)
#undef G4W_OUT
    }
    __builtin_amdgcn_s_barrier();
  }
}

// ---- v3 ("7" / "8"): the combination the round-4 table never held -- four waves, 128 x 128 wave tiles, the PRODUCT's staging and
// MFMA shape.  Tile-major operands (GemmOperands::packed) travel L2 -> LDS by gemm_stage_block, 16 one-KiB pieces per wave as four
// groups of four (waves 0, 1: the halves of the A block, waves 2, 3: of the B block); v_mfma_i32_16x16x64_i8; the persistent
// XCD-aware walk of gemm_map_tile, and like the product ONE flat k-sequence through the 2-slot ring across output tiles.  No
// epilogue.  Accumulator block (fa, fb) -- rows 16 fa.., columns 16 fb.. of the wave tile -- is pinned to a[(8 fa + fb) * 4 .. + 3].
//
// One k-tile = two k-steps of 64 B = four half-steps of 32 MFMAs: one group of 4 A fragments against the 8 B fragments of the
// k-step, B-outer.  Four fragment groups, 96 VGPRs: ga / gc = A rows 0-63 / 64-127, gb / gd = B of k-step 0 / 1; each is refilled
// as soon as its last MFMA has issued, ONE ds_read_b128 behind an MFMA at a time (with one wave per SIMD nobody else fills a gap):
//   HS0  ga x gb   behind its MFMAs: gc <- A high, k-step 0 (4);  gd <- B, k-step 1 (8)
//   HS1  gc x gb                     ga <- A low, k-step 1 (4)
//   HS2  ga x gd                     gc <- A high, k-step 1 (4)
//   -- every read of this slot has landed, and this wave's pieces of the next k-tile: s_barrier --
//   HS3  gc x gd                     the four LDS-DMA groups of the k-tile AFTER next into the slot just freed;
//                                    ga, gb <- the next k-tile's first fragments (12), out of the other slot
// so the DMA of a k-tile has a whole k-tile's time to land, as in the product, and the barrier sits in front of 32 MFMAs that
// need nothing from LDS.  MODE 1: no staging in the loop (timing only: stale data, outputs wrong by construction).  MODE 2: a
// second barrier per k-tile releases the B half of the slot early (see the body).  MODE 4: the same a quarter k-tile earlier.
// MODE 3: the whole slot, through registers (body3).  (G4W_ONLY = 7, 8, 9, 10, 11 are MODE 0, 1, 2, 3, 4.)
struct G4wDmaGroup { static constexpr int PPW = 4; };          // gemm_stage_block: one group of four 1-KiB pieces per call
template <int BLK> __device__ __forceinline__ void g4d_mfma(const v4i &a, const v4i &b) {
  asm volatile("v_mfma_i32_16x16x64_i8 a[%c2:%c3], %0, %1, a[%c2:%c3]" :: "v"(a), "v"(b), "i"(BLK * 4), "i"(BLK * 4 + 3) : G4W_CLOBBER);
}
template <int R> __device__ __forceinline__ int g4d_acc_read() {
  int v; asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(v) : "i"(R)); return v;
}
// an MFMA's result -> any reader or writer but the next MFMA accumulating into it needs wait states of its own in inline asm
__device__ __forceinline__ void g4d_mfma_drain() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }
template <int IMM> __device__ __forceinline__ void g4d_rd(v4i &v, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(IMM) : "memory");
}
template <int N> __device__ __forceinline__ void g4d_wait4(v4i (&g)[4]) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void g4d_wait12(v4i (&g)[4], v4i (&h)[8]) {
  asm volatile("s_waitcnt lgkmcnt(%12)" : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]), "+v"(h[0]), "+v"(h[1]), "+v"(h[2]), "+v"(h[3]),
               "+v"(h[4]), "+v"(h[5]), "+v"(h[6]), "+v"(h[7]) : "n"(N) : "memory");
}
template <int I> using G4I = std::integral_constant<int, I>;
// half-step H (A rows 64 H ..): MFMA q = 4 j + s multiplies A fragment g[s] with B fragment b[j]; hook(G4I<q>) is called behind it
template <int H, int Q = 0, class F>
__device__ __forceinline__ void g4d_half(const v4i (&g)[4], const v4i (&b)[8], F &&hook) {
  if constexpr (Q < 32) {
    g4d_mfma<(4 * H + (Q & 3)) * 8 + (Q >> 2)>(g[Q & 3], b[Q >> 2]);
    hook(G4I<Q>());
    g4d_half<H, Q + 1>(g, b, hook);
  }
}
template <int R = 0> __device__ __forceinline__ void g4d_zero() {
  if constexpr (R < 256) {
    asm volatile("v_accvgpr_write_b32 a%c0, 0\n\tv_accvgpr_write_b32 a%c1, 0\n\tv_accvgpr_write_b32 a%c2, 0\n\tv_accvgpr_write_b32 a%c3, 0"
                 :: "i"(R), "i"(R + 1), "i"(R + 2), "i"(R + 3) : G4W_CLOBBER);
    g4d_zero<R + 4>();
  } else asm volatile("s_nop 3" ::: "memory");                 // accvgpr write -> MFMA reading it as C
}
// spot check: register lane & 3 of every accumulator block of every lane -> dst[blk * 64 + lane]
template <int BLK = 0> __device__ __forceinline__ void g4d_dump(int *dst, int lane) {
  if constexpr (BLK < 64) {
    const int r0 = g4d_acc_read<BLK * 4>(), r1 = g4d_acc_read<BLK * 4 + 1>(), r2 = g4d_acc_read<BLK * 4 + 2>(), r3 = g4d_acc_read<BLK * 4 + 3>();
    const int e = lane & 3;
    dst[BLK * 64 + lane] = e == 0 ? r0 : (e == 1 ? r1 : (e == 2 ? r2 : r3));
    g4d_dump<BLK + 1>(dst, lane);
  }
}
constexpr int G4D_DUMP_INTS = 4 * 64 * 64;                     // per dumped output tile: 4 waves x 64 blocks x 64 lanes
constexpr int G4D_DUMPS = 6;                                   // workgroups 0 and 1: their first, second and last output tile

template <int MODE>
__global__ __launch_bounds__(256) void gemm4w_dma_kernel(const unsigned char *__restrict__ A, const unsigned char *__restrict__ B,
                                                         int nM, int nN, int nk, int *__restrict__ out) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  constexpr unsigned SLOT = 512 * 128, BLOCK = 256 * 128;      // ring slot = A block | B block of one k-tile
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, kq = lane >> 4;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
  // fragment f of the wave tile = 16 rows, lane l: row l % 16, 16-B chunk 4 ks + l / 16 at its swizzled position; fragments are
  // 2 KiB apart (immediate offsets).  One address per operand, k-step and slot.
  const unsigned sw = (unsigned)gemm_swz(l15);
  const unsigned rowA = lds0 + (unsigned)(wr * 128 + l15) * 128u, rowB = lds0 + BLOCK + (unsigned)(wc * 128 + l15) * 128u;
  const unsigned off0 = ((unsigned)kq ^ sw) << 4, off1 = ((unsigned)(4 + kq) ^ sw) << 4;
  // staging: this wave's 16 KiB of the k-tile's 64: waves 0, 1 the halves of the A block, waves 2, 3 of the B block
  const bool wa = wave < 2;
  const unsigned char *opbase = (wa ? A : B) + (size_t)(wave & 1) * 16384;
  unsigned char *wdst = smem + wave * 16384;
  const int ntile = nM * nN;
  const int my_tiles = (ntile - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // (host: grid <= ntile)
  // DMA cursor: runs two k-tiles ahead of the MFMAs through the workgroup's flat (output tile, k-tile) sequence
  int d_tile = blockIdx.x, d_kt = 0, d_left = my_tiles * nk;
  const unsigned char *d_src = opbase;
  auto d_enter = [&]() {
    int tm, tn;
    gemm_map_tile(d_tile, nM, nN, tm, tn);
    d_src = opbase + (size_t)(wa ? tm : tn) * (size_t)nk * BLOCK;
  };
  auto d_group = [&](unsigned so, auto gtag) {
    constexpr int g = decltype(gtag)::value;
    gemm_stage_block<G4wDmaGroup>(d_src + g * 4096, wdst + so + g * 4096, lane);
  };
  auto d_advance = [&]() {
    --d_left;
    d_src += BLOCK;
    if (++d_kt == nk) { d_kt = 0; d_tile += gridDim.x; if (d_left > 0) d_enter(); }
  };
  // the MFMAs' own position
  int c_kt = 0, c_idx = 0;
  v4i ga[4], gc[4], gb[8], gd[8];
  auto read_first = [&](unsigned sn, auto qtag) {              // fragment q of the 12 first ones of a k-tile: ga (4) then gb (8)
    constexpr int q = decltype(qtag)::value;
    if constexpr (q < 4) g4d_rd<q * 2048>(ga[q], rowA + off0 + sn);
    else g4d_rd<(q - 4) * 2048>(gb[q - 4], rowB + off0 + sn);
  };
  auto body = [&](auto slot_tag) {
    constexpr unsigned so = decltype(slot_tag)::value * SLOT, sn = SLOT - so;
    g4d_wait12<0>(ga, gb);
    g4d_half<0>(ga, gb, [&](auto qt) {
      constexpr int q = decltype(qt)::value;
      if constexpr (q < 4) g4d_rd<8192 + q * 2048>(gc[q], rowA + off0 + so);
      else if constexpr (q < 20 && (q & 1) == 0) g4d_rd<((q - 4) >> 1) * 2048>(gd[(q - 4) >> 1], rowB + off1 + so);
    });
    const bool more = MODE != 1 && d_left > 0;                  // wave-uniform
    if constexpr (MODE == 4) {                                  // MODE 2's barrier a quarter k-tile earlier: gd has landed here too
      g4d_wait12<0>(gc, gd);
      __builtin_amdgcn_s_barrier();
    } else g4d_wait4<8>(gc);                                    // younger: the 8 reads of gd
    g4d_half<1>(gc, gb, [&](auto qt) {
      constexpr int q = decltype(qt)::value;
      if constexpr (q < 4) g4d_rd<q * 2048>(ga[q], rowA + off1 + so);
      else if constexpr (MODE == 4 && q < 8) { if (more && !wa) d_group(so, G4I<q - 4>()); }
    });
    g4d_wait12<0>(ga, gd);
    // MODE 2: behind this wait a wave has read its last B fragment of slot so.  One more barrier, and the B block of the slot is
    // free half a k-tile before the A block: waves 2, 3 issue their pieces now, waves 0, 1 behind the barrier below as before, so
    // the L2 -> LDS stream has two half-slots in flight instead of pausing at every barrier.
    if constexpr (MODE == 2) __builtin_amdgcn_s_barrier();
    g4d_half<0>(ga, gd, [&](auto qt) {
      constexpr int q = decltype(qt)::value;
      if constexpr (q < 4) g4d_rd<8192 + q * 2048>(gc[q], rowA + off1 + so);
      else if constexpr (MODE == 2 && q < 8) { if (more && !wa) d_group(so, G4I<q - 4>()); }
    });
    g4d_wait4<0>(gc);                                           // the last read of slot so ...
    // ... and this wave's pieces of the next k-tile (slot sn).  MODE 2, waves 2, 3: the 16 pieces just issued are younger
    if ((MODE == 2 || MODE == 4) && more && !wa) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                               // everybody's: sn is complete, so is free
    g4d_half<1>(gc, gd, [&](auto qt) {
      constexpr int q = decltype(qt)::value;
      if constexpr (q < 4) { if (more && ((MODE != 2 && MODE != 4) || wa)) d_group(so, G4I<q>()); }
      else if constexpr (q < 16) read_first(sn, G4I<q - 4>());
    });
    if (more) d_advance();
    if (++c_kt == nk) {                                         // output tile complete: (no epilogue) spot check, then zero
      c_kt = 0;
      g4d_mfma_drain();
      const int which = c_idx == 0 ? 0 : (c_idx == 1 ? 1 : (c_idx == my_tiles - 1 ? 2 : -1));
      if (blockIdx.x < 2 && which >= 0)
        g4d_dump(out + ((size_t)(blockIdx.x * 3 + which) * 4 + wave) * (64 * 64), lane);
      ++c_idx;
      g4d_zero();
    }
  };
  // MODE 3: the whole k-tile's fragments are in registers (or in flight) by the end of HS0 -- ge / gf hold the A halves of k-step 1,
  // 128 fragment VGPRs -- so the WHOLE slot is free a quarter into the k-tile.  Barrier A there, then every wave issues its pieces
  // of the k-tile after next; barrier B in front of HS3 publishes the NEXT k-tile, whose pieces were issued a k-tile and a half
  // earlier (vmcnt(16): the 16 just issued are younger).  Two k-tiles of DMA are in flight half of the time.
  v4i ge[4], gf[4];
  auto body3 = [&](auto slot_tag) {
    constexpr unsigned so = decltype(slot_tag)::value * SLOT, sn = SLOT - so;
    g4d_wait12<0>(ga, gb);
    g4d_half<0>(ga, gb, [&](auto qt) {
      constexpr int q = decltype(qt)::value;
      if constexpr (q < 4) g4d_rd<8192 + q * 2048>(gc[q], rowA + off0 + so);
      else if constexpr (q < 12) g4d_rd<(q - 4) * 2048>(gd[q - 4], rowB + off1 + so);
      else if constexpr (q < 16) g4d_rd<(q - 12) * 2048>(ge[q - 12], rowA + off1 + so);
      else if constexpr (q < 20) g4d_rd<8192 + (q - 16) * 2048>(gf[q - 16], rowA + off1 + so);
    });
    g4d_wait12<0>(gc, gd);
    g4d_wait4<0>(ge);
    g4d_wait4<0>(gf);
    __builtin_amdgcn_s_barrier();                               // A: nobody reads slot so any more
    const bool more = d_left > 0;
    g4d_half<1>(gc, gb, [&](auto qt) {
      constexpr int q = decltype(qt)::value;
      if constexpr (q < 4) { if (more) d_group(so, G4I<q>()); }
    });
    g4d_half<0>(ge, gd, [&](auto) {});
    if (more) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // this wave's pieces of the next k-tile (slot sn) ...
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                               // B: ... and everybody's
    g4d_half<1>(gf, gd, [&](auto qt) {
      constexpr int q = decltype(qt)::value;
      if constexpr (q < 12) read_first(sn, G4I<q>());
    });
    if (more) d_advance();
    if (++c_kt == nk) {
      c_kt = 0;
      g4d_mfma_drain();
      const int which = c_idx == 0 ? 0 : (c_idx == 1 ? 1 : (c_idx == my_tiles - 1 ? 2 : -1));
      if (blockIdx.x < 2 && which >= 0)
        g4d_dump(out + ((size_t)(blockIdx.x * 3 + which) * 4 + wave) * (64 * 64), lane);
      ++c_idx;
      g4d_zero();
    }
  };
  // prologue: k-tiles 0 and 1 of the first output tile into slots 0 and 1, the first fragments of slot 0 in flight
  d_enter();
  d_group(0u, G4I<0>()); d_group(0u, G4I<1>()); d_group(0u, G4I<2>()); d_group(0u, G4I<3>());
  d_advance();
  d_group(SLOT, G4I<0>()); d_group(SLOT, G4I<1>()); d_group(SLOT, G4I<2>()); d_group(SLOT, G4I<3>());
  d_advance();
  g4d_zero();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  read_first(0u, G4I<0>()); read_first(0u, G4I<1>()); read_first(0u, G4I<2>()); read_first(0u, G4I<3>());
  read_first(0u, G4I<4>()); read_first(0u, G4I<5>()); read_first(0u, G4I<6>()); read_first(0u, G4I<7>());
  read_first(0u, G4I<8>()); read_first(0u, G4I<9>()); read_first(0u, G4I<10>()); read_first(0u, G4I<11>());
  for (int s = my_tiles * nk; s > 0; s -= 2) {                  // (host: nk even)
    if constexpr (MODE == 3) { body3(G4I<0>()); body3(G4I<1>()); }
    else { body(G4I<0>()); body(G4I<1>()); }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ga[0]), "+v"(gb[0]) :: "memory");   // the read-ahead behind the last k-tile
}

// sigma <= 0: small values -3 .. 3 (round 2's fill: hardly any switching activity); sigma > 0: round(N(0, sigma)) clamped to
// +-127 -- what a quantised residual stream / encoder row looks like to the multipliers (round 4: the power / clock comparison
// against the product's kernel, tools/gpu_r04_power.sh)
__global__ void fill(unsigned char *p, size_t n, unsigned seed, float sigma) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull + seed * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z ^= z >> 27;
    if (sigma <= 0.f) { p[i] = (unsigned char)(signed char)((int)(z % 7) - 3); continue; }
    z *= 0x94D049BB133111EBull; z ^= z >> 31;
    float g = 0.f;
    for (int q = 0; q < 4; ++q) g += (float)((z >> (16 * q)) & 0xFFFF) / 65536.f - 0.5f;   // variance 4/12
    int v = (int)rintf(g * 1.7320508f * sigma);
    p[i] = (unsigned char)(signed char)(v > 127 ? 127 : (v < -127 ? -127 : v));
  }
}

template <int SETS>
void run(const unsigned char *A, const unsigned char *B, int T, int N, int d, int *out, const signed char *hA, const signed char *hB) {
  const int nM = T / 256, nN = N / 256, nk = d / 128;
  const size_t smem = 2 * 512 * 128;
  auto kern = SETS == 0 ? gemm4w_sched_kernel : (SETS == 3 ? gemm4w_v2_kernel<0> : (SETS == 4 ? gemm4w_v2_kernel<1> : (SETS == 5 ? gemm4w_v2_kernel<2> : (SETS == 6 ? gemm4w_v2_kernel<3> : gemm4w_kernel<(SETS == 2 ? 2 : 1)>))));
  CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(kern, dim3(256), dim3(256), smem, 0, A, B, (size_t)d, nM, nN, nk, out, N);
  CK(hipDeviceSynchronize());
  float best = 1e30f;
  const int reps = getenv("G4W_REPS") ? atoi(getenv("G4W_REPS")) : 5;     // many: long enough for rocm-smi's power / clock samples
  for (int i = 0; i < reps; ++i) {
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(kern, dim3(256), dim3(256), smem, 0, A, B, (size_t)d, nM, nN, nk, out, N);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); if (ms < best) best = ms;
  }
  int h[16 + 128]; CK(hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int tile = 0; tile < 2; ++tile) {
    int tm, tn; { int b = tile; const int xcd = b & 7, slot = b >> 3; const int st = (slot / 32) * 8 + xcd; tm = (st % (nM / 8)) * 8 + (slot % 32) % 8; tn = (st / (nM / 8)) * 4 + (slot % 32) / 8; }
    for (int wave = 0; wave < 4; ++wave) for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
      const int row = tm * 256 + (wave >> 1) * 128 + i * 32, col = tn * 256 + (wave & 1) * 128 + j * 32;
      long ref = 0; for (int k = 0; k < d; ++k) ref += (long)hA[(size_t)row * d + k] * hB[(size_t)col * d + k];
      if ((int)ref != h[16 + tile * 64 + wave * 16 + i * 4 + j]) ++bad;
    }
  }
  const double ops = 2.0 * T * N * d;
  printf("4 waves, register staging, %d set(s) in flight: %7.3f ms  %6.0f TOP/s  %5.2f us per k-tile   outputs checked: %s\n", SETS, best,
         ops / best / 1e9, best * 1e3 / ((double)nM * nN * nk / 256), bad ? "MISMATCH" : "ok");
}

// v3.  The operand buffers are READ as tile-major: byte k of row r of an operand with nk k-tiles lives in the 32-KB block of
// (row tile r / 256, k-tile k / 128), row r % 256, at the swizzled position of its 16-B chunk -- the naive reference reads it there.
static inline int tm_at(const signed char *X, int nk, int row, int k) {
  const int r = row & 255, c = (k & 127) >> 4;
  return X[((size_t)(row >> 8) * nk + (k >> 7)) * 32768 + (size_t)r * 128 + (size_t)((c ^ ((r >> 1) & 7)) << 4) + (k & 15)];
}
template <int MODE>
void run_dma(const unsigned char *A, const unsigned char *B, int T, int N, int d, int *out, const signed char *hA, const signed char *hB) {
  const int nM = T / 256, nN = N / 256, nk = d / 128, grid = 256;
  if (nk < 2 || (nk & 1) || nM * nN < grid) { printf("4 waves, LDS-DMA: shape not supported\n"); return; }
  const size_t smem = 2 * 512 * 128;
  auto kern = gemm4w_dma_kernel<MODE>;
  CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, 0, A, B, nM, nN, nk, out);
  CK(hipDeviceSynchronize());
  if (getenv("G4W_READY")) { printf("ready\n"); fflush(stdout); }
  float best = 1e30f, sum = 0.f;
  const int reps = getenv("G4W_REPS") ? atoi(getenv("G4W_REPS")) : 5;
  for (int i = 0; i < reps; ++i) {
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, 0, A, B, nM, nN, nk, out);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); if (ms < best) best = ms; sum += ms;
  }
  int *h = (int *)malloc((size_t)G4D_DUMPS * G4D_DUMP_INTS * 4);
  CK(hipMemcpy(h, out, (size_t)G4D_DUMPS * G4D_DUMP_INTS * 4, hipMemcpyDeviceToHost));
  const int ntile = nM * nN;
  long bad = 0, checked = 0;
  for (int b = 0; b < 2; ++b) for (int which = 0; which < 3; ++which) {
    const int mine = (ntile - b + grid - 1) / grid, idx = which < 2 ? which : mine - 1;
    const int tile = b + idx * grid;
    int tm, tn;
    if (nM % 8 == 0 && nN % 4 == 0 && ((nM / 8) * (nN / 4)) % 8 == 0) {     // gemm_map_tile, 8 x 4 super-tiles
      const int xcd = tile & 7, slot = tile >> 3, st = (slot / 32) * 8 + xcd;
      tm = (st % (nM / 8)) * 8 + (slot % 32) % 8; tn = (st / (nM / 8)) * 4 + (slot % 32) / 8;
    } else { tm = tile % nM; tn = tile / nM; }
    for (int wave = 0; wave < 4; ++wave) for (int blk = 0; blk < 64; ++blk) for (int lane = 0; lane < 64; ++lane) {
      const int row = tm * 256 + (wave >> 1) * 128 + (blk >> 3) * 16 + 4 * (lane >> 4) + (lane & 3);
      const int col = tn * 256 + (wave & 1) * 128 + (blk & 7) * 16 + (lane & 15);
      int ref = 0;
      for (int k = 0; k < d; ++k) ref += tm_at(hA, nk, row, k) * tm_at(hB, nk, col, k);
      if (ref != h[((size_t)(b * 3 + which) * 4 + wave) * 4096 + blk * 64 + lane]) ++bad;
      ++checked;
    }
  }
  free(h);
  const double ops = 2.0 * T * N * d;
  printf("4 waves, LDS-DMA, 16x16x64%s: mean %7.3f ms  best %7.3f ms  %6.0f TOP/s  %5.2f us per k-tile   %ld outputs of 6 tiles checked: %s\n",
         MODE == 1 ? ", no staging" : (MODE == 2 ? ", B half released early" : (MODE == 3 ? ", slot released at 1/4" : (MODE == 4 ? ", B half released at 1/4" : ""))), sum / reps, best, ops / best / 1e9, best * 1e3 / ((double)nM * nN * nk / grid), checked,
         bad ? "MISMATCH" : "ok");
}

int main() {
  const int T = 8192, N = getenv("G4W_N") ? atoi(getenv("G4W_N")) : 131072, d = 4096;
  unsigned char *A, *B; int *out;
  CK(hipMalloc(&A, (size_t)T * d)); CK(hipMalloc(&B, (size_t)N * d)); CK(hipMalloc(&out, (size_t)G4D_DUMPS * G4D_DUMP_INTS * 4));
  const float sigma = getenv("G4W_SIGMA") ? (float)atof(getenv("G4W_SIGMA")) : 0.f;
  fill<<<2048, 256>>>(A, (size_t)T * d, 1, sigma); fill<<<2048, 256>>>(B, (size_t)N * d, 2, sigma);
  if (sigma > 0.f) printf("int8 operands: round(N(0, %.0f))\n", sigma);
  CK(hipDeviceSynchronize());
  // host copies of the rows the check touches (tiles 0 and 1: a few rows of A and B)
  signed char *hA = (signed char *)malloc((size_t)T * d), *hB = (signed char *)malloc((size_t)2048 * d * 4);
  CK(hipMemcpy(hA, A, (size_t)T * d, hipMemcpyDeviceToHost));
  signed char *hBfull = (signed char *)malloc((size_t)N * d);
  CK(hipMemcpy(hBfull, B, (size_t)N * d, hipMemcpyDeviceToHost));
  if (getenv("G4W_ONLY")) {                    // one variant, many repetitions: power sampling
    switch (atoi(getenv("G4W_ONLY"))) {
      case 0: run<0>(A, B, T, N, d, out, hA, hBfull); break;
      case 3: run<3>(A, B, T, N, d, out, hA, hBfull); break;
      case 4: run<4>(A, B, T, N, d, out, hA, hBfull); break;
      case 5: run<5>(A, B, T, N, d, out, hA, hBfull); break;
      case 6: run<6>(A, B, T, N, d, out, hA, hBfull); break;
      case 7: run_dma<0>(A, B, T, N, d, out, hA, hBfull); break;     // v3: LDS-DMA staging, 16x16x64 MFMAs, flat k-sequence
      case 8: run_dma<1>(A, B, T, N, d, out, hA, hBfull); break;     // v3 without staging in the loop
      case 9: run_dma<2>(A, B, T, N, d, out, hA, hBfull); break;     // v3 with the B half of a slot released half a k-tile early
      case 11: run_dma<4>(A, B, T, N, d, out, hA, hBfull); break;    // as 9, the B half released a quarter into the k-tile
      case 10: run_dma<3>(A, B, T, N, d, out, hA, hBfull); break;    // v3 with the whole slot released a quarter into the k-tile
      default: run<1>(A, B, T, N, d, out, hA, hBfull); break;
    }
    return 0;
  }
  run<1>(A, B, T, N, d, out, hA, hBfull);
  run<0>(A, B, T, N, d, out, hA, hBfull);     // "0 set(s)" = the hand-scheduled kernel
  run<3>(A, B, T, N, d, out, hA, hBfull);     // "3 set(s)" = v2: AGPR-pinned accumulators, two staging sets
  run<4>(A, B, T, N, d, out, hA, hBfull);     // "4": v2 without staging in the loop (outputs wrong by construction)
  run<5>(A, B, T, N, d, out, hA, hBfull);     // "5": v2 with the LDS writes but without the loads
  run<6>(A, B, T, N, d, out, hA, hBfull);     // "6": v2 with MFMAs only
  run<3>(A, B, T, N, d, out, hA, hBfull);
  run_dma<0>(A, B, T, N, d, out, hA, hBfull);
  run_dma<1>(A, B, T, N, d, out, hA, hBfull);
  (void)hB;
  return 0;
}
