// wave_ops.h -- reductions and prefix sums over the 64 lanes of a wave and over the waves of a workgroup.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Sum / maximum over the wave, the result in every lane: xor butterfly, partner distance 32 down to 1.  For a float the order
// of the additions is part of the result (kernels promise bit-reproducible sums): do not reorder the loop.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const T o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Inclusive prefix sum over the wave in lane order (lane = threadIdx.x & 63).
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T n = __shfl_up(v, off, 64);
    if (lane >= off) v += n;
  }
  return v;
}

// The cross-wave half of a workgroup scan over NW waves: wave_total is the sum of the caller's wave (lane 63's copy counts);
// returns the sum of the waves in front of the caller's and gives every thread the workgroup's total in *total.  wave_tot is
// an [NW] LDS array.  Two barriers, all threads call: one before wave_tot is written (the readers of an earlier call are done
// with it) and one before it is read -- so calls may follow each other in a loop with nothing in between.
template <int NW, class T>
__device__ __forceinline__ T block_wave_offset(T wave_total, T *wave_tot, T *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 63) wave_tot[wave] = wave_total;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const T t = wave_tot[w];
    if (w < wave) base += t;
    tot += t;
  }
  *total = tot;
  return base;
}

// Exclusive prefix sum of v in thread order over a workgroup of NW waves: the wave scan, then block_wave_offset (its barriers).
template <int NW, class T>
__device__ __forceinline__ T block_excl_scan(T v, T *wave_tot, T *total) {
  const T incl = wave_incl_scan(v, (int)(threadIdx.x & 63));
  return block_wave_offset<NW>(incl, wave_tot, total) + incl - v;
}

}  // namespace
