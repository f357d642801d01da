// pos_q.h -- q(v), the fixed-point value the position profiles (pos_profile.hip) and the token profiles (token_profile.hip) sum
// into their `mass` counters: ONE function of the float32 bits for both (include/msae.h promises that they agree).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// q(v) for v > 0 (not NaN), from the float32 bits: v = m * 2^(e - 150) with the 24-bit significand m, so q = m * 2^(e - 130)
// rounded half to even; 2^60 from 2^40 on (+inf included).
__host__ __device__ __forceinline__ unsigned long long pp_q(float v) {
  unsigned u;
  __builtin_memcpy(&u, &v, 4);
  const int eb = (int)((u >> 23) & 0xffu);
  const unsigned long long m = eb ? ((u & 0x7fffffu) | 0x800000u) : (u & 0x7fffffu);
  const int sh = (eb ? eb : 1) - 130;
  if (sh >= 37) return 1ull << 60;                  // v >= 2^40 (eb = 255: +inf)
  if (sh >= 0) return m << sh;
  const int r = -sh;
  if (r > 25) return 0;                             // m < 2^24: below a half
  const unsigned long long fl = m >> r, rem = m & ((1ull << r) - 1ull), half = 1ull << (r - 1);
  return fl + ((rem > half || (rem == half && (fl & 1ull))) ? 1ull : 0ull);
}

}  // namespace
