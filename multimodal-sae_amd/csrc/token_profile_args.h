// token_profile_args.h -- the argument checks and launch sizes of msae_token_profile_* (token_profile.hip) in plain C++, with no
// HIP in them: tools/token_profile_args_check.cpp compiles this header for the host alone, under the sanitisers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tp_args {

constexpr int MAX_T = 65536, MAX_K = 256, MAX_N = 262144;      // the envelope of every cache-loop update (pool_segments.h)
constexpr int MAX_F = 16384, MAX_O = 4, MAX_OFFSET = 64, MAX_M = 64;
constexpr int ENTRIES = 1024;                                  // list entries (update) / positions (token counts) per workgroup
constexpr int METRIC_COUNT = 0, METRIC_PRECISION = 1, METRIC_MEAN = 2;

struct Offsets {       // the offset planes of one call, by value into the kernels
  int o[MAX_O];
  int n;
};

// B * S into *T, or false where a size is negative or the product passes MAX_T (no int overflow on the way)
inline bool tokens(int B, int S, int *T) {
  if (B < 0 || S < 0 || (B > 0 && S > MAX_T / B)) return false;
  *T = B * S;
  return true;
}

// 1 <= O <= 4 distinct offsets in [-64, 64], read from the HOST array `offsets`
inline bool offsets_ok(const int32_t *offsets, int O, Offsets *out) {
  if (!offsets || O < 1 || O > MAX_O) return false;
  out->n = O;
  for (int a = 0; a < MAX_O; ++a) out->o[a] = 0;
  for (int a = 0; a < O; ++a) {
    if (offsets[a] < -MAX_OFFSET || offsets[a] > MAX_OFFSET) return false;
    for (int b = 0; b < a; ++b)
      if (offsets[b] == offsets[a]) return false;
    out->o[a] = offsets[a];
  }
  return true;
}

// O * F * V < 2^31: a cell index is a non-negative int
inline bool cells_ok(int O, int F, int V) {
  if (O < 1 || O > MAX_O || F < 1 || F > MAX_F || V < 1) return false;
  return (long long)O * F * (long long)V < (1ll << 31);
}

inline bool update_shape_ok(int B, int S, int k, int N, int F, int V, int O, int ids_bits, int *T) {
  if (!tokens(B, S, T)) return false;
  if (k < 1 || k > MAX_K || N < 1 || N > MAX_N) return false;
  return cells_ok(O, F, V) && (ids_bits == 32 || ids_bits == 64);
}

inline bool topk_shape_ok(int F, int V, int m, int metric, int min_count, bool has_mass) {
  if (!cells_ok(1, F, V) || m < 1 || m > MAX_M || min_count < 1) return false;
  if (metric == METRIC_MEAN) return has_mass;
  return metric == METRIC_COUNT || metric == METRIC_PRECISION;
}

// workgroups over n items, ENTRIES each
inline unsigned chunks(long long n) { return (unsigned)((n + ENTRIES - 1) / ENTRIES); }

}  // namespace tp_args
