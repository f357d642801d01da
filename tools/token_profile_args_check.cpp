// The argument checks and launch sizes of msae_token_profile_* (multimodal-sae_amd/csrc/token_profile_args.h) on the host alone:
// every MSAE_EINVAL case of include/msae.h's "token profiles" section, and the accepted envelope's corners.  No HIP, no GPU:
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I multimodal-sae_amd/csrc
//       tools/token_profile_args_check.cpp -o /tmp/token_profile_args_check && /tmp/token_profile_args_check
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "token_profile_args.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

int main() {
  using namespace tp_args;
  int T = -1;
  Offsets off;
  // ---- update: shapes
  EXPECT(update_shape_ok(3, 37, 4, 512, 5, 97, 3, 64, &T) && T == 111);
  EXPECT(update_shape_ok(0, 37, 4, 512, 5, 97, 3, 32, &T) && T == 0);
  EXPECT(update_shape_ok(1, 65536, 256, 262144, 16384, 131071, 1, 32, &T) && T == 65536);   // 2^14 * (2^17 - 1) < 2^31
  EXPECT(!update_shape_ok(-1, 37, 4, 512, 5, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, -1, 4, 512, 5, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(2, 32769, 4, 512, 5, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(INT_MAX, INT_MAX, 4, 512, 5, 97, 3, 64, &T));                  // no overflow on the way
  EXPECT(!update_shape_ok(3, 37, 0, 512, 5, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 257, 512, 5, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 0, 5, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 262145, 5, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 0, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 16385, 97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 5, 0, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 5, -97, 3, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 5, 97, 0, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 5, 97, 5, 64, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 5, 97, 3, 16, &T));
  EXPECT(!update_shape_ok(3, 37, 4, 512, 16384, 131072, 1, 64, &T));                     // exactly 2^31 cells
  EXPECT(!update_shape_ok(3, 37, 4, 512, 16384, INT_MAX, 4, 64, &T));                    // the product is taken in 64 bits
  EXPECT(cells_ok(4, 4095, 131072) && !cells_ok(4, 4096, 131072));
  // ---- update: offsets
  const int32_t good[4] = {-64, 0, 64, 1}, twice[3] = {0, 1, 0}, far[2] = {0, 65}, low[1] = {-65};
  EXPECT(offsets_ok(good, 4, &off) && off.n == 4 && off.o[0] == -64 && off.o[2] == 64 && off.o[3] == 1);
  EXPECT(offsets_ok(good, 1, &off) && off.n == 1 && off.o[1] == 0 && off.o[3] == 0);
  EXPECT(!offsets_ok(nullptr, 1, &off) && !offsets_ok(good, 0, &off) && !offsets_ok(good, 5, &off));
  EXPECT(!offsets_ok(twice, 3, &off) && offsets_ok(twice, 2, &off));
  EXPECT(!offsets_ok(far, 2, &off) && !offsets_ok(low, 1, &off));
  // ---- top tokens
  EXPECT(topk_shape_ok(5, 97, 10, METRIC_COUNT, 1, false) && topk_shape_ok(5, 97, 64, METRIC_PRECISION, 3, false));
  EXPECT(topk_shape_ok(5, 97, 1, METRIC_MEAN, 1, true) && !topk_shape_ok(5, 97, 1, METRIC_MEAN, 1, false));
  EXPECT(!topk_shape_ok(0, 97, 10, 0, 1, true) && !topk_shape_ok(16385, 97, 10, 0, 1, true) && !topk_shape_ok(5, 0, 10, 0, 1, true));
  EXPECT(!topk_shape_ok(5, 97, 0, 0, 1, true) && !topk_shape_ok(5, 97, 65, 0, 1, true) && !topk_shape_ok(5, 97, 10, 3, 1, true));
  EXPECT(!topk_shape_ok(5, 97, 10, -1, 1, true) && !topk_shape_ok(5, 97, 10, 0, 0, true) && !topk_shape_ok(5, 97, 10, 0, -4, true));
  EXPECT(!topk_shape_ok(16384, 131072, 10, 0, 1, true));
  // ---- launch sizes
  EXPECT(chunks(1) == 1 && chunks(1024) == 1 && chunks(1025) == 2 && chunks((long long)65536 * 256) == 16384);
  std::printf(failures ? "%d check(s) failed\n" : "token_profile_args: all checks passed\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
