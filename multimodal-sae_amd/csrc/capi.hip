// capi.hip -- library-level entry points of libmsae_hip.so (see include/msae.h).
#include "common.h"

extern "C" int msae_abi_version(void) { return MSAE_ABI_VERSION; }

extern "C" const char *msae_target_arch(void) { return "gfx950"; }

extern "C" const char *msae_error_string(int code) {
  switch (code) {
    case 0: return "success";
    case MSAE_EINVAL: return "msae: invalid argument (shape, k or dtype code)";
    case MSAE_EALIGN: return "msae: pointer or leading dimension not aligned as required";
    case MSAE_EWS: return "msae: workspace missing or too small";
    case MSAE_ENOTIMPL: return "msae: shape outside what this build supports";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "msae: unknown error";
  }
}

// ---- debug entry: the fused encoder's threshold select on rows the caller owns (topk.hip) ----
bool msae_kth_value_launch(const float *rows, int T, int S, int ld, int r, float *out, int out_ld, int out_col, hipStream_t s,
                           const KthPush &push);

extern "C" int msae_kth_value_f32(const float *rows, int T, int S, int ld, int r, float *out, int32_t *cnt,
                                  unsigned long long *cand, int cap, int stride, int off, void *stream) {
  if (!rows || !out || T < 0 || S <= 0 || ld < S || r < 1 || r > S || (cnt && (!cand || cap < 0 || stride < 1 || off < 0)))
    return MSAE_EINVAL;
  if (T == 0) return 0;
  KthPush push{};
  if (cnt) { push.cnt = cnt; push.cand = cand; push.cap = cap; push.stride = stride; push.off = off; }
  if (!msae_kth_value_launch(rows, T, S, ld, r, out, 1, 0, (hipStream_t)stream, push)) return MSAE_ENOTIMPL;
  return msae_launch_status();
}
