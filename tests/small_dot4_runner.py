"""Child process of tests/test_gpu_encode_shape_lattice.py::test_shipped_dot4_kernels_for_2_and_4_tokens.

The small-T path streams the weights through v_dot4 for one token and through the matrix cores from two tokens on; the dot4
kernels for 2 and 4 tokens (gemv_small_kernel<., 2>, <., 4>) are compiled and shipped behind the tuning knob
MSAE_SMALL_DOT4_MAX, which csrc/encode_fused.hip reads ONCE per process -- hence a process of its own, started with the knob at
4.  Encodes 2, 3 and 4 tokens at d_in = 1024 and 4096 and compares every token with oracle.encode_topk, bit for bit.  Prints one
"ok:" line per case; exit status 0 iff all six are right.
"""
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "tests", REPO / "multimodal-sae_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def main() -> int:
    if os.environ.get("MSAE_SMALL_DOT4_MAX") != "4":
        print("start this runner with MSAE_SMALL_DOT4_MAX=4 in its environment")
        return 2
    import numpy as np
    import torch

    from encode_routes import np32, rand_sae, rand_x, same_bits
    from msae import ops
    from oracle import oracle

    dev = torch.device("cuda:0")
    N, k = 8192, 32
    ops.set_dither("on", seed=0xD074)
    bad = 0
    for d in (1024, 4096):
        W, b, bd = rand_sae(dev, d, N, seed=500 + d)
        prepared = ops.prepare_encoder(W)
        x = rand_x(dev, 4, d, seed=600 + d)
        rv, ri = oracle.encode_topk(np32(x), np32(W), np32(b), np32(bd), k)
        for T in (2, 3, 4):
            v, i, st = ops.encode_topk(x[:T], W, b, bd, prepared, k)
            v, i, st = v.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()
            same = same_bits(v, rv[:T]) & same_bits(i, ri[:T].astype(np.int64))
            # no token unresolved, every token's bits, and all but at most one token verified by the fast path
            good = bool((st != 2).all()) and bool(same.all()) and int((st != 0).sum()) <= 1
            print(f"{'ok:' if good else 'WRONG:'} T = {T}, d = {d}: status {st.tolist()}, tokens equal {same.tolist()}", flush=True)
            bad += 0 if good else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
