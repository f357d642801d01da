"""Float32 against 8-bit Adam moments on the device (profiles/adam8.txt).

    timeout -k 10 300 python tools/adam8_bench.py --part sweep     # the Adam pass over W_dec and W_enc, modes alternated
    timeout -k 10 300 python tools/adam8_bench.py --part step      # one SaeTrainStep at T tokens in both modes

sweep: device-event time of ops.adam_rows_ (float32 moments: the yardstick) and ops.adam8_rows_ (8-bit moments) over one
[N, d] matrix, alternating in one process after a warm-up: W_dec runs with the projection and the fused renorm, W_enc with
the fused operand refresh for T tokens.  Bytes are computed from shapes: W read + write 8, G read 4 (its second read by the
projection is an L2 hit and not counted), moments read + write 16 or 4 per element, plus 16 bytes of scales per 256-element
block in 8-bit mode; the operand writes of the refresh tail are the same in both modes and not counted.
step: SaeTrainStep(optim_bits=32 | 8).step on random activations, device events around each step."""
from __future__ import annotations

import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "multimodal-sae_amd"))


def _stats(ms):
    s = sorted(ms)
    return (f"median {statistics.median(s):.3f} ms  min {s[0]:.3f}  p10 {s[len(s) // 10]:.3f}  p90 {s[-1 - len(s) // 10]:.3f}  "
            f"max {s[-1]:.3f}  (n = {len(s)})")


def sweep(args) -> None:
    from msae import ops

    dev = torch.device("cuda:0")
    N, d = args.N, args.d
    n = N * d
    nb = N * -(-d // 256)
    bytes32, bytes8 = 28 * n, 16 * n + 16 * nb
    print(f"sweep: [{N}, {d}] float32 pass moves {bytes32 / 2**30:.2f} GiB, 8-bit pass {bytes8 / 2**30:.2f} GiB "
          f"(ratio {bytes8 / bytes32:.3f}); warm-up {args.warmup}, {args.reps} timed repetitions each, alternating")
    g = torch.Generator(device=dev).manual_seed(1)
    W0 = torch.randn(N, d, generator=g, device=dev) / d ** 0.5
    G = torch.randn(N, d, generator=g, device=dev) * 1e-3
    ss = (G.double() ** 2).sum().float().reshape(1)
    eps = torch.finfo(torch.float32).eps
    for name in ("W_dec (projection + renorm)", "W_enc (operand refresh)"):
        dec = name.startswith("W_dec")
        Wa, Wb = W0.clone(), W0.clone()
        M = torch.randn(N, d, generator=g, device=dev) * 1e-4
        V = torch.rand(N, d, generator=g, device=dev) * 1e-7
        st = ops.adam8_quantize(M, V)
        if dec:
            ops.unit_norm_rows_(Wa, eps); ops.unit_norm_rows_(Wb, eps)
            kwa = kwb = dict(project=True, renorm_eps=eps)
        else:
            nbytes = ops.prepare_encoder(Wa).numel()
            bufa = ops.prepare_encoder(Wa, out=torch.zeros(nbytes, dtype=torch.uint8, device=dev))
            bufb = bufa.clone()
            kwa, kwb = dict(refresh=bufa, tokens_next=args.T), dict(refresh=bufb, tokens_next=args.T)
        t32, t8 = [], []
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.warmup + args.reps)]
        for i, (e0, e1, e2) in enumerate(ev):
            e0.record()
            ops.adam_rows_(Wa, G, M, V, 2 + i, 1e-4, total_sumsq=ss, **kwa)
            e1.record()
            ops.adam8_rows_(Wb, G, st, 2 + i, 1e-4, total_sumsq=ss, **kwb)
            e2.record()
        torch.cuda.synchronize()
        for e0, e1, e2 in ev[args.warmup:]:
            t32.append(e0.elapsed_time(e1)); t8.append(e1.elapsed_time(e2))
        m32, m8 = statistics.median(t32), statistics.median(t8)
        print(f"{name}")
        print(f"  float32 moments  {_stats(t32)}  {bytes32 / m32 / 1e9:.2f} TB/s")
        print(f"  8-bit moments    {_stats(t8)}  {bytes8 / m8 / 1e9:.2f} TB/s")
        print(f"  8-bit / float32 time {m8 / m32:.3f} (bandwidth model {bytes8 / bytes32:.3f})")
        assert bool(torch.isfinite(Wb).all()) and bool(torch.isfinite(Wa).all())
        del Wa, Wb, M, V, st
        torch.cuda.empty_cache()


def step(args) -> None:
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    dev = torch.device("cuda:0")
    print(f"step: SaeTrainStep at d = {args.d}, N = {args.N}, k = {args.k}, T = {args.T}; warm-up 3, {args.steps} timed steps")
    for bits in (32, 8, 32, 8):
        torch.manual_seed(3)
        sae = Sae(args.d, SaeConfig(num_latents=args.N, k=args.k), device=dev)
        ts = SaeTrainStep(sae, optim_bits=bits)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(3 + args.steps)]
        g = torch.Generator(device=dev).manual_seed(5)
        for e0, e1 in ev:
            x = torch.randn(args.T, args.d, generator=g, device=dev)
            e0.record()
            ts.step(x)
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev[3:]]
        print(f"  optim_bits={bits:<2}  {_stats(ms)}  optimiser state {ts.optimizer_state_bytes / 2**30:.2f} GiB")
        del sae, ts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["sweep", "step"], required=True)
    ap.add_argument("--N", type=int, default=131072)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--T", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measures on the GPU"
    (sweep if a.part == "sweep" else step)(a)
