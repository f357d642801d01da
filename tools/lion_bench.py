"""Adam against the sign-momentum optimiser (Lion) on the device (profiles/lion.txt).

    timeout -k 10 300 python tools/lion_bench.py --part sweep     # the optimiser pass over W_dec and W_enc, alternated
    timeout -k 10 300 python tools/lion_bench.py --part step      # one SaeTrainStep at T tokens with either optimiser

sweep: device-event time of ops.adam_rows_ (unchanged code: the yardstick) and ops.lion_rows_ over one [N, d] matrix,
alternating in one process after a warm-up: W_dec runs with the projection and the fused renorm, W_enc with the fused operand
refresh for T tokens.  Bytes are computed from shapes: W read + write 8, G read 4 (its second read by the projection is an L2
hit and not counted), moments read + write 16 (Adam) or 8 (Lion) per element: 28 n against 20 n; the operand writes of the
refresh tail are the same for both and not counted.
step: SaeTrainStep(optimizer="adam" | "lion").step on random activations, device events around each step."""
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
    bytes_adam, bytes_lion = 28 * n, 20 * n
    print(f"sweep: [{N}, {d}] Adam pass moves {bytes_adam / 2**30:.2f} GiB, Lion pass {bytes_lion / 2**30:.2f} GiB "
          f"(ratio {bytes_lion / bytes_adam:.3f}); warm-up {args.warmup}, {args.reps} timed repetitions each, alternating")
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
        Ml = M.clone()
        if dec:
            ops.unit_norm_rows_(Wa, eps); ops.unit_norm_rows_(Wb, eps)
            kwa = kwb = dict(project=True, renorm_eps=eps)
        else:
            nbytes = ops.prepare_encoder(Wa).numel()
            bufa = ops.prepare_encoder(Wa, out=torch.zeros(nbytes, dtype=torch.uint8, device=dev))
            bufb = bufa.clone()
            kwa, kwb = dict(refresh=bufa, tokens_next=args.T), dict(refresh=bufb, tokens_next=args.T)
        ta, tl = [], []
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.warmup + args.reps)]
        for i, (e0, e1, e2) in enumerate(ev):
            e0.record()
            ops.adam_rows_(Wa, G, M, V, 2 + i, 1e-4, total_sumsq=ss, **kwa)
            e1.record()
            ops.lion_rows_(Wb, G, Ml, 1e-5, total_sumsq=ss, **kwb)
            e2.record()
        torch.cuda.synchronize()
        for e0, e1, e2 in ev[args.warmup:]:
            ta.append(e0.elapsed_time(e1)); tl.append(e1.elapsed_time(e2))
        ma, ml = statistics.median(ta), statistics.median(tl)
        print(f"{name}")
        print(f"  Adam (two moments)  {_stats(ta)}  {bytes_adam / ma / 1e9:.2f} TB/s")
        print(f"  Lion (one moment)   {_stats(tl)}  {bytes_lion / ml / 1e9:.2f} TB/s")
        print(f"  Lion / Adam time {ml / ma:.3f} (bandwidth model {bytes_lion / bytes_adam:.3f})")
        assert bool(torch.isfinite(Wb).all()) and bool(torch.isfinite(Wa).all())
        del Wa, Wb, M, V, Ml
        torch.cuda.empty_cache()


def step(args) -> None:
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    dev = torch.device("cuda:0")
    print(f"step: SaeTrainStep at d = {args.d}, N = {args.N}, k = {args.k}, T = {args.T}; warm-up 3, {args.steps} timed steps")
    for optimizer in ("adam", "lion", "adam", "lion"):
        torch.manual_seed(3)
        sae = Sae(args.d, SaeConfig(num_latents=args.N, k=args.k), device=dev)
        ts = SaeTrainStep(sae, lr=args.lr, optimizer=optimizer)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(3 + args.steps)]
        g = torch.Generator(device=dev).manual_seed(5)
        for e0, e1 in ev:
            x = torch.randn(args.T, args.d, generator=g, device=dev)
            e0.record()
            ts.step(x)
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev[3:]]
        print(f"  optimizer={optimizer:<4}  {_stats(ms)}  optimiser state {ts.optimizer_state_bytes / 2**30:.2f} GiB")
        del sae, ts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["sweep", "step"], required=True)
    ap.add_argument("--N", type=int, default=131072)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--T", type=int, default=8192)
    ap.add_argument("--lr", type=float, default=7e-5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measures on the GPU"
    (sweep if a.part == "sweep" else step)(a)
