"""AuxK with and without the dense latents on the device (profiles/auxk_subset.txt).

    timeout -k 10 600 python tools/auxk_bench.py --dead 1500
    timeout -k 10 600 python tools/auxk_bench.py --dead 6554       # N / 20
    timeout -k 10 600 python tools/auxk_bench.py --dead 32768      # N / 4

One process per dead count, no retries.  Three SaeTrainStep twins (the same seed) at d, N, k, T: auxk_alpha = 1/32 with
auxk_path="dense", the same with auxk_path="subset", and auxk_alpha = 0 (the benchmarked configuration).  After a warm-up the
three take one step each in turn, `--steps` times, device events around every step; before each AuxK step exactly `--dead`
features (a fixed random set) are marked dead through num_tokens_since_fired, outside the timed region.  The step's one host
read (the dead count) is inside it.  Then one more step per mode under reset_peak_memory_stats: the peak of
max_memory_allocated above the allocation at rest."""
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


def main(args) -> None:
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    dev = torch.device("cuda:0")
    k_aux = min(args.d // 2, args.dead)
    print(f"auxk: SaeTrainStep at d = {args.d}, N = {args.N}, k = {args.k}, T = {args.T}; {args.dead} dead features "
          f"({100.0 * args.dead / args.N:.2f} % of N), k_aux = {k_aux}; warm-up {args.warmup}, {args.steps} timed steps per mode, "
          "modes taking turns")
    dead = torch.randperm(args.N, generator=torch.Generator(device=dev).manual_seed(9), device=dev)[:args.dead]
    modes = [("auxk dense ", dict(auxk_alpha=1.0 / 32, auxk_path="dense")),
             ("auxk subset", dict(auxk_alpha=1.0 / 32, auxk_path="subset")),
             ("auxk_alpha=0", dict(auxk_alpha=0.0))]
    steps = []
    for _, kw in modes:
        torch.manual_seed(3)
        steps.append(SaeTrainStep(Sae(args.d, SaeConfig(num_latents=args.N, k=args.k), device=dev), **kw))

    def mark(ts):
        if ts.auxk_alpha > 0:
            ts.num_tokens_since_fired.zero_()
            ts.num_tokens_since_fired[dead] = ts.dead_feature_threshold + 1

    g = torch.Generator(device=dev).manual_seed(5)
    n = args.warmup + args.steps
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in modes] for _ in range(n)]
    aux = [[] for _ in modes]
    for i in range(n):
        x = torch.randn(args.T, args.d, generator=g, device=dev)
        for j, ts in enumerate(steps):
            mark(ts)
            e0, e1 = ev[i][j]
            e0.record()
            out = ts.step(x)
            e1.record()
            aux[j].append(out["auxk_loss"])
    torch.cuda.synchronize()
    for j, (name, _) in enumerate(modes):
        ms = [ev[i][j][0].elapsed_time(ev[i][j][1]) for i in range(args.warmup, n)]
        print(f"  {name:<13} {_stats(ms)}  last auxk_loss {float(aux[j][-1]):.6f}")
    x = torch.randn(args.T, args.d, generator=g, device=dev)
    for (name, _), ts in zip(modes, steps):
        mark(ts)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        ts.step(x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - base
        print(f"  {name:<13} peak allocated above rest {peak / 2**30:.3f} GiB ({peak} B); dense [T, N] f32 = "
              f"{args.T * args.N * 4 / 2**30:.3f} GiB")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dead", type=int, required=True)
    ap.add_argument("--N", type=int, default=131072)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--T", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measures on the GPU"
    main(a)
