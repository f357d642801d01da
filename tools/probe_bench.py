"""Sae.probe (fused: pooled GEMM + top-k of the pooled rows + map recompute) against the dense probe of
tools/probe_activations.py (pre_acts -> per-segment mean -> topk -> gather) at C2 width (d = 4096, N = 131072, k = 10), on one
MI355X.  Per case: wall time per call (device events, after a warm-up), the pooled kernel alone next to msae_pre_acts_f32 at
the same T (alternated, same inputs), and the peak torch.cuda.max_memory_allocated increase of each path.  The outputs of the
two paths' rankings are compared where the dense one fits (torch's mean is not the probe's sequential f64 sum, so a near
tie may rank differently; the values are not expected to match bit for bit).

    python tools/probe_bench.py [--reps 3] [--out profiles/probe.txt]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "multimodal-sae_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

D, N, K = 4096, 131072, 10
CASES = [("T=576, S=1", 1, 576, True), ("T=2880, S=1", 1, 2880, True), ("8 x 576, S=8", 8, 576, True),
         ("64 x 2880, S=64", 64, 2880, False)]


def timed(fn, reps):
    """(median ms per call, last result): device events around each call."""
    ts, out = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], out


def peak_mb(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, out


def dense_probe(sae, x, segs, k):
    """tools/probe_activations.py:116-126 per segment, batched: latents -> mean -> topk -> gather."""
    from msae import ops

    lat = sae.pre_acts(x)
    pooled = torch.stack([lat[b:e].mean(0) for b, e in segs])
    vals, idx = ops.topk(pooled, k)
    maps = torch.zeros(x.shape[0], k, device=x.device)
    for s, (b, e) in enumerate(segs):
        maps[b:e] = lat[b:e][:, idx[s]]
    return vals, idx, maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from msae import Sae, SaeConfig, ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    sae = Sae(D, SaeConfig(num_latents=N, k=32), device=dev, decoder=False).eval().requires_grad_(False)
    with torch.no_grad():
        for r0 in range(0, N, 16384):
            blk = torch.randn(16384, D, generator=g, device=dev)
            sae.encoder.weight[r0:r0 + 16384] = blk / blk.norm(dim=1, keepdim=True)
        sae.encoder.bias.copy_(torch.randn(N, generator=g, device=dev) * 0.02)
        sae.b_dec.copy_(torch.randn(D, generator=g, device=dev) * 0.1)
    W, be, bd = sae.encoder.weight, sae.encoder.bias, sae.b_dec
    lines = [f"# tools/probe_bench.py: d={D} N={N} k={K}, x bf16, reps={args.reps} (median), {torch.cuda.get_device_name(dev)}",
             "# case | fused Sae.probe ms | dense probe ms | pooled kernel ms | msae_pre_acts_f32 ms (same T) | pooled/pre_acts"
             " | fused peak MB | dense peak MB | same top-k indices as dense"]
    print(lines[0], "\n" + lines[1], flush=True)
    for name, B, L, dense_fits in CASES:
        T = B * L
        x = (torch.randn(T, D, generator=g, device=dev) + 0.25).to(torch.bfloat16)
        segs = [(b * L, (b + 1) * L) for b in range(B)]
        seg_dev = torch.tensor(segs, dtype=torch.int32, device=dev)
        from msae.sae.probe import plan_chunks

        plan = torch.tensor(plan_chunks(segs, N, torch.cuda.get_device_properties(dev).multi_processor_count),
                            dtype=torch.int32, device=dev)
        fused = lambda: sae.probe(x, K, segments=segs)                                   # noqa: E731
        pooled = lambda: ops.pooled_acts(x, W, be, bd, seg_dev, plan, 0)                  # noqa: E731
        if dense_fits:
            pre = lambda: ops.pre_acts(x, W, be, bd)                                      # noqa: E731
            pre_label = ""
        else:   # [T, N] f32 would be 96 GB: msae_pre_acts_f32 over one 2880-row slice at a time into one buffer
            buf = torch.empty(L, N, device=dev)
            lib = __import__("msae._hip", fromlist=["_hip"])

            def pre():
                for b in range(B):
                    xs = x[b * L:(b + 1) * L]
                    lib.check(lib.load().msae_pre_acts_f32(lib.ptr(xs), 1, lib.ptr(W), lib.ptr(be), lib.ptr(bd), L, D, N,
                                                           1, lib.ptr(buf), lib.stream_of(xs)), "pre_acts")
            pre_label = f" ({B} x {L}-row slices)"
        fused()                                                                            # warm-up: every shape once
        pooled()
        pre()
        t_fused, out = timed(fused, args.reps)
        t_pool, t_pre = [], []
        for _ in range(args.reps):                                                         # alternated
            t_pre.append(timed(pre, 1)[0])
            t_pool.append(timed(pooled, 1)[0])
        t_pool, t_pre = sorted(t_pool)[len(t_pool) // 2], sorted(t_pre)[len(t_pre) // 2]
        m_fused, _ = peak_mb(fused, dev)
        if dense_fits:
            dense_probe(sae, x, segs, K)
            t_dense, ref = timed(lambda: dense_probe(sae, x, segs, K), args.reps)
            m_dense, _ = peak_mb(lambda: dense_probe(sae, x, segs, K), dev)
            same = torch.equal(out.indices, ref[1])
            dense_s, mdense_s, same_s = f"{t_dense:.2f}", f"{m_dense:.0f}", str(same)
        else:
            dense_s, mdense_s, same_s = "does not fit", f"{T * N * 4 / 2**20:.0f} (latents alone)", "n/a"
        line = (f"{name} | {t_fused:.2f} | {dense_s} | {t_pool:.2f} | {t_pre:.2f}{pre_label} | {t_pool / t_pre:.3f} | "
                f"{m_fused:.0f} | {mdense_s} | {same_s}")
        lines.append(line)
        print(line, flush=True)
        del x
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
