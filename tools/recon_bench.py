"""What the reconstruction-error curve (ops.recon_curve, msae_recon_curve_f32) costs at C2 width
(d = 4096, N = 131072, T = 8192, bf16 x), against the same numbers composed from the older ops.  Writes profiles/recon.txt:

  fused        ops.recon_curve: one pass over the k decoder rows, the checkpoints reduced on the way
  composed     per checkpoint kappa: ops.decode over the first kappa columns (+ b_dec), then torch: e = r - x,
               e.square().sum(-1), (x * r).sum(-1), r.square().sum(-1); x.float() and its square sum once per call
  decode at k  one plain ops.decode of the whole list: the yardstick ("about one decode" was the expectation)
  cache loop   Sae.encode (fused) + Cache.add_recon + Cache.add_topk at T = 8192 (32 rows of 256) with recon off, off again
               (the twin: the spread every other difference is read against) and on (two position groups)

  shapes       k = 32 with ks = (0, 1, 2, 4, 8, 16, 32); k = 256 with ks = (0, 1, 2, 4, ..., 256)

Three input batches (activations and their lists from Sae.encode's kernel) take turns; the variants take turns inside ONE
process, one timed call of each per round after 3 warm-up rounds; REPS timed rounds; device events around each call.  Per
variant: the median, the interquartile range and the whole range (min .. max).  ACCEPTANCE: the fused median lies below the
composed median by more than the sum of the two spreads -- stated for both spreads.

--out PATH  write there instead"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "multimodal-sae_amd"))
import bench  # noqa: E402
from msae import Sae, SaeConfig, ops  # noqa: E402
from msae.features.cache import Cache  # noqa: E402

dev = torch.device("cuda:0")
d, N, T, REPS, NB = 4096, 131072, 8192, 24, 3


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants):
    """variants: [(label, fn(round))] -> {label: [ms] * REPS}; one timed call of each per round, 3 warm-up rounds."""
    ts = {label: [] for label, _ in variants}
    for rnd in range(3 + REPS):
        for label, fn in variants:
            t = once(lambda: fn(rnd))
            if rnd >= 3:
                ts[label].append(t)
    return ts


def summary(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[2] - q[0], min(v), max(v)


def composed(x, vals, idx, W_dec, b_dec, ks):
    xf = x.float()
    out = [xf.square().sum(-1)]
    for kappa in ks:
        if kappa == 0:
            r = b_dec.expand_as(xf)
        else:
            r = ops.decode(idx[:, :kappa].contiguous(), vals[:, :kappa].contiguous(), W_dec, b_dec)
        e = r - xf
        out += [e.square().sum(-1), (xf * r).sum(-1), r.square().sum(-1)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "recon.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    W_enc, b_enc, W_dec, b_dec, x0 = bench.make_inputs(dev, T, d, N)
    xs = [x0] + [bench.make_inputs(dev, T, d, 8192, seed=s)[4] for s in range(1, NB)]
    prep = ops.prepare_encoder(W_enc)
    accepted = []
    for k in (32, 256):
        ks = [0] + [1 << i for i in range(k.bit_length()) if (1 << i) <= k]
        lists = [ops.encode_topk(x, W_enc, b_enc, b_dec, prep, k)[:2] for x in xs]
        # the two paths agree (same meaning; the fused sums are ordered differently from torch's)
        mom, xx = ops.recon_curve(xs[0], *lists[0], W_dec, b_dec, ks)
        ref = composed(xs[0], *lists[0], W_dec, b_dec, ks)
        worst = max(float(((mom[:, c, m] - ref[1 + 3 * c + m]).abs() / (ref[1 + 3 * c + m].abs() + 1e-30)).max())
                    for c in range(len(ks)) for m in (0, 2))
        variants = [
            ("fused", lambda r: ops.recon_curve(xs[r % NB], *lists[r % NB], W_dec, b_dec, ks)),
            ("composed", lambda r: composed(xs[r % NB], *lists[r % NB], W_dec, b_dec, ks)),
            ("decode at k", lambda r: ops.decode(lists[r % NB][1], lists[r % NB][0], W_dec, b_dec)),
        ]
        res = {label: summary(v) for label, v in alternate(variants).items()}
        lines.append(f"T={T} d={d} N={N} k={k} ks={tuple(ks)} bf16 x, {REPS} timed rounds, {NB} input batches")
        for label, (med, iqr, lo, hi) in res.items():
            lines.append(f"    {label:12s} median {med:8.3f} ms   iqr {iqr:6.3f} ms   range {lo:8.3f} .. {hi:8.3f} ms")
        f, c, y = res["fused"], res["composed"], res["decode at k"]
        by_iqr = c[0] - f[0] > f[1] + c[1]
        by_range = c[0] - f[0] > (f[3] - f[2]) + (c[3] - c[2])
        accepted.append(by_iqr and by_range)
        lines.append(f"    composed - fused {c[0] - f[0]:+.3f} ms; sum of the spreads {f[1] + c[1]:.3f} ms (iqr), "
                     f"{(f[3] - f[2]) + (c[3] - c[2]):.3f} ms (range): acceptance {'MET' if by_iqr and by_range else 'NOT MET'}"
                     f" (iqr: {by_iqr}, range: {by_range})")
        lines.append(f"    fused / decode at k = {f[0] / y[0]:.2f}; composed / fused = {c[0] / f[0]:.2f}; "
                     f"worst relative difference fused vs composed (|e|^2, |r|^2) {worst:.2e}")
        del lists, mom, xx, ref
        torch.cuda.empty_cache()

    # ---- the cache loop, k = 32
    k, rows = 32, 32
    S = T // rows
    sae = Sae(d, SaeConfig(num_latents=N, k=k), device=dev)
    with torch.no_grad():
        sae.encoder.weight.copy_(W_enc); sae.encoder.bias.copy_(b_enc); sae.W_dec.copy_(W_dec); sae.b_dec.copy_(b_dec)
    sae.eval()
    del W_enc, W_dec, prep
    torch.cuda.empty_cache()
    loops = []
    for label, recon in (("recon off", None), ("recon off'", None),
                         ("recon on", dict(ks=[0, 1, 2, 4, 8, 16, 32], position_edges=(0, S // 2)))):
        cache = Cache(0, None, batch_size=rows, recon=recon)
        n = [0]

        def step(r, cache=cache, n=n):
            hidden = xs[r % NB].view(rows, S, d)
            top = sae.encode(hidden)
            cache.add_recon(hidden, top.top_acts, top.top_indices, sae, "layers.24")
            cache.add_topk(top.top_acts, top.top_indices, N, n[0], "layers.24")
            n[0] += 1
        loops.append((label, step, cache))
    with torch.no_grad():
        res = {label: summary(v) for label, v in alternate([(label, step) for label, step, _ in loops]).items()}
    lines.append(f"cache loop T={T} k={k} rows={rows}x{S}, two position groups")
    for label, _, cache in loops:
        cache.flush_pending()
        med, iqr, lo, hi = res[label]
        lines.append(f"    cache loop, {label:11s} median {med:8.3f} ms   iqr {iqr:6.3f} ms   range {lo:8.3f} .. {hi:8.3f} ms")
    off, twin, on = (res[label][0] for label, _, _ in loops)
    lines.append(f"    spread of the two identical variants {abs(off - twin):.3f} ms; on - off {on - off:+.3f} ms")
    st = loops[2][2].recon_stats["layers.24"]
    lines.append("    fvu per checkpoint after the run (random weights): " + " ".join(f"{v:.4f}" for v in st.fvu().tolist()))
    lines.append("")
    lines.append("ACCEPTANCE at both shapes: " + ("MET" if all(accepted) else "NOT MET -- the fused kernel does not beat the "
                                                   "composition by the required margin"))
    print("\n".join(lines), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
