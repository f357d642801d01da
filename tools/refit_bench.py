"""What the support refit (ops.support_refit, msae_support_refit_f32) costs at C2 width (d = 4096,
N = 131072, T = 8192, bf16 x), against the same coefficients composed in torch.  Writes profiles/refit.txt:

  fused        ops.support_refit: Gram matrix, Cholesky, both solves and the two error walks in one kernel per token
  composed     in chunks of CHUNK tokens: D = W_dec[idx] ([chunk, s, d] gathered), y = x.float() - b_dec, G = bmm(D, D^T),
               h = bmm(D, y), torch.linalg.cholesky, cholesky_solve, then the two reconstructions and their errors by bmm
  decode       one plain ops.decode of the k-wide list; recon_curve: one ops.recon_curve with ks = (0, s) -- the yardsticks
  cache loop   Sae.encode (fused) + Cache.add_recon + Cache.add_topk at T = 8192 (32 rows of 256) with recon on, on again
               (the twin: the spread every other difference is read against) and on with refit=True

  shapes       k = s = 32; k = s = 64; k = 256 refit on its first 64 slots (s=64, the list read in place)

Three input batches (activations and their lists from Sae.encode's kernel) take turns; the variants take turns inside ONE
process, one timed call of each per round after 3 warm-up rounds; REPS timed rounds; device events around each call.  Per
variant: the median, the interquartile range and the whole range (min .. max).  CONDITION: the fused median is not above the
composed median, at every shape.

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
d, N, T, REPS, NB, CHUNK = 4096, 131072, 8192, 12, 3, 512


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps=REPS):
    """variants: [(label, fn(round))] -> {label: [ms] * reps}; one timed call of each per round, 3 warm-up rounds."""
    ts = {label: [] for label, _ in variants}
    for rnd in range(3 + reps):
        for label, fn in variants:
            t = once(lambda: fn(rnd))
            if rnd >= 3:
                ts[label].append(t)
    return ts


def summary(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[2] - q[0], min(v), max(v)


def composed(x, vals, idx, W_dec, b_dec, s):
    coef, e_fit, e_enc = [], [], []
    for a in range(0, x.shape[0], CHUNK):
        D = W_dec[idx[a:a + CHUNK, :s]]                                  # [chunk, s, d]
        y = (x[a:a + CHUNK].float() - b_dec)[..., None]
        G, h = torch.bmm(D, D.transpose(1, 2)), torch.bmm(D, y)
        c = torch.cholesky_solve(h, torch.linalg.cholesky(G))
        coef.append(c[..., 0])
        e_fit.append((y - torch.bmm(D.transpose(1, 2), c)).square().sum((1, 2)))
        e_enc.append((y - torch.bmm(D.transpose(1, 2), vals[a:a + CHUNK, :s, None])).square().sum((1, 2)))
    return torch.cat(coef), torch.cat(e_fit), torch.cat(e_enc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "refit.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    W_enc, b_enc, W_dec, b_dec, x0 = bench.make_inputs(dev, T, d, N)
    xs = [x0] + [bench.make_inputs(dev, T, d, 8192, seed=s)[4] for s in range(1, NB)]
    prep = ops.prepare_encoder(W_enc)
    met = []
    for k, s in ((32, 32), (64, 64), (256, 64)):
        lists = [ops.encode_topk(x, W_enc, b_enc, b_dec, prep, k)[:2] for x in xs]
        raw = ops.support_refit(xs[0], *lists[0], W_dec, b_dec, s)
        ref = composed(xs[0], *lists[0], W_dec, b_dec, s)
        worst_c = float(((raw.coef - ref[0]).abs().amax(1) / ref[0].abs().amax(1)).max())
        worst_e = float(((raw.err_fit - ref[1]).abs() / ref[1]).max())
        variants = [
            ("fused", lambda r: ops.support_refit(xs[r % NB], *lists[r % NB], W_dec, b_dec, s)),
            ("composed", lambda r: composed(xs[r % NB], *lists[r % NB], W_dec, b_dec, s)),
            ("decode", lambda r: ops.decode(lists[r % NB][1], lists[r % NB][0], W_dec, b_dec)),
            ("recon_curve", lambda r: ops.recon_curve(xs[r % NB], *lists[r % NB], W_dec, b_dec, [0, s])),
        ]
        res = {label: summary(v) for label, v in alternate(variants).items()}
        lines.append(f"T={T} d={d} N={N} k={k} s={s} bf16 x, {REPS} timed rounds, {NB} input batches, composed in chunks of {CHUNK}")
        for label, (med, iqr, lo, hi) in res.items():
            lines.append(f"    {label:12s} median {med:8.3f} ms   iqr {iqr:6.3f} ms   range {lo:8.3f} .. {hi:8.3f} ms")
        f, c, y = res["fused"], res["composed"], res["decode"]
        met.append(f[0] <= c[0])
        lines.append(f"    composed / fused = {c[0] / f[0]:.2f}; fused / decode = {f[0] / y[0]:.2f}: condition "
                     f"{'MET' if met[-1] else 'NOT MET'}; worst relative difference fused vs composed: coef {worst_c:.2e} "
                     f"(of the token's largest), err_fit {worst_e:.2e}; dependent slots {int(raw.n_dependent.sum())}")
        del lists, raw, ref
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
    base = dict(ks=[0, 1, 2, 4, 8, 16, 32], position_edges=(0, S // 2))
    for label, recon in (("refit off", base), ("refit off'", base), ("refit on", dict(base, refit=True))):
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
    lines.append(f"cache loop T={T} k={k} rows={rows}x{S}, recon_stats on, two position groups")
    for label, _, cache in loops:
        cache.flush_pending()
        med, iqr, lo, hi = res[label]
        lines.append(f"    cache loop, {label:11s} median {med:8.3f} ms   iqr {iqr:6.3f} ms   range {lo:8.3f} .. {hi:8.3f} ms")
    off, twin, on = (res[label][0] for label, _, _ in loops)
    lines.append(f"    spread of the two identical variants {abs(off - twin):.3f} ms; on - off {on - off:+.3f} ms")
    lines.append("    after the run (random weights):")
    lines += ["    " + ln for ln in loops[2][2].recon_stats["layers.24"].summary().splitlines()]
    lines.append("")
    lines.append("CONDITION at every shape: " + ("MET" if all(met) else "NOT MET -- the fused kernel is slower than the composition"))
    print("\n".join(lines), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
