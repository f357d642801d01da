"""What the per-feature statistics (FeatureStats, msae_feature_stats_update) add to the cache loop at C2 width
(d = 4096, N = 131072): Sae.encode (fused) + Cache.add_topk with stats off and on, same batches, per-batch median of
CUDA-event timings, and the statistics update alone.  Feature usage is Zipf-biased: the encoder's bias favours a few
features, so hot features fire on most tokens.  Shapes: T = 8192 at k = 32 and 256 (window mode, W = 64, rows of
256 tokens), T = 2880 in image mode (one row of 2880 tokens, P = 576).  Writes profiles/feature_stats_overhead.txt.

--n_sample N [N ...]  also time the update with the uniform example sample on (FeatureStats(n_sample=N)), one variant per N
--parent_lib PATH     also time the sample-off path of ANOTHER build of libmsae_hip.so (the parent commit's, built into a
                      scratch directory), loaded beside this build's: is the sample-off path still the same code?
--out PATH            write there instead

With either of the first two, all variants of a shape run in ONE process and ALTERNATE (one timed step of each per
round, REPS rounds), and the sample-off variant of this build runs twice ("off" and "off'"): the difference of those two is
the run-to-run spread every other difference has to be read against."""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "multimodal-sae_amd"))
import bench  # noqa: E402
from msae import _hip, ops  # noqa: E402
from msae.features.cache import Cache  # noqa: E402
from msae.features.stats import FeatureStats  # noqa: E402

dev = torch.device("cuda:0")
d, N, REPS = 4096, 131072, 24


def timed(fn):
    ts = []
    for _ in range(REPS):
        ts.append(once(fn))
    return statistics.median(ts)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def load_other(path):
    """Another build of the library beside this one: the symbols it has get their prototypes (an older build lacks the
    newer entry points; the sample-off path needs none of them)."""
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in _hip.PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    assert lib.msae_abi_version() == _hip.ABI_VERSION
    return lib


def shape(T, k, rows, pool, W_enc, b_enc, b_dec, prep, x):
    S = T // rows
    stats = dict(pool="window", window=64) if pool == "window" else dict(pool="image", pool_len=576)
    v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, k)
    v, i = v.view(rows, S, k), i.view(rows, S, k)
    hot = torch.bincount(i.reshape(-1), minlength=N).max().item()
    res = {}
    for on in (False, True):
        cache = Cache(0, None, batch_size=rows, stats=stats if on else None)
        n = [0]

        def step():
            vv, ii, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, k)
            cache.add_topk(vv.view(rows, S, k), ii.view(rows, S, k), N, n[0], "layers.24")
            n[0] += 1
        for _ in range(3):
            step()
        res[on] = timed(step)
        cache.flush_pending()
    st = FeatureStats(N, device=dev, **stats)
    base = [0]

    def upd():
        st.update(v, i, base[0]); base[0] += rows
    upd()
    alone = timed(upd)
    over = (res[True] - res[False]) / res[False] * 100
    return (f"T={T:5d} k={k:3d} {pool:6s} rows={rows:3d}x{S:4d}  hottest feature on {hot / T:6.1%} of tokens | "
            f"loop stats off {res[False]:.3f} ms  on {res[True]:.3f} ms  (+{over:.1f} %) | update alone {alone:.3f} ms"), over


def shape_variants(T, k, rows, pool, W_enc, b_enc, b_dec, prep, x, variants):
    """variants: [(label, library handle, n_sample)] -> one line per variant: cache loop and update alone, medians over REPS
    rounds in which the variants take turns."""
    S = T // rows
    stats = dict(pool="window", window=64) if pool == "window" else dict(pool="image", pool_len=576)
    v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, k)
    v, i = v.view(rows, S, k), i.view(rows, S, k)
    mine = _hip.load()
    runs = []
    for label, lib, n_sample in variants:
        cache = Cache(0, None, batch_size=rows, stats=dict(stats, n_sample=n_sample))
        st = FeatureStats(N, device=dev, n_sample=n_sample, **stats)
        runs.append(dict(label=label, lib=lib, cache=cache, st=st, n=0, base=0, loop=[], alone=[]))

    def step(r):
        vv, ii, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, k)
        r["cache"].add_topk(vv.view(rows, S, k), ii.view(rows, S, k), N, r["n"], "layers.24")
        r["n"] += 1

    def upd(r):
        r["st"].update(v, i, r["base"]); r["base"] += rows
    try:
        for rnd in range(3 + REPS):
            for r in runs:
                _hip._lib = r["lib"]
                tl, ta = once(lambda: step(r)), once(lambda: upd(r))
                if rnd >= 3:
                    r["loop"].append(tl), r["alone"].append(ta)
    finally:
        _hip._lib = mine
    lines = [f"T={T:5d} k={k:3d} {pool:6s} rows={rows:3d}x{S:4d}"]
    ref_alone = statistics.median(runs[0]["alone"])
    for r in runs:
        r["cache"].flush_pending()
        loop, alone = statistics.median(r["loop"]), statistics.median(r["alone"])
        lines.append(f"    {r['label']:22s} loop {loop:7.3f} ms | update alone {alone:6.3f} ms  ({alone / ref_alone:4.2f} x the first line)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_sample", type=int, nargs="*", default=[])
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=str(REPO / "profiles" / "feature_stats_overhead.txt"))
    args = ap.parse_args()
    alternating = bool(args.n_sample or args.parent_lib)
    variants = []
    if alternating:
        mine = _hip.load()
        variants = [("this build, sample off", mine, 0)]
        if args.parent_lib:
            variants.append(("parent build, sample off", load_other(args.parent_lib), 0))
        variants.append(("this build, sample off'", mine, 0))
        variants += [(f"this build, n_sample {n}", mine, n) for n in args.n_sample]
    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    worst = 0.0
    for T, k, rows, pool in ((8192, 32, 32, "window"), (8192, 256, 32, "window"), (2880, 32, 1, "image")):
        W_enc, b_enc, W_dec, b_dec, x = bench.make_inputs(dev, T, d, N)
        with torch.no_grad():   # Zipf-biased usage: bias rank r gets +c / r^0.5 on top of the weights' own spread
            ranks = torch.randperm(N, device=dev).float() + 1
            b_enc.add_(b_enc.abs().mean() * 8 / ranks.sqrt())
        prep = ops.prepare_encoder(W_enc)
        if alternating:
            out = shape_variants(T, k, rows, pool, W_enc, b_enc, b_dec, prep, x, variants)
            print("\n".join(out), flush=True)
            lines += out
        else:
            line, over = shape(T, k, rows, pool, W_enc, b_enc, b_dec, prep, x)
            print(line, flush=True)
            lines.append(line)
            if T == 8192 and k == 32:
                worst = over
        del W_enc, W_dec, prep
        torch.cuda.empty_cache()
    if not alternating:
        verdict = "within" if worst <= 5 else "ABOVE"
        lines += ["", f"target: <= 5 % at T = 8192, k = 32 -> measured +{worst:.1f} %: {verdict} the target"]
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
