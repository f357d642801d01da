"""What the co-activation counters (CoactStats, msae_coact_update / msae_coact_topk) cost at C2 width (d = 4096, N = 131072,
k = 32, F = 5000 random query features), modelled on tools/feature_stats_overhead.py.  Feature usage is Zipf-biased (the
encoder's bias favours a few features, so hot features fire on most tokens).  Writes profiles/coact.txt:

  cache loop   Sae.encode (fused) + Cache.add_topk at T = 8192 (32 rows of 256) with coact off, off again (the twin: the
               difference of the two is the run-to-run spread every other difference has to be read against) and on (token
               pool); the variants take turns inside ONE process, one timed step of each per round, medians over REPS rounds
  update alone token pool at T = 8192; image pool at B = 4, S = 2880, P = 576; each also with a slot table that names no
               query (everything but the pair adds: load, sort, run heads, seg_count), and the feature statistics' update
               (window pool, W = 64) at the token shape beside them
  neighbours   coact_topk at F = 5000, m = 10, both metrics

--out PATH  write there instead"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "multimodal-sae_amd"))
import bench  # noqa: E402
from msae import ops  # noqa: E402
from msae.features.cache import Cache  # noqa: E402
from msae.features.coact import POOL_MODES, CoactStats  # noqa: E402
from msae.features.stats import FeatureStats  # noqa: E402

dev = torch.device("cuda:0")
d, N, K, F, REPS = 4096, 131072, 32, 5000, 24


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants):
    """variants: [(label, fn)] -> {label: median ms}; one timed call of each per round, 3 warm-up rounds."""
    ts = {label: [] for label, _ in variants}
    for rnd in range(3 + REPS):
        for label, fn in variants:
            t = once(fn)
            if rnd >= 3:
                ts[label].append(t)
    return {label: statistics.median(v) for label, v in ts.items()}


def encoder(T):
    W_enc, b_enc, W_dec, b_dec, x = bench.make_inputs(dev, T, d, N)
    with torch.no_grad():   # Zipf-biased usage: bias rank r gets +c / r^0.5 on top of the weights' own spread
        ranks = torch.randperm(N, device=dev).float() + 1
        b_enc.add_(b_enc.abs().mean() * 8 / ranks.sqrt())
    del W_dec
    return W_enc, b_enc, b_dec, ops.prepare_encoder(W_enc), x


def update_alone(v, i, pool, queries, extra=()):
    st = CoactStats(N, queries, pool=pool, pool_len=576, device=dev)
    slot_of, _ = st._device_lists()
    nobody = torch.full_like(slot_of, -1)
    variants = [("update", lambda: st.update(v, i)),
                ("update, no query named", lambda: torch.ops.msae.coact_update(
                    v, i, st.thresh, POOL_MODES[pool], st.pool_len, st.window, nobody, st.counts, st.seg_count))]
    res = alternate(variants + list(extra))
    members = int((st.counts > 0).sum())
    return st, res, members


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "coact.txt"))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    queries = torch.randperm(N)[:F].tolist()

    # ---- T = 8192: the cache loop and the token update
    T, rows = 8192, 32
    S = T // rows
    W_enc, b_enc, b_dec, prep, x = encoder(T)
    v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
    v, i = v.view(rows, S, K), i.view(rows, S, K)
    hot = torch.bincount(i.reshape(-1), minlength=N).max().item()
    lines.append(f"T={T} k={K} rows={rows}x{S}  F={F}  hottest feature on {hot / T:.1%} of tokens")
    loops = []
    for label, coact in (("coact off", None), ("coact off'", None), ("coact on (token)", dict(pool="token", queries=queries))):
        cache = Cache(0, None, batch_size=rows, coact=coact)
        n = [0]

        def step(cache=cache, n=n):
            vv, ii, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
            cache.add_topk(vv.view(rows, S, K), ii.view(rows, S, K), N, n[0], "layers.24")
            n[0] += 1
        loops.append((label, step, cache))
    res = alternate([(label, step) for label, step, _ in loops])
    for label, _, cache in loops:
        cache.flush_pending()
        lines.append(f"    cache loop, {label:18s} {res[label]:7.3f} ms")
    off, twin, on = (res[label] for label, _, _ in loops)
    lines.append(f"    spread of the two identical variants {abs(off - twin):.3f} ms; on - off {on - off:+.3f} ms")
    del loops, cache, step
    fs = FeatureStats(N, device=dev, pool="window", window=64)
    base = [0]

    def fs_update():
        fs.update(v, i, base[0]); base[0] += rows
    st, res, members = update_alone(v, i, "token", queries, extra=[("feature statistics update (window)", fs_update)])
    for label, t in res.items():
        lines.append(f"    token pool, {label:36s} {t:7.3f} ms")
    lines.append(f"    ({members} nonzero counters after the run)")
    nb = alternate([(f"coact_topk m=10 {metric}", lambda metric=metric: st.neighbors(k=10, metric=metric))
                    for metric in ("jaccard", "count")])
    for label, t in nb.items():
        lines.append(f"    neighbours F={F}, {label:24s} {t:7.3f} ms")
    del st, fs, W_enc, prep
    torch.cuda.empty_cache()

    # ---- image pool: B = 4 rows of 2880 positions
    B, S = 4, 2880
    W_enc, b_enc, b_dec, prep, x = encoder(B * S)
    v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
    v, i = v.view(B, S, K), i.view(B, S, K)
    st, res, members = update_alone(v, i, "image", queries)
    lines.append(f"T={B * S} k={K} rows={B}x{S} P=576  F={F}")
    for label, t in res.items():
        lines.append(f"    image pool, {label:36s} {t:7.3f} ms")
    lines.append(f"    ({members} nonzero counters after the run)")
    print("\n".join(lines), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
