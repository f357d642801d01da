"""What the activation histograms (ActHist, msae_act_hist_update / msae_act_hist_quantiles) cost at C2 width (d = 4096,
N = 131072, k = 32), modelled on tools/coact_overhead.py.  Feature usage is Zipf-biased (the encoder's bias favours a few
features, so hot features fire on most tokens).  Writes profiles/act_hist.txt:

  cache loop   Sae.encode (fused) + Cache.add_topk at T = 8192 (32 rows of 256) with the histograms off, off again (the twin:
               the difference of the two is the run-to-run spread every other difference has to be read against) and on
               (token pool); the variants take turns inside ONE process, one timed step of each per round, medians over REPS
               rounds
  update alone each pool at T = 8192 (32 rows of 256; window 64; pool_len 576, i.e. the whole row), with the feature
               statistics' update (window pool) and the co-activation update (token pool, 5000 queries) at the same shape
               taking turns with them; the image pool also at B = 4, S = 2880, P = 576
  contention   the token update on planted lists: no feature twice (the floor), ONE feature with one value on every token,
               and all 32 slots of every token taken by the same 32 features with one value each (every add of the call
               lands on 32 addresses)
  quantiles    quantile_bins for all 131072 features at Q = 7

--out PATH   write there instead
--parent_lib PATH  also time every pooled update of ANOTHER build of libmsae_hip.so (the parent commit's, built into a scratch
             directory), loaded beside this build's and called through ctypes on the same buffers: the histograms', the feature
             statistics' and the co-activation counters' update, per pool, this build, the parent's and the parent's again (the
             twin: its difference from the first is the run-to-run spread the difference of the builds has to be read against)
--loop-only  only the cache loop with the histograms off (and its twin); with --tree PATH the package and bench.py are taken
             from another checkout (a build of the parent commit: its loop must match this one's "off")"""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
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


def load_other(path, _hip):
    """Another build of the library beside this one, with this build's prototypes (the ABI version must agree)."""
    lib = ctypes.CDLL(str(path))
    for name, (res, argtypes) in _hip.PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    assert lib.msae_abi_version() == _hip.ABI_VERSION
    return lib


def against_parent(mine, parent, v, i, pool_len, pools=("token", "window", "image")):
    """Lines: every pooled update at the shape of v / i [B, S, K] through the C ABI, the builds taking turns on ONE set of
    buffers (the state's contents do not change what an update costs; window 64)."""
    from msae import _hip
    from msae.features.coact import POOL_MODES

    B, S, k = v.shape
    vals, idx = v.float().contiguous(), i.to(torch.int32).contiguous()
    ws = torch.empty(max(f(B * S, k, N) for f in (mine.msae_feature_stats_ws_bytes, mine.msae_coact_ws_bytes,
                                                   mine.msae_act_hist_ws_bytes)), dtype=torch.uint8, device=dev)
    hist = torch.zeros(N, 256, dtype=torch.int32, device=dev)
    count, act_max = torch.zeros(N, dtype=torch.int64, device=dev), torch.full((N,), float("-inf"), device=dev)
    act_sum, top_val = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, 64, device=dev)
    top_id = torch.full((N, 64), -1, dtype=torch.int64, device=dev)
    slot_of = torch.full((N,), -1, dtype=torch.int32, device=dev)
    slot_of[torch.randperm(N, device=dev)[:F]] = torch.arange(F, dtype=torch.int32, device=dev)
    counts, seg_count = torch.zeros(F, N, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
    P, st, base = _hip.ptr, _hip.stream_of(vals), [0]
    head = (P(vals), P(idx), B, S, k, 1e-5, N)
    tail = (P(ws), ws.numel(), st)

    def call(lib, what, pool):
        pool_args = (POOL_MODES[pool], pool_len, 64)
        if what == "act_hist":
            rc = lib.msae_act_hist_update(*head, *pool_args, 3, -16, 32, P(hist), *tail)
        elif what == "coact":
            rc = lib.msae_coact_update(*head, *pool_args, P(slot_of), F, P(counts), P(seg_count), *tail)
        else:
            rc = lib.msae_feature_stats_update(*head, *pool_args, base[0], 64, P(count), P(act_max), P(act_sum), P(top_val),
                                               P(top_id), *tail)
            base[0] += B
        assert rc == 0, (what, pool, rc)

    lines = []
    for what in ("act_hist", "feature_stats", "coact"):
        for pool in pools:
            if what == "feature_stats" and pool == "token":
                continue
            res = alternate([(label, lambda lib=lib: call(lib, what, pool))
                             for label, lib in (("this", mine), ("parent", parent), ("parent'", parent))])
            this, par, twin = res["this"], res["parent"], res["parent'"]
            lines.append(f"    {what} update ({pool}, T={B * S})".ljust(42) + f"this {this:7.3f} ms  parent {par:7.3f} ms  parent' "
                         f"{twin:7.3f} ms | this - parent {this - par:+.3f} ms, twin spread {abs(par - twin):.3f} ms")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--tree", default=str(REPO))
    args = ap.parse_args()
    tree = Path(args.tree).resolve()
    sys.path.insert(0, str(tree)); sys.path.insert(0, str(tree / "multimodal-sae_amd"))
    import bench
    from msae import ops
    from msae.features.cache import Cache

    def encoder(T):
        W_enc, b_enc, W_dec, b_dec, x = bench.make_inputs(dev, T, d, N)
        with torch.no_grad():   # Zipf-biased usage: bias rank r gets +c / r^0.5 on top of the weights' own spread
            ranks = torch.randperm(N, device=dev).float() + 1
            b_enc.add_(b_enc.abs().mean() * 8 / ranks.sqrt())
        del W_dec
        return W_enc, b_enc, b_dec, ops.prepare_encoder(W_enc), x

    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    T, rows = 8192, 32
    S = T // rows
    W_enc, b_enc, b_dec, prep, x = encoder(T)
    v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
    v, i = v.view(rows, S, K), i.view(rows, S, K)
    hot = torch.bincount(i.reshape(-1), minlength=N).max().item()
    lines.append(f"T={T} k={K} rows={rows}x{S}  hottest feature on {hot / T:.1%} of tokens  (tree: {tree.name})")

    # ---- the cache loop
    kinds = [("act_hist off", None), ("act_hist off'", None)]
    if not args.loop_only:
        kinds.append(("act_hist on (token)", dict(pool="token")))
    loops = []
    for label, hist in kinds:
        cache = Cache(0, None, batch_size=rows, **({} if hist is None else dict(hist=hist)))
        n = [0]

        def step(cache=cache, n=n):
            vv, ii, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
            cache.add_topk(vv.view(rows, S, K), ii.view(rows, S, K), N, n[0], "layers.24")
            n[0] += 1
        loops.append((label, step, cache))
    res = alternate([(label, step) for label, step, _ in loops])
    for label, _, cache in loops:
        cache.flush_pending()
        lines.append(f"    cache loop, {label:20s} {res[label]:7.3f} ms")
    off, twin = res["act_hist off"], res["act_hist off'"]
    lines.append(f"    spread of the two identical variants {abs(off - twin):.3f} ms"
                 + ("" if args.loop_only else f"; on - off {res['act_hist on (token)'] - off:+.3f} ms"))
    del loops, cache, step
    if args.loop_only:
        return finish(lines, args.out)

    from msae.features.coact import CoactStats
    from msae.features.hist import ActHist
    from msae.features.stats import FeatureStats

    # ---- the updates alone, taking turns
    hists = {pool: ActHist(N, pool=pool, window=64, pool_len=576, device=dev) for pool in ("token", "window", "image")}
    fs = FeatureStats(N, device=dev, pool="window", window=64)
    co = CoactStats(N, torch.randperm(N)[:F].tolist(), pool="token", device=dev)
    base = [0]

    def fs_update():
        fs.update(v, i, base[0]); base[0] += rows
    variants = [(f"act_hist update ({pool})", lambda h=h: h.update(v, i)) for pool, h in hists.items()]
    variants += [("feature statistics update (window)", fs_update), ("coact update (token, F=5000)", lambda: co.update(v, i))]
    for label, t in alternate(variants).items():
        lines.append(f"    {label:40s} {t:7.3f} ms")
    lines.append(f"    ({int((hists['token'].hist > 0).sum())} nonzero token-pool counters after the run)")
    parent = None
    if args.parent_lib:
        from msae import _hip
        parent = load_other(args.parent_lib, _hip)
        lines.append("  this build against the parent's (--parent_lib), through the C ABI on the same buffers")
        lines += against_parent(_hip.load(), parent, v, i, 576)

    # ---- quantiles
    st = hists["token"]
    qs = [0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99]
    q = alternate([("quantile_bins N=131072 Q=7", lambda: st.quantile_bins(qs)),
                   ("quantile_bins N=131072 Q=7, zeros", lambda: st.quantile_bins(qs, zeros=True))])
    for label, t in q.items():
        lines.append(f"    {label:40s} {t:7.3f} ms")

    # ---- contention: planted lists
    g = torch.Generator(device="cpu").manual_seed(1)
    spread = torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(T)]).to(dev).view(rows, S, K)
    ones = torch.full((rows, S, K), 1.5, device=dev)
    one_hot = spread.clone(); one_hot[:, :, 11] = 7
    all_hot = torch.arange(K, device=dev).expand(rows, S, K).contiguous()
    cont = ActHist(N, pool="token", device=dev)
    res = alternate([("token update, no feature twice", lambda: cont.update(ones, spread)),
                     ("token update, 1 feature on every token", lambda: cont.update(ones, one_hot)),
                     ("token update, the same 32 on every token", lambda: cont.update(ones, all_hot))])
    for label, t in res.items():
        lines.append(f"    {label:40s} {t:7.3f} ms")
    del hists, fs, co, cont, W_enc, prep
    torch.cuda.empty_cache()

    # ---- image pool: B = 4 rows of 2880 positions
    B, S2 = 4, 2880
    W_enc, b_enc, b_dec, prep, x = encoder(B * S2)
    v2, i2, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
    v2, i2 = v2.view(B, S2, K), i2.view(B, S2, K)
    him = ActHist(N, pool="image", pool_len=576, device=dev)
    fim = FeatureStats(N, device=dev, pool="image", pool_len=576)
    b2 = [0]

    def fim_update():
        fim.update(v2, i2, b2[0]); b2[0] += B
    lines.append(f"T={B * S2} k={K} rows={B}x{S2} P=576")
    for label, t in alternate([("act_hist update (image)", lambda: him.update(v2, i2)),
                               ("feature statistics update (image)", fim_update)]).items():
        lines.append(f"    {label:40s} {t:7.3f} ms")
    if parent is not None:
        lines += against_parent(_hip.load(), parent, v2, i2, 576, pools=("image",))
    finish(lines, args.out or str(REPO / "profiles" / "act_hist.txt"))


def finish(lines, out):
    print("\n".join(lines), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
