"""What the position profiles (PosProfile, msae_pos_profile_update / msae_pos_profile_summary) cost at C2 width (d = 4096,
N = 131072, k = 32), modelled on tools/act_hist_overhead.py.  Feature usage is Zipf-biased (the encoder's bias favours a few
features, so hot features fire on most tokens).  Writes profiles/pos_profile.txt:

  cache loop   Sae.encode (fused) + Cache.add_topk at T = 8192 (32 rows of 256) with the profiles off, off again (the twin:
               the difference of the two is the run-to-run spread every other difference has to be read against) and on
               (log2 bins over the row); the variants take turns inside ONE process, one timed step of each per round over
               BATCHES distinct input batches in rotation, medians over REPS rounds
  update alone text rows (32 x 256, log2 bins) and image rows (B = 4, S = 2880, the 24 x 24 grid in cells of 4 and the rest),
               each with the ActHist token update at the same shape taking turns with it; BATCHES distinct top-k batches in
               rotation
  contention   the update on planted lists at T = 8192: no feature twice (the floor), ONE feature with one value on every
               token into ONE bin, and the same feature spread over 36 bins
  summary      the peak bins of all 131072 features, 37 bins (the kernel), and `summary_host` on the CPU for scale

Every line: the median, and the range (min .. max) of the timed calls.
--out PATH   write there instead
--loop-only  only the cache loop with the profiles off (and its twin); with --tree PATH the package and bench.py are taken
             from another checkout (a build of the parent commit: its loop must match this one's "off")"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
dev = torch.device("cuda:0")
d, N, K, REPS, BATCHES = 4096, 131072, 32, 24, 4


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants):
    """variants: [(label, fn(round))] -> {label: (median, min, max) ms}; one timed call of each per round, 3 warm-up rounds."""
    ts = {label: [] for label, _ in variants}
    for rnd in range(3 + REPS):
        for label, fn in variants:
            t = once(lambda: fn(rnd))
            if rnd >= 3:
                ts[label].append(t)
    return {label: (statistics.median(v), min(v), max(v)) for label, v in ts.items()}


def fmt(label, t, width=44):
    return f"    {label:{width}s} {t[0]:7.3f} ms   ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
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
        xs = [x] + [x[torch.randperm(T, device=dev)] * (1.0 + 0.01 * j) for j in range(1, BATCHES)]
        return W_enc, b_enc, b_dec, ops.prepare_encoder(W_enc), xs

    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    T, rows = 8192, 32
    S = T // rows
    W_enc, b_enc, b_dec, prep, xs = encoder(T)
    tops = []
    for x in xs:
        v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
        tops.append((v.view(rows, S, K), i.view(rows, S, K)))
    hot = torch.bincount(tops[0][1].reshape(-1), minlength=N).max().item()
    lines.append(f"T={T} k={K} rows={rows}x{S}  hottest feature on {hot / T:.1%} of tokens  (tree: {tree.name})")

    # ---- the cache loop
    kinds = [("pos_profile off", None), ("pos_profile off'", None)]
    if not args.loop_only:
        from msae.features.pos import PosProfile

        table, tail, P, _ = PosProfile.log2_bins(S)
        kinds.append(("pos_profile on (log2)", dict(bins=table, tail_bin=tail, n_bins=P)))
    loops = []
    for label, pos in kinds:
        cache = Cache(0, None, batch_size=rows, **({} if pos is None else dict(pos=pos)))
        n = [0]

        def step(rnd, cache=cache, n=n):
            vv, ii, _ = ops.encode_topk(xs[rnd % BATCHES], W_enc, b_enc, b_dec, prep, K)
            cache.add_topk(vv.view(rows, S, K), ii.view(rows, S, K), N, n[0], "layers.24")
            n[0] += 1
        loops.append((label, step, cache))
    res = alternate([(label, step) for label, step, _ in loops])
    for label, _, cache in loops:
        cache.flush_pending()
        lines.append(fmt(f"cache loop, {label}", res[label]))
    off, twin = res["pos_profile off"][0], res["pos_profile off'"][0]
    lines.append(f"    spread of the two identical variants {abs(off - twin):.3f} ms"
                 + ("" if args.loop_only else f"; on - off {res['pos_profile on (log2)'][0] - off:+.3f} ms"))
    del loops, cache, step
    if args.loop_only:
        return finish(lines, args.out)

    from msae.features.hist import ActHist

    # ---- the updates alone, taking turns: text rows
    pp = PosProfile(N, table, tail, P, device=dev)
    ah = ActHist(N, pool="token", device=dev)
    res = alternate([("pos_profile update (text rows, log2: 9 bins)", lambda r: pp.update(*tops[r % BATCHES])),
                     ("act_hist update (token)", lambda r: ah.update(*tops[r % BATCHES]))])
    lines += [fmt(label, t) for label, t in res.items()]
    lines.append(f"    ({int((pp.count > 0).sum())} nonzero (feature, bin) counters after the run)")

    # ---- contention: planted lists
    g = torch.Generator(device="cpu").manual_seed(1)
    spread = torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(T)]).to(dev).view(rows, S, K)
    ones = torch.full((rows, S, K), 1.5, device=dev)
    one_hot = spread.clone(); one_hot[:, :, 11] = 7
    one_bin = PosProfile(N, [0] * S, n_bins=1, device=dev)
    bins36 = PosProfile(N, (torch.arange(S) % 36).tolist(), n_bins=36, device=dev)
    res = alternate([("update, no feature twice, 1 bin", lambda r: one_bin.update(ones, spread)),
                     ("update, 1 feature on every token, 1 bin", lambda r: one_bin.update(ones, one_hot)),
                     ("update, no feature twice, 36 bins", lambda r: bins36.update(ones, spread)),
                     ("update, 1 feature on every token, 36 bins", lambda r: bins36.update(ones, one_hot))])
    lines += [fmt(label, t) for label, t in res.items()]
    del one_bin, bins36, ah, pp, W_enc, prep, xs, tops
    torch.cuda.empty_cache()

    # ---- image rows: B = 4 rows of 2880 positions, the image launcher's default bins
    B, S2 = 4, 2880
    W_enc, b_enc, b_dec, prep, xs = encoder(B * S2)
    tops = []
    for x in xs:
        v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
        tops.append((v.view(B, S2, K), i.view(B, S2, K)))
    gt, gtail, gP, _ = PosProfile.grid_bins()
    pim = PosProfile(N, gt, gtail, gP, device=dev)
    him = ActHist(N, pool="token", device=dev)
    lines.append(f"T={B * S2} k={K} rows={B}x{S2}")
    res = alternate([("pos_profile update (image rows, grid: 37 bins)", lambda r: pim.update(*tops[r % BATCHES])),
                     ("act_hist update (token)", lambda r: him.update(*tops[r % BATCHES]))])
    lines += [fmt(label, t) for label, t in res.items()]

    # ---- the summary
    res = alternate([("summary N=131072 P=37 (kernel)", lambda r: pim.summary())])
    lines += [fmt(label, t) for label, t in res.items()]
    from msae.features.pos import summary_host

    count, bp = pim.count.cpu(), pim.bin_positions
    t0 = time.perf_counter(); hf, hp = summary_host(count, bp); t1 = time.perf_counter()
    fired, peak = pim.summary()
    assert torch.equal(fired.cpu(), hf) and torch.equal(peak.cpu(), hp)
    lines.append(f"    summary_host on the CPU, the same integers    {1e3 * (t1 - t0):7.1f} ms (one call)")
    finish(lines, args.out or str(REPO / "profiles" / "pos_profile.txt"))


def finish(lines, out):
    print("\n".join(lines), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
