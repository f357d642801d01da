"""What the token profiles (TokenProfile, msae_token_profile_update / msae_token_profile_topk) cost at C2 width (d = 4096,
N = 131072, k = 32), modelled on tools/pos_profile_overhead.py: 8192 tokens as 128 rows of 64 positions, F = 5000 query
features (the 5000 most used of the batch, so that the queries fire), V = 32000 and V = 128256, token ids Zipf-distributed over
the vocabulary.  Feature usage is Zipf-biased (the encoder's bias favours a few features).  Writes profiles/token_profile.txt:

  update alone the update for offsets (0,) and (-1, 0, 1), with and without mass, and the PosProfile update (log2 bins) on the
               same pairs taking turns with it in ONE process; BATCHES distinct batches in rotation
  hot batch    offsets (0,), with mass: every id ONE token and query 0 planted on every position, against the same list with
               8192 DISTINCT ids -- next to two identical runs of the ordinary batch (the twins: their difference is the
               run-to-run spread every other difference has to be read against)
  cache loop   Sae.encode (fused) + Cache.add_topk at T = 8192 with the profiles off, off again (the twin) and on (offsets
               (-1, 0, 1), with mass); one timed step of each per round, medians over REPS rounds
  top tokens   top_tokens(m = 10) over all F rows of one plane, per metric (the kernel)

Every line: the median, and the range (min .. max) of the timed calls.
--out PATH   write there instead"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
dev = torch.device("cuda:0")
d, N, K, REPS, BATCHES, F = 4096, 131072, 32, 24, 4, 5000
T, ROWS = 8192, 128
S = T // ROWS


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


def fmt(label, t, width=58):
    return f"    {label:{width}s} {t[0]:7.3f} ms   ({t[1]:.3f} .. {t[2]:.3f})"


def zipf_ids(V, g):
    """[ROWS, S] token ids, rank r of the vocabulary with weight 1 / (r + 1)."""
    w = 1.0 / torch.arange(1, V + 1, dtype=torch.float64)
    return torch.multinomial(w, T, replacement=True, generator=g).view(ROWS, S).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "multimodal-sae_amd"))
    import bench
    from msae import ops
    from msae.features.cache import Cache
    from msae.features.pos import PosProfile
    from msae.features.tokens import TokenProfile

    torch.manual_seed(0)
    g = torch.Generator(device="cpu").manual_seed(1)
    lines = [__doc__.strip(), ""]
    W_enc, b_enc, W_dec, b_dec, x = bench.make_inputs(dev, T, d, N)
    with torch.no_grad():       # Zipf-biased usage: bias rank r gets +c / r^0.5 on top of the weights' own spread
        ranks = torch.randperm(N, device=dev).float() + 1
        b_enc.add_(b_enc.abs().mean() * 8 / ranks.sqrt())
    del W_dec
    prep = ops.prepare_encoder(W_enc)
    xs = [x] + [x[torch.randperm(T, device=dev)] * (1.0 + 0.01 * j) for j in range(1, BATCHES)]
    tops = []
    for xb in xs:
        v, i, _ = ops.encode_topk(xb, W_enc, b_enc, b_dec, prep, K)
        tops.append((v.view(ROWS, S, K), i.view(ROWS, S, K)))
    use = torch.bincount(tops[0][1].reshape(-1), minlength=N)
    queries = torch.sort(torch.topk(use, F).indices).values.cpu()
    is_q = torch.zeros(N, dtype=torch.bool, device=dev)
    is_q[queries.to(dev)] = True
    share = is_q[tops[0][1].reshape(-1)].float().mean().item()
    lines.append(f"T={T} k={K} rows={ROWS}x{S} F={F}  hottest feature on {use.max().item() / T:.1%} of tokens, "
                 f"{share:.1%} of the entries name a query")
    table, tail, P, _ = PosProfile.log2_bins(S)

    for V in (32000, 128256):
        ids = [zipf_ids(V, g) for _ in range(BATCHES)]
        lines.append(f"V={V}")
        # ---- (a) the update alone
        pp = PosProfile(N, table, tail, P, device=dev)
        variants = [("pos_profile update (log2: 7 bins), the same pairs", lambda r: pp.update(*tops[r % BATCHES]))]
        profiles = {}
        for offs in ((0,), (-1, 0, 1)):
            for mass in (False, True):
                tp = TokenProfile(N, queries, V, offsets=offs, mass=mass, device=dev, max_bytes=64 << 30)
                label = f"token_profile update, offsets {offs}, {'with' if mass else 'no'} mass"
                profiles[label] = tp
                variants.append((label, lambda r, tp=tp: tp.update(*tops[r % BATCHES], ids[r % BATCHES])))
        res = alternate(variants)
        lines += [fmt(label, t) for label, t in res.items()]
        tp3 = profiles["token_profile update, offsets (-1, 0, 1), with mass"]
        lines.append(f"    ({int((tp3.counts > 0).sum())} nonzero (offset, query, token) cells after the run, of {tp3.counts.numel()})")
        del profiles, variants, pp, tp

        # ---- (b) the hot batch
        q0 = int(queries[0])
        planted = tops[0][1].clone(); planted[:, :, 0] = q0
        pvals = tops[0][0].clone(); pvals[:, :, 0] = 1.5
        hot_ids = torch.full((ROWS, S), 17, dtype=torch.int64, device=dev)
        distinct_ids = torch.randperm(V, generator=g)[:T].view(ROWS, S).to(dev)
        tps = [TokenProfile(N, queries, V, mass=True, device=dev, max_bytes=64 << 30) for _ in range(4)]
        res = alternate([("update, ordinary batch", lambda r: tps[0].update(*tops[0], ids[0])),
                         ("update, ordinary batch' (the twin)", lambda r: tps[1].update(*tops[0], ids[0])),
                         ("update, query on every position, 8192 distinct ids", lambda r: tps[2].update(pvals, planted, distinct_ids)),
                         ("update, query on every position, ONE id (the hot cell)", lambda r: tps[3].update(pvals, planted, hot_ids))])
        lines += [fmt(label, t) for label, t in res.items()]
        twin = abs(res["update, ordinary batch"][0] - res["update, ordinary batch' (the twin)"][0])
        hot = (res["update, query on every position, ONE id (the hot cell)"][0]
               - res["update, query on every position, 8192 distinct ids"][0])
        lines.append(f"    spread of the twins {twin:.3f} ms; hot - distinct {hot:+.3f} ms")
        del tps

        # ---- (d) top tokens
        res = alternate([(f"top_tokens(m=10, by={by!r}), all {F} rows of plane 0", lambda r, by=by: tp3.top_tokens(m=10, by=by))
                         for by in ("count", "precision", "mean")])
        lines += [fmt(label, t) for label, t in res.items()]
        del tp3
        torch.cuda.empty_cache()

        # ---- (c) the cache loop
        kinds = [("token_profile off", None), ("token_profile off'", None),
                 ("token_profile on (-1, 0, 1; mass)", dict(vocab_size=V, queries=queries, offsets=(-1, 0, 1), mass=True,
                                                            max_bytes=64 << 30))]
        loops = []
        for label, tokens in kinds:
            cache = Cache(0, None, batch_size=ROWS, **({} if tokens is None else dict(tokens=tokens)))
            n = [0]

            def step(rnd, cache=cache, n=n, on=tokens is not None):
                vv, ii, _ = ops.encode_topk(xs[rnd % BATCHES], W_enc, b_enc, b_dec, prep, K)
                cache.add_topk(vv.view(ROWS, S, K), ii.view(ROWS, S, K), N, n[0], "layers.24",
                               **(dict(token_ids=ids[rnd % BATCHES]) if on else {}))
                n[0] += 1
            loops.append((label, step, cache))
        res = alternate([(label, step) for label, step, _ in loops])
        for label, _, cache in loops:
            cache.flush_pending()
            lines.append(fmt(f"cache loop, {label}", res[label]))
        off, twin = res["token_profile off"][0], res["token_profile off'"][0]
        lines.append(f"    spread of the two identical variants {abs(off - twin):.3f} ms; "
                     f"on - off {res['token_profile on (-1, 0, 1; mass)'][0] - off:+.3f} ms")
        del loops, cache, step
        torch.cuda.empty_cache()
    finish(lines, args.out or str(REPO / "profiles" / "token_profile.txt"))


def finish(lines, out):
    print("\n".join(lines), flush=True)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
