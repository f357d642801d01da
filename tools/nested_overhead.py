"""What the Matryoshka SAE (msae_nested_decode_f32, msae_nested_combine_f32, the grouped decoder backward,
ops.nested_reconstruct, SaeConfig.matryoshka, SaeTrainStep) costs at C2 width (d = 4096, N = 131072, T = 8192, k = 32, prefix
sizes N/16, N/8, N/4, N/2, N), modelled on tools/batchtopk_overhead.py.  Writes profiles/matryoshka.txt:

  forward      the fused nested decode with and without the residual planes E, against the composed form (the group-major
               sort, G masked ops.decode calls and G squared-error passes) and against one plain decode (and that again: the
               twin, whose difference from the first is the run-to-run spread every other difference has to be read against)
  backward     msae_nested_combine_f32 + the two grouped backward kernels against G ops.decode_bwd pairs (one per prefix,
               each rewriting the whole weight gradient) + the G - 1 additions that sum them, and against one pair
  fwd + bwd    ops.nested_reconstruct as one autograd node against the composed expression under ordinary autograd: THE ONE
               CONDITION is that the fused form is not slower than the composed one by more than the spread of the twins
  train step   one SaeTrainStep.step of a Matryoshka Sae (fused node) against a TopK step (and that again: the twin) and
               against the Matryoshka step on the composed expression; each trainer follows its own trajectory, so a
               difference between the TopK and the Matryoshka step is not attributed to a cause
  bench        with --parent: bench.py's headline of this tree and of the parent commit's

The variants of a group take turns inside ONE process, one timed call of each per round, medians over REPS rounds, device
events.  --out PATH writes there instead; --no-train skips the training steps; --parent DIR (a built checkout of the parent
commit) adds the bench.py headline of both trees, fresh processes in turn."""
import argparse
import contextlib
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
dev = torch.device("cuda:0")
d, N, T, K, REPS = 4096, 131072, 8192, 32, 12
BOUNDS = (N // 16, N // 8, N // 4, N // 2, N)
G = len(BOUNDS)


def once(fn, setup=None):
    if setup is not None:
        setup()                                    # outside the timed region
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps=REPS):
    """variants: [(label, fn) or (label, fn, setup)] -> {label: median ms}; one timed call of each per round, 3 warm-up rounds;
    `setup` runs before every call, untimed."""
    ts = {v[0]: [] for v in variants}
    for rnd in range(3 + reps):
        for label, fn, *rest in variants:
            t = once(fn, rest[0] if rest else None)
            if rnd >= 3:
                ts[label].append(t)
    return {label: statistics.median(v) for label, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "matryoshka.txt"))
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its bench.py headline beside this tree's")
    args = ap.parse_args()
    sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "multimodal-sae_amd"))
    import bench
    from msae import Sae, SaeConfig, ops
    from msae.train import SaeTrainStep

    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    W_enc, b_enc, W_dec, b_dec, x = bench.make_inputs(dev, T, d, N)
    xf = x.float()
    prep = ops.prepare_encoder(W_enc)
    with torch.no_grad():
        v, i, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
        grp = torch.bucketize(i.long(), torch.tensor(BOUNDS, device=dev), right=True)
    share = [float((grp == g).float().mean()) for g in range(G)]
    lines.append(f"d={d} N={N} T={T} k={K} bounds={BOUNDS}: share of the listed entries per group " +
                 " / ".join(f"{s:.3f}" for s in share) + f"; E is {G * T * d * 4 / 2 ** 30:.2f} GiB")

    def show(res, fmt="    {:66s} {:8.4f} ms"):
        for label, t in res.items():
            lines.append(fmt.format(label, t))

    def composed_forward():
        out, sq, es = ops.nested_composed(xf, v, i, W_dec, b_dec, BOUNDS)
        return out, sq

    # ---- forward
    with torch.no_grad():
        res = alternate([("decode, plain", lambda: ops.decode(i, v, W_dec, b_dec)),
                         ("decode, plain'", lambda: ops.decode(i, v, W_dec, b_dec)),
                         ("nested_decode, fused, without E", lambda: ops.nested_decode(xf, v, i, W_dec, b_dec, BOUNDS)),
                         ("nested_decode, fused, with E", lambda: ops.nested_decode(xf, v, i, W_dec, b_dec, BOUNDS, want_residuals=True)),
                         (f"composed: sort + {G} masked decodes + {G} squared-error passes", composed_forward)])
        same = torch.equal(ops.nested_decode(xf, v, i, W_dec, b_dec, BOUNDS)[0], composed_forward()[0])
    show(res)
    lines.append(f"    spread of the two identical variants {abs(res['decode, plain'] - res['decode, plain' + chr(39)]):.4f} ms; "
                 f"fused out bit-identical to the composed one: {same}")

    # ---- backward
    with torch.no_grad():
        _, _, E = ops.nested_decode(xf, v, i, W_dec, b_dec, BOUNDS, want_residuals=True)
        E0 = E.clone()
        coef = torch.full((G,), 2.0 / (G * T * d), device=dev)
        g1 = E0[0].contiguous()

        def restore():                                  # the combine works in place: every timed call starts from the residuals
            E.copy_(E0)

        def fused_bwd():
            S = ops.nested_combine_(E, coef, None)
            return ops.nested_decode_bwd(i, v, W_dec, S, BOUNDS, True, True)

        def composed_bwd():
            ga = gw = None
            for g in range(G):
                a, w = ops.decode_bwd(i, torch.where(grp <= g, v, torch.zeros((), device=dev)), W_dec, E0[g], True, True)
                ga, gw = (a, w) if ga is None else (ga.add_(a), gw.add_(w))
            return ga, gw

        res = alternate([("decode_bwd (acts + W), one pair", lambda: ops.decode_bwd(i, v, W_dec, g1, True, True)),
                         ("decode_bwd (acts + W), one pair'", lambda: ops.decode_bwd(i, v, W_dec, g1, True, True)),
                         ("combine + grouped backward (acts + W)", fused_bwd, restore),
                         ("combine alone", lambda: ops.nested_combine_(E, coef, None), restore),
                         (f"{G} decode_bwd pairs + {G - 1} additions of the results", composed_bwd)], reps=8)
    show(res)
    one = "decode_bwd (acts + W), one pair"
    lines.append(f"    spread of the two identical variants {abs(res[one] - res[one + chr(39)]):.4f} ms")
    del E, E0, g1
    torch.cuda.empty_cache()

    # ---- forward + backward through autograd: the one condition
    Wg, bg = W_dec.clone().requires_grad_(), b_dec.clone().requires_grad_()
    w = torch.full((G,), 1.0 / G, device=dev)

    def fwd_bwd(fused):
        vg = v.clone().requires_grad_()
        if fused:
            out, sq_sum = ops.nested_reconstruct(xf, vg, i, Wg, bg, BOUNDS)
        else:
            out, sq = ops.nested_composed(xf, vg, i, Wg, bg, BOUNDS)[:2]
            sq_sum = sq.sum(0)
        (sq_sum * w).sum().backward()
        Wg.grad = bg.grad = None

    res = alternate([("nested_reconstruct fwd + bwd, fused node", lambda: fwd_bwd(True)),
                     ("nested_reconstruct fwd + bwd, fused node'", lambda: fwd_bwd(True)),
                     ("the composed expression fwd + bwd", lambda: fwd_bwd(False))], reps=8)
    show(res)
    f, f2, c = (res[n] for n in res)
    spread = abs(f - f2)
    lines.append(f"    spread of the two identical variants {spread:.4f} ms; composed / fused = {c / min(f, f2):.2f}")
    lines.append(f"    THE ONE CONDITION (fused fwd + bwd not slower than composed by more than the spread): "
                 f"{'met' if max(f, f2) <= c + spread else 'NOT met'}")
    del Wg, bg
    torch.cuda.empty_cache()

    # ---- one training step of each
    if not args.no_train:
        def trainer(matryoshka):
            sae = Sae(d, SaeConfig(num_latents=N, k=K, matryoshka=list(BOUNDS) if matryoshka else []), device=dev)
            with torch.no_grad():
                sae.encoder.weight.copy_(W_enc); sae.encoder.bias.copy_(b_enc); sae.W_dec.copy_(W_dec); sae.b_dec.copy_(b_dec)
            sae.invalidate_prepared()
            return SaeTrainStep(sae, auxk_alpha=0.0)

        real = ops.nested_reconstruct

        def composed(x_, a_, i_, W_, b_, bounds_, lengths_=None):
            out, sq, _ = ops.nested_composed(x_, a_, i_, W_, b_, tuple(bounds_), lengths_)
            return out, sq.sum(0)

        @contextlib.contextmanager
        def composed_node():
            ops.nested_reconstruct = composed
            try:
                yield
            finally:
                ops.nested_reconstruct = real

        def composed_step():
            with composed_node():
                ts_c.step(xf)

        # (every trainer walks its own trajectory on the repeated batch, the TopK one two steps per round: the states the
        # variants are timed in are NOT equal, and a difference between them is not attributed to a cause here)
        ts_t, ts_m, ts_c = trainer(False), trainer(True), trainer(True)
        res = alternate([("train step, TopK k = 32", lambda: ts_t.step(xf)),
                         ("train step, TopK k = 32'", lambda: ts_t.step(xf)),
                         (f"train step, Matryoshka G = {G}, fused node", lambda: ts_m.step(xf)),
                         (f"train step, Matryoshka G = {G}, composed expression", composed_step)], reps=6)
        show(res)
        tk = "train step, TopK k = 32"
        lines.append(f"    spread of the two identical variants {abs(res[tk] - res[tk + chr(39)]):.4f} ms")
    # ---- the benchmark headline of this tree against another tree's (the parent commit's checkout), fresh processes in turn
    if args.parent:
        import json
        import subprocess

        runs = {"this tree": [], "parent": []}
        for _ in range(2):
            for who, root in (("this tree", REPO), ("parent", Path(args.parent).resolve())):
                res = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                                     cwd=str(root), capture_output=True, text=True, timeout=600, check=True)
                runs[who].append(json.loads(res.stdout.strip().splitlines()[-1])["ms_per_step"])
        lines.append("    bench.py --gpus 1 --steps 20 --warmup 5, ms per step, two fresh processes of each in turn:")
        for who, v in runs.items():
            lines.append(f"        {who:10s} " + " / ".join(f"{t:.4f}" for t in v))
        a_, b_ = statistics.mean(runs["this tree"]), statistics.mean(runs["parent"])
        lines.append(f"        this tree / parent = {a_ / b_:.4f} (the benchmarked code is unchanged: inside the box's +-3 %: "
                     f"{abs(a_ / b_ - 1) <= 0.03})")
    print("\n".join(lines), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
