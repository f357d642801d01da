"""What the JumpReLU selection (msae_jump_filter_f32, msae_jump_bwd_f32, Sae(activation="jump"),
SaeTrainStep(l0_alpha=)) costs at C2 width (d = 4096, N = 131072, T = 8192, k = 32, cap C = 128), modelled on
tools/batchtopk_overhead.py.  Writes profiles/jump.txt:

  filter       ops.jump_filter next to ops.list_filter in table mode on the SAME list and table.  jump_filter does strictly
               more (a third compaction, reach and the slot map): both times are reported, no ratio is asked for.
  backward     ops.jump_bwd (routing copy + per-feature reduction over the band entries) next to the torch.where mask that is
               the whole backward of ops.batch_select, on the same upstream gradient; the share of band entries in the run.
  decode       ops.decode(lengths=reach) next to ops.decode(lengths=len) on the same partitioned list (and the latter again:
               the twin, whose difference from the first is the run-to-run spread every other difference is read against).
  train step   one SaeTrainStep.step of a "jump" Sae next to one of a "batchtopk" Sae, same weights, same batch (and the
               latter again: the twin).

The variants of a group take turns inside ONE process, one timed call of each per round, medians over REPS rounds, device
events.  --out PATH writes there instead; --no-train skips the training steps."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
dev = torch.device("cuda:0")
d, N, T, K, C, REPS = 4096, 131072, 8192, 32, 128, 16


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps=REPS):
    """variants: [(label, fn)] -> {label: median ms}; one timed call of each per round, 3 warm-up rounds."""
    ts = {label: [] for label, _ in variants}
    for rnd in range(3 + reps):
        for label, fn in variants:
            t = once(fn)
            if rnd >= 3:
                ts[label].append(t)
    return {label: statistics.median(v) for label, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "jump.txt"))
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "multimodal-sae_amd"))
    import bench
    from msae import Sae, SaeConfig, ops
    from msae.train import SaeTrainStep

    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    W_enc, b_enc, W_dec, b_dec, x = bench.make_inputs(dev, T, d, N)
    prep = ops.prepare_encoder(W_enc)
    with torch.no_grad():
        vC, iC, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, C)
        # a table around the k-th value of the rows (about k entries a token kept), a band of +-10 % of it
        mid = float(vC[:, K].median())
        theta = mid * (0.8 + 0.4 * torch.rand(N, device=dev))
        eps = 0.2 * mid
        kept, io, ln, reach, src, n_kept, n_sat = ops.jump_filter(vC, iC, theta, eps)
        h = ops.jump_half_band(eps)
        th_f = theta[iC.long()]
        n_band = int(((vC > 0) & ((vC - th_f).abs() < h)).sum())
    lines.append(f"d={d} N={N} T={T} k={K} C={C}: median {K}-th value {mid:.4f}, theta in [0.8, 1.2] of it, eps {eps:.4f}; "
                 f"sum(len) {int(n_kept)} ({int(n_kept) / T:.1f} a token), sum(reach) {int(reach.long().sum())}, band entries "
                 f"{n_band} ({n_band / (T * C):.4f} of T*C), {int(n_sat)} rows saturated")

    def show(res, fmt="    {:58s} {:8.4f} ms"):
        for label, t in res.items():
            lines.append(fmt.format(label, t))

    # ---- the filter next to the table filter
    with torch.no_grad():
        res = alternate([("list_filter [T, C], per-feature table", lambda: ops.list_filter(vC, iC, None, theta)),
                         ("list_filter [T, C], per-feature table'", lambda: ops.list_filter(vC, iC, None, theta)),
                         ("jump_filter [T, C] (3 compactions, reach, src, counters)", lambda: ops.jump_filter(vC, iC, theta, eps))])
    show(res)
    lf = "list_filter [T, C], per-feature table"
    lines.append(f"    spread of the two identical variants {abs(res[lf] - res[lf + chr(39)]):.4f} ms (both include a theta.min() "
                 "for the saturation floor)")

    # ---- the backward next to the mask backward of batch_select
    g = torch.randn(T, C, device=dev)
    s = torch.full((), 1e-4, device=dev)
    zero = torch.zeros((), device=dev)
    with torch.no_grad():
        res = alternate([("batch_select backward: torch.where(kept > 0, g, 0)", lambda: torch.where(kept > 0, g, zero)),
                         ("batch_select backward: torch.where(kept > 0, g, 0)'", lambda: torch.where(kept > 0, g, zero)),
                         ("jump_bwd (zero, rows, scan, rows, reduce: 5 launches)", lambda: ops.jump_bwd(vC, iC, theta, eps, src, ln, reach, g, s))])
        a, b2 = ops.jump_bwd(vC, iC, theta, eps, src, ln, reach, g, s)[1], ops.jump_bwd(vC, iC, theta, eps, src, ln, reach, g, s)[1]
    show(res)
    lines.append(f"    band entries {n_band} of {T * C} ({n_band / (T * C):.4f}); two runs of g_theta bit-identical: {torch.equal(a, b2)}")

    # ---- the reach decode next to the len decode
    with torch.no_grad():
        res = alternate([("decode, lengths = len", lambda: ops.decode(io, kept, W_dec, b_dec, ln)),
                         ("decode, lengths = len'", lambda: ops.decode(io, kept, W_dec, b_dec, ln)),
                         ("decode, lengths = reach", lambda: ops.decode(io, kept, W_dec, b_dec, reach))])
        same = torch.equal(ops.decode(io, kept, W_dec, b_dec, ln), ops.decode(io, kept, W_dec, b_dec, reach))
    show(res)
    dl = "decode, lengths = len"
    lines.append(f"    spread of the two identical variants {abs(res[dl] - res[dl + chr(39)]):.4f} ms; outputs bit-identical: {same}")
    del g, prep, vC, iC, kept, io, src
    torch.cuda.empty_cache()

    # ---- one training step of each
    if not args.no_train:
        def trainer(activation, **kw):
            sae = Sae(d, SaeConfig(num_latents=N, k=K, activation=activation, batch_cap=C, **kw), device=dev)
            with torch.no_grad():
                sae.encoder.weight.copy_(W_enc); sae.encoder.bias.copy_(b_enc); sae.W_dec.copy_(W_dec); sae.b_dec.copy_(b_dec)
            sae.invalidate_prepared()
            return sae
        xf = x.float()
        jump = trainer("jump", jump_bandwidth=eps)
        jump.set_threshold(theta)
        ts_j = SaeTrainStep(jump, auxk_alpha=0.0, l0_alpha=1e-3)
        ts_b = SaeTrainStep(trainer("batchtopk"), auxk_alpha=0.0)
        res = alternate([(f"train step, BatchTopK k = {K}, C = {C}", lambda: ts_b.step(xf)),
                         (f"train step, BatchTopK k = {K}, C = {C}'", lambda: ts_b.step(xf)),
                         (f"train step, JumpReLU C = {C}, l0_alpha = 1e-3", lambda: ts_j.step(xf))], reps=8)
        show(res)
        tb = f"train step, BatchTopK k = {K}, C = {C}"
        last = ts_j.step(xf)
        lines.append(f"    spread of the two identical variants {abs(res[tb] - res[tb + chr(39)]):.4f} ms; L0 of the jump Sae after the "
                     f"run {float(last['l0']):.2f} a token, {int(last['n_saturated'])} rows saturated")
    print("\n".join(lines), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
