"""What BatchTopK (msae_batch_kth_f32, msae_list_filter_f32, msae_decode_prefix_f32, Sae(activation=
"batchtopk"), SaeTrainStep) costs at C2 width (d = 4096, N = 131072, T = 8192, k = 32, cap C = 128), modelled on
tools/act_hist_overhead.py.  Writes profiles/batchtopk.txt:

  kernels      ops.batch_kth over the [T, C] list (1 M values), ops.list_filter (scalar theta), and the prefix decode
  encode       ops.encode_topk at width C against width k (and width k again: the twin)
  decode       ops.decode(lengths=) against ops.decode on the SAME filtered list at width C (and the latter again: the twin,
               whose difference from the first is the run-to-run spread every other difference has to be read against) and
               against a plain k = 32 decode.  The one condition: the prefix decode issues a subset of the plain decode's
               loads, so it must not be slower than it by more than that spread.
  backward     the decoder backward (ops.decode_bwd: activations + weights) at width C against width k: the backward still
               runs at width C
  train step   one SaeTrainStep.step of a "batchtopk" Sae against one of a TopK Sae (and the latter again: the twin)

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
    ap.add_argument("--out", default=str(REPO / "profiles" / "batchtopk.txt"))
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
        vk, ik, _ = ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)
        kept, lengths, theta, n_sat = ops.batch_select(vC, iC, K)
    ln = lengths.long()
    lines.append(f"d={d} N={N} T={T} k={K} C={C}: theta {float(theta):.4f}, sum(len) {int(ln.sum())} (T*k = {T * K}), len min / "
                 f"median / max {int(ln.min())} / {int(ln.median())} / {int(ln.max())}, {int(n_sat)} rows saturated")

    def show(res, fmt="    {:52s} {:8.4f} ms"):
        for label, t in res.items():
            lines.append(fmt.format(label, t))

    # ---- the three kernels
    with torch.no_grad():
        res = alternate([("batch_kth [T, C] (zero + 4 passes + pick: 6 launches)", lambda: ops.batch_kth(vC, T * K)),
                         ("list_filter [T, C], scalar theta", lambda: ops.list_filter(vC, iC, theta)),
                         ("batch_select (both, one autograd node)", lambda: ops.batch_select(vC, iC, K)),
                         ("decode, prefix kernel (lengths=)", lambda: ops.decode(iC, kept, W_dec, b_dec, lengths))])
    show(res)

    # ---- encode at width C against width k
    with torch.no_grad():
        res = alternate([(f"encode_topk, width k = {K}", lambda: ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)),
                         (f"encode_topk, width k = {K}'", lambda: ops.encode_topk(x, W_enc, b_enc, b_dec, prep, K)),
                         (f"encode_topk, width C = {C}", lambda: ops.encode_topk(x, W_enc, b_enc, b_dec, prep, C))])
    show(res)
    ek = f"encode_topk, width k = {K}"
    lines.append(f"    spread of the two identical variants {abs(res[ek] - res[ek + chr(39)]):.4f} ms")

    # ---- the decodes on the same filtered list
    with torch.no_grad():
        res = alternate([("decode, filtered list at width C (existing kernel)", lambda: ops.decode(iC, kept, W_dec, b_dec)),
                         ("decode, filtered list at width C (existing kernel)'", lambda: ops.decode(iC, kept, W_dec, b_dec)),
                         ("decode, filtered list at width C, lengths= (prefix)", lambda: ops.decode(iC, kept, W_dec, b_dec, lengths)),
                         (f"decode, plain top-k list at width k = {K}", lambda: ops.decode(ik, vk, W_dec, b_dec))])
        same = torch.equal(ops.decode(iC, kept, W_dec, b_dec), ops.decode(iC, kept, W_dec, b_dec, lengths))
    show(res)
    plain, twin = res["decode, filtered list at width C (existing kernel)"], res["decode, filtered list at width C (existing kernel)'"]
    pre = res["decode, filtered list at width C, lengths= (prefix)"]
    spread = abs(plain - twin)
    lines.append(f"    spread of the two identical variants {spread:.4f} ms; prefix - existing {pre - min(plain, twin):+.4f} ms; "
                 f"outputs bit-identical: {same}")
    lines.append(f"    condition (prefix not slower than the existing decode on the same list by more than the spread): "
                 f"{'met' if pre <= max(plain, twin) + spread else 'NOT met'}")

    # ---- the decoder backward, which still runs at width C
    g = torch.randn(T, d, device=dev)
    with torch.no_grad():
        res = alternate([(f"decode_bwd (acts + W), width C = {C}, filtered list", lambda: ops.decode_bwd(iC, kept, W_dec, g, True, True)),
                         (f"decode_bwd (acts + W), width k = {K}", lambda: ops.decode_bwd(ik, vk, W_dec, g, True, True))], reps=8)
    show(res)
    del g, prep, vC, iC, vk, ik, kept
    torch.cuda.empty_cache()

    # ---- one training step of each
    if not args.no_train:
        def trainer(activation):
            sae = Sae(d, SaeConfig(num_latents=N, k=K, activation=activation, batch_cap=C if activation == "batchtopk" else 0),
                      device=dev)
            with torch.no_grad():
                sae.encoder.weight.copy_(W_enc); sae.encoder.bias.copy_(b_enc); sae.W_dec.copy_(W_dec); sae.b_dec.copy_(b_dec)
            sae.invalidate_prepared()
            return SaeTrainStep(sae, auxk_alpha=0.0)
        xf = x.float()
        ts_b, ts_t = trainer("batchtopk"), trainer("topk")
        res = alternate([("train step, TopK k = 32", lambda: ts_t.step(xf)),
                         ("train step, TopK k = 32'", lambda: ts_t.step(xf)),
                         (f"train step, BatchTopK k = 32, C = {C}", lambda: ts_b.step(xf))], reps=8)
        show(res)
        tk = "train step, TopK k = 32"
        lines.append(f"    spread of the two identical variants {abs(res[tk] - res[tk + chr(39)]):.4f} ms; "
                     f"learned threshold after the run {float(ts_b.sae.threshold):.4f}")
    print("\n".join(lines), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
