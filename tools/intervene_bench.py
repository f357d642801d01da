"""What an error-preserving intervention costs at the bench width (d = 4096, N = 131072) on one MI355X:
the fused difference decode against the same quantity composed from the ops that existed before it, and the steering
prefill three ways.  One process, legs alternated per repetition, medians of --reps; fp16 hidden states.

    per (k, E) in (32 | 256) x (1 | 50), T = 2880 tokens, one FeatureEdits of E clamps
        op        (a) composed: ops.decode(edited) - ops.decode(plain, made contiguous), + x, cast     the yardstick
                  (b) ops.delta_decode on the over-fetched list's [:, :k] view
        prefill   (c) composed: encode k + E, edit_topk, (a)
                  (d) Sae.intervene
                  (e) sae_reconstruct(out_dtype=fp16): today's hook body (it REPLACES the layer output; another quantity)
    the same prefill legs for 16 x 2880 tokens with a RowEdits of 16 groups of E clamps (ops.edit_topk_rows)
    S = 1 steps: the preserve_error hook (returns its input: Python only) against today's hook (captured graph), B = 1 and 16

(b) is checked against (a) within the bound of tests/intervene_ref.py's kind (here: 2^-9 relative to the largest magnitude, an
fp16 sanity bar, not the test's).  The end-to-end effect on a LLaVA-NeXT generation needs the checkpoint: not measured.

    python tools/intervene_bench.py [--reps 7] [--out profiles/intervene.txt]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "multimodal-sae_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

D, N = 4096, 131072
B, S = 16, 2880


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window of the T = 2880 legs")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from msae import Sae, SaeConfig, ops
    from msae.features import FeatureEdits, RowEdits, clamp_features_max, clamp_features_rows, sae_reconstruct

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/intervene_bench.py: d={D} N={N}, fp16 hidden states, medians of {args.reps} alternated windows, "
             f"{torch.cuda.get_device_name(dev)}", "# k E T | leg | ms per call | vs yardstick (min, max of the windows)"]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    def run(tag, legs, inner, base_name):
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                def window(fn=fn):
                    for _ in range(inner):
                        fn()
                ts[name].append(once(window)[0] / inner)
        base = median(ts[base_name])
        for name in legs:
            m = median(ts[name])
            emit(f"{tag} | {name} | {m:.4f} | {m / base:.3f}x (min {min(ts[name]):.4f}, max {max(ts[name]):.4f})")

    with torch.no_grad():
        sae = Sae(D, SaeConfig(num_latents=N, k=32), device=dev).eval().requires_grad_(False)
        for r0 in range(0, N, 16384):
            blk = torch.randn(16384, D, generator=g, device=dev)
            blk = blk / blk.norm(dim=1, keepdim=True)
            sae.encoder.weight[r0:r0 + 16384] = blk
            sae.W_dec[r0:r0 + 16384] = blk
        sae.encoder.bias.copy_(torch.randn(N, generator=g, device=dev) * 0.02)
        sae.b_dec.copy_(torch.randn(D, generator=g, device=dev) * 0.1)
        sae.invalidate_prepared()
        W = sae.W_dec
        hp1 = (torch.randn(1, S, D, generator=g, device=dev) + 0.25).to(torch.float16)
        hpB = (torch.randn(B, S, D, generator=g, device=dev) + 0.25).to(torch.float16)
        feats = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:B * 50].tolist()

        def composed_op(x, acts, idx, q_acts, q_idx, k):
            delta = ops.decode(q_idx, q_acts, W, None) - ops.decode(idx[:, :k].contiguous(), acts[:, :k].contiguous(), W, None)
            return (x.float() + delta).to(x.dtype)

        for k in (32, 256):
            sae.cfg.k = k
            for E in (1, 50):
                fe = FeatureEdits(N, set={f: 6.0 for f in feats[:E]}, device=dev)
                x = hp1.reshape(-1, D)
                acts, idx, _ = ops.encode_topk(x, sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights(), k + E)
                q_acts, q_idx = ops.edit_topk(acts, idx, fe.feat, fe.val, fe.kind, N, k)
                a = composed_op(x, acts, idx, q_acts, q_idx, k)
                b = ops.delta_decode(x, acts[:, :k], idx[:, :k], q_acts, q_idx, W)
                dev_ab = (a.float() - b.float()).abs().max().item()
                moved = (b != x).any(-1).float().mean().item()
                emit(f"{k} {E} {S} | (b) against (a): max |difference| {dev_ab:.3e} of max |x| {x.float().abs().max().item():.3e} "
                     f"(within 2^-9 relative: {dev_ab <= 2.0 ** -9 * b.float().abs().max().item()}); tokens moved {moved:.3f}")
                run(f"{k} {E} {S}", {"(a) op, composed: 2 x ops.decode + add": lambda: composed_op(x, acts, idx, q_acts, q_idx, k),
                                     "(b) op, ops.delta_decode": lambda: ops.delta_decode(x, acts[:, :k], idx[:, :k], q_acts, q_idx, W)},
                    args.inner, "(a) op, composed: 2 x ops.decode + add")

                def composed_prefill(h, k=k, E=E, fe=fe):
                    xf = h.reshape(-1, D)
                    av, ai, _ = ops.encode_topk(xf, sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights(), k + E)
                    qv, qi = ops.edit_topk(av, ai, fe.feat, fe.val, fe.kind, N, k)
                    return composed_op(xf, av, ai, qv, qi, k).view(h.shape)

                run(f"{k} {E} {S}", {"(c) prefill, composed from the earlier ops": lambda: composed_prefill(hp1),
                                     "(d) prefill, Sae.intervene": lambda: sae.intervene(hp1, fe),
                                     "(e) prefill, today's reconstruct hook body": lambda: sae_reconstruct(sae, hp1, edits=fe, out_dtype=torch.float16)},
                    args.inner, "(c) prefill, composed from the earlier ops")

                rows = RowEdits(N, [dict(set={f: 6.0 for f in feats[b * 50:b * 50 + E]}) for b in range(B)], device=dev)
                row = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(S)

                def composed_rows(h, k=k, E=E, rows=rows):
                    xf = h.reshape(-1, D)
                    av, ai, _ = ops.encode_topk(xf, sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights(), k + E)
                    qv, qi = ops.edit_topk_rows(av, ai, row, rows, N, k)
                    return composed_op(xf, av, ai, qv, qi, k).view(h.shape)

                run(f"{k} {E} {B * S}", {"(c) rows prefill, composed from the earlier ops": lambda: composed_rows(hpB),
                                         "(d) rows prefill, Sae.intervene": lambda: sae.intervene(hpB, rows),
                                         "(e) rows prefill, today's reconstruct hook body": lambda: sae_reconstruct(sae, hpB, edits=rows, out_dtype=torch.float16)},
                    1, "(c) rows prefill, composed from the earlier ops")
                del acts, idx, q_acts, q_idx, a, b
        # ---- the S = 1 step
        sae.cfg.k = 32
        for nb in (1, B):
            hs = (torch.randn(nb, 1, D, generator=g, device=dev) + 0.25).to(torch.float16)
            keep, today = torch.nn.Identity(), torch.nn.Identity()
            if nb == 1:
                handles = clamp_features_max(sae, feats[0], keep, k=6.0, preserve_error=True) + clamp_features_max(sae, feats[0], today, k=6.0)
            else:
                handles = clamp_features_rows(sae, feats[:nb], keep, k=6.0, preserve_error=True) + clamp_features_rows(sae, feats[:nb], today, k=6.0)
            run(f"32 1 {nb}", {"(g) step, today's hook (captured graph)": lambda: today(hs),
                               "(f) step, preserve_error hook (returns its input)": lambda: keep(hs)}, 50,
                "(g) step, today's hook (captured graph)")
            for h in handles:
                h.remove()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
