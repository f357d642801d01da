"""What per-row latent edits cost at the bench shape (d = 4096, N = 131072, k = 32) on one MI355X: the
grouped list-edit kernel against the parent's one-table kernel, and the batched steering hook against 16 single-row calls.
Legs, alternated per repetition, medians of --reps:

    kernels, T = 46 080 (16 rows x 2 880 tokens), every token edited, lists of kk = k + 1 entries
        (a) ops.edit_topk       one table of E = 1 for all tokens: msae_edit_topk_i64_f32, the yardstick
        (b) ops.edit_topk_rows  16 groups of one edit, row b -> group b: msae_edit_topk_rows_i64_f32 (wave layout)
        (c) ops.edit_topk_rows  the same with want_mask=True (the differentiable encode's call)
    hook, fp16 hidden states
        (d) prefill  clamp_features_rows on [16, 2880, d]   against (e) 16 x clamp_features_max on [1, 2880, d]
        (f) step     clamp_features_rows on [16, 1, d]      against (g) 16 x clamp_features_max on [1, 1, d]   (HIP graphs)

Wall time per call from device events after a warm-up of every leg.  (b) is checked against (a) run once per table: equal
bits.  The end-to-end gain of a batched `generate` needs the LLM and is not measured here.

    python tools/row_edits_bench.py [--reps 5] [--out profiles/row_edits.txt]
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "multimodal-sae_amd"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

D, N, K = 4096, 131072, 32
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window of the kernel legs")
    ap.add_argument("--only", choices=["all", "kernels"], default="all")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from msae import Sae, SaeConfig, ops
    from msae.features import FeatureEdits, RowEdits, clamp_features_max, clamp_features_rows

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# tools/row_edits_bench.py: d={D} N={N} k={K}, medians of {args.reps} alternated windows, "
             f"{torch.cuda.get_device_name(dev)}", "# T | leg | ms per call | vs yardstick"]
    print("\n".join(lines), flush=True)

    def run(T, legs, inner, base_name):
        for fn in legs.values():                                     # warm-up: every leg once
            fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():                            # alternated
                def window(fn=fn):
                    for _ in range(inner):
                        fn()
                ts[name].append(once(window)[0] / inner)
        base = median(ts[base_name])
        for name in legs:
            m = median(ts[name])
            line = f"{T} | {name} | {m:.4f} | {m / base:.3f}x (min {min(ts[name]):.4f}, max {max(ts[name]):.4f})"
            lines.append(line)
            print(line, flush=True)

    feats = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:B].tolist()
    with torch.no_grad():
        # ---- the kernels alone: canonical lists of k + 1 entries (descending positive values, distinct features; token t
        # of row b holds row b's feature at a varying rank, so the edit drops an entry in most tokens)
        T, kk = B * S, K + 1
        vals = torch.rand(T, kk, generator=g, device=dev).sort(dim=1, descending=True).values + 0.5
        idx = torch.stack([torch.randperm(N, generator=g, device=dev)[:kk] for _ in range(64)]).repeat(T // 64, 1)
        row = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(S)
        fcol = torch.tensor(feats, device=dev)[row.long()]
        tok = torch.arange(T, device=dev)
        idx[tok, tok % kk] = fcol                                    # (a duplicate of the feature elsewhere in a row is harmless)
        one = FeatureEdits(N, set={feats[0]: 3.0}, device=dev)
        rows = RowEdits(N, [dict(set={f: 3.0}) for f in feats], device=dev)
        ref_v, ref_i = torch.empty(T, K, device=dev), torch.empty(T, K, dtype=torch.int64, device=dev)
        for b, f in enumerate(feats):                                # (b) against (a) per table
            fe = FeatureEdits(N, set={f: 3.0}, device=dev)
            v, i = ops.edit_topk(vals[b * S:(b + 1) * S], idx[b * S:(b + 1) * S], fe.feat, fe.val, fe.kind, N, K)
            ref_v[b * S:(b + 1) * S], ref_i[b * S:(b + 1) * S] = v, i
        got_v, got_i, got_e = ops.edit_topk_rows(vals, idx, row, rows, N, K, want_mask=True)
        same = torch.equal(got_i, ref_i) and torch.equal(got_v.view(torch.int32), ref_v.view(torch.int32))
        marked = torch.equal(got_e.bool(), got_i == fcol[:, None])
        line = f"{T} | (b) equals (a) run once per table: {same}; edited mask marks the row's feature: {marked}"
        lines.append(line)
        print(line, flush=True)
        run(T, {"(a) edit_topk, one table E=1 (the one-table kernel)": lambda: ops.edit_topk(vals, idx, one.feat, one.val, one.kind, N, K),
                "(b) edit_topk_rows, 16 groups of one edit": lambda: ops.edit_topk_rows(vals, idx, row, rows, N, K),
                "(c) edit_topk_rows, want_mask=True": lambda: ops.edit_topk_rows(vals, idx, row, rows, N, K, want_mask=True)},
            args.inner, "(a) edit_topk, one table E=1 (the one-table kernel)")
        del vals, idx, ref_v, ref_i, got_v, got_i, got_e
        if args.only == "kernels":
            if args.out:
                Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                Path(args.out).write_text("\n".join(lines) + "\n")
            return

        # ---- the hook
        sae = Sae(D, SaeConfig(num_latents=N, k=K), device=dev).eval().requires_grad_(False)
        for r0 in range(0, N, 16384):
            blk = torch.randn(16384, D, generator=g, device=dev)
            blk = blk / blk.norm(dim=1, keepdim=True)
            sae.encoder.weight[r0:r0 + 16384] = blk
            sae.W_dec[r0:r0 + 16384] = blk
        sae.encoder.bias.copy_(torch.randn(N, generator=g, device=dev) * 0.02)
        sae.b_dec.copy_(torch.randn(D, generator=g, device=dev) * 0.1)
        sae.invalidate_prepared()
        batch, single = torch.nn.Identity(), [torch.nn.Identity() for _ in feats]
        handles = clamp_features_rows(sae, feats, batch, k=3.0)
        for f, layer in zip(feats, single):
            handles += clamp_features_max(sae, f, layer, k=3.0)
        hp = (torch.randn(B, S, D, generator=g, device=dev) + 0.25).to(torch.float16)
        hs = (torch.randn(B, 1, D, generator=g, device=dev) + 0.25).to(torch.float16)

        def singles(h):
            return [layer(h[b:b + 1]) for b, layer in enumerate(single)]

        out_b, out_s = batch(hp), torch.cat(singles(hp))
        line = f"{B * S} | (d) equals (e) row by row: {torch.equal(out_b, out_s)}"
        lines.append(line)
        print(line, flush=True)
        del out_b, out_s
        run(B * S, {"(e) prefill, 16 x clamp_features_max [1, 2880, d]": lambda: singles(hp),
                    "(d) prefill, clamp_features_rows [16, 2880, d]": lambda: batch(hp)}, 1,
            "(e) prefill, 16 x clamp_features_max [1, 2880, d]")
        run(B, {"(g) step, 16 x clamp_features_max [1, 1, d]": lambda: singles(hs),
                "(f) step, clamp_features_rows [16, 1, d]": lambda: batch(hs)}, args.inner,
            "(g) step, 16 x clamp_features_max [1, 1, d]")
        for h in handles:
            h.remove()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
