"""What set-valued latent edits cost at the bench shape (d = 4096, N = 131072, k = 32, bf16 x) on one MI355X: the over-fetching
encode + list edit (Sae.encode(x, edits=...)) against the unedited encode, the scalar in-kernel edit
and the dense seam pre_acts -> edit -> select_topk.  Legs, alternated per repetition, medians of --reps:

    (a) encode(k) unedited                      (b) encode(k, zero_feature=f): the scalar in-kernel edit
    (c) encode(edits) for E in 1, 8, 50, 100    (d) the dense seam for E = 50 on --dense-tokens tokens (4 GiB of latents per 8192)
    T = 8192, and T = 1 and 64 for E in 1, 8

Wall time per call from device events after a warm-up of every leg.  The edit kernel alone is read from a separate
`rocprofv3 --kernel-trace --stats` run of `--only edits` (kernel name edit_topk_kernel).  Outputs of (c) are compared with
the dense seam's where it is run.

    python tools/feature_edits_bench.py [--reps 3] [--out profiles/feature_edits.txt]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window at T = 8192 (more at small T)")
    ap.add_argument("--dense-tokens", type=int, default=8192)
    ap.add_argument("--only", choices=["all", "edits"], default="all", help="edits: leg (c) alone (for the kernel trace)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from msae import Sae, SaeConfig
    from msae.features import FeatureEdits

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    sae = Sae(D, SaeConfig(num_latents=N, k=K), device=dev, decoder=False).eval().requires_grad_(False)
    with torch.no_grad():
        for r0 in range(0, N, 16384):
            blk = torch.randn(16384, D, generator=g, device=dev)
            sae.encoder.weight[r0:r0 + 16384] = blk / blk.norm(dim=1, keepdim=True)
        sae.encoder.bias.copy_(torch.randn(N, generator=g, device=dev) * 0.02)
        sae.b_dec.copy_(torch.randn(D, generator=g, device=dev) * 0.1)
    sae.invalidate_prepared()
    feats = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:100].tolist()

    def edits(E):          # half clamps, half ablations
        return FeatureEdits(N, set={f: 3.0 for f in feats[:E:2]}, zero=feats[1:E:2] or None, device=dev)

    lines = [f"# tools/feature_edits_bench.py: d={D} N={N} k={K}, x bf16, medians of {args.reps} alternated windows, "
             f"{torch.cuda.get_device_name(dev)}", "# T | leg | ms per call | vs (a)"]
    print("\n".join(lines), flush=True)

    def run(T, legs, inner):
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
        base = median(ts["(a) encode"]) if "(a) encode" in ts else None
        for name in legs:
            m = median(ts[name])
            line = f"{T} | {name} | {m:.3f} | " + (f"{m / base:.3f}x, +{m - base:.3f} ms" if base else "-")
            lines.append(line)
            print(line, flush=True)

    with torch.no_grad():
        for T, Es, inner in ((8192, (1, 8, 50, 100), args.inner), (64, (1, 8), 20 * args.inner), (1, (1, 8), 20 * args.inner)):
            x = (torch.randn(T, D, generator=g, device=dev) + 0.25).to(torch.bfloat16)
            legs = {}
            if args.only == "all":
                legs["(a) encode"] = lambda x=x: sae.encode(x)
                legs["(b) encode, scalar zero_feature"] = lambda x=x: sae.encode(x, zero_feature=feats[1])
            for E in Es:
                legs[f"(c) encode(edits), E={E}"] = lambda x=x, ed=edits(E): sae.encode(x, edits=ed)
            run(T, legs, inner)
            if T == 8192 and args.only == "all":
                Td = min(args.dense_tokens, T)
                xd, ed = x[:Td], edits(50)
                idx = ed.feat.long()
                setv = torch.where(ed.kind == 0, ed.val, torch.zeros_like(ed.val))

                def dense(xd=xd):
                    lat = sae.pre_acts(xd)
                    lat[:, idx] = setv
                    return sae.select_topk(lat)

                ref = dense()
                got = sae.encode(xd, edits=ed)
                same = torch.equal(ref.top_indices, got.top_indices) and torch.equal(ref.top_acts, got.top_acts)
                t = median([once(dense)[0] for _ in range(args.reps)])
                line = (f"{Td} | (d) dense seam pre_acts -> edit -> select_topk, E=50 | {t:.3f} | outputs equal to (c): {same}; "
                        f"latents {Td * N * 4 / 2**30:.1f} GiB")
                lines.append(line)
                print(line, flush=True)
                del ref, got
                torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
