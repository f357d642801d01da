"""What value-dependent latent edits (FeatureEdits(scale=, add=, floor=, cap=), the VALUED instantiation
of csrc/edit_topk.hip, the `cur` pass of ops.pre_acts_features) cost at C2 width (d = 4096, N = 131072, k = 32) for
T = 2880 and 8192 tokens and E = 1 and 50 edited features, modelled on tools/batchtopk_overhead.py.  Writes
profiles/value_edits.txt:

  kernel       the valued edit kernel (SCALE table, with and without the gain output) against the existing kernel (SET
               table) on the same over-fetched list
  cur          ops.pre_acts_features over the E features on its own
  encode       Sae.encode(edits=FeatureEdits(scale=)) against Sae.encode(edits=FeatureEdits(set=)) of the same E (and the
               latter again: the twin, whose difference from the first is the run-to-run spread every other difference has
               to be read against)
  dense route  pre_acts -> torch edit of the E columns -> select_topk: what the valued encode replaces.  The one condition:
               the valued encode is faster than the dense route, in the same session.

The variants of a group take turns inside ONE process, one timed call of each per round, medians over REPS rounds, device
events.  --out PATH writes there instead."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
dev = torch.device("cuda:0")
d, N, K, REPS = 4096, 131072, 32, 12
TOKENS, TABLES = (2880, 8192), (1, 50)


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
    ap.add_argument("--out", default=str(REPO / "profiles" / "value_edits.txt"))
    args = ap.parse_args()
    sys.path.insert(0, str(REPO)); sys.path.insert(0, str(REPO / "multimodal-sae_amd"))
    import bench
    from msae import Sae, SaeConfig, ops
    from msae.features import FeatureEdits

    torch.manual_seed(0)
    lines = [__doc__.strip(), ""]
    W_enc, b_enc, W_dec, b_dec, x_all = bench.make_inputs(dev, max(TOKENS), d, N)
    sae = Sae(d, SaeConfig(num_latents=N, k=K), device=dev)
    with torch.no_grad():
        sae.encoder.weight.copy_(W_enc); sae.encoder.bias.copy_(b_enc); sae.W_dec.copy_(W_dec); sae.b_dec.copy_(b_dec)
    sae.invalidate_prepared()
    sae.eval()
    del W_enc, W_dec
    W, be, bd = sae.encoder.weight, sae.encoder.bias, sae.b_dec
    met = True

    def show(res, fmt="    {:58s} {:9.4f} ms"):
        for label, t in res.items():
            lines.append(fmt.format(label, t))

    for T in TOKENS:
        x = x_all[:T]
        for E in TABLES:
            # the E features: token 0's strongest, then features spread over the dictionary
            with torch.no_grad():
                top0 = sae.encode(x[:1]).top_indices[0, :min(E, 4)].tolist()
            feats = list(dict.fromkeys(top0 + [(7 + 2621 * j) % N for j in range(E)]))[:E]
            scale = FeatureEdits(N, scale={f: 4.0 for f in feats}, device=dev)
            setv = FeatureEdits(N, set={f: 4.0 for f in feats}, device=dev)
            fl = torch.tensor(feats, device=dev)
            lines.append(f"d={d} N={N} k={K} T={T} E={E}")
            with torch.no_grad():
                v, i, _ = ops.encode_topk(x, W, be, bd, sae._prepared_weights(), K + E)
                cur = ops.pre_acts_features(x, W, be, bd, scale.feat)
                res = alternate([("edit kernel, SET table (existing kernel)",
                                  lambda: ops.edit_topk(v, i, setv.feat, setv.val, setv.kind, N, K)),
                                 ("edit kernel, SET table (existing kernel)'",
                                  lambda: ops.edit_topk(v, i, setv.feat, setv.val, setv.kind, N, K)),
                                 ("edit kernel, SCALE table (valued)",
                                  lambda: ops.edit_topk(v, i, scale.feat, scale.val, scale.kind, N, K, cur=cur)),
                                 ("edit kernel, SCALE table (valued, with gain)",
                                  lambda: ops.edit_topk(v, i, scale.feat, scale.val, scale.kind, N, K, cur=cur, want_gain=True)),
                                 ("cur pass: pre_acts_features over the E features",
                                  lambda: ops.pre_acts_features(x, W, be, bd, scale.feat))])
                show(res)
                a = "edit kernel, SET table (existing kernel)"
                lines.append(f"    spread of the two identical variants {abs(res[a] - res[a + chr(39)]):.4f} ms")
                del v, i, cur

                def dense():
                    lat = sae.pre_acts(x)
                    lat[:, fl] = lat[:, fl] * 4.0
                    return sae.select_topk(lat)

                res = alternate([("encode, SET edits", lambda: sae.encode(x, edits=setv)),
                                 ("encode, SET edits'", lambda: sae.encode(x, edits=setv)),
                                 ("encode, SCALE edits (valued)", lambda: sae.encode(x, edits=scale)),
                                 ("dense route: pre_acts -> torch edit -> select_topk", dense)], reps=8)
                show(res)
                got, want = sae.encode(x, edits=scale), dense()
                same = torch.equal(got.top_indices, want[1]) and torch.equal(got.top_acts.view(torch.int32),
                                                                            want[0].view(torch.int32))
                del got, want
            s, s2 = res["encode, SET edits"], res["encode, SET edits'"]
            val, den = res["encode, SCALE edits (valued)"], res["dense route: pre_acts -> torch edit -> select_topk"]
            ok = val < den
            met = met and ok
            lines.append(f"    spread of the two identical variants {abs(s - s2):.4f} ms; valued - SET {val - min(s, s2):+.4f} ms; "
                         f"dense / valued {den / val:.1f}x; valued == dense route bit for bit: {same}")
            lines.append(f"    condition (the valued encode is faster than the dense route): {'met' if ok else 'NOT met'}")
            lines.append("")
            torch.cuda.empty_cache()
    lines.append(f"condition at every shape: {'met' if met else 'NOT met'}")
    print("\n".join(lines), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
