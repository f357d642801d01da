#!/usr/bin/env python
"""Generate tests/golden/g18_row_edits.npz by RUNNING THE REFERENCE'S OWN steering hook, one feature at a time.

The reference steers one feature per `generate` at batch 1 (features/steering.py:78-86, hook :102-128).
`msae.features.clamp_features_rows` puts F features into the F rows of one batch; the fixture holds what the F separate
batch-1 runs of the reference produce for ONE hidden state, so row f of the batched hook can be held to run f:

    x [1, S, d] fp16 (S = 5), features [F] (F = 4), clamp, out [F, S, d] fp16 -- out[f] = the hook's output for features[f]
    x_S1 [1, 1, d] fp16, out_S1 [1, 1, d] fp16 -- the S = 1 step (no clamp: the hook edits the prefill only)

The hook is imported from the reference and called as it is (the method does not use `self`) on a layer that returns a
tuple like an HF decoder layer, with g5's shapes (d = 64, N = 1024, k = 8; weights synth.sae_weights(seed 9), regenerated
by the tests).  Data only.  Runs only where the reference exists.
Usage: python tests/golden/make_golden_row_edits.py [--out DIR]"""
from __future__ import annotations

import argparse
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
import make_golden  # noqa: E402
import synth  # noqa: E402

D, N, K, WSEED = 64, 1024, 8, 9
S, CLAMP = 5, 10.0


class _TupleLayer(torch.nn.Module):
    def forward(self, x):
        return (x,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_dir = Path(args.out) if args.out else HERE
    Sae, SaeConfig, _, _ = make_golden._import_reference()
    spec = importlib.util.spec_from_file_location("sae_auto_interp.features.steering",
                                                  make_golden.REF / "sae_auto_interp" / "features" / "steering.py")
    steering = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(steering)

    torch.set_num_threads(1)
    sae = make_golden._make_ref_sae(Sae, SaeConfig, D, N, K, seed=WSEED)
    layer = _TupleLayer()
    x = torch.from_numpy(synth.activations(S, D, 41, n_outlier=1)).to(torch.float16)[None]
    with torch.no_grad():
        lat = sae.pre_acts(x[0])
        order = torch.argsort(lat, dim=1, descending=True, stable=True)
    never = int((lat > 0).sum(0).argmin())
    # token 0's strongest feature, token 2's (k + 1)-th, one no token activates, and feature 0
    features = [int(order[0, 0]), int(order[2, K]), never, 0]
    assert len(set(features)) == len(features)

    def run(feature, inp):
        handles = steering.SteeringController.clamp_features_max(None, sae, feature, layer, k=CLAMP)
        with torch.no_grad():
            y = layer(inp)[0]
        for h in handles:
            h.remove()
        return y.numpy()

    outs = np.stack([run(f, x)[0] for f in features])
    x1 = torch.from_numpy(synth.activations(1, D, 42, n_outlier=1)).to(torch.float16)[None]
    out = {"d": D, "N": N, "k": K, "wseed": WSEED, "clamp": CLAMP, "features": np.array(features, dtype=np.int64),
           "x": x.numpy(), "out": outs, "x_S1": x1.numpy(), "out_S1": run(features[0], x1)}
    assert outs.shape == (len(features), S, D) and outs.dtype == np.float16
    np.savez_compressed(out_dir / "g18_row_edits.npz", **out)
    print("wrote", out_dir / "g18_row_edits.npz", "| features:", features)


if __name__ == "__main__":
    main()
