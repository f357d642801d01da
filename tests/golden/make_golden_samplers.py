#!/usr/bin/env python
"""Generate tests/golden/g17_samplers.npz by RUNNING THE REFERENCE'S OWN example sampler on CPU.

Like make_golden_stats.py (whose import helpers and stubs this reuses), it runs only where the reference exists.  On the
window records of g14_feature_stats.npz (every feature has fewer than 256 nonzero windows) it builds each feature's examples
the way the reference does -- _to_dense and _top_k_pools(..., max_examples=10000) of features/constructors.py, best window
first -- hands the window ids as the list of examples to features/samplers.py `train(examples, n_train=3, train_type)` and
records the ids it returns for "top", "random" and "quantile".  The fixture holds arrays of ids only.

Usage:  python tests/golden/make_golden_samplers.py [--out DIR] [--check-reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden  # noqa: E402
import make_golden_stats  # noqa: E402

N_TRAIN, N_QUANTILES, MAX_EXAMPLES = 3, 10, 10000


def _import_samplers():
    """features/samplers.py with stubs for what it imports: `..config` (ExperimentConfig) and `.features` (Example,
    FeatureRecord; make_golden_stats installs that module for the constructors)."""
    cfg = types.ModuleType("sae_auto_interp.config")
    cfg.ExperimentConfig = object
    sys.modules["sae_auto_interp.config"] = cfg
    sys.modules["sae_auto_interp.features.features"].Example = object
    spec = importlib.util.spec_from_file_location("sae_auto_interp.features.samplers",
                                                  make_golden.REF / "sae_auto_interp" / "features" / "samplers.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def fixture(cons, samplers):
    g = np.load(HERE / "g14_feature_stats.npz")
    S, W = int(g["window_S"]), int(g["window_W"])
    loc, act = g["window_locations"], g["window_activations"]
    rows = int(loc[:, 0].max()) + 1
    nw = S // W
    tokens = torch.arange(rows * S, dtype=torch.int64).reshape(rows, S)      # token = r * S + s
    feats, out = [], {"top": [], "random": [], "quantile": []}
    width = {"top": N_TRAIN, "random": N_TRAIN, "quantile": N_TRAIN * N_QUANTILES}
    for f in g["window_features"].tolist():
        m = loc[:, 2] == f
        token_batches, dense = cons._to_dense(tokens, torch.from_numpy(act[m]), torch.from_numpy(loc[m][:, :2]))
        tw, _ = cons._top_k_pools(dense, token_batches, W, MAX_EXAMPLES)
        first = tw[:, 0].numpy()                                             # r * S + w * W
        examples = ((first // S) * nw + (first % S) // W).tolist()
        assert N_TRAIN <= len(examples) < 256, (f, len(examples))
        feats.append(f)
        for train_type, w in width.items():
            ids = samplers.train(examples, n_train=N_TRAIN, train_type=train_type, n_quantiles=N_QUANTILES)
            row = np.full(w, -1, np.int64)
            row[:len(ids)] = ids
            out[train_type].append(row)
    return {"features": np.asarray(feats, np.int64), "n_train": N_TRAIN, "n_quantiles": N_QUANTILES,
            **{k: np.stack(v) for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(HERE))
    ap.add_argument("--check-reference", action="store_true",
                    help="only report whether the reference is present (exit status 0) or not (exit status 3)")
    args = ap.parse_args()
    if args.check_reference:
        sys.exit(0 if make_golden.REF.is_dir() else 3)
    torch.manual_seed(0)
    cons = make_golden_stats._import_constructors()
    out = fixture(cons, _import_samplers())
    path = Path(args.out) / "g17_samplers.npz"
    path.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, {k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
