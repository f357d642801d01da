#!/usr/bin/env python
"""Generate tests/golden/g14_feature_stats.npz by RUNNING THE REFERENCE'S OWN top-example constructors on CPU.

Like make_golden.py (whose stubs and import helpers this reuses), it runs only where the reference exists.  On
synthetic COO records with well separated pooled values it records what

    window mode  _top_k_pools  (features/constructors.py:47-65; the pooling pool_max_activation_windows runs)
    image mode   pool_max_activations_windows_image  (constructors.py:88-141), with prepare_image_examples replaced by
                 a recorder of its arguments and a datasets.Dataset whose `image` column holds row numbers and whose
                 `id` column repeats ids, so the duplicate-image rule is exercised

select, per feature.  Usage:  python tests/golden/make_golden_stats.py [--out DIR] [--check-reference]
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

W, S_WIN, ROWS_WIN, N_WIN = 16, 5 * 16 + 7, 40, 64        # 5 windows of 16 + a ragged tail of 7 per row
S_IMG, P, ROWS_IMG, N_IMG = 12, 8, 150, 32                  # pool the first 8 of 12 positions
MAX_EXAMPLES = 5


def _import_constructors():
    make_golden._install_stubs()
    sys.path.insert(0, str(make_golden.REF))
    feats = types.ModuleType("sae_auto_interp.features.features")
    feats.FeatureRecord = object
    feats.prepare_examples = lambda tokens, activations: (tokens, activations)
    feats.prepare_image_examples = None                     # replaced per call below
    loader = types.ModuleType("sae_auto_interp.features.loader")
    loader.BufferOutput = object
    pkg = types.ModuleType("sae_auto_interp.features")
    pkg.__path__ = [str(make_golden.REF / "sae_auto_interp" / "features")]
    sys.modules.update({"sae_auto_interp.features": pkg, "sae_auto_interp.features.features": feats,
                        "sae_auto_interp.features.loader": loader})
    spec = importlib.util.spec_from_file_location("sae_auto_interp.features.constructors",
                                                  make_golden.REF / "sae_auto_interp" / "features" / "constructors.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def _records(rng, rows, S, N, fire):
    """COO records (row, pos, feature) ascending, values on a grid of 1/1024 so pooled values separate well."""
    loc, act = [], []
    scale = rng.permutation(rows * S).reshape(rows, S).astype(np.float32)   # distinct magnitudes per (row, pos)
    for r in range(rows):
        for s in range(S):
            for f in np.flatnonzero(rng.random(N) < fire):
                loc.append((r, s, f))
                act.append(np.float32(1.0 + scale[r, s] / 64.0 + f / 4096.0))
    return np.asarray(loc, np.int64), np.asarray(act, np.float32)


def window_fixture(cons, rng):
    loc, act = _records(rng, ROWS_WIN, S_WIN, N_WIN, 0.05)
    nw = S_WIN // W
    tokens = torch.arange(ROWS_WIN * S_WIN, dtype=torch.int64).reshape(ROWS_WIN, S_WIN)   # token = r * S + s
    feats, sel, pooled = [], [], []
    for f in range(N_WIN):
        m = loc[:, 2] == f
        if m.sum() == 0:
            continue
        l, a = torch.from_numpy(loc[m][:, :2]), torch.from_numpy(act[m])
        token_batches, dense = cons._to_dense(tokens, a, l)
        tw, aw = cons._top_k_pools(dense, token_batches, W, MAX_EXAMPLES)
        first = tw[:, 0].numpy()                               # r * S + w * W
        ids = (first // S_WIN) * nw + (first % S_WIN) // W
        row = np.full(MAX_EXAMPLES, -1, np.int64)
        row[:len(ids)] = ids
        pv = np.zeros(MAX_EXAMPLES, np.float32)
        pv[:len(ids)] = aw.max(dim=1).values.numpy()
        feats.append(f), sel.append(row), pooled.append(pv)
    return {"window_S": S_WIN, "window_N": N_WIN, "window_W": W, "window_locations": loc, "window_activations": act,
            "window_features": np.asarray(feats, np.int64), "window_selected": np.stack(sel),
            "window_pooled": np.stack(pooled)}


def image_fixture(cons, rng):
    from datasets import Dataset

    loc, act = _records(rng, ROWS_IMG, S_IMG, N_IMG, 0.5)
    image_ids = (np.arange(ROWS_IMG) % 97).tolist()          # rows r and r + 97 show the same image
    rng.shuffle(image_ids)
    tokens = Dataset.from_dict({"image": list(range(ROWS_IMG)), "id": image_ids})
    processor = types.SimpleNamespace(num_image_tokens=P)
    cfg = types.SimpleNamespace(max_examples=MAX_EXAMPLES)
    record = types.SimpleNamespace()
    captured = {}

    def capture(tok, dense, images, proc):
        captured["images"] = list(images)
        return []

    cons.prepare_image_examples = capture
    feats, sel = [], []
    for f in range(N_IMG):
        m = loc[:, 2] == f
        buf = types.SimpleNamespace(locations=torch.from_numpy(loc[m][:, :2]), activations=torch.from_numpy(act[m]))
        cons.pool_max_activations_windows_image(record, buf, tokens, cfg, processor)
        feats.append(f)
        sel.append(captured["images"])
    return {"image_S": S_IMG, "image_N": N_IMG, "image_P": P, "image_locations": loc, "image_activations": act,
            "image_ids": np.asarray(image_ids, np.int64), "image_features": np.asarray(feats, np.int64),
            "image_selected": np.asarray(sel, np.int64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(HERE))
    ap.add_argument("--check-reference", action="store_true",
                    help="only report whether the reference is present (exit status 0) or not (exit status 3)")
    args = ap.parse_args()
    if args.check_reference:
        sys.exit(0 if make_golden.REF.is_dir() else 3)
    torch.manual_seed(0)
    cons = _import_constructors()
    out = {"max_examples": MAX_EXAMPLES}
    out.update(window_fixture(cons, np.random.default_rng(14)))
    out.update(image_fixture(cons, np.random.default_rng(15)))
    path = Path(args.out) / "g14_feature_stats.npz"
    path.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, {k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
