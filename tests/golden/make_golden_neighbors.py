#!/usr/bin/env python
"""Generate tests/golden/g15_neighbors.npz by RUNNING THE REFERENCE'S OWN features/stats.py on CPU.

The module is loaded by file path (its package's heavy imports are replaced by a stub that provides FeatureRecord), so it
runs only where the reference exists.  Seeded case: a decoder of d = 64, N = 1000, 200 selected features (unsorted), an
unembedding of V = 300.  Recorded (data only: inputs, the reference's values and indices):

    W_dec [N, d], W_U [V, d], features [200]
    cos_head [16, N]            stats.cos for the first 16 selected features (the dense form, small)
    nb_values / nb_indices      torch.topk(stats.cos(...), k + 1): what get_neighbors ranks, plus the value just below
    gn_indices / gn_values      get_neighbors' own dict for k = 10 ([200, 9]: the top 10 with rank 0 dropped)
    gn_layer_features           its per_layer_features list
    lg_indices [200, 10]        stats.logits' token ids (through a tokenizer stub that returns the ids)
    lg_values [200, 11]         torch.topk of the same product, k + 1 values: the separation rule needs them

The reference's decoder.weight is [d, N] (features are columns); the fixture stores its transpose, this project's
layout.  At generation time the recipe asserts that the separation rule of tests/neighbors_ref.compare_with_reference
leaves out fewer than 1 % of the positions.  Usage: python tests/golden/make_golden_neighbors.py [--out DIR]"""
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
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
import make_golden  # noqa: E402
import neighbors_ref  # noqa: E402

D, N, V, M, K = 64, 1000, 300, 200, 10
MODULE = "model.layers.0"


def _import_stats():
    pkg = types.ModuleType("sae_auto_interp.features")
    pkg.__path__ = [str(make_golden.REF / "sae_auto_interp" / "features")]
    pkg.FeatureRecord = object
    top = types.ModuleType("sae_auto_interp")
    top.__path__ = [str(make_golden.REF / "sae_auto_interp")]
    sys.modules.setdefault("sae_auto_interp", top)
    sys.modules["sae_auto_interp.features"] = pkg
    spec = importlib.util.spec_from_file_location("sae_auto_interp.features.stats",
                                                  make_golden.REF / "sae_auto_interp" / "features" / "stats.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


class _IdTokenizer:
    def batch_decode(self, ids):
        return [int(i) for i in ids]


def _submodule(weight_dN):
    """submodule.ae.autoencoder._module.decoder.weight, as get_neighbors reaches it."""
    ns = types.SimpleNamespace
    return ns(ae=ns(autoencoder=ns(_module=ns(decoder=ns(weight=weight_dN)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = Path(args.out) if args.out else HERE
    stats = _import_stats()
    torch.set_num_threads(1)

    rng = np.random.default_rng(1515)
    # a decoder with structure: 40 cluster directions + noise, so neighbours are meaningful, and free row norms
    centers = rng.standard_normal((40, D)).astype(np.float32)
    W = (centers[rng.integers(0, 40, N)] * 0.8 + rng.standard_normal((N, D)).astype(np.float32))
    W = (W * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    W_U = rng.standard_normal((V, D)).astype(np.float32)
    features = rng.permutation(N)[:M].astype(np.int64)          # unsorted, no repeats (a filter list)

    W_dN = torch.from_numpy(np.ascontiguousarray(W.T))          # the reference's layout
    feats = features.tolist()
    with torch.no_grad():
        cos = stats.cos(W_dN, selected_features=feats)
        top = torch.topk(cos, k=K + 1)
        nd, plf = stats.get_neighbors({MODULE: _submodule(W_dN)}, {MODULE: feats}, k=K)
        records = [types.SimpleNamespace(feature=types.SimpleNamespace(feature_index=f), top_logits=None) for f in feats]
        stats.logits(records, torch.from_numpy(W_U), W_dN, k=K, tokenizer=_IdTokenizer())
        lg = torch.topk(torch.matmul(torch.from_numpy(W_U), W_dN[:, feats]), K + 1, dim=0)
    gn_idx = np.array([nd[MODULE][i]["indices"] for i in range(M)], dtype=np.int64)
    gn_val = np.array([nd[MODULE][i]["values"] for i in range(M)], dtype=np.float32)
    lg_idx = np.array([r.top_logits for r in records], dtype=np.int64)
    lg_val = lg.values.T.contiguous().numpy()
    assert np.array_equal(gn_idx, top.indices[:, 1:K].numpy()) and np.array_equal(lg_idx, lg.indices.T[:, :K].numpy())

    # the separation rule must leave (nearly) everything compared
    nb = neighbors_ref.cos_bound(D)
    sep_out = neighbors_ref.compare_with_reference(top.values[:, :K].numpy(), top.indices[:, :K].numpy(),
                                                   top.values.numpy(), top.indices[:, :K].numpy(), nb)[3]
    qn = np.linalg.norm(W[features].astype(np.float64), axis=1)[:, None] * np.linalg.norm(W_U.astype(np.float64), axis=1).max()
    sep_out_lg = neighbors_ref.compare_with_reference(lg_val[:, :K], lg_idx, lg_val, lg_idx, nb * qn)[3]
    assert sep_out < 0.01 * M * K and sep_out_lg < 0.01 * M * K, (sep_out, sep_out_lg)

    np.savez_compressed(out / "g15_neighbors.npz", W_dec=W, W_U=W_U, features=features,
                        cos_head=cos[:16].numpy(), nb_values=top.values.numpy(), nb_indices=top.indices.numpy(),
                        gn_indices=gn_idx, gn_values=gn_val, gn_layer_features=np.array(plf[MODULE], dtype=np.int64),
                        lg_indices=lg_idx, lg_values=lg_val, k=np.int64(K))
    print("wrote", out / "g15_neighbors.npz", "| positions left out by the separation rule:", sep_out, sep_out_lg,
          "of", M * K)


if __name__ == "__main__":
    main()
