"""python -m msae.launch.features.neighbors --sae_path CKPT [--features FILTER.json] [--k 10] [--matrix decoder]
[--include_self] --out FILE   (reference sae_auto_interp/features/stats.py:76-120, cos + get_neighbors).

The k nearest features of every selected feature by cosine similarity of the decoder (or encoder) rows, as one
`Sae.neighbors` call: a fused f32 GEMM + per-row top-k, so the table of ALL features of a production SAE costs the
outputs and a few MB of scratch instead of N x N cosines.  CKPT is a directory with cfg.json + sae.safetensors.
FILTER.json is a list of feature indices, or {module: [indices]} as the probe launcher writes it (the first module's list
is used); without it every feature is a query.  Writes one safetensors file:
  indices  int32 [M, k]    values  f32 [M, k]    features  int32 [M]
with k, matrix and exclude_self in the metadata."""
from __future__ import annotations

import argparse
import json

import torch
from safetensors.torch import save_file

from ...sae import Sae


def parse_argument(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--sae_path", "--sae-path", type=str, required=True, help="checkpoint directory of the SAE")
    p.add_argument("--features", type=str, default=None, help="JSON file: a list of feature indices or {module: [...]}")
    p.add_argument("--k", type=int, default=10, help="neighbours per feature (<= 64)")
    p.add_argument("--matrix", type=str, default="decoder", choices=["decoder", "encoder"])
    p.add_argument("--include_self", "--include-self", action="store_true",
                   help="do not skip the feature's own index")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--out", type=str, required=True, help="the safetensors file to write")
    return p.parse_args(argv)


def load_features(path):
    if path is None:
        return None
    with open(path) as f:
        obj = json.load(f)
    if isinstance(obj, dict):
        if not obj:
            raise ValueError(f"{path}: empty filter")
        obj = next(iter(obj.values()))
    return [int(i) for i in obj]


def main(argv=None):
    args = parse_argument(argv)
    sae = Sae.load_from_disk(args.sae_path, device=args.device, decoder=args.matrix == "decoder")
    features = load_features(args.features)
    values, indices = sae.neighbors(features, k=args.k, matrix=args.matrix, exclude_self=not args.include_self)
    feats = torch.arange(sae.num_latents, dtype=torch.int32) if features is None else torch.tensor(features, dtype=torch.int32)
    save_file({"indices": indices.to(torch.int32).cpu().contiguous(), "values": values.cpu().contiguous(),
               "features": feats},
              args.out, metadata={"k": str(args.k), "matrix": args.matrix, "exclude_self": str(not args.include_self)})


if __name__ == "__main__":
    main()
