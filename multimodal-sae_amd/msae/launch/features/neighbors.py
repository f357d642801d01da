"""python -m msae.launch.features.neighbors --sae_path CKPT [--features FILTER.json] [--k 10] [--matrix decoder]
[--include_self] --out FILE   (reference sae_auto_interp/features/stats.py:76-120, cos + get_neighbors).

The k nearest features of every selected feature by cosine similarity of the decoder (or encoder) rows, as one
`Sae.neighbors` call: a fused f32 GEMM + per-row top-k, so the table of ALL features of a production SAE costs the
outputs and a few MB of scratch instead of N x N cosines.  CKPT is a directory with cfg.json + sae.safetensors.
FILTER.json is a list of feature indices, or {module: [indices]} as the probe launcher writes it (the first module's list
is used); without it every feature is a query.  Writes one safetensors file:
  indices  int32 [M, k]    values  f32 [M, k]    features  int32 [M]
with k, matrix and exclude_self in the metadata.

With `--coact SAVE_DIR` the neighbours come from co-activation in a cache instead (msae/features/coact.py): the
`coact.safetensors` a cache run with --coact wrote under SAVE_DIR (`--module` picks one when there are several; no
checkpoint and no GPU needed), ranked by `--metric` jaccard or count.  The same file layout (free slots: index -1, value 0;
`features` = the query features, or those of FILTER.json), with k, metric, pool and exclude_self in the metadata; without
--out the lists are printed."""
from __future__ import annotations

import argparse
import json

import torch
from safetensors.torch import save_file

from ...features.coact import CoactStats
from ...sae import Sae


def parse_argument(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--sae_path", "--sae-path", type=str, default=None, help="checkpoint directory of the SAE")
    p.add_argument("--coact", type=str, default=None, help="save dir of a cache run with --coact: co-activation neighbours")
    p.add_argument("--module", type=str, default=None, help="with --coact: the module whose statistics to read")
    p.add_argument("--metric", type=str, default="jaccard", choices=["jaccard", "count"], help="with --coact")
    p.add_argument("--features", type=str, default=None, help="JSON file: a list of feature indices or {module: [...]}")
    p.add_argument("--k", type=int, default=10, help="neighbours per feature (<= 64)")
    p.add_argument("--matrix", type=str, default="decoder", choices=["decoder", "encoder"])
    p.add_argument("--include_self", "--include-self", action="store_true",
                   help="do not skip the feature's own index")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--out", type=str, default=None, help="the safetensors file to write")
    args = p.parse_args(argv)
    if args.coact is None and (args.sae_path is None or args.out is None):
        p.error("--sae_path and --out are required (or --coact SAVE_DIR)")
    return args


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


def find_coact(save_dir: str, module=None) -> str:
    """The coact.safetensors under `save_dir` (of `module`, or the only one)."""
    import os

    found = {os.path.relpath(root, save_dir): os.path.join(root, "coact.safetensors")
             for root, _, files in os.walk(save_dir) if "coact.safetensors" in files}
    if module is not None:
        if module not in found:
            raise FileNotFoundError(f"{save_dir}: no coact.safetensors of module {module!r} (found: {sorted(found)})")
        return found[module]
    if len(found) != 1:
        raise FileNotFoundError(f"{save_dir}: expected one coact.safetensors, found {sorted(found)}; pick one with --module")
    return next(iter(found.values()))


def coact_main(args):
    st = CoactStats.load(find_coact(args.coact, args.module), device=args.device if args.device != "cuda:0" or
                         torch.cuda.is_available() else "cpu")
    indices, values = st.neighbors(k=args.k, metric=args.metric, exclude_self=not args.include_self)
    indices, values, feats = indices.cpu(), values.cpu(), st.queries.cpu()
    features = load_features(args.features)
    if features is not None:
        slot = {q: i for i, q in enumerate(feats.tolist())}
        rows = torch.tensor([slot[f] for f in features], dtype=torch.int64)
        indices, values, feats = indices[rows], values[rows], feats[rows]
    if args.out is None:
        for f, ind, val in zip(feats.tolist(), indices.tolist(), values.tolist()):
            print(f, [(i, v) for i, v in zip(ind, val) if i >= 0])
        return
    save_file({"indices": indices.to(torch.int32).contiguous(), "values": values.contiguous(),
               "features": feats.to(torch.int32).contiguous()}, args.out,
              metadata={"k": str(args.k), "metric": args.metric, "pool": st.pool,
                        "exclude_self": str(not args.include_self)})


def main(argv=None):
    args = parse_argument(argv)
    if args.coact is not None:
        return coact_main(args)
    sae = Sae.load_from_disk(args.sae_path, device=args.device, decoder=args.matrix == "decoder")
    features = load_features(args.features)
    values, indices = sae.neighbors(features, k=args.k, matrix=args.matrix, exclude_self=not args.include_self)
    feats = torch.arange(sae.num_latents, dtype=torch.int32) if features is None else torch.tensor(features, dtype=torch.int32)
    save_file({"indices": indices.to(torch.int32).cpu().contiguous(), "values": values.cpu().contiguous(),
               "features": feats},
              args.out, metadata={"k": str(args.k), "matrix": args.matrix, "exclude_self": str(not args.include_self)})


if __name__ == "__main__":
    main()
