"""Which of a feature's examples an explainer or scorer is shown -- the drop-in for the reference's
sae_auto_interp/features/samplers.py (`train_type` "top", "random" or "quantile"; config.py:33, n_quantiles = 10).

`train` and `split_quantiles` work on any list of examples ordered best first, as `record.examples` is, and draw with Python's
`random` module seeded the way the reference seeds it: the same list gives the same picks.  `stats_examples` feeds them from
the statistics the cache wrote (msae/features/stats.py) instead of a dense per-feature tensor: "top" reads the top table;
"random" and "quantile" read the uniform sample table, whose rank quantiles estimate those of all the feature's nonzero
pooled segments (and equal them when the feature has no more than `n_sample` of them).  The reference's
`split_activation_quantiles` has no counterpart: nothing calls it, and it raises on its own documented input order.
"""
from __future__ import annotations

import random
from typing import List, Sequence, Tuple

import torch
from torch import Tensor

TRAIN_TYPES = ("top", "random", "quantile")


def split_quantiles(examples: Sequence, n_quantiles: int, n_samples: int, seed: int = 22) -> List:
    """`n_quantiles` consecutive strata of `len(examples) // n_quantiles` examples each (the remainder at the tail is never
    drawn from); up to `n_samples` drawn from every stratum, strata in order."""
    random.seed(seed)
    size = len(examples) // n_quantiles
    picked: List = []
    for q in range(n_quantiles):
        stratum = examples[q * size:(q + 1) * size]
        picked.extend(random.sample(stratum, min(len(stratum), n_samples)))
    return picked


def train(examples: Sequence, n_train: int, train_type: str, seed: int = 22, n_quantiles: int = 10) -> List:
    """The training examples of one feature: the first `n_train` ("top"), `n_train` drawn uniformly ("random"; fewer examples
    than that raise, as random.sample does), or `n_train` per stratum ("quantile")."""
    if train_type == "top":
        return examples[:n_train]
    if train_type == "random":
        random.seed(seed)
        return random.sample(examples, n_train)
    if train_type == "quantile":
        return split_quantiles(examples, n_quantiles, n_train)
    raise ValueError(f"Invalid train_type: {train_type}")


def sample(record, cfg) -> None:
    """Sets `record.train` from `record.examples` by the experiment configuration (n_examples_train, train_type,
    n_quantiles)."""
    record.train = train(record.examples, n_train=cfg.n_examples_train, train_type=cfg.train_type,
                         n_quantiles=cfg.n_quantiles)


def stats_examples(stats, feature: int, train_type: str, n_train: int, n_quantiles: int = 10,
                   seed: int = 22) -> Tuple[Tensor, Tensor]:
    """(ids int64, pooled values f32) of the examples `train` picks for `feature`, from a FeatureStats.  "top": the first
    `n_train` of the top table.  "random" / "quantile": `train` over the sample table put in the order `record.examples`
    has in the reference (value descending, then id ascending)."""
    if train_type not in TRAIN_TYPES:
        raise ValueError(f"Invalid train_type: {train_type}")
    if train_type == "top":
        ids, vals = stats.top_examples(feature)
        return ids[:n_train], vals[:n_train]
    ids, vals = stats.sample_examples(feature)
    by_id = torch.argsort(ids, stable=True)
    order = by_id[torch.argsort(vals[by_id], descending=True, stable=True)]
    picked = train(order.tolist(), n_train, train_type, seed=seed, n_quantiles=n_quantiles)
    picked = torch.tensor(picked, dtype=torch.int64)
    return ids[picked], vals[picked]
