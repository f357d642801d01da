"""Reader side of the feature-cache format -- the contract the writer in cache.py must satisfy.

Restates the naming / lookup rule of the reference's `FeatureDataset` and `TensorBuffer`
(sae_auto_interp/features/loader.py:28-90,143-196): the feature axis is cut at
`linspace(0, width, n_splits + 1)`, split i lives in `<raw_dir>/<module>/{start}_{end-1}.safetensors`,
a feature's records are the rows of that file whose third location column equals the feature id, and
consumers get `locations[:, :2]` = (row, position) plus the activations.  CPU-side post-processing,
deliberately not accelerated.

When the cache also wrote per-feature statistics (`<raw_dir>/<module>/feature_stats.safetensors`, msae/features/
stats.py), two questions are answered from them instead of the records: the `min_examples` cut screens features by
their count before any split file is read (the count covers every record of the feature, so a feature it drops has
fewer records than `min_examples` too: the selection is the same), and `top_example_records` returns one feature's
top examples -- what `pool_max_activation_windows` / `pool_max_activations_windows_image` select
(features/constructors.py:28-141) -- from the one split file that holds it.  `sample_example_records` does the same for the
examples the reference's samplers pick (features/samplers.py: "top", "random", "quantile"), from the statistics' uniform sample.
"""
from __future__ import annotations

import os
from typing import Dict, Iterator, List, NamedTuple, Optional, Sequence

import torch
from safetensors.torch import load_file
from torch import Tensor

from .stats import FeatureStats

STATS_FILE = "feature_stats.safetensors"
CACHE_THRESH = 1e-5     # the cache's keep rule (features/cache.py:80-81)


class FeatureRecords(NamedTuple):
    module: str
    feature: int
    locations: Tensor      # [n, 2] int64 (row, position)
    activations: Tensor    # [n] f32


def split_edges(width: int, n_splits: int) -> Tensor:
    return torch.linspace(0, width, steps=n_splits + 1).long()   # loader.py:143-144


def split_path(raw_dir: str, module: str, width: int, n_splits: int, feature: int) -> str:
    """File that holds `feature` (loader.py:164-187: bucketize(right=True) over the edges)."""
    edges = split_edges(width, n_splits)
    b = int(torch.bucketize(torch.tensor([feature]), edges, right=True)[0])
    start, end = int(edges[b - 1]), int(edges[b])
    return f"{raw_dir}/{module}/{start}_{end - 1}.safetensors"


class SplitBuffer:
    """One split file, lazily loaded; iterates / indexes per feature like TensorBuffer."""

    def __init__(self, path: str, module: str, features: Optional[Tensor] = None, min_examples: int = 0,
                 counts: Optional[Tensor] = None):
        self.path, self.module, self.features, self.min_examples = path, module, features, min_examples
        self.counts = counts    # per-feature record counts (feature statistics): features below min_examples skipped
        self.locations = self.activations = None

    def _load(self):
        if self.locations is None:
            data = load_file(self.path)
            self.locations, self.activations = data["locations"], data["activations"]
            if self.features is None:
                self.features = torch.unique(self.locations[:, 2])

    def get(self, feature: int) -> FeatureRecords:
        self._load()
        mask = self.locations[:, 2] == feature
        return FeatureRecords(self.module, int(feature), self.locations[mask][:, :2], self.activations[mask])

    def __iter__(self) -> Iterator[FeatureRecords]:
        if self.features is not None and self.features.numel() == 0:
            return      # every selected feature screened out by its count: the file is not read
        self._load()
        for f in self.features.tolist():
            if self.counts is not None and int(self.counts[f]) < self.min_examples:
                continue
            rec = self.get(f)
            if len(rec.activations) >= self.min_examples:   # loader.py:103-106
                yield rec


class FeatureDataset:
    """All (or selected) features of the cached modules (loader.py:130-196)."""

    def __init__(self, raw_dir: str, width: int, n_splits: int, modules: Optional[List[str]] = None,
                 features: Optional[Dict[str, Tensor]] = None, min_examples: int = 0, use_stats: bool = True):
        """`use_stats`: answer the `min_examples` cut from `<module>/feature_stats.safetensors` where the cache wrote one
        (same selection, fewer records read)."""
        self.buffers: List[SplitBuffer] = []
        edges = split_edges(width, n_splits)
        modules = sorted(os.listdir(raw_dir)) if modules is None else modules
        for module in modules:
            counts = _stats_counts(f"{raw_dir}/{module}", width) if use_stats and min_examples > 0 else None
            if features is None:
                for s, e in zip(edges[:-1].tolist(), edges[1:].tolist()):
                    self.buffers.append(SplitBuffer(f"{raw_dir}/{module}/{s}_{e - 1}.safetensors", module,
                                                    min_examples=min_examples, counts=counts))
            else:
                sel = features[module]
                bucket = torch.bucketize(sel, edges, right=True)
                for b in torch.unique(bucket).tolist():
                    s, e = int(edges[b - 1]), int(edges[b])
                    part = sel[bucket == b]
                    if counts is not None:
                        part = part[counts[part] >= min_examples]
                    self.buffers.append(SplitBuffer(f"{raw_dir}/{module}/{s}_{e - 1}.safetensors", module,
                                                    part, min_examples=min_examples, counts=counts))

    def __len__(self):
        return len(self.buffers)

    def __iter__(self) -> Iterator[FeatureRecords]:
        for buf in self.buffers:
            yield from buf


def _stats_counts(module_dir: str, width: int) -> Optional[Tensor]:
    """Per-feature record counts from the module's statistics file, when there is one that describes these records
    (the cache's keep rule, the same width)."""
    path = os.path.join(module_dir, STATS_FILE)
    if not os.path.exists(path):
        return None
    st = FeatureStats.load(path)
    if st.num_latents != width or st.thresh != CACHE_THRESH:
        return None
    return st.count


class TopExamples(NamedTuple):
    ids: Tensor            # [m] int64: window ids (window mode) or rows (image mode), best first
    values: Tensor         # [m] f32: their pooled values
    tokens: Optional[Tensor]   # window mode: token windows [m, W] (None without `tokens`); image mode: zeros [m, seq_len]
    activations: Tensor    # window mode: activation windows [m, W]; image mode: dense rows [m, seq_len]


def dedup_image_rows(rows: Sequence[int], image_ids: Sequence, max_examples: int) -> List[int]:
    """The image constructor's duplicate-image rule (features/constructors.py:118-135): keep the first row of every image
    id, in rank order, then cut to `max_examples`.  When fewer remain, the list is padded by repeating its first row --
    what constructors.py:131-134 evidently intends; as written it calls len() on the int max_examples and raises."""
    seen, out = set(), []
    for r in rows:
        iid = image_ids[int(r)]
        if iid not in seen:
            seen.add(iid)
            out.append(int(r))
    if out and len(out) < max_examples:
        out += [out[0]] * (max_examples - len(out))
    return out[:max_examples]


def _feature_records(raw_dir: str, st: FeatureStats, module: str, feature: int, n_splits: int) -> FeatureRecords:
    return SplitBuffer(split_path(raw_dir, module, st.num_latents, n_splits, feature), module).get(feature)


def _rebuild_examples(st: FeatureStats, rec: FeatureRecords, ids: Tensor, vals: Tensor, tokens: Optional[Tensor],
                      seq_len: int) -> TopExamples:
    """The examples `ids` (window ids in window mode, rows in image mode) of one feature rebuilt from its records:
    activation windows [m, W] (and token windows from `tokens` [rows, S] if given), or dense rows [m, seq_len] and the image
    constructor's zero tokens."""
    rows_of, pos_of, acts = rec.locations[:, 0], rec.locations[:, 1], rec.activations
    if st.pool == "window":
        W = st.window
        nw = st.windows_per_row if tokens is None else tokens.shape[1] // W
        rows, wins = ids // nw, ids % nw
        act_w = torch.zeros(len(ids), W, dtype=torch.float32)
        for m, (r, w) in enumerate(zip(rows.tolist(), wins.tolist())):
            sel = (rows_of == r) & (pos_of >= w * W) & (pos_of < (w + 1) * W)
            act_w[m, pos_of[sel] - w * W] = acts[sel]
        tok_w = None
        if tokens is not None:
            tok_w = torch.stack([tokens[r, w * W:(w + 1) * W] for r, w in zip(rows.tolist(), wins.tolist())]) \
                if len(ids) else tokens.new_zeros(0, W)
        return TopExamples(ids, vals, tok_w, act_w)
    dense = torch.zeros(len(ids), seq_len, dtype=torch.float32)
    for m, r in enumerate(ids.tolist()):
        sel = rows_of == r
        dense[m, pos_of[sel]] = acts[sel]
    return TopExamples(ids, vals, torch.zeros(len(ids), seq_len), dense)


def top_example_records(raw_dir: str, stats, module: str, feature: int, max_examples: int, n_splits: int,
                        tokens: Optional[Tensor] = None, image_ids: Optional[Sequence] = None,
                        seq_len: int = 8000) -> TopExamples:
    """The top examples of `feature` from its statistics (a FeatureStats or a path to one) and the ONE split file that
    holds its records.

    window mode: the `max_examples` best windows, as pool_max_activation_windows selects them (constructors.py:28-85):
                 activation windows [m, W] rebuilt from the records, token windows from `tokens` [rows, S] if given.
    image mode:  the `max_examples + 50` best rows, deduplicated by `image_ids[row]` when given (the dataset's `id`
                 column, dedup_image_rows) or cut to `max_examples`, as pool_max_activations_windows_image selects them
                 (constructors.py:88-141): dense activation rows [m, seq_len] and the constructor's zero tokens."""
    st = stats if isinstance(stats, FeatureStats) else FeatureStats.load(stats)
    ids, vals = st.top_examples(feature)
    rec = _feature_records(raw_dir, st, module, feature, n_splits)
    if st.pool == "window":
        return _rebuild_examples(st, rec, ids[:max_examples], vals[:max_examples], tokens, seq_len)
    ids, vals = ids[:max_examples + 50], vals[:max_examples + 50]
    if image_ids is not None:
        keep = dedup_image_rows(ids.tolist(), image_ids, max_examples)
        first = {}
        for j, r in enumerate(ids.tolist()):
            first.setdefault(r, j)
        vals = vals[[first[r] for r in keep]] if keep else vals[:0]
        ids = torch.tensor(keep, dtype=torch.int64)
    else:
        ids, vals = ids[:max_examples], vals[:max_examples]
    return _rebuild_examples(st, rec, ids, vals, tokens, seq_len)


def sample_example_records(raw_dir: str, stats, module: str, feature: int, train_type: str, n_train: int,
                           n_splits: int, tokens: Optional[Tensor] = None, image_ids: Optional[Sequence] = None,
                           seq_len: int = 8000, n_quantiles: int = 10, seed: int = 22) -> TopExamples:
    """The examples the reference's sampler would train on (features/samplers.py: `train_type` "top", "random" or
    "quantile"), picked from the statistics by `samplers.stats_examples` and rebuilt, like `top_example_records`, from the
    ONE split file that holds the feature's records.  "random" and "quantile" need statistics with a sample
    (`n_sample > 0`).  Image mode with `image_ids`: the first row of every image id is kept, in list order, and the list is
    not padded."""
    from .samplers import stats_examples

    st = stats if isinstance(stats, FeatureStats) else FeatureStats.load(stats)
    ids, vals = stats_examples(st, feature, train_type, n_train, n_quantiles=n_quantiles, seed=seed)
    if st.pool == "image" and image_ids is not None:
        seen, keep = set(), []
        for j, r in enumerate(ids.tolist()):
            if image_ids[r] not in seen:
                seen.add(image_ids[r])
                keep.append(j)
        ids, vals = ids[keep], vals[keep]
    return _rebuild_examples(st, _feature_records(raw_dir, st, module, feature, n_splits), ids, vals, tokens, seq_len)
