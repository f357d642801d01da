"""Co-activation counters of a list of query features, built while the cache runs, and neighbour lists from them.

`Sae.neighbors` / `get_neighbors` (msae/features/stats.py) rank neighbours by decoder geometry.  `CoactStats` answers the
other question -- which features FIRE together -- from the top-k pairs the cache loop already holds on the device
(msae_coact_update, include/msae.h), next to `FeatureStats`:

    pool="token"   every position is a segment
    pool="window"  windows of `window` positions (the ragged tail of a row is not pooled)
    pool="image"   the first `pool_len` positions of a row

A feature is active in a segment that holds a kept entry of it (|v| > thresh, the cache's rule, without the cache's
feature filter).  For F query features and width N:

    counts [F, N] int32   counts[i, g] = segments in which queries[i] and g are both active
    seg_count [N] int64   segments in which g is active
    n_segments            segments seen, empty ones included (a Python int, from the shapes alone)

All of it is exact integer arithmetic: the state does not depend on how rows are cut into calls or ranks, or on the
order of the calls.  `neighbors` ranks the candidates of a query (counts > 0) by Jaccard similarity or by the count,
(score descending, feature ascending)."""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from .. import _hip, ops
from . import _pooled
from ._pooled import POOL_MODES, _write_safetensors

METRICS = {"jaccard": 0, "count": 1}
FORMAT = "msae.coact.v1"
MAX_QUERIES, MAX_NEIGHBORS = 16384, 64


@torch.library.custom_op("msae::coact_update", mutates_args=("counts", "seg_count"))
def coact_update(top_acts: Tensor, top_indices: Tensor, thresh: float, mode: int, pool_len: int, window: int,
                 slot_of: Tensor, counts: Tensor, seg_count: Tensor) -> None:
    """One batch of `[B, S, k]` top-k pairs into the counters (in place, stream-ordered, no host read)."""
    F, N = counts.shape
    assert slot_of.shape == (N,) and slot_of.dtype == torch.int32 and seg_count.shape == (N,)
    assert counts.dtype == torch.int32 and seg_count.dtype == torch.int64
    assert counts.is_contiguous() and seg_count.is_contiguous() and slot_of.is_contiguous()
    dev, lib, vals, idx, Tk = _pooled.topk_inputs(top_acts, top_indices, slot_of, counts, seg_count)
    with torch.cuda.device(dev):
        ws = ops._workspace(dev, lib.msae_coact_ws_bytes(*Tk, N))
        _pooled.pooled_update(lib, "msae_coact_update", vals, idx, thresh, N, mode, pool_len, window,
                              (_hip.ptr(slot_of), F, _hip.ptr(counts), _hip.ptr(seg_count)), ws)


@coact_update.register_fake
def _(top_acts, top_indices, thresh, mode, pool_len, window, slot_of, counts, seg_count):
    return None


@torch.library.custom_op("msae::coact_topk", mutates_args=())
def coact_topk(counts: Tensor, seg_count: Tensor, queries: Tensor, m: int, metric: int, exclude_self: bool,
               wide: bool) -> Tuple[Tensor, Tensor]:
    """(values [F, m] f32, indices [F, m] int64 if `wide` else int32) of the best m candidates per query row."""
    dev = _hip.require_device(counts, seg_count, queries)
    lib = _hip.load()
    F, N = counts.shape
    assert counts.dtype == torch.int32 and seg_count.dtype == torch.int64 and queries.dtype == torch.int32
    assert counts.is_contiguous() and seg_count.shape == (N,) and queries.shape == (F,)
    val = torch.empty(F, m, dtype=torch.float32, device=dev)
    ind = torch.empty(F, m, dtype=torch.int64 if wide else torch.int32, device=dev)
    fn, name = (lib.msae_coact_topk_i64, "msae_coact_topk_i64") if wide else (lib.msae_coact_topk, "msae_coact_topk")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(counts), _hip.ptr(seg_count.contiguous()), _hip.ptr(queries.contiguous()), F, N, m, metric,
                      int(exclude_self), _hip.ptr(val), _hip.ptr(ind), _hip.stream_of(counts)), name)
    return val, ind


@coact_topk.register_fake
def _(counts, seg_count, queries, m, metric, exclude_self, wide):
    F = counts.shape[0]
    return (counts.new_empty((F, m), dtype=torch.float32),
            counts.new_empty((F, m), dtype=torch.int64 if wide else torch.int32))


def _query_list(queries, num_latents: int) -> list:
    if isinstance(queries, Tensor):
        queries = queries.detach().cpu().reshape(-1).tolist()
    q = [int(x) for x in queries]
    if not 1 <= len(q) <= MAX_QUERIES:
        raise ValueError(f"the number of query features must lie in [1, {MAX_QUERIES}], got {len(q)}")
    if len(set(q)) != len(q):
        raise ValueError("query features must be distinct")
    if min(q) < 0 or max(q) >= num_latents:
        raise ValueError(f"query features must lie in [0, {num_latents})")
    return q


class CoactStats:
    """Co-activation counters of `queries` (slot i = queries[i], order kept) against all `num_latents` features; see the
    module docstring.  The counters live on `device`; `update` and the kernel path of `neighbors` need a HIP device,
    `merge`, `row`, `save` and reading a loaded file do not."""

    def __init__(self, num_latents: int, queries, pool: str = "token", pool_len: int = 576, window: int = 64,
                 thresh: float = 1e-5, device=None, max_bytes: int = 8 << 30):
        _pooled.check_pool(pool)
        _pooled.check_pool_args(num_latents, pool, pool_len, window)
        q = _query_list(queries, num_latents)
        if len(q) * num_latents * 4 > max_bytes:
            raise ValueError(f"{len(q)} queries x {num_latents} features need {len(q) * num_latents * 4} bytes of counters, "
                             f"more than max_bytes = {max_bytes}")
        self.num_latents, self.pool = num_latents, pool
        self.pool_len, self.window, self.thresh = int(pool_len), int(window), float(thresh)
        self.n_segments = 0
        dev = torch.device("cpu") if device is None else torch.device(device)
        self.queries = torch.tensor(q, dtype=torch.int64, device=dev)
        self.counts = torch.zeros(len(q), num_latents, dtype=torch.int32, device=dev)
        self.seg_count = torch.zeros(num_latents, dtype=torch.int64, device=dev)
        self._slot_of: Optional[Tensor] = None
        self._queries32: Optional[Tensor] = None

    @property
    def device(self) -> torch.device:
        return self.counts.device

    @property
    def num_queries(self) -> int:
        return self.counts.shape[0]

    def _kind(self):
        return (self.num_latents, *_pooled.pool_kind(self.pool, self.pool_len, self.window), self.thresh)

    def _device_lists(self) -> Tuple[Tensor, Tensor]:
        if self._slot_of is None or self._slot_of.device != self.device:
            slot_of = torch.full((self.num_latents,), -1, dtype=torch.int32, device=self.device)
            slot_of[self.queries] = torch.arange(self.num_queries, dtype=torch.int32, device=self.device)
            self._slot_of, self._queries32 = slot_of, self.queries.to(torch.int32)
        return self._slot_of, self._queries32

    def update(self, top_acts: Tensor, top_indices: Tensor) -> None:
        """Add one batch of `[B, S, k]` top-k pairs (complete rows only).  Every limit is checked on the host, from the
        shapes alone, before any device work; nothing is read back."""
        B, S, k = _pooled.topk_shape(top_acts, top_indices)
        _pooled.check_call_limits(S, k)
        total = _pooled.total_segments(self.n_segments, _pooled.segments_of(self.pool, B, S, self.window))
        _hip.require_device(top_acts, top_indices, self.counts)
        if B * S == 0:
            return
        slot_of, _ = self._device_lists()
        for rows in _pooled.row_chunks(B, S):
            torch.ops.msae.coact_update(top_acts[rows], top_indices[rows], self.thresh, POOL_MODES[self.pool], self.pool_len,
                                        self.window, slot_of, self.counts, self.seg_count)
        self.n_segments = total

    def merge(self, other: "CoactStats") -> "CoactStats":
        """self += other (another rank's counters of the same kind and query list), on self's device, in plain torch."""
        if self._kind() != other._kind():
            raise ValueError(f"cannot merge co-activation statistics of different kinds: {self._kind()} vs {other._kind()}")
        if self.queries.cpu().tolist() != other.queries.cpu().tolist():
            raise ValueError("cannot merge co-activation statistics of different query lists")
        total = _pooled.total_segments(self.n_segments, other.n_segments)
        self.counts += other.counts.to(self.device)
        self.seg_count += other.seg_count.to(self.device)
        self.n_segments = total
        return self

    def row(self, feature: int) -> Tensor:
        """The counter row [N] of query `feature`."""
        hit = (self.queries == int(feature)).nonzero()
        if hit.numel() == 0:
            raise KeyError(f"feature {feature} is not a query of these statistics")
        return self.counts[int(hit[0, 0])]

    def neighbors(self, k: int = 10, metric: str = "jaccard", exclude_self: bool = True) -> Tuple[Tensor, Tensor]:
        """(indices [F, k] int64, values [F, k] f32): per query the k best co-firing features, (score descending, feature
        ascending); a row with fewer candidates ends in free slots (-1, 0.0).  The kernel on a HIP device, the same bits
        from plain torch on the CPU."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
        if not 1 <= k <= MAX_NEIGHBORS:
            raise ValueError(f"k must lie in [1, {MAX_NEIGHBORS}], got {k}")
        if self.counts.is_cuda:
            _, q32 = self._device_lists()
            val, ind = torch.ops.msae.coact_topk(self.counts, self.seg_count, q32, k, METRICS[metric], bool(exclude_self),
                                                 True)
            return ind, val
        return _neighbors_host(self.counts, self.seg_count, self.queries, k, metric, exclude_self)

    # ---- file ----------------------------------------------------------------------------------------------------
    def metadata(self) -> dict:
        return {"format": FORMAT, "pool": self.pool, "pool_len": str(self.pool_len), "window": str(self.window),
                "thresh": repr(self.thresh), "num_latents": str(self.num_latents), "n_segments": str(self.n_segments)}

    def save(self, path: str) -> None:
        """queries, seg_count and the NONZERO counters: pair_key int64 = slot * N + g (ascending), pair_count int32."""
        flat = self.counts.reshape(-1)
        key = flat.nonzero().reshape(-1)
        tensors = {"queries": self.queries, "seg_count": self.seg_count, "pair_key": key, "pair_count": flat[key]}
        _write_safetensors({k: v.detach().contiguous().cpu() for k, v in tensors.items()}, path, self.metadata())

    @classmethod
    def load(cls, path: str, device=None, max_bytes: int = 8 << 30) -> "CoactStats":
        meta, tensors = _pooled.open_stats_file(path, FORMAT, "a co-activation statistics")
        st = cls(int(meta["num_latents"]), tensors["queries"], pool=meta["pool"], pool_len=int(meta["pool_len"]),
                 window=int(meta["window"]), thresh=float(meta["thresh"]), device=device, max_bytes=max_bytes)
        dev = st.device
        st.counts.reshape(-1)[tensors["pair_key"].to(dev)] = tensors["pair_count"].to(dev)
        st.seg_count.copy_(tensors["seg_count"])
        st.n_segments = int(meta["n_segments"])
        return st


def _neighbors_host(counts: Tensor, seg_count: Tensor, queries: Tensor, m: int, metric: str, exclude_self: bool):
    """`msae_coact_topk` in plain torch: the same integers, the same f64 quotient rounded to f32, the same order."""
    F, _ = counts.shape
    ind = torch.full((F, m), -1, dtype=torch.int64)
    val = torch.zeros(F, m, dtype=torch.float32)
    counts, seg_count = counts.cpu(), seg_count.cpu()
    for i, q in enumerate(queries.cpu().tolist()):
        g = counts[i].nonzero().reshape(-1)              # ascending features
        if exclude_self:
            g = g[g != q]
        c = counts[i][g].to(torch.int64)
        if metric == "count":
            score = c.to(torch.float32)
        else:
            u = seg_count[q] + seg_count[g] - c
            score = (c.to(torch.float64) / u.to(torch.float64)).to(torch.float32)
        order = torch.sort(score, descending=True, stable=True).indices[:m]      # stable: ties stay by ascending feature
        ind[i, :order.numel()] = g[order]
        val[i, :order.numel()] = score[order]
    return ind, val


def coact_neighbors(stats_by_module: Dict[str, CoactStats], feature_filter, k: int = 10, metric: str = "jaccard"):
    """`get_neighbors` (msae/features/stats.py) from co-activation instead of decoder geometry, in its return shape: for
    every module with selected features in `feature_filter` (each a query of the module's statistics),
    (neighbors_dict {module: {i: {"indices", "values"}}}, per_layer_features {module: sorted unique features}).  As there,
    entry i holds up to k - 1 neighbours of the i-th selected feature, the feature itself left out (free slots are not
    listed), and per_layer_features holds the selected features and every listed neighbour."""
    if not 2 <= k <= MAX_NEIGHBORS + 1:
        raise ValueError(f"k must lie in [2, {MAX_NEIGHBORS + 1}], got {k}")
    neighbors_dict, per_layer_features = defaultdict(dict), {}
    for module_path, st in stats_by_module.items():
        selected = feature_filter.get(module_path, False)
        if selected is None or selected is False or len(selected) == 0:
            continue
        selected = selected.tolist() if isinstance(selected, Tensor) else [int(f) for f in selected]
        slot = {q: i for i, q in enumerate(st.queries.cpu().tolist())}
        missing = [f for f in selected if f not in slot]
        if missing:
            raise ValueError(f"{module_path}: features {missing[:8]} are not queries of the co-activation statistics")
        indices, values = st.neighbors(k=k - 1, metric=metric, exclude_self=True)
        indices, values = indices.cpu(), values.cpu()
        seen = set(selected)
        for i, f in enumerate(selected):
            row_i, row_v = indices[slot[f]], values[slot[f]]
            keep = row_i >= 0
            neighbors_dict[module_path][i] = {"indices": row_i[keep].tolist(), "values": row_v[keep].tolist()}
            seen.update(row_i[keep].tolist())
        per_layer_features[module_path] = sorted(seen)
    return neighbors_dict, per_layer_features
