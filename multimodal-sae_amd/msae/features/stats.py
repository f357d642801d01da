"""Per-feature statistics and top-example tables, built while the cache runs.

The reference's explain side re-derives two facts per feature from the COO split files after the cache is written:
how often the feature fires (the loader's `min_examples` cut, sae_auto_interp/features/loader.py:103-106) and which
rows activate it most (features/constructors.py:28-85 for text windows, 88-141 for images) -- the latter through a
dense `[rows, seq]` tensor per feature on the CPU, so only behind a small filter.  `FeatureStats` answers both for
every feature from the top-k pairs the cache loop already holds on the device (msae_feature_stats_update,
include/msae.h): count / max / sum of the kept records, and the `n_top` largest nonzero pooled values per feature
with their ids.

    pool="image"   one segment per row: mean of the first `pool_len` positions; id = global row
    pool="window"  windows of `window` positions: max; id = global row * (S // window) + w

The keep rule is the cache's (|v| > thresh, default 1e-5), without the cache's feature filter.

With `n_sample > 0` the same update also keeps, per feature, a uniform random sample of `n_sample` of ALL its nonzero pooled
segments (not only the largest) and their number `seg_count`: the `n_sample` segments whose hash of (sample_seed, feature,
id) is smallest.  That is what the reference's "random" and "quantile" example samplers need (msae/features/samplers.py).
The sample does not depend on the values, on how rows are cut into calls or ranks, or on the order of the calls.
"""
from __future__ import annotations

import ctypes
import json
from typing import Optional, Tuple

import torch
from safetensors.torch import save_file
from torch import Tensor

from .. import _hip, ops
from . import _pooled
from ._pooled import POOL_MODES

FORMAT = "msae.feature_stats.v1"
POOLS = ("image", "window")     # a token is no segment with examples to show
MIN_TOP, MAX_TOP = 55, 256      # 55 = the README's --max_examples 5 + the image constructor's 50 spare ids
MAX_SAMPLE = 256


@torch.library.custom_op("msae::feature_stats_update", mutates_args=("count", "act_max", "act_sum", "top_val",
                                                                      "top_id"))
def feature_stats_update(top_acts: Tensor, top_indices: Tensor, row_base: int, thresh: float, mode: int,
                         pool_len: int, window: int, count: Tensor, act_max: Tensor, act_sum: Tensor, top_val: Tensor,
                         top_id: Tensor) -> None:
    """One batch of `[B, S, k]` top-k pairs into the statistics (in place, stream-ordered, no host read)."""
    N, n = top_val.shape
    state = (count, act_max, act_sum, top_val, top_id)
    dev, lib, vals, idx, Tk = _pooled.topk_inputs(top_acts, top_indices, *state)
    with torch.cuda.device(dev):
        ws = ops._workspace(dev, lib.msae_feature_stats_ws_bytes(*Tk, N))
        _pooled.pooled_update(lib, "msae_feature_stats_update", vals, idx, thresh, N, mode, pool_len, window,
                              (row_base, n, *[_hip.ptr(t) for t in state]), ws)


@feature_stats_update.register_fake
def _(top_acts, top_indices, row_base, thresh, mode, pool_len, window, count, act_max, act_sum, top_val, top_id):
    return None


@torch.library.custom_op("msae::feature_stats_update_sampled",
                         mutates_args=("count", "act_max", "act_sum", "top_val", "top_id", "seg_count", "smp_val", "smp_id"))
def feature_stats_update_sampled(top_acts: Tensor, top_indices: Tensor, row_base: int, thresh: float, mode: int,
                                 pool_len: int, window: int, count: Tensor, act_max: Tensor, act_sum: Tensor,
                                 top_val: Tensor, top_id: Tensor, seed: int, seg_count: Tensor, smp_val: Tensor,
                                 smp_id: Tensor) -> None:
    """`feature_stats_update` that also merges the batch into the uniform sample tables (`seed`: the 64-bit sample seed,
    taken mod 2^64) -- one more table merge in the same launch."""
    N, n = top_val.shape
    assert smp_val.shape == smp_id.shape and smp_val.shape[0] == N and seg_count.shape == (N,)
    state = (count, act_max, act_sum, top_val, top_id)
    dev, lib, vals, idx, Tk = _pooled.topk_inputs(top_acts, top_indices, *state, seg_count, smp_val, smp_id)
    sample = _hip.MsaeFeatureSample(ctypes.sizeof(_hip.MsaeFeatureSample), smp_val.shape[1], seed % (1 << 64),
                                    seg_count.data_ptr(), smp_val.data_ptr(), smp_id.data_ptr())
    with torch.cuda.device(dev):
        ws = ops._workspace(dev, lib.msae_feature_stats_ws_bytes(*Tk, N))
        _pooled.pooled_update(lib, "msae_feature_stats_update_sampled", vals, idx, thresh, N, mode, pool_len, window,
                              (row_base, n, *[_hip.ptr(t) for t in state], ctypes.byref(sample)), ws)


@feature_stats_update_sampled.register_fake
def _(top_acts, top_indices, row_base, thresh, mode, pool_len, window, count, act_max, act_sum, top_val, top_id, seed,
      seg_count, smp_val, smp_id):
    return None


class FeatureStats:
    """Statistics of `num_latents` features: count (int64), act_max (f32), act_sum (f64), and the sorted top-n tables
    top_val [N, n] (f32) / top_id [N, n] (int64; -1 = free slot).  With `n_sample > 0` also seg_count (int64: nonzero pooled
    segments seen) and the uniform sample tables smp_val / smp_id [N, n_sample], sorted by hash priority.  The tables live
    on `device`; `update` and `merge` need a HIP device, reading a loaded file does not."""

    def __init__(self, num_latents: int, n_top: int = 64, pool: str = "image", pool_len: int = 576, window: int = 64,
                 thresh: float = 1e-5, device=None, n_sample: int = 0, sample_seed: int = 22):
        _pooled.check_pool(pool, POOLS)
        if not MIN_TOP <= n_top <= MAX_TOP:
            raise ValueError(f"n_top must lie in [{MIN_TOP}, {MAX_TOP}], got {n_top}")
        _pooled.check_pool_args(num_latents, pool, pool_len, window)
        if not 0 <= n_sample <= MAX_SAMPLE:
            raise ValueError(f"n_sample must lie in [0, {MAX_SAMPLE}] (0: no sample), got {n_sample}")
        if not 0 <= sample_seed < 1 << 64:
            raise ValueError(f"sample_seed must lie in [0, 2^64), got {sample_seed}")
        self.num_latents, self.n_top, self.pool = num_latents, n_top, pool
        self.pool_len, self.window, self.thresh = pool_len, window, float(thresh)
        self.tokens_seen = 0
        self.windows_per_row: Optional[int] = None      # S // window of the rows seen (window mode)
        dev = torch.device("cpu") if device is None else torch.device(device)
        N = num_latents
        self.count = torch.zeros(N, dtype=torch.int64, device=dev)
        self.act_max = torch.full((N,), float("-inf"), dtype=torch.float32, device=dev)
        self.act_sum = torch.zeros(N, dtype=torch.float64, device=dev)
        self.top_val = torch.zeros(N, n_top, dtype=torch.float32, device=dev)
        self.top_id = torch.full((N, n_top), -1, dtype=torch.int64, device=dev)
        self.n_sample, self.sample_seed = int(n_sample), int(sample_seed)
        if self.n_sample:
            self.seg_count = torch.zeros(N, dtype=torch.int64, device=dev)
            self.smp_val = torch.zeros(N, n_sample, dtype=torch.float32, device=dev)
            self.smp_id = torch.full((N, n_sample), -1, dtype=torch.int64, device=dev)

    @property
    def device(self) -> torch.device:
        return self.count.device

    def _same_kind(self, other: "FeatureStats") -> None:
        mine = (self.num_latents, self.n_top, self.pool, self.pool_len if self.pool == "image" else self.window,
                self.thresh, self.n_sample, self.sample_seed)
        theirs = (other.num_latents, other.n_top, other.pool, other.pool_len if other.pool == "image" else other.window,
                  other.thresh, other.n_sample, other.sample_seed)
        if mine != theirs:
            raise ValueError(f"cannot merge feature statistics of different kinds: {mine} vs {theirs}")

    def update(self, top_acts: Tensor, top_indices: Tensor, row_base: int) -> None:
        """Add one batch of `[B, S, k]` top-k pairs whose rows are `row_base + b` (complete rows only)."""
        B, S, _ = top_acts.shape
        if self.pool == "window":
            nw = S // self.window
            if self.windows_per_row is not None and self.windows_per_row != nw:
                raise ValueError(f"rows of {S} positions give {nw} windows, earlier rows gave {self.windows_per_row}")
            self.windows_per_row = nw
        args = (top_acts, top_indices, int(row_base), self.thresh, POOL_MODES[self.pool], self.pool_len, self.window,
                self.count, self.act_max, self.act_sum, self.top_val, self.top_id)
        if self.n_sample:       # the custom op's int is 64-bit signed: the seed travels as its two's complement
            seed = self.sample_seed - (1 << 64) if self.sample_seed >= 1 << 63 else self.sample_seed
            torch.ops.msae.feature_stats_update_sampled(*args, seed, self.seg_count, self.smp_val, self.smp_id)
        else:
            torch.ops.msae.feature_stats_update(*args)
        self.tokens_seen += B * S

    def merge(self, other: "FeatureStats") -> "FeatureStats":
        """self += other (another rank's or module part's statistics of the same kind), on self's device."""
        self._same_kind(other)
        if (self.windows_per_row is not None and other.windows_per_row is not None
                and self.windows_per_row != other.windows_per_row):
            raise ValueError("cannot merge window statistics of different row lengths")
        dev = _hip.require_device(self.count)
        o = [t.to(dev).contiguous() for t in (other.count, other.act_max, other.act_sum, other.top_val, other.top_id)]
        with torch.cuda.device(dev):
            _hip.check(_hip.load().msae_feature_stats_merge(
                self.num_latents, self.n_top, _hip.ptr(self.count), _hip.ptr(self.act_max), _hip.ptr(self.act_sum),
                _hip.ptr(self.top_val), _hip.ptr(self.top_id), *[_hip.ptr(t) for t in o],
                _hip.stream_of(self.count)), "msae_feature_stats_merge")
            if self.n_sample:
                so = [t.to(dev).contiguous() for t in (other.seg_count, other.smp_val, other.smp_id)]
                _hip.check(_hip.load().msae_feature_sample_merge(
                    self.num_latents, self.n_sample, self.sample_seed, _hip.ptr(self.seg_count), _hip.ptr(self.smp_val),
                    _hip.ptr(self.smp_id), *[_hip.ptr(t) for t in so], _hip.stream_of(self.count)),
                    "msae_feature_sample_merge")
        self.tokens_seen += other.tokens_seen
        if self.windows_per_row is None:
            self.windows_per_row = other.windows_per_row
        return self

    def density(self) -> Tensor:
        """Fraction of the tokens seen on which each feature fired (f64)."""
        return self.count.double() / max(self.tokens_seen, 1)

    def top_examples(self, feature: int) -> Tuple[Tensor, Tensor]:
        """(ids int64, pooled values f32) of the feature's top examples, best first (host tensors)."""
        ids, vals = self.top_id[feature].cpu(), self.top_val[feature].cpu()
        keep = ids >= 0
        return ids[keep], vals[keep]

    def sample_examples(self, feature: int) -> Tuple[Tensor, Tensor]:
        """(ids int64, pooled values f32) of the feature's uniform sample, in priority order (host tensors): a uniform
        draw without replacement from all `seg_count[feature]` nonzero pooled segments; any prefix is one too."""
        if not self.n_sample:
            raise ValueError("these statistics keep no sample (n_sample = 0)")
        ids, vals = self.smp_id[feature].cpu(), self.smp_val[feature].cpu()
        keep = ids >= 0
        return ids[keep], vals[keep]

    def sample_fraction(self) -> Tensor:
        """min(1, n_sample / seg_count) per feature (f64): the share of a feature's nonzero pooled segments its sample
        holds (1 where the sample is the whole population)."""
        if not self.n_sample:
            raise ValueError("these statistics keep no sample (n_sample = 0)")
        return (self.n_sample / self.seg_count.double().clamp(min=1.0)).clamp(max=1.0)

    def metadata(self) -> dict:
        meta = {"format": FORMAT, "pool": self.pool, "pool_len": str(self.pool_len),
                "window": str(self.window), "n_top": str(self.n_top), "thresh": repr(self.thresh),
                "num_latents": str(self.num_latents), "tokens_seen": str(self.tokens_seen),
                "windows_per_row": json.dumps(self.windows_per_row)}
        if self.n_sample:
            meta.update(n_sample=str(self.n_sample), sample_seed=str(self.sample_seed))
        return meta

    def save(self, path: str) -> None:
        tensors = {"count": self.count, "act_max": self.act_max, "act_sum": self.act_sum, "top_val": self.top_val,
                   "top_id": self.top_id}
        if self.n_sample:
            tensors.update(seg_count=self.seg_count, smp_val=self.smp_val, smp_id=self.smp_id)
        save_file({k: v.detach().contiguous().cpu() for k, v in tensors.items()}, path, metadata=self.metadata())

    @classmethod
    def load(cls, path: str, device=None) -> "FeatureStats":
        meta, tensors = _pooled.open_stats_file(path, FORMAT, "a feature statistics")
        st = cls(int(meta["num_latents"]), n_top=int(meta["n_top"]), pool=meta["pool"],
                 pool_len=int(meta["pool_len"]), window=int(meta["window"]), thresh=float(meta["thresh"]),
                 device="cpu", n_sample=int(meta.get("n_sample", 0)), sample_seed=int(meta.get("sample_seed", 22)))
        for k, v in tensors.items():
            setattr(st, k, v if device is None else v.to(device))
        st.tokens_seen = int(meta["tokens_seen"])
        st.windows_per_row = json.loads(meta["windows_per_row"])
        return st


# ---- neighbours and top logits (sae_auto_interp/features/stats.py:12-47,76-120) ----------------------------------------
def cos(matrix: Tensor, selected_features=(0,)) -> Tensor:
    """Dense cosine similarities [M, N] of the selected rows of `matrix` against all of its rows (stats.py:76-85), for
    small selections.  matrix is [N, d] -- one row per feature, as `Sae.W_dec` and `Sae.encoder.weight` are here (the
    reference's decoder.weight is its transpose).  Same arithmetic as `Sae.neighbors`: the exact f32 dot, then
    * inv[m], then * inv[n]."""
    ops._no_grad_inputs("features.cos", matrix)
    W = matrix.detach().to(torch.float32).contiguous()
    sel = torch.as_tensor(list(selected_features) if not isinstance(selected_features, Tensor) else selected_features,
                          dtype=torch.int64).to(W.device)
    inv = ops.row_inv_norms(W)
    dots = ops._dense_gemm_nt(W.index_select(0, sel), W)
    return dots * inv.index_select(0, sel)[:, None] * inv[None, :]


def get_neighbors(sae_dict, feature_filter, k: int = 10):
    """The reference's get_neighbors (stats.py:88-120) over {module name: Sae}: for every module with selected features in
    `feature_filter`, the top k decoder cosines of each selected feature INCLUDING itself with rank 0 dropped, so each
    entry holds k - 1 neighbours -> (neighbors_dict {module: {i: {"indices", "values"}}}, per_layer_features {module:
    sorted unique indices of the full top k}).  As in the reference, with exact duplicate decoder rows the dropped rank 0
    may be the twin rather than the feature itself; `Sae.neighbors(exclude_self=True)` skips the
    feature by index instead."""
    from collections import defaultdict

    neighbors_dict, per_layer_features = defaultdict(dict), {}
    for module_path, sae in sae_dict.items():
        selected = feature_filter.get(module_path, False)
        if selected is None or selected is False or len(selected) == 0:
            continue
        values, indices = sae.neighbors(selected, k=k, matrix="decoder", exclude_self=False)
        values, indices = values.cpu(), indices.cpu()
        for i in range(indices.shape[0]):
            neighbors_dict[module_path][i] = {"indices": indices[i].tolist()[1:], "values": values[i].tolist()[1:]}
        per_layer_features[module_path] = torch.unique(indices).tolist()
    return neighbors_dict, per_layer_features


def logits(records, W_U: Tensor, W_dec, k: int = 10, tokenizer=None):
    """Direct logit attribution of a list of feature records (stats.py:12-47): sets `record.top_logits` to the decoded
    top-k tokens of `W_U @ W_dec[feature]` and returns the list.  W_U: the unembedding [V, d]; W_dec: an `Sae`, or its
    decoder as [N, d] (a [d, N] matrix, the reference's layout, is transposed)."""
    from ..sae import Sae

    feats = [int(r.feature.feature_index) for r in records]
    if isinstance(W_dec, Sae):
        _, top = W_dec.top_logits(W_U, feats, k=k)
    else:
        if W_dec.shape[-1] != W_U.shape[-1] and W_dec.shape[0] == W_U.shape[-1]:
            W_dec = W_dec.t()
        rows = torch.tensor(feats, dtype=torch.int32).to(W_dec.device)
        _, top = ops.rows_topk(W_dec.detach(), W_U.detach(), k, q_rows=rows)     # (token strings carry no gradient)
    top = top.cpu()
    decoded_top_logits = []
    for i, record in enumerate(records):
        decoded = tokenizer.batch_decode(top[i])
        decoded_top_logits.append(decoded)
        record.top_logits = decoded
    return decoded_top_logits
