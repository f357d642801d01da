"""Per-feature histograms of activation strength, built while the cache runs, and quantiles from them.

`FeatureStats` says how often a feature fires and shows its best and its typical examples, `CoactStats` what fires with it.
`ActHist` says HOW STRONGLY it fires: for every one of the N features a histogram of its segment values, from the top-k pairs
the cache loop already holds on the device (msae_act_hist_update, include/msae.h), next to the other two:

    pool="token"   every kept entry is a value (no de-duplication)
    pool="window"  the max-pooled value of a window of `window` positions  } exactly the candidate `FeatureStats` ranks,
    pool="image"   the mean over the first `pool_len` positions of a row  } bit for bit

An entry is kept by the cache's rule (|v| > thresh, 0 <= index < N, no feature filter); a segment value c is counted iff
c > 0 (NaN, zero and negative values are counted nowhere).  The bin of c is defined on its float32 bits:

    raw = (bits >> (23 - sub_bits)) - ((127 + e_lo) << sub_bits),  bin = clamp(raw, 0, n_bins - 1),  n_bins = octaves << sub_bits

i.e. 2^sub_bits bins per octave from 2^e_lo up; the defaults give 256 bins over [2^-16, 2^16), each under 12.5 % wide.

    hist [N, n_bins] int32   hist[f, b] = segment values of f in bin b
    n_segments               segments seen, empty ones included (a Python int, from the shapes alone)

All of it is exact integer arithmetic: the state does not depend on how rows are cut into calls or ranks, or on the order of
the calls, and two states merge by addition.  A quantile is read off the running counts with one f64 multiply (rank =
ceil(q * population)); with `zeros=True` the population is every segment seen, the ones in which the feature did not fire
counting as zeros below every bin."""
from __future__ import annotations

import math
from typing import Sequence, Union

import torch
from torch import Tensor

from .. import _hip, ops
from . import _pooled
from ._pooled import POOL_MODES, _write_safetensors

FORMAT = "msae.act_hist.v1"
MAX_BINS, MAX_Q = 512, 64
IS_ZERO, IS_EMPTY = -1, -2       # quantile_bins: the quantile is a zero / the feature has nothing to rank


@torch.library.custom_op("msae::act_hist_update", mutates_args=("hist",))
def act_hist_update(top_acts: Tensor, top_indices: Tensor, thresh: float, mode: int, pool_len: int, window: int,
                    sub_bits: int, e_lo: int, octaves: int, hist: Tensor) -> None:
    """One batch of `[B, S, k]` top-k pairs into the histograms (in place, stream-ordered, no host read)."""
    N, n_bins = hist.shape
    assert hist.dtype == torch.int32 and hist.is_contiguous() and n_bins == octaves << sub_bits
    dev, lib, vals, idx, Tk = _pooled.topk_inputs(top_acts, top_indices, hist)
    with torch.cuda.device(dev):
        ws = ops._workspace(dev, lib.msae_act_hist_ws_bytes(*Tk, N))
        _pooled.pooled_update(lib, "msae_act_hist_update", vals, idx, thresh, N, mode, pool_len, window,
                              (sub_bits, e_lo, octaves, _hip.ptr(hist)), ws)


@act_hist_update.register_fake
def _(top_acts, top_indices, thresh, mode, pool_len, window, sub_bits, e_lo, octaves, hist):
    return None


@torch.library.custom_op("msae::act_hist_quantiles", mutates_args=())
def act_hist_quantiles(hist: Tensor, qs: Tensor, n_segments: int, zeros: bool) -> Tensor:
    """bins [N, Q] int32 of the Q probabilities `qs` (f64, on the device) for every row of `hist`."""
    dev = _hip.require_device(hist, qs)
    lib = _hip.load()
    N, n_bins = hist.shape
    assert hist.dtype == torch.int32 and hist.is_contiguous() and qs.dtype == torch.float64 and qs.dim() == 1
    qs = qs.contiguous()
    out = torch.empty(N, qs.numel(), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_act_hist_quantiles(_hip.ptr(hist), N, n_bins, _hip.ptr(qs), qs.numel(), n_segments, int(zeros),
                                               _hip.ptr(out), _hip.stream_of(hist)), "msae_act_hist_quantiles")
    return out


@act_hist_quantiles.register_fake
def _(hist, qs, n_segments, zeros):
    return hist.new_empty((hist.shape[0], qs.shape[0]), dtype=torch.int32)


def _prob_list(qs, what: str = "qs") -> list:
    if isinstance(qs, Tensor):
        qs = qs.detach().cpu().reshape(-1).tolist()
    elif isinstance(qs, (int, float)):
        qs = [qs]
    q = [float(x) for x in qs]
    if not 1 <= len(q) <= MAX_Q:
        raise ValueError(f"the number of probabilities in {what} must lie in [1, {MAX_Q}], got {len(q)}")
    if any(not 0.0 <= x <= 1.0 for x in q):          # a NaN fails the comparison too
        raise ValueError(f"every probability in {what} must lie in [0, 1], got {q}")
    return q


def quantile_bins_host(hist: Tensor, qs: Sequence[float], n_segments: int, zeros: bool, rows: int = 16384) -> Tensor:
    """`msae_act_hist_quantiles` in plain torch on the CPU: the same integers, the same f64 multiply and ceil."""
    hist = hist.cpu()
    q = torch.tensor(list(qs), dtype=torch.float64)
    out = torch.empty(hist.shape[0], q.numel(), dtype=torch.int32)
    for r0 in range(0, hist.shape[0], rows):
        cum = hist[r0:r0 + rows].to(torch.int64).cumsum(1)
        n = cum[:, -1]
        z = (n_segments - n).clamp(min=0) if zeros else torch.zeros_like(n)
        tot = n + z
        r = torch.ceil(q[None, :] * tot[:, None].to(torch.float64)).to(torch.int64)
        r = torch.minimum(r.clamp(min=1), tot[:, None])
        b = torch.searchsorted(cum + z[:, None], r.contiguous(), right=False)      # the first bin whose running count reaches r
        b = torch.where(r <= z[:, None], torch.full_like(b, IS_ZERO), b)
        b = torch.where(tot[:, None] == 0, torch.full_like(b, IS_EMPTY), b)
        out[r0:r0 + rows] = b.to(torch.int32)
    return out


class ActHist:
    """Activation histograms of all `num_latents` features; see the module docstring.  The counters live on `device`;
    `update` and the kernel path of `quantile_bins` need a HIP device, `merge`, `quantile`, `save` and reading a loaded file
    do not."""

    def __init__(self, num_latents: int, pool: str = "token", pool_len: int = 576, window: int = 64, thresh: float = 1e-5,
                 sub_bits: int = 3, e_lo: int = -16, octaves: int = 32, device=None, max_bytes: int = 1 << 30):
        _pooled.check_pool(pool)
        _pooled.check_pool_args(num_latents, pool, pool_len, window)
        sub_bits, e_lo, octaves = int(sub_bits), int(e_lo), int(octaves)
        if not 0 <= sub_bits <= 4:
            raise ValueError(f"sub_bits must lie in [0, 4], got {sub_bits}")
        if octaves < 1 or e_lo < -126 or e_lo + octaves > 128:
            raise ValueError(f"the octaves [e_lo, e_lo + octaves) must lie in [-126, 128], got e_lo = {e_lo}, "
                             f"octaves = {octaves}")
        n_bins = octaves << sub_bits
        if n_bins > MAX_BINS:
            raise ValueError(f"n_bins = octaves << sub_bits must lie in [1, {MAX_BINS}], got {n_bins}")
        if num_latents * n_bins * 4 > max_bytes:
            raise ValueError(f"{num_latents} features x {n_bins} bins need {num_latents * n_bins * 4} bytes of counters, "
                             f"more than max_bytes = {max_bytes}")
        self.num_latents, self.pool = int(num_latents), pool
        self.pool_len, self.window, self.thresh = int(pool_len), int(window), float(thresh)
        self.sub_bits, self.e_lo, self.octaves, self.n_bins = sub_bits, e_lo, octaves, n_bins
        self.n_segments = 0
        dev = torch.device("cpu") if device is None else torch.device(device)
        self.hist = torch.zeros(num_latents, n_bins, dtype=torch.int32, device=dev)
        self._qs = {}                             # probabilities already on the device: a query reads nothing back

    @property
    def device(self) -> torch.device:
        return self.hist.device

    def _kind(self):
        return (self.num_latents, *_pooled.pool_kind(self.pool, self.pool_len, self.window), self.thresh, self.sub_bits,
                self.e_lo, self.octaves)

    def update(self, top_acts: Tensor, top_indices: Tensor) -> None:
        """Add one batch of `[B, S, k]` top-k pairs (complete rows only).  Every limit is checked on the host, from the
        shapes alone, before any device work; nothing is read back.  Empty input is a no-op."""
        B, S, k = _pooled.topk_shape(top_acts, top_indices)
        if B * S * k == 0:
            return
        _pooled.check_call_limits(S, k)
        total = _pooled.total_segments(self.n_segments, _pooled.segments_of(self.pool, B, S, self.window))
        _hip.require_device(top_acts, top_indices, self.hist)
        for rows in _pooled.row_chunks(B, S):
            torch.ops.msae.act_hist_update(top_acts[rows], top_indices[rows], self.thresh, POOL_MODES[self.pool],
                                           self.pool_len, self.window, self.sub_bits, self.e_lo, self.octaves, self.hist)
        self.n_segments = total

    def merge(self, other: "ActHist") -> "ActHist":
        """self += other (another rank's histograms of the same kind), on self's device, in plain torch."""
        if self._kind() != other._kind():
            raise ValueError(f"cannot merge activation histograms of different kinds: {self._kind()} vs {other._kind()}")
        total = _pooled.total_segments(self.n_segments, other.n_segments)
        self.hist += other.hist.to(self.device)
        self.n_segments = total
        return self

    # ---- reading -------------------------------------------------------------------------------------------------
    def edges(self) -> Tensor:
        """f32 [n_bins + 1]: bin b holds edge[b] <= c < edge[b + 1] (the two end bins also what lies beyond them)."""
        b = torch.arange(self.n_bins + 1, dtype=torch.int32, device=self.device)
        return ((b + ((127 + self.e_lo) << self.sub_bits)) << (23 - self.sub_bits)).view(torch.float32)

    def fired(self) -> Tensor:
        """int64 [N]: segment values counted per feature (the row totals)."""
        return self.hist.sum(dim=1, dtype=torch.int64)

    def quantile_bins(self, qs, zeros: bool = False) -> Tensor:
        """int32 [N, Q]: per feature and probability q the bin that holds the r-th smallest counted value, r =
        clamp(ceil(q * population), 1, population).  The population is the feature's counted values, with `zeros` every
        segment seen (the others count as zeros below bin 0): -1 = the quantile is such a zero, -2 = an empty population.
        The kernel on a HIP device, the same integers from plain torch anywhere else."""
        q = _prob_list(qs)
        if not self.hist.is_cuda:
            return quantile_bins_host(self.hist, q, self.n_segments, bool(zeros)).to(self.device)
        key = tuple(q)
        qd = self._qs.get(key)
        if qd is None or qd.device != self.device:
            if len(self._qs) >= 16:
                self._qs.clear()
            qd = self._qs[key] = torch.tensor(q, dtype=torch.float64, device=self.device)
        return torch.ops.msae.act_hist_quantiles(self.hist, qd, self.n_segments, bool(zeros))

    def quantile(self, qs, zeros: bool = False) -> Tensor:
        """f32 [N, Q]: the lower edge of `quantile_bins`' bin; 0.0 where the quantile is a zero, NaN for an empty
        population.  The true quantile lies in [edge, next edge): under 2^-sub_bits relative above the returned value."""
        bins = self.quantile_bins(qs, zeros).to(torch.int64)
        val = self.edges()[bins.clamp(min=0)]
        val = torch.where(bins == IS_ZERO, torch.zeros_like(val), val)
        return torch.where(bins == IS_EMPTY, torch.full_like(val, math.nan), val)

    def threshold_at_rate(self, rate: Union[float, Sequence[float]]) -> Tensor:
        """f32 [N, R]: the value a feature reaches or exceeds on (at least) a `rate` share of ALL segments seen -- the
        threshold a per-feature encoder firing at that rate would use: quantile(1 - rate, zeros=True).  0.0 where the
        feature fires on less than that share."""
        rates = _prob_list(rate, "rate")
        return self.quantile([1.0 - r for r in rates], zeros=True)

    # ---- file ----------------------------------------------------------------------------------------------------
    def metadata(self) -> dict:
        return {"format": FORMAT, "pool": self.pool, "pool_len": str(self.pool_len), "window": str(self.window),
                "thresh": repr(self.thresh), "num_latents": str(self.num_latents), "sub_bits": str(self.sub_bits),
                "e_lo": str(self.e_lo), "octaves": str(self.octaves), "n_segments": str(self.n_segments)}

    def save(self, path: str) -> None:
        """`hist` [N, n_bins] int32 as it is; every parameter and n_segments in the metadata.  Equal state, equal bytes."""
        _write_safetensors({"hist": self.hist.detach().contiguous().cpu()}, path, self.metadata())

    @classmethod
    def load(cls, path: str, device=None, max_bytes: int = 1 << 30) -> "ActHist":
        meta, tensors = _pooled.open_stats_file(path, FORMAT, "an activation histogram")
        hist = tensors["hist"]
        st = cls(int(meta["num_latents"]), pool=meta["pool"], pool_len=int(meta["pool_len"]), window=int(meta["window"]),
                 thresh=float(meta["thresh"]), sub_bits=int(meta["sub_bits"]), e_lo=int(meta["e_lo"]),
                 octaves=int(meta["octaves"]), device=device, max_bytes=max_bytes)
        if hist.shape != st.hist.shape or hist.dtype != torch.int32:
            raise ValueError(f"{path}: hist is {tuple(hist.shape)} {hist.dtype}, expected {tuple(st.hist.shape)} int32")
        st.hist.copy_(hist)
        st.n_segments = int(meta["n_segments"])
        return st
