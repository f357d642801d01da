"""Per-feature position profiles, built while the cache runs: WHERE IN A ROW a feature fires.

`FeatureStats` says how often a feature fires and on what, `CoactStats` what fires with it, `ActHist` how strongly.
`PosProfile` says where: for every one of the N features, per position bin, how often it fired there and how strongly, from
the top-k pairs the cache loop already holds on the device (msae_pos_profile_update, include/msae.h).  Two uses: listing the
POSITIONAL features (position 0 / BOS, the first few tokens, the image border, attention sinks) so that an interp or steering
run can leave them out, and a dataset-level map of where on the image grid a feature fires.

A position table `bins` (int32 [L], values in [-1, P)) and `tail_bin` name the bin of position s of a row: bins[s] for s < L,
tail_bin for s >= L; bin -1 is counted nowhere.  An entry (v, f) is kept by the cache's rule (|v| > thresh, 0 <= f < N, no
feature filter) and counted iff v > 0 (`ActHist`'s rule: NaN, zero and negative values are counted nowhere):

    count [N, P] int32       count[f, b] = counted entries of f in bin b
    mass  [N, P] int64       the sum of q(v) = llrint(v * 2^20) (half to even, at most 2^60) over them: an unsigned sum mod 2^64
    bin_positions [P] int64  positions seen per bin, empty ones included (on the host, from the shapes alone)
    n_rows, n_positions      Python ints

All of it is exact integer arithmetic: the state does not depend on how rows are cut into calls or ranks, or on the order of
the calls, and two states of one kind (N, P, tail_bin, thresh and the table) merge by addition.  The PEAK of a feature is the
bin with its highest firing RATE count / bin_positions (bins are unequal: the "rest" bin of an anyres row holds 2304
positions against 16 per grid cell), compared exactly, ties to the lowest bin."""
from __future__ import annotations

import hashlib
import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _hip, ops
from . import _pooled
from ._pooled import _write_safetensors

FORMAT = "msae.pos_profile.v1"
MAX_POSITIONS, MAX_BINS = 65536, 1024
MASS_ONE = 1 << 20                 # q(1.0)


@torch.library.custom_op("msae::pos_profile_update", mutates_args=("count", "mass"))
def pos_profile_update(top_acts: Tensor, top_indices: Tensor, thresh: float, pos_bin: Tensor, tail_bin: int, count: Tensor,
                       mass: Tensor) -> None:
    """One batch of `[B, S, k]` top-k pairs into the profiles (in place, stream-ordered, no host read)."""
    N, P = count.shape
    assert count.dtype == torch.int32 and count.is_contiguous() and mass.dtype == torch.int64 and mass.is_contiguous()
    assert mass.shape == count.shape and pos_bin.dtype == torch.int32 and pos_bin.dim() == 1 and pos_bin.is_contiguous()
    dev, lib, vals, idx, Tk = _pooled.topk_inputs(top_acts, top_indices, pos_bin, count, mass)
    B, S, k = vals.shape
    with torch.cuda.device(dev):
        ws = ops._workspace(dev, lib.msae_pos_profile_ws_bytes(*Tk, N))
        _hip.check(lib.msae_pos_profile_update(_hip.ptr(vals), _hip.ptr(idx), B, S, k, thresh, N, _hip.ptr(pos_bin),
                                               pos_bin.numel(), tail_bin, P, _hip.ptr(count), _hip.ptr(mass), _hip.ptr(ws),
                                               ws.numel(), _hip.stream_of(vals)), "msae_pos_profile_update")


@pos_profile_update.register_fake
def _(top_acts, top_indices, thresh, pos_bin, tail_bin, count, mass):
    return None


@torch.library.custom_op("msae::pos_profile_summary", mutates_args=())
def pos_profile_summary(count: Tensor, bin_positions: Tensor) -> Tuple[Tensor, Tensor]:
    """(fired [N] int64, peak [N, 2] int32 = (bin, count in it)) for every row of `count`; `bin_positions` int64 [P] on the
    device."""
    dev = _hip.require_device(count, bin_positions)
    lib = _hip.load()
    N, P = count.shape
    assert count.dtype == torch.int32 and count.is_contiguous()
    assert bin_positions.dtype == torch.int64 and bin_positions.shape == (P,) and bin_positions.is_contiguous()
    fired = torch.empty(N, dtype=torch.int64, device=dev)
    peak = torch.empty(N, 2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_pos_profile_summary(_hip.ptr(count), _hip.ptr(bin_positions), N, P, _hip.ptr(fired),
                                                _hip.ptr(peak), _hip.stream_of(count)), "msae_pos_profile_summary")
    return fired, peak


@pos_profile_summary.register_fake
def _(count, bin_positions):
    return (count.new_empty((count.shape[0],), dtype=torch.int64), count.new_empty((count.shape[0], 2), dtype=torch.int32))


def summary_host(count: Tensor, bin_positions: Tensor) -> Tuple[Tensor, Tensor]:
    """`msae_pos_profile_summary` in plain torch on the CPU: the same integers.  One pass over the bins in ascending order;
    a bin takes the peak only with a strictly higher rate (c * n_best > c_best * n in int64), so ties stay with the lowest."""
    count, bp = count.cpu(), bin_positions.cpu().to(torch.int64).tolist()
    N, P = count.shape
    fired = count.sum(dim=1, dtype=torch.int64)
    best_c = torch.zeros(N, dtype=torch.int64)
    best_n = torch.ones(N, dtype=torch.int64)
    best_b = torch.full((N,), -1, dtype=torch.int64)
    for b in range(P):
        n = bp[b]
        if n <= 0:
            continue
        c = count[:, b].to(torch.int64)
        better = c * best_n > best_c * n
        best_c = torch.where(better, c, best_c)
        best_n = torch.where(better, torch.full_like(best_n, n), best_n)
        best_b = torch.where(better, torch.full_like(best_b, b), best_b)
    return fired, torch.stack([best_b, best_c], dim=1).to(torch.int32)


def _as_table(bins) -> Tensor:
    t = bins.detach().cpu() if isinstance(bins, Tensor) else torch.as_tensor(list(bins))
    if t.dim() != 1:
        raise ValueError(f"bins must be one-dimensional, got shape {tuple(t.shape)}")
    if t.numel() and (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool):
        raise ValueError(f"bins must hold integers, got {t.dtype}")
    return t.to(torch.int64)


class PosProfile:
    """Position profiles of all `num_latents` features; see the module docstring.  The counters live on `device`; `update`
    and the kernel path of `summary` need a HIP device, everything else -- `merge`, `save`, and every reading of a loaded
    file -- does not."""

    def __init__(self, num_latents: int, bins, tail_bin: int = -1, n_bins: Optional[int] = None, thresh: float = 1e-5,
                 device=None, max_bytes: int = 1 << 30):
        if not 0 < num_latents <= _pooled.MAX_LATENTS:
            raise ValueError(f"num_latents must lie in [1, {_pooled.MAX_LATENTS}], got {num_latents}")
        table = _as_table(bins)
        L, tail_bin = table.numel(), int(tail_bin)
        if not 1 <= L <= MAX_POSITIONS:
            raise ValueError(f"the position table must hold 1 to {MAX_POSITIONS} positions, got {L}")
        top = max(int(table.max()), tail_bin)
        n_bins = max(top + 1, 1) if n_bins is None else int(n_bins)
        if not 1 <= n_bins <= MAX_BINS:
            raise ValueError(f"n_bins must lie in [1, {MAX_BINS}], got {n_bins}")
        if int(table.min()) < -1 or top >= n_bins or tail_bin < -1:
            raise ValueError(f"every bin of the table and tail_bin must lie in [-1, {n_bins}), got a table over "
                             f"[{int(table.min())}, {int(table.max())}] and tail_bin = {tail_bin}")
        if num_latents * n_bins * 12 > max_bytes:
            raise ValueError(f"{num_latents} features x {n_bins} bins need {num_latents * n_bins * 12} bytes of counters, "
                             f"more than max_bytes = {max_bytes}")
        self.num_latents, self.n_bins, self.tail_bin, self.thresh = int(num_latents), n_bins, tail_bin, float(thresh)
        self.table = table.to(torch.int32)                      # on the host; `_table_dev` is its copy next to the counters
        self.n_rows = self.n_positions = 0
        dev = torch.device("cpu") if device is None else torch.device(device)
        self.count = torch.zeros(num_latents, n_bins, dtype=torch.int32, device=dev)
        self.mass = torch.zeros(num_latents, n_bins, dtype=torch.int64, device=dev)
        self.bin_positions = torch.zeros(n_bins, dtype=torch.int64)
        self._table_dev = self.table.to(dev)
        self._row_hist = {}            # S -> (positions per bin of one row of S positions, the same on the device)
        self._bp_dev = None            # bin_positions on the device, kept in step by `update`; None: rebuild from the host's

    @property
    def device(self) -> torch.device:
        return self.count.device

    def _kind(self):
        return (self.num_latents, self.n_bins, self.tail_bin, self.thresh, self.table.numpy().tobytes())

    def kind_hash(self) -> str:
        """sha256 over (N, P, tail_bin, thresh, the table): what two states must share to merge."""
        N, P, tail, thresh, table = self._kind()
        return hashlib.sha256(f"{N},{P},{tail},{thresh!r},".encode() + table).hexdigest()

    def _positions_of_row(self, S: int):
        hit = self._row_hist.get(S)
        if hit is None:
            if len(self._row_hist) >= 64:
                self._row_hist.clear()
            head = self.table[:S].to(torch.int64)
            row = torch.bincount(head[head >= 0], minlength=self.n_bins)
            if S > self.table.numel() and self.tail_bin >= 0:
                row[self.tail_bin] += S - self.table.numel()
            hit = self._row_hist[S] = (row, row.to(self.device) if self.count.is_cuda else None)
        return hit

    def update(self, top_acts: Tensor, top_indices: Tensor) -> None:
        """Add one batch of `[B, S, k]` top-k pairs (complete rows only).  Every limit is checked on the host, from the
        shapes alone, before any device work; nothing is read back.  Empty input is a no-op."""
        B, S, k = _pooled.topk_shape(top_acts, top_indices)
        if B * S * k == 0:
            return
        _pooled.check_call_limits(S, k)
        total = _pooled.total_segments(self.n_positions, B * S)
        _hip.require_device(top_acts, top_indices, self.count)
        row, row_dev = self._positions_of_row(S)
        for rows in _pooled.row_chunks(B, S):
            torch.ops.msae.pos_profile_update(top_acts[rows], top_indices[rows], self.thresh, self._table_dev, self.tail_bin,
                                              self.count, self.mass)
        self.bin_positions += row * B
        if self._bp_dev is not None:
            self._bp_dev.add_(row_dev, alpha=B)
        self.n_rows += B
        self.n_positions = total

    def merge(self, other: "PosProfile") -> "PosProfile":
        """self += other (another rank's profiles of the same kind), on self's device, in plain torch."""
        if self._kind() != other._kind():
            raise ValueError("cannot merge position profiles of different kinds: "
                             f"{self._kind()[:4]} / table {self.kind_hash()[:12]} vs "
                             f"{other._kind()[:4]} / table {other.kind_hash()[:12]}")
        total = _pooled.total_segments(self.n_positions, other.n_positions)
        self.count += other.count.to(self.device)
        self.mass += other.mass.to(self.device)               # int64 adds wrap: the unsigned sum mod 2^64
        self.bin_positions += other.bin_positions
        self._bp_dev = None
        self.n_rows += other.n_rows
        self.n_positions = total
        return self

    # ---- bin builders: (table, tail_bin, n_bins, names) -----------------------------------------------------------
    @staticmethod
    def grid_bins(side: int = 24, cell: int = 4, rest: bool = True) -> Tuple[Tensor, int, int, List[str]]:
        """The row-major `side` x `side` base grid coarsened to (side / cell)^2 cells of `cell` x `cell` positions, plus --
        with `rest` -- one bin for every later position (anyres tiles, text)."""
        side, cell = int(side), int(cell)
        if side < 1 or cell < 1 or side % cell:
            raise ValueError(f"the grid side must be a positive multiple of the cell, got side = {side}, cell = {cell}")
        g = side // cell
        s = torch.arange(side * side)
        table = ((s // side) // cell * g + (s % side) // cell).to(torch.int32)
        names = [f"cell {r},{c}" for r in range(g) for c in range(g)]
        return (table, g * g, g * g + 1, names + ["rest"]) if rest else (table, -1, g * g, names)

    @staticmethod
    def log2_bins(L: int) -> Tuple[Tensor, int, int, List[str]]:
        """Bin 0 for position 0, then 1 + floor(log2 s): positions 1, 2-3, 4-7, ..."""
        L = int(L)
        if not 1 <= L <= MAX_POSITIONS:
            raise ValueError(f"L must lie in [1, {MAX_POSITIONS}], got {L}")
        table = torch.tensor([s.bit_length() for s in range(L)], dtype=torch.int32)
        P = (L - 1).bit_length() + 1
        names = ["0"] + [f"{1 << (b - 1)}-{min((1 << b), L) - 1}" for b in range(1, P)]
        return table, -1, P, names

    @staticmethod
    def linear_bins(L: int, P: int) -> Tuple[Tensor, int, int, List[str]]:
        """P bins of (nearly) equal width over L positions: position s falls into s * P // L."""
        L, P = int(L), int(P)
        if not 1 <= L <= MAX_POSITIONS or not 1 <= P <= MAX_BINS:
            raise ValueError(f"L must lie in [1, {MAX_POSITIONS}] and P in [1, {MAX_BINS}], got L = {L}, P = {P}")
        table = (torch.arange(L) * P // L).to(torch.int32)
        names = [f"{-(-b * L // P)}-{-(-(b + 1) * L // P) - 1}" for b in range(P)]
        return table, -1, P, names

    def grid_shape(self) -> Tuple[int, int]:
        """(gh, gw) when the table is one `grid_bins` builds (with or without the rest bin); ValueError otherwise."""
        side = math.isqrt(self.table.numel())
        if side * side == self.table.numel():
            row = self.table[:side].tolist()
            cell = row.count(0)
            if cell and side % cell == 0 and torch.equal(self.table, PosProfile.grid_bins(side, cell, False)[0]):
                return side // cell, side // cell
        raise ValueError("maps need the bins of PosProfile.grid_bins")

    # ---- reading -------------------------------------------------------------------------------------------------
    def _rows(self, t: Tensor, features) -> Tensor:
        if features is None:
            return t
        f = torch.as_tensor(features, dtype=torch.int64, device=t.device).reshape(-1)
        return t[f]

    def summary(self) -> Tuple[Tensor, Tensor]:
        """(fired int64 [N], peak int32 [N, 2] = (bin, count in it)): per feature its counted entries and the bin with its
        highest firing rate (-1: it never fired).  The kernel on a HIP device, the same integers from `summary_host`
        anywhere else."""
        if not self.count.is_cuda:
            fired, peak = summary_host(self.count, self.bin_positions)
            return fired.to(self.device), peak.to(self.device)
        if self._bp_dev is None:
            self._bp_dev = self.bin_positions.to(self.device)
        return torch.ops.msae.pos_profile_summary(self.count, self._bp_dev)

    def fired(self) -> Tensor:
        """int64 [N]: counted entries per feature (the row totals)."""
        return self.count.sum(dim=1, dtype=torch.int64)

    def share(self) -> Tensor:
        """f64 [N]: the share of a feature's fires that fall into its peak bin; NaN for a feature that never fired."""
        fired, peak = self.summary()
        return peak[:, 1].to(torch.float64) / fired.to(torch.float64)

    def rate(self, features=None) -> Tensor:
        """f64 [N, P] (or the rows of `features`): count / bin_positions, the firing rate per position of the bin; NaN for
        a bin no position fell into."""
        return self._rows(self.count, features).to(torch.float64) / self.bin_positions.to(self.device, torch.float64)

    def mean_activation(self, features=None) -> Tensor:
        """f64 [N, P] (or the rows of `features`): mass / 2^20 / count, the mean strength of the fires in the bin; NaN
        where there are none."""
        m = self._rows(self.mass, features)
        mass = m.to(torch.float64) + (m < 0).to(torch.float64) * 2.0 ** 64         # the int64 holds an unsigned sum
        return mass / MASS_ONE / self._rows(self.count, features).to(torch.float64)

    def maps(self, features=None) -> Tuple[Tensor, Tensor]:
        """(rate, mean strength), each f64 [F, gh, gw] over the grid cells, for bins built by `grid_bins`."""
        gh, gw = self.grid_shape()
        rate, mean = self.rate(features), self.mean_activation(features)
        return rate[:, :gh * gw].reshape(-1, gh, gw), mean[:, :gh * gw].reshape(-1, gh, gw)

    def modality_share(self, features, bins_a: Sequence[int]) -> Tensor:
        """f64 [F]: the share of a feature's fires inside the bin set `bins_a` (e.g. the base image's cells against the
        rest of the row); NaN for a feature that never fired."""
        c = self._rows(self.count, features).to(torch.int64)
        sel = torch.as_tensor(list(bins_a), dtype=torch.int64, device=c.device)
        return c[:, sel].sum(dim=1).to(torch.float64) / c.sum(dim=1).to(torch.float64)

    def positional(self, min_share: float = 0.9, min_fired: int = 16) -> Tensor:
        """int64 feature ids, ascending: features with at least `min_fired` fires of which at least `min_share` fall into
        the peak bin -- the ones to leave out of an interp or steering run."""
        fired, peak = self.summary()
        share = peak[:, 1].to(torch.float64) / fired.to(torch.float64)
        return torch.nonzero((fired >= min_fired) & (share >= min_share)).reshape(-1)

    # ---- file ----------------------------------------------------------------------------------------------------
    def metadata(self) -> dict:
        return {"format": FORMAT, "num_latents": str(self.num_latents), "n_bins": str(self.n_bins),
                "tail_bin": str(self.tail_bin), "thresh": repr(self.thresh), "kind": self.kind_hash(),
                "pos_bin": ",".join(str(b) for b in self.table.tolist()), "n_rows": str(self.n_rows),
                "n_positions": str(self.n_positions)}

    def save(self, path: str) -> None:
        """`count` int32, `mass` and `bin_positions` int64 as they are; the table, the kind and the totals in the metadata.
        Equal state, equal bytes."""
        _write_safetensors({"count": self.count.detach().contiguous().cpu(), "mass": self.mass.detach().contiguous().cpu(),
                            "bin_positions": self.bin_positions}, path, self.metadata())

    @classmethod
    def load(cls, path: str, device=None, max_bytes: int = 1 << 30) -> "PosProfile":
        meta, tensors = _pooled.open_stats_file(path, FORMAT, "a position profile")
        st = cls(int(meta["num_latents"]), [int(b) for b in meta["pos_bin"].split(",")], tail_bin=int(meta["tail_bin"]),
                 n_bins=int(meta["n_bins"]), thresh=float(meta["thresh"]), device=device, max_bytes=max_bytes)
        if st.kind_hash() != meta["kind"]:
            raise ValueError(f"{path}: the kind {meta['kind'][:12]} does not match the file's parameters")
        for name, dtype in (("count", torch.int32), ("mass", torch.int64), ("bin_positions", torch.int64)):
            t, own = tensors[name], getattr(st, name)
            if t.shape != own.shape or t.dtype != dtype:
                raise ValueError(f"{path}: {name} is {tuple(t.shape)} {t.dtype}, expected {tuple(own.shape)} {dtype}")
            own.copy_(t)
        st.n_rows, st.n_positions = int(meta["n_rows"]), int(meta["n_positions"])
        return st
