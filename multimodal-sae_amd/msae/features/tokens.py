"""Token profiles of a list of query features, built while the cache runs: ON WHICH TOKENS a feature fires.

`FeatureStats` says how often a feature fires, `ActHist` how strongly, `PosProfile` where in a row, `CoactStats` with which
other features.  `TokenProfile` says on which tokens: for F query features, per token of the vocabulary, how often the feature
fired on it and how strongly, from the top-k pairs and the `input_ids` the text cache already holds on the device
(msae_token_profile_update, include/msae.h).  Two uses: the "top tokens" panel of a feature and the list of SINGLE-TOKEN
features an interp or steering run may want to leave out (the reference's `unigram`, features/stats.py, over every position
instead of the top examples), and -- with the offsets +1 / -1 -- the distribution of the NEXT / PREVIOUS token at a feature's
firing positions, which `top_logits` can only approximate through the unembedding.

For the offsets o_0 .. o_{O-1} (distinct, in [-64, 64]) and the batch's token ids [B, S], an entry (v, f) at position (b, s)
is kept by the cache's rule (|v| > thresh, 0 <= f < N, no feature filter) and counted iff v > 0 (`PosProfile`'s rule):

    counts [O, F, V] int32     counts[a, i, t] = counted entries of queries[i] at positions with ids[b, s + o_a] == t
    mass   [O, F, V] int64     (mass=True) the sum of q(v), `PosProfile`'s fixed-point value, over them: unsigned, mod 2^64
    tok_count [O, V] int64     positions (b, s) with 0 <= s + o_a < S and ids[b, s + o_a] == t, whatever fired there
    n_rows, n_positions        Python ints

A token id outside [0, V) is counted nowhere and an offset never crosses a row.  All of it is exact integer arithmetic: the
state does not depend on how rows are cut into calls or ranks, or on the order of the calls, and two states of one kind (N, V,
the queries in order, the offsets, thresh, whether mass is kept) merge by addition."""
from __future__ import annotations

import ctypes
import hashlib
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _hip, ops
from . import _pooled
from ._pooled import _write_safetensors
from .coact import _query_list

FORMAT = "msae.token_profile.v1"
METRICS = {"count": 0, "precision": 1, "mean": 2}
MAX_OFFSETS, MAX_OFFSET, MAX_TOP = 4, 64, 64
MASS_ONE = 1 << 20                 # q(1.0)


@torch.library.custom_op("msae::token_profile_update", mutates_args=("counts", "mass", "tok_count"))
def token_profile_update(top_acts: Tensor, top_indices: Tensor, token_ids: Tensor, thresh: float, slot_of: Tensor,
                         offsets: List[int], counts: Tensor, mass: Tensor, tok_count: Tensor) -> None:
    """One batch of `[B, S, k]` top-k pairs and its `[B, S]` token ids into the profiles (in place, stream-ordered, no host
    read).  `mass` with no element: no mass is kept.  The list's indices and the ids go in as they are, 32 or 64 bits wide."""
    O, F, V = counts.shape
    assert counts.dtype == torch.int32 and counts.is_contiguous() and len(offsets) == O
    assert tok_count.dtype == torch.int64 and tok_count.shape == (O, V) and tok_count.is_contiguous()
    assert mass.dtype == torch.int64 and mass.is_contiguous() and (mass.numel() == 0 or mass.shape == counts.shape)
    assert slot_of.dtype == torch.int32 and slot_of.dim() == 1 and slot_of.is_contiguous()
    assert top_acts.dim() == 3 and top_acts.shape == top_indices.shape and token_ids.shape == top_acts.shape[:2]
    assert top_indices.dtype in (torch.int32, torch.int64) and token_ids.dtype in (torch.int32, torch.int64)
    dev = _hip.require_device(top_acts, top_indices, token_ids, slot_of, counts, mass, tok_count)
    lib = _hip.load()
    vals, idx, ids = ops._f32c(top_acts), top_indices.detach().contiguous(), token_ids.detach().contiguous()
    B, S, k = vals.shape
    wide = idx.dtype == torch.int64
    fn, name = ((lib.msae_token_profile_update_i64, "msae_token_profile_update_i64") if wide
                else (lib.msae_token_profile_update, "msae_token_profile_update"))
    offs = (ctypes.c_int32 * O)(*offsets)             # a host array: the entry reads it during the call
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(vals), _hip.ptr(idx), _hip.ptr(ids), 64 if ids.dtype == torch.int64 else 32, B, S, k, thresh,
                      slot_of.numel(), _hip.ptr(slot_of), F, V, offs, O, _hip.ptr(counts),
                      _hip.ptr(mass) if mass.numel() else None, _hip.ptr(tok_count), _hip.stream_of(vals)), name)


@token_profile_update.register_fake
def _(top_acts, top_indices, token_ids, thresh, slot_of, offsets, counts, mass, tok_count):
    return None


@torch.library.custom_op("msae::token_profile_topk", mutates_args=())
def token_profile_topk(counts: Tensor, mass: Tensor, tok_count: Tensor, m: int, metric: int,
                       min_count: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(values [F, m] f32, tokens [F, m] int32, totals [F] int64) of one offset plane: counts [F, V], mass [F, V] (or no
    element), tok_count [V]."""
    dev = _hip.require_device(counts, mass, tok_count)
    lib = _hip.load()
    F, V = counts.shape
    assert counts.dtype == torch.int32 and counts.is_contiguous()
    assert tok_count.dtype == torch.int64 and tok_count.shape == (V,) and tok_count.is_contiguous()
    assert mass.dtype == torch.int64 and mass.is_contiguous() and (mass.numel() == 0 or mass.shape == counts.shape)
    val = torch.empty(F, m, dtype=torch.float32, device=dev)
    tok = torch.empty(F, m, dtype=torch.int32, device=dev)
    tot = torch.empty(F, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_token_profile_topk(_hip.ptr(counts), _hip.ptr(mass) if mass.numel() else None, _hip.ptr(tok_count),
                                               F, V, m, metric, min_count, _hip.ptr(val), _hip.ptr(tok), _hip.ptr(tot),
                                               _hip.stream_of(counts)), "msae_token_profile_topk")
    return val, tok, tot


@token_profile_topk.register_fake
def _(counts, mass, tok_count, m, metric, min_count):
    F = counts.shape[0]
    return (counts.new_empty((F, m), dtype=torch.float32), counts.new_empty((F, m), dtype=torch.int32),
            counts.new_empty((F,), dtype=torch.int64))


def _unsigned_f64(t: Tensor) -> Tensor:
    """An int64 tensor read as unsigned, in float64, correctly rounded: both 32-bit halves are exact in f64 and so is the upper
    one times 2^32, so their sum is rounded once (the kernel's one conversion)."""
    hi, lo = (t >> 32) & 0xFFFFFFFF, t & 0xFFFFFFFF
    return hi.to(torch.float64) * 4294967296.0 + lo.to(torch.float64)


def top_tokens_host(counts: Tensor, mass: Optional[Tensor], tok_count: Tensor, m: int, metric: str, min_count: int,
                    rows_per_step: int = 64) -> Tuple[Tensor, Tensor, Tensor]:
    """`msae_token_profile_topk` in plain torch: the same integers, the same operation sequence per metric, the same order
    (a stable descending sort of the f32 score: ties stay by ascending token).  Over one offset plane."""
    counts, tok_count = counts.cpu(), tok_count.cpu()
    F, V = counts.shape
    val = torch.zeros(F, m, dtype=torch.float32)
    tok = torch.full((F, m), -1, dtype=torch.int32)
    tot = counts.sum(dim=1, dtype=torch.int64)
    take = min(m, V)
    for r0 in range(0, F, rows_per_step):
        c = counts[r0:r0 + rows_per_step]
        cand = c >= min_count
        if metric == "count":
            score = c.to(torch.float32)
        elif metric == "precision":
            score = (c.to(torch.float64) / tok_count.to(torch.float64)).to(torch.float32)
        else:
            score = (_unsigned_f64(mass[r0:r0 + rows_per_step].cpu()) / c.to(torch.float64) * 2.0 ** -20).to(torch.float32)
        score = torch.where(cand, score, torch.full_like(score, float("-inf")))      # a candidate's score is never -inf
        order = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :take]
        has = torch.arange(take)[None, :] < cand.sum(dim=1)[:, None]
        val[r0:r0 + rows_per_step, :take] = torch.where(has, torch.gather(score, 1, order), torch.zeros(()))
        tok[r0:r0 + rows_per_step, :take] = torch.where(has, order, torch.full_like(order, -1)).to(torch.int32)
    return val, tok, tot


def _offset_list(offsets) -> List[int]:
    offs = [int(o) for o in ([offsets] if isinstance(offsets, int) else offsets)]
    if not 1 <= len(offs) <= MAX_OFFSETS:
        raise ValueError(f"the number of offsets must lie in [1, {MAX_OFFSETS}], got {len(offs)}")
    if len(set(offs)) != len(offs):
        raise ValueError(f"offsets must be distinct, got {offs}")
    if min(offs) < -MAX_OFFSET or max(offs) > MAX_OFFSET:
        raise ValueError(f"offsets must lie in [{-MAX_OFFSET}, {MAX_OFFSET}], got {offs}")
    return offs


class TokenProfile:
    """Token profiles of `queries` (slot i = queries[i], order kept) over a vocabulary of `vocab_size` tokens; see the module
    docstring.  The counters live on `device`; `update` and the kernel path of `top_tokens` need a HIP device, everything else
    -- `merge`, `save`, and every reading of a loaded file, `top_tokens` included (the same bits from plain torch) -- does
    not."""

    def __init__(self, num_latents: int, queries, vocab_size: int, offsets: Sequence[int] = (0,), mass: bool = False,
                 thresh: float = 1e-5, device=None, max_bytes: int = 8 << 30):
        if not 0 < num_latents <= _pooled.MAX_LATENTS:
            raise ValueError(f"num_latents must lie in [1, {_pooled.MAX_LATENTS}], got {num_latents}")
        q = _query_list(queries, num_latents)
        offs = _offset_list(offsets)
        V, O, F = int(vocab_size), len(offs), len(q)
        if V < 1:
            raise ValueError(f"vocab_size must be positive, got {vocab_size}")
        if O * F * V >= 1 << 31:
            raise ValueError(f"{O} offsets x {F} queries x {V} tokens are {O * F * V} cells: a cell index holds fewer than 2^31")
        need = O * F * V * (12 if mass else 4) + O * V * 8
        if need > max_bytes:
            raise ValueError(f"{O} offsets x {F} queries x {V} tokens need {need} bytes of counters, more than "
                             f"max_bytes = {max_bytes}")
        self.num_latents, self.vocab_size, self.offsets, self.thresh = int(num_latents), V, tuple(offs), float(thresh)
        self.n_rows = self.n_positions = 0
        dev = torch.device("cpu") if device is None else torch.device(device)
        self.queries = torch.tensor(q, dtype=torch.int64, device=dev)
        self.counts = torch.zeros(O, F, V, dtype=torch.int32, device=dev)
        self.mass = torch.zeros(O, F, V, dtype=torch.int64, device=dev) if mass else None
        self.tok_count = torch.zeros(O, V, dtype=torch.int64, device=dev)
        self._slot_of: Optional[Tensor] = None
        self._no_mass: Optional[Tensor] = None

    @property
    def device(self) -> torch.device:
        return self.counts.device

    @property
    def num_queries(self) -> int:
        return self.counts.shape[1]

    @property
    def has_mass(self) -> bool:
        return self.mass is not None

    def _kind(self):
        return (self.num_latents, self.vocab_size, tuple(self.queries.cpu().tolist()), self.offsets, self.thresh, self.has_mass)

    def kind_hash(self) -> str:
        """sha256 over (N, V, the queries in order, the offsets, thresh, whether mass is kept): what two states must share."""
        N, V, q, offs, thresh, mass = self._kind()
        text = f"{N},{V},{thresh!r},{int(mass)};" + ",".join(map(str, offs)) + ";" + ",".join(map(str, q))
        return hashlib.sha256(text.encode()).hexdigest()

    def _mass_arg(self) -> Tensor:
        if self.mass is not None:
            return self.mass
        if self._no_mass is None or self._no_mass.device != self.device:
            self._no_mass = torch.empty(0, dtype=torch.int64, device=self.device)
        return self._no_mass

    def _slots(self) -> Tensor:
        if self._slot_of is None or self._slot_of.device != self.device:
            slot_of = torch.full((self.num_latents,), -1, dtype=torch.int32, device=self.device)
            slot_of[self.queries] = torch.arange(self.num_queries, dtype=torch.int32, device=self.device)
            self._slot_of = slot_of
        return self._slot_of

    def update(self, top_acts: Tensor, top_indices: Tensor, token_ids: Tensor) -> None:
        """Add one batch of `[B, S, k]` top-k pairs with its `[B, S]` token ids (int32 or int64; complete rows only).  Every
        limit is checked on the host, from the shapes alone, before any device work; nothing is read back.  Empty input is a
        no-op."""
        B, S, k = _pooled.topk_shape(top_acts, top_indices)
        if token_ids.dim() != 2 or tuple(token_ids.shape) != (B, S):
            raise ValueError(f"token_ids must be [B, S] = {(B, S)}, got {tuple(token_ids.shape)}")
        if token_ids.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"token_ids must be int32 or int64, got {token_ids.dtype}")
        if B * S * k == 0:
            return
        _pooled.check_call_limits(S, k)
        total = _pooled.total_segments(self.n_positions, B * S)
        _hip.require_device(top_acts, top_indices, token_ids, self.counts)
        if top_indices.dtype not in (torch.int32, torch.int64):
            top_indices = top_indices.to(torch.int64)
        slot_of, mass = self._slots(), self._mass_arg()
        for rows in _pooled.row_chunks(B, S):
            torch.ops.msae.token_profile_update(top_acts[rows], top_indices[rows], token_ids[rows], self.thresh, slot_of,
                                                list(self.offsets), self.counts, mass, self.tok_count)
        self.n_rows += B
        self.n_positions = total

    def merge(self, other: "TokenProfile") -> "TokenProfile":
        """self += other (another rank's profiles of the same kind), on self's device, in plain torch."""
        if self._kind() != other._kind():
            a, b = self._kind(), other._kind()
            raise ValueError("cannot merge token profiles of different kinds: "
                             f"{a[:2] + a[3:]} / kind {self.kind_hash()[:12]} vs {b[:2] + b[3:]} / kind {other.kind_hash()[:12]}")
        total = _pooled.total_segments(self.n_positions, other.n_positions)
        self.counts += other.counts.to(self.device)
        if self.mass is not None:
            self.mass += other.mass.to(self.device)           # int64 adds wrap: the unsigned sum mod 2^64
        self.tok_count += other.tok_count.to(self.device)
        self.n_rows += other.n_rows
        self.n_positions = total
        return self

    # ---- reading -------------------------------------------------------------------------------------------------
    def _plane(self, offset: int) -> int:
        if int(offset) not in self.offsets:
            raise ValueError(f"offset {offset} is not one of these profiles' offsets {self.offsets}")
        return self.offsets.index(int(offset))

    def _slot_rows(self, features) -> Optional[Tensor]:
        if features is None:
            return None
        want = features.detach().cpu().reshape(-1).tolist() if isinstance(features, Tensor) else [int(f) for f in features]
        slot = {q: i for i, q in enumerate(self.queries.cpu().tolist())}
        missing = [f for f in want if f not in slot]
        if missing:
            raise KeyError(f"features {missing[:8]} are not queries of these profiles")
        return torch.tensor([slot[f] for f in want], dtype=torch.int64, device=self.device)

    def row(self, feature: int, offset: int = 0) -> Tensor:
        """The counter row [V] of query `feature` in the plane of `offset`."""
        return self.counts[self._plane(offset), int(self._slot_rows([feature])[0])]

    def top_tokens(self, m: int = 10, by: str = "count", offset: int = 0, min_count: int = 1,
                   features=None) -> Tuple[Tensor, Tensor, Tensor]:
        """(values [F, m] f32, tokens [F, m] int32, totals [F] int64) per query (or per feature of `features`, each a query):
        the m best tokens with at least `min_count` fires in the plane of `offset`, by

            "count"      f32(c)
            "precision"  f32(f64(c) / f64(tok_count)): P(the feature fires at s | the token at s + offset)
            "mean"       f32(f64(mass, unsigned) / f64(c) * 2^-20): the mean strength (needs mass=True)

        in (score descending, token ascending) order -- the order of the f32 score, so counts above 2^24 that round to one
        float tie and the lower token comes first; a row with fewer candidates ends in free slots (0.0, -1).  `totals` is the
        row total of the counts.  The kernel on a HIP device, the same bits from plain torch anywhere else."""
        if by not in METRICS:
            raise ValueError(f"by must be one of {sorted(METRICS)}, got {by!r}")
        if by == "mean" and self.mass is None:
            raise ValueError("by='mean' needs profiles built with mass=True")
        if not 1 <= m <= MAX_TOP:
            raise ValueError(f"m must lie in [1, {MAX_TOP}], got {m}")
        if min_count < 1:
            raise ValueError(f"min_count must be at least 1, got {min_count}")
        a, rows = self._plane(offset), self._slot_rows(features)
        counts = self.counts[a] if rows is None else self.counts[a][rows]
        mass = None if self.mass is None else (self.mass[a] if rows is None else self.mass[a][rows])
        if not counts.is_cuda:
            return top_tokens_host(counts, mass, self.tok_count[a], m, by, int(min_count))
        if counts.shape[0] == 0:
            return (counts.new_empty((0, m), dtype=torch.float32), counts.new_empty((0, m), dtype=torch.int32),
                    counts.new_empty(0, dtype=torch.int64))
        return torch.ops.msae.token_profile_topk(counts, self._mass_arg() if mass is None else mass, self.tok_count[a], m,
                                                 METRICS[by], int(min_count))

    def single_token(self, share: float = 0.9, max_tokens: int = 1, offset: int = 0, min_fired: int = 1) -> Tensor:
        """int64 feature ids, in query order: the queries with at least `min_fired` fires (at positions whose token at `offset`
        lies in the vocabulary) of which at least `share` fall on their `max_tokens` most frequent tokens -- the single-token
        features.  In float64 from `top_tokens`' output."""
        val, _, tot = self.top_tokens(m=max_tokens, by="count", offset=offset)
        top = val.to(torch.float64).sum(dim=1).cpu()
        tot = tot.cpu()
        keep = (tot >= max(int(min_fired), 1)) & (top / tot.to(torch.float64) >= share)
        return self.queries.cpu()[keep]

    @staticmethod
    def decode(tokens, tokenizer) -> List[List[str]]:
        """Token strings of `top_tokens`' token ids, row by row (free slots left out): `tokenizer.convert_ids_to_tokens`."""
        rows = tokens.cpu().tolist() if isinstance(tokens, Tensor) else [list(r) for r in tokens]
        return [tokenizer.convert_ids_to_tokens([t for t in row if t >= 0]) for row in rows]

    # ---- file ----------------------------------------------------------------------------------------------------
    def metadata(self) -> dict:
        return {"format": FORMAT, "num_latents": str(self.num_latents), "vocab_size": str(self.vocab_size),
                "offsets": ",".join(str(o) for o in self.offsets), "mass": str(int(self.has_mass)), "thresh": repr(self.thresh),
                "kind": self.kind_hash(), "n_rows": str(self.n_rows), "n_positions": str(self.n_positions)}

    def save(self, path: str) -> None:
        """queries, tok_count and the NONZERO cells: cell_key int64 = (a * F + slot) * V + token (ascending), cell_count int32
        and, with mass, cell_mass int64.  Equal state, equal bytes."""
        flat = self.counts.reshape(-1)
        used = flat != 0
        if self.mass is not None:
            used |= self.mass.reshape(-1) != 0
        key = used.nonzero().reshape(-1)
        tensors = {"queries": self.queries, "tok_count": self.tok_count, "cell_key": key, "cell_count": flat[key]}
        if self.mass is not None:
            tensors["cell_mass"] = self.mass.reshape(-1)[key]
        _write_safetensors({k: v.detach().contiguous().cpu() for k, v in tensors.items()}, path, self.metadata())

    @classmethod
    def load(cls, path: str, device=None, max_bytes: int = 8 << 30) -> "TokenProfile":
        meta, tensors = _pooled.open_stats_file(path, FORMAT, "a token profile")
        st = cls(int(meta["num_latents"]), tensors["queries"], int(meta["vocab_size"]),
                 offsets=[int(o) for o in meta["offsets"].split(",")], mass=meta["mass"] == "1", thresh=float(meta["thresh"]),
                 device=device, max_bytes=max_bytes)
        if st.kind_hash() != meta["kind"]:
            raise ValueError(f"{path}: the kind {meta['kind'][:12]} does not match the file's parameters")
        if tensors["tok_count"].shape != st.tok_count.shape or tensors["tok_count"].dtype != torch.int64:
            raise ValueError(f"{path}: tok_count is {tuple(tensors['tok_count'].shape)}, expected {tuple(st.tok_count.shape)}")
        key = tensors["cell_key"].to(st.device)
        if key.numel() and (int(key.min()) < 0 or int(key.max()) >= st.counts.numel()):
            raise ValueError(f"{path}: a cell key lies outside the {st.counts.numel()} cells")
        st.counts.reshape(-1)[key] = tensors["cell_count"].to(st.device)
        if st.mass is not None:
            st.mass.reshape(-1)[key] = tensors["cell_mass"].to(st.device)
        st.tok_count.copy_(tensors["tok_count"])
        st.n_rows, st.n_positions = int(meta["n_rows"]), int(meta["n_positions"])
        return st
