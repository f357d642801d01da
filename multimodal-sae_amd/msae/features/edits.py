"""FeatureEdits -- a set of latent edits for one encode: clamp some features to values, ablate others.

The reference's hooks edit the dense latents with torch indexing, so the feature may be a list or tensor:

    steering     latents[:, :, f] = clamp            features/steering.py:113-114
    attribution  mask[:, off_features] = 0           features/patching/utils.py:43-48

`Sae.encode(x, edits=FeatureEdits(...))` applies such a set without the dense [T, N] latents: the unedited fused encode
over-fetches k + E entries per token and `ops.edit_topk` (csrc/edit_topk.hip) drops the edited features from each list,
adds the edits' own (value, feature) pairs and re-ranks -- exact, DESIGN.md section 7d.  Beside SET and ZERO an entry
may SCALE, ADD to, FLOOR or CAP the feature's own latent (section 7p): the encode then passes the edited features' exact
latents (`ops.pre_acts_features`) to the same kernels' valued form.

Everything host-side happens ONCE, here: range checks, duplicates, the merge of the two lists (a feature in both is
zeroed: the oracle applies set, then zero), the sort, and one upload of the three device arrays.  Afterwards nothing is
read back, so an encode with a prebuilt object is stream-ordered like every other op.
"""
from __future__ import annotations

from typing import Iterable, Mapping, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

EDIT_SET, EDIT_ZERO = 0, 1          # include/msae.h: MSAE_EDIT_SET / MSAE_EDIT_ZERO
EDIT_SCALE, EDIT_ADD, EDIT_FLOOR, EDIT_CAP = 2, 3, 4, 5     # MSAE_EDIT_SCALE ..: functions of the feature's own latent
VALUE_KINDS = {"scale": EDIT_SCALE, "add": EDIT_ADD, "floor": EDIT_FLOOR, "cap": EDIT_CAP}
EDIT_MODES = ("set",) + tuple(VALUE_KINDS)                  # the hooks' `mode`
MAX_SELECTED = 4096                 # k + E: msae_encode_topk's own limit on k


def _int_list(features, what: str) -> list:
    if isinstance(features, Tensor):
        if features.dtype.is_floating_point or features.dtype == torch.bool:
            raise ValueError(f"FeatureEdits: {what} features must be integers, got {features.dtype}")
        features = features.detach().reshape(-1).cpu().tolist()
    elif isinstance(features, np.ndarray):
        if features.dtype.kind not in "iu":
            raise ValueError(f"FeatureEdits: {what} features must be integers, got {features.dtype}")
        features = features.reshape(-1).tolist()
    elif isinstance(features, (int, np.integer)):
        features = [features]
    out = []
    for f in features:
        if isinstance(f, (bool, float)) or not isinstance(f, (int, np.integer)):
            raise ValueError(f"FeatureEdits: {what} features must be integers, got {f!r}")
        out.append(int(f))
    return out


def _float_list(values) -> list:
    if isinstance(values, Tensor):
        values = values.detach().reshape(-1).float().cpu().tolist()
    elif isinstance(values, np.ndarray):
        values = values.reshape(-1).tolist()
    return [float(v) for v in values]


def _valued_pairs(spec, what: str) -> Tuple[list, list]:
    """A mapping feature -> parameter, or a (features, values) pair -> (features, values) of one length."""
    if isinstance(spec, Mapping):
        feats, vals = _int_list(list(spec.keys()), what), _float_list(list(spec.values()))
    else:
        try:
            f_in, v_in = spec
        except (TypeError, ValueError):
            raise ValueError(f"FeatureEdits: {what} must be a mapping feature -> value or a (features, values) pair") from None
        feats, vals = _int_list(f_in, what), _float_list(v_in)
    if len(feats) != len(vals):
        raise ValueError(f"FeatureEdits: {what} has {len(feats)} features and {len(vals)} values")
    return feats, vals


class FeatureEdits:
    """FeatureEdits(num_latents, set=None, zero=None, device="cuda", scale=None, add=None, floor=None, cap=None)

    set   a mapping feature -> value, or a (features, values) pair of equal-length sequences / tensors
    zero  an int, or any iterable / tensor of features
    scale / add / floor / cap   like `set`; the parameter v of an edit that depends on the feature's own latent c:
          c * v, c + v, max(c, v), min(c, v) -- amplify a feature where it fires, instead of
          lighting it up at every position
    A feature named in `zero` and anywhere else is zeroed.  Errors (ValueError): a feature outside [0, num_latents), a
    feature twice among set / scale / add / floor / cap (inside one of them or across two), a non-finite value, nothing to
    edit, more than 4095 distinct features.  Duplicates inside `zero` are harmless (the reference's
    `mask[:, off_features] = 0` accepts them) and collapse.

    Attributes: E (distinct edited features), features (their sorted tuple), num_latents, device; the device arrays
    feat / val / kind [E] that ops.edit_topk takes; value_dependent (does any entry need the feature's latent?); mask (bool
    [num_latents], True at every edited feature, built on the device at first use: the backward of the differentiable
    encode masks those latents' gradients)."""

    def __init__(self, num_latents: int, set: Union[Mapping, Tuple, None] = None, zero: Optional[Iterable] = None,
                 device: Union[str, torch.device] = "cuda", scale: Union[Mapping, Tuple, None] = None,
                 add: Union[Mapping, Tuple, None] = None, floor: Union[Mapping, Tuple, None] = None,
                 cap: Union[Mapping, Tuple, None] = None):
        self.num_latents = int(num_latents)
        table, named = {}, {}
        for what, kind, spec in (("set", EDIT_SET, set), ("scale", EDIT_SCALE, scale), ("add", EDIT_ADD, add),
                                 ("floor", EDIT_FLOOR, floor), ("cap", EDIT_CAP, cap)):
            if spec is None:
                continue
            for f, v in zip(*_valued_pairs(spec, what)):
                if f in table:
                    raise ValueError(f"FeatureEdits: feature {f} appears twice in {what}" if named[f] == what else
                                     f"FeatureEdits: feature {f} appears in both {named[f]} and {what}")
                if not np.isfinite(v):
                    raise ValueError(f"FeatureEdits: {what} value of feature {f} is not finite ({v})")
                table[f], named[f] = (kind, v), what
        if zero is not None:
            for f in _int_list(zero, "zero"):
                table[f] = (EDIT_ZERO, 0.0)                      # ZERO over everything else
        if not table:
            raise ValueError("FeatureEdits: nothing to edit (every argument is empty)")
        bad = [f for f in table if not 0 <= f < self.num_latents]
        if bad:
            raise ValueError(f"FeatureEdits: features must lie in [0, {self.num_latents}), got {sorted(bad)[:8]}")
        if len(table) >= MAX_SELECTED:
            raise ValueError(f"FeatureEdits: {len(table)} edited features; k + E <= {MAX_SELECTED} is the encoder's limit")
        self.features = tuple(sorted(table))
        self.E = len(self.features)
        self.kinds = tuple(table[f][0] for f in self.features)       # host copies: tests, repr
        self.values = tuple(table[f][1] for f in self.features)
        self.value_dependent = any(kd >= EDIT_SCALE for kd in self.kinds)
        # one buffer, one copy: int32 [3, E] = features, value bits, kinds
        host = np.empty((3, self.E), dtype=np.int32)
        host[0] = self.features
        host[1] = np.asarray(self.values, dtype=np.float32).view(np.int32)
        host[2] = self.kinds
        self.device = torch.device(device)
        buf = torch.from_numpy(host)
        if self.device.type == "cuda":
            buf = buf.pin_memory().to(self.device, non_blocking=True)
        self._buf = buf
        self.feat, self.val, self.kind = buf[0], buf[1].view(torch.float32), buf[2]
        self._mask: Optional[Tensor] = None

    @property
    def mask(self) -> Tensor:
        if self._mask is None:
            m = torch.zeros(self.num_latents, dtype=torch.bool, device=self.device)
            m[self.feat.long()] = True
            self._mask = m
        return self._mask

    def check(self, num_latents: int, k: int, device=None) -> None:
        """Raise ValueError unless this object fits an encode of `num_latents` features selecting k."""
        if self.num_latents != num_latents:
            raise ValueError(f"FeatureEdits was built for num_latents = {self.num_latents}, the Sae has {num_latents}")
        if k + self.E > min(num_latents, MAX_SELECTED):
            raise ValueError(f"k + E = {k} + {self.E} exceeds min(num_latents, {MAX_SELECTED}) = "
                             f"{min(num_latents, MAX_SELECTED)}")
        if device is not None:
            want, have = torch.device(device), self.feat.device
            if want.type != have.type or (want.index is not None and have.index is not None and want.index != have.index):
                raise ValueError(f"FeatureEdits lives on {have}, the encode runs on {want}")

    def __len__(self) -> int:
        return self.E

    def __repr__(self) -> str:
        n_zero = sum(1 for kd in self.kinds if kd == EDIT_ZERO)
        n_dep = sum(1 for kd in self.kinds if kd >= EDIT_SCALE)
        return (f"FeatureEdits(num_latents={self.num_latents}, E={self.E}: {self.E - n_zero - n_dep} set, {n_zero} zero" +
                (f", {n_dep} value-dependent)" if n_dep else ")"))


class RowEdits:
    """RowEdits(num_latents, groups, device="cuda") -- one edit table PER GROUP of tokens for one encode: B features steered
    in the B rows of one `generate`, G ablations in the G copies of one attribution batch.

    groups  a sequence; element g is a FeatureEdits, a dict(set=..., zero=...) spec (FeatureEdits' arguments and rules), or
            None: an empty group, whose tokens stay unedited -- it keeps its index, so "row b uses group b" holds.
    `Sae.encode(x, edits=RowEdits, edit_group=...)` names every token's group; an id outside [0, G) is unedited as well.

    Everything host-side happens ONCE, here: each group's validation (FeatureEdits), the concatenation, the offsets and ONE
    pinned upload of one int32 buffer.  Errors (ValueError): whatever FeatureEdits raises for a group, a group built for
    another num_latents, an element of another type, no group at all, every group empty.

    Attributes: G, E_max (the longest group), E_total, num_latents, device, tables (host copy: per group a
    (features, values, kinds) triple of tuples, features ascending); the device arrays offsets int32 [G + 1], feat int32 / val f32 / kind int32 [E_total] that
    ops.edit_topk_rows takes.  A spec also takes FeatureEdits' scale / add / floor / cap; for those entries: value_dependent,
    union (int32 device tensor: the sorted distinct features of the value-dependent entries of all groups -- the columns of
    the one ops.pre_acts_features pass an encode runs) and col (int32 [E_total]: each entry's position in union, 0 for an
    entry that reads no latent)."""

    def __init__(self, num_latents: int, groups, device: Union[str, torch.device] = "cuda"):
        self.num_latents = int(num_latents)
        if isinstance(groups, (FeatureEdits, Mapping)) or not hasattr(groups, "__len__"):
            raise ValueError("RowEdits: groups must be a sequence of FeatureEdits, dict(set=..., zero=...) specs or None")
        feats, vals, kinds, offsets = [], [], [], [0]
        for g, spec in enumerate(groups):
            if spec is None:
                fe = None
            elif isinstance(spec, FeatureEdits):
                if spec.num_latents != self.num_latents:
                    raise ValueError(f"RowEdits: group {g} was built for num_latents = {spec.num_latents}, not {self.num_latents}")
                fe = spec
            elif isinstance(spec, Mapping):
                if not set(spec) <= {"set", "zero", *VALUE_KINDS}:
                    raise ValueError(f"RowEdits: group {g}: a spec has the keys 'set', 'zero', 'scale', 'add', 'floor' and "
                                     f"'cap', got {sorted(map(str, spec))}")
                fe = FeatureEdits(self.num_latents, device="cpu", **{key: spec.get(key) for key in spec})
            else:
                raise ValueError(f"RowEdits: group {g} must be a FeatureEdits, a dict(set=..., zero=...) or None, got "
                                 f"{type(spec).__name__}")
            if fe is not None:                      # host copies only: a FeatureEdits on the device is not read back
                feats += fe.features
                vals += fe.values
                kinds += fe.kinds
            offsets.append(len(feats))
        self.G = len(offsets) - 1
        if self.G < 1 or not feats:
            raise ValueError("RowEdits: nothing to edit (no group, or every group is empty)")
        self.E_total = len(feats)
        self.E_max = max(b - a for a, b in zip(offsets[:-1], offsets[1:]))
        self.tables = tuple((tuple(feats[a:b]), tuple(vals[a:b]), tuple(kinds[a:b])) for a, b in zip(offsets[:-1], offsets[1:]))
        # the value-dependent entries' features, once each: the columns of the one `cur` pass an encode runs for all groups
        union = sorted({f for f, kd in zip(feats, kinds) if kd >= EDIT_SCALE})
        where = {f: c for c, f in enumerate(union)}
        self.value_dependent = bool(union)
        # one buffer, one copy: int32 [G + 1 + 4 E_total + U] = offsets, features, value bits, kinds, columns, union
        G1, E, U = self.G + 1, self.E_total, len(union)
        host = np.empty(G1 + 4 * E + U, dtype=np.int32)
        host[:G1] = offsets
        host[G1:G1 + E] = feats
        host[G1 + E:G1 + 2 * E] = np.asarray(vals, dtype=np.float32).view(np.int32)
        host[G1 + 2 * E:G1 + 3 * E] = kinds
        host[G1 + 3 * E:G1 + 4 * E] = [where[f] if kd >= EDIT_SCALE else 0 for f, kd in zip(feats, kinds)]
        host[G1 + 4 * E:] = union
        self.device = torch.device(device)
        buf = torch.from_numpy(host)
        if self.device.type == "cuda":
            buf = buf.pin_memory().to(self.device, non_blocking=True)
        self._buf = buf
        self.offsets, self.feat, self.kind = buf[:G1], buf[G1:G1 + E], buf[G1 + 2 * E:G1 + 3 * E]
        self.val = buf[G1 + E:G1 + 2 * E].view(torch.float32)
        self.col, self.union = buf[G1 + 3 * E:G1 + 4 * E], buf[G1 + 4 * E:]

    def check(self, num_latents: int, k: int, device=None) -> None:
        """Raise ValueError unless this object fits an encode of `num_latents` features selecting k."""
        if self.num_latents != num_latents:
            raise ValueError(f"RowEdits was built for num_latents = {self.num_latents}, the Sae has {num_latents}")
        if k + self.E_max > min(num_latents, MAX_SELECTED):
            raise ValueError(f"k + E_max = {k} + {self.E_max} exceeds min(num_latents, {MAX_SELECTED}) = "
                             f"{min(num_latents, MAX_SELECTED)}")
        if device is not None:
            want, have = torch.device(device), self.feat.device
            if want.type != have.type or (want.index is not None and have.index is not None and want.index != have.index):
                raise ValueError(f"RowEdits lives on {have}, the encode runs on {want}")

    def __len__(self) -> int:
        return self.G

    def __repr__(self) -> str:
        return f"RowEdits(num_latents={self.num_latents}, G={self.G}, E_max={self.E_max}, E_total={self.E_total})"


def as_off_features(off_features, sae) -> Tuple[int, Optional[FeatureEdits]]:
    """The attribution hooks' `off_features` (None, an int, a sequence or a tensor: what `mask[:, off_features] = 0`
    takes) -> (zero_feature for the in-kernel scalar route, or -1; FeatureEdits on `sae`'s device for the list route, or
    None).  `sae` is only looked at for a list: a feature-sharded engine takes the scalar route alone."""
    if off_features is None:
        return -1, None
    if isinstance(off_features, (FeatureEdits, RowEdits)):
        return -1, off_features
    if isinstance(off_features, (int, np.integer)) and not isinstance(off_features, bool):
        return int(off_features), None
    if isinstance(off_features, Tensor) and off_features.dim() == 0:
        return int(off_features), None
    feats = _int_list(off_features, "zero")
    if not feats:                                   # `mask[:, []] = 0` edits nothing
        return -1, None
    if not hasattr(sae, "encoder"):
        raise NotImplementedError("ablating a set of features runs on the single-GPU msae.Sae only: a feature-sharded "
                                  "engine takes one feature")
    return -1, FeatureEdits(sae.num_latents, zero=feats, device=sae.encoder.weight.device)
