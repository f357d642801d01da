"""Numpy restatement of value-dependent latent edits (include/msae.h, "value-dependent edits").

The definition, on the DENSE latents L = oracle.pre_acts(x): with c = L[t][f] and v the entry's parameter

    SET v        ZERO +0        SCALE c * v        ADD c + v        FLOOR max(c, v)        CAP min(c, v)

each ONE float32 operation, then the canonical top-k (value descending, index ascending) by lexsort, as
edits_ref.dense_topk does through oracle.topk; and the gain dL'/dL * [c > 0] of every selected slot, 1 for a feature the
table does not name.

`wrong_variants` holds four plausible mis-statements; tests/test_value_edits_host.py shows that the planted cases tell each of them
from the definition, so a kernel that implemented one would fail the GPU tests built on the same cases.
"""
from __future__ import annotations

import numpy as np

SET, ZERO, SCALE, ADD, FLOOR, CAP = 0, 1, 2, 3, 4, 5
KINDS = {"set": SET, "scale": SCALE, "add": ADD, "floor": FLOOR, "cap": CAP}


def merge(set=None, zero=None, scale=None, add=None, floor=None, cap=None):
    """FeatureEdits' arguments -> (features int32 [E] ascending, values f32 [E], kinds int32 [E]); ZERO over everything; a
    feature in two of the other lists is an error."""
    table = {}
    for name, spec in (("set", set), ("scale", scale), ("add", add), ("floor", floor), ("cap", cap)):
        if spec is None:
            continue
        items = list(spec.items()) if hasattr(spec, "items") else list(zip(*spec))
        for f, v in items:
            assert int(f) not in table, f"feature {f} twice"
            table[int(f)] = (KINDS[name], np.float32(v))
    for f in (zero if zero is not None else ()):
        table[int(f)] = (ZERO, np.float32(0.0))
    feats = np.array(sorted(table), dtype=np.int32)
    return (feats, np.array([table[int(f)][1] for f in feats], dtype=np.float32),
            np.array([table[int(f)][0] for f in feats], dtype=np.int32))


def edit_column(c, v, kind):
    """L'[:, f] from c = L[:, f] (f32 [T]) with float32 scalar operations; a kind outside [0, 5] reads as SET."""
    c, v = np.asarray(c, dtype=np.float32), np.float32(v)
    if kind == ZERO:
        return np.zeros_like(c)
    if kind == SCALE:
        return (c * v).astype(np.float32)
    if kind == ADD:
        return (c + v).astype(np.float32)
    if kind == FLOOR:
        return np.maximum(c, v)
    if kind == CAP:
        return np.minimum(c, v)
    return np.full_like(c, v)


def gain_column(c, v, kind):
    """dL'/dL * [c > 0] (torch.clamp's convention at the tie)."""
    c, v = np.asarray(c, dtype=np.float32), np.float32(v)
    on = c > 0
    if kind == SCALE:
        return np.where(on, v, np.float32(0)).astype(np.float32)
    if kind == ADD:
        return on.astype(np.float32)
    if kind == FLOOR:
        return (on & (c >= v)).astype(np.float32)
    if kind == CAP:
        return (on & (c <= v)).astype(np.float32)
    return np.zeros_like(c)


def apply_dense(latents, feats, vals, kinds):
    """(L' f32 [T, N], gain f32 [T, N]: 1 at every feature the table does not name)."""
    out = np.array(latents, dtype=np.float32, copy=True)
    gain = np.ones_like(out)
    for f, v, kd in zip(feats, vals, kinds):
        c = np.asarray(latents[:, int(f)], dtype=np.float32)
        out[:, int(f)] = edit_column(c, v, int(kd))
        gain[:, int(f)] = gain_column(c, v, int(kd))
    return out, gain


def canonical_topk(latents, k):
    """Top-k of every row by lexsort: value descending (-0 == +0), index ascending.  Selected values of -0 come back as +0,
    as the library's rank key returns them."""
    latents = np.asarray(latents, dtype=np.float32)
    T, n = latents.shape
    vals = np.empty((T, k), dtype=np.float32)
    idx = np.empty((T, k), dtype=np.int32)
    for t in range(T):
        o = np.lexsort((np.arange(n), -latents[t].astype(np.float64)))[:k]
        idx[t] = o
        vals[t] = latents[t, o] + np.float32(0.0)          # -0 + +0 = +0
    return vals, idx


def dense_topk(latents, k, feats, vals, kinds, edit=apply_dense):
    """-> (vals f32 [T, k], idx int32 [T, k], gain f32 [T, k]) of the edited dense latents."""
    out, gain = edit(latents, feats, vals, kinds)
    v, i = canonical_topk(out, k)
    return v, i, np.take_along_axis(gain, i.astype(np.int64), 1)


def dense_topk_rows(latents, k, group_of, tables):
    """One table per token: tables[g] = (feats, vals, kinds) or None; a group id outside [0, G) or an empty group is
    unedited (gain 1)."""
    T = latents.shape[0]
    v, i = canonical_topk(latents, k)
    g = np.ones((T, k), dtype=np.float32)
    for t in range(T):
        gid = int(group_of[t])
        if 0 <= gid < len(tables) and tables[gid] is not None and len(tables[gid][0]):
            v[t:t + 1], i[t:t + 1], g[t:t + 1] = dense_topk(latents[t:t + 1], k, *tables[gid])
    return v, i, g


# ---- four wrong variants ------------------------------------------------------------------------------------------------
def _wrong_current_from_list(k):
    """The current value taken from the token's top-(k + E) list, 0 if the feature is not in it."""
    def edit(latents, feats, vals, kinds):
        E = len(feats)
        lv, li = canonical_topk(latents, k + E)
        seen = np.zeros_like(np.asarray(latents, dtype=np.float32))
        np.put_along_axis(seen, li.astype(np.int64), lv, 1)
        out, gain = apply_dense(seen, feats, vals, kinds)
        keep = np.array(latents, dtype=np.float32, copy=True)
        keep[:, feats] = out[:, feats]
        full = np.ones_like(keep)
        full[:, feats] = gain[:, feats]
        return keep, full
    return edit


def _wrong_gain_without_relu(latents, feats, vals, kinds):
    """The gain without [c > 0]."""
    out, gain = apply_dense(latents, feats, vals, kinds)
    for f, v, kd in zip(feats, vals, kinds):
        c = np.asarray(latents[:, int(f)], dtype=np.float32)
        if kd == SCALE:
            gain[:, int(f)] = v
        elif kd == ADD:
            gain[:, int(f)] = 1
        elif kd == FLOOR:
            gain[:, int(f)] = c >= v
        elif kd == CAP:
            gain[:, int(f)] = c <= v
    return out, gain


def _wrong_scale_before_relu(pre):
    """SCALE applied to the pre-ReLU value, the ReLU afterwards (differs for a negative factor, and in nothing else)."""
    def edit(latents, feats, vals, kinds):
        out, gain = apply_dense(latents, feats, vals, kinds)
        for f, v, kd in zip(feats, vals, kinds):
            if kd == SCALE:
                out[:, int(f)] = np.maximum((np.asarray(pre[:, int(f)], dtype=np.float32) * np.float32(v)), np.float32(0))
        return out, gain
    return edit


def _wrong_floor_as_set(latents, feats, vals, kinds):
    """FLOOR written as SET."""
    kinds = np.where(np.asarray(kinds) == FLOOR, SET, kinds)
    return apply_dense(latents, feats, vals, kinds)


def wrong_variants(k, pre):
    """name -> edit function for dense_topk(..., edit=); `pre`: the pre-ReLU activations of the same tokens."""
    return {"current value from the list": _wrong_current_from_list(k), "gain without [c > 0]": _wrong_gain_without_relu,
            "scale before the relu": _wrong_scale_before_relu(pre), "floor as set": _wrong_floor_as_set}


# ---- the planted cases ------------------------------------------------------------------------------------------------------
def plan(L, order, k, E, seed=0, special=(4000, 17, 900, 5000)):
    """FeatureEdits keyword arguments with E distinct features, planted relative to token 0's ranking (order[0]) in priority
    order -- the first is the case a kernel without `cur` must fail -- then `special` (the degenerate rows' own positives:
    features 4000, 17, 900, 5000 of the GPU tests' inputs), a SET and a ZERO, and a seeded random fill over all six kinds."""
    n = L.shape[1]
    o0 = order[0]
    v = lambda r: float(L[0, o0[r]])
    far = int(o0[k + E + 5])
    assert v(k + E + 5) > 0 and v(k - 1) > 0, "token 0 needs more than k + E + 5 active features"
    inactive = [int(f) for f in o0[::-1][:8] if L[0, f] == 0]
    assert len(inactive) >= 2
    picks = [("scale", far, 2.0 * v(0) / v(k + E + 5)),                     # beyond rank k + E, small and positive: enters
             ("add", inactive[0], v(min(1, k - 1))),                       # inactive under ADD: enters with delta itself
             ("scale", inactive[1], -1.0e6),                               # inactive under SCALE: 0 * v stays out
             ("add", int(o0[0]), -2.0 * v(0)),                             # a selected feature driven below 0: dropped
             ("cap", int(o0[min(1, k - 1)]), 0.5 * v(k - 1)),              # CAP below the k-th value
             ("floor", int(o0[min(2, k - 1)]), 0.5 * v(min(2, k - 1))),    # FLOOR below the current value: bits unchanged
             ("floor", int(o0[k + 1]), v(min(3, k - 1))),                  # FLOOR exactly equal to a selected value
             ("set", int(o0[k]), v(0)), ("zero", int(o0[k + 2]), None)]
    picks[7:7] = list(zip(("scale", "cap", "add", "floor"), special, (3.0, 0.1, -0.05, 2.0)))
    rng = np.random.default_rng(1000 * k + E + seed)
    names = ("scale", "zero", "add", "set", "floor", "cap")
    for j, f in enumerate(rng.permutation(n)[:E + 16]):
        name = names[j % 6]
        par = {"scale": rng.uniform(-1.0, 4.0), "add": rng.uniform(-1.0, 1.0) * v(0), "zero": 0.0}.get(
            name, rng.uniform(0.0, 2.0) * v(k - 1))
        picks.append((name, int(f), float(par)))
    kw, used = {}, set()
    for name, f, par in picks:
        if len(used) >= E:
            break
        if f in used:
            continue
        used.add(f)
        if name == "zero":
            kw.setdefault("zero", []).append(f)
        else:
            kw.setdefault(name, {})[f] = float(np.float32(par))
    return kw


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
