"""Numpy restatement of set-valued latent edits (include/msae.h, "set-valued hook edits").

Two independent statements of the same result:

  dense_*   the definition: dense latents from oracle.pre_acts, `L[:, f] = v` for SET edits, `L[:, f] = +0` for ZERO edits
            (ZERO wins where a feature is in both lists: oracle/sae_oracle.c applies set, then zero), oracle.topk.
  list_*    the rule the HIP kernel implements on an unedited top-(k + E) list: drop the entries of edited features,
            append the edits' own (value, feature) pairs, sort by the library's 64-bit rank key, keep k.

tests/test_edits_host.py shows that the two agree; tests/test_gpu_edits.py holds the HIP path to them bit for bit.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle

SET, ZERO = 0, 1


def merge(set_edits=None, zero=None):
    """(set: mapping feature -> value or (features, values); zero: iterable) -> (features int32 [E] ascending,
    values f32 [E], kinds int32 [E]); ZERO over SET; a duplicate inside `set` is an error."""
    table = {}
    if set_edits is not None:
        items = list(set_edits.items()) if hasattr(set_edits, "items") else list(zip(*set_edits))
        for f, v in items:
            assert int(f) not in table, f"feature {f} twice in set"
            table[int(f)] = (SET, np.float32(v))
    for f in (zero if zero is not None else ()):
        table[int(f)] = (ZERO, np.float32(0.0))
    feats = np.array(sorted(table), dtype=np.int32)
    return (feats, np.array([table[int(f)][1] for f in feats], dtype=np.float32),
            np.array([table[int(f)][0] for f in feats], dtype=np.int32))


def apply_dense(latents, feats, vals, kinds):
    """A copy of latents [T, N] with the merged edit table applied."""
    out = np.array(latents, dtype=np.float32, copy=True)
    for f, v, kd in zip(feats, vals, kinds):
        out[:, int(f)] = np.float32(0.0) if kd == ZERO else v
    return out


def dense_topk(latents, k, feats, vals, kinds):
    """Canonical top-k of the edited dense latents -> (vals f32 [T, k], idx int32 [T, k])."""
    return oracle.topk(apply_dense(latents, feats, vals, kinds), k)


def dense_encode(x, W_enc, b_enc, b_dec, k, set_edits=None, zero=None):
    """pre_acts -> edit -> topk: the definition of Sae.encode(x, edits=...)."""
    return dense_topk(oracle.pre_acts(np.asarray(x, dtype=np.float32), W_enc, b_enc, b_dec), k, *merge(set_edits, zero))


# ---- the list-level rule ---------------------------------------------------------------------------------------------
def order_key(v):
    """csrc/common.h f32_order_key: an order-preserving map f32 -> u32 with -0 folded onto +0."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def value_of_order_key(key):
    key = np.asarray(key, dtype=np.uint32)
    b = np.where((key & np.uint32(0x80000000)) != 0, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)
    return b.view(np.float32)


def rank_key(v, idx):
    """csrc/common.h rank_key: value descending, then index ascending  <=>  key descending."""
    return (order_key(v).astype(np.uint64) << np.uint64(32)) | (np.uint64(0x7FFFFFFF) - np.asarray(idx).astype(np.uint64))


def list_edit(vals_in, idx_in, k, feats, vals, kinds):
    """[T, kk] unedited canonical list (kk >= k + E) -> the edited latents' top-k by the list rule.  Reads the first k + E
    entries of every row only."""
    vals_in, idx_in = np.asarray(vals_in, dtype=np.float32), np.asarray(idx_in)
    T, kk = vals_in.shape
    E = len(feats)
    assert kk >= k + E and E >= 1
    edit_keys = rank_key(np.where(kinds == ZERO, np.float32(0.0), vals).astype(np.float32), feats)
    out_v = np.empty((T, k), dtype=np.float32)
    out_i = np.empty((T, k), dtype=np.int32)
    for t in range(T):
        v, i = vals_in[t, :k + E], idx_in[t, :k + E]
        keep = ~np.isin(i, feats)
        keys = np.concatenate([rank_key(v[keep], i[keep]), edit_keys])
        keys = np.sort(keys)[::-1][:k]
        out_v[t] = value_of_order_key((keys >> np.uint64(32)).astype(np.uint32))
        out_i[t] = (np.uint64(0x7FFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int32)
    return out_v, out_i


def list_encode(x, W_enc, b_enc, b_dec, k, set_edits=None, zero=None, extra=0):
    """Over-fetch (oracle.encode_topk with k + E + extra and no edit), then the list rule."""
    feats, vals, kinds = merge(set_edits, zero)
    v, i = oracle.encode_topk(np.asarray(x, dtype=np.float32), W_enc, b_enc, b_dec, k + len(feats) + extra)
    return list_edit(v, i, k, feats, vals, kinds)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
