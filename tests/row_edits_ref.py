"""Numpy restatement of PER-TOKEN latent edits (include/msae.h, "per-token edit tables"), built on
tests/edits_ref.py.  Token t applies the table of group group_of[t]; an id outside [0, G) or an empty group leaves it alone.

  dense_topk_rows   the definition: each token's table applied to its dense row, then oracle.topk.
  list_edit_rows    the rule the HIP kernel implements per token on an unedited top-kk list (kk >= k + E_max): the list
                    rule of edits_ref.list_edit with that token's table over its first k + E_g entries; an unedited token
                    keeps its first k entries.

tests/test_row_edits_host.py shows that the two agree; tests/test_gpu_row_edits.py holds the HIP path to the first.
"""
from __future__ import annotations

import numpy as np

import edits_ref as eref
from oracle import oracle


def merge_groups(specs):
    """[dict(set=..., zero=...) | None, ...] -> [(feats, vals, kinds) | None, ...] (edits_ref.merge per group)."""
    return [None if s is None else eref.merge(s.get("set"), s.get("zero")) for s in specs]


def table_of(groups, g):
    """The merged table of group id g, or None where the token is unedited (id outside [0, G), empty group)."""
    if not 0 <= int(g) < len(groups):
        return None
    tab = groups[int(g)]
    return None if tab is None or len(tab[0]) == 0 else tab


def apply_dense_rows(latents, groups, group_of):
    out = np.array(latents, dtype=np.float32, copy=True)
    for t, g in enumerate(np.asarray(group_of).reshape(-1)):
        tab = table_of(groups, g)
        if tab is not None:
            out[t:t + 1] = eref.apply_dense(out[t:t + 1], *tab)
    return out


def dense_topk_rows(L, k, groups, group_of):
    """Canonical top-k of the latents [T, N] with every token's own table applied -> (vals f32 [T, k], idx int32 [T, k])."""
    return oracle.topk(apply_dense_rows(L, groups, group_of), k)


def list_edit_rows(vals_in, idx_in, k, groups, group_of):
    """[T, kk] unedited canonical lists -> (vals [T, k], idx [T, k], edited uint8 [T, k]) by the list rule per token."""
    vals_in, idx_in = np.asarray(vals_in, dtype=np.float32), np.asarray(idx_in)
    T = vals_in.shape[0]
    out_v = np.empty((T, k), dtype=np.float32)
    out_i = np.empty((T, k), dtype=np.int32)
    edited = np.zeros((T, k), dtype=np.uint8)
    for t, g in enumerate(np.asarray(group_of).reshape(-1)):
        tab = table_of(groups, g)
        if tab is None:
            out_v[t], out_i[t] = vals_in[t, :k], idx_in[t, :k]
            continue
        E = len(tab[0])
        v, i = eref.list_edit(vals_in[t:t + 1, :k + E], idx_in[t:t + 1, :k + E], k, *tab)
        out_v[t], out_i[t] = v[0], i[0]
        edited[t] = np.isin(i[0], tab[0])
    return out_v, out_i, edited


def plan(L, order, k, E, t0, n, seed=0, start=0):
    """dict(set=..., zero=...) with E distinct features planted relative to token t0's ranking, in the manner of
    test_gpu_edits._plan for any width n: a ZERO inside the top-k, a SET equal to a selected value, a SET below the k-th
    value, a SET to -1, SETs and ZEROs on the lowest feature ids (the zero fill of an all-zero row), then random features.
    `start` rotates the priority order, so that short tables plant different positions."""
    o = order[t0]
    v = lambda r: float(L[t0, o[r]])
    picks = [("zero", int(o[0]), None),                                   # a feature inside the top-k
             ("set", int(o[k]), v(min(1, k - 1))),                        # rank k + 1, SET exactly equal to a selected value
             ("set", int(o[k + E + 5]), 0.5 * v(k - 1)),                  # outside the list, SET below the k-th value
             ("set", int(o[k + 1]), -1.0),                                # SET to -1: never selected
             ("set", 0, 0.25), ("set", 1, 0.0), ("zero", 2, None), ("zero", 3, None),   # among the zero fill
             ("set", int(o[min(2, k - 1)]), 2.0 * v(0)),                  # SET on a feature already selected
             ("set", int(o[min(3, k - 1)]), 0.0)]                         # SET to 0 on a selected feature
    picks = picks[start:] + picks[:start]
    rng = np.random.default_rng(1000 * k + E + seed)
    picks += [("set" if j % 2 else "zero", int(f), float(rng.uniform(0.0, 2.0) * v(k - 1))) for j, f in
              enumerate(rng.permutation(n)[:E + 12])]
    set_edits, zero = {}, []
    for kind, f, val in picks:
        if len(set_edits) + len(zero) >= E:
            break
        if f in set_edits or f in zero:
            continue
        if kind == "set":
            set_edits[f] = val
        else:
            zero.append(f)
    return {"set": set_edits or None, "zero": zero or None}
