"""Numpy restatement of the neighbours / top-logits numerics contract (include/msae.h, "neighbours"):

  dot    dot[m, n] = oracle.pre_acts(Q[q_rows], K, 0, 0, relu=False): the ascending-k f32 fma chain from +0
  inv    inv[n] = f32(1 / max(||W_n||_2, 1e-12)), the norm in f64 (F.normalize's clamp)
  value  dot, then * q_scale[m], then * k_scale[n]: two separately rounded f32 multiplies
  rank   tests/probe_ref.topk (value descending, index ascending, -0 ranks with +0) after the excluded index is masked out;
         values come back decoded from the rank key, so a -0 reads +0

q_rows outside [0, Qn) are clamped as the kernel clamps them."""
from __future__ import annotations

import numpy as np

import probe_ref
from oracle import oracle


def inv_norms(W: np.ndarray) -> np.ndarray:
    n = np.sqrt((W.astype(np.float64) ** 2).sum(axis=1))
    return (1.0 / np.maximum(n, 1e-12)).astype(np.float32)


def dots(Q: np.ndarray, K: np.ndarray, q_rows=None) -> np.ndarray:
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    if q_rows is not None:
        Q = Q[np.clip(np.asarray(q_rows, dtype=np.int64), 0, Q.shape[0] - 1)]
    d = Q.shape[1]
    if Q.shape[0] == 0:
        return np.zeros((0, K.shape[0]), dtype=np.float32)
    return oracle.pre_acts(Q, np.ascontiguousarray(K, dtype=np.float32), None, np.zeros(d, np.float32), relu=False)


def values(dot: np.ndarray, q_scale=None, k_scale=None) -> np.ndarray:
    v = dot.astype(np.float32)
    if q_scale is not None:
        v = (v * np.asarray(q_scale, dtype=np.float32)[:, None]).astype(np.float32)
    if k_scale is not None:
        v = (v * np.asarray(k_scale, dtype=np.float32)[None, :]).astype(np.float32)
    return v


def rank(v: np.ndarray, k: int, exclude=None):
    """Canonical top-k of each row of the dense values, the row's excluded column left out."""
    M, N = v.shape
    assert 1 <= k <= N - (0 if exclude is None else 1), (k, N)
    vals = np.empty((M, k), dtype=np.float32)
    idx = np.empty((M, k), dtype=np.int64)
    cols = np.arange(N)
    for m in range(M):
        keep = cols if exclude is None or not 0 <= int(exclude[m]) < N else np.delete(cols, int(exclude[m]))
        rv, ri = probe_ref.topk(v[m, keep][None], k)
        vals[m], idx[m] = rv[0], keep[ri[0]]
    return vals + np.float32(0.0), idx          # (-0 -> +0: values are decoded from the rank key)


def rows_topk(Q, K, k, q_rows=None, q_scale=None, k_scale=None, exclude=None):
    return rank(values(dots(Q, K, q_rows), q_scale, k_scale), k, exclude)


def neighbors(W, features, k, exclude_self=True):
    """Sae.neighbors: cos = dot * inv[m] * inv[n], the feature's own index skipped."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    feats = np.arange(W.shape[0]) if features is None else np.asarray(features, dtype=np.int64)
    inv = inv_norms(W)
    return rows_topk(W, W, k, q_rows=feats, q_scale=inv[feats], k_scale=inv, exclude=feats if exclude_self else None)


def cos_bound(d: int) -> float:
    """|cos_ours - cos_reference|: both are f32 sums of d products of unit-norm rows (gamma_d per side) plus the
    normalisation roundings."""
    return 2.0 * (d + 4) * 2.0 ** -24


def compare_with_reference(vals, idx, ref_vals_ext, ref_idx, bound):
    """Ours (vals, idx: [M, k]) against the reference's own summation, which differs from ours within `bound` (a scalar or
    [M, 1]).  ref_vals_ext [M, k + 1]: the reference's ranked values and the one ranking just below them; ref_idx [M, k].
    -> (values within the bound, index positions compared, mismatches among them, positions left out by the separation
    rule): indices must agree wherever the reference's value is further than `bound` from both of its ranking neighbours."""
    vals, ext = np.asarray(vals, dtype=np.float64), np.asarray(ref_vals_ext, dtype=np.float64)
    k = vals.shape[1]
    assert ext.shape == (vals.shape[0], k + 1) and np.asarray(ref_idx).shape == vals.shape
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), (vals.shape[0], 1))
    ok_vals = bool(np.all(np.abs(vals - ext[:, :k]) <= bound))
    gap = np.abs(np.diff(ext, axis=1))                 # gap[:, j] between ranks j and j + 1
    sep = gap > bound                                  # rank j against the one below it
    sep[:, 1:] &= gap[:, :-1] > bound                  # ... and against the one above it
    mism = int(np.sum((np.asarray(idx) != np.asarray(ref_idx)) & sep))
    return ok_vals, int(sep.sum()), mism, int((~sep).sum())
