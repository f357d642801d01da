"""Numpy restatement of the batch-level selection (include/msae.h, "batch-level selection") by SORTING:
it shares nothing with the radix select and the ballot compaction of csrc/batch_select.hip.

    theta(vals, K)                    step 2: the K-th largest of the entries with v > 0 (min P / +inf), and |P|
    list_filter(vals, idx, theta, ...)  steps 3-6: keep mask, stable partition, len, saturated
    batch_select(vals, idx, k)        theta + filter of canonical lists
    dense_batchtopk(pre, k)           uncapped BatchTopK over the dense [T, N] latents: theta and the keep mask
    canonical_lists(pre, C)           the top-C list of every row: value descending, index ascending
"""
from __future__ import annotations

import numpy as np


def positive(v: np.ndarray) -> np.ndarray:
    """v > 0: false for NaN, -0.0 and negatives; +inf is positive."""
    with np.errstate(invalid="ignore"):
        return np.asarray(v) > 0


def theta(vals: np.ndarray, K: int):
    """-> (theta as np.float32, |P|)"""
    v = np.asarray(vals, dtype=np.float32).reshape(-1)
    P = np.sort(v[positive(v)])[::-1]                       # descending; +inf first
    if P.size == 0:
        return np.float32(np.inf), 0
    return np.float32(P[min(int(K), P.size) - 1]), int(P.size)


def keep_mask(vals: np.ndarray, idx: np.ndarray, th, theta_feat=None) -> np.ndarray:
    v = np.asarray(vals, dtype=np.float32)
    if theta_feat is None:
        with np.errstate(invalid="ignore"):
            return positive(v) & (v >= np.float32(th))
    tf = np.asarray(theta_feat, dtype=np.float32)
    i = np.asarray(idx).astype(np.int64)
    ok = (i >= 0) & (i < tf.shape[0])
    with np.errstate(invalid="ignore"):
        return ok & positive(v) & (v >= tf[np.where(ok, i, 0)])


def list_filter(vals: np.ndarray, idx: np.ndarray, th, theta_feat=None):
    """-> (vals_out, idx_out, len int32 [T], saturated bool [T]).  Every row: the kept entries in list order, then the dropped
    ones in theirs with activation +0.0.  saturated = v_last > 0 && v_last >= th (th = the floor in table mode)."""
    v = np.asarray(vals, dtype=np.float32)
    i = np.asarray(idx)
    keep = keep_mask(v, i, th, theta_feat)
    T, C = v.shape
    vo, io = np.zeros_like(v), np.empty_like(i)
    for t in range(T):
        kept, dropped = np.flatnonzero(keep[t]), np.flatnonzero(~keep[t])
        vo[t, :kept.size] = v[t, kept]
        io[t] = i[t, np.concatenate([kept, dropped])]
    last = v[:, -1]
    with np.errstate(invalid="ignore"):
        sat = positive(last) & (last >= np.float32(th))
    return vo, io, keep.sum(1).astype(np.int32), sat


def batch_select(vals: np.ndarray, idx: np.ndarray, k: int):
    """-> (vals_kept, idx, len, theta, saturated) of canonical [T, C] lists"""
    th, _ = theta(vals, vals.shape[0] * k)
    vo, io, ln, sat = list_filter(vals, idx, th)
    return vo, io, ln, th, sat


def dense_batchtopk(pre: np.ndarray, k: int):
    """Uncapped BatchTopK over dense latents [T, N] -> (theta, keep mask [T, N]); ties at theta all kept."""
    th, _ = theta(pre, pre.shape[0] * k)
    return th, keep_mask(pre, None, th)


def canonical_lists(pre: np.ndarray, C: int):
    """-> (vals [T, C] f32, idx [T, C] int64): value descending, index ascending among equals (-0.0 ties with +0.0)."""
    pre = np.asarray(pre, dtype=np.float32)
    order = np.argsort(-(pre + np.float32(0.0)), axis=1, kind="stable")[:, :C]
    return np.take_along_axis(pre, order, 1), order.astype(np.int64)
