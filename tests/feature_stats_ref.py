"""numpy restatement of the feature statistics (include/msae.h, msae_feature_stats_*): the keep rule, the two pooling
modes and the top-n order, written from the rules and not from the kernels."""
from __future__ import annotations

import numpy as np


def records(vals, idx, S, thresh=1e-5, N=None):
    """[T, k] top-k -> kept records (b, s, f, v) of one call (sparsify's rule, no filter)."""
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx, np.int64)
    T, k = vals.shape
    t = np.repeat(np.arange(T), k)
    v, f = vals.reshape(-1), idx.reshape(-1)
    keep = np.abs(v) > np.float32(thresh)
    if N is not None:
        keep &= (f >= 0) & (f < N)
    t, v, f = t[keep], v[keep], f[keep]
    return t // S, t % S, f, v


def basic_stats(f, v, N):
    count = np.bincount(f, minlength=N).astype(np.int64)
    mx = np.full(N, -np.inf, np.float32)
    np.maximum.at(mx, f, v)
    sm = np.zeros(N, np.float64)
    np.add.at(sm, f, v.astype(np.float64))
    return count, mx, sm


def candidates(b, s, f, v, S, mode, row_base, P=576, W=64):
    """(feature, pooled, id) of every pooling segment with a nonzero pooled value."""
    b, s, f, v = (np.asarray(a) for a in (b, s, f, v))
    if mode == "window":
        nw = S // W
        seg = s // W
        m = seg < nw
        b, s, f, v, seg = b[m], s[m], f[m], v[m], seg[m]
    else:
        m = s < P
        b, s, f, v = b[m], s[m], f[m], v[m]
        seg = np.zeros_like(b)
    if len(v) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64)
    order = np.lexsort((s, seg, b, f))
    b, s, f, v, seg = b[order], s[order], f[order], v[order], seg[order]
    start = np.ones(len(v), bool)
    start[1:] = (f[1:] != f[:-1]) | (b[1:] != b[:-1]) | (seg[1:] != seg[:-1])
    gidx = np.cumsum(start) - 1
    G = int(gidx[-1]) + 1
    gf, gb, gseg = f[start], b[start], seg[start]
    cnt = np.bincount(gidx, minlength=G)
    if mode == "window":
        pooled = np.full(G, -np.inf, np.float32)
        np.maximum.at(pooled, gidx, v)
        pooled = np.where(cnt < W, np.maximum(pooled, np.float32(0)), pooled).astype(np.float32)
        ids = (row_base + gb) * nw + gseg
    else:
        # f32 sum in ascending position, one addition at a time
        acc = np.zeros(G, np.float32)
        rank = np.arange(len(v)) - np.flatnonzero(start)[gidx]
        for j in range(int(rank.max()) + 1):
            m = rank == j
            acc[gidx[m]] = (acc[gidx[m]] + v[m]).astype(np.float32)
        pooled = (acc / np.float32(P)).astype(np.float32)
        ids = row_base + gb
    keep = pooled != 0
    return gf[keep].astype(np.int64), pooled[keep], ids[keep].astype(np.int64)


def top_tables(cf, cv, ci, N, n):
    """Top-n tables from all candidates: value descending, id ascending; free slots (0, -1)."""
    tv = np.zeros((N, n), np.float32)
    ti = np.full((N, n), -1, np.int64)
    order = np.lexsort((ci, -cv.astype(np.float64), cf))
    cf, cv, ci = cf[order], cv[order], ci[order]
    if len(cf):
        first = np.ones(len(cf), bool)
        first[1:] = cf[1:] != cf[:-1]
        rank = np.arange(len(cf)) - np.flatnonzero(first)[np.cumsum(first) - 1]
        m = rank < n
        tv[cf[m], rank[m]] = cv[m]
        ti[cf[m], rank[m]] = ci[m]
    return tv, ti


def merge_tables(a, b, n):
    """dst += src restated: counts add, maxima max, sums add, tables merge in the same total order."""
    (ca, ma, sa, va, ia), (cb, mb, sb, vb, ib) = a, b
    N = len(ca)
    fa = np.repeat(np.arange(N), n)
    m = np.concatenate([ia.reshape(-1), ib.reshape(-1)]) >= 0
    cf = np.concatenate([fa, fa])[m]
    cv = np.concatenate([va.reshape(-1), vb.reshape(-1)])[m]
    ci = np.concatenate([ia.reshape(-1), ib.reshape(-1)])[m]
    tv, ti = top_tables(cf, cv, ci, N, n)
    return ca + cb, np.maximum(ma, mb), sa + sb, tv, ti
