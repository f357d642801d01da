"""numpy restatement of the co-activation counters and neighbour lists (include/msae.h, msae_coact_*; DESIGN.md section
7h): the keep rule, the three segment maps, the counters as exact integer sums over segments, and the neighbour order."""
from __future__ import annotations

import numpy as np


def segments(B: int, S: int, pool: str, P: int = 576, W: int = 64):
    """(seg_of [B, S] int64 with -1 = in no segment, number of segments of the call)."""
    b = np.arange(B, dtype=np.int64)[:, None]
    s = np.arange(S, dtype=np.int64)[None, :]
    if pool == "token":
        return b * S + s, B * S
    if pool == "window":
        nw = S // W
        return np.where(s < nw * W, b * nw + s // W, -1), B * nw
    if pool == "image":
        return np.where(s < P, b + 0 * s, -1), B
    raise ValueError(pool)


def active_pairs(vals, idx, pool, N, thresh=1e-5, P=576, W=64):
    """vals / idx [B, S, k] -> (sorted unique (segment, feature) pairs as two int64 arrays, segments of the call)."""
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx, np.int64)
    B, S, k = vals.shape
    seg_of, nseg = segments(B, S, pool, P, W)
    seg = np.broadcast_to(seg_of[:, :, None], vals.shape)
    keep = (np.abs(vals) > np.float32(thresh)) & (idx >= 0) & (idx < N) & (seg >= 0)
    key = np.unique(seg[keep] * N + idx[keep])
    return key // N, key % N, nseg


def update(state, vals, idx, queries, pool, N, thresh=1e-5, P=576, W=64):
    """state = (counts [F, N] int32, seg_count [N] int64, n_segments) or None -> the state after this batch."""
    queries = np.asarray(queries, np.int64)
    F = len(queries)
    if state is None:
        state = (np.zeros((F, N), np.int32), np.zeros(N, np.int64), 0)
    counts, seg_count, n_segments = state[0].copy(), state[1].copy(), state[2]
    seg, feat, nseg = active_pairs(vals, idx, pool, N, thresh, P, W)
    seg_count += np.bincount(feat, minlength=N)
    slot_of = np.full(N, -1, np.int64)
    slot_of[queries] = np.arange(F)
    # sorted by segment: [lo, hi) of every segment that holds a query member
    lo = np.searchsorted(seg, seg, side="left")
    hi = np.searchsorted(seg, seg, side="right")
    for j in np.flatnonzero(slot_of[feat] >= 0):
        np.add.at(counts[slot_of[feat[j]]], feat[lo[j]:hi[j]], 1)
    return counts, seg_count, n_segments + nseg


def run(calls, queries, pool, N, thresh=1e-5, P=576, W=64):
    """calls: [(vals [B, S, k], idx)] -> state"""
    state = None
    for vals, idx in calls:
        state = update(state, vals, idx, queries, pool, N, thresh, P, W)
    if state is None:
        state = (np.zeros((len(queries), N), np.int32), np.zeros(N, np.int64), 0)
    return state


def brute_force(calls, queries, pool, N, thresh=1e-5, P=576, W=64):
    """The set definition itself: per segment the Python set of active features; counts[i, g] = sum over segments of
    [q_i in A][g in A]."""
    F = len(queries)
    counts, seg_count, n_segments = np.zeros((F, N), np.int32), np.zeros(N, np.int64), 0
    for vals, idx in calls:
        B, S, k = np.shape(vals)
        sets = {}
        for b in range(B):
            for s in range(S):
                if pool == "token":
                    sg = b * S + s
                elif pool == "window":
                    if s >= (S // W) * W:
                        continue
                    sg = b * (S // W) + s // W
                else:
                    if s >= P:
                        continue
                    sg = b
                A = sets.setdefault(sg, set())
                for j in range(k):
                    v, f = float(np.float32(vals[b][s][j])), int(idx[b][s][j])
                    if abs(v) > float(np.float32(thresh)) and 0 <= f < N:
                        A.add(f)
        n_segments += {"token": B * S, "window": B * (S // W), "image": B}[pool]
        for A in sets.values():
            for g in A:
                seg_count[g] += 1
            for i, q in enumerate(queries):
                if int(q) in A:
                    for g in A:
                        counts[i, g] += 1
    return counts, seg_count, n_segments


def scores(counts_row, seg_count, q, metric="jaccard"):
    """f32 scores of the candidates (c > 0) of one query row; others 0."""
    c = counts_row.astype(np.int64)
    out = np.zeros(len(c), np.float32)
    nz = c > 0
    if metric == "count":
        out[nz] = c[nz].astype(np.float32)
    else:
        u = seg_count[q] + seg_count[nz] - c[nz]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[nz] = (c[nz].astype(np.float64) / u.astype(np.float64)).astype(np.float32)
    return out, nz


def neighbors(counts, seg_count, queries, m=10, metric="jaccard", exclude_self=True):
    """(indices [F, m] int64, values [F, m] f32): (score descending, feature ascending), free slots (-1, 0.0)."""
    F, N = counts.shape
    ind = np.full((F, m), -1, np.int64)
    val = np.zeros((F, m), np.float32)
    for i, q in enumerate(np.asarray(queries, np.int64)):
        sc, nz = scores(counts[i], seg_count, q, metric)
        if exclude_self:
            nz = nz.copy()
            nz[q] = False
        g = np.flatnonzero(nz)
        order = np.lexsort((g, -sc[g].astype(np.float64)))[:m]
        ind[i, :len(order)] = g[order]
        val[i, :len(order)] = sc[g[order]]
    return ind, val


def planted_state():
    """A state with planted ties: Jaccard 1/2 == 2/4 and 1/3 == 2/6 from different pairs; a short row; an empty row."""
    n = 64
    q = [4, 9, 20, 6]
    counts = np.zeros((4, n), np.int32)
    sc = np.zeros(n, np.int64)
    sc[4] = 3
    # row of query 4 (seg_count 3): c, seg_count[g] -> u = 3 + s - c
    for g, (c, s) in {4: (3, 3), 17: (1, 1), 2: (2, 3), 11: (1, 1), 25: (2, 5), 7: (1, 1), 30: (3, 3),
                      12: (1, 2)}.items():
        counts[0, g], sc[g] = c, s
    # 17: c=1, s=1 -> u=3 -> 1/3;  11, 7: 1/3;  2: c=2, s=3 -> u=4 -> 2/4;  25: c=2, s=5 -> u=6 -> 2/6 == 1/3;
    # 12: c=1, s=2 -> u=4 -> 1/4;  30: c=3, s=3 -> u=3 -> 1.0 (ties with the query itself)
    sc[9] = 2
    counts[1, 9], counts[1, 3] = 2, 1          # short row: self + one neighbour; sc[3] below
    sc[3] = 1                                  # u = 2 + 1 - 1 = 2 -> 1/2
    counts[1, 2] = 2                           # u = 2 + 3 - 2 = 3 -> 2/3
    sc[6] = 5
    counts[3, 6] = 5
    for g in range(32, 64):                    # a long row: 32 candidates, three distinct scores
        counts[3, g] = 1 + (g % 3)
        sc[g] = 4
    return counts, sc, q
