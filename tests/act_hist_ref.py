"""numpy restatement of the activation histograms (include/msae.h, msae_act_hist_*), sharing no code
with the package: the bin rule by bit operations, the three segment values by explicit loops over rows and positions (the
f32 ascending-position sum for the image pool), the histogram as a plain count, and the quantile rank rule."""
from __future__ import annotations

import numpy as np


def n_bins_of(s=3, e_lo=-16, E=32):
    return E << s


def bins_of(c, s=3, e_lo=-16, E=32):
    """Bin of every value of `c` (f32, all > 0): raw = (bits >> (23 - s)) - ((127 + e_lo) << s), clamped."""
    u = np.ascontiguousarray(np.asarray(c, np.float32)).view(np.uint32).astype(np.int64)
    raw = (u >> (23 - s)) - ((127 + e_lo) << s)
    return np.clip(raw, 0, (E << s) - 1)


def raw_bins_of(c, s=3, e_lo=-16, E=32):
    u = np.ascontiguousarray(np.asarray(c, np.float32)).view(np.uint32).astype(np.int64)
    return (u >> (23 - s)) - ((127 + e_lo) << s)


def edges(s=3, e_lo=-16, E=32):
    """f32 [n_bins + 1]: the float with bits ((b + ((127 + e_lo) << s)) << (23 - s))."""
    b = np.arange((E << s) + 1, dtype=np.int64)
    return ((b + ((127 + e_lo) << s)) << (23 - s)).astype(np.uint32).view(np.float32)


def segment_values(vals, idx, pool, N, thresh=1e-5, P=576, W=64):
    """vals / idx [B, S, k] -> (features int64 [m], values f32 [m], segments of the call): every segment value of the call,
    whatever its sign.  Token pool: every kept entry.  Window pool: per (row, window, feature) the maximum of the kept
    values, joined with 0 unless the feature is kept on all W positions.  Image pool: per (row, feature) the f32 sum of the
    kept values at s < P in ascending s (list order inside a position), divided by f32(P)."""
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx, np.int64)
    B, S, k = vals.shape
    with np.errstate(invalid="ignore"):
        keep = (np.abs(vals) > np.float32(thresh)) & (idx >= 0) & (idx < N)
    feats, out = [], []
    if pool == "token":
        for b in range(B):
            for s in range(S):
                for j in np.flatnonzero(keep[b, s]):
                    feats.append(int(idx[b, s, j]))
                    out.append(vals[b, s, j])
        nseg = B * S
    elif pool == "window":
        nw = S // W
        for b in range(B):
            for w in range(nw):
                mx, pos = {}, {}
                for s in range(w * W, (w + 1) * W):
                    for j in np.flatnonzero(keep[b, s]):
                        f, v = int(idx[b, s, j]), vals[b, s, j]
                        mx[f] = v if f not in mx else np.maximum(mx[f], v)
                        pos.setdefault(f, set()).add(s)
                for f in mx:
                    feats.append(f)
                    out.append(mx[f] if len(pos[f]) == W else np.maximum(mx[f], np.float32(0)))
        nseg = B * nw
    elif pool == "image":
        for b in range(B):
            acc = {}
            for s in range(min(S, P)):
                for j in np.flatnonzero(keep[b, s]):
                    f = int(idx[b, s, j])
                    with np.errstate(invalid="ignore", over="ignore"):
                        acc[f] = np.float32(acc.get(f, np.float32(0)) + vals[b, s, j])
            for f, a in acc.items():
                feats.append(f)
                with np.errstate(invalid="ignore", over="ignore"):
                    out.append(np.float32(a / np.float32(P)))
        nseg = B
    else:
        raise ValueError(pool)
    return np.asarray(feats, np.int64), np.asarray(out, np.float32), nseg


def update(state, vals, idx, pool, N, thresh=1e-5, P=576, W=64, s=3, e_lo=-16, E=32):
    """state = (hist [N, n_bins] int32, n_segments) or None -> the state after this batch.  Counted iff c > 0."""
    if state is None:
        state = (np.zeros((N, E << s), np.int32), 0)
    hist, n_segments = state[0].copy(), state[1]
    f, c, nseg = segment_values(vals, idx, pool, N, thresh, P, W)
    with np.errstate(invalid="ignore"):
        m = c > 0
    np.add.at(hist, (f[m], bins_of(c[m], s, e_lo, E)), 1)
    return hist, n_segments + nseg


def run(calls, pool, N, thresh=1e-5, P=576, W=64, s=3, e_lo=-16, E=32):
    """calls: [(vals [B, S, k], idx)] -> (hist, n_segments)"""
    state = (np.zeros((N, E << s), np.int32), 0)
    for vals, idx in calls:
        state = update(state, vals, idx, pool, N, thresh, P, W, s, e_lo, E)
    return state


def ranks(n, qs, n_segments=0, zeros=False):
    """(r [N, Q] int64, z [N] int64, tot [N] int64): r = clamp(ceil(q * (n + z)), 1, n + z) with one f64 multiply."""
    n = np.asarray(n, np.int64)
    z = np.maximum(np.int64(n_segments) - n, 0) if zeros else np.zeros_like(n)
    tot = n + z
    r = np.ceil(np.asarray(qs, np.float64)[None, :] * tot[:, None].astype(np.float64)).astype(np.int64)
    return np.minimum(np.maximum(r, 1), tot[:, None]), z, tot


def quantile_bins(hist, qs, n_segments=0, zeros=False):
    """int32 [N, Q]: the first bin whose running count plus z reaches r = the number of bins whose running count plus z
    stays below r; -1 when r <= z, -2 when n + z = 0."""
    cum = np.cumsum(np.asarray(hist, np.int64), axis=1)
    r, z, tot = ranks(cum[:, -1], qs, n_segments, zeros)
    out = np.empty(r.shape, np.int32)
    for i in range(r.shape[1]):
        b = ((cum + z[:, None]) < r[:, i:i + 1]).sum(axis=1)
        b = np.where(r[:, i] <= z, -1, b)
        out[:, i] = np.where(tot == 0, -2, b)
    return out


def quantile(hist, qs, n_segments=0, zeros=False, s=3, e_lo=-16, E=32):
    b = quantile_bins(hist, qs, n_segments, zeros)
    v = edges(s, e_lo, E)[np.maximum(b, 0)]
    v = np.where(b == -1, np.float32(0), v)
    return np.where(b == -2, np.float32(np.nan), v).astype(np.float32)
