"""Numpy restatement of the JumpReLU selection (include/msae.h, "JumpReLU selection") by SORTING, and of
its backward in float64: it shares nothing with the ballot compactions and the counting sort of csrc/jump_select.hip.

    half_band(eps), floor(theta, h)     the two host-side scalars, rounded as the product rounds them
    classes(vals, idx, theta, h)        kept / near / band masks and theta_f, in the arrays' own dtype
    select(vals, idx, theta, eps)       the three-way stable partition, len, reach, src, l0, saturated rows
    backward(vals, idx, theta, eps, sel, g, s)   g_in (a routing copy: exact) and g_theta in float64 with sum |c| and n_f
    gamma(m), g_theta_bound(n_f, abs_sum)        the derived bound on an f32 g_theta
    DenseJump, dense_loss               a literal dense JumpReLU over [T, N] latents with the STE as custom autograd (torch)

Everything works in the dtype it is given: float32 arrays restate the kernels' single-precision comparisons bit for bit,
float64 arrays are the definition itself.
"""
from __future__ import annotations

import numpy as np
import torch


def half_band(eps) -> np.float32:
    return np.float32(0.5) * np.float32(eps)


def floor(theta: np.ndarray, h) -> np.float32:
    return np.float32(np.asarray(theta, np.float32).min() - np.float32(h))


def classes(vals: np.ndarray, idx: np.ndarray, theta: np.ndarray, h):
    """-> (kept, near, band, theta_f).  valid = 0 <= f < N && a > 0 (false for NaN, -0.0, negatives)."""
    v = np.asarray(vals)
    i = np.asarray(idx).astype(np.int64)
    th_all = np.asarray(theta, dtype=v.dtype)
    h = v.dtype.type(h)
    with np.errstate(invalid="ignore"):
        ok = (i >= 0) & (i < th_all.shape[0]) & (v > 0)
        th = th_all[np.where(ok, i, 0)]
        kept = ok & (v >= th)
        near = ok & ~kept & ((th - v) < h)
        band = ok & (np.abs(v - th) < h)
    return kept, near, band, th


def select(vals: np.ndarray, idx: np.ndarray, theta: np.ndarray, eps, floor_value=None) -> dict:
    v = np.asarray(vals)
    i = np.asarray(idx)
    h = half_band(eps) if v.dtype == np.float32 else 0.5 * float(eps)
    kept, near, band, _ = classes(v, i, theta, h)
    part = np.where(kept, 0, np.where(near, 1, 2))
    src = np.argsort(part, axis=1, kind="stable")                   # kept, near, rest: each part in list order
    ln = kept.sum(1).astype(np.int32)
    reach = (ln + near.sum(1)).astype(np.int32)
    live = np.arange(v.shape[1])[None] < ln[:, None]
    vo = np.where(live, np.take_along_axis(v, src, 1), v.dtype.type(0.0))
    fl = (np.asarray(theta, v.dtype).min() - v.dtype.type(h)) if floor_value is None else v.dtype.type(floor_value)
    last = v[:, -1]
    with np.errstate(invalid="ignore"):
        sat = (last > 0) & (last >= fl)
    return dict(vals=vo, idx=np.take_along_axis(i, src, 1), len=ln, reach=reach, src=src, l0=int(ln.sum()), saturated=sat,
                band=band, kept=kept, near=near)


def backward(vals: np.ndarray, idx: np.ndarray, theta: np.ndarray, eps, sel: dict, g: np.ndarray, s):
    """g [T, C]: the gradient by OUTPUT slot; s: the gradient of l0 -> (g_in in g's dtype, g_theta f64 [N], sum |c| f64 [N],
    n_f int [N]); c = -(theta_f g + s) / eps over the band entries, in float64 from the given (f32) numbers."""
    v = np.asarray(vals)
    T, C = v.shape
    g = np.asarray(g)
    live = np.arange(C)[None] < sel["len"][:, None]
    g_in = np.zeros_like(g)
    np.put_along_axis(g_in, sel["src"], np.where(live, g, g.dtype.type(0.0)), 1)
    g_at = np.zeros(g.shape, np.float64)
    np.put_along_axis(g_at, sel["src"], g.astype(np.float64), 1)
    h = half_band(eps) if v.dtype == np.float32 else 0.5 * float(eps)
    _, _, band, th = classes(v, idx, theta, h)
    e = float(np.float32(eps)) if v.dtype == np.float32 else float(eps)
    c = -(th.astype(np.float64) * g_at + float(s)) / e
    N = np.asarray(theta).shape[0]
    feats = np.asarray(idx).astype(np.int64)[band]
    g_theta = np.zeros(N, np.float64)
    abs_sum = np.zeros(N, np.float64)
    np.add.at(g_theta, feats, c[band])
    np.add.at(abs_sum, feats, np.abs(c[band]))
    return g_in, g_theta, abs_sum, np.bincount(feats, minlength=N)


def gamma(m) -> np.ndarray:
    u = 2.0 ** -24
    m = np.asarray(m, np.float64)
    return m * u / (1.0 - m * u)


def g_theta_bound(n_f, abs_sum) -> np.ndarray:
    """|fl(g_theta[f]) - g_theta[f]| <= gamma_{n_f + 3} sum |c|: n_f - 1 additions in any order and at most three roundings
    of every c, each relative to |c| -- which is why the product computes theta_f g + s with ONE rounding (a fused
    multiply-add, then the division): a separately rounded theta_f g leaves u |theta_f g|, unbounded against |c| where the
    two terms cancel."""
    return gamma(np.asarray(n_f) + 3) * np.asarray(abs_sum, np.float64)


class DenseJump(torch.autograd.Function):
    """z = a H(a - theta) over dense latents [T, N] and the count of kept entries, with the rectangle-kernel pseudo-derivatives:
    dz/da = kept, dz/dtheta = -(theta / eps) band, dH/dtheta = -(1 / eps) band."""

    @staticmethod
    def forward(ctx, pre, theta, eps):
        kept = (pre > 0) & (pre >= theta)
        band = (pre > 0) & ((pre - theta).abs() < 0.5 * eps)
        ctx.save_for_backward(kept, band, theta)
        ctx.eps = eps
        return pre * kept, kept.sum().to(pre.dtype)

    @staticmethod
    def backward(ctx, gz, gl0):
        kept, band, theta = ctx.saved_tensors
        c = -(theta * gz + gl0) / ctx.eps
        return gz * kept, (c * band).sum(0), None


# ---- test data -----------------------------------------------------------------------------------------------------------------
def lists_around(rng, T: int, C: int, N: int, theta: np.ndarray, eps, spread: float = 3.0):
    """[T, C] lists (value descending) whose values lie within spread * h of their features' thresholds: every class occurs."""
    theta = np.asarray(theta, np.float32)
    idx = np.stack([rng.permutation(N)[:C] if C <= N else rng.integers(0, N, C) for _ in range(T)]).astype(np.int64)
    th = theta[idx]
    u = rng.random((T, C)).astype(np.float32)
    vals = (th + (u - np.float32(0.5)) * np.float32(2 * spread) * half_band(eps)).astype(np.float32)
    vals = np.where(np.isfinite(th), vals, np.float32(1.0) + u).astype(np.float32)
    order = np.argsort(-vals, axis=1, kind="stable")
    return np.take_along_axis(vals, order, 1), np.take_along_axis(idx, order, 1)


def plant_hostile(vals: np.ndarray, idx: np.ndarray, theta: np.ndarray, eps) -> int:
    """In place: NaN, -0.0, +0.0, a negative, +inf, indices outside [0, N), a tie at theta_f, values at theta_f +- h, and a
    feature whose threshold is +inf where the table has one.  Spread over the list; -> how many were planted (0: too small)."""
    T, C = vals.shape
    N = theta.shape[0]
    h = half_band(eps)
    inf_feats = np.flatnonzero(np.isinf(theta))
    plants = ["nan", "negzero", "zero", "neg", "inf", "idx_hi", "idx_lo", "tie", "plus_h", "minus_h"] + (["theta_inf"] if inf_feats.size else [])
    if T * C < len(plants):
        return 0
    for j, what in enumerate(plants):
        t, c = divmod(j * (T * C) // len(plants), C)
        f = int(idx[t, c])
        th = theta[f] if np.isfinite(theta[f]) else np.float32(1.0)
        if what == "nan": vals[t, c] = np.nan
        elif what == "negzero": vals[t, c] = -0.0
        elif what == "zero": vals[t, c] = 0.0
        elif what == "neg": vals[t, c] = -1.5
        elif what == "inf": vals[t, c] = np.inf
        elif what == "idx_hi": idx[t, c] = N + 3
        elif what == "idx_lo": idx[t, c] = -2
        elif what == "tie": vals[t, c] = th
        elif what == "plus_h": vals[t, c] = np.float32(th + h)
        elif what == "minus_h": vals[t, c] = np.float32(th - h)
        elif what == "theta_inf": idx[t, c], vals[t, c] = inf_feats[0], 2.0
    return len(plants)
