"""Numpy restatement of error-preserving interventions (include/msae.h, "error-preserving interventions"; DESIGN.md
section 7i): out = x + (decode(Q) - decode(P)) for a token's plain top-k list P and its edited list Q, computed from the
entries in which the two lists DIFFER.

  diff_lists     the difference sequence D_t: an entry survives when its value is not +-0 and the other list holds no entry
                 with the same feature and the bit-identical value; Q's survivors in slot order with +value, then P's with
                 -value; padded to 2 k with zero coefficients (oracle.decode skips a zero value).
  intervene      delta = oracle.decode(D idx, D coef, W_dec, None) -- the project's j-ordered fmaf chain from +0 -- then
                 out = rne_to_dtype(f32(x) + delta); a token with an empty D_t keeps x's own bits.  THE DEFINITION: the HIP
                 kernel is held to it bit for bit.
  composed_f64   x + sum_Q v W_dec[f] - sum_P v W_dec[f] in float64: the MEANING of the definition.
  bound          the elementwise bound on |intervene - composed_f64| derived below.

THE BOUND.  u = 2^-24 (f32 unit roundoff), n = |D_t|, c_j / f_j the coefficients / features of D_t, w_j = W_dec[f_j][c].
Lists without a repeated feature (every list an encode or an edit kernel returns): the entries that do not survive occur in
both lists with the same value and feature, so they cancel EXACTLY in real arithmetic and
    composed = x + S,   S = sum_j c_j w_j,   A = sum_j |c_j w_j|.
 1. chain: n fused multiply-adds from +0, each one rounding.  The standard recursive-summation analysis (Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.1, with one rounding per term for an fma) gives
        |delta - S| <= gamma_n A,   gamma_n = n u / (1 - n u),   and so |delta| <= (1 + gamma_n) A.
 2. add: s = fl(x + delta), |s - (x + delta)| <= u |x + delta| <= u (|x| + (1 + gamma_n) A).
 3. output conversion, round to nearest even: |out - s| <= u_out |s| + sub, |s| <= (1 + u) (|x| + (1 + gamma_n) A), with
    u_out = 0 for f32 (s is an f32 already), 2^-8 for bf16 (8 significand bits), 2^-11 for f16 (11 bits); sub = half the
    smallest subnormal of the type (2^-134 bf16, 2^-25 f16), which covers s below the normal range.
 4. the float64 evaluation of `composed` itself: at most 2 k + 1 roundings of unit 2^-53 on terms bounded by
    |x| + sum_Q |v w| + sum_P |v w|: (2 k + 2) 2^-53 times that sum.
bound = gamma_n A + u B + u_out (1 + u) B + sub + (4),  B = |x| + (1 + gamma_n) A.  Nothing in it is fitted to an output.
For an empty D_t it reduces to (3) + (4) of x alone, and out == x holds exactly anyway.

THE AUTOGRAD FORM (msae.features.hooks.sae_reconstruct(preserve_error=True) with gradients on) evaluates the composition
itself in f32: y_Q and y_P by the decoder (a k-term fma chain, then + b_dec: k + 1 roundings each), r = fl(x - y_P),
s = fl(y_Q + r), then the conversion.  With A_Q = sum_Q |v w|, A_P = sum_P |v w|, b = |b_dec|, g = gamma_{k+1} and
M = |x| + (1 + g) (A_P + A_Q + 2 b), which bounds every intermediate's magnitude,
    |y_Q - exact| <= g (A_Q + b),  |y_P - exact| <= g (A_P + b),  each of the two adds rounds a value <= M (1 + u): 2 u (1 + u) M,
    conversion u_out (1 + u)^2 M + sub:
bound_composed_f32 = g (A_Q + A_P + 2 b) + 2 u (1 + u) M + u_out (1 + u)^2 M + sub + (4).  The fused path and this form
are each within their bound of the SAME float64 composition, so they differ by at most the sum of the two bounds.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle

U = 2.0 ** -24
U_OUT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
SUB = {"f32": 0.0, "bf16": 2.0 ** -134, "f16": 2.0 ** -25}


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def to_f32(x_bits, dtype):
    """The stored bits of x (uint32 for f32, uint16 for bf16 / f16) -> the f32 values the kernel up-casts to (exact)."""
    x_bits = np.ascontiguousarray(x_bits)
    if dtype == "f32":
        return x_bits.view(np.float32)
    if dtype == "bf16":
        return (x_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return x_bits.view(np.float16).astype(np.float32)


def from_f32(v, dtype):
    """Round-to-nearest-even conversion of f32 values to the bits of `dtype`; a NaN stays a (quiet) NaN."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dtype == "f32":
        return v.view(np.uint32).copy()
    if dtype == "bf16":
        u = v.view(np.uint32)
        r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
        return np.where(np.isnan(v), ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)
    with np.errstate(over="ignore"):
        return v.astype(np.float16).view(np.uint16).copy()


def diff_lists(P_v, P_i, Q_v, Q_i, N=None, with_split=False):
    """[T, k] plain and edited lists -> (idx int32 [T, 2 k], coef f32 [T, 2 k], n int [T], flagged bool): D_t in the first
    n[t] slots of row t, zero coefficients (feature 0) behind.  With N, a surviving entry whose feature lies outside [0, N) is
    skipped; `flagged` says whether ANY entry of either list was out of range.  with_split: a fifth result, n_q int [T], how many of
    the n[t] came from Q (they stand first)."""
    P_v, Q_v = np.asarray(P_v, dtype=np.float32), np.asarray(Q_v, dtype=np.float32)
    P_i, Q_i = np.asarray(P_i).astype(np.int64), np.asarray(Q_i).astype(np.int64)
    T, k = P_v.shape
    assert Q_v.shape == (T, k) and P_i.shape == (T, k) and Q_i.shape == (T, k)
    idx = np.zeros((T, 2 * k), dtype=np.int32)
    coef = np.zeros((T, 2 * k), dtype=np.float32)
    n = np.zeros(T, dtype=np.int64)
    n_q = np.zeros(T, dtype=np.int64)
    pb, qb = bits32(P_v), bits32(Q_v)
    flagged = False if N is None else bool(((P_i < 0) | (P_i >= N) | (Q_i < 0) | (Q_i >= N)).any())
    for t in range(T):
        in_p = set(zip(P_i[t].tolist(), pb[t].tolist()))
        in_q = set(zip(Q_i[t].tolist(), qb[t].tolist()))
        m = 0
        for vals, feats, vbits, other, sign in ((Q_v[t], Q_i[t], qb[t], in_p, 1.0), (P_v[t], P_i[t], pb[t], in_q, -1.0)):
            for j in range(k):
                f, b = int(feats[j]), int(vbits[j])
                if (b & 0x7FFFFFFF) == 0 or (f, b) in other:
                    continue
                if N is not None and not 0 <= f < N:
                    continue
                idx[t, m], coef[t, m] = f, np.float32(sign) * vals[j]
                m += 1
            if sign > 0:
                n_q[t] = m
        n[t] = m
    return (idx, coef, n, flagged, n_q) if with_split else (idx, coef, n, flagged)


def intervene(x_bits, dtype, P_v, P_i, Q_v, Q_i, W_dec, N=None):
    """THE DEFINITION -> (out bits [T, d] in x's storage type, n [T] = |D_t|, flagged)."""
    x_bits = np.ascontiguousarray(x_bits)
    idx, coef, n, flagged = diff_lists(P_v, P_i, Q_v, Q_i, N)
    delta = oracle.decode(idx, coef, W_dec, None)
    with np.errstate(over="ignore", invalid="ignore"):
        out = from_f32(to_f32(x_bits, dtype) + delta, dtype)
    out[n == 0] = x_bits[n == 0]
    return out, n, flagged


def _abs_sum(v, i, W, t):
    return np.abs(v[t].astype(np.float64)[:, None] * W[i[t]].astype(np.float64)).sum(0)


def composed_f64(x_f32, P_v, P_i, Q_v, Q_i, W_dec):
    """x + sum_Q - sum_P in float64, [T, d]."""
    x = np.asarray(x_f32, dtype=np.float64)
    W = np.asarray(W_dec, dtype=np.float64)
    out = np.empty_like(x)
    for t in range(x.shape[0]):
        q = (np.asarray(Q_v[t], dtype=np.float64)[:, None] * W[np.asarray(Q_i[t])]).sum(0)
        p = (np.asarray(P_v[t], dtype=np.float64)[:, None] * W[np.asarray(P_i[t])]).sum(0)
        out[t] = x[t] + (q - p)
    return out


def bound(x_f32, dtype, P_v, P_i, Q_v, Q_i, W_dec):
    """The elementwise bound of the docstring, float64 [T, d]."""
    x = np.abs(np.asarray(x_f32, dtype=np.float64))
    W = np.asarray(W_dec, dtype=np.float32)
    P_v, Q_v = np.asarray(P_v, dtype=np.float32), np.asarray(Q_v, dtype=np.float32)
    P_i, Q_i = np.asarray(P_i), np.asarray(Q_i)
    idx, coef, n, _ = diff_lists(P_v, P_i, Q_v, Q_i)
    k = P_v.shape[1]
    out = np.empty_like(x)
    for t in range(x.shape[0]):
        A = _abs_sum(coef, idx, W, t)
        gam = n[t] * U / (1.0 - n[t] * U)
        B = x[t] + (1.0 + gam) * A
        f64 = (2 * k + 2) * 2.0 ** -53 * (x[t] + _abs_sum(Q_v, Q_i, W, t) + _abs_sum(P_v, P_i, W, t))
        out[t] = gam * A + U * B + U_OUT[dtype] * (1.0 + U) * B + SUB[dtype] + f64
    return out


def bound_composed_f32(x_f32, dtype, P_v, P_i, Q_v, Q_i, W_dec, b_dec):
    """The bound on |autograd form - composed_f64| of the docstring, float64 [T, d]."""
    x = np.abs(np.asarray(x_f32, dtype=np.float64))
    W = np.asarray(W_dec, dtype=np.float32)
    b = np.abs(np.asarray(b_dec, dtype=np.float64))
    P_v, Q_v = np.asarray(P_v, dtype=np.float32), np.asarray(Q_v, dtype=np.float32)
    P_i, Q_i = np.asarray(P_i), np.asarray(Q_i)
    k = P_v.shape[1]
    g = (k + 1) * U / (1.0 - (k + 1) * U)
    out = np.empty_like(x)
    for t in range(x.shape[0]):
        A_q, A_p = _abs_sum(Q_v, Q_i, W, t), _abs_sum(P_v, P_i, W, t)
        M = x[t] + (1.0 + g) * (A_p + A_q + 2 * b)
        f64 = (2 * k + 2) * 2.0 ** -53 * (x[t] + A_q + A_p)
        out[t] = g * (A_q + A_p + 2 * b) + 2 * U * (1 + U) * M + U_OUT[dtype] * (1 + U) ** 2 * M + SUB[dtype] + f64
    return out


def values_f64(out_bits, dtype):
    return to_f32(out_bits, dtype).astype(np.float64)
