"""CPU restatement of the reconstruction-error curve (include/msae.h, "reconstruction error against sparsity"; DESIGN.md
section 7j), the fixtures the GPU test runs, and the nearly-correct VARIANTS the fixtures must be able to tell apart.

  r_kappa    oracle.decode(idx[:, :kappa], vals[:, :kappa], W_dec, b_dec) -- the project's slot-ordered fmaf chain from +0 with
             + b_dec behind it; kappa = 0 is (+0) + b_dec.  An out-of-range entry is skipped (value 0) before the oracle sees it.
  e          r - f32(x), one f32 subtract
  moments    (sum e^2, sum x r, sum r^2) and xx = sum x^2 in FLOAT64 over the f32 terms e, x, r (their products are exact in
             float64).

THE BOUND (derived, not measured).  u = 2^-24, gamma_d = d u / (1 - d u).  A sum of d products formed in f32 -- rounded or
fused, added in ANY order -- differs from the exact sum S by at most gamma_d sum |term| (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1: every term passes through at most d roundings; tests/intervene_ref.py argues the same), plus
d 2^-149 for products that underflow.  r and e underneath are bit-defined, so nothing else enters:
    |out - S64| <= gamma_d sum |term| + d 2^-149.
ReconStats' float64 sums of n f32 outputs are held to 2 n 2^-53 sum |term| against the float64 sum of the same outputs
(n - 1 float64 additions in any order, and the restatement's own n - 1)."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from oracle import oracle

U = 2.0 ** -24
N = 512
DTYPES = ("f32", "bf16", "f16")
EDGE_D = (4, 6, 100, 1024, 1028, 4096, 5000)
KS_KINDS = ("zero", "k", "ends", "first16", "pow2")


def gamma(d: int) -> float:
    return d * U / (1.0 - d * U)


def to_dtype(a: np.ndarray, dtype: str) -> np.ndarray:
    """f32 values rounded to values representable in `dtype`, as f32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "f32":
        return a
    if dtype == "f16":
        return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


def ks_of(kind: str, k: int) -> list:
    if kind == "zero":
        return [0]
    if kind == "k":
        return [k]
    if kind == "ends":
        return sorted({0, 1, k})
    if kind == "first16":
        return list(range(0, min(k, 15) + 1))
    return sorted({1 << i for i in range(k.bit_length()) if (1 << i) <= k} | {k})


def sanitize(vals, idx, n_lat: int):
    """-> (vals f32 with 0 where the feature is out of range, idx int32 with 0 there, flagged)."""
    vals = np.array(vals, dtype=np.float32)
    idx = np.array(idx).astype(np.int64)
    bad = (idx < 0) | (idx >= n_lat)
    vals[bad] = 0.0
    idx[bad] = 0
    return vals, idx.astype(np.int32), bool(bad.any())


def recon(vals, idx, W_dec, b_dec, kappa: int) -> np.ndarray:
    """r_kappa [T, d] f32 of sanitized lists."""
    if kappa == 0:
        return np.broadcast_to(np.float32(0.0) + np.asarray(b_dec, dtype=np.float32), (vals.shape[0], W_dec.shape[1])).copy()
    return oracle.decode(np.ascontiguousarray(idx[:, :kappa]), np.ascontiguousarray(vals[:, :kappa]), W_dec, b_dec)


def _sums(x, r, e):
    """float64 (sum, sum of magnitudes) of the three moments: [T, 3] each."""
    x, r, e = x.astype(np.float64), r.astype(np.float64), e.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        terms = (e * e, x * r, r * r)
        return np.stack([t.sum(1) for t in terms], 1), np.stack([np.abs(t).sum(1) for t in terms], 1)


def moments(x_f32, vals, idx, W_dec, b_dec, ks, n_lat=None, variant=None):
    """-> (mom [T, C, 3], xx [T], mom_abs [T, C, 3], xx_abs [T], flagged), all float64.  `variant`: one of VARIANTS instead of
    the definition (the power check)."""
    x = np.ascontiguousarray(x_f32, dtype=np.float32)
    W_dec = np.ascontiguousarray(W_dec, dtype=np.float32)
    n_lat = W_dec.shape[0] if n_lat is None else n_lat
    vals, idx, flagged = sanitize(vals, idx, n_lat)
    T, k = vals.shape
    mom = np.empty((T, len(ks), 3))
    mom_abs = np.empty((T, len(ks), 3))
    for c, kappa in enumerate(ks):
        if variant == "off_by_one":
            kappa = min(kappa + 1, k)
        with np.errstate(over="ignore", invalid="ignore"):
            r = recon(vals, idx, W_dec, None if variant == "no_bias" else b_dec, kappa)
            if variant == "no_bias" and kappa == 0:
                r = np.zeros_like(r)
            if variant == "keep_zeros":
                for t, j in zip(*np.nonzero(vals[:, :kappa] == 0)):
                    r[t] += vals[t, j] * W_dec[idx[t, j]]
            if variant == "f64_recon":
                W64 = W_dec.astype(np.float64)
                r64 = np.stack([(vals[t, :kappa].astype(np.float64)[:, None] * W64[idx[t, :kappa]]).sum(0) for t in range(T)])
                r64 = r64 + np.asarray(b_dec, dtype=np.float64)
                e64 = r64 - x.astype(np.float64)
                terms = (e64 * e64, x.astype(np.float64) * r, r.astype(np.float64) ** 2)
                mom[:, c] = np.stack([t_.sum(1) for t_ in terms], 1)
                mom_abs[:, c] = np.stack([np.abs(t_).sum(1) for t_ in terms], 1)
                continue
            e = r - x
        mom[:, c], mom_abs[:, c] = _sums(x, r, e)
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        xx = (x64 * x64).sum(1)
    return mom, xx, mom_abs, xx.copy(), flagged


VARIANTS = ("off_by_one", "no_bias", "keep_zeros", "f64_recon", "ld_k")


def bound(mom_abs, d: int):
    return gamma(d) * mom_abs + d * 2.0 ** -149


def outside(got, exp, exp_abs, d: int) -> np.ndarray:
    """[T] bool: token t has an output outside the bound (a NaN on one side only counts as outside)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(got - exp) <= bound(exp_abs, d)) | (np.isnan(got) & np.isnan(exp)) | \
             (np.isinf(got) & np.isinf(exp) & (np.sign(got) == np.sign(exp)))
    return ~ok.reshape(ok.shape[0], -1).all(1)


# ---- fixtures ------------------------------------------------------------------------------------------------------------
class Case:
    """One op-level fixture.  `buf_vals` / `buf_idx` [T, k + pad]: the buffers handed to the op (pad = 7 for a `view` case: the
    list is their `[:, :k]` view, the columns behind hold a DIFFERENT plausible list tail); `x` f32 values representable in
    `dtype`; `offset`: x is handed over one element off the allocation's start (the unaligned path)."""

    def __init__(self, d, k, T, ks_kind, dtype, wide, view, offset=False, seed=0, close=False, n_lat=N):
        self.d, self.k, self.T, self.dtype, self.wide, self.view, self.offset = d, k, T, dtype, wide, view, offset
        self.ks = ks_of(ks_kind, k)
        self.n_lat = n_lat
        self.id = f"d{d}-k{k}-T{T}-{ks_kind}-{dtype}-{'i64' if wide else 'i32'}" + ("-view" if view else "") + \
            ("-offset" if offset else "") + ("-close" if close else "")
        rng = np.random.default_rng([seed, d, k, T])
        self.W_dec = (rng.standard_normal((n_lat, d)) / np.sqrt(d)).astype(np.float32)
        self.b_dec = (0.5 * rng.standard_normal(d)).astype(np.float32)
        kk = k + (7 if view else 0)
        vals = -np.sort(-rng.uniform(0.05, 4.0, (T, kk)).astype(np.float32), axis=1)
        idx = np.stack([np.resize(rng.permutation(n_lat), kk) for _ in range(T)])
        self.buf_vals = np.ascontiguousarray(vals)
        self.buf_idx = np.ascontiguousarray(idx.astype(np.int64 if wide else np.int32))
        dense = np.zeros((T, n_lat))
        np.add.at(dense, (np.arange(T)[:, None], idx[:, :k]), vals[:, :k].astype(np.float64))
        r = dense @ self.W_dec.astype(np.float64) + self.b_dec
        noise = rng.standard_normal((T, d)) * (2.0 ** -12 if close else 0.5)
        self.x = to_dtype((r + noise * (np.abs(r) if close else 1.0)).astype(np.float32), dtype)

    @property
    def vals(self):
        return self.buf_vals[:, :self.k]

    @property
    def idx(self):
        return self.buf_idx[:, :self.k]

    def __repr__(self):
        return self.id


def _cases():
    out = []
    ks_cycle, k_cycle, t_cycle = itertools.cycle(KS_KINDS), itertools.cycle((1, 4, 32, 256)), itertools.cycle((1, 5, 300))
    for i, (d, dtype) in enumerate(itertools.product(EDGE_D, DTYPES)):
        k, T = next(k_cycle), next(t_cycle)
        if d >= 4096 and k == 256 and T == 300:
            T = 5                                          # (the largest reference: kept small, T = 300 runs at other widths)
        out.append(Case(d, k, T, next(ks_cycle), dtype, wide=bool(i % 2), view=bool((i // 2) % 2)))
    # x one element off the 16-byte grid: the one-column path at widths the vector path would take
    out += [Case(4096, 32, 5, "pow2", "f32", False, False, offset=True), Case(1024, 4, 300, "ends", "bf16", True, True, offset=True),
            Case(100, 32, 5, "first16", "f16", False, False, offset=True)]
    # the production list shape, and x CLOSE to its reconstruction at a width where one rounding of r is visible in e
    out += [Case(4096, 32, 300, "pow2", "bf16", True, False), Case(1028, 256, 300, "pow2", "f32", False, True),
            Case(4, 4, 300, "ends", "f32", False, False, close=True), Case(6, 32, 300, "pow2", "f32", True, True, close=True)]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def expected(i: int):
    """The restatement of CASES[i], computed once per process and shared: (mom, xx, mom_abs, xx_abs, flagged)."""
    c = CASES[i]
    return moments(c.x, c.vals, c.idx, c.W_dec, c.b_dec, c.ks, c.n_lat)


def hostile_case():
    """T = 8, k = 8, d = 100, N = 512: +0 and -0 values (one of them in front of a NON-FINITE decoder row), a repeated feature,
    features N and -1, and (token 5) a non-finite x."""
    rng = np.random.default_rng(77)
    T, k, d = 8, 8, 100
    W = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    W[7] = np.inf                                        # only ever listed with a zero value
    W[0, :3] = np.nan                                    # row 0: what a skipped entry's load may touch
    b = (0.5 * rng.standard_normal(d)).astype(np.float32)
    vals = -np.sort(-rng.uniform(0.1, 3.0, (T, k)).astype(np.float32), axis=1)
    idx = np.stack([rng.permutation(np.arange(8, N))[:k] for _ in range(T)]).astype(np.int64)
    vals[0, 2], idx[0, 2] = 0.0, 7
    vals[1, 0], idx[1, 0] = -0.0, 7
    idx[2, 3] = idx[2, 1]                                # repeated feature: both entries count
    idx[3, 4] = N
    idx[4, 0] = -1
    idx[6, 7] = 2 ** 31 - 1
    x = rng.standard_normal((T, d)).astype(np.float32)
    x[5, 17] = np.inf
    return dict(W_dec=W, b_dec=b, vals=vals, idx=idx, x=x, ks=[0, 1, 3, 8], d=d, k=k, T=T)


# ---- ReconStats over a list of update calls ------------------------------------------------------------------------------
def stats(calls, W_dec, b_dec, ks, edges, mom_of=None):
    """calls: [(x [B, S, d] f32 values, vals [B, S, k], idx [B, S, k])] -> per group g a dict of the float64 state
    (n, sums [C, 3], sums_abs = sum |moment|, terms_abs = sum over tokens and columns of |term|, xx_sum, cos_sum [C], x_sum [d]) over the checkpoints `ks` (give 0 among them to get the centre's
    sum).  `mom_of(x2d, vals2d, idx2d)` -> (mom [T, C, 3], xx [T]) replaces the restatement's moments (the kernel's own f32
    outputs: then only the float64 accumulation is restated)."""
    G, C = len(edges), len(ks)
    d = W_dec.shape[1]
    out = [dict(n=0, sums=np.zeros((C, 3)), sums_abs=np.zeros((C, 3)), terms_abs=np.zeros((C, 3)), xx_sum=0.0, cos_sum=np.zeros(C), x_sum=np.zeros(d))
           for _ in range(G)]
    for x, vals, idx in calls:
        B, S, _ = x.shape
        k = vals.shape[-1]
        if mom_of is None:
            mom, xx, t_abs = moments(x.reshape(-1, d), vals.reshape(-1, k), idx.reshape(-1, k), W_dec, b_dec, ks)[:3]
        else:
            mom, xx = mom_of(x.reshape(-1, d), vals.reshape(-1, k), idx.reshape(-1, k))
            t_abs = np.abs(np.asarray(mom, dtype=np.float64))
        t_abs = t_abs.reshape(B, S, C, 3)
        mom, xx = np.asarray(mom, dtype=np.float64).reshape(B, S, C, 3), np.asarray(xx, dtype=np.float64).reshape(B, S)
        den = np.sqrt(xx[..., None] * mom[..., 2])
        cos = np.where(den > 0, mom[..., 1] / np.where(den > 0, den, 1.0), 0.0)
        ends = list(edges[1:]) + [S]
        for g, (a, b) in enumerate(zip(edges, ends)):
            a, b = min(a, S), min(b, S)
            if b <= a:
                continue
            o = out[g]
            o["n"] += B * (b - a)
            o["sums"] += mom[:, a:b].sum((0, 1))
            o["sums_abs"] += np.abs(mom[:, a:b]).sum((0, 1))
            o["terms_abs"] += t_abs[:, a:b].sum((0, 1))
            o["xx_sum"] += xx[:, a:b].sum()
            o["cos_sum"] += cos[:, a:b].sum((0, 1))
            o["x_sum"] += x[:, a:b].astype(np.float64).sum((0, 1))
    return out


def stats_bound(n: int, sums_abs):
    return 2.0 * n * 2.0 ** -53 * sums_abs


def total_variance_direct(xs) -> float:
    """sum |x - mean|^2 over the rows of xs [n, d] in float64, two passes."""
    xs = np.asarray(xs, dtype=np.float64)
    return float(((xs - xs.mean(0)) ** 2).sum())
