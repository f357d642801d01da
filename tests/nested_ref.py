"""CPU restatement of the nested decode (include/msae.h, "nested decode"), the fixtures its tests run and
the nearly-correct VARIANTS those fixtures must be able to tell apart.

  group(n)     the number of g with bounds[g] <= n (numpy.searchsorted, side="right")
  group-major  a stable sort of every row by group; an entry behind the row's length or with an index outside [0, N) comes
               last with value 0 on feature 0 (it adds nothing wherever it stands, and neither does a zero value)
  r_g          oracle.decode -- the project's slot-ordered fmaf chain from +0 with + b_dec behind it -- of the group-major list
               with the entries of the groups above g set to 0: the BITS of the kernel's out and E
  e_g          r_g - f32(x), one f32 subtract
  sq, S, g_acts, g_W, g_b   in FLOAT64 over the f32 terms e_g, with the sums of the terms' magnitudes beside them:
      sq[t][g]      = sum_c e_g[c]^2
      S[g]          = grad_full + sum_{h >= g} coef[h] e_h             (the combine)
      g_acts[t][j]  = S[group(i_j)][t] . W_dec[i_j]                     (0 for a dead index)
      g_W[n]        = sum over the pairs with i = n and v != 0 of v S[group(n)][t]
      g_b           = sum_t S[0][t]

THE BOUNDS (derived, not measured).  u = 2^-24, gamma_n = n u / (1 - n u).  sq is held to recon_ref.bound: gamma_d over the
sum of the terms' magnitudes, the bound of recon_curve's moments (same reduction).  A gradient is a sum of products whose
every term passes through at most d + G + 2 rounded operations -- at most G + 1 for the combine's fmaf chain under it, one
product, and a reduction of at most d terms (the test shapes keep the pairs of a feature and log2 of the tokens below d) --
so it is held to gamma_{d + G + 2} sum |term| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The
ENCODER's gradients (encoder_backward) reduce a second time over a feature's pairs, on top of a latent gradient that already
has that depth: they are held to the deeper gamma of encoder_depths, single-sided against float64."""
from __future__ import annotations

import functools

import numpy as np

import recon_ref
from oracle import oracle

U = 2.0 ** -24
VARIANTS_FWD = ("slot_major", "suffix_as_prefix", "boundary_off_by_one")
VARIANTS_BWD = ("grad_full_last_only", "coef_without_2")
VARIANTS = VARIANTS_FWD + VARIANTS_BWD


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def group_of(idx, bounds, variant=None) -> np.ndarray:
    side = "left" if variant == "boundary_off_by_one" else "right"     # the variant sends index m_g itself to group g
    return np.searchsorted(np.asarray(bounds, dtype=np.int64), np.asarray(idx, dtype=np.int64), side=side)


def group_major(vals, idx, bounds, lengths=None, variant=None):
    """-> (vals f32 [T, k], idx int32 [T, k], group [T, k] (G for a dead entry), order [T, k], flagged)."""
    vals = np.array(vals, dtype=np.float32)
    idx = np.array(idx).astype(np.int64)
    T, k = vals.shape
    N, G = int(bounds[-1]), len(bounds)
    read = np.ones((T, k), dtype=bool) if lengths is None else \
        np.arange(k)[None, :] < np.clip(np.asarray(lengths, dtype=np.int64), 0, k)[:, None]
    bad = (idx < 0) | (idx >= N)
    flagged = bool((bad & read).any())
    dead = bad | ~read
    grp = np.where(dead, G, group_of(np.where(dead, 0, idx), bounds, variant))
    vals[dead] = 0.0
    idx[dead] = 0
    if variant == "slot_major":
        # the list is NOT partitioned: the checkpoints (the cumulative group counts) cut the slot order instead
        counts = np.stack([(grp <= g).sum(1) for g in range(G)], 1)
        slot = np.arange(k)[None, :]
        grp = np.where(dead, G, (slot[:, :, None] >= counts[:, None, :]).sum(2))
        order = np.broadcast_to(slot, (T, k)).copy()
    else:
        order = np.argsort(grp, axis=1, kind="stable")
    take = lambda a: np.take_along_axis(a, order, 1)
    return take(vals), take(idx).astype(np.int32), take(grp), order, flagged


def recons(vals, idx, W_dec, b_dec, bounds, lengths=None, variant=None):
    """-> ([r_0 .. r_{G-1}] f32 [T, d] each, flagged)."""
    G = len(bounds)
    v, i, grp, _, flagged = group_major(vals, idx, bounds, lengths, variant)
    W_dec = np.ascontiguousarray(W_dec, dtype=np.float32)
    out = []
    for g in range(G):
        keep = (grp >= G - 1 - g) & (grp < G) if variant == "suffix_as_prefix" else grp <= g
        with np.errstate(over="ignore", invalid="ignore"):
            out.append(oracle.decode(np.ascontiguousarray(i), np.ascontiguousarray(np.where(keep, v, np.float32(0.0))), W_dec, b_dec))
    return out, flagged


def forward(x_f32, vals, idx, W_dec, b_dec, bounds, lengths=None, variant=None):
    """-> dict(out f32 [T, d], E f32 [G, T, d], sq f64 [T, G], sq_abs f64 [T, G], flagged)."""
    x = np.ascontiguousarray(x_f32, dtype=np.float32)
    rs, flagged = recons(vals, idx, W_dec, b_dec, bounds, lengths, variant)
    with np.errstate(over="ignore", invalid="ignore"):
        E = np.stack([r - x for r in rs])
        e2 = E.astype(np.float64) ** 2
    sq = e2.sum(2).T
    return dict(out=rs[-1], E=E, sq=sq, sq_abs=sq.copy(), flagged=flagged)


def combine(E, coef, grad_full=None, variant=None):
    """The float64 planes S [G, T, d] and the sums of their terms' magnitudes."""
    E = np.asarray(E, dtype=np.float64)
    G = E.shape[0]
    coef = np.asarray(coef, dtype=np.float64) * (0.5 if variant == "coef_without_2" else 1.0)
    gf = np.zeros(E.shape[1:]) if grad_full is None else np.asarray(grad_full, dtype=np.float64)
    S, S_abs = np.empty_like(E), np.empty_like(E)
    s, a = gf.copy(), np.abs(gf)
    for g in range(G - 1, -1, -1):
        s = s + coef[g] * E[g]
        a = a + np.abs(coef[g] * E[g])
        S[g], S_abs[g] = s, a
        if variant == "grad_full_last_only" and g == G - 1:
            s, a = s - gf, a - np.abs(gf)
    return S, S_abs


def combine_f32(E, coef, grad_full=None) -> np.ndarray:
    """The BITS of msae_nested_combine_f32: one fmaf per plane, from the last plane down."""
    E = np.asarray(E, dtype=np.float32)
    s = np.zeros(E.shape[1:], dtype=np.float32) if grad_full is None else np.asarray(grad_full, dtype=np.float32).copy()
    out = np.empty_like(E)
    for g in range(E.shape[0] - 1, -1, -1):
        s = fma_f32(np.float32(coef[g]), E[g], s)
        out[g] = s
    return out


def fma_f32(a, b, c) -> np.ndarray:
    """f32(a b + c) with ONE rounding, elementwise.  In float64 the product of two f32 is exact and the sum t is rounded once
    to 53 bits; rounding t to f32 equals rounding the exact value unless t sits exactly on the midpoint of two f32 (rounding
    to float64 is monotone, so it cannot carry a value across a midpoint, only onto it).  Those elements -- normal range only
    -- are decided in exact rational arithmetic."""
    from fractions import Fraction

    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32), np.asarray(c, dtype=np.float32))
    t = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = t.astype(np.float32)
    tie = ((np.ascontiguousarray(t).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & np.isfinite(t)
    for pos in zip(*np.nonzero(tie)):
        y = Fraction(float(a[pos])) * Fraction(float(b[pos])) + Fraction(float(c[pos]))
        m = Fraction(float(t[pos]))
        r = out[pos]
        lo, hi = (np.nextafter(r, np.float32(-np.inf)), r) if float(r) > float(t[pos]) else (r, np.nextafter(r, np.float32(np.inf)))
        if y != m:
            out[pos] = hi if y > m else lo
    return out


def backward(vals, idx, W_dec, bounds, S, S_abs, lengths=None):
    """float64 gradients of the list `vals` / `idx` as handed over (slot order) -> dict(g_acts, g_acts_abs [T, k], g_W,
    g_W_abs [N, d], g_b, g_b_abs [d])."""
    vals = np.asarray(vals, dtype=np.float32)
    idx = np.asarray(idx).astype(np.int64)
    T, k = vals.shape
    N = int(bounds[-1])
    W = np.asarray(W_dec, dtype=np.float64)
    read = np.ones((T, k), dtype=bool) if lengths is None else \
        np.arange(k)[None, :] < np.clip(np.asarray(lengths, dtype=np.int64), 0, k)[:, None]
    ok = (idx >= 0) & (idx < N) & read
    grp = group_of(np.where(ok, idx, 0), bounds)
    g_acts, g_acts_abs = np.zeros((T, k)), np.zeros((T, k))
    g_W, g_W_abs = np.zeros_like(W), np.zeros_like(W)
    for t in range(T):
        for j in range(k):
            if not ok[t, j]:
                continue
            n, g = idx[t, j], grp[t, j]
            g_acts[t, j] = S[g, t] @ W[n]
            g_acts_abs[t, j] = S_abs[g, t] @ np.abs(W[n])
            if vals[t, j] != 0:
                g_W[n] += float(vals[t, j]) * S[g, t]
                g_W_abs[n] += abs(float(vals[t, j])) * S_abs[g, t]
    return dict(g_acts=g_acts, g_acts_abs=g_acts_abs, g_W=g_W, g_W_abs=g_W_abs, g_b=S[0].sum(0), g_b_abs=S_abs[0].sum(0))


def encoder_backward(idx, acts, g, g_abs, x_f32, b_dec, W_enc):
    """The sparse encoder backward (ops._SparseEncode.backward) in float64, for the latent gradients g [T, K] of the lists
    idx / acts [T, K] (the main list, or the main and AuxK lists side by side) with the sums of their terms' magnitudes g_abs:
        g_W_enc[n] = sum over the pairs of n with a POSITIVE activation of g (x - b_dec)
        g_b_enc[n] = sum over the same pairs of g
        b_dec share = - sum_n g_b_enc[n] W_enc[n]
    -> dict(g_W_enc, g_W_enc_abs [N, d], g_b_enc, g_b_enc_abs [N], g_bd, g_bd_abs [d], pairs = the most pairs of one feature)."""
    idx = np.asarray(idx).astype(np.int64)
    W = np.asarray(W_enc, dtype=np.float64)
    N, d = W.shape
    live = np.asarray(acts, dtype=np.float32) > 0
    x, b = np.asarray(x_f32, dtype=np.float64), np.asarray(b_dec, dtype=np.float64)
    a, a_abs = x - b, np.abs(x) + np.abs(b)
    gl, gal = np.asarray(g, dtype=np.float64) * live, np.asarray(g_abs, dtype=np.float64) * live
    flat = idx.reshape(-1)
    gW, gW_abs = np.zeros((N, d)), np.zeros((N, d))
    np.add.at(gW, flat, (gl[:, :, None] * a[:, None, :]).reshape(-1, d))
    np.add.at(gW_abs, flat, (gal[:, :, None] * a_abs[:, None, :]).reshape(-1, d))
    gb, gb_abs = np.zeros(N), np.zeros(N)
    np.add.at(gb, flat, gl.reshape(-1))
    np.add.at(gb_abs, flat, gal.reshape(-1))
    return dict(g_W_enc=gW, g_W_enc_abs=gW_abs, g_b_enc=gb, g_b_enc_abs=gb_abs, g_bd=-(gb @ W), g_bd_abs=gb_abs @ np.abs(W),
                pairs=int(np.bincount(flat[live.reshape(-1)], minlength=N).max()))


def weighted_row_sum_depth(N: int) -> int:
    """The depth of msae_weighted_row_sum_f32 as tests/train_ref.py (weighted_row_sum) reads it off the kernel."""
    groups = -(-N // 64)
    per = -(-groups // 64)
    n_mid = -(-groups // per)
    return min(N, 64) + (-(-per // 4) + 3 + 2 + 1) + (-(-n_mid // 4) + 3 + 2 + 1)


def encoder_depths(d: int, G: int, pairs: int, N: int) -> dict:
    """Rounded operations a term of an ENCODER gradient passes through.  The latent gradient under it is itself a result of
    the node's backward, held to depth d + G + 2; the encoder backward then reduces a SECOND time, over a feature's pairs,
    which the node's depth has no room for.  So these gradients are held to the depth that does hold, single-sided against
    float64 (a deviation from gamma_{d+G+2}, stated in DESIGN.md section 7o):
        g_W_enc   d + G + 2, the subtract x - b_dec, the product, a chain over at most `pairs` pairs
        g_b_enc   d + G + 2, a sum over at most `pairs` pairs
        b_dec     the larger of the node's own share (d + G + 2) and g_b_enc's depth + the weighted row sum's, + 1 for the
                  addition of the two shares"""
    base = d + G + 2
    return dict(g_W_enc=base + 2 + pairs, g_b_enc=base + pairs, b_dec=base + pairs + weighted_row_sum_depth(N) + 1)


def grad_bound(abs_terms, d: int, G: int, depth=None):
    return gamma(d + G + 2 if depth is None else depth) * np.asarray(abs_terms, dtype=np.float64) + d * 2.0 ** -149


def inside(got, exp, lim) -> bool:
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    return bool((np.abs(got - exp) <= lim).all())


def worst(got, exp, lim) -> float:
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    lim = np.asarray(lim, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(lim > 0, np.abs(got - exp) / lim, 0.0)))


# ---- fixtures ------------------------------------------------------------------------------------------------------------
N = 2048
BOUNDS = {1: (N,), 2: (512, N), 5: (128, 256, 512, 1024, N), 8: (1, 2, 64, 65, 300, 1024, 2047, N)}      # G = 8: m_0 = 1
KINDS = ("mixed", "last", "first", "gaps", "zeros")


class Case:
    """One forward fixture: the buffers handed to the op (`view`: the list is the [:, :k] view of a [T, k + 7] buffer whose
    tail holds another plausible list), x as f32 values representable in `dtype`.  kind: "mixed" (features anywhere), "last"
    (every entry in the last group), "first" (every entry in the first), "gaps" (the middle groups stay empty), "zeros" (mixed,
    a third of the activations +-0)."""

    def __init__(self, d, k, T, G, kind="mixed", dtype="f32", wide=False, view=False, lengths=None, seed=0):
        self.d, self.k, self.T, self.G, self.kind, self.dtype, self.wide, self.view = d, k, T, G, kind, dtype, wide, view
        self.bounds = BOUNDS[G]
        self.id = f"d{d}-k{k}-T{T}-G{G}-{kind}-{dtype}-{'i64' if wide else 'i32'}" + ("-view" if view else "") + \
            (f"-len_{lengths}" if lengths else "")
        rng = np.random.default_rng([seed, d, k, T, G])
        self.W_dec = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
        self.b_dec = (0.5 * rng.standard_normal(d)).astype(np.float32)
        kk = k + (7 if view else 0)
        vals = -np.sort(-rng.uniform(0.05, 4.0, (T, kk)).astype(np.float32), axis=1)
        lo, hi = 0, N
        b = self.bounds
        if kind == "last":
            lo = b[-2] if G > 1 else 0
        elif kind == "first":
            hi = b[0]
        idx = np.stack([rng.integers(lo, hi, kk) if hi - lo < kk else lo + rng.permutation(hi - lo)[:kk] for _ in range(T)])
        if kind == "gaps" and G > 2:                       # only the first and the last group hold entries
            first = rng.integers(0, b[0], (T, kk))
            last = rng.integers(b[-2], N, (T, kk))
            idx = np.where(rng.random((T, kk)) < 0.5, first, last)
        if kind == "zeros":
            z = rng.random((T, kk))
            vals[z < 0.2] = 0.0
            vals[(z >= 0.2) & (z < 0.33)] = -0.0
        self.buf_vals = np.ascontiguousarray(vals)
        self.buf_idx = np.ascontiguousarray(idx.astype(np.int64 if wide else np.int32))
        self.lengths = None
        if lengths == "around8":                           # around the unroll of 8, 0, and values the kernel must clamp
            pool = np.array([0, 1, 7, 8, 9, 15, 16, 17, k - 1, k, k + 5, -3, 2 ** 31 - 1], dtype=np.int64)
            self.lengths = pool[np.arange(T) % len(pool)].astype(np.int32)
            tail = np.arange(kk)[None, :] >= np.clip(self.lengths.astype(np.int64), 0, k)[:, None]
            tail[:, k:] = False
            self.buf_vals[tail] = np.nan                   # poisoned: the slots behind a row's length are not read
            self.buf_idx[tail] = N + 17
        x = rng.standard_normal((T, d)) * 0.7
        self.x = recon_ref.to_dtype(x.astype(np.float32), dtype)

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
    ds, ks, Ts, Gs = (4, 128, 1000, 1002, 1028), (1, 8, 9, 65, 300), (1, 37, 300), (1, 2, 5, 8)
    dts = ("f32", "bf16", "f16")
    n = 0
    for a, d in enumerate(ds):                             # every d with every k; T, G, kind, dtype, index type, view cycle
        for b_, k in enumerate(ks):
            T = Ts[n % 3]
            if k == 300 and T == 300 and d >= 1000:
                T = 37                                     # (the largest reference: kept small)
            out.append(Case(d, k, T, Gs[(a + b_) % 4], KINDS[n % 5], dts[n % 3], wide=bool(n % 2), view=bool((n // 2) % 2)))
            n += 1
    # every G and every kind at one vector and the one-column width, and lengths on both
    out += [Case(128, 8, 37, G, kind) for G in Gs for kind in KINDS if not (G == 1 and kind in ("last", "first", "gaps"))]
    out += [Case(1002, 9, 37, 5, kind, "bf16", wide=True) for kind in ("last", "first", "gaps", "zeros")]
    out += [Case(128, 32, 37, 5, "mixed", lengths="around8"), Case(1002, 65, 37, 8, "zeros", "f16", wide=True, view=True, lengths="around8"),
            Case(1028, 300, 37, 2, "mixed", "bf16", view=True, lengths="around8")]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def expected(i: int):
    c = CASES[i]
    return forward(c.x, c.vals, c.idx, c.W_dec, c.b_dec, c.bounds, c.lengths)


def small_case(seed: int = 5, T: int = 6, k: int = 8, d: int = 12, n_lat: int = 64, bounds=(4, 16, 17, 64)):
    """The host tests' fixture: every group populated, one index on a boundary (16), repeated features, one zero activation,
    x far from the reconstruction."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((n_lat, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.5 * rng.standard_normal(d)).astype(np.float32)
    vals = -np.sort(-rng.uniform(0.1, 3.0, (T, k)).astype(np.float32), axis=1)
    idx = np.stack([rng.permutation(n_lat)[:k] for _ in range(T)]).astype(np.int64)
    idx[:, 0] = rng.integers(17, n_lat, T)                 # the largest activation in the last group: slot order != group order
    idx[:, 1] = 16                                         # a boundary index: group 2, not group 1
    idx[:, 2] = rng.integers(0, 4, T)
    idx[:, 3] = rng.integers(4, 16, T)
    vals[0, 4] = 0.0
    x = rng.standard_normal((T, d)).astype(np.float32)
    grad_full = rng.standard_normal((T, d)).astype(np.float32)
    coef = (2.0 * rng.uniform(0.1, 1.0, len(bounds))).astype(np.float32)
    return dict(W_dec=W, b_dec=b, vals=vals, idx=idx, x=x, bounds=tuple(bounds), grad_full=grad_full, coef=coef, T=T, k=k, d=d)
