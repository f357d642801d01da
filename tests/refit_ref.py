"""Float64 restatement of the support refit (include/msae.h, "support refit"), the fixtures the GPU
test runs, the bounds its outputs are held to, and the nearly-correct SOLVERS the bounds must be able to tell apart.

The restatement is written from the definition, not from the kernel's recurrence: per token, the live rows D of W_dec (f32
values in float64), y = f32(x) - b_dec (the one f32 subtract of the definition, then float64), and for EVERY prefix kappa of
the support a literal `numpy.linalg.lstsq` of y on the first kappa rows.  opt[kappa] = |y - D_kappa^T c_kappa|^2.

THE BOUNDS (derived, not measured).  u = 2^-24, gamma_n = n u / (1 - n u).
  Gram.    An entry of G = D D^T or h = D y is a sum of d f32 products added in some order plus three additions of partial
           sums: every term passes through at most d + 3 roundings (Higham, Accuracy and Stability of Numerical Algorithms,
           section 3.1), so |dG_ij| <= gamma_{d+3} |D_i| |D_j| and |dh_i| <= gamma_{d+3} |D_i| |y|, hence
           ||dG||_2 <= gamma_{d+3} tr G <= s gamma_{d+3} ||G||_2 and ||dh||_2 <= gamma_{d+3} ||D||_F ||y||_2.
  Solve.   Cholesky and the two substitutions return c with (G^ + E) c = h^, ||E||_2 <= s gamma_{3s+1} ||G^||_2 /
           (1 - s gamma_{s+1}) (Higham, theorem 10.4 with (10.7)).
  eps_G  = s gamma_{d+3} + s gamma_{3s+1} (1 + s gamma_{d+3}) / (1 - s gamma_{s+1}): the matrix the coefficients solve
           EXACTLY is G + F with ||F||_2 <= eps_G ||G||_2 and right-hand side h + dh.
  1. Residual.   G c - h = -F c + dh, so ||G c - h||_2 <= eps (||G||_2 ||c||_2 + ||h||_2) with
           eps = eps_G + gamma_{d+3} rho, rho = ||D||_F ||y||_2 / ||h||_2 (the Gram error of h is relative to |D_i| |y|, not
           to |h_i|).  The cases are asserted to have cond(G) <= 1e3 and rho <= 16: on a support that is ill-conditioned, or
           nearly orthogonal to y, the bound says nothing.
  2. Excess.     The objective is quadratic: f(c) - f(c*) = r^T G^-1 r with r = G c - h, so the excess is at most
           (bound 1)^2 / lambda_min(G).
  3. Gains.      sum_{j < kappa} gain_j = h^_k^T (G_k + F_k)^-1 h^_k (the forward solve of a leading block) against
           q = h_k^T G_k^-1 h_k = yy - opt[kappa]: with c = G_k^-1 h_k, mu = lambda_min(G) - eps_G ||G||_2 > 0 and
           dc = (||dh|| + eps_G ||G|| ||c||) / mu, |q^ - q| <= ||dh|| (||c|| + dc) + ||h_k|| dc; plus u sum gain for
           the one rounding of each z_j * z_j.
  4. Evaluation. err_fit and err_enc are sums over d columns of (y_c - chain_c)^2 with a slot-ordered f32 fma chain: the chain
           and the subtract are off by at most delta_c = gamma_{s+1} (sum_j |a_j D_jc| + |y_c|); the sum of squares by
           gamma_{d+8} of its terms' magnitudes (d products, the butterfly, the waves and the slabs); together
           sum_c (2 |e_c| delta_c + delta_c^2) + gamma_{d+8} sum_c (|e_c| + delta_c)^2.  yy: gamma_{d+8} yy.
Each bound also carries d 2^-149 for products that underflow."""
from __future__ import annotations

import functools

import numpy as np

from recon_ref import to_dtype

U = 2.0 ** -24
N = 1024
TINY = 2.0 ** -149
COND_MAX = 1e3
RHO_MAX = 16.0


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def eps_G(d: int, s: int) -> float:
    return s * gamma(d + 3) + s * gamma(3 * s + 1) * (1.0 + s * gamma(d + 3)) / (1.0 - s * gamma(s + 1))


def tau(d: int, s: int) -> float:
    """The kernel's dependence threshold, 2 gamma_{d+s} rounded to f32."""
    return float(np.float32(2.0 * gamma(d + s)))


# ---- fixtures -------------------------------------------------------------------------------------------------------------
class Case:
    """One call's inputs.  x [T, d] f32 values representable in `dtype`; vals / idx [T, ld] with the list in the first s
    columns; `dropped` [T, s]: slots the definition removes as dependent (the later copy of a repeated index)."""

    def __init__(self, d, s, T, dtype="f32", wide=False, ld=None, seed=0, zeros=(), bad=None, dup=None):
        self.d, self.s, self.T, self.dtype, self.wide = d, s, T, dtype, wide
        self.ld = s if ld is None else ld
        rng = np.random.default_rng([seed, d, s, T])
        W = rng.standard_normal((N, d)).astype(np.float32)
        self.W_dec = (W / np.linalg.norm(W.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        self.b_dec = (0.1 * rng.standard_normal(d)).astype(np.float32)
        idx = np.stack([rng.permutation(N)[:self.ld] for _ in range(T)]).astype(np.int64)
        true = rng.uniform(0.5, 2.0, (T, self.ld))
        vals = -np.sort(-(true * (1.0 + 0.2 * rng.standard_normal((T, self.ld)))).clip(0.05), axis=1)
        self.dropped = np.zeros((T, s), dtype=bool)
        for j in zeros:                                  # zero-valued slots (every token)
            vals[:, j] = 0.0
        if bad is not None:                              # (token, slot): one index outside [0, N)
            idx[bad] = N + 7
        if dup is not None:                              # (token, first, later): slot `later` repeats slot `first`
            t, a, b = dup
            idx[t, b] = idx[t, a]
            self.dropped[t, b] = True
        live = (vals[:, :s] != 0) & (idx[:, :s] >= 0) & (idx[:, :s] < N)
        mix = np.einsum("tj,tjc->tc", true[:, :s] * live, self.W_dec[np.where(live, idx[:, :s], 0)].astype(np.float64))
        noise = rng.standard_normal((T, d)) * (0.3 / np.sqrt(d))
        self.x = to_dtype((mix + noise + self.b_dec).astype(np.float32), dtype)
        self.vals = vals.astype(np.float32)
        self.idx = idx if wide else idx.astype(np.int32)
        self.flagged = bad is not None

    @classmethod
    def from_arrays(cls, x, vals, idx, W_dec, b_dec, dtype="f32"):
        """A case over given inputs (x as f32 values representable in `dtype`; W_dec must have N rows)."""
        c = cls.__new__(cls)
        c.x, c.vals, c.idx = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(vals, dtype=np.float32), np.asarray(idx)
        c.W_dec, c.b_dec = np.ascontiguousarray(W_dec, dtype=np.float32), np.ascontiguousarray(b_dec, dtype=np.float32)
        assert c.W_dec.shape[0] == N
        (c.T, c.d), c.s, c.ld, c.dtype, c.wide = c.x.shape, c.vals.shape[1], c.vals.shape[1], dtype, c.idx.dtype == np.int64
        c.dropped, c.flagged = np.zeros((c.T, c.s), dtype=bool), False
        return c

    def __repr__(self):
        return f"Case(d={self.d}, s={self.s}, T={self.T}, {self.dtype}, {'i64' if self.wide else 'i32'}, ld={self.ld})"


class TokenRef:
    """The definition for one token in float64.  `keep` [s]: the support after the definition's removals."""

    def __init__(self, case: Case, t: int, center: bool = True):
        s, d = case.s, case.d
        v, i = case.vals[t, :s], case.idx[t, :s].astype(np.int64)
        self.live = (v != 0) & (i >= 0) & (i < N)
        self.keep = self.live & ~case.dropped[t]
        rows = case.W_dec[np.where(self.live, i, 0)].astype(np.float64) * self.live[:, None]
        self.rows = rows                                                          # [s, d], zero for a dead slot
        y32 = case.x[t] - case.b_dec if center else case.x[t]                      # the definition's f32 subtract
        self.y = y32.astype(np.float64)
        self.vals = np.where(self.live, v, 0).astype(np.float64)
        self.yy = float(self.y @ self.y)
        D = rows[self.keep]
        self.D, self.G, self.h = D, D @ D.T, D @ self.y
        self.opt = np.empty(s + 1)                                                # literal lstsq per prefix
        self.opt[0] = self.yy
        for kappa in range(1, s + 1):
            Dk = rows[:kappa][self.keep[:kappa]]
            if Dk.shape[0] == 0:
                self.opt[kappa] = self.yy
                continue
            c, *_ = np.linalg.lstsq(Dk.T, self.y, rcond=None)
            r = self.y - Dk.T @ c
            self.opt[kappa] = float(r @ r)
            if kappa == s:
                self.cstar = c
        if not self.keep.any():
            self.cstar = np.zeros(0)
        ev = np.linalg.eigvalsh(self.G) if D.shape[0] else np.ones(1)
        self.lam_min, self.normG = float(ev[0]), float(ev[-1])
        self.cond = self.normG / self.lam_min
        self.normh, self.normD, self.normy = float(np.linalg.norm(self.h)), float(np.linalg.norm(D)), float(np.sqrt(self.yy))
        self.rho = self.normD * self.normy / self.normh if self.normh > 0 else np.inf

    def objective(self, coef) -> float:
        """|y - rows^T coef|^2 in float64, coef over all s slots."""
        e = self.y - np.asarray(coef, dtype=np.float64) @ self.rows
        return float(e @ e)

    def eval_bound(self, coef, d: int, s: int) -> float:
        """Bound 4 for the f32 evaluation of |y - rows^T coef|^2."""
        a = np.abs(np.asarray(coef, dtype=np.float64))
        e = np.abs(self.y - np.asarray(coef, dtype=np.float64) @ self.rows)
        delta = gamma(s + 1) * (a @ np.abs(self.rows) + np.abs(self.y))
        return float((2 * e * delta + delta ** 2).sum() + gamma(d + 8) * ((e + delta) ** 2).sum() + d * TINY)


@functools.lru_cache(maxsize=None)
def _token_ref(case: Case, t: int) -> TokenRef:
    return TokenRef(case, t)


def token_ref(case: Case, t: int) -> TokenRef:
    """Computed once per (case, token) and shared by the tests; never modified."""
    return _token_ref(case, t)


def premises(case: Case, tokens) -> list:
    """What bound 1 needs of a case, in float64: [] when it holds."""
    out = []
    for t in tokens:
        r = token_ref(case, t)
        if r.D.shape[0] and not (r.cond <= COND_MAX and r.rho <= RHO_MAX and r.lam_min > 2 * eps_G(case.d, case.s) * r.normG):
            out.append(f"token {t}: cond {r.cond:.3g} rho {r.rho:.3g}")
    return out


def gain_bound(r: TokenRef, d: int, s: int, kappa: int, gain_sum: float) -> float:
    """Bound 3: how far sum_{j < kappa} gain_j (`gain_sum`) may lie from yy - opt[kappa]; equally how far the optimal error
    yy - gain_sum formed in float64 may lie from opt[kappa].  0 when no slot of the prefix is in the support."""
    n = int(r.keep[:kappa].sum())
    if n == 0:
        return 0.0
    eG = eps_G(d, s)
    dh = gamma(d + 3) * r.normD * r.normy
    mu = r.lam_min - eG * r.normG
    c = np.linalg.solve(r.G[:n, :n], r.h[:n])
    dc = (dh + eG * r.normG * float(np.linalg.norm(c))) / mu
    return (dh * (float(np.linalg.norm(c)) + dc) + float(np.linalg.norm(r.h[:n])) * dc + U * abs(gain_sum) + d * TINY
            + 8 * 2.0 ** -53 * r.yy)


def violations(case: Case, out: dict, tokens, log=None) -> list:
    """Every way the outputs `out` (coef [T, s], gain [T, s], err_fit, err_enc, yy, n_dependent [T]) of the tokens leave the
    definition's bounds, as strings; [] when they hold.  `log`: a list that receives every (figure, bound) pair."""
    d, s = case.d, case.s
    eG, g3 = eps_G(d, s), gamma(d + 3)
    bad = []

    def hold(what, t, err, bound):
        if log is not None:
            log.append((what, t, float(err), float(bound)))
        if not err <= bound:
            bad.append(f"{what} token {t}: {err:.6g} > {bound:.6g}")

    for t in tokens:
        r = token_ref(case, t)
        coef, gain = out["coef"][t].astype(np.float64), out["gain"][t].astype(np.float64)
        if not (np.isfinite(coef).all() and np.isfinite(gain).all()):
            bad.append(f"non-finite token {t}")
            continue
        if (coef[~r.keep] != 0).any() or (gain[~r.keep] != 0).any():
            bad.append(f"token {t}: a slot outside the support has a coefficient or a gain")
        if int(out["n_dependent"][t]) != int((r.live & ~r.keep).sum()):
            bad.append(f"token {t}: n_dependent {int(out['n_dependent'][t])} != {int((r.live & ~r.keep).sum())}")
        hold("yy", t, abs(float(out["yy"][t]) - r.yy), gamma(d + 8) * r.yy + d * TINY)
        ck = coef[r.keep]
        b1 = 0.0
        if ck.size:
            # 1. residual of the normal equations
            eps = eG + g3 * r.rho
            res = float(np.linalg.norm(r.G @ ck - r.h))
            b1 = eps * (r.normG * float(np.linalg.norm(ck)) + r.normh) + d * TINY
            hold("residual", t, res, b1)
            # 2. excess objective
            full = np.zeros(s)
            full[r.keep] = ck
            hold("excess", t, r.objective(full) - r.opt[s], b1 * b1 / r.lam_min + 4 * 2.0 ** -53 * r.yy)
        # 3. gain prefix sums against yy - opt[kappa]
        pre = np.concatenate([[0.0], np.cumsum(gain)])
        for kappa in range(1, s + 1):
            hold(f"gain[:{kappa}]", t, abs(pre[kappa] - (r.yy - r.opt[kappa])), gain_bound(r, d, s, kappa, pre[kappa]))
        # 4. the two errors, each against the float64 objective at the coefficients it was evaluated with
        hold("err_fit", t, abs(float(out["err_fit"][t]) - r.objective(coef)), r.eval_bound(coef, d, s))
        hold("err_enc", t, abs(float(out["err_enc"][t]) - r.objective(r.vals)), r.eval_bound(r.vals, d, s))
        # err_fit <= err_enc on every token, up to the excess and the two evaluations: the optimum over the kept support lies
        # below any other point of its span, and the encoder's point is one -- a slot dropped as dependent is an exact
        # repeat of a kept row here, so its value moves along that row
        slack = b1 * b1 / r.lam_min + r.eval_bound(coef, d, s) + r.eval_bound(r.vals, d, s) + 4 * 2.0 ** -53 * r.yy
        hold("err_fit - err_enc", t, float(out["err_fit"][t]) - float(out["err_enc"][t]), slack)
    return bad


# ---- solvers: the definition in plain f32, and nearly-right ones -------------------------------------------------------------
SOLVERS = ("f32", "diagonal", "no_bias", "keep_zeros", "no_back_solve", "reversed_prefix", "coef_1e-3")


def solve(case: Case, solver: str = "f32") -> dict:
    """The outputs of a plain-f32 numpy solve of `case` ("f32": the definition; the others: one mistake each)."""
    d, s, T = case.d, case.s, case.T
    f32 = np.float32
    out = dict(coef=np.zeros((T, s), f32), gain=np.zeros((T, s), f32), err_fit=np.zeros(T, f32), err_enc=np.zeros(T, f32),
               yy=np.zeros(T, f32), n_dependent=np.zeros(T, np.int32))
    for t in range(T):
        v, i = case.vals[t, :s], case.idx[t, :s].astype(np.int64)
        ok = (i >= 0) & (i < N)
        live = ok & (v != 0)
        sup = ok if solver == "keep_zeros" else live
        y = case.x[t] if solver == "no_bias" else case.x[t] - case.b_dec
        rows = case.W_dec[np.where(ok, i, 0)] * ok[:, None].astype(f32)
        order = [j for j in range(s) if sup[j]]
        if solver == "reversed_prefix":
            order = order[::-1]
        G = (rows[order] @ rows[order].T).astype(f32)
        h = (rows[order] @ y).astype(f32)
        n = len(order)
        L, z, kept = np.zeros((n, n), f32), np.zeros(n, f32), np.zeros(n, bool)
        for j in range(n):                                                      # Cholesky with the definition's drop rule
            p = f32(G[j, j] - (L[j, :j] * L[j, :j]).sum(dtype=f32))
            if not p > f32(tau(d, s)) * G[j, j]:
                continue
            kept[j] = True
            L[j, j] = np.sqrt(p)
            for m in range(j + 1, n):
                L[m, j] = f32(G[m, j] - (L[m, :j] * L[j, :j]).sum(dtype=f32)) / L[j, j]
            z[j] = f32(h[j] - (L[j, :j] * z[:j]).sum(dtype=f32)) / L[j, j]
        c = np.zeros(n, f32)
        if solver == "diagonal":
            c = np.where(kept, h / np.where(kept, np.diag(G), 1), 0).astype(f32)
        elif solver == "no_back_solve":
            c = z.copy()
        else:
            for j in range(n - 1, -1, -1):
                if kept[j]:
                    c[j] = f32(z[j] - (L[j + 1:, j] * c[j + 1:]).sum(dtype=f32)) / L[j, j]
        if solver == "coef_1e-3" and n:
            c[np.argmax(np.abs(c))] *= f32(1.001)
        out["coef"][t, order], out["gain"][t, order] = c, z * z
        out["n_dependent"][t] = n - int(kept.sum())
        yt = case.x[t] - case.b_dec
        out["yy"][t] = (yt * yt).sum(dtype=f32)
        ef, ee = yt - out["coef"][t] @ rows, yt - np.where(live, v, 0).astype(f32) @ rows
        out["err_fit"][t], out["err_enc"][t] = (ef * ef).sum(dtype=f32), (ee * ee).sum(dtype=f32)
    return out


# ---- ReconStats(refit=True) over a list of update calls -------------------------------------------------------------------------
def stats_sums(opt_curves, positions, ks, edges):
    """float64 sums of the optimal error per (position group, checkpoint): opt_curves [n, len(ks)] per token, positions [n]."""
    edges = list(edges)
    grp = np.searchsorted(np.asarray(edges), np.asarray(positions), side="right") - 1
    out = np.zeros((len(edges), len(ks)))
    for g in range(len(edges)):
        out[g] = np.asarray(opt_curves, dtype=np.float64)[grp == g].sum(0)
    return out
