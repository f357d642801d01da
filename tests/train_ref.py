"""Float64 restatement of the parameter-sized passes of the training step (csrc/train.hip) with DERIVED forward-error bounds,
the checking function both the GPU tests and the host tests use, and the table of cases they share.

Every function takes the float32 inputs the kernel reads, evaluates the pass in float64 (torch, CPU) and returns the result
together with an elementwise bound on |kernel - result| that holds for ANY correct float32 evaluation with the kernel's
documented summation structure.  Nothing here is fitted to what a GPU produced.

Error model.  u = 2^-24 is the unit roundoff of float32.  To first order in u:

  * one float32 +, -, * or fma of exact operands is off by at most u |result|; sqrtf and the division are given 2 u;
  * a float32 sum of terms t_i in which every term passes through at most `depth` rounded operations (its own products
    included) is off by at most  depth * u * sum_i |t_i|.  `depth` is read off the kernel:
        block_sum        6 xor-shuffle levels + the sequential sum of the wave partials (4 at 256 threads, 16 at 1024)
        a row reduction  `trips` sequential per-thread accumulations (row length / 1024 on the f32x4 path, / 256 on the scalar
                         path of d % 4 != 0), 3 more adds inside an f32x4 on the vector path, then block_sum
        grad_sumsq       the same per thread over the grid stride, one more add for the scalar tail, block_sum, then one float
                         atomic per workgroup and the value already in the accumulator
        sum (fixed)      two add levels inside an f32x4, `trips`, one tail add, block_sum over 16 waves, the accumulator
        weighted rows    an fma chain over the (at most 64) rows of a group, then twice: four interleaved chains over the
                         partial rows, two combining adds and the multiplication by the scale
  * input errors are propagated as an interval (see adam_rows);
  * ONE overall safety factor of 2 (SAFETY) covers the second-order terms the first-order model drops.

The hyper-parameters reach the kernels as C floats, so the restatement evaluates at their float32 values (f32()): 1 - beta2 of
a float32 0.999 differs from 0.001 by 3e-5 relative, which is the kernel's contract and not an error of it.

Scope: magnitudes where g^2, the row sums of squares and every intermediate are finite, normal float32 numbers (or exactly
zero).  Overflow and gradual underflow are not modelled."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

U = 2.0 ** -24
SAFETY = 2.0
F64 = torch.float64


def f32(x) -> float:
    """The float32 value a C float argument carries, as a Python float."""
    return float(np.float32(x))


def _d(t, device="cpu") -> torch.Tensor:
    return t.detach().to(device, F64)


def kernel_rows(shape) -> Tuple[int, int]:
    """[rows, d] as ops.adam_rows_ hands a parameter to the kernel: matrices as they are, vectors as [numel / 1024, 1024]
    when that divides and as one row otherwise."""
    if len(shape) == 2:
        return int(shape[0]), int(shape[1])
    n = int(np.prod(shape))
    d = 1024 if n % 1024 == 0 else n
    return n // d, d


def row_reduction_depth(d: int) -> int:
    """Rounded additions a term of a one-workgroup row reduction passes through (unit_norm_rows_kernel, the projection dot
    product and the renorm of the Adam kernels): 3 inside the f32x4 and d/1024 trips on the vector path, d/256 trips on the
    scalar path, 6 shuffle levels, 4 wave partials.  The term's own products are the caller's to add."""
    vec = d % 4 == 0
    trips = -(-d // 1024) if vec else -(-d // 256)
    return (3 if vec else 0) + trips + 6 + 4


def _sqrt_interval(x, dx):
    """sqrt(x) and a bound on |sqrtf(x') - sqrt(x)| for |x' - x| <= dx: the larger one-sided deviation of the concave
    function (the lower end clamped at 0) plus the 2 u of sqrtf itself."""
    s = torch.sqrt(x)
    lo = torch.sqrt(torch.clamp(x - dx, min=0.0))
    hi = torch.sqrt(x + dx)
    return s, torch.maximum(s - lo, hi - s) + 2 * U * s


def _renorm(w, dw, eps: float, d: int):
    """w / (|w|_row + eps) for rows known to within dw, and its bound (not yet multiplied by SAFETY).

        S  = sum w^2            dS  = sum (2 |w| dw + dw^2) + D u sum (|w| + dw)^2      D = 1 product + row_reduction_depth
        n  = sqrt(S)            dn  = sqrt interval of (S, dS)
        den = n + eps           dden = dn + u den
        inv = 1 / den (2 u), w * inv (u)
        d(w / den) <= dw / den_lo + |w| dden / den_lo^2 + 4 u |w / den|             den_lo = den - dden (>= eps / 2)"""
    D = 1 + row_reduction_depth(d)
    S = (w * w).sum(1, keepdim=True)
    dS = (2 * w.abs() * dw + dw * dw).sum(1, keepdim=True) + D * U * ((w.abs() + dw) ** 2).sum(1, keepdim=True)
    n, dn = _sqrt_interval(S, dS)
    den = n + eps
    dden = dn + U * den
    den_lo = torch.clamp(den - dden, min=0.5 * eps)
    out = w / den
    return out, dw / den_lo + w.abs() * dden / den_lo ** 2 + 4 * U * out.abs()


def unit_norm_rows(W, eps: float):
    """W[r] / (|W[r]|_2 + eps) -> (result, bound), both float64 [rows, d]."""
    w = _d(W)
    out, b = _renorm(w, torch.zeros_like(w), f32(eps), w.shape[1])
    return out, SAFETY * b


def adam_rows(W, G, M, V, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, total_sumsq=None,
              max_norm: float = 1.0, project: bool = False, renorm_eps: Optional[float] = None, device="cpu"):
    """One step of clip -> (projection) -> Adam -> (row renorm) -> ((W', M', V'), (dW, dM, dV)), float64, shaped like W.
    `device`: where the float64 arithmetic runs (the same torch expressions; a trajectory test with 8M-element matrices
    evaluates them next to its inputs).

        c  = min(1, max_norm / (sqrt(S) + 1e-6))          S = total_sumsq, the float32 value the kernel reads (None: c = 1)
        g  = c G ;  g -= <g, w> w  if project
        m' = m + (g - m)(1 - b1) ;  v' = b2 v + (1 - b2) g^2
        w' = w - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps) ;  then w' /= |w'| + renorm_eps (optional)

    Bounds, propagated as an interval (x-hat is the float32 value, dx bounds |x-hat - x|):

        clip    sqrtf 2 u, the add u, the float32 constant 1e-6f u, the division 2 u: dc = 6 u c; min(1, .) is 1-Lipschitz
                and dc = 0 once the quotient clears 1 by more than that
        g0      dg0 = |G| dc + u |c G|
        along   a = sum g0 w:  da = sum |w| dg0 + D u sum |g0 w|,  D = 1 product + row_reduction_depth(d)
        g       dg = dg0 + |w| da + u |a w| + u |g|
        m'      dm = (1 - b1) dg + u (3 |(g - m)(1 - b1)| + |m'|)                 (subtract, 1 - b1, multiply; add)
        v'      dv = (1 - b2)(2 |g| dg + dg^2) + u (|b2 v| + 3 (1 - b2) g^2 + |v'|)
        sqrt    _sqrt_interval(v', dv): evaluated at v' - dv clamped at 0 -- an element whose v' is mostly a cancellation
                residue gets a wide bound from this by itself
        denom   q = sqrt(v') / bc2 (bc2 rounded to float: u, division 2 u): dq = dsqrt / bc2 + 3 u q; ddenom = dq + u denom
        ratio   dr = dm / denom_lo + |m'| ddenom / denom_lo^2 + 2 u |r|,  denom_lo = denom - ddenom
        update  step_size = lr / bc1 (bc1 rounded u, division 2 u), the product u: dupd = step_size dr + 4 u |upd|
        w'      dw = dupd + u |w'|
        renorm  _renorm(w', dw)"""
    shape = W.shape
    rows, d = kernel_rows(shape)
    w, g_in, m, v = (_d(t, device).reshape(rows, d) for t in (W, G, M, V))
    assert not project or len(shape) == 2
    lr_, b1, b2, eps_, mn = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(max_norm)
    if total_sumsq is None:
        c, dc = 1.0, 0.0
    else:
        S = float(total_sumsq)
        c_raw = mn / (math.sqrt(S) + 1e-6)
        c = min(1.0, c_raw)
        dc = 0.0 if c_raw * (1 - 8 * U) >= 1.0 else 6 * U * c
    g0 = c * g_in
    dg0 = g_in.abs() * dc + U * g0.abs()
    if project:
        D = 1 + row_reduction_depth(d)
        a = (g0 * w).sum(1, keepdim=True)
        da = (w.abs() * dg0).sum(1, keepdim=True) + D * U * (g0 * w).abs().sum(1, keepdim=True)
        g = g0 - a * w
        dg = dg0 + w.abs() * da + U * (a * w).abs() + U * g.abs()
    else:
        g, dg = g0, dg0
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    t = (g - m) * omb1
    m1 = m + t
    dm = omb1 * dg + U * (3 * t.abs() + m1.abs())
    v1 = b2 * v + omb2 * g * g
    dv = omb2 * (2 * g.abs() * dg + dg * dg) + U * ((b2 * v).abs() + 3 * omb2 * g * g + v1.abs())
    bc1 = 1.0 - b1 ** step
    bc2 = math.sqrt(1.0 - b2 ** step)
    step_size = lr_ / bc1
    sq, dsq = _sqrt_interval(v1, dv)
    q = sq / bc2
    dq = dsq / bc2 + 3 * U * q
    denom = q + eps_
    ddenom = dq + U * denom
    denom_lo = torch.clamp(denom - ddenom, min=0.5 * eps_)
    r = m1 / denom
    dr = dm / denom_lo + m1.abs() * ddenom / denom_lo ** 2 + 2 * U * r.abs()
    upd = step_size * r
    dupd = step_size * dr + 4 * U * upd.abs()
    w1 = w - upd
    dw = dupd + U * w1.abs()
    if renorm_eps is not None:
        assert len(shape) == 2
        w1, dw = _renorm(w1, dw, f32(renorm_eps), d)
    return (tuple(x.reshape(shape) for x in (w1, m1, v1)),
            tuple(SAFETY * x.reshape(shape) for x in (dw, dm, dv)))


def grad_sumsq_grid(n: int) -> Tuple[int, int, int]:
    """(n4, grid, trips) of msae_grad_sumsq_f32: f32x4 elements, workgroups (capped at 4096), grid-stride trips per thread."""
    n4 = n // 4
    grid = min(4096, max(1, -(-n4 // 256)))
    return n4, grid, max(1, -(-n4 // (grid * 256)))


def grad_sumsq(g, accum: float = 0.0):
    """accum + sum g^2 -> (float, bound).  depth = 1 product + 3 adds inside the f32x4 + trips + 1 (tail) + 6 + 4 (block_sum)
    + one atomic per workgroup (in any order) -- the accumulator's own value rides through all of them."""
    x = _d(g).reshape(-1)
    _, grid, trips = grad_sumsq_grid(x.numel())
    depth = 1 + 3 + trips + 1 + 6 + 4 + grid
    s = float((x * x).sum())
    return float(accum) + s, SAFETY * depth * U * (abs(float(accum)) + s)


def sum(v, accum: float = 0.0):  # noqa: A001 (named after the pass)
    """accum + sum v in the fixed order of sum_fixed_kernel -> (float, bound).  depth = 2 adds inside the f32x4 + trips over
    1024 threads + 1 (tail) + 6 shuffle levels + 16 wave partials + the add onto the accumulator."""
    x = _d(v).reshape(-1)
    trips = max(1, -(-(x.numel() // 4) // 1024))
    depth = 2 + trips + 1 + 6 + 16 + 1
    return float(accum) + float(x.sum()), SAFETY * depth * U * (abs(float(accum)) + float(x.abs().sum()))


def weighted_row_sum(W, s, scale: float = 1.0):
    """scale * sum_n s[n] W[n, :] over the rows with s[n] != 0 ONLY (the others are not read: they may hold anything) ->
    (result [d], bound [d]).  depth: the fma chain over min(N, 64) rows; then per level four interleaved chains
    (ceil(rows / 4) + up to 3 leftovers onto the first), two combining adds and the multiplication by the scale."""
    Wd, sd = _d(W), _d(s).reshape(-1)
    N, d = Wd.shape
    live = sd != 0
    groups = -(-N // 64)
    per = -(-groups // 64)
    n_mid = -(-groups // per)
    depth = min(N, 64) + (-(-per // 4) + 3 + 2 + 1) + (-(-n_mid // 4) + 3 + 2 + 1)
    sc = f32(scale)
    if not bool(live.any()):
        z = torch.zeros(d, dtype=F64)
        return z, z.clone()
    Wl, sl = Wd[live], sd[live]
    out = sc * (sl[:, None] * Wl).sum(0)
    return out, SAFETY * depth * U * abs(sc) * (sl.abs()[:, None] * Wl.abs()).sum(0)


# ---- the check both files use ----------------------------------------------------------------------------------------------
def assert_within(got, ref, bound, what: str = "", device="cpu") -> float:
    """Every element of `got` within its own bound of `ref` (nothing excluded; a zero bound demands equality) -> the largest
    ratio of observed error to bound.  `device`: where the comparison runs."""
    got = torch.as_tensor(got).detach().to(device, F64)
    ref = torch.as_tensor(ref, dtype=F64).to(device)
    bound = torch.as_tensor(bound, dtype=F64).to(device).expand_as(ref)
    got = got.reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    assert bool(torch.isfinite(bound).all()), f"{what}: non-finite bound"
    err = (got - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).reshape(-1)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside their bound; worst at flat index {i}: "
                             f"got {float(got.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r} "
                             f"err {float(err.reshape(-1)[i]):.3e} bound {float(bound.reshape(-1)[i]):.3e}")
    pos = bound > 0
    return float(torch.where(pos, err / torch.where(pos, bound, torch.ones_like(bound)), torch.zeros_like(err)).max()) \
        if bool(pos.any()) else 0.0


# ---- the cases --------------------------------------------------------------------------------------------------------------
def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


@dataclass(frozen=True)
class AdamCase:
    """One adam_rows_ call: warm moments (M ~ 1e-4 signed, 0 <= V ~ 1e-7); with three kernel rows or more, row 1 has G == 0
    and nonzero moments (it must still move and decay) and row 2 has G = M = V = 0 (it must stay bit-identical).
    norm_ratio: |G| / max_norm (G is scaled to it); None keeps G ~ gscale.  sumsq: "given" | "none" | "zero" (all-zero G).
    mutants: the wrong restatements of test_train_ref_host.py this case must reject."""
    name: str
    shape: Tuple[int, ...]
    step: int = 2
    lr: float = 1e-3
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    max_norm: float = 1.0
    project: bool = True
    gscale: float = 1e-3
    norm_ratio: Optional[float] = 2.0
    sumsq: str = "given"
    mutants: Tuple[str, ...] = field(default=())

    def kwargs(self):
        return dict(betas=self.betas, eps=self.eps, max_norm=self.max_norm, project=self.project and len(self.shape) == 2)


ADAM_SHAPES = [(3, 1), (5, 50), (4, 1025),            # scalar path
               (3, 4), (7, 1000), (4, 1028),          # vector path; 1028: the second trip runs with one live thread
               (3, 252), (3, 256), (3, 260),          # one wave's 256-element trip: one f32x4 short, full, one over
               (3, 8188), (3, 8192),                  # the KEEP = 8 register window, full and one f32x4 short
               (2, 8196), (2, 12288),                 # d > 8192: the fused entry hands back to the separate passes
               (1, 1000), (1, 1024), (1, 4096), (1, 8192), (1, 12288),     # one row
               (1,), (3072,), (4100,)]                # vectors: [1, 1], [3, 1024], [1, 4100]
_HYPER_SHAPES = [(7, 1000), (5, 50)]
_HYPERS = [
    dict(name="step1", step=1),
    dict(name="step2", step=2, mutants=("no_sqrt_bc2", "bc_at_step_minus_1", "v_from_unprojected", "tail4_untouched")),
    dict(name="step1000", step=1000, mutants=("bc_at_step_minus_1",)),
    dict(name="step100000", step=100000),
    dict(name="betas", step=3, betas=(0.8, 0.95), mutants=("no_sqrt_bc2",)),
    dict(name="eps1e-3", step=3, eps=1e-3, norm_ratio=None, gscale=1e-3, mutants=("eps_before_bc2",)),
    dict(name="maxnorm1e-4", max_norm=1e-4, norm_ratio=2.0, mutants=("clip_without_1e-6",)),
    dict(name="norm0.5x", norm_ratio=0.5, mutants=("clip_without_min",)),
    dict(name="norm0.999x", norm_ratio=0.999, mutants=("clip_without_min",)),
    dict(name="norm1.001x", norm_ratio=1.001),
    dict(name="norm2x", norm_ratio=2.0),
    dict(name="sumsq_none", sumsq="none", norm_ratio=None),
    dict(name="sumsq_zero", sumsq="zero", norm_ratio=None),
    dict(name="project_off", project=False),
]


def _adam_cases():
    out = []
    for sh in ADAM_SHAPES:
        out.append(AdamCase(name="shape" + "x".join(map(str, sh)), shape=sh,
                            mutants=("tail4_untouched",) if kernel_rows(sh)[1] >= 4 else ()))
    for sh in _HYPER_SHAPES:
        for h in _HYPERS:
            h = dict(h)
            out.append(AdamCase(name=f"{h.pop('name')}-{sh[0]}x{sh[1]}", shape=sh, **h))
    return out


ADAM_CASES = _adam_cases()


def adam_inputs(case: AdamCase):
    """-> W, G, M, V (float32, CPU, shaped case.shape) and S (float32 [1] or None)."""
    gen = _gen(case.name)
    rows, d = kernel_rows(case.shape)
    W = torch.randn(rows, d, generator=gen) * (d ** -0.5 if len(case.shape) == 2 else 0.1)
    G = torch.randn(rows, d, generator=gen) * case.gscale
    M = torch.randn(rows, d, generator=gen) * 1e-4
    V = torch.rand(rows, d, generator=gen) * 1e-7
    if rows >= 3:
        G[1] = 0.0
        G[2] = 0.0; M[2] = 0.0; V[2] = 0.0
    if case.sumsq == "zero":
        G.zero_()
    elif case.norm_ratio is not None:
        G = (G.double() * (case.norm_ratio * f32(case.max_norm) / G.double().norm())).float()
    S = None if case.sumsq == "none" else (G.double() ** 2).sum().float().reshape(1)
    return tuple(t.reshape(case.shape).contiguous() for t in (W, G, M, V)) + (S,)


UNIT_NORM_D = [1, 2, 3, 4, 5, 1023, 1024, 1025, 1028, 4100]
UNIT_NORM_EPS = float(torch.finfo(torch.float32).eps)


def unit_norm_inputs(d: int):
    """Rows scaled 1e-3 .. 1e3, a zero row (row 3) and a row whose norm is below eps (row 4)."""
    W = torch.randn(7, d, generator=_gen(f"unit{d}"))
    W[W == 0] = 1.0
    scales = torch.tensor([1e-3, 1.0, 1e3, 0.0, 1e-9, 30.0, 0.05])
    return (W * scales[:, None]).contiguous()


GRAD_SUMSQ_BIG = 4096 * 256 * 4 + 7
GRAD_SUMSQ_N = [1, 3, 4, 5, 1023, 4097, GRAD_SUMSQ_BIG]
# (n, region): that region alone carries two thirds of the sum
GRAD_SUMSQ_PLANTED = [(5, "body"), (5, "tail"), (4097, "body"), (4097, "tail"), (4097, "last_block"),
                      (GRAD_SUMSQ_BIG, "body"), (GRAD_SUMSQ_BIG, "tail"), (GRAD_SUMSQ_BIG, "stride2"),
                      (GRAD_SUMSQ_BIG, "last_block")]


def grad_sumsq_region(n: int, region: str) -> slice:
    """The float indices of a structural region of grad_sumsq_kernel."""
    n4, grid, _ = grad_sumsq_grid(n)
    if region == "body":
        return slice(0, n4 * 4)
    if region == "tail":
        return slice(n4 * 4, n)
    if region == "stride2":                      # reached only by a thread's second grid-stride trip
        assert n4 > grid * 256
        return slice(grid * 256 * 4, n4 * 4)
    if region == "last_block":                   # the first trip of workgroup grid - 1
        return slice((grid - 1) * 256 * 4, min(grid * 256, n4) * 4)
    raise ValueError(region)


def plant(x: torch.Tensor, region: slice, squares: bool) -> torch.Tensor:
    """Scale x[region] so that it carries two thirds of sum(x^2) (squares) or of sum(|x|)."""
    x = x.clone()
    mass = (lambda t: float((t.double() ** 2).sum())) if squares else (lambda t: float(t.double().abs().sum()))
    inside = mass(x[region])
    rest = mass(x) - inside
    assert inside > 0
    if rest > 0:
        f = 2 * rest / inside
        x[region] *= math.sqrt(f) if squares else f
    return x


def grad_sumsq_inputs(n: int, region: Optional[str] = None) -> torch.Tensor:
    x = torch.randn(n, generator=_gen(f"gss{n}")) * 1e-3
    x[x == 0] = 1e-3
    return plant(x, grad_sumsq_region(n, region), True) if region else x


SUM_N = [1, 3, 1023, 1024, 4097, 131077]


def sum_inputs(n: int, tail: bool = False) -> torch.Tensor:
    x = torch.randn(n, generator=_gen(f"sum{n}")) ** 2 + 0.01          # per-row squared norms: positive
    return plant(x, slice(n // 4 * 4, n), False) if tail and n % 4 else x


WRS_PATTERNS = ["dense", "two_thirds_zero", "group_zero", "all_zero", "last_row_only"]


def _wrs_cases():
    Ns, ds = [1, 7, 64, 65, 100, 4096, 4097, 8333], [4100, 1028, 512, 4]
    out = [(N, ds[i % 4], (-1.0, 0.5)[i % 2], "dense") for i, N in enumerate(Ns)]
    out += [(100, d, (0.5, -1.0)[i % 2], "two_thirds_zero") for i, d in enumerate(ds)]
    for i, p in enumerate(WRS_PATTERNS):
        out += [(4097, 512, (-1.0, 0.5)[i % 2], p), (200, 1028, (0.5, -1.0)[i % 2], p), (8333, 4, -1.0, p)]
    return list(dict.fromkeys(out))


WRS_CASES = _wrs_cases()


def wrs_inputs(N: int, d: int, pattern: str):
    """W [N, d] and s [N]; rows with s == 0 hold NaN and +-inf (they are not to be read)."""
    gen = _gen(f"wrs{N}x{d}{pattern}")
    W = torch.randn(N, d, generator=gen) / d ** 0.5
    s = torch.randn(N, generator=gen)
    s[s == 0] = 1.0
    if pattern == "two_thirds_zero":
        s[torch.arange(N) % 3 != 1] = 0.0
    elif pattern == "group_zero":
        s[64:128] = 0.0
    elif pattern == "all_zero":
        s.zero_()
    elif pattern == "last_row_only":
        s[:-1] = 0.0
    dead = (s == 0).nonzero().reshape(-1)
    W[dead[0::3]] = float("nan")
    W[dead[1::3]] = float("inf")
    W[dead[2::3]] = float("-inf")
    return W.contiguous(), s
