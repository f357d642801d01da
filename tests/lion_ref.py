"""Float64 restatement of the sign-momentum pass (csrc/train.hip: msae_lion_rows_f32; Lion, and Signum as its beta1 == beta2
case) with DERIVED bounds, the acceptance rule the GPU tests and the host tests share, and the table of cases.
tests/train_ref.py is the template: its error model (U, SAFETY, one safety factor at the end), its clip and projection
bounds, its `_renorm` and `assert_within`; hyper-parameters are evaluated at their float32 values.

        c  = min(1, max_norm / (sqrt(S) + 1e-6))       S = total_sumsq (None: c = 1)
        g  = c G ;  g -= <g, w> w  if project
        u  = m + (g - m)(1 - b1)                        the interpolated momentum that is signed
        s  = sign(u)                                    0 for u == 0
        w' = w - lr s ;  then w' /= |w'| + renorm_eps (optional)
        m' = m + (g - m)(1 - b2)                        the carried momentum

Bounds.  g is known to within dg exactly as in train_ref.adam_rows (clip 6 u c, the product u, the projection's row sum at
depth 1 + row_reduction_depth(d), its product and subtraction).  u and m' are each ONE float32 subtraction and ONE fma:

        t  = g - m            e_t  = u |t|, and 0 where g is an exact zero (the subtraction of an exact 0 is exact)
        ob = 1 - b            one float32 subtraction of two float32 values: e_ob = u |t ob|, 0 when 1 - b is itself a
                              float32 (it is for every b in [0.5, 1] and for b = 0)
        u  = fma(t, ob, m)    du = ob (dg + e_t) + e_ob + u |u|            (dm the same with b2)

W is NOT judged by a forward-error bound: a sign is a discontinuity.  The acceptance rule (`check_w`):

  * every element of the device's W' is bit-equal to float32(w - lr s) for some s in {-1, 0, 1} (numpy float32 arithmetic:
    one exact product, one rounded subtraction -- what the header documents);
  * wherever |u64| > du that s is sign(u64) (where lr is so small that candidates coincide, sign(u64) must be among the
    matching ones: that is all the bits can show);
  * where u64 == 0 and du == 0 (G = M = 0; or G = 0 with b1 = 0, where fma(-m, 1, m) is an exact 0) s is 0: W' == W bit for bit;
  * elements with |u64| <= du otherwise are UNDECIDED and accept any of the three.  Their share is capped at UNDECIDED_CAP
    per case: a condition on the cases, asserted from float64 alone (`undecided_share`), not a measurement.
With the renorm, W' is checked through the ADOPTED s: the rows float32(w - lr s) are exact inputs of train_ref._renorm
(`renorm_of`), whose bound then applies.  s comes from a run of the same pass without tails, which the bit-equality of the
fused and the separate tails licenses.

Nothing here is fitted to what a GPU produced."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from train_ref import (ADAM_SHAPES, F64, SAFETY, U, _d, _renorm, adam_inputs, assert_within, f32, kernel_rows,  # noqa: F401
                       row_reduction_depth)

UNDECIDED_CAP = 0.01


class LionBounds(NamedTuple):
    dM: torch.Tensor       # |m'_f32 - m'|, SAFETY included
    du: torch.Tensor       # |u_f32 - u|, SAFETY included: the sign of u is decided where |u| exceeds it
    dg: torch.Tensor       # |g_f32 - g| after clip and projection, SAFETY included


def _lerp(g, dg, m, b: float):
    """m + (g - m)(1 - b) and its raw bound: one float32 subtraction, the float32 1 - b, one fma."""
    ob = 1.0 - b
    t = g - m
    e_t = torch.where((g == 0) & (dg == 0), torch.zeros_like(t), U * t.abs())
    e_ob = 0.0 if f32(ob) == ob else U * (t * ob).abs()
    out = m + t * ob
    return out, ob * (dg + e_t) + e_ob + U * out.abs()


def lion_rows(W, G, M, lr: float, betas=(0.9, 0.99), total_sumsq=None, max_norm: float = 1.0, project: bool = False,
              renorm_eps: Optional[float] = None, device="cpu"):
    """-> ((W', M', u, s), LionBounds), float64, shaped like W.  W' is w - lr s (then renormalised) with s = sign(u64): what
    check_w and renorm_of judge a device result by, not a value to compare within a bound."""
    shape = W.shape
    rows, d = kernel_rows(shape)
    w, g_in, m = (_d(t, device).reshape(rows, d) for t in (W, G, M))
    assert not project or len(shape) == 2
    lr_, b1, b2, mn = f32(lr), f32(betas[0]), f32(betas[1]), f32(max_norm)
    if total_sumsq is None:
        c, dc = 1.0, 0.0
    else:
        S = float(total_sumsq)
        c_raw = mn / (math.sqrt(S) + 1e-6)
        c = min(1.0, c_raw)
        dc = 0.0 if c_raw * (1 - 8 * U) >= 1.0 else 6 * U * c
    g0 = c * g_in
    dg0 = g_in.abs() * dc + (0.0 if c == 1.0 and dc == 0.0 else U * g0.abs())     # (a product with an exact 1 is exact)
    if project:
        D = 1 + row_reduction_depth(d)
        a = (g0 * w).sum(1, keepdim=True)
        da = (w.abs() * dg0).sum(1, keepdim=True) + D * U * (g0 * w).abs().sum(1, keepdim=True)
        g = g0 - a * w
        dg = dg0 + w.abs() * da + U * (a * w).abs() + U * g.abs()
    else:
        g, dg = g0, dg0
    u, du = _lerp(g, dg, m, b1)
    m1, dm = _lerp(g, dg, m, b2)
    s = torch.sign(u)
    w1 = w - lr_ * s
    if renorm_eps is not None:
        assert len(shape) == 2
        w1, _ = _renorm(w1, torch.zeros_like(w1), f32(renorm_eps), d)
    return (tuple(x.reshape(shape) for x in (w1, m1, u, s)),
            LionBounds(*(SAFETY * x.reshape(shape) for x in (dm, du, dg))))


def undecided(u, du) -> torch.Tensor:
    """The elements whose sign float64 leaves open: |u| <= du, the exact zeros (u == 0 with du == 0) aside."""
    return (u.abs() <= du) & ~((u == 0) & (du == 0))


def undecided_share(u, du) -> float:
    return float(undecided(u, du).double().mean())


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def candidates(W, lr: float):
    """float32(w - lr s) for s = -1, 0, 1 in float32 arithmetic -> three numpy float32 arrays."""
    w = W.detach().cpu().numpy().astype(np.float32)
    lr32 = np.float32(lr)
    return tuple((w - lr32 * np.float32(s)).astype(np.float32) for s in (-1.0, 0.0, 1.0))


def check_w(W_got, W_in, lr: float, u, du, what: str = "") -> Tuple[torch.Tensor, float]:
    """The acceptance rule for the updated parameter BEFORE any renorm -> (the adopted s as float64 shaped like W, the
    undecided share).  u, du: lion_rows' float64 u and its bound."""
    got = _bits(W_got.detach().cpu().numpy())
    cand = candidates(W_in, lr)
    match = np.stack([got == _bits(c) for c in cand])                    # [3, ...]: s = -1, 0, 1
    u_np, du_np = u.detach().cpu().numpy().reshape(got.shape), du.detach().cpu().numpy().reshape(got.shape)
    assert np.isfinite(u_np).all() and np.isfinite(du_np).all(), f"{what}: non-finite reference"
    none = ~match.any(0)
    assert not none.any(), (f"{what}: {int(none.sum())} of {none.size} elements are float32(w - lr s) for no s in (-1, 0, 1); "
                            f"first at flat index {int(np.flatnonzero(none.reshape(-1))[0])}")
    sgn = np.sign(u_np).astype(np.int64)
    by_sign = np.take_along_axis(match, (sgn + 1)[None], 0)[0]            # does the candidate of sign(u64) match
    exact0 = (u_np == 0) & (du_np == 0)
    decided = (np.abs(u_np) > du_np) | exact0
    bad = decided & ~by_sign
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements moved against sign(u) where |u| > du (or moved "
                           f"at u == 0); first at flat index {int(np.flatnonzero(bad.reshape(-1))[0])}: "
                           f"u {u_np.reshape(-1)[np.flatnonzero(bad.reshape(-1))[0]]!r}")
    moved0 = exact0 & (got != _bits(W_in.detach().cpu().numpy()))
    assert not moved0.any(), f"{what}: {int(moved0.sum())} elements with G = M = 0 changed their bits"
    s = np.where(by_sign, sgn, np.where(match[1], 0, np.where(match[0], -1, 1)))
    return torch.from_numpy(s.astype(np.float64)).reshape(W_in.shape), float((~decided).mean())


def renorm_of(W_in, s, lr: float, renorm_eps: float):
    """The renormalised rows of float32(w - lr s) for an adopted s -> (float64 result, bound): exact float32 inputs of
    train_ref._renorm."""
    c = candidates(W_in, lr)
    s_np = s.detach().cpu().numpy().reshape(c[0].shape)
    pre = np.where(s_np < 0, c[0], np.where(s_np > 0, c[2], c[1]))
    w = torch.from_numpy(pre.astype(np.float64))
    out, b = _renorm(w, torch.zeros_like(w), f32(renorm_eps), w.shape[1])
    return out, SAFETY * b


# ---- the cases --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LionCase:
    """One lion_rows_ call on train_ref.adam_inputs' tensors (warm momentum M ~ 1e-4 signed, G scaled to the clip; with three
    kernel rows or more, row 1 has G == 0 and M != 0 and row 2 is all zero).  The fields adam_inputs reads are AdamCase's.
    mutants: the near-correct optimisers of test_lion_ref_host.py this case must reject."""
    name: str
    shape: Tuple[int, ...]
    lr: float = 1e-3
    betas: Tuple[float, float] = (0.9, 0.99)
    max_norm: float = 1.0
    project: bool = True
    gscale: float = 1e-3
    norm_ratio: Optional[float] = 2.0
    sumsq: str = "given"
    mutants: Tuple[str, ...] = field(default=())

    def kwargs(self):
        return dict(betas=self.betas, max_norm=self.max_norm, project=self.project and len(self.shape) == 2)


MUTANTS = ("sign_of_m_prime", "sign_of_g", "m_with_beta1", "bias_correction", "clip_without_min",
           "projection_after_momentum", "sign_of_zero_is_plus", "no_sign")

_HYPER_SHAPES = [(7, 1000), (5, 50)]
_HYPERS = [
    dict(name="betas0.9_0.99", betas=(0.9, 0.99), mutants=("sign_of_m_prime", "sign_of_g", "m_with_beta1", "bias_correction",
                                                            "sign_of_zero_is_plus", "no_sign")),
    dict(name="betas0.95_0.98", betas=(0.95, 0.98), mutants=("sign_of_m_prime", "m_with_beta1")),
    dict(name="betas0.9_0.9", betas=(0.9, 0.9), mutants=("sign_of_g", "bias_correction")),
    dict(name="betas0_0.99", betas=(0.0, 0.99), mutants=("sign_of_m_prime",)),
    dict(name="lr1e-2", lr=1e-2, mutants=("bias_correction", "no_sign")),
    dict(name="lr1e-6", lr=1e-6),
    dict(name="lr1e-10", lr=1e-10),              # below half an ulp of nearly every weight: the three candidates coincide
    dict(name="norm0.5x", norm_ratio=0.5, mutants=("clip_without_min",)),
    dict(name="norm0.999x", norm_ratio=0.999, mutants=("clip_without_min",)),
    dict(name="norm1.001x", norm_ratio=1.001),
    dict(name="norm2x", norm_ratio=2.0, mutants=("projection_after_momentum",)),
    dict(name="sumsq_none", sumsq="none", norm_ratio=None),
    dict(name="sumsq_zero", sumsq="zero", norm_ratio=None),
    dict(name="project_off", project=False),
]


def _lion_cases():
    out = [LionCase(name="shape" + "x".join(map(str, sh)), shape=sh) for sh in ADAM_SHAPES]
    for sh in _HYPER_SHAPES:
        for h in _HYPERS:
            h = dict(h)
            out.append(LionCase(name=f"{h.pop('name')}-{sh[0]}x{sh[1]}", shape=sh, **h))
    return out


LION_CASES = _lion_cases()


def lion_inputs(case: LionCase):
    """-> W, G, M (float32, CPU, shaped case.shape) and S (float32 [1] or None): train_ref.adam_inputs without its V."""
    W, G, M, _, S = adam_inputs(case)
    return W, G, M, S
