"""tests/lion_ref.py on the CPU: the float64 restatement equals a literal float64 torch loop, an independent float32 numpy
evaluation passes the acceptance rule in every case the GPU file runs (test_gpu_lion.py), the share of undecided signs is under
the cap in every case from float64 alone, and each of a list of near-correct optimisers is rejected by the same checking
functions on the cases named for it."""
import numpy as np
import pytest
import torch

import lion_ref as lr_
import train_ref as tr

F = np.float32
EPS32 = float(torch.finfo(torch.float32).eps)


def _fma32(a, b, c):
    """float32 fma: the product of two float32 values is exact in float64; one float64 add, then the rounding to float32
    (a double rounding in rare half-way cases, which the acceptance rule's bounds cover)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)


def lion_f32(W, G, M, lr, betas=(0.9, 0.99), total_sumsq=None, max_norm=1.0, project=False, renorm_eps=None, mutant=None):
    """The pass in numpy float32, operation for operation as include/msae.h states it; the row sum in numpy's order."""
    shape = W.shape
    rows, d = tr.kernel_rows(shape)
    w, g0, m = (t.numpy().astype(F).reshape(rows, d).copy() for t in (W, G, M))
    c = F(1.0)
    if total_sumsq is not None:
        c = F(max_norm) / (np.sqrt(F(float(total_sumsq))) + F(1e-6))
        if mutant != "clip_without_min":
            c = min(c, F(1.0))
    g0 = g0 * c
    late = mutant == "projection_after_momentum"

    def proj(v):
        return v - (v * w).sum(1, keepdims=True, dtype=F) * w

    g = proj(g0) if project and not late else g0
    ob1, ob2 = F(1.0) - F(betas[0]), F(1.0) - F(betas[1])
    t = g - m
    u = _fma32(t, ob1, m)
    m1 = _fma32(t, ob1 if mutant == "m_with_beta1" else ob2, m)
    if project and late:
        u = proj(u)
    src = {"sign_of_m_prime": m1, "sign_of_g": g}.get(mutant, u)
    s = np.sign(src).astype(F)
    if mutant == "sign_of_zero_is_plus":
        s = np.where(src == 0, F(1.0), s).astype(F)
    step = F(lr)
    if mutant == "bias_correction":
        step = F(lr) / F(1.0 - float(F(betas[0])) ** 2)                  # lr / (1 - beta1^t) at t = 2
    w1 = (w - step * (u if mutant == "no_sign" else s)).astype(F)
    if renorm_eps is not None:
        w1 = (w1 * (F(1.0) / (np.sqrt((w1 * w1).sum(1, keepdims=True, dtype=F)) + F(renorm_eps)))).astype(F)
    return torch.from_numpy(w1.reshape(shape)), torch.from_numpy(m1.reshape(shape))


def _check(case, mutant=None, renorm=False):
    """The checks of test_gpu_lion.py on lion_f32's result -> the undecided share."""
    W, G, M, S = lr_.lion_inputs(case)
    (_, M1, u, _), b = lr_.lion_rows(W, G, M, case.lr, total_sumsq=S, **case.kwargs())
    W1, M1_got = lion_f32(W, G, M, case.lr, total_sumsq=S, mutant=mutant, **case.kwargs())
    s, share = lr_.check_w(W1, W, case.lr, u, b.du, case.name)
    tr.assert_within(M1_got, M1, b.dM, f"{case.name} M")
    if renorm:
        Wn, _ = lion_f32(W, G, M, case.lr, total_sumsq=S, renorm_eps=EPS32, mutant=mutant, **case.kwargs())
        want, bound = lr_.renorm_of(W, s, case.lr, EPS32)
        tr.assert_within(Wn, want, bound, f"{case.name} W after the renorm")
    return share


def _literal(W, G, M, lr, betas, S, max_norm, project):
    """Lion as the paper writes it, row by row in float64 torch: u = b1 m + (1 - b1) g, w -= lr sign(u), m = b2 m + (1 - b2) g."""
    rows, d = tr.kernel_rows(W.shape)
    w, g, m = (t.double().reshape(rows, d) for t in (W, G, M))
    b1, b2, lr, mn = tr.f32(betas[0]), tr.f32(betas[1]), tr.f32(lr), tr.f32(max_norm)
    c = 1.0 if S is None else min(1.0, mn / (float(S) ** 0.5 + 1e-6))
    W1, M1, Us = [], [], []
    for r in range(rows):
        gr = c * g[r]
        if project:
            gr = gr - torch.dot(gr, w[r]) * w[r]
        ur = b1 * m[r] + (1.0 - b1) * gr
        W1.append(w[r] - lr * torch.sign(ur))
        M1.append(b2 * m[r] + (1.0 - b2) * gr)
        Us.append(ur)
    return tuple(torch.stack(x).reshape(W.shape) for x in (W1, M1, Us))


@pytest.mark.parametrize("case", lr_.LION_CASES, ids=lambda c: c.name)
def test_restatement_equals_a_literal_float64_loop(case):
    W, G, M, S = lr_.lion_inputs(case)
    (W1, M1, u, s), _ = lr_.lion_rows(W, G, M, case.lr, total_sumsq=S, **case.kwargs())
    Wl, Ml, ul = _literal(W, G, M, case.lr, case.betas, S, case.max_norm, case.kwargs()["project"])
    assert float((M1 - Ml).abs().max()) <= 1e-12 and float((u - ul).abs().max()) <= 1e-12
    firm = ul.abs() > 1e-12                      # (the two ways of writing the interpolation may round an exact 0 apart)
    assert torch.equal(W1[firm], Wl[firm])
    assert bool((s[firm] == torch.sign(ul[firm])).all())
    assert float((W1 - Wl).abs().max()) <= 2 * tr.f32(case.lr) + 1e-12


@pytest.mark.parametrize("case", lr_.LION_CASES, ids=lambda c: c.name)
def test_float32_evaluation_passes_and_the_cap_holds(case):
    W, G, M, S = lr_.lion_inputs(case)
    (_, _, u, _), b = lr_.lion_rows(W, G, M, case.lr, total_sumsq=S, **case.kwargs())
    share64 = lr_.undecided_share(u, b.du)
    assert share64 <= lr_.UNDECIDED_CAP, (case.name, share64)
    share = _check(case, renorm=len(case.shape) == 2)
    assert share == share64


def test_planted_rows_decide_what_they_are_there_for():
    """Row 1 (G = 0, M != 0) is decided as sign(m) with a shrinking momentum, row 2 (all zero) as an exact zero."""
    case = next(c for c in lr_.LION_CASES if c.name == "betas0.9_0.99-7x1000")
    W, G, M, S = lr_.lion_inputs(case)
    (W1, M1, u, s), b = lr_.lion_rows(W, G, M, case.lr, total_sumsq=S, **case.kwargs())
    assert bool((G[1] == 0).all()) and bool((M[1] != 0).all())
    assert bool((u[1].abs() > b.du[1]).all()) and torch.equal(s[1], torch.sign(M[1].double()))
    assert bool((M1[1].abs() < M[1].double().abs()).all())
    assert bool((u[2] == 0).all()) and bool((b.du[2] == 0).all()) and torch.equal(W1[2], W[2].double())
    W32, M32 = lion_f32(W, G, M, case.lr, total_sumsq=S, **case.kwargs())
    assert torch.equal(W32[2], W[2]) and bool((W32[1] != W[1]).all()) and bool((M32[1].abs() < M[1].abs()).all())


def test_every_mutant_is_named_by_a_case():
    named = {m for c in lr_.LION_CASES for m in c.mutants}
    assert named == set(lr_.MUTANTS)
    assert any(c.betas[0] != c.betas[1] for c in lr_.LION_CASES if "sign_of_m_prime" in c.mutants)


@pytest.mark.parametrize("case,mutant", [(c, m) for c in lr_.LION_CASES for m in c.mutants],
                         ids=lambda v: v.name if isinstance(v, lr_.LionCase) else v)
def test_near_correct_optimisers_are_rejected(case, mutant):
    with pytest.raises(AssertionError):
        _check(case, mutant)
