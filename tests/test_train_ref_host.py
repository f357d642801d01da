"""tests/train_ref.py on the CPU: the float64 restatement equals float64 torch, an independent float32 evaluation lies inside
every bound of every case the GPU file runs (test_gpu_train_passes.py), the bounds are tight enough to mean something, and
each of a list of nearly-correct optimisers is rejected by the same checking function on the case named for it."""
import math

import numpy as np
import pytest
import torch

import train_ref as tr

F32 = torch.float32


def _t(x):
    return torch.tensor(x, dtype=F32)


# ---- float32 restatements: plain torch.sum (a pairwise / vectorised order, not the kernels') -----------------------------------
def adam_f32(W, G, M, V, step, lr, betas=(0.9, 0.999), eps=1e-8, total_sumsq=None, max_norm=1.0, project=False,
             renorm_eps=None, mutant=None):
    shape = W.shape
    rows, d = tr.kernel_rows(shape)
    W, G, M, V = (t.reshape(rows, d).clone() for t in (W, G, M, V))
    b1, b2, eps_t, lr_t = _t(betas[0]), _t(betas[1]), _t(eps), _t(lr)
    c = _t(1.0)
    if total_sumsq is not None:
        den = torch.sqrt(total_sumsq.reshape(()).to(F32))
        if mutant != "clip_without_1e-6":
            den = den + _t(1e-6)
        c = _t(max_norm) / den
        if mutant != "clip_without_min":
            c = torch.minimum(c, _t(1.0))
    g0 = G * c
    g = g0 - (g0 * W).sum(1, keepdim=True) * W if project else g0
    gv = g0 if mutant == "v_from_unprojected" else g
    m1 = M + (g - M) * (_t(1.0) - b1)
    v1 = b2 * V + (_t(1.0) - b2) * gv * gv
    t = step - 1 if mutant == "bc_at_step_minus_1" else step
    bc1 = _t(1.0 - float(b1) ** t)
    bc2 = 1.0 - float(b2) ** t
    bc2s = _t(bc2 if mutant == "no_sqrt_bc2" else math.sqrt(bc2))
    if mutant == "eps_before_bc2":
        denom = (torch.sqrt(v1) + eps_t) / bc2s
    else:
        denom = torch.sqrt(v1) / bc2s + eps_t
    w1 = W - (lr_t / bc1) * (m1 / denom)
    if mutant == "tail4_untouched":
        w1[:, -4:], m1[:, -4:], v1[:, -4:] = W[:, -4:], M[:, -4:], V[:, -4:]
    if renorm_eps is not None:
        w1 = unit_norm_f32(w1, renorm_eps)
    return tuple(x.reshape(shape) for x in (w1, m1, v1))


def unit_norm_f32(W, eps):
    return W * (_t(1.0) / (torch.sqrt((W * W).sum(1, keepdim=True)) + _t(eps)))


def grad_sumsq_f32(g, accum=0.0, mutant=None):
    if mutant == "drop_tail":
        g = g[: g.numel() // 4 * 4]
    return _t(accum) + (g * g).sum()


def sum_f32(v, accum=0.0):
    return _t(accum) + v.sum()


def wrs_f32(W, s, scale, mutant=None):
    live = s != 0
    if mutant == "drop_last_partial_group":
        live = live & (torch.arange(s.numel()) < s.numel() // 64 * 64)
    if not bool(live.any()):
        return torch.zeros(W.shape[1])
    return _t(scale) * (s[live][:, None] * W[live]).sum(0)


def _check_adam(case, got, renorm_eps=None):
    W, G, M, V, S = tr.adam_inputs(case)
    ref, bnd = tr.adam_rows(W, G, M, V, case.step, case.lr, total_sumsq=S, renorm_eps=renorm_eps, **case.kwargs())
    return [tr.assert_within(g, r, b, f"{case.name} {n}") for g, r, b, n in zip(got, ref, bnd, "WMV")]


def _run_adam_f32(case, renorm_eps=None, mutant=None):
    W, G, M, V, S = tr.adam_inputs(case)
    return adam_f32(W, G, M, V, case.step, case.lr, total_sumsq=S, renorm_eps=renorm_eps, mutant=mutant, **case.kwargs())


_IDS = [c.name for c in tr.ADAM_CASES]


# ---- the reference against float64 torch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyper", [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0),
                                   dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-3, max_norm=0.5)], ids=["default", "other"])
def test_reference_equals_float64_torch_over_three_steps(hyper):
    """clip_grad_norm_ -> projection -> torch.optim.Adam in float64 on a matrix and a bias vector, three consecutive steps, then
    the row renorm; the hyper-parameters are the float32 values the kernels receive.  1e-12 relative."""
    lr, eps, mn = tr.f32(hyper["lr"]), tr.f32(hyper["eps"]), tr.f32(hyper["max_norm"])
    betas = (tr.f32(hyper["betas"][0]), tr.f32(hyper["betas"][1]))
    gen = torch.Generator().manual_seed(5)
    N, d = 6, 40
    W0 = (torch.randn(N, d, generator=gen) / d ** 0.5).double()
    b0 = torch.randn(N, generator=gen).double()
    Wr, br = torch.nn.Parameter(W0.clone()), torch.nn.Parameter(b0.clone())
    opt = torch.optim.Adam([Wr, br], lr=lr, betas=betas, eps=eps)
    W, b = W0.clone(), b0.clone()
    mW, vW, mb, vb = (torch.zeros_like(t) for t in (W, W, b, b))
    close = lambda a, r: torch.testing.assert_close(a, r, rtol=1e-12, atol=0.0)
    for step in range(1, 4):
        gW = (torch.randn(N, d, generator=gen) * (0.3 if step != 2 else 1e-3)).double()      # clip active, inactive, active
        gb = (torch.randn(N, generator=gen) * (0.3 if step != 2 else 1e-3)).double()
        Wr.grad, br.grad = gW.clone(), gb.clone()
        torch.nn.utils.clip_grad_norm_([Wr, br], mn)
        along = (Wr.grad * Wr.data).sum(dim=1, keepdim=True)
        Wr.grad -= along * Wr.data
        opt.step()
        S = float((gW ** 2).sum() + (gb ** 2).sum())
        kw = dict(betas=betas, eps=eps, total_sumsq=S, max_norm=mn)
        (W, mW, vW), _ = tr.adam_rows(W, gW, mW, vW, step, lr, project=True, **kw)
        (b, mb, vb), _ = tr.adam_rows(b, gb, mb, vb, step, lr, **kw)
        close(W, Wr.data); close(b, br.data)
        close(mW, opt.state[Wr]["exp_avg"]); close(vW, opt.state[Wr]["exp_avg_sq"])
        close(mb, opt.state[br]["exp_avg"]); close(vb, opt.state[br]["exp_avg_sq"])
    re = tr.UNIT_NORM_EPS
    (Wn, _, _), _ = tr.adam_rows(W, gW, mW, vW, 4, lr, project=True, renorm_eps=re, **kw)
    (Wp, _, _), _ = tr.adam_rows(W, gW, mW, vW, 4, lr, project=True, **kw)
    close(Wn, Wp / (Wp.norm(dim=1, keepdim=True) + re))
    close(tr.unit_norm_rows(Wp, re)[0], Wp / (Wp.norm(dim=1, keepdim=True) + re))


def test_reference_reductions_equal_float64_torch():
    g = tr.grad_sumsq_inputs(4097)
    assert tr.grad_sumsq(g, 0.25)[0] == pytest.approx(0.25 + float((g.double() ** 2).sum()), rel=1e-12)
    assert tr.sum(g, -0.5)[0] == pytest.approx(-0.5 + float(g.double().sum()), rel=1e-12)
    W, s = tr.wrs_inputs(100, 512, "two_thirds_zero")
    live = s != 0
    ref = -(s[live].double() @ W[live].double())
    torch.testing.assert_close(tr.weighted_row_sum(W, s, -1.0)[0], ref, rtol=1e-12, atol=1e-15)


# ---- soundness: a correct float32 evaluation in another order is inside every bound -------------------------------------------
@pytest.mark.parametrize("case", tr.ADAM_CASES, ids=_IDS)
def test_float32_adam_restatement_is_inside_the_bounds(case):
    ratios = _check_adam(case, _run_adam_f32(case))
    print(f"{case.name}: max err/bound W {ratios[0]:.3f} M {ratios[1]:.3f} V {ratios[2]:.3f}")
    if len(case.shape) == 2:
        re = tr.UNIT_NORM_EPS
        r = _check_adam(case, _run_adam_f32(case, renorm_eps=re), renorm_eps=re)
        print(f"{case.name} + renorm: max err/bound W {r[0]:.3f}")


@pytest.mark.parametrize("case", tr.ADAM_CASES, ids=_IDS)
def test_adam_bounds_are_not_vacuous(case):
    """At least 99 % of the elements of every case have dw <= 0.01 lr (a hundredth of one Adam update)."""
    W, G, M, V, S = tr.adam_inputs(case)
    _, (dW, _, _) = tr.adam_rows(W, G, M, V, case.step, case.lr, total_sumsq=S, **case.kwargs())
    share = float((dW > 0.01 * case.lr).double().mean())
    print(f"{case.name}: {share:.4%} of the elements have dw > 0.01 lr; largest dw / lr {float(dW.max()) / case.lr:.3e}")
    assert share <= 0.01


def test_float32_reduction_restatements_are_inside_the_bounds():
    eps = tr.UNIT_NORM_EPS
    for d in tr.UNIT_NORM_D:
        W = tr.unit_norm_inputs(d)
        ref, bnd = tr.unit_norm_rows(W, eps)
        tr.assert_within(unit_norm_f32(W, eps), ref, bnd, f"unit_norm d={d}")
    for n, region in [(n, None) for n in tr.GRAD_SUMSQ_N] + tr.GRAD_SUMSQ_PLANTED:
        g = tr.grad_sumsq_inputs(n, region)
        for acc in (0.0, 0.5 * float((g.double() ** 2).sum())):
            ref, bnd = tr.grad_sumsq(g, tr.f32(acc))
            tr.assert_within(grad_sumsq_f32(g, acc), ref, bnd, f"grad_sumsq n={n} {region}")
    for n in tr.SUM_N:
        for tail in (False, True):
            v = tr.sum_inputs(n, tail)
            ref, bnd = tr.sum(v, 3.0)
            tr.assert_within(sum_f32(v, 3.0), ref, bnd, f"sum n={n}")
    for N, d, scale, pattern in tr.WRS_CASES:
        W, s = tr.wrs_inputs(N, d, pattern)
        ref, bnd = tr.weighted_row_sum(W, s, scale)
        tr.assert_within(wrs_f32(W, s, scale), ref, bnd, f"weighted_row_sum {N}x{d} {pattern}")


def test_planted_regions_carry_half_of_the_sum():
    for n, region in tr.GRAD_SUMSQ_PLANTED:
        g = tr.grad_sumsq_inputs(n, region).double()
        assert float((g[tr.grad_sumsq_region(n, region)] ** 2).sum()) >= 0.5 * float((g ** 2).sum()), (n, region)
    for n in tr.SUM_N:
        if n % 4:
            v = tr.sum_inputs(n, True).double()
            assert float(v[n // 4 * 4:].sum()) >= 0.5 * float(v.sum()), n
    n4, grid, trips = tr.grad_sumsq_grid(tr.GRAD_SUMSQ_BIG)
    assert grid == 4096 and trips == 2 and tr.GRAD_SUMSQ_BIG % 4 == 3


# ---- power: nearly-correct optimisers are rejected ---------------------------------------------------------------------------
_MUTANTS = ["no_sqrt_bc2", "eps_before_bc2", "bc_at_step_minus_1", "clip_without_min", "clip_without_1e-6",
            "v_from_unprojected", "tail4_untouched"]
_POWER = [(c, m) for c in tr.ADAM_CASES for m in c.mutants]


def test_every_adam_mutant_has_a_case():
    assert {m for _, m in _POWER} == set(_MUTANTS)


@pytest.mark.parametrize("case,mutant", _POWER, ids=[f"{m}@{c.name}" for c, m in _POWER])
def test_adam_mutant_is_rejected_on_its_case(case, mutant):
    with pytest.raises(AssertionError, match="outside their bound"):
        _check_adam(case, _run_adam_f32(case, mutant=mutant))
    if len(case.shape) == 2:                  # ... and through the composed bound of the fused entry
        re = tr.UNIT_NORM_EPS
        with pytest.raises(AssertionError, match="outside their bound"):
            _check_adam(case, _run_adam_f32(case, renorm_eps=re, mutant=mutant), renorm_eps=re)


@pytest.mark.parametrize("N,d", [(100, 4100), (65, 4), (8333, 4)])
def test_weighted_row_sum_without_its_last_partial_group_is_rejected(N, d):
    W, s = tr.wrs_inputs(N, d, "dense")
    ref, bnd = tr.weighted_row_sum(W, s, -1.0)
    with pytest.raises(AssertionError, match="outside their bound"):
        tr.assert_within(wrs_f32(W, s, -1.0, mutant="drop_last_partial_group"), ref, bnd, "mutant")


@pytest.mark.parametrize("n", [5, 4097, tr.GRAD_SUMSQ_BIG])
def test_grad_sumsq_without_its_scalar_tail_is_rejected(n):
    g = tr.grad_sumsq_inputs(n, "tail")
    ref, bnd = tr.grad_sumsq(g, 0.0)
    with pytest.raises(AssertionError, match="outside their bound"):
        tr.assert_within(grad_sumsq_f32(g, mutant="drop_tail"), ref, bnd, "mutant")
    g = tr.grad_sumsq_inputs(n)                      # ... and even unplanted, where the tail is an ordinary share of the sum
    if n < 100:
        ref, bnd = tr.grad_sumsq(g, 0.0)
        with pytest.raises(AssertionError, match="outside their bound"):
            tr.assert_within(grad_sumsq_f32(g, mutant="drop_tail"), ref, bnd, "mutant")


def test_a_zero_bound_demands_equality():
    z = torch.zeros(3, dtype=torch.float64)
    assert tr.assert_within(torch.zeros(3), z, z) == 0.0
    with pytest.raises(AssertionError):
        tr.assert_within(torch.tensor([0.0, 1e-30, 0.0]), z, z)
    with pytest.raises(AssertionError):
        tr.assert_within(torch.tensor([0.0, float("nan"), 0.0]), z, z + 1.0)
