"""The parameter-sized passes of the training step (csrc/train.hip: adam_rows_, its fused renorm entry, unit_norm_rows_,
grad_sumsq_, sum_into_, weighted_row_sum) against the float64 restatement of tests/train_ref.py.  EVERY element is compared
with its own derived bound -- nothing is excluded -- on shapes that put the load on a structural edge of each kernel: the
scalar path and the scalar tail, the last live thread of a trip, the grid-stride wrap, partial row groups, the KEEP = 8
register window and the d > 8192 hand-back of the fused kernel, the [rows, 1024] view of bias vectors.  The inputs, the table
of cases and the proof that the bounds reject nearly-correct optimisers are in train_ref.py / test_train_ref_host.py.

Each test prints, per case, the largest ratio of observed error to bound.

Out of scope: magnitudes at which g^2 or a row's sum of squares overflows or leaves the normal float32 range."""
import gc

import pytest
import torch

import train_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_after():
    yield
    from msae import ops

    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


_IDS = [c.name for c in tr.ADAM_CASES]
_CASES_2D = [c for c in tr.ADAM_CASES if len(c.shape) == 2]


def _special_rows(case, W0, G0, M0, V0, W, M, V, renormed):
    """Rows without a gradient but with moments still move and decay; rows with G = M = V = 0 stay bit-identical."""
    rows, d = tr.kernel_rows(case.shape)
    if rows < 3:
        return
    v = lambda t: t.reshape(rows, d).cpu()
    W0, G0, M0, V0, W, M, V = map(v, (W0, G0, M0, V0, W, M, V))
    assert not G0[1].any() and M0[1].any()
    assert bool((M[1].abs() < M0[1].abs()).all()) and bool((V[1] < V0[1])[V0[1] > 0].all())
    assert torch.equal(M[2], M0[2]) and torch.equal(V[2], V0[2]) and not M[2].any() and not V[2].any()
    if not renormed:
        assert bool((W[1] != W0[1]).any()), "a row with moments but no gradient did not move"
        assert torch.equal(W[2], W0[2]), "a row with G = M = V = 0 changed"


@pytest.mark.parametrize("case", tr.ADAM_CASES, ids=_IDS)
def test_adam_rows_within_float64_bounds(dev, case):
    """One step from warm moments: W, M and V within the bounds of train_ref.adam_rows, element by element."""
    from msae import ops

    W0, G0, M0, V0, S = tr.adam_inputs(case)
    ref, bnd = tr.adam_rows(W0, G0, M0, V0, case.step, case.lr, total_sumsq=S, **case.kwargs())
    W, G, M, V = (t.to(dev) for t in (W0, G0, M0, V0))
    ops.adam_rows_(W, G, M, V, case.step, case.lr, total_sumsq=None if S is None else S.to(dev), **case.kwargs())
    assert torch.equal(G.cpu(), G0), "the gradient is an input"
    ratios = [tr.assert_within(g, r, b, f"{case.name} {n}") for g, r, b, n in zip((W, M, V), ref, bnd, "WMV")]
    print(f"\nadam_rows_ {case.name}: max err/bound W {ratios[0]:.3f} M {ratios[1]:.3f} V {ratios[2]:.3f}")
    _special_rows(case, W0, G0, M0, V0, W, M, V, False)


@pytest.mark.parametrize("case", _CASES_2D, ids=[c.name for c in _CASES_2D])
def test_fused_renorm_entry_equals_the_two_passes_and_the_composed_bound(dev, case):
    """adam_rows_(renorm_eps=eps), no refresh buffer: bit for bit adam_rows_ then unit_norm_rows_ (one row, the scalar path and
    the d > 8192 hand-back included), and within the composed float64 bound."""
    from msae import ops

    re = tr.UNIT_NORM_EPS
    W0, G0, M0, V0, S = tr.adam_inputs(case)
    ref, bnd = tr.adam_rows(W0, G0, M0, V0, case.step, case.lr, total_sumsq=S, renorm_eps=re, **case.kwargs())
    Sd = None if S is None else S.to(dev)
    W, G, M, V = (t.to(dev) for t in (W0, G0, M0, V0))
    W2, M2, V2 = W.clone(), M.clone(), V.clone()
    ops.adam_rows_(W, G, M, V, case.step, case.lr, total_sumsq=Sd, **case.kwargs())
    ops.unit_norm_rows_(W, re)
    ops.adam_rows_(W2, G, M2, V2, case.step, case.lr, total_sumsq=Sd, renorm_eps=re, **case.kwargs())
    assert torch.equal(W, W2) and torch.equal(M, M2) and torch.equal(V, V2)
    ratios = [tr.assert_within(g, r, b, f"{case.name} fused {n}") for g, r, b, n in zip((W2, M2, V2), ref, bnd, "WMV")]
    print(f"\nadam_rows_ + renorm {case.name}: max err/bound W {ratios[0]:.3f} M {ratios[1]:.3f} V {ratios[2]:.3f}")
    _special_rows(case, W0, G0, M0, V0, W2, M2, V2, True)


@pytest.mark.parametrize("d", tr.UNIT_NORM_D)
def test_unit_norm_rows_within_float64_bounds(dev, d):
    from msae import ops

    W0 = tr.unit_norm_inputs(d)
    ref, bnd = tr.unit_norm_rows(W0, tr.UNIT_NORM_EPS)
    W = ops.unit_norm_rows_(W0.to(dev), tr.UNIT_NORM_EPS)
    ratio = tr.assert_within(W, ref, bnd, f"unit_norm_rows_ d={d}")
    print(f"\nunit_norm_rows_ d={d}: max err/bound {ratio:.3f}")
    W = W.cpu()
    assert not W[3].any(), "a zero row must stay zero"
    assert float(W0[4].double().norm()) < tr.UNIT_NORM_EPS and bool(W[4].any())       # the row below eps is scaled by ~1 / eps
    for r in (0, 1, 2, 5, 6):                              # |row| -> |row| / (|row| + eps): short of 1 by eps / |row| (1e-4 at 1e-3)
        n = float(W0[r].double().norm())
        assert abs(float(W[r].double().norm()) - n / (n + tr.UNIT_NORM_EPS)) < 1e-5


_BIG = {}


def _grad_sumsq_case(dev, n, region):
    """The 16 MB case is generated once; its planted variants rescale one region of it."""
    if n not in _BIG:
        _BIG.clear()
        _BIG[n] = tr.grad_sumsq_inputs(n)
    g = tr.plant(_BIG[n], tr.grad_sumsq_region(n, region), True) if region else _BIG[n]
    return g, g.to(dev)


@pytest.mark.parametrize("n,region", [(n, None) for n in tr.GRAD_SUMSQ_N] + tr.GRAD_SUMSQ_PLANTED)
def test_grad_sumsq_within_float64_bounds(dev, n, region):
    """From zero, onto a nonzero accumulator, and called twice; `region` (when given) alone carries two thirds of the sum, so a
    kernel that drops it is off by far more than any tolerance."""
    from msae import ops

    g0, g = _grad_sumsq_case(dev, n, region)
    total = float((g0.double() ** 2).sum())
    ratios = []
    for start in (0.0, 0.5 * total):
        acc = torch.full((1,), start, device=dev)
        start = float(acc)
        ops.grad_sumsq_(acc, g)
        ref, bnd = tr.grad_sumsq(g0, start)
        ratios.append(tr.assert_within(acc, [ref], [bnd], f"grad_sumsq_ n={n} {region} from {start}"))
        once = float(acc)
        ops.grad_sumsq_(acc, g)                                # the second call reads the float32 value the first one left
        ref, bnd = tr.grad_sumsq(g0, once)
        ratios.append(tr.assert_within(acc, [ref], [bnd], f"grad_sumsq_ n={n} {region} second call"))
    print(f"\ngrad_sumsq_ n={n} {region}: max err/bound {max(ratios):.4f}")


@pytest.mark.parametrize("n", tr.SUM_N)
@pytest.mark.parametrize("tail", [False, True], ids=["plain", "tail_planted"])
def test_sum_into_within_float64_bounds(dev, n, tail):
    from msae import ops

    v0 = tr.sum_inputs(n, tail)
    v = v0.to(dev)
    ratios, outs = [], []
    for start in (0.0, 3.0):
        for _ in range(2):
            acc = torch.full((1,), start, device=dev)
            ops.sum_into_(acc, v)
            outs.append(acc.cpu())
        assert torch.equal(outs[-1], outs[-2]), "sum_into_ is not reproducible"
        ref, bnd = tr.sum(v0, start)
        ratios.append(tr.assert_within(acc, [ref], [bnd], f"sum_into_ n={n} from {start}"))
    print(f"\nsum_into_ n={n} tail={tail}: max err/bound {max(ratios):.3f}")


@pytest.mark.parametrize("N,d,scale,pattern", tr.WRS_CASES)
def test_weighted_row_sum_within_float64_bounds(dev, N, d, scale, pattern):
    """Rows with s == 0 hold NaN and inf: they are not read, the output is finite (assert_within) and within the bound."""
    from msae import ops

    W0, s0 = tr.wrs_inputs(N, d, pattern)
    ref, bnd = tr.weighted_row_sum(W0, s0, scale)
    W, s = W0.to(dev), s0.to(dev)
    out = ops.weighted_row_sum(W, s, scale)
    ratio = tr.assert_within(out, ref, bnd, f"weighted_row_sum {N}x{d} {pattern}")
    print(f"\nweighted_row_sum N={N} d={d} scale={scale} {pattern}: max err/bound {ratio:.3f}")
    if pattern == "all_zero":
        assert bool((out == 0).all())
    else:
        assert bool(out.any())
    assert torch.equal(out, ops.weighted_row_sum(W, s, scale)), "weighted_row_sum is not reproducible"


def test_sparse_encode_backward_at_a_width_that_is_no_multiple_of_four(dev):
    """d = 50: the d % 4 guard of _SparseEncode.backward takes the gather branch for the b_dec gradient.  The gradients of
    W_enc, b_enc and b_dec against a float64 dense restatement on the same selection.  Bound: every gradient element is a sum
    of at most T k products g[t, j] * operand, each operand (a = x - b_dec) rounded once: (T k + 3) u sum |terms|, times 2."""
    from msae import ops

    d, N, T, k = 50, 100, 9, 4
    gen = torch.Generator().manual_seed(31)
    W0 = torch.randn(N, d, generator=gen) / d ** 0.5
    b0 = torch.randn(N, generator=gen) * 0.05
    bd0 = torch.randn(d, generator=gen) * 0.1
    x0 = torch.randn(T, d, generator=gen)
    go0 = torch.randn(T, k, generator=gen)
    W, b, bd = (t.to(dev).requires_grad_() for t in (W0, b0, bd0))
    (acts, idx), = ops.sparse_encode(x0.to(dev), W, b, bd, k)
    (acts * go0.to(dev)).sum().backward()
    idx = idx.cpu().long()
    assert bool((acts > 0).all())
    Wr, br, bdr = (t.double().requires_grad_() for t in (W0, b0, bd0))
    pre = torch.relu(torch.nn.functional.linear(x0.double() - bdr, Wr, br))
    (pre.gather(1, idx) * go0.double()).sum().backward()
    assert bool((pre.gather(1, idx) > 0).all())
    depth = tr.SAFETY * (T * k + 3) * tr.U
    a = (x0.double() - bd0.double()).abs()
    g = go0.double().abs()
    flat = idx.reshape(-1)
    bW = torch.zeros(N, d, dtype=torch.float64).index_add_(0, flat, (g[:, :, None] * a[:, None, :]).reshape(-1, d))
    bb = torch.zeros(N, dtype=torch.float64).index_add_(0, flat, g.reshape(-1))
    bbd = (g[:, :, None] * W0.double().abs()[idx]).sum((0, 1))
    for name, got, ref, bnd in (("W_enc", W.grad, Wr.grad, bW), ("b_enc", b.grad, br.grad, bb), ("b_dec", bd.grad, bdr.grad, bbd)):
        ratio = tr.assert_within(got, ref, depth * bnd, f"sparse_encode backward {name}")
        print(f"\nsparse_encode backward d={d} {name}: max err/bound {ratio:.3f}")
