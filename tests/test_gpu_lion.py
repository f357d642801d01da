"""The sign-momentum pass on the GPU (csrc/train.hip: msae_lion_rows_f32; ops.lion_rows_; SaeTrainStep(optimizer="lion" |
"signum")) against the restatement and the acceptance rule of tests/lion_ref.py (proved on the host by
test_lion_ref_host.py: a float32 evaluation passes, eight near-correct optimisers do not).  The shapes are the smallest that
reach each edge of the kernels (train_ref.ADAM_SHAPES).  Every call of the ops runs under
torch.cuda.set_sync_debug_mode("error").

Measured on an MI355X (printed by the tests): see NOTEBOOK.md, "Sign momentum"."""
import copy
import gc

import numpy as np
import pytest
import torch

import lion_ref as L
import train_ref as tr

pytestmark = pytest.mark.gpu

EPS32 = float(torch.finfo(torch.float32).eps)


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


class _NoSync:
    """Inside: a host synchronisation raises."""

    def __enter__(self):
        torch.cuda.synchronize()
        self.prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.prev)
        return False


# ---- one pass -----------------------------------------------------------------------------------------------------------------------
def _pass(dev, case, inputs, **kw):
    from msae import ops

    W0, G0, M0, S = inputs
    W, G, M = W0.to(dev), G0.to(dev), M0.to(dev)
    Sd = None if S is None else S.to(dev)
    with _NoSync():
        ops.lion_rows_(W, G, M, case.lr, total_sumsq=Sd, **case.kwargs(), **kw)
    assert torch.equal(G.cpu(), G0), "the gradient is an input"
    return W.cpu(), M.cpu()


@pytest.mark.parametrize("case", L.LION_CASES, ids=[c.name for c in L.LION_CASES])
def test_lion_rows_passes_the_acceptance_rule(dev, case):
    """W' is float32(w - lr s) bit for bit with s = sign(u64) wherever float64 decides it and s = 0 at an exact zero, M' within
    its derived bound, the undecided share under the cap; with the renorm (matrices) W' within train_ref._renorm's bound of the
    renormalised adopted rows.  Row 1 (G = 0, M != 0) moves by sign(m) and its momentum shrinks, row 2 (all zero) keeps its
    bits.  Two identical calls give identical bits."""
    inputs = L.lion_inputs(case)
    W0, G0, M0, S = inputs
    (_, M1, u, _), b = L.lion_rows(W0, G0, M0, case.lr, total_sumsq=S, **case.kwargs())
    W, M = _pass(dev, case, inputs)
    s, share = L.check_w(W, W0, case.lr, u, b.du, case.name)
    ratio = tr.assert_within(M, M1, b.dM, f"{case.name} M")
    assert share <= L.UNDECIDED_CAP, (case.name, share)
    W_again, M_again = _pass(dev, case, inputs)
    assert torch.equal(W, W_again) and torch.equal(M, M_again), "two identical calls gave different bits"
    rn = 0.0
    if len(case.shape) == 2:
        Wn, Mn = _pass(dev, case, inputs, renorm_eps=EPS32)
        assert torch.equal(Mn, M), "the renorm tail changed the momentum"
        want, bound = L.renorm_of(W0, s, case.lr, EPS32)
        rn = tr.assert_within(Wn, want, bound, f"{case.name} W after the renorm")
    print(f"\nlion_rows_ {case.name}: undecided share {share:.2e}; max err/bound M {ratio:.3f} renorm {rn:.3f}")
    rows, d = tr.kernel_rows(case.shape)
    if rows >= 3:
        Wh, W0h, Mh, M0h = (t.reshape(rows, d) for t in (W, W0, M, M0))
        assert not G0.reshape(rows, d)[1].any() and bool((M0h[1] != 0).all())
        if case.betas[0] > 0:
            down, _, up = L.candidates(W0h[1], case.lr)            # float32(w + lr), w, float32(w - lr)
            want = torch.from_numpy(np.where(M0h[1].numpy() < 0, down, up))
            assert torch.equal(Wh[1], want), "a row with a momentum and no gradient moves by sign(m)"
        else:                                       # u = fma(-m, 1, m) is an exact zero
            assert torch.equal(Wh[1], W0h[1])
        assert bool((Mh[1].abs() < M0h[1].abs()).all()), "the momentum of a row without a gradient must shrink"
        assert torch.equal(Wh[2], W0h[2]) and not Mh[2].any(), "a row with G = M = 0 changed"


# ---- the fused tails ----------------------------------------------------------------------------------------------------------------
def _state(dev, N, d, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    W = torch.randn(N, d, generator=g, device=dev) / d ** 0.5
    G = torch.randn(N, d, generator=g, device=dev) * 1e-3
    G[::7] = 0.0                                           # rows without a gradient (features that did not fire)
    M = torch.randn(N, d, generator=g, device=dev) * 1e-4
    ss = (G.double() ** 2).sum().float().reshape(1)
    return W, G, M, ss


@pytest.mark.parametrize("project", [True, False], ids=["project", "no_project"])
@pytest.mark.parametrize("d", [1024, 4096, 8192, 1000, 12288])
def test_lion_pass_with_the_next_steps_renorm_equals_the_two_passes(dev, d, project):
    """lion_rows_(renorm_eps=eps) == lion_rows_ then unit_norm_rows_, bit for bit (W, M) -- including the shapes that run
    the plain kernel and the separate passes (d % 4 != 0, d > 8192)."""
    from msae import ops

    N = 2048
    W, G, M, ss = _state(dev, N, d, 3)
    W0, W2, M2 = W.clone(), W.clone(), M.clone()
    with _NoSync():
        ops.lion_rows_(W, G, M, 1e-3, total_sumsq=ss, project=project)
    assert not torch.equal(W, W0)
    with _NoSync():
        ops.unit_norm_rows_(W, EPS32)
        ops.lion_rows_(W2, G, M2, 1e-3, total_sumsq=ss, project=project, renorm_eps=EPS32)
    assert torch.equal(W, W2) and torch.equal(M, M2)
    assert torch.allclose(W2.norm(dim=1), torch.ones(N, device=dev), atol=1e-5)


@pytest.mark.parametrize("mode,tokens", [("int8", 8192), ("int8", 64), ("bf16", 8192)])
def test_lion_pass_with_the_encoder_operand_refresh_equals_the_two_passes(dev, mode, tokens):
    """lion_rows_(refresh=buf, tokens_next=T) == lion_rows_ then prepare_encoder(active_mode_only=True, tokens_next=T): the
    updated weight, the momentum and the WHOLE prepared buffer bit for bit; an encode against the fused buffer is verified
    and equals the exact path."""
    from msae import ops

    N, d, k = 16384, 1024, 32
    ops.set_coarse_mode(mode)
    ops.set_dither("on", seed=0x5EED)
    try:
        W, G, M, ss = _state(dev, N, d, 5)
        W2, M2 = W.clone(), M.clone()
        nbytes = ops.prepare_encoder(W).numel()
        buf_a = ops.prepare_encoder(W, out=torch.zeros(nbytes, dtype=torch.uint8, device=dev))
        buf_b = ops.prepare_encoder(W, out=torch.zeros(nbytes, dtype=torch.uint8, device=dev))
        assert torch.equal(buf_a, buf_b)
        with _NoSync():
            ops.lion_rows_(W, G, M, 1e-3, total_sumsq=ss)
        ops.prepare_encoder(W, out=buf_a, active_mode_only=True, tokens_next=tokens)
        with _NoSync():
            ops.lion_rows_(W2, G, M2, 1e-3, total_sumsq=ss, refresh=buf_b, tokens_next=tokens)
        assert torch.equal(W, W2) and torch.equal(M, M2)
        diff = (buf_a != buf_b).nonzero()
        assert diff.numel() == 0, f"prepared buffers differ at {diff.numel()} bytes, first at {int(diff[0])}"
        b = torch.zeros(N, device=dev)
        x = torch.randn(tokens, d, generator=torch.Generator(device=dev).manual_seed(9), device=dev).to(torch.bfloat16)
        v, i, st = ops.encode_topk(x, W2, b, None, buf_b, k)
        ev, ei = ops.topk(ops.pre_acts(x[:512], W2, b, None), k)
        assert float((st == 0).float().mean()) > 0.95
        assert torch.equal(i[:512], ei) and torch.equal(v[:512], ev)
    finally:
        ops.set_coarse_mode("int8")
        ops.set_dither("default")


# ---- the training step --------------------------------------------------------------------------------------------------------------
_D, _N, _K, _T = 512, 8192, 16, 1024


def _trainer(dev, optimizer, **kw):
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    torch.manual_seed(7)
    sae = Sae(_D, SaeConfig(num_latents=_N, k=_K), device=dev)
    return sae, SaeTrainStep(sae, lr=1e-3, optimizer=optimizer, **kw)


def _batch(dev, seed):
    return torch.randn(_T, _D, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)


@pytest.mark.parametrize("optimizer", ["lion", "signum"])
def test_train_step_state_and_no_host_sync(dev, optimizer, monkeypatch):
    """One moment: 4 bytes per element, no second moment, no 8-bit state; a whole step (after the first, which allocates and
    plans) runs without a host synchronisation, through ops.lion_rows_ alone."""
    from msae import ops

    sae, ts = _trainer(dev, optimizer)
    numel = sum(p.numel() for p in ts.params)
    assert ts.optimizer_state_bytes == 4 * numel
    assert all(v is None for v in ts.exp_avg_sq) and all(s is None for s in ts.state8)
    assert ts.betas == ((0.9, 0.99) if optimizer == "lion" else (0.9, 0.9))
    calls = []
    real = ops.lion_rows_

    def lion_rows_(p, g, m, lr, **kw):
        calls.append(kw["betas"])
        return real(p, g, m, lr, **kw)

    def adam_rows_(*a, **kw):
        raise AssertionError("ops.adam_rows_ was called by a sign optimiser")

    monkeypatch.setattr(ops, "lion_rows_", lion_rows_)
    monkeypatch.setattr(ops, "adam_rows_", adam_rows_)
    before = [p.detach().clone() for p in ts.params]
    ts.step(_batch(dev, 1))
    x = _batch(dev, 2)
    with _NoSync():
        out = ts.step(x)
    assert len(calls) == 2 * len(ts.params) and all(b == ts.betas for b in calls)
    assert bool(torch.isfinite(out["fvu"])) and ts.t == 2
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, ts.params))
    assert all(bool(m.any()) for m in ts.exp_avg)


def test_train_step_checkpoint_round_trip(dev):
    """state_dict -> a fresh step object -> load_state_dict -> the next step's parameters are bit-identical to the uninterrupted
    run.  (fuse_next_step off and max_grad_norm = 1e9 for the reasons test_train_step_8bit_checkpoint_round_trip gives: a
    fresh object renormalises W_dec once more, and the bias gradients' norm is summed with float atomics.)"""
    sae, ts = _trainer(dev, "lion", fuse_next_step=False)
    ts.max_grad_norm = 1e9
    for s in range(3):
        ts.step(_batch(dev, 100 + s))
    sd = copy.deepcopy(ts.state_dict())
    params = {n: p.detach().clone() for n, p in sae.named_parameters()}
    assert sd["optimizer"] == "lion" and tuple(sd["betas"]) == (0.9, 0.99) and sd["step"] == 3
    assert all(v is None for v in sd["exp_avg_sq"]) and "optim_bits" not in sd
    ts.step(_batch(dev, 103))
    sae2, ts2 = _trainer(dev, "lion", fuse_next_step=False)
    ts2.max_grad_norm = 1e9
    with torch.no_grad():
        for n, p in sae2.named_parameters():
            p.copy_(params[n])
    ts2.load_state_dict(sd)
    ts2.step(_batch(dev, 103))
    for (n, a), (_, b) in zip(sae.named_parameters(), sae2.named_parameters()):
        assert torch.equal(a, b), f"{n} differs after the checkpoint round trip"
    for a, b in zip(ts.exp_avg, ts2.exp_avg):
        assert torch.equal(a, b)
    _, adam = _trainer(dev, "adam")
    with pytest.raises(ValueError, match="lion"):
        adam.load_state_dict(sd)


# ---- it learns ----------------------------------------------------------------------------------------------------------------------
_STEPS, _LAST = 60, 10


def _structured(dev, dictionary, seed):
    """T tokens: 8 of the 2048 hidden unit directions each, |N(0, 1)| coefficients, plus 0.05 N(0, 1) noise
    (test_gpu_adam8.py's data)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = torch.randint(0, dictionary.shape[0], (_T, 8), generator=g, device=dev)
    coef = torch.randn(_T, 8, generator=g, device=dev).abs()
    return (dictionary[idx] * coef[:, :, None]).sum(1) + 0.05 * torch.randn(_T, _D, generator=g, device=dev)


def _trajectory(dev, dictionary, optimizer):
    _, ts = _trainer(dev, optimizer)
    fvu = [ts.step(_structured(dev, dictionary, 10_000 + s))["fvu"] for s in range(_STEPS)]
    return torch.stack(fvu).double().cpu()


def test_lion_learns_at_least_half_of_what_adam_learns(dev):
    """The trainer, data and 60 steps of test_8bit_trajectory_stays_within_the_float32_optimisers_own_spread (d = 512,
    N = 8192, k = 16, T = 1024, lr 1e-3 for both, batch seed 0).  Lion (0.9, 0.99) is finite throughout, and its mean FVU
    over the last 10 steps has dropped from its first-step FVU by at least half of what the Adam run of the same test
    dropped.  (A dense float32 restatement on the CPU gave first-step 0.777, Adam 0.691, Lion 0.649: 1.5 times Adam's drop;
    half leaves room for the GPU's different sign decisions.)"""
    g = torch.Generator(device=dev).manual_seed(4242)
    dictionary = torch.nn.functional.normalize(torch.randn(2048, _D, generator=g, device=dev), dim=1)
    adam = _trajectory(dev, dictionary, "adam")
    lion = _trajectory(dev, dictionary, "lion")
    end_a, end_l = float(adam[-_LAST:].mean()), float(lion[-_LAST:].mean())
    drop_a, drop_l = float(adam[0]) - end_a, float(lion[0]) - end_l
    print(f"\nit learns: first-step FVU adam {float(adam[0]):.5f} lion {float(lion[0]):.5f}; mean of the last {_LAST} steps "
          f"adam {end_a:.5f} lion {end_l:.5f}; drop adam {drop_a:.5f} lion {drop_l:.5f}")
    assert bool(torch.isfinite(lion).all())
    assert drop_a > 0 and drop_l >= 0.5 * drop_a
