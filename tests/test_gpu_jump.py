"""The JumpReLU selection on the HIP path (csrc/jump_select.hip; include/msae.h, "JumpReLU selection")
against the sorting restatement tests/jump_ref.py.

  * msae_jump_filter_f32 / _i64_f32 on BITS: widths that fill no wave, one wave, one wave and a bit, four registers a lane;
    one token, a few workgroups, a last workgroup that is not full; a strided view; hostile values; rows that are all kept,
    all near, all rest; accumulating counters; C = 257 refused.
  * msae_jump_bwd_f32: the routing copy on bits; g_theta inside the DERIVED bound gamma_{n_f + 3} sum |c| of the float64
    restatement (n_f - 1 additions in any order and up to three roundings of c, each relative to |c|; gamma_m = m 2^-24 / (1 - m 2^-24)) for features
    with 0, 1, 64, 65, 300 and 1100 band entries -- every path of the reduction: empty, registers of one wave's LDS slice, the
    lane-strided sum, the in-place sort beyond 1024 --, N = 96 and 8192; two runs bit-identical; the workspace contract.
  * a "jump" Sae under torch.cuda.set_sync_debug_mode("error"): forward against the restatement on the project's own
    pre_acts, the reach decode against the len decode, the inference encode against a TopK twin's encode(threshold=table),
    gradients against the same graph with the restatement in place of ops.jump_select.
  * forty training steps: an L0 penalty lowers L0 and moves the thresholds; without it and with a vanishing bandwidth
    log_threshold keeps its bits.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import batch_select_ref as bref
import guarded_ws
import jump_ref as ref
import synth

pytestmark = pytest.mark.gpu

MSAE_EINVAL, MSAE_EWS = -1, -3
EPS = 0.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), what


def _theta(rng, N):
    theta = (0.9 + 0.6 * rng.random(N)).astype(np.float32)
    theta[7 % N] = np.inf
    return theta


def _check_filter(dev, vals, idx, theta, eps, what):
    from msae import ops

    sel = ref.select(vals, idx, theta, eps)
    n_sat = int(sel["saturated"].sum())
    for dt in (torch.int32, torch.int64):
        v, i = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, dt)
        c_l0 = torch.full((), 11, dtype=torch.int64, device=dev)
        c_sat = torch.full((), 5, dtype=torch.int32, device=dev)
        th = torch.from_numpy(theta).to(dev)
        vo, io, ln, reach, src, l0, ns = ops.jump_filter(v, i, th, eps, l0=c_l0, n_saturated=c_sat)
        ops.jump_filter(v, i, th, eps, l0=c_l0, n_saturated=c_sat)                    # the counters accumulate over calls
        w = f"{what}, {dt}"
        _same_bits(vo, sel["vals"], w)
        assert io.dtype == dt and np.array_equal(io.cpu().numpy(), sel["idx"]), w
        assert np.array_equal(ln.cpu().numpy(), sel["len"]) and np.array_equal(reach.cpu().numpy(), sel["reach"]), w
        assert src.dtype == torch.uint8 and np.array_equal(src.cpu().numpy(), sel["src"]), w
        assert l0 is c_l0 and int(c_l0) == 11 + 2 * sel["l0"] and ns is c_sat and int(c_sat) == 5 + 2 * n_sat, w
    return sel


# ---- msae_jump_filter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 32, 64, 65, 256])
def test_jump_filter(dev, C):
    from msae import ops

    N = 512
    seen = set()
    for T in (1, 37, 300):
        rng = np.random.default_rng(1000 * C + T)
        theta = _theta(rng, N)
        vals, idx = ref.lists_around(rng, T, C, N, theta, EPS)
        if T > 1:
            vals[T // 2] += np.float32(0.5)                                         # a row that keeps everything: saturated
        planted = ref.plant_hostile(vals, idx, theta, EPS)
        assert planted or T * C < 11
        sel = _check_filter(dev, vals, idx, theta, EPS, f"T = {T}, C = {C}")
        seen |= set(sel["saturated"].tolist())
        if T * C >= 64:
            assert sel["kept"].any() and sel["near"].any() and (~sel["kept"] & ~sel["near"]).any()
        # the [:, :C] view of a wider list is read in place
        wide_v = torch.from_numpy(np.concatenate([vals, np.full((T, 5), 9.0, np.float32)], 1)).to(dev)
        wide_i = torch.from_numpy(np.concatenate([idx, np.zeros((T, 5), np.int64)], 1)).to(dev)
        out = ops.jump_filter(wide_v[:, :C], wide_i[:, :C], torch.from_numpy(theta).to(dev), EPS)
        _same_bits(out[0], sel["vals"], f"T = {T}, C = {C}: view")
        assert np.array_equal(out[1].cpu().numpy(), sel["idx"]) and np.array_equal(out[3].cpu().numpy(), sel["reach"])
    assert seen == {True, False}, "the case needs saturated and unsaturated rows"


def test_jump_filter_rows_of_one_class(dev):
    rng = np.random.default_rng(5)
    T, C, N = 9, 70, 512
    theta = (0.9 + 0.6 * rng.random(N)).astype(np.float32)
    idx = np.stack([rng.permutation(N)[:C] for _ in range(T)]).astype(np.int64)
    h = ref.half_band(EPS)
    vals = np.empty((T, C), np.float32)
    for t in range(T):
        off = (np.float32(2) * h, np.float32(-0.5) * h, np.float32(-3) * h)[t % 3]  # all kept / all near / all rest
        vals[t] = theta[idx[t]] + off
    sel = _check_filter(dev, vals, idx, theta, EPS, "one class per row")
    assert sel["len"].tolist() == [C, 0, 0] * 3 and sel["reach"].tolist() == [C, C, 0] * 3
    assert np.array_equal(sel["src"], np.tile(np.arange(C), (T, 1)))                # nothing moves


def test_jump_filter_refusals(dev):
    from msae import _hip, ops

    lib = _hip.load()
    P_ = _hip.ptr
    C = 257
    v = torch.rand(4, C, device=dev)
    i = torch.zeros(4, C, dtype=torch.int32, device=dev)
    th = torch.ones(8, device=dev)
    fl = torch.zeros((), device=dev)
    vo, io = torch.full_like(v, -7.0), torch.full_like(i, -7)
    ln, rc = (torch.full((4,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    src = torch.full((4, C), 9, dtype=torch.uint8, device=dev)
    st = _hip.stream_of(v)
    call = lambda T=4, C_=8, ld=C, N=8, h=0.125, theta=th, floor=fl: lib.msae_jump_filter_f32(
        P_(v), P_(i), T, C_, ld, P_(theta), N, h, P_(floor), P_(vo), P_(io), P_(ln), P_(rc), P_(src), None, None, st)
    for kw in (dict(C_=257), dict(C_=0), dict(T=-1), dict(ld=7), dict(N=0), dict(h=0.0), dict(h=-1.0), dict(theta=None),
               dict(floor=None)):
        assert call(**kw) == MSAE_EINVAL, kw
    assert call(T=0) == 0
    torch.cuda.synchronize()
    assert bool((ln == -7).all()) and bool((vo == -7).all()) and bool((io == -7).all()) and bool((src == 9).all())
    with pytest.raises(ValueError):
        ops.jump_select(v, i, th, EPS)                                              # C = 257


# ---- msae_jump_bwd --------------------------------------------------------------------------------------------------------------
_BWD = {}


def _bwd_case(T, C, N):
    """Lists with features whose band counts are known: F[0] on every token (T entries), F[1] 64, F[2] 65, F[3] one, F[4]
    on every token but outside the band; the other columns random around their thresholds, hostile values planted."""
    key = (T, C, N)
    if key not in _BWD:
        rng = np.random.default_rng(T + C + N)
        theta = (0.9 + 0.6 * rng.random(N)).astype(np.float32)
        F = np.array([3, 11, 20, 41, 57])
        pool = np.setdiff1d(np.arange(N), F)
        idx = np.stack([rng.permutation(pool)[:C] for _ in range(T)]).astype(np.int64)
        th = theta[idx]
        h = ref.half_band(EPS)
        vals = (th + (rng.random((T, C)).astype(np.float32) - np.float32(0.5)) * np.float32(6) * h).astype(np.float32)
        if C > 12:
            ref.plant_hostile(vals[:, 5:], idx[:, 5:], theta, EPS)
        rows = (np.arange(T), np.arange(min(64, T)), np.arange(min(65, T)), np.array([5 % T]), np.arange(T))
        offs = (np.float32(0.5) * h, np.float32(-0.5) * h, np.float32(0.25) * h, np.float32(-0.25) * h, np.float32(2) * h)
        for c, (f, r, o) in enumerate(zip(F, rows, offs)):
            idx[r, c] = f
            vals[r, c] = theta[f] + o
        sel = ref.select(vals, idx, theta, EPS)
        g = rng.standard_normal((T, C)).astype(np.float32)
        s = np.float32(0.375)
        _BWD[key] = (vals, idx, theta, sel, g, s, F, ref.backward(vals, idx, theta, EPS, sel, g, s))
    return _BWD[key]


def _run_bwd(dev, vals, idx, theta, g, s, dt=torch.int32):
    from msae import ops

    v, i, th = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, dt), torch.from_numpy(theta).to(dev)
    _, _, ln, reach, src, _, _ = ops.jump_filter(v, i, th, EPS)
    return ops.jump_bwd(v, i, th, EPS, src, ln, reach, torch.from_numpy(g).to(dev), torch.tensor(float(s), device=dev))


@pytest.mark.parametrize("T,C,N", [(300, 32, 96), (300, 32, 8192), (1100, 8, 96)])
def test_jump_bwd(dev, T, C, N):
    vals, idx, theta, sel, g, s, F, (r_in, r_theta, abs_sum, n_f) = _bwd_case(T, C, N)
    assert [int(n_f[f]) for f in F] == [T, min(64, T), min(65, T), 1, 0], "the case plants these band counts"
    assert N == 96 or int((n_f == 0).sum()) > N // 2
    runs = []
    for dt in (torch.int32, torch.int64, torch.int32):
        g_in, g_theta = _run_bwd(dev, vals, idx, theta, g, s, dt)
        _same_bits(g_in, r_in, f"routing, {dt}")
        got = g_theta.cpu().numpy()
        err, bound = np.abs(got.astype(np.float64) - r_theta), ref.g_theta_bound(n_f, abs_sum)
        worst = float((err[n_f > 0] / bound[n_f > 0]).max())
        print(f"T = {T}, C = {C}, N = {N}, {dt}: largest error / bound {worst:.3f}; band share {n_f.sum() / (T * C):.3f}")
        assert (err <= bound).all(), f"g_theta outside its bound: {worst:.3f} of it"
        assert (_bits(got)[n_f == 0] == 0).all(), "a feature without band entries gets +0.0"
        runs.append(_bits(got))
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), "two runs must be bit-identical"
    # g = 0, s > 0: g_theta[f] = -s n_f / eps -- the sign and the count
    zero = np.zeros_like(g)
    _, g_theta = _run_bwd(dev, vals, idx, theta, zero, s)
    want = -float(s) * n_f / float(np.float32(EPS))
    _, _, abs0, _ = ref.backward(vals, idx, theta, EPS, sel, zero, s)
    assert (np.abs(g_theta.cpu().numpy().astype(np.float64) - want) <= ref.g_theta_bound(n_f, abs0)).all()
    assert float(g_theta[int(F[0])]) < 0


_BWD_FILLS = {}


@pytest.mark.parametrize("fill", guarded_ws.FILLS)
def test_jump_bwd_under_guarded_workspaces(dev, monkeypatch, fill):
    from msae import _hip, ops

    T, C, N = 300, 32, 96
    vals, idx, theta, sel, g, s, F, (r_in, r_theta, abs_sum, n_f) = _bwd_case(T, C, N)
    gws = guarded_ws.GuardedWorkspace(fill, dev)
    gws.what = f"msae_jump_bwd_f32 T={T} C={C} N={N}"
    monkeypatch.setattr(ops, "_workspace", gws)
    if fill == "recycled":
        _run_bwd(dev, vals[::-1].copy(), idx[::-1].copy(), theta, g, s)
        gws.check()
    g_in, g_theta = _run_bwd(dev, vals, idx, theta, g, s)
    gws.check()
    _same_bits(g_in, r_in, fill)
    assert (np.abs(g_theta.cpu().numpy().astype(np.float64) - r_theta) <= ref.g_theta_bound(n_f, abs_sum)).all()
    assert {n for _, n in gws.requests} == {_hip.load().msae_jump_bwd_ws_bytes(T, C, N)}
    bits = _bits(g_theta).tolist()
    assert _BWD_FILLS.setdefault("g_theta", bits) == bits                           # nothing is read before it is written


def test_jump_bwd_refuses_a_short_workspace_and_bad_shapes(dev):
    from msae import _hip, ops

    lib = _hip.load()
    P_ = _hip.ptr
    T, C, N = 37, 13, 96
    rng = np.random.default_rng(2)
    theta = (0.9 + 0.6 * rng.random(N)).astype(np.float32)
    vals, idx = ref.lists_around(rng, T, C, N, theta, EPS)
    v, i, th = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, torch.int32), torch.from_numpy(theta).to(dev)
    _, _, ln, reach, src, _, _ = ops.jump_filter(v, i, th, EPS)
    g = torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32)).to(dev)
    s = torch.full((), 0.375, device=dev)
    g_in, g_theta = torch.full((T, C), -7.0, device=dev), torch.full((N,), -7.0, device=dev)
    st = _hip.stream_of(v)
    need = lib.msae_jump_bwd_ws_bytes(T, C, N)
    assert need == ((3 * (N + 1) + 1) // 2 * 2) * 4 + T * C * 8
    assert lib.msae_jump_bwd_ws_bytes(0, C, N) == lib.msae_jump_bwd_ws_bytes(T, 257, N) == lib.msae_jump_bwd_ws_bytes(T, C, 0) == 0
    gws = guarded_ws.GuardedWorkspace("word3", dev)
    call = lambda ws, n, T_=T, C_=C, ld=C, N_=N, h=0.125, eps=0.25: lib.msae_jump_bwd_f32(
        P_(v), P_(i), T_, C_, ld, P_(th), N_, h, eps, P_(src), P_(ln), P_(reach), P_(g), P_(s), P_(g_in), P_(g_theta), ws, n, st)
    big = ctypes.c_void_p(v.data_ptr())                                             # (never touched: refused before any launch)
    for kw in (dict(C_=257, ld=257), dict(C_=0), dict(T_=-1), dict(ld=C - 1), dict(N_=0), dict(h=0.0), dict(eps=0.0)):
        assert call(big, 1 << 40, **kw) == MSAE_EINVAL, kw
    ptr, n, blk = gws.block(need - 1)
    before = blk.view.clone()
    assert call(ctypes.c_void_p(ptr), n) == MSAE_EWS and call(None, need) == MSAE_EWS
    gws.check()
    assert bool((g_in == -7).all()) and bool((g_theta == -7).all()) and torch.equal(blk.view, before)
    ptr, n, _ = gws.block(need)
    assert call(ctypes.c_void_p(ptr), n) == 0
    gws.check()
    sel = ref.select(vals, idx, theta, EPS)
    r_in, r_theta, abs_sum, n_f = ref.backward(vals, idx, theta, EPS, sel, g.cpu().numpy(), np.float32(0.375))
    _same_bits(g_in, r_in, "exact-size workspace")
    assert (np.abs(g_theta.cpu().numpy().astype(np.float64) - r_theta) <= ref.g_theta_bound(n_f, abs_sum)).all()


# ---- Sae level --------------------------------------------------------------------------------------------------------------
D_, N_, K_, C_ = 128, 8192, 8, 32


def _sae(dev, activation="jump", bandwidth=1e-3):
    from msae import Sae, SaeConfig

    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(D_, N_, seed=21)
    kw = dict(jump_bandwidth=bandwidth) if activation == "jump" else {}
    sae = Sae(D_, SaeConfig(num_latents=N_, k=K_, activation=activation, **kw), device=dev)
    with torch.no_grad():
        for p, a in ((sae.encoder.weight, W_enc), (sae.encoder.bias, b_enc), (sae.W_dec, W_dec), (sae.b_dec, b_dec)):
            p.copy_(torch.from_numpy(a))
    sae.invalidate_prepared()
    return sae


_PRE = {}


def _restated(dev, T):
    """x, a "jump" Sae whose thresholds straddle the lists' values, and the restatement applied to the project's own exact
    pre_acts with the Sae's own table exp(log_threshold) (computed once per shape, never modified)"""
    if T not in _PRE:
        x = torch.from_numpy(synth.activations(T, D_, seed=22, n_outlier=0)).to(dev)
        with torch.no_grad():
            pre = _sae(dev, "topk").pre_acts(x).cpu().numpy()
        vals, idx = bref.canonical_lists(pre, C_)
        rng = np.random.default_rng(T)
        mid = float(np.median(vals[:, K_]))                                         # about K_ entries a row lie above it
        sae = _sae(dev, bandwidth=float(np.float32(0.2 * mid)))                     # a band of +-10 % around a threshold
        assert sae.cfg.cap == C_
        sae.set_threshold(torch.from_numpy((mid * (0.8 + 0.4 * rng.random(N_))).astype(np.float32)))
        with torch.no_grad():
            theta = sae.log_threshold.exp().cpu().numpy()
        _PRE[T] = (x, sae, pre, vals, idx, theta, ref.select(vals, idx, theta, sae.cfg.jump_bandwidth))
    return _PRE[T]


class _RestatedSelect(torch.autograd.Function):
    """ops.jump_select through tests/jump_ref.py on the host: the same outputs, the routing copy as the backward"""

    @staticmethod
    def forward(ctx, acts, idx, theta, eps):
        dev = acts.device
        v, i, th = acts.detach().cpu().numpy(), idx.cpu().numpy(), theta.detach().cpu().numpy()
        sel = ref.select(v, i, th, eps)
        ctx.args = (v, i, th, eps, sel)
        return (torch.from_numpy(sel["vals"]).to(dev), torch.from_numpy(sel["idx"]).to(dev, idx.dtype),
                torch.from_numpy(sel["len"]).to(dev), torch.from_numpy(sel["reach"]).to(dev),
                torch.tensor(float(sel["l0"]), device=dev), torch.tensor(int(sel["saturated"].sum()), dtype=torch.int32, device=dev))

    @staticmethod
    def backward(ctx, g, _gi, _gl, _gr, g_l0, _gn):
        v, i, th, eps, sel = ctx.args
        s = np.float32(0.0) if g_l0 is None else np.float32(g_l0.item())
        g_in, g_theta, _, _ = ref.backward(v, i, th, eps, sel, g.cpu().numpy(), s)
        return torch.from_numpy(g_in).to(g.device), None, torch.from_numpy(g_theta.astype(np.float32)).to(g.device), None


@pytest.mark.parametrize("T", [300, 40])
def test_sae_forward_encode_and_gradients_against_the_restatement(dev, monkeypatch, T):
    from msae import ops

    x, sae, pre, vals, idx, theta, sel = _restated(dev, T)
    n_band = int(sel["band"].sum())
    print(f"T = {T}: kept {sel['l0']}, near {int(sel['near'].sum())}, band {n_band}, saturated {int(sel['saturated'].sum())}")
    assert sel["near"].any() and n_band > 0 and 0 < sel["l0"] < T * C_
    sae.train()
    alpha = 0.5
    calls = []
    real_bwd = ops.jump_bwd

    def spy(*a):
        out = real_bwd(*a)
        calls.append((a, out))
        return out

    def run():
        for p in sae.parameters():
            p.grad = None
        out = sae(x)
        (out.fvu + alpha * out.l0).backward()
        return out

    run()                                                           # warm: library load, operand preparation, workspaces
    with torch.no_grad():
        sae.encode(x)
    monkeypatch.setattr(ops, "jump_bwd", spy)
    with no_sync():
        out = run()
        with torch.no_grad():
            enc, lengths = sae.encode(x, return_lengths=True)
            by_len = sae.decode(out.latent_acts, out.latent_indices, out.lengths)
    what = f"T = {T}"
    _same_bits(out.latent_acts, sel["vals"], what)
    assert np.array_equal(out.latent_indices.cpu().numpy(), sel["idx"]), what
    assert np.array_equal(out.lengths.cpu().numpy(), sel["len"]) and np.array_equal(out.reach.cpu().numpy(), sel["reach"]), what
    assert int(out.n_saturated) == int(sel["saturated"].sum()) and out.latent_acts.shape == (T, C_)
    # the mean: the exact integer count as a float32 (exact below 2^24) over T, a division or a product with 1 / T
    assert sel["l0"] < 2 ** 24 and abs(float(out.l0) - sel["l0"] / T) <= 2.0 ** -22 * sel["l0"] / T, what
    _same_bits(out.sae_out, by_len, f"{what}: the reach decode has the bits of the len decode")
    # inference: the table filter, bit-identical to a TopK twin's encode(threshold=table, cap=C)
    twin = _sae(dev, activation="topk")
    twin.eval()
    with torch.no_grad():
        t_enc, t_len = twin.encode(x, threshold=torch.from_numpy(theta).to(dev), cap=C_, return_lengths=True)
    _same_bits(enc.top_acts, t_enc.top_acts, f"{what}: inference encode")
    assert torch.equal(enc.top_indices, t_enc.top_indices) and torch.equal(lengths, t_len)
    assert np.array_equal(lengths.cpu().numpy(), sel["len"])
    # the threshold gradient: g_theta inside its bound given the upstream g and s the node received, log_threshold.grad its
    # product with theta (exp's backward: one more float32 multiplication, checked on bits)
    (a, (g_in, g_theta)), = calls
    g_up, s_up = a[7].cpu().numpy().reshape(T, C_), np.float32(a[8].cpu().item())
    assert s_up > 0
    r_in, r_theta, abs_sum, n_f = ref.backward(vals, idx, theta, sae.cfg.jump_bandwidth, sel, g_up, s_up)
    _same_bits(g_in, r_in, f"{what}: routing")
    err, bound = np.abs(g_theta.cpu().numpy().astype(np.float64) - r_theta), ref.g_theta_bound(n_f, abs_sum)
    print(f"  g_theta: largest error / bound {float((err[n_f > 0] / bound[n_f > 0]).max()):.3f}, features in the band {int((n_f > 0).sum())}")
    assert (err <= bound).all()
    _same_bits(sae.log_threshold.grad, g_theta * torch.from_numpy(theta).to(dev), f"{what}: log_threshold.grad")
    grads = {n: p.grad.clone() for n, p in sae.named_parameters()}
    # the same graph with the host restatement in place of ops.jump_select: encoder and decoder gradients keep their bits
    monkeypatch.setattr(ops, "jump_select", lambda acts, idx_, th, eps: _RestatedSelect.apply(acts, idx_, th, eps))
    out2 = run()
    _same_bits(out2.sae_out, out.sae_out, what)
    for n, p in sae.named_parameters():
        if n != "log_threshold":
            _same_bits(p.grad, grads[n], f"{what}: {n}.grad")
    assert float(grads["encoder.weight"].abs().max()) > 0 and float(grads["W_dec"].abs().max()) > 0


# ---- training ---------------------------------------------------------------------------------------------------------------
_D, _N, _K, _T, _STEPS = 512, 8192, 16, 1024, 40


def _structured(dev, dictionary, seed):
    """tests/test_gpu_lion.py's data: 8 of 2048 hidden unit directions per token, |N(0, 1)| coefficients, 0.05 N(0, 1) noise"""
    g = torch.Generator(device=dev).manual_seed(seed)
    idx = torch.randint(0, dictionary.shape[0], (_T, 8), generator=g, device=dev)
    coef = torch.randn(_T, 8, generator=g, device=dev).abs()
    return (dictionary[idx] * coef[:, :, None]).sum(1) + 0.05 * torch.randn(_T, _D, generator=g, device=dev)


def _train(dev, l0_alpha, bandwidth, init):
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    torch.manual_seed(7)
    sae = Sae(_D, SaeConfig(num_latents=_N, k=_K, activation="jump", jump_init=init, jump_bandwidth=bandwidth), device=dev)
    ts = SaeTrainStep(sae, lr=TRAIN_LR, l0_alpha=l0_alpha)
    g = torch.Generator(device=dev).manual_seed(4242)
    dictionary = torch.nn.functional.normalize(torch.randn(2048, _D, generator=g, device=dev), dim=1)
    before = sae.log_threshold.detach().clone()
    l0 = [ts.step(_structured(dev, dictionary, 10_000 + s))["l0"] for s in range(_STEPS)]
    return sae, before, torch.stack(l0).double().cpu()


JUMP_INIT, TRAIN_LR, TRAIN_EPS, TRAIN_ALPHA = 0.1, 1e-2, 0.1, 0.05


def test_an_l0_penalty_lowers_l0_and_moves_the_thresholds(dev):
    sae, before, l0 = _train(dev, TRAIN_ALPHA, TRAIN_EPS, JUMP_INIT)
    first, last = float(l0[:5].mean()), float(l0[-5:].mean())
    moved = float((sae.log_threshold.detach() - before).abs().max())
    print(f"\nmean L0 of the first five steps {first:.3f}, of the last five {last:.3f}; largest move of log_threshold {moved:.4f}")
    assert bool(torch.isfinite(l0).all()) and last < first and moved > 0


def test_without_penalty_and_band_the_thresholds_keep_their_bits(dev):
    # (a threshold of 1e-3: an activation that equals it bit for bit -- the one way into a band of 5e-31 -- is ~300 times
    # rarer than at 0.1, where the floats lie 2^6 times farther apart and the activations are denser)
    sae, before, l0 = _train(dev, 0.0, 1e-30, 1e-3)
    assert bool(torch.isfinite(l0).all()) and float(l0[0]) > 0
    _same_bits(sae.log_threshold, before, "log_threshold after forty steps with nothing in the band")
