"""Support refit on the HIP path (ops.support_refit, Sae.refit, ReconStats(refit=True)) against the float64 restatement
tests/refit_ref.py within the bounds derived there, and BIT FOR BIT where the contract (include/msae.h, "support refit")
defines bits: orthonormal supports, and a token alone, in a batch, through chunk= and from two runs.  Fixtures and the power
of the bounds: tests/refit_ref.py, tests/test_refit_host.py.  Shapes are the smallest that reach each structural edge: d = 64
(one partial 128-column slab), 200 (d % 4 == 0 off the slab), 203 (the element-load path), 1152 (nine slabs, two slabs of the
second walk); s = 1, 2, 31, 32 (one 32 x 32 tile), 33, 64 (three tiles); T = 1, 3, 257."""
import contextlib

import numpy as np
import pytest
import torch

import fakes
import refit_ref as ref

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPES = ("f32", "bf16", "f16")
SHAPES = [(d, s) for d in (64, 200, 203, 1152) for s in (1, 2, 31, 32, 33, 64) if s <= d // 2]


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


def _case(n: int) -> ref.Case:
    """Case n of SHAPES: the x types, the index types, ld > s and zero-valued slots (first, middle, last) rotate over the list."""
    d, s = SHAPES[n]
    zeros = (0, s // 2, s - 1) if n % 3 == 2 and s >= 4 else ()
    return ref.Case(d, s, 3, dtype=DTYPES[n % 3], wide=bool(n % 2), ld=s + 5 if n % 4 == 1 else None, seed=40 + n, zeros=zeros)


_CASES = {}


def case(n: int) -> ref.Case:
    if n not in _CASES:
        _CASES[n] = _case(n)
    return _CASES[n]


def _inputs(c: ref.Case, dev):
    v, i = torch.from_numpy(c.vals).to(dev), torch.from_numpy(c.idx).to(dev)
    return (torch.from_numpy(c.x).to(dev, TDT[c.dtype]), v, i, torch.from_numpy(c.W_dec).to(dev), torch.from_numpy(c.b_dec).to(dev))


def _np(out) -> dict:
    return {k: v.cpu().numpy() for k, v in out._asdict().items()}


def _assert_inside(c, out, tokens, what):
    log = []
    bad = ref.violations(c, out, tokens, log)
    worst = {}
    for name, _, err, lim in log:
        key = name.split("[")[0]
        worst[key] = max(worst.get(key, 0.0), err / lim if lim > 0 else (0.0 if err == 0 else float("inf")))
    print(f"{what}: worst figure / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert bad == [], (what, bad[:5])


def test_the_case_list_covers_what_it_must():
    cs = [case(n) for n in range(len(SHAPES))]
    assert {c.d for c in cs} == {64, 200, 203, 1152} and {c.s for c in cs} == {1, 2, 31, 32, 33, 64}
    assert all(c.s <= c.d // 2 for c in cs) and {c.dtype for c in cs} == set(DTYPES) and {c.wide for c in cs} == {True, False}
    assert any(c.ld > c.s for c in cs) and any((c.vals[:, 0] == 0).all() and (c.vals[:, c.s - 1] == 0).all() for c in cs)
    for s in (31, 32, 33, 64):
        assert {c.d % 4 == 0 for c in cs if c.s == s} == {True, False}, s


# ---- 1, 2: the bounds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(SHAPES)), ids=lambda n: "d%d-s%d" % SHAPES[n])
def test_outputs_lie_inside_the_derived_bounds(dev, n):
    """Residual of the normal equations, excess objective, gain prefix sums against the per-prefix lstsq, err_fit, err_enc, yy,
    and err_fit <= err_enc -- on supports asserted well-conditioned in float64."""
    from msae import ops

    c = case(n)
    assert ref.premises(c, range(c.T)) == []                               # cond(G) <= 1e3, rho <= 16
    x, v, i, W, b = _inputs(c, dev)
    out = ops.support_refit(x, v[:, :c.s] if c.ld > c.s else v, i[:, :c.s] if c.ld > c.s else i, W, b)
    assert out.coef.shape == (c.T, c.s) and out.n_dependent.dtype == torch.int32
    _assert_inside(c, _np(out), range(c.T), repr(c))
    if c.ld > c.s:                                                         # the whole list with s=: the same bits
        again = ops.support_refit(x, v, i, W, b, s=c.s)
        assert all(torch.equal(p, q) for p, q in zip(out, again))


# ---- 3: orthonormal supports -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,s,dtype", [(200, 32, "f32"), (203, 33, "bf16"), (1152, 64, "f16")])
def test_orthonormal_supports_return_y_bit_for_bit(dev, d, s, dtype):
    """Rows that are signed unit basis vectors: G is the exact identity, so coef is the gathered y (signed), gain its square."""
    from msae import ops

    rng = np.random.default_rng(d)
    T = 3
    col, sign = np.arange(ref.N) % d, np.where(rng.random(ref.N) < 0.5, -1.0, 1.0).astype(np.float32)
    W = np.zeros((ref.N, d), np.float32)
    W[np.arange(ref.N), col] = sign
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    x = ref.to_dtype(rng.standard_normal((T, d)).astype(np.float32), dtype)
    idx = np.stack([rng.permutation(min(d, ref.N))[:s] + d * rng.integers(0, max(ref.N // d, 1), s) for _ in range(T)]).astype(np.int64)
    vals = -np.sort(-rng.uniform(0.1, 2.0, (T, s)).astype(np.float32), 1)
    out = ops.support_refit(torch.from_numpy(x).to(dev, TDT[dtype]), torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev),
                            torch.from_numpy(W).to(dev), torch.from_numpy(b).to(dev))
    y = x - b
    want = sign[idx] * np.take_along_axis(y, col[idx], 1)
    assert np.array_equal(out.coef.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(out.gain.cpu().numpy().view(np.int32), (want * want).view(np.int32))
    assert (out.n_dependent == 0).all()


def test_tied_orthonormal_sae_refits_to_its_own_activations(dev):
    """Encoder tied to an orthonormal decoder, zero biases: the encoder's activations ARE the least-squares coefficients."""
    from msae import Sae, SaeConfig

    d = N = ref.N
    rng = np.random.default_rng(8)
    W = np.zeros((N, d), np.float32)
    W[np.arange(N), rng.permutation(d)] = np.where(rng.random(N) < 0.5, -1.0, 1.0)
    sae = Sae(d, SaeConfig(num_latents=N, k=32), device=dev)
    with torch.no_grad():
        sae.encoder.weight.copy_(torch.from_numpy(W))
        sae.W_dec.copy_(torch.from_numpy(W))
        sae.encoder.bias.zero_()
        sae.b_dec.zero_()
        x = torch.from_numpy(rng.standard_normal((5, d)).astype(np.float32)).to(dev)
        top = sae.encode(x)
        out = sae.refit(x)
    assert torch.equal(out.top_acts.view(torch.int32), top.top_acts.view(torch.int32)) and torch.equal(out.top_indices, top.top_indices)
    assert torch.equal(out.err_fit, out.err_enc) and float(out.gap) == 0.0 and (out.n_dependent == 0).all()


# ---- 4: dependent slots ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,s", [(200, 32), (203, 64)])
def test_a_repeated_index_is_dropped_and_counted(dev, d, s):
    from msae import ops

    c = ref.Case(d, s, 3, seed=5, dup=(1, 3, s - 2))
    out = _np(ops.support_refit(*_inputs(c, dev)))
    assert out["n_dependent"].tolist() == [0, 1, 0] and out["coef"][1, s - 2] == 0 and out["gain"][1, s - 2] == 0
    assert all(np.isfinite(v).all() for v in out.values())
    assert ref.premises(c, range(3)) == []
    _assert_inside(c, out, range(3), f"repeat {c!r}")                      # the restatement with that slot dropped


def test_an_index_out_of_range_is_dropped_and_flagged(dev):
    from msae import ops

    c = ref.Case(200, 33, 3, seed=6, bad=(2, 5), wide=True)
    args = _inputs(c, dev)
    out = _np(ops.support_refit(*args))
    assert out["coef"][2, 5] == 0 and out["gain"][2, 5] == 0 and (out["n_dependent"] == 0).all()
    _assert_inside(c, out, range(3), f"bad index {c!r}")
    ops.set_debug_bounds(True)
    try:
        ops.support_refit(*(a[:2] for a in args[:3]), *args[3:])             # tokens 0, 1: every index in range
        with pytest.raises(IndexError):
            ops.support_refit(*args)
    finally:
        ops.set_debug_bounds(False)


# ---- 5: bit-invariance -------------------------------------------------------------------------------------------------------
def test_a_token_has_the_same_bits_alone_in_a_batch_chunked_and_twice(dev):
    from msae import Sae, SaeConfig, ops

    c = ref.Case(203, 33, 257, dtype="bf16", seed=9, zeros=(4,))
    x, v, i, W, b = _inputs(c, dev)
    whole = ops.support_refit(x, v, i, W, b)
    again = ops.support_refit(x, v, i, W, b)
    assert all(torch.equal(p, q) for p, q in zip(whole, again))
    for t in (0, 100, 256):                                                 # T = 1
        one = ops.support_refit(x[t:t + 1], v[t:t + 1], i[t:t + 1], W, b)
        assert all(torch.equal(p[t:t + 1], q) for p, q in zip(whole, one)), t
    sae = Sae(c.d, SaeConfig(num_latents=ref.N, k=c.s), device=dev)
    with torch.no_grad():
        sae.W_dec.copy_(W)
        sae.b_dec.copy_(b)
    for chunk in (None, 100, 256):
        r = sae.refit(x, top=(v, i), chunk=chunk)
        got = (r.top_acts, r.gain, r.err_fit, r.err_enc, r.xx, r.n_dependent)
        assert all(torch.equal(p, q) for p, q in zip(whole, got)), chunk
    _assert_inside(c, _np(whole), (0, 128, 256), repr(c))


# ---- 6: Sae.refit end to end -------------------------------------------------------------------------------------------------
def test_sae_refit_end_to_end(dev):
    from msae import Sae, SaeConfig

    d, k, T = 256, 32, 48
    torch.manual_seed(3)
    sae = Sae(d, SaeConfig(num_latents=ref.N, k=k), device=dev)
    with torch.no_grad():
        sae.b_dec.copy_(0.1 * torch.randn(d, device=dev))
        x = (torch.randn(T, d, device=dev) + sae.b_dec).to(torch.bfloat16)
        top = sae.encode(x)
        sae.refit(x, top=top)                                               # (warm: the library is loaded, the op registered)
        with no_sync():
            out = sae.refit(x, top=top)
        own = sae.refit(x)                                                  # encodes by itself
        assert all(torch.equal(p, q) for p, q in zip(out[:7], own[:7]))
        recon = sae.decode(out.top_acts, out.top_indices)
        ks = [0, 1, 2, 4, 8, 16, 32]
        curve = sae.recon_error(x, ks, top=top)
    c = ref.Case.from_arrays(x.float().cpu().numpy(), top.top_acts.cpu().numpy(), top.top_indices.cpu().numpy(),
                             sae.W_dec.detach().cpu().numpy(), sae.b_dec.detach().cpu().numpy(), "bf16")
    tokens = range(0, T, 8)
    res = dict(coef=out.top_acts.cpu().numpy(), gain=out.gain.cpu().numpy(), err_fit=out.err_fit.cpu().numpy(),
               err_enc=out.err_enc.cpu().numpy(), yy=out.xx.cpu().numpy(), n_dependent=out.n_dependent.cpu().numpy())
    assert ref.premises(c, tokens) == []
    _assert_inside(c, res, tokens, "Sae.refit")
    assert float(out.gap) > 0 and float(out.fvu_fit) < float(out.fvu_enc)
    # decode(top_acts, top_indices) is the refit reconstruction: r = chain + b_dec against err_fit's y - chain, y = x - b_dec:
    # the two f32 roundings move a column's error by at most u (|x| + 2 |b| + |chain|) =: delta, the sum as in bound 4
    r64, x64, b64 = recon.double().cpu().numpy(), c.x.astype(np.float64), np.abs(c.b_dec.astype(np.float64))
    e = np.abs(r64 - x64)
    delta = 2 * ref.U * (np.abs(x64) + 2 * b64 + np.abs(r64))
    lim = (2 * e * delta + delta ** 2).sum(1) + ref.gamma(d + 8) * ((e + delta) ** 2).sum(1)
    direct = ((r64 - x64) ** 2).sum(1)
    print(f"decode vs err_fit: worst figure / bound {np.max(np.abs(direct - res['err_fit']) / lim):.3e}")
    assert (np.abs(direct - res["err_fit"]) <= lim).all()
    # the optimal curve is the lower envelope of recon_error's, checkpoint by checkpoint
    opt = out.optimal_curve(ks).cpu().numpy()
    enc = curve.err2.double().cpu().numpy()
    for t in tokens:
        r = ref.token_ref(c, t)
        for ci, kappa in enumerate(ks):
            pre = np.where(np.arange(k) < kappa, r.vals, 0.0)
            # optimal_curve <= recon_error's err2, each side by its derived distance from float64: the optimum yy - sum gain
            # by bound 3 and yy's own bound; recon_error's column error (chain + b_dec) - x by eval_bound's roundings (twice:
            # it rounds r and e) and u |b_dec| more.  Between them, in float64: opt[kappa] <= the objective at the encoder's point
            e_abs = np.abs(r.y - pre @ r.rows)
            g_sum = float(out.gain[t, :kappa].double().sum())
            slack = (ref.gain_bound(r, d, k, kappa, g_sum) + ref.gamma(d + 8) * r.yy
                     + 2 * r.eval_bound(pre, d, k) + 4 * ref.U * float(e_abs @ np.abs(c.b_dec)))
            assert opt[t, ci] <= enc[t, ci] + slack, (t, kappa)
            assert r.opt[kappa] <= r.objective(pre) * (1 + 1e-12)


# ---- 7: ReconStats(refit=True) through the cache ---------------------------------------------------------------------------
def test_recon_stats_refit_agrees_across_batch_cuts(dev, tmp_path):
    from msae import Sae, SaeConfig
    from msae.features import FeatureCache, ReconStats

    B, S, d, k = 4, 6, 200, 32
    c = ref.Case(d, k, B * S, dtype="f16", seed=12)
    x, v, i, W, b = _inputs(c, dev)
    sae = Sae(d, SaeConfig(num_latents=ref.N, k=k), device=dev)
    with torch.no_grad():
        sae.W_dec.copy_(W)
        sae.b_dec.copy_(b)
    ks, edges = (0, 1, 8, 32), (0, 2)
    x3, v3, i3 = x.view(B, S, d), v.view(B, S, k), i.view(B, S, k)
    stats = []
    for cuts in ((slice(0, 4),), (slice(0, 1), slice(1, 4))):
        fc = FeatureCache(fakes.TinyLlava(vocab=40, d=d).to(dev), None, {"layers.1": sae}, batch_size=2, shard_size=0,
                          recon=dict(ks=ks, position_edges=edges, refit=True))
        fc.cache.add_recon(x3[cuts[0]], v3[cuts[0]], i3[cuts[0]], sae, "layers.1")            # (warm)
        fc.cache.recon_stats.clear()
        with no_sync():
            for cut in cuts:
                fc.cache.add_recon(x3[cut], v3[cut], i3[cut], sae, "layers.1")
        stats.append(fc.cache.recon_stats["layers.1"])
    one, two = stats
    assert one.refit and one.refit_ks == ks and one.n == two.n == [8, 16]
    p, q = one.refit_sums.cpu().numpy(), two.refit_sums.cpu().numpy()
    assert (np.abs(p - q) <= 2 * 24 * 2.0 ** -53 * np.abs(p) * 2).all()     # identical per-token terms, float64 sums of 24
    assert torch.equal(one.sums, two.sums) or np.allclose(one.sums.cpu().numpy(), two.sums.cpu().numpy(), rtol=1e-13)
    # the float64 sums of the op's own per-token outputs (held to their bounds above), per position group
    from msae import ops

    raw = ops.support_refit(x, v, i, W, b)
    g64, yy64 = raw.gain.double().cpu().numpy(), raw.yy.double().cpu().numpy()
    opt = yy64[:, None] - np.concatenate([np.zeros((c.T, 1)), np.cumsum(g64, 1)], 1)[:, list(ks)]
    exp = ref.stats_sums(opt, np.tile(np.arange(S), B), ks, edges)
    assert (np.abs(p - exp) <= 2 * 24 * (k + 1) * 2.0 ** -53 * yy64.sum()).all()
    assert (p[:, 0] > p[:, 1]).all() and (p[:, 1] > p[:, 3]).all()
    path = str(tmp_path / "recon_stats.safetensors")
    one.save(path)
    back = ReconStats.load(path)
    assert back.refit and torch.equal(back.refit_sums, one.refit_sums.cpu()) and (back.gap()[1:] > 0).all()
