"""CPU: the Matryoshka feature's host side -- the plain-torch paths of ops.nested_decode /
ops.nested_reconstruct against the restatement tests/nested_ref.py, the power of that restatement's fixtures against its
nearly-correct variants, SaeConfig / Sae validation and serialisation, Sae.truncate, the C entry points' argument errors
(returned before any device work), and three optimisation steps driven by nested_loss against a literal torch loop.

Tolerances.  The host paths are f32 torch expressions with their own summation order, the restatement is the oracle's f32
chain: both lie within gamma_{k+2} A of the exact r_g, A = sum |v W| + |b| (k products, k additions, the bias), so they are
held to 2 gamma_{k+2} A of each other (e_g adds one exact-operand subtract on both sides: + 2 u |e|, covered by taking
gamma_{k+3} and adding |x| to A).  Gradients: nested_ref.grad_bound, doubled for the same reason."""
import json

import numpy as np
import pytest
import torch

import nested_ref as ref


def _t(c):
    return (torch.from_numpy(c["x"]), torch.from_numpy(c["vals"]), torch.from_numpy(c["idx"]), torch.from_numpy(c["W_dec"]),
            torch.from_numpy(c["b_dec"]))


def _amp(c, G):
    """A [T, d]: the sum of the magnitudes of everything that enters r_g - x."""
    W = np.abs(c["W_dec"].astype(np.float64))
    idx = np.clip(c["idx"], 0, W.shape[0] - 1)
    return (np.abs(c["vals"].astype(np.float64))[:, :, None] * W[idx]).sum(1) + np.abs(c["b_dec"]) + np.abs(c["x"])


def _fwd_close(got_out, got_E, exp, c):
    lim = 2 * ref.gamma(c["k"] + 3) * _amp(c, len(c["bounds"]))
    return ref.inside(got_out, exp["out"], lim) and all(ref.inside(got_E[g], exp["E"][g], lim) for g in range(len(c["bounds"])))


# ---- host paths against the restatement ------------------------------------------------------------------------------------
def test_host_decode_matches_the_restatement():
    from msae import ops

    c = ref.small_case()
    exp = ref.forward(c["x"], c["vals"], c["idx"], c["W_dec"], c["b_dec"], c["bounds"])
    out, sq, E = ops.nested_decode(*_t(c), c["bounds"], want_residuals=True)
    assert out.shape == (c["T"], c["d"]) and sq.shape == (c["T"], 4) and E.shape == (4, c["T"], c["d"])
    assert _fwd_close(out.numpy(), E.numpy(), exp, c)
    e2 = E.double().numpy() ** 2
    assert ref.inside(sq.numpy(), e2.sum(2).T, ref.gamma(c["d"] + 1) * e2.sum(2).T)
    assert ops.nested_decode(*_t(c), c["bounds"])[2] is None
    # lengths: the slots behind a row's length count for nothing, whatever they hold
    lengths = np.array([0, 1, 3, 8, 11, -2], dtype=np.int32)
    vals, idx = c["vals"].copy(), c["idx"].copy()
    tail = np.arange(c["k"])[None] >= np.clip(lengths, 0, c["k"])[:, None]
    exp_l = ref.forward(c["x"], vals, idx, c["W_dec"], c["b_dec"], c["bounds"], lengths)
    vals[tail], idx[tail] = 1e30, 10 ** 6
    x, _, _, W, b = _t(c)
    out_l, _, E_l = ops.nested_decode(x, torch.from_numpy(vals), torch.from_numpy(idx), W, b, c["bounds"], torch.from_numpy(lengths), True)
    assert _fwd_close(out_l.numpy(), E_l.numpy(), exp_l, c)
    assert np.array_equal(exp_l["E"][:, 0], np.broadcast_to((c["b_dec"] - c["x"][0]), (4, c["d"])))      # length 0: b_dec alone


def test_one_group_is_the_plain_decode_and_an_empty_group_repeats_the_one_before():
    from msae import ops

    c = ref.small_case()
    x, v, i, W, b = _t(c)
    out, sq, E = ops.nested_decode(x, v, i, W, b, [64], want_residuals=True)
    plain = ops.decode(i, v, W, b, torch.full((c["T"],), c["k"], dtype=torch.int32))
    assert torch.equal(out, plain) and torch.equal(E[0], plain - x)
    # bounds (4, 5, 6, 64) on a list without feature 4 or 5: the groups 1 and 2 are empty
    i2 = torch.where((i == 4) | (i == 5), torch.full_like(i, 7), i)
    _, sq2, E2 = ops.nested_decode(x, v, i2, W, b, [4, 5, 6, 64], want_residuals=True)
    assert torch.equal(E2[1], E2[0]) and torch.equal(E2[2], E2[0]) and torch.equal(sq2[:, 1], sq2[:, 0])
    assert not torch.equal(E2[3], E2[0])
    exp = ref.forward(c["x"], c["vals"], i2.numpy(), c["W_dec"], c["b_dec"], (4, 5, 6, 64))
    assert np.array_equal(exp["E"][1], exp["E"][0]) and np.array_equal(exp["E"][2], exp["E"][0])


def test_the_restatement_orders_by_group_then_slot():
    v = np.array([[5, 4, 3, 2, 1, 0.5]], dtype=np.float32)
    i = np.array([[40, 3, 16, 70, 2, 15]])
    vo, io, go, order, flagged = ref.group_major(v, i, (4, 16, 17, 64))
    assert flagged and order.tolist() == [[1, 4, 5, 2, 0, 3]]
    assert io.tolist() == [[3, 2, 15, 16, 40, 0]] and go.tolist() == [[0, 0, 1, 2, 3, 4]] and vo[0, -1] == 0
    assert ref.group_of([0, 3, 4, 15, 16, 17, 63], (4, 16, 17, 64)).tolist() == [0, 0, 1, 1, 2, 3, 3]
    from msae import ops
    tv, ti, tg, to = ops.nested_group_major(torch.from_numpy(v), torch.from_numpy(i), (4, 16, 17, 64))
    assert to.tolist() == order.tolist() and ti.tolist() == io.tolist() and tg.tolist() == go.tolist()


def test_fma_f32_rounds_once():
    # a b + c that float64 rounds onto the midpoint of two f32: 1 + 2^-24 + 2^-60 must round UP, not to even
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -12 + 2.0 ** -36), np.float32(1 - 2.0 ** -24)
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    got = Fraction(float(ref.fma_f32(a, b, c)))
    lo = Fraction(float(np.nextafter(np.float32(float(got)), np.float32(-np.inf))))
    hi = Fraction(float(np.nextafter(np.float32(float(got)), np.float32(np.inf))))
    assert abs(got - exact) <= min(abs(lo - exact), abs(hi - exact))
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    got = ref.fma_f32(a, b, c)
    for n in range(0, 2000, 97):
        exact = Fraction(float(a[n])) * Fraction(float(b[n])) + Fraction(float(c[n]))
        g = np.float32(got[n])
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(np.nextafter(g, np.float32(np.inf)))) - exact)
        assert err <= abs(Fraction(float(np.nextafter(g, np.float32(-np.inf)))) - exact)


# ---- the autograd path on the host, and the power of the fixtures ----------------------------------------------------------
def _host_grads(c, with_full=True):
    from msae import ops

    x, v, i, W, b = _t(c)
    v, W, b = v.clone().requires_grad_(), W.clone().requires_grad_(), b.clone().requires_grad_()
    out, sq_sum = ops.nested_reconstruct(x, v, i, W, b, c["bounds"])
    half = torch.from_numpy(c["coef"]) / 2                 # coef = 2 dL / d sq_sum
    loss = (sq_sum * half).sum() + ((out * torch.from_numpy(c["grad_full"])).sum() if with_full else 0.0)
    loss.backward()
    return v.grad.numpy(), W.grad.numpy(), b.grad.numpy()


def _ref_grads(c, with_full=True, variant=None):
    fwd = ref.forward(c["x"], c["vals"], c["idx"], c["W_dec"], c["b_dec"], c["bounds"],
                      variant=variant if variant in ref.VARIANTS_FWD else None)
    S, S_abs = ref.combine(fwd["E"], c["coef"], c["grad_full"] if with_full else None,
                           variant=variant if variant in ref.VARIANTS_BWD else None)
    return ref.backward(c["vals"], c["idx"], c["W_dec"], c["bounds"], S, S_abs)


def _grads_inside(got, exp, c) -> bool:
    G, d = len(c["bounds"]), c["d"]
    # twice the kernel's bound: the host expression and the restatement each round their own way, and the f32 residuals
    # under S differ by the forward tolerance above (|coef| <= 2, folded into the same sum of magnitudes)
    k_fwd = 2 * ref.gamma(c["k"] + 3) * 2.0 * G * _amp(c, G).max()
    ga, gW, gb = got
    return (ref.inside(ga, exp["g_acts"], 2 * ref.grad_bound(exp["g_acts_abs"], d, G) + k_fwd * np.abs(c["W_dec"]).sum(1).max()) and
            ref.inside(gW, exp["g_W"], 2 * ref.grad_bound(exp["g_W_abs"], d, G) + k_fwd * np.abs(c["vals"]).sum()) and
            ref.inside(gb, exp["g_b"], 2 * ref.grad_bound(exp["g_b_abs"], d, G) + k_fwd * c["T"]))


def test_host_gradients_match_the_restatement():
    c = ref.small_case()
    for with_full in (True, False):
        assert _grads_inside(_host_grads(c, with_full), _ref_grads(c, with_full), c)
    # a zero activation still receives its gradient S[group] . W[i], as ops.decode's backward gives it
    assert c["vals"][0, 4] == 0 and _ref_grads(c)["g_acts"][0, 4] != 0


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_the_fixtures_reject_every_wrong_variant(variant):
    from msae import ops

    c = ref.small_case()
    if variant in ref.VARIANTS_FWD:
        out, _, E = ops.nested_decode(*_t(c), c["bounds"], want_residuals=True)
        wrong = ref.forward(c["x"], c["vals"], c["idx"], c["W_dec"], c["b_dec"], c["bounds"], variant=variant)
        assert not _fwd_close(out.numpy(), E.numpy(), wrong, c), variant
    assert not _grads_inside(_host_grads(c), _ref_grads(c, variant=variant), c), variant


def test_ops_argument_errors():
    from msae import ops

    c = ref.small_case()
    x, v, i, W, b = _t(c)
    for bad in ([], [4, 4, 64], [16, 4, 64], [0, 64], [4, 63], [4, 65], list(range(1, 9)) + [64], [4.5, 64], "ab"):
        with pytest.raises(ValueError):
            ops.nested_decode(x, v, i, W, b, bad)
    with pytest.raises(ValueError, match="share d"):
        ops.nested_decode(x[:, :5], v, i, W, b, [64])
    with pytest.raises(ValueError, match="b_dec"):
        ops.nested_decode(x, v, i, W, None, [64])
    with pytest.raises(ValueError, match="float32, bfloat16"):
        ops.nested_decode(x.double(), v, i, W, b, [64])
    with pytest.raises(ValueError, match="one shape"):
        ops.nested_decode(x, v, i[:, :3], W, b, [64])
    with pytest.raises(ValueError, match="one row per token"):
        ops.nested_decode(x[:3], v, i, W, b, [64])
    with pytest.raises(ValueError, match="int32 or int64"):
        ops.nested_decode(x, v, i.to(torch.int16), W, b, [64])
    with pytest.raises(ValueError, match="values must be float32"):
        ops.nested_decode(x, v.double(), i, W, b, [64])
    with pytest.raises(ValueError, match="lengths"):
        ops.nested_reconstruct(x, v, i, W, b, [64], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="inference path"):
        ops.nested_decode(x, v.clone().requires_grad_(), i, W, b, [64])


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    import ctypes

    from msae import _hip

    lib = _hip.load()
    EINVAL = lib.msae_nested_decode_f32(None, 0, None, None, 0, None, None, 1, None, None, 1, 1, 1, 1, None, None, None, None, None)
    assert EINVAL != 0 and EINVAL == lib.msae_recon_curve_f32(None, 0, None, None, 0, None, None, 1, 1, 1, 1, None, 1, None, None, None, None)
    p = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments

    def call(fn=lib.msae_nested_decode_f32, dt=_hip.DTYPE_CODE[torch.float32], ld=8, bounds=(4, 64), G=2, T=3, k=8, N=64, d=16, x=p, out=p, sq=p):
        b = (ctypes.c_int32 * max(len(bounds), 1))(*bounds)
        return fn(x, dt, p, p, ld, None, b, G, p, p, T, k, N, d, out, None, sq, None, None)

    for fn in (lib.msae_nested_decode_f32, lib.msae_nested_decode_i64_f32):
        assert call(fn, T=0) == 0
        for kw in (dict(T=-1), dict(k=0), dict(k=4097, ld=4097), dict(ld=7), dict(N=0), dict(d=0), dict(G=0), dict(G=9), dict(dt=77),
                   dict(x=None), dict(out=None), dict(sq=None), dict(bounds=(4, 63)), dict(bounds=(4, 65)), dict(bounds=(64, 64)),
                   dict(bounds=(0, 64)), dict(bounds=(70, 64))):
            assert call(fn, **kw) == EINVAL, kw
    assert lib.msae_nested_combine_f32(p, p, None, 0, 4, 2, None) == 0
    for args in ((None, p, None, 1, 4, 2), (p, None, None, 1, 4, 2), (p, p, None, -1, 4, 2), (p, p, None, 1, 0, 2), (p, p, None, 1, 4, 0),
                 (p, p, None, 1, 4, 9)):
        assert lib.msae_nested_combine_f32(*args, None) == EINVAL, args
    assert lib.msae_decode_bwd_acts_grouped_f32(p, p, None, 2, p, 1, 1, 4, 4, p, None, None) == EINVAL
    assert lib.msae_decode_bwd_acts_grouped_f32(p, p, p, 9, p, 1, 1, 4, 4, p, None, None) == EINVAL
    assert lib.msae_decode_bwd_acts_grouped_f32(p, p, p, 2, p, 0, 1, 4, 4, p, None, None) == 0
    assert lib.msae_decode_bwd_wdec_grouped_f32(p, p, p, None, 2, 1, 1, 4, 4, p, None, None, None, p, 1 << 20, None) == EINVAL
    assert lib.msae_decode_bwd_wdec_grouped_f32(p, p, p, p, 0, 1, 1, 4, 4, p, None, None, None, p, 1 << 20, None) == EINVAL
    assert lib.msae_decode_bwd_wdec_grouped_f32(p, p, p, p, 2, 1, 1, 4, 6, p, None, None, None, p, 1 << 20, None) == EINVAL
    assert lib.msae_decode_bwd_wdec_grouped_f32(p, p, p, p, 2, 1, 1, 4, 4, p, None, None, None, None, 0, None) != 0     # no workspace
    assert lib.msae_abi_version() == 4


# ---- SaeConfig and Sae -----------------------------------------------------------------------------------------------------
def test_config_validation():
    from msae import Sae, SaeConfig

    ok = SaeConfig(num_latents=64, k=4, matryoshka=[8, 16, 64], matryoshka_weights=[1, 0, 2.5])
    assert ok.nested_weights == [1.0, 0.0, 2.5] and SaeConfig(num_latents=64, matryoshka=[8, 64]).nested_weights == [0.5, 0.5]
    for kw in (dict(matryoshka=[8, 8, 64]), dict(matryoshka=[16, 8, 64]), dict(matryoshka=[0, 64]), dict(matryoshka=list(range(1, 10))),
               dict(matryoshka=[8.5, 64]), dict(matryoshka=[8, 64], matryoshka_weights=[1.0]),
               dict(matryoshka=[8, 64], matryoshka_weights=[1.0, float("nan")]), dict(matryoshka=[8, 64], matryoshka_weights=[1.0, -0.5]),
               dict(matryoshka=[8, 64], matryoshka_weights=[0.0, 0.0]), dict(matryoshka=[8, 64], matryoshka_weights=[1.0, float("inf")]),
               dict(matryoshka_weights=[1.0]), dict(matryoshka=[8, 64], multi_topk=True), dict(matryoshka=[8, 32], num_latents=64)):
        with pytest.raises(ValueError):
            SaeConfig(**kw)
    with pytest.raises(ValueError, match="multi_topk"):
        SaeConfig(matryoshka=[8, 64], multi_topk=True)
    # only Sae.__init__ knows d_in: the last size must be the dictionary's width
    with pytest.raises(ValueError, match="number of latents"):
        Sae(4, SaeConfig(expansion_factor=8, matryoshka=[8, 64]))
    Sae(4, SaeConfig(expansion_factor=16, matryoshka=[8, 64]))
    SaeConfig(num_latents=64, k=4, activation="batchtopk", matryoshka=[8, 64])


def test_cfg_json_round_trip_and_an_unchanged_topk_checkpoint(tmp_path):
    from msae import Sae, SaeConfig

    plain = Sae(8, SaeConfig(num_latents=64, k=4))
    plain.save_to_disk(tmp_path / "plain")
    assert (tmp_path / "plain" / "cfg.json").read_text() == \
        '{"expansion_factor": 32, "normalize_decoder": true, "num_latents": 64, "k": 4, "multi_topk": false, "signed": false, "d_in": 8}'
    assert list(plain.state_dict()) == ["W_dec", "b_dec", "encoder.weight", "encoder.bias"]
    from safetensors import safe_open
    with safe_open(str(tmp_path / "plain" / "sae.safetensors"), "pt") as f:
        assert sorted(f.keys()) == ["W_dec", "b_dec", "encoder.bias", "encoder.weight"]

    cfg = SaeConfig(num_latents=64, k=4, matryoshka=[8, 16, 64], matryoshka_weights=[0.5, 0.25, 0.25])
    sae = Sae(8, cfg)
    assert list(sae.state_dict()) == list(plain.state_dict())                  # the weights buffer is not saved
    sae.save_to_disk(tmp_path / "nested")
    d = json.loads((tmp_path / "nested" / "cfg.json").read_text())
    assert d["matryoshka"] == [8, 16, 64] and d["matryoshka_weights"] == [0.5, 0.25, 0.25] and "activation" not in d
    back = Sae.load_from_disk(tmp_path / "nested")
    assert back.cfg == cfg and torch.equal(back._nested_w, torch.tensor([0.5, 0.25, 0.25]))
    assert torch.equal(back.W_dec, sae.W_dec)
    assert "matryoshka_weights" not in SaeConfig(num_latents=64, matryoshka=[8, 64]).to_dict()
    assert SaeConfig.from_dict(SaeConfig(num_latents=64, matryoshka=[8, 64]).to_dict()).matryoshka == [8, 64]


def test_truncate_shares_storage_unless_copied():
    from msae import Sae, SaeConfig

    sae = Sae(8, SaeConfig(num_latents=64, k=4, activation="batchtopk", batch_cap=8, matryoshka=[8, 16, 64], matryoshka_weights=[0.5, 0.5, 0.0]))
    sae.set_threshold(0.25)
    t = sae.truncate(16)
    assert isinstance(t, Sae) and t.num_latents == 16 and t.cfg.num_latents == 16 and t.cfg.matryoshka == [8, 16]
    assert t.cfg.matryoshka_weights == [0.5, 0.5] and float(t.threshold) == 0.25 and t.cfg.k == 4
    assert t.encoder.weight.shape == (16, 8) and t.W_dec.shape == (16, 8) and t.encoder.bias.shape == (16,)
    for a, b in ((t.encoder.weight, sae.encoder.weight), (t.encoder.bias, sae.encoder.bias), (t.W_dec, sae.W_dec), (t.b_dec, sae.b_dec)):
        assert a.data_ptr() == b.data_ptr() and a.is_contiguous()
    with torch.no_grad():
        sae.W_dec[3, 2] = 7.0
    assert float(t.W_dec.detach()[3, 2]) == 7.0
    assert list(t.state_dict()) == list(sae.state_dict()) and t._prepared is None
    c = sae.truncate(16, copy=True)
    assert c.W_dec.data_ptr() != sae.W_dec.data_ptr() and torch.equal(c.W_dec, sae.W_dec[:16])
    with torch.no_grad():
        sae.W_dec[3, 2] = 9.0
    assert float(c.W_dec.detach()[3, 2]) == 7.0
    # a size that is no bound becomes the last one, with uniform weights; a plain Sae stays plain
    assert sae.truncate(20).cfg.matryoshka == [8, 16, 20] and sae.truncate(20).cfg.matryoshka_weights == []
    assert sae.truncate(8).cfg.matryoshka == [8]
    assert Sae(8, SaeConfig(num_latents=64, k=4)).truncate(10).cfg.matryoshka == []
    for bad in (7, 65, 0):
        with pytest.raises(ValueError, match="truncate"):
            sae.truncate(bad)
    assert "RE-SELECTS" in Sae.truncate.__doc__ and "nested_error" in Sae.truncate.__doc__


def test_nested_error_argument_errors():
    from msae import Sae, SaeConfig

    plain, x = Sae(8, SaeConfig(num_latents=64, k=4)), torch.zeros(3, 8)
    with pytest.raises(ValueError, match="bounds"):
        plain.nested_error(x)
    with pytest.raises(ValueError, match="number of latents"):
        plain.nested_error(x, [8, 32])
    with pytest.raises(ValueError, match=r"\[\.\.\., 8\]"):
        plain.nested_error(torch.zeros(3, 9), [8, 64])
    with pytest.raises(ValueError, match="top must be"):
        plain.nested_error(x, [8, 64], top=(x,))
    # with the list in hand the host path answers
    top = (torch.rand(3, 4), torch.randint(0, 64, (3, 4)))
    out = plain.nested_error(x + 1, [8, 64], top=top)
    assert out.err2.shape == (3, 2) and out.xnorm2.shape == (3,) and out.fvu.dtype == torch.float64 and out.bounds == (8, 64)
    assert torch.allclose(out.xnorm2, torch.full((3,), 8.0))


# ---- three optimisation steps on the host path -----------------------------------------------------------------------------
def _cpu_train_step(sae, lr, **kw):
    from msae import ops
    from msae.sae.sae import NestedForwardOutput
    from msae.train import SaeTrainStep

    class CpuTrainStep(SaeTrainStep):
        def _forward(self, x, dead_mask):
            s = self.sae
            pre = torch.relu((x - s.b_dec) @ s.encoder.weight.T + s.encoder.bias)
            acts, idx = pre.topk(s.cfg.k, dim=-1)
            bounds = tuple(s.cfg.matryoshka)
            out, sq_sum = ops.nested_reconstruct(x, acts, idx, s.W_dec, s.b_dec, bounds)
            nested_fvu = sq_sum / (x - x.mean(0)).pow(2).sum()
            zero = out.new_zeros(())
            return NestedForwardOutput(out, acts, idx, nested_fvu[-1], zero, zero, nested_fvu=nested_fvu,
                                       nested_loss=(nested_fvu * s._nested_w).sum(), bounds=bounds)

        def _update(self, lr):
            with torch.no_grad():
                for p in self.params:
                    p.add_(p.grad, alpha=-lr)
                    p.grad = None

    return CpuTrainStep(sae, lr=lr, **kw)


def test_three_training_steps_descend_on_the_nested_loss():
    import synth
    from msae import Sae, SaeConfig

    d, N, k, T, lr = 16, 64, 4, 24, 0.05
    bounds, w = [8, 24, 64], [0.5, 0.3, 0.2]
    sae = Sae(d, SaeConfig(num_latents=N, k=k, normalize_decoder=False, matryoshka=bounds, matryoshka_weights=w))
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, N, seed=4)
    with torch.no_grad():
        sae.encoder.weight.copy_(torch.from_numpy(W_enc)); sae.encoder.bias.copy_(torch.from_numpy(b_enc))
        sae.W_dec.copy_(torch.from_numpy(W_dec)); sae.b_dec.copy_(torch.from_numpy(b_dec))
    x = torch.from_numpy(synth.activations(T, d, seed=6, bf16=False, n_outlier=1))

    start = {n: v.detach().clone() for n, v in sae.named_parameters()}

    def literal(weights, steps=3):
        """The definition, written out: dense latents, the first m_g columns alone, the weighted FVUs, plain SGD."""
        p = {n: v.detach().clone().requires_grad_() for n, v in start.items()}
        fvus = []
        for _ in range(steps):
            for chunk in x.chunk(2):
                pre = torch.relu((chunk - p["b_dec"]) @ p["encoder.weight"].T + p["encoder.bias"])
                acts, idx = pre.topk(k, dim=-1)
                z = torch.zeros(chunk.shape[0], N).scatter(1, idx, acts)
                tv = (chunk - chunk.mean(0)).pow(2).sum()
                fvu = torch.stack([((z[:, :m] @ p["W_dec"][:m] + p["b_dec"] - chunk) ** 2).sum() / tv for m in bounds])
                ((fvu * torch.tensor(weights)).sum() / 2).backward()
                fvus.append(fvu.detach())
            with torch.no_grad():
                for v in p.values():
                    v.add_(v.grad, alpha=-lr)
                    v.grad = None
        return p, fvus

    ts = _cpu_train_step(sae, lr, micro_acc_steps=2)
    results = [ts.step(x) for _ in range(3)]
    want, fvus = literal(w)
    plain, _ = literal([0.0, 0.0, 1.0])
    for n, v in sae.named_parameters():
        # f32 against f32 in another summation order: three steps of lr times gradients that are sums of at most T k d products of
        # O(1) terms -- relative 3 lr gamma_{T k} -- far below the distance to a step on the plain FVU
        assert torch.allclose(v, want[n], rtol=1e-4, atol=3 * lr * ref.gamma(T * k) * 10), n
        assert not torch.allclose(v, plain[n], rtol=1e-3, atol=1e-5), f"{n}: the nested loss did not drive the update"
    assert all(r["stepped"] for r in results)
    got = results[-1]["nested_fvu"]
    assert got.shape == (3,) and torch.allclose(got, (fvus[-2] + fvus[-1]) / 2, rtol=1e-4)
    assert torch.allclose(results[-1]["fvu"], got[-1])
