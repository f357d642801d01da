"""Support refit, everything that needs no GPU: the restatement's prefix identity, the float64 fallback
of ops.support_refit, the POWER of the bounds the GPU test uses (a plain-f32 solve lies inside every one, each nearly-right
solver outside one), argument errors, the C entries' argument checks, ReconStats(refit=True) and its off switch, the
command line."""
import ctypes
import os

import numpy as np
import pytest
import torch

import refit_ref as ref
from msae import Sae, SaeConfig, _hip, ops
from msae.features import Cache, ReconStats
from msae.sae import RefitOutput


def _sae(d, N, k, W=None, b=None):
    sae = Sae(d, SaeConfig(num_latents=N, k=k))
    if W is not None:
        with torch.no_grad():
            sae.W_dec.copy_(torch.from_numpy(W))
            sae.b_dec.copy_(torch.from_numpy(b))
    return sae


def _run(c: ref.Case, s=None):
    out = ops.support_refit(torch.from_numpy(c.x), torch.from_numpy(c.vals), torch.from_numpy(c.idx),
                            torch.from_numpy(c.W_dec), torch.from_numpy(c.b_dec), s)
    return {k: v.numpy() for k, v in out._asdict().items()}


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,s", [(64, 1), (64, 32), (200, 64), (203, 33)])
def test_prefix_identity_of_the_restatement(d, s):
    """yy - sum_{j < kappa} z_j^2 with z from ONE float64 Cholesky of the full Gram matrix equals the literal lstsq of every
    prefix, to float64 rounding at the Gram matrix's conditioning."""
    c = ref.Case(d, s, 2, seed=11, zeros=(0,) if s > 2 else ())
    for t in range(c.T):
        r = ref.token_ref(c, t)
        L = np.linalg.cholesky(r.G)
        z = np.linalg.solve(L, r.h)
        pre = np.concatenate([[0.0], np.cumsum(z * z)])
        kept = np.concatenate([[0], np.cumsum(r.keep)])
        for kappa in range(s + 1):
            assert abs((r.yy - pre[kept[kappa]]) - r.opt[kappa]) <= 1e-12 * r.cond * r.yy, (t, kappa)
        assert (np.diff(r.opt) <= 1e-12 * r.yy).all()                   # a larger support never fits worse


# ---- ops.support_refit off the GPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(d=64, s=8, T=3), dict(d=200, s=33, T=2, dtype="bf16", wide=True, ld=40, zeros=(0, 5, 32)),
                                dict(d=64, s=6, T=3, bad=(1, 2)), dict(d=64, s=6, T=3, dup=(2, 1, 4))], ids=str)
def test_fallback_meets_the_restatement(kw):
    c = ref.Case(**kw)
    out = _run(c, c.s)
    assert ref.premises(c, range(c.T)) == [] and ref.violations(c, out, range(c.T)) == []
    assert out["coef"].shape == (c.T, c.s) and out["n_dependent"].dtype == np.int32
    if c.ld > c.s:                                                       # the longer list is read on its first s slots
        short = ops.support_refit(torch.from_numpy(c.x), torch.from_numpy(c.vals[:, :c.s].copy()),
                                  torch.from_numpy(c.idx[:, :c.s].copy()), torch.from_numpy(c.W_dec), torch.from_numpy(c.b_dec))
        assert all(np.array_equal(out[k], v.numpy()) for k, v in short._asdict().items())


def test_sae_refit_on_the_cpu_and_its_properties():
    c = ref.Case(64, 8, 6, seed=3)
    sae = _sae(c.d, ref.N, c.s, c.W_dec, c.b_dec)
    x = torch.from_numpy(c.x)
    top = (torch.from_numpy(c.vals), torch.from_numpy(c.idx))
    out = sae.refit(x.view(2, 3, c.d), top=(top[0].view(2, 3, c.s), top[1].view(2, 3, c.s)))
    assert isinstance(out, RefitOutput) and out.top_acts.shape == (2, 3, c.s) and out.err_fit.shape == (2, 3)
    assert torch.equal(out.top_indices, top[1].view(2, 3, c.s))
    flat = {k: getattr(out, k).reshape(c.T, -1).squeeze(-1).numpy() for k in ("gain", "err_fit", "err_enc", "n_dependent")}
    flat.update(coef=out.top_acts.reshape(c.T, c.s).numpy(), yy=out.xx.reshape(c.T).numpy())
    assert ref.violations(c, flat, range(c.T)) == []
    tv = float(((x.double() - x.double().mean(0)) ** 2).sum())
    assert out.fvu_fit.dtype == torch.float64 and np.isclose(float(out.fvu_fit), flat["err_fit"].astype(np.float64).sum() / tv, rtol=1e-12)
    assert np.isclose(float(out.gap), (flat["err_enc"].astype(np.float64) - flat["err_fit"].astype(np.float64)).sum() / tv, rtol=1e-9)
    assert float(out.gap) > 0 and float(out.fvu_enc) > float(out.fvu_fit)
    curve = out.optimal_curve([0, 1, c.s]).reshape(c.T, 3).numpy()
    for t in range(c.T):
        r = ref.token_ref(c, t)
        assert np.allclose(curve[t], r.opt[[0, 1, c.s]], rtol=1e-4, atol=1e-6 * r.yy)
    # the refit reconstruction is what decode makes of (top_acts, top_indices): W_dec[idx]^T acts + b_dec
    recon = np.einsum("tj,tjc->tc", flat["coef"].astype(np.float64), c.W_dec[c.idx].astype(np.float64)) + c.b_dec
    assert np.allclose(((recon - c.x) ** 2).sum(-1), flat["err_fit"], rtol=1e-4)
    part = sae.refit(x, top=top, chunk=4)
    assert torch.equal(part.top_acts, out.top_acts.reshape(c.T, c.s)) and torch.equal(part.err_fit, out.err_fit.reshape(c.T))
    assert sae.refit(x[:0], top=(top[0][:0], top[1][:0])).top_acts.shape == (0, c.s)


# ---- power ---------------------------------------------------------------------------------------------------------------
POWER = ref.Case(64, 8, 3, zeros=(2,), seed=1)


def test_a_plain_f32_solve_lies_inside_every_bound():
    assert ref.premises(POWER, range(POWER.T)) == []
    assert ref.violations(POWER, ref.solve(POWER, "f32"), range(POWER.T)) == []


@pytest.mark.parametrize("solver", [s for s in ref.SOLVERS if s != "f32"])
def test_every_nearly_right_solver_falls_outside(solver):
    bad = ref.violations(POWER, ref.solve(POWER, solver), range(POWER.T))
    assert bad, solver
    want = {"diagonal": "residual", "no_bias": "residual", "keep_zeros": "outside the support", "no_back_solve": "residual",
            "reversed_prefix": "gain[", "coef_1e-3": "residual"}[solver]
    assert any(want in b for b in bad), (solver, bad[:3])


def test_tau_separates_a_repeated_index_from_a_random_row():
    for d, s in ((64, 2), (4096, 64)):
        t = ref.tau(d, s)
        assert 3 * ref.U < t < 0.25 * (1 - s / d) and t == ops.refit_tau(d, s)


# ---- argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_device_work():
    d, N, k, T = 8, 16, 4, 3
    x, v, i = torch.zeros(T, d), torch.ones(T, k), torch.zeros(T, k, dtype=torch.int64)
    W, b = torch.zeros(N, d), torch.zeros(d)
    big = dict(v=torch.ones(T, 65), i=torch.zeros(T, 65, dtype=torch.int64))
    bad = [
        (dict(s=0), "s must be"), (dict(s=k + 1), "s must be"), (dict(s=1.5), "integer"), (dict(s=True), "integer"),
        (big, "s must be"), ({**big, "s": 65}, "s must be"),
        (dict(x=torch.zeros(T, d + 1)), "share d"), (dict(x=torch.zeros(T, d, dtype=torch.float64)), "float32"),
        (dict(v=torch.ones(T, k + 1)), "share one shape"), (dict(v=torch.ones(T + 1, k), i=torch.zeros(T + 1, k, dtype=torch.int64)), "one row"),
        (dict(i=torch.zeros(T, k, dtype=torch.int16)), "int32 or int64"), (dict(v=torch.ones(T, k, dtype=torch.float64)), "float32"),
        (dict(b=torch.zeros(d + 1)), "b_dec"), (dict(b=None), "b_dec"),
    ]
    for kw, msg in bad:
        a = dict(x=x, v=v, i=i, W=W, b=b, s=None)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.support_refit(a["x"], a["v"], a["i"], a["W"], a["b"], a["s"])
    assert ops.support_refit(x, big["v"], big["i"], W, b, s=64).coef.shape == (T, 64)      # a long list on its first 64 slots
    with pytest.raises(RuntimeError, match="inference"):
        ops.support_refit(x.clone().requires_grad_(True), v, i, W, b)
    sae = _sae(d, N, k)
    for kw, msg in ((dict(s=k + 1), "s must be"), (dict(s=0), "s must be"), (dict(chunk=0), "chunk"), (dict(top=(v,)), "pair")):
        with pytest.raises(ValueError, match=msg):
            sae.refit(x, **{"top": (v, i), **kw})
    with pytest.raises(ValueError, match="pass s=64"):
        sae.refit(x, top=(big["v"], big["i"]))
    with pytest.raises(ValueError, match="pass s=64"):
        _sae(d, 128, 65).refit(x)
    with pytest.raises(ValueError, match="must be"):
        sae.refit(torch.zeros(T, d + 1), top=(v, i))
    with pytest.raises(RuntimeError, match="inference"):
        sae.refit(x.clone().requires_grad_(True), top=(v, i))
    for cfg in (dict(activation="batchtopk"), dict(activation="jump"), dict(transcode=True)):
        with pytest.raises(NotImplementedError):
            Sae(d, SaeConfig(num_latents=N, k=k, **cfg)).refit(x)
    from msae.parallel import ShardedSae

    with pytest.raises(NotImplementedError, match="msae.Sae"):
        ShardedSae.refit(object(), None)


def test_the_c_entries_check_their_arguments():
    lib = _hip.load()
    one = ctypes.c_void_p(16)
    for name in ("msae_support_refit_f32", "msae_support_refit_i64_f32"):
        f = getattr(lib, name)
        args = lambda **kw: [kw.get("x", one), kw.get("dt", 0), one, kw.get("idx", one), kw.get("ld", 4), one, kw.get("b", one),
                             kw.get("T", 1), kw.get("s", 4), kw.get("N", 8), kw.get("d", 8), kw.get("coef", one), one, one, one,
                             one, kw.get("nd", one), None, None]
        assert f(*args(T=0)) == 0
        einval = f(*args(s=0))
        assert einval != 0 and einval == lib.msae_recon_curve_f32(None, 0, None, None, 0, None, None, 1, 1, 1, 1, None, 1, None,
                                                                  None, None, None)
        for kw in (dict(s=65, ld=65), dict(ld=3), dict(x=None), dict(idx=None), dict(b=None), dict(coef=None), dict(nd=None),
                   dict(dt=9), dict(T=-1), dict(N=0), dict(d=0), dict(d=(1 << 22) + 1)):
            assert f(*args(**kw)) == einval, kw
    assert ops.REFIT_MAX_S == 64


# ---- ReconStats(refit=True) ------------------------------------------------------------------------------------------------
def _parts(seed=5):
    B, S = 2, 6
    cases = [ref.Case(32, 8, B * S, seed=seed + n) for n in range(3)]
    W, b = cases[0].W_dec, cases[0].b_dec                  # (the same seed -> d -> rows: one dictionary for the three)
    for c in cases:
        c.W_dec, c.b_dec = W, b
    sae = _sae(32, ref.N, 8, W, b)
    return sae, [(c.x.reshape(B, S, 32), c.vals.reshape(B, S, 8), c.idx.reshape(B, S, 8).astype(np.int64)) for c in cases], cases


def _stat(sae, parts, refit=True, ks=(0, 1, 4, 8), edges=(0, 4)):
    st = ReconStats(sae.d_in, ks, position_edges=edges, refit=refit)
    for x, v, i in parts:
        st.update(torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(i), sae)
    return st


def test_recon_stats_refit_sums_merge_and_file(tmp_path):
    sae, parts, cases = _parts()
    ks, edges = (0, 1, 4, 8), (0, 4)
    whole = _stat(sae, parts)
    assert whole.refit and whole.refit_ks == ks and whole.refit_sums.shape == (2, 4) and whole.refit_sums.dtype == torch.float64
    # against the restatement: the optimal error of every token at every checkpoint, summed per position group
    opt = np.stack([ref.TokenRef(c, t).opt[list(ks)] for c in cases for t in range(c.T)])
    pos = np.tile(np.arange(6), 6)
    exp = ref.stats_sums(opt, pos, ks, edges)
    assert np.allclose(whole.refit_sums.numpy(), exp, rtol=1e-4)
    merged = _stat(sae, parts[:1]).merge(_stat(sae, parts[1:]))
    assert (np.abs(merged.refit_sums.numpy() - whole.refit_sums.numpy()) <= 36 * 2.0 ** -52 * np.abs(whole.refit_sums.numpy())).all()
    assert merged.n == whole.n
    # the optimum lies below the encoder's own error; the gap is what separates them
    gap, fit, fvu = whole.gap(), whole.fvu_fit(), whole.fvu()
    assert gap.dtype == torch.float64 and gap.shape == (4,) and (gap[1:] > 0).all() and abs(float(gap[0])) < 1e-6
    assert torch.allclose(fit + gap, fvu, rtol=1e-12) and (whole.gap(1)[1:] > 0).all()
    assert "gap" in whole.summary().splitlines()[0] and len(whole.summary().splitlines()) == 5
    with pytest.raises(ValueError, match="different kinds"):
        whole.merge(_stat(sae, parts, refit=False))
    with pytest.raises(ValueError, match="without refit"):
        _stat(sae, parts[:1], refit=False).gap()
    path = str(tmp_path / "recon_stats.safetensors")
    whole.save(path)
    back = ReconStats.load(path)
    assert back.refit and back.refit_ks == ks and torch.equal(back.refit_sums, whole.refit_sums) and torch.equal(back.gap(), gap)
    # checkpoints above 64 are reported by the curve alone
    assert ReconStats(8, (1, 64, 65, 128), refit=True).refit_ks == (1, 64)


def test_off_switch_leaves_the_file_and_the_sums_as_they_were(tmp_path):
    sae, parts, _ = _parts(9)
    plain = ReconStats(sae.d_in, (0, 1, 4, 8), position_edges=(0, 4))
    off = _stat(sae, parts, refit=False)
    for x, v, i in parts:
        plain.update(torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(i), sae)
    plain.save(str(tmp_path / "plain.safetensors"))
    off.save(str(tmp_path / "off.safetensors"))
    _stat(sae, parts).save(str(tmp_path / "on.safetensors"))
    # (safetensors writes the metadata keys in an order of its own from save to save: the files are compared as what they
    # hold -- the same length, the same metadata, the same tensors bit for bit)
    from safetensors import safe_open

    held = []
    for name in ("plain", "off"):
        with safe_open(str(tmp_path / f"{name}.safetensors"), "pt") as f:
            held.append((os.path.getsize(tmp_path / f"{name}.safetensors"), f.metadata(),
                         {k: f.get_tensor(k).numpy().tobytes() for k in sorted(f.keys())}))
    assert held[0] == held[1] and sorted(held[0][2]) == ["b_dec", "cos_sum", "sums", "x_sum", "xx_sum"]
    assert sorted(held[0][1]) == ["d", "format", "ks", "n", "position_edges"]
    assert off.refit_sums is None and "gap" not in off.summary()
    on = ReconStats.load(str(tmp_path / "on.safetensors"))
    for name in ("sums", "xx_sum", "cos_sum", "x_sum"):                   # the flag adds, it changes nothing
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    # the cache: the key reaches the accumulator, and only then
    c = Cache(0, recon=dict(ks=[0, 4], refit=True))
    x, v, i = parts[0]
    c.add_recon(torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(i), sae, "m")
    assert c.recon_stats["m"].refit and c.recon_stats["m"].refit_ks == (0, 4)
    c = Cache(0, recon=dict(ks=[0, 4]))
    c.add_recon(torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(i), sae, "m")
    assert not c.recon_stats["m"].refit
    with pytest.raises(ValueError, match="keys"):
        Cache(0, recon=dict(refits=True))


def test_cli_flag():
    from msae.config import parse_cache_config, recon_kwargs

    cfg = parse_cache_config(["m", "ds", "--recon_stats"])
    assert cfg.recon_refit is False and recon_kwargs(cfg) == dict(ks=None, position_edges=(0,))
    cfg = parse_cache_config(["m", "ds", "--recon_stats", "--recon_refit", "--recon_ks", "0,8"])
    assert recon_kwargs(cfg, (0, 576)) == dict(ks=[0, 8], position_edges=(0, 576), refit=True)
    with pytest.raises(SystemExit):
        parse_cache_config(["m", "ds", "--recon_refit"])


def test_the_cache_tree_without_the_flag_is_what_it_was(tmp_path):
    """FeatureCache through save_splits and the concat, recon on: without `refit` (absent or False) the tree is the same --
    split files byte for byte, recon_stats.safetensors by length, metadata and tensor bytes (safetensors orders the metadata
    keys anew on every save); with it the split files do not move and recon_stats gains its two entries, nothing else."""
    import fakes
    from msae.features import FeatureCache
    from safetensors import safe_open

    sae = _sae(64, 128, 4)
    model = fakes.TinyLlava(vocab=40, d=64)
    locs = torch.tensor([[0, 1, 5], [1, 2, 70], [2, 0, 127]])
    acts = torch.tensor([0.5, 1.5, 2.5])
    torch.manual_seed(4)
    hidden = torch.randn(1, 2, 64)
    top = (torch.tensor([[[2.0, 1.5, 1.0, 0.5], [1.0, 0.75, 0.5, 0.25]]]), torch.tensor([[[3, 9, 27, 81], [4, 16, 64, 100]]]))
    trees = {}
    for name, recon in (("absent", dict(ks=[0, 2, 4])), ("false", dict(ks=[0, 2, 4], refit=False)),
                        ("on", dict(ks=[0, 2, 4], refit=True))):
        fc = FeatureCache(model, None, {"layers.1": sae}, batch_size=2, shard_size=0, recon=recon)
        fc.cache.add_recon(hidden, top[0], top[1], sae, "layers.1")
        fc.cache._append("layers.1", locs, acts)
        fc.cache.save()
        out = tmp_path / name
        fc.save_splits(2, str(out), rank=0)
        fc.concate_safetensors(2, str(out))
        tree = {}
        for p in sorted(out.rglob("*")):
            if p.is_file() and p.name == "recon_stats.safetensors":
                with safe_open(str(p), "pt") as f:
                    tree[str(p.relative_to(out))] = (p.stat().st_size, f.metadata(),
                                                     {k: f.get_tensor(k).numpy().tobytes() for k in sorted(f.keys())})
            elif p.is_file():
                tree[str(p.relative_to(out))] = p.read_bytes()
        trees[name] = tree
    assert trees["absent"] == trees["false"] and sorted(trees["absent"]) == sorted(trees["on"]) and len(trees["absent"]) == 3
    rs = "layers.1/recon_stats.safetensors"
    for f in trees["absent"]:
        if f != rs:
            assert trees["on"][f] == trees["absent"][f], f
    (_, meta_off, t_off), (_, meta_on, t_on) = trees["absent"][rs], trees["on"][rs]
    assert set(meta_on) - set(meta_off) == {"refit_ks"} and set(t_on) - set(t_off) == {"refit_sums"}
    assert all(meta_on[k] == v for k, v in meta_off.items()) and all(t_on[k] == v for k, v in t_off.items())
