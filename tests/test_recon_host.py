"""Reconstruction error against sparsity, everything that needs no GPU: the restatement tests/recon_ref.py against a float64
torch composition of the reference's expressions, the POWER of the fixtures the GPU test runs (every nearly-correct variant
lands outside the derived bound somewhere), ReconStats' total-variance identity, merge laws and file format, argument
errors, the cache's off switch, the command line, the plain-torch fallback of ops.recon_curve and the C ABI."""
import os

import numpy as np
import pytest
import torch

import recon_ref as ref
from msae import Sae, SaeConfig, _hip, ops
from msae.features import Cache, ReconStats
from msae.sae import ReconOutput


def _sae(case_or_d, N=None, k=4, W=None, b=None):
    d = case_or_d if isinstance(case_or_d, int) else case_or_d.d
    sae = Sae(d, SaeConfig(num_latents=N or ref.N, k=k))
    if W is not None:
        with torch.no_grad():
            sae.W_dec.copy_(torch.from_numpy(W))
            sae.b_dec.copy_(torch.from_numpy(b))
    return sae


SMALL = [i for i, c in enumerate(ref.CASES) if c.T * c.d * max(c.ks) <= 300 * 1028 * 32]


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [i for i in SMALL if ref.CASES[i].d <= 1028][:8], ids=lambda i: ref.CASES[i].id)
def test_restatement_equals_float64_composition(i):
    """sae.py: sae_out = decode(top_acts, top_indices) (+ b_dec); e = sae_out - x; e.pow(2).sum() -- in float64 torch.  The
    restatement's r is the f32 chain: |r - r64| <= gamma_{kappa+1} (sum |v w| + |b|) =: D elementwise, so each moment moves
    by at most sum |x| D and sum D (2 |r| + D); its e = fl(r - x) is one more f32 rounding, |e - e64| <= D + u (|e64| + D) =: E,
    so the error moment moves by at most sum E (2 |e64| + E)."""
    c = ref.CASES[i]
    mom, xx, _, _, _ = ref.expected(i)
    x = torch.from_numpy(c.x).double()
    W, b = torch.from_numpy(c.W_dec).double(), torch.from_numpy(c.b_dec).double()
    v, f = torch.from_numpy(c.vals.copy()).double(), torch.from_numpy(c.idx.astype(np.int64))
    for ci, kappa in enumerate(c.ks):
        rows = W[f[:, :kappa]] * v[:, :kappa, None]
        r = rows.sum(1) + b
        D = ref.gamma(kappa + 1) * (rows.abs().sum(1) + b.abs())
        e = r - x
        E = D + ref.U * (e.abs() + D)
        exp = torch.stack([e.pow(2).sum(1), (x * r).sum(1), r.pow(2).sum(1)], 1).numpy()
        tol = torch.stack([(E * (2 * e.abs() + E)).sum(1), (x.abs() * D).sum(1), (D * (2 * r.abs() + D)).sum(1)], 1).numpy()
        assert (np.abs(mom[:, ci] - exp) <= tol + 1e-300).all(), (c.id, kappa)
    assert np.allclose(xx, x.pow(2).sum(1).numpy(), rtol=1e-14, atol=0)


def test_total_variance_identity_on_offset_data():
    """sum |x - mean|^2 = sum |x - c|^2 - n |mean - c|^2 against the direct centred sum, on data whose mean is 100 times its
    spread and a centre near the mean (what b_dec is); the naive sum |x|^2 - n |mean|^2 in f32 moments would lose 4 digits."""
    rng = np.random.default_rng(3)
    B, S, d, k, N = 3, 40, 64, 4, 128
    mean = 100.0 * (1.0 + rng.random(d))
    x = (mean + rng.standard_normal((B, S, d))).astype(np.float32)
    W = (rng.standard_normal((N, d)) / 8).astype(np.float32)
    b = (mean + 0.05 * rng.standard_normal(d)).astype(np.float32)
    sae = _sae(d, N, k, W, b)
    vals = np.sort(rng.uniform(0.1, 2.0, (B, S, k)).astype(np.float32), -1)[..., ::-1].copy()
    idx = rng.integers(0, N, (B, S, k))
    st = ReconStats(d, [1, k], position_edges=(0, 10))
    st.update(torch.from_numpy(x), torch.from_numpy(vals), torch.from_numpy(idx), sae)
    flat = x.reshape(-1, d)
    direct = ref.total_variance_direct(flat)
    # the kappa = 0 moments are f32 sums of d terms: relative gamma_d on sum |x - b|^2, which is ~ the variance itself
    assert abs(float(st.total_variance()) - direct) <= 2 * ref.gamma(d) * direct
    for g, (a, e) in enumerate(((0, 10), (10, S))):
        part = x[:, a:e].reshape(-1, d)
        assert abs(float(st.total_variance(g)) - ref.total_variance_direct(part)) <= 2 * ref.gamma(d) * ref.total_variance_direct(part)
    exp = ref.stats([(x, vals, idx)], W, b, [0, 1, k], (0, 10))
    for g in range(2):
        assert st.n[g] == exp[g]["n"]
        fvu = exp[g]["sums"][1:, 0] / ref.total_variance_direct(x[:, (0, 10)[g]:(10, S)[g]].reshape(-1, d))
        assert np.allclose(st.fvu(g).numpy(), fvu, rtol=4 * ref.gamma(d), atol=0)
        assert np.allclose(st.explained_variance(g).numpy(), 1 - fvu, rtol=0, atol=4 * ref.gamma(d) * fvu.max())


# ---- power ---------------------------------------------------------------------------------------------------------------
def _variant_outside(c, exp, variant):
    mom, xx, mom_abs, _, _ = exp
    if variant == "ld_k":
        if not c.view:
            return False
        kk = c.buf_vals.shape[1]
        vals = c.buf_vals.reshape(-1)[:c.T * c.k].reshape(c.T, c.k)
        idx = c.buf_idx.reshape(-1)[:c.T * c.k].reshape(c.T, c.k)
        assert kk > c.k
        got = ref.moments(c.x, vals, idx, c.W_dec, c.b_dec, c.ks, c.n_lat)[0]
    else:
        got = ref.moments(c.x, c.vals, c.idx, c.W_dec, c.b_dec, c.ks, c.n_lat, variant=variant)[0]
    return bool(ref.outside(got, mom, mom_abs, c.d).any())


def test_fixtures_tell_the_variants_apart():
    """Every nearly-correct variant lands outside the bound for at least one token of at least one fixture the GPU test runs
    (the parametrised cases and the hostile lists); the variants that every multi-entry fixture must catch are checked on each."""
    caught = {v: [] for v in ref.VARIANTS}
    for i in SMALL:
        c, exp = ref.CASES[i], ref.expected(i)
        for v in ref.VARIANTS:
            if v != "keep_zeros" and _variant_outside(c, exp, v):
                caught[v].append(c.id)
        if min(c.ks) < c.k:                                 # a row behind a checkpoint exists: one row too many must show
            assert c.id in caught["off_by_one"], c.id
        assert c.id in caught["no_bias"], c.id
        if c.view and c.T > 1 and max(c.ks) > 0:
            assert c.id in caught["ld_k"], c.id
    h = ref.hostile_case()
    exp = ref.moments(h["x"], h["vals"], h["idx"], h["W_dec"], h["b_dec"], h["ks"], ref.N)
    got = ref.moments(h["x"], h["vals"], h["idx"], h["W_dec"], h["b_dec"], h["ks"], ref.N, variant="keep_zeros")
    out = ref.outside(got[0], exp[0], exp[2], h["d"])
    assert out[0] and out[1] and not out[2]                 # the tokens with a zero value in front of the infinite row
    caught["keep_zeros"].append("hostile")
    assert all(caught.values()), {v: len(c) for v, c in caught.items()}
    assert any("close" in cid for cid in caught["f64_recon"])


# ---- ops.recon_curve off the GPU -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [i for i in SMALL if ref.CASES[i].T <= 5 or ref.CASES[i].d <= 100][:10], ids=lambda i: ref.CASES[i].id)
def test_torch_fallback_stays_inside_the_bound(i):
    c = ref.CASES[i]
    mom, xx, mom_abs, xx_abs, _ = ref.expected(i)
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[c.dtype]
    x = torch.from_numpy(c.x).to(tdt)
    got_m, got_x = ops.recon_curve(x, torch.from_numpy(c.buf_vals)[:, :c.k], torch.from_numpy(c.buf_idx)[:, :c.k],
                                   torch.from_numpy(c.W_dec), torch.from_numpy(c.b_dec), c.ks)
    assert got_m.shape == (c.T, len(c.ks), 3) and got_x.shape == (c.T,) and got_m.dtype == torch.float32
    # the fallback's r comes from a torch sum, not the chain: it moves by D as in the float64 composition test
    W, b = c.W_dec.astype(np.float64), c.b_dec.astype(np.float64)
    for ci, kappa in enumerate(c.ks):
        rows = np.abs(c.vals[:, :kappa, None].astype(np.float64) * W[c.idx[:, :kappa]])
        D = 2 * ref.gamma(kappa + 1) * (rows.sum(1) + np.abs(b))
        r = np.abs(ref.recon(*ref.sanitize(c.vals, c.idx, c.n_lat)[:2], c.W_dec, c.b_dec, kappa).astype(np.float64))
        e = r + np.abs(c.x)                                  # >= |e|
        E = D + ref.U * (e + D)
        slack = np.stack([(E * (2 * e + E)).sum(1), (np.abs(c.x) * D).sum(1), (D * (2 * r + D)).sum(1)], 1)
        assert (np.abs(got_m[:, ci].double().numpy() - mom[:, ci]) <= ref.bound(mom_abs[:, ci], c.d) + slack).all(), kappa
    assert (np.abs(got_x.double().numpy() - xx) <= ref.bound(xx_abs, c.d)).all()


def test_fallback_skips_hostile_entries_and_sae_recon_error_on_the_cpu():
    h = ref.hostile_case()
    exp = ref.moments(h["x"], h["vals"], h["idx"], h["W_dec"], h["b_dec"], h["ks"], ref.N)
    mom, xx = ops.recon_curve(*(torch.from_numpy(h[n]) for n in ("x", "vals", "idx", "W_dec", "b_dec")), h["ks"])
    fin = np.isfinite(exp[0]).all((1, 2))
    assert list(np.nonzero(~fin)[0]) == [5] and not torch.isfinite(mom[5]).all() and torch.isfinite(mom[fin]).all()
    assert np.allclose(mom[fin].double().numpy(), exp[0][fin], rtol=1e-5)
    sae = _sae(h["d"], ref.N, h["k"], np.nan_to_num(h["W_dec"], nan=0.0, posinf=0.0), h["b_dec"])
    top = (torch.from_numpy(h["vals"]), torch.from_numpy(h["idx"]).clamp(0, ref.N - 1))
    out = sae.recon_error(torch.from_numpy(h["x"])[:5], ks=[0, 8], top=(top[0][:5], top[1][:5]))
    assert isinstance(out, ReconOutput) and out.ks == (0, 8) and out.err2.shape == (5, 2) and out.xnorm2.shape == (5,)
    x = h["x"][:5].astype(np.float64)
    assert np.isclose(float(out.total_variance), ref.total_variance_direct(x), rtol=1e-12)
    assert out.fvu.dtype == torch.float64 and out.mse.dtype == torch.float64 and out.cosine.dtype == torch.float64
    assert np.allclose(out.fvu.numpy(), out.err2.double().sum(0).numpy() / ref.total_variance_direct(x), rtol=1e-12)
    assert np.allclose(out.mse.numpy(), out.err2.double().numpy() / h["d"], rtol=1e-15)
    assert sae.default_recon_ks() == (1, 2, 4, 8)
    assert Sae(8, SaeConfig(num_latents=16, k=6)).default_recon_ks() == (1, 2, 4, 6)


def test_argument_errors_raise_before_any_device_work():
    d, N, k, T = 8, 16, 4, 3
    x, v, i = torch.zeros(T, d), torch.ones(T, k), torch.zeros(T, k, dtype=torch.int64)
    W, b = torch.zeros(N, d), torch.zeros(d)
    bad = [
        (dict(ks=[]), "checkpoints"), (dict(ks=list(range(17))), "checkpoints"), (dict(ks=[2, 1]), "ascending"),
        (dict(ks=[1, 1]), "ascending"), (dict(ks=[-1]), "ascending"), (dict(ks=[k + 1]), "ascending"),
        (dict(ks=[0.5]), "integers"), (dict(x=torch.zeros(T, d + 1)), "share d"), (dict(x=torch.zeros(T, d, dtype=torch.float64)), "float32"),
        (dict(v=torch.ones(T, k + 1)), "share one shape"), (dict(v=torch.ones(T + 1, k), i=torch.zeros(T + 1, k, dtype=torch.int64)), "one row"),
        (dict(i=torch.zeros(T, k, dtype=torch.int16)), "int32 or int64"), (dict(v=torch.ones(T, k, dtype=torch.float64)), "float32"),
        (dict(b=torch.zeros(d + 1)), "b_dec"), (dict(b=None), "b_dec"),
        (dict(v=torch.ones(T, 4097), i=torch.zeros(T, 4097, dtype=torch.int64)), "k must be"),
    ]
    for kw, msg in bad:
        a = dict(x=x, v=v, i=i, W=W, b=b, ks=[0, k])
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.recon_curve(a["x"], a["v"], a["i"], a["W"], a["b"], a["ks"])
    sae = _sae(d, N, k)
    for kw, msg in ((dict(ks=[k + 1]), "ascending"), (dict(chunk=0), "chunk"), (dict(top=(v,)), "pair")):
        with pytest.raises(ValueError, match=msg):
            sae.recon_error(x, **{"top": (v, i), **kw})
    with pytest.raises(ValueError, match="must be"):
        sae.recon_error(torch.zeros(T, d + 1), top=(v, i))
    with pytest.raises(RuntimeError, match="inference"):
        sae.recon_error(x.clone().requires_grad_(True), top=(v, i))
    for args, msg in ((([1, 2], (1,)), "start at 0"), (([1, 2], (0, 4, 4)), "ascend"), (([1, 2], tuple(range(9))), "groups"),
                      ((list(range(1, 17)), (0,)), "besides 0"), (([2, 1], (0,)), "ascending")):
        with pytest.raises(ValueError, match=msg):
            ReconStats(d, *args)
    st = ReconStats(d, [0, 8])
    with pytest.raises(ValueError, match="lists hold"):
        st.update(torch.zeros(1, T, d), v[None], i[None], sae)
    with pytest.raises(ValueError, match="hidden must be"):
        ReconStats(d, [0, 2]).update(x, v, i, sae)
    with pytest.raises(ValueError, match="keys"):
        Cache(0, recon=dict(pool="image"))


def test_sharded_engines_refuse():
    from msae.parallel import ShardedSae

    with pytest.raises(NotImplementedError, match="msae.Sae"):
        ShardedSae.recon_error(object(), None)


# ---- ReconStats: merge laws, file ----------------------------------------------------------------------------------------
def _three_parts(seed=5):
    rng = np.random.default_rng(seed)
    B, S, d, k, N = 2, 12, 16, 8, 64
    W = (rng.standard_normal((N, d)) / 4).astype(np.float32)
    b = (0.3 * rng.standard_normal(d)).astype(np.float32)
    sae = _sae(d, N, k, W, b)
    parts = []
    for _ in range(3):
        x = (rng.standard_normal((B, S, d)) + b).astype(np.float32)
        vals = np.sort(rng.uniform(0.1, 2.0, (B, S, k)).astype(np.float32), -1)[..., ::-1].copy()
        parts.append((x, vals, rng.integers(0, N, (B, S, k))))
    return sae, W, b, parts


def _stat(sae, parts, ks=(1, 4, 8), edges=(0, 5)):
    st = ReconStats(sae.d_in, ks, position_edges=edges)
    for x, v, i in parts:
        st.update(torch.from_numpy(x), torch.from_numpy(v), torch.from_numpy(i), sae)
    return st


def _close(a: ReconStats, b: ReconStats, n_terms: int):
    assert a.n == b.n
    for name in ("sums", "xx_sum", "cos_sum", "x_sum"):
        p, q = getattr(a, name).numpy(), getattr(b, name).numpy()
        assert (np.abs(p - q) <= 2 * n_terms * 2.0 ** -53 * np.maximum(np.abs(p), np.abs(q)) * 4).all(), name


def test_merge_is_associative_to_the_float64_bound_and_refuses_mismatches():
    """The terms of sums / xx_sum are non-negative or (x . r) summed with their magnitudes bounded by 4 x the result here, so
    2 n 2^-53 sum |term| <= 8 n 2^-53 |sum|."""
    sae, W, b, parts = _three_parts()
    n_terms = 3 * 2 * 12
    whole = _stat(sae, parts)
    left = _stat(sae, parts[:1]).merge(_stat(sae, parts[1:2])).merge(_stat(sae, parts[2:]))
    right = _stat(sae, parts[:1]).merge(_stat(sae, parts[1:2]).merge(_stat(sae, parts[2:])))
    _close(left, right, n_terms)
    _close(left, whole, n_terms)
    exp = ref.stats(parts, W, b, [0, 1, 4, 8], (0, 5))
    for g in range(2):
        assert whole.n[g] == exp[g]["n"]
        assert (np.abs(whole.x_sum[g].numpy() - exp[g]["x_sum"]) <= 1e-12 * np.abs(exp[g]["x_sum"]) + 1e-12).all()
        assert np.allclose(whole.sums[g].numpy(), exp[g]["sums"], rtol=16 * ref.gamma(16), atol=0)
    with pytest.raises(ValueError, match="different kinds"):
        whole.merge(_stat(sae, parts, ks=(1, 8)))
    with pytest.raises(ValueError, match="different kinds"):
        whole.merge(_stat(sae, parts, edges=(0, 6)))
    other = _sae(16, 64, 8, W, np.nextafter(b, np.float32(9)).astype(np.float32))
    with pytest.raises(ValueError, match="centres"):
        whole.merge(_stat(other, parts))


def test_file_round_trip_on_the_cpu(tmp_path):
    sae, W, b, parts = _three_parts(6)
    st = _stat(sae, parts)
    path = str(tmp_path / "recon_stats.safetensors")
    st.save(path)
    back = ReconStats.load(path)
    assert back.ks == st.ks and back.position_edges == st.position_edges and back.n == st.n and back.d == st.d
    for name in ("sums", "xx_sum", "cos_sum", "x_sum", "b_dec"):
        assert torch.equal(getattr(back, name), getattr(st, name)), name
    for fn in ("fvu", "explained_variance", "mse", "nmse", "cosine"):
        for g in (None, 0, 1):
            a, c = getattr(st, fn)(g), getattr(back, fn)(g)
            assert a.dtype == torch.float64 and a.shape == (3,) and torch.equal(a, c), (fn, g)
    assert (st.fvu() > 0).all() and (st.cosine() <= 1 + 1e-6).all() and (st.nmse() > 0).all()
    with pytest.raises(ValueError, match="not a reconstruction"):
        from safetensors.torch import save_file

        save_file({"a": torch.zeros(1)}, str(tmp_path / "x.safetensors"), metadata={"format": "other"})
        ReconStats.load(str(tmp_path / "x.safetensors"))
    from msae.features.cache import merge_rank_recon

    os.makedirs(tmp_path / "m")
    _stat(sae, parts[:2]).save(str(tmp_path / "m" / "Rank0_recon_stats.safetensors"))
    _stat(sae, parts[2:]).save(str(tmp_path / "m" / "Rank1_recon_stats.safetensors"))
    assert merge_rank_recon(str(tmp_path / "m")) == str(tmp_path / "m" / "recon_stats.safetensors")
    assert os.listdir(tmp_path / "m") == ["recon_stats.safetensors"]
    _close(ReconStats.load(str(tmp_path / "m" / "recon_stats.safetensors")), st, 72)
    assert merge_rank_recon(str(tmp_path)) is None


# ---- cache off, command line, ABI ----------------------------------------------------------------------------------------
def test_cache_off_allocates_nothing_and_writes_the_same_files(tmp_path):
    import fakes
    from msae.features import FeatureCache

    sae = _sae(64, 128, 4)
    model = fakes.TinyLlava(vocab=40, d=64)
    locs = torch.tensor([[0, 1, 5], [1, 2, 70], [2, 0, 127]])
    acts = torch.tensor([0.5, 1.5, 2.5])
    files = {}
    for name, kw in (("absent", {}), ("none", dict(recon=None)), ("unused", dict(recon=dict(ks=[0, 2])))):
        fc = FeatureCache(model, None, {"layers.1": sae}, batch_size=2, shard_size=0, **kw)
        assert fc.cache.recon_stats == {} and (fc.cache.recon is None) == (name != "unused")
        fc.cache.add_recon(torch.zeros(1, 2, 64), torch.ones(1, 2, 4), torch.zeros(1, 2, 4, dtype=torch.int64), sae, "layers.1") \
            if name != "unused" else None
        assert fc.cache.recon_stats == {}
        fc.cache._append("layers.1", locs, acts)
        fc.cache.save()
        out = tmp_path / name
        os.makedirs(out)
        fc.save(str(out))
        fc.save_splits(2, str(out), rank=0)
        fc.concate_safetensors(2, str(out))
        files[name] = {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}
    assert files["absent"] == files["none"] == files["unused"] and len(files["absent"]) == 3
    # on: the hidden state the loop holds goes in, and the rank file appears
    fc = FeatureCache(model, None, {"layers.1": sae}, batch_size=2, shard_size=0, recon=dict(position_edges=(0, 1)))
    fc.cache.add_recon(torch.randn(1, 2, 64), torch.ones(1, 2, 4), torch.zeros(1, 2, 4, dtype=torch.int64), sae, "layers.1")
    st = fc.cache.recon_stats["layers.1"]
    assert st.ks == (1, 2, 4) and st.n == [1, 1] and st.position_edges == (0, 1)
    fc.cache._append("layers.1", locs, acts)
    fc.cache.save()
    fc.save_splits(2, str(tmp_path / "on"), rank=3)
    assert "Rank3_recon_stats.safetensors" in os.listdir(tmp_path / "on" / "layers.1")
    fc.concate_safetensors(2, str(tmp_path / "on"))
    assert sorted(os.listdir(tmp_path / "on" / "layers.1")) == ["0_63.safetensors", "64_127.safetensors", "recon_stats.safetensors"]
    for f in ("0_63.safetensors", "64_127.safetensors"):
        assert (tmp_path / "on" / "layers.1" / f).read_bytes() == files["absent"][f"layers.1/{f}"]


def test_cli_flags_parse():
    from msae.config import parse_cache_config, recon_kwargs

    cfg = parse_cache_config(["m", "ds"])
    assert cfg.recon_stats is False and cfg.recon_ks is None and recon_kwargs(cfg) is None
    cfg = parse_cache_config(["m", "ds", "--recon_stats", "--recon_ks", "0,1,2,4,8,16,32"])
    assert recon_kwargs(cfg, (0, 576)) == dict(ks=[0, 1, 2, 4, 8, 16, 32], position_edges=(0, 576))
    assert recon_kwargs(parse_cache_config(["m", "ds", "--recon_stats"])) == dict(ks=None, position_edges=(0,))
    for bad in ("1,1", "a,b", "4,2", "-1,2", ",".join(str(i) for i in range(17))):
        with pytest.raises(SystemExit):
            parse_cache_config(["m", "ds", "--recon_stats", "--recon_ks", bad])
    import inspect

    from msae.launch.cache import cache, cache_image
    assert "recon_kwargs(cfg)" in inspect.getsource(cache.main) and "recon_kwargs(cfg, (0, pool_len))" in inspect.getsource(cache_image.main)


def test_abi_version_stays_and_the_symbols_are_there():
    assert _hip.ABI_VERSION == 4
    lib = _hip.load()
    assert lib.msae_abi_version() == 4
    for name in ("msae_recon_curve_f32", "msae_recon_curve_i64_f32"):
        assert getattr(lib, name) is not None
    # host-side argument checks of the C entry point: no device work happens before them
    import ctypes

    ks = (ctypes.c_int32 * 2)(0, 4)
    one = ctypes.c_void_p(16)
    args = lambda **kw: [kw.get("x", one), kw.get("dt", 0), one, one, kw.get("ld", 4), one, kw.get("b", one), kw.get("T", 1),
                         kw.get("k", 4), 8, 8, kw.get("ks", ks), kw.get("C", 2), one, one, None, None]
    f = lib.msae_recon_curve_f32
    assert f(*args(T=0)) == 0
    einval = f(*args(k=0))
    assert einval != 0
    for kw in (dict(k=4097, ld=4097), dict(ld=3), dict(C=0), dict(C=17), dict(x=None), dict(b=None), dict(dt=9), dict(T=-1),
               dict(ks=(ctypes.c_int32 * 2)(4, 4)), dict(ks=(ctypes.c_int32 * 2)(0, 5)), dict(ks=(ctypes.c_int32 * 2)(-1, 2))):
        assert f(*args(**kw)) == einval, kw
