"""CPU: the per-feature uniform example sample -- its hash and table rules (feature_sample_ref.py), the reference's own
sampler picks (g17), the file format with the sample on and off, the reader side (sample_example_records), and the
CacheConfig flags."""
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from safetensors import safe_open
from safetensors.torch import save_file

import feature_sample_ref as sref
import feature_stats_ref as ref
from conftest import GOLDEN, REPO

RECIPE = GOLDEN / "make_golden_samplers.py"


def _g14():
    return np.load(GOLDEN / "g14_feature_stats.npz")


def _g17():
    return np.load(GOLDEN / "g17_samplers.npz")


def test_pinned_priorities():
    """The five values include/msae.h pins, from the numpy restatement (and a pure-Python one, mod 2^64)."""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    assert len(sref.PINNED) == 5
    for (seed, f, i), want in sref.PINNED:
        assert int(sref.prio(seed, f, i)) == want, (seed, f, i)
        assert mix(mix((seed + 0x9E3779B97F4A7C15 * (f + 1)) & M) ^ i) == want
    assert sref.PINNED[0] == ((22, 0, 0), 0xbe5264ad2aa020f4)
    assert sref.PINNED[4] == ((2 ** 64 - 1, 262143, 2 ** 40 + 3), 0xaf8ee0a530541d25)
    header = (REPO / "include" / "msae.h").read_text()
    for _, want in sref.PINNED:
        assert f"{want:#018x}" in header


def _window_candidates():
    g = _g14()
    S, N, W = int(g["window_S"]), int(g["window_N"]), int(g["window_W"])
    loc, act = g["window_locations"], g["window_activations"]
    return ref.candidates(loc[:, 0], loc[:, 1], loc[:, 2], act, S, "window", 0, W=W), N


def test_prefix_property_and_table_order():
    (cf, cv, ci), N = _window_candidates()
    seg, v64, i64 = sref.sample_tables(cf, cv, ci, N, 64, 22)
    seg16, v16, i16 = sref.sample_tables(cf, cv, ci, N, 16, 22)
    assert np.array_equal(i16, i64[:, :16]) and np.array_equal(v16.view(np.uint32), v64[:, :16].view(np.uint32))
    assert np.array_equal(seg, seg16) and np.array_equal(seg, np.bincount(cf, minlength=N))
    assert seg.max() > 64 and seg.min() > 16                # tables with evictions
    for f in range(N):
        n = min(64, int(seg[f]))
        assert (i64[f, :n] >= 0).all() and (i64[f, n:] == -1).all() and (v64[f, n:] == 0).all()
        p = sref.prio(22, f, i64[f, :n])
        assert (p[1:] > p[:-1]).all()                        # priority ascending, no ties
        pool = ci[cf == f]
        assert np.array_equal(np.sort(pool[np.argsort(sref.prio(22, f, pool))[:n]]), np.sort(i64[f, :n]))
        vals = dict(zip(pool.tolist(), cv[cf == f].tolist()))
        assert [vals[i] for i in i64[f, :n].tolist()] == v64[f, :n].tolist()
    other = sref.sample_tables(cf, cv, ci, N, 64, 23)[2]
    assert not np.array_equal(other, i64)                    # the seed matters


def test_merge_is_associative_and_commutative_bitwise():
    (cf, cv, ci), N = _window_candidates()
    n, seed = 16, 22
    part = (ci // 5) % 3                                     # rows dealt to three "ranks"
    a, b, c = (sref.sample_tables(cf[part == r], cv[part == r], ci[part == r], N, n, seed) for r in range(3))
    whole = sref.sample_tables(cf, cv, ci, N, n, seed)
    ab_c = sref.merge_samples(sref.merge_samples(a, b, n, seed), c, n, seed)
    a_bc = sref.merge_samples(a, sref.merge_samples(b, c, n, seed), n, seed)
    cb_a = sref.merge_samples(sref.merge_samples(c, b, n, seed), a, n, seed)
    for got in (ab_c, a_bc, cb_a):
        for x, y in zip(got, whole):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_uniformity_on_a_fixed_input():
    """Ids 5i + 7 (i < 1000), n = 64, f = 5, seeds 1..2000: inclusion counts have mean exactly 128, each within 4.5 binomial
    standard deviations (sigma = 10.95), Pearson's statistic over the 1000 counts in [850, 1150] (999 degrees of freedom).
    Measured: largest deviation 3.29 sigma, statistic 943.5."""
    ids = 5 * np.arange(1000, dtype=np.int64) + 7
    seeds = np.arange(1, 2001, dtype=np.uint64)[:, None]
    p = sref.prio(seeds, 5, ids[None, :])
    chosen = np.argsort(p, axis=1)[:, :64]
    counts = np.bincount(chosen.reshape(-1), minlength=1000)
    assert counts.sum() == 2000 * 64 and counts.mean() == 128
    sigma = np.sqrt(2000 * 0.064 * (1 - 0.064))
    dev = np.abs(counts - 128).max() / sigma
    chi2 = ((counts - 128.0) ** 2).sum() / sigma ** 2        # each count against its binomial variance n p (1 - p)
    print(f"largest deviation {dev:.2f} sigma, Pearson statistic {chi2:.1f}")
    assert abs(sigma - 10.95) < 0.01
    assert dev <= 4.5
    assert 850 <= chi2 <= 1150
    # the restated table picks the same 64 for one of the seeds
    _, _, si = sref.sample_tables(np.full(1000, 5), np.ones(1000, np.float32), ids, 6, 64, 1234)
    assert np.array_equal(si[5], ids[np.argsort(sref.prio(1234, 5, ids))[:64]])


def _stats_from(loc, act, S, N, mode, n_sample, seed=22, n=64, **kw):
    from msae.features import FeatureStats

    st = FeatureStats(N, n_top=n, pool=mode, n_sample=n_sample, sample_seed=seed, **kw)
    cf, cv, ci = ref.candidates(loc[:, 0], loc[:, 1], loc[:, 2], act, S, mode, 0, P=kw.get("pool_len", 576),
                                W=kw.get("window", 64))
    tv, ti = ref.top_tables(cf, cv, ci, N, n)
    c, mx, sm = ref.basic_stats(loc[:, 2], act, N)
    st.count, st.act_max, st.act_sum = torch.from_numpy(c), torch.from_numpy(mx), torch.from_numpy(sm)
    st.top_val, st.top_id = torch.from_numpy(tv), torch.from_numpy(ti)
    if n_sample:
        seg, sv, si = sref.sample_tables(cf, cv, ci, N, n_sample, seed)
        st.seg_count, st.smp_val, st.smp_id = torch.from_numpy(seg), torch.from_numpy(sv), torch.from_numpy(si)
    if mode == "window":
        st.windows_per_row = S // kw["window"]
    return st


def _window_stats(n_sample=256, seed=22):
    g = _g14()
    S, N, W = int(g["window_S"]), int(g["window_N"]), int(g["window_W"])
    return g, _stats_from(g["window_locations"], g["window_activations"], S, N, "window", n_sample, seed=seed, window=W)


def test_reference_sampler_picks_g17():
    """With n_sample = 256 every feature's sample is its whole population (fewer than 256 nonzero windows), so
    stats_examples must return exactly the ids the reference's train() returned."""
    from msae.features.samplers import stats_examples

    g17 = _g17()
    _, st = _window_stats(256)
    n_train, nq = int(g17["n_train"]), int(g17["n_quantiles"])
    assert (st.seg_count <= 256).all() and (st.sample_fraction() == 1).all()
    for i, f in enumerate(g17["features"].tolist()):
        for train_type in ("top", "random", "quantile"):
            want = g17[train_type][i]
            ids, vals = stats_examples(st, f, train_type, n_train, n_quantiles=nq)
            assert ids.tolist() == want[want >= 0].tolist(), (f, train_type)
            pool = dict(zip(st.smp_id[f].tolist(), st.smp_val[f].tolist()))
            assert vals.tolist() == [pool[j] for j in ids.tolist()]
    with pytest.raises(ValueError):
        stats_examples(st, 0, "best", 3)


def test_train_and_split_quantiles_semantics():
    """Seeding and draws are the `random` module's: random.seed, random.sample, len // n_quantiles per stratum."""
    import random

    from msae.features import samplers

    ex = list(range(100, 147))                               # 47 examples: strata of 4, the last 7 never drawn
    assert samplers.train(ex, 5, "top") == ex[:5]
    random.seed(22)
    drawn = random.sample(ex, 5)
    assert samplers.train(ex, 5, "random") == drawn
    random.seed(22)
    want = []
    for q in range(10):
        want += random.sample(ex[4 * q:4 * q + 4], 3)
    assert samplers.train(ex, 3, "quantile") == want == samplers.split_quantiles(ex, 10, 3)
    assert len(samplers.split_quantiles(ex, 10, 9)) == 40     # a stratum smaller than n_samples is taken whole
    assert samplers.split_quantiles(ex[:7], 10, 3) == []
    with pytest.raises(ValueError):
        samplers.train(ex, 3, "bottom")
    with pytest.raises(ValueError):
        samplers.train(ex[:2], 3, "random")
    rec = types.SimpleNamespace(examples=ex)
    samplers.sample(rec, types.SimpleNamespace(n_examples_train=3, train_type="quantile", n_quantiles=10))
    assert rec.train == want
    assert not hasattr(samplers, "split_activation_quantiles")


def test_recipe_regenerates_g17_byte_for_byte(tmp_path):
    if subprocess.run([sys.executable, str(RECIPE), "--check-reference"], capture_output=True).returncode != 0:
        pytest.skip("the reference is not on this machine")
    subprocess.run([sys.executable, str(RECIPE), "--out", str(tmp_path)], check=True, capture_output=True)
    a, b = np.load(tmp_path / "g17_samplers.npz"), _g17()
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert all(a[k].dtype == np.int64 for k in a.files)      # ids (and three integers) only


def test_save_load_round_trip_with_the_sample_on(tmp_path):
    from msae.features import FeatureStats

    _, st = _window_stats(16, seed=2 ** 64 - 3)
    st.tokens_seen = 99
    st.save(str(tmp_path / "s.safetensors"))
    back = FeatureStats.load(str(tmp_path / "s.safetensors"))
    assert (back.n_sample, back.sample_seed) == (16, 2 ** 64 - 3)
    assert back.metadata() == st.metadata()
    assert back.metadata()["n_sample"] == "16" and back.metadata()["sample_seed"] == str(2 ** 64 - 3)
    for k in ("count", "act_max", "act_sum", "top_val", "top_id", "seg_count", "smp_val", "smp_id"):
        assert torch.equal(getattr(back, k), getattr(st, k)), k
    assert back.seg_count.dtype == torch.int64 and back.smp_id.dtype == torch.int64 and back.smp_val.dtype == torch.float32
    ids, vals = back.sample_examples(3)
    assert len(ids) == 16 and torch.equal(ids, st.smp_id[3]) and torch.equal(vals, st.smp_val[3])
    frac = back.sample_fraction()
    assert frac.dtype == torch.float64 and torch.equal(frac, (16 / st.seg_count.double()).clamp(max=1.0))
    with pytest.raises(ValueError):
        FeatureStats(10, n_sample=257)
    with pytest.raises(ValueError):
        FeatureStats(10, n_sample=-1)


def test_sample_off_writes_exactly_the_old_file(tmp_path):
    """With the sample off, the tensor names and metadata keys are the sets they were before the sample existed; such a
    file (any old-format file) loads with n_sample = 0."""
    from msae.features import FeatureStats

    st = FeatureStats(300, n_top=60, pool="window", window=32)
    assert st.n_sample == 0 and not hasattr(st, "smp_id") and not hasattr(st, "seg_count")
    st.save(str(tmp_path / "off.safetensors"))
    with safe_open(str(tmp_path / "off.safetensors"), framework="pt") as fh:
        assert set(fh.keys()) == {"count", "act_max", "act_sum", "top_val", "top_id"}
        assert set(fh.metadata()) == {"format", "pool", "pool_len", "window", "n_top", "thresh", "num_latents",
                                      "tokens_seen", "windows_per_row"}
    assert set(st.metadata()) == {"format", "pool", "pool_len", "window", "n_top", "thresh", "num_latents",
                                  "tokens_seen", "windows_per_row"}
    # an old-format file written without this class
    old = {"count": torch.zeros(8, dtype=torch.int64), "act_max": torch.zeros(8), "act_sum": torch.zeros(8, dtype=torch.float64),
           "top_val": torch.zeros(8, 55), "top_id": torch.full((8, 55), -1, dtype=torch.int64)}
    meta = {"format": "msae.feature_stats.v1", "pool": "image", "pool_len": "576", "window": "64", "n_top": "55",
            "thresh": "1e-05", "num_latents": "8", "tokens_seen": "0", "windows_per_row": "null"}
    save_file(old, str(tmp_path / "old.safetensors"), metadata=meta)
    back = FeatureStats.load(str(tmp_path / "old.safetensors"))
    assert back.n_sample == 0 and back.metadata() == meta
    with pytest.raises(ValueError):
        back.sample_examples(0)
    with pytest.raises(ValueError):
        back.sample_fraction()


def test_same_kind_compares_the_sample():
    from msae.features import FeatureStats

    a = FeatureStats(16, n_sample=8, sample_seed=22)
    for other in (FeatureStats(16, n_sample=8, sample_seed=23), FeatureStats(16, n_sample=4, sample_seed=22),
                  FeatureStats(16)):
        with pytest.raises(ValueError):
            a._same_kind(other)
        with pytest.raises(ValueError):
            a.merge(other)
    a._same_kind(FeatureStats(16, n_sample=8, sample_seed=22))


def _split_dir(tmp_path, loc, act, width, n_splits, module="m"):
    from msae.features.cache import generate_split_indices

    d = tmp_path / module
    d.mkdir(parents=True, exist_ok=True)
    for s, e in generate_split_indices(width, n_splits):
        m = (loc[:, 2] >= s) & (loc[:, 2] < e)
        save_file({"locations": torch.from_numpy(loc[m]), "activations": torch.from_numpy(act[m])},
                  str(d / f"{s}_{e}.safetensors"))
    return d


def test_sample_example_records_window_mode(tmp_path):
    from msae.features import sample_example_records, top_example_records
    from msae.features.samplers import stats_examples

    g, st = _window_stats(256)
    g17 = _g17()
    S, N, W = int(g["window_S"]), int(g["window_N"]), int(g["window_W"])
    loc, act = g["window_locations"], g["window_activations"]
    _split_dir(tmp_path, loc, act, N, 4)
    rows = int(loc[:, 0].max()) + 1
    tokens = torch.arange(rows * S).reshape(rows, S)
    st.save(str(tmp_path / "stats.safetensors"))
    for i, f in enumerate(g17["features"].tolist()[:12]):
        if f in (15, 31, 47, 63):
            continue                                    # the split files drop each split's last feature (reference quirk)
        for train_type in ("random", "quantile"):
            ex = sample_example_records(str(tmp_path), str(tmp_path / "stats.safetensors"), "m", f, train_type, 3,
                                        n_splits=4, tokens=tokens)
            want = g17[train_type][i]
            assert ex.ids.tolist() == want[want >= 0].tolist()
            assert torch.equal(ex.activations.max(dim=1).values, ex.values)
            r, w = ex.ids // (S // W), ex.ids % (S // W)
            assert torch.equal(ex.tokens[:, 0], r * S + w * W)
            for j, (rr, ww) in enumerate(zip(r.tolist(), w.tolist())):
                sel = (loc[:, 0] == rr) & (loc[:, 2] == f) & (loc[:, 1] // W == ww)
                dense = np.zeros(W, np.float32)
                dense[loc[sel, 1] - ww * W] = act[sel]
                assert np.array_equal(ex.activations[j].numpy(), dense)
        top = sample_example_records(str(tmp_path), st, "m", f, "top", 5, n_splits=4, tokens=tokens)
        old = top_example_records(str(tmp_path), st, "m", f, 5, n_splits=4, tokens=tokens)
        for x, y in zip(top, old):
            assert torch.equal(x, y)
        assert torch.equal(top.ids, stats_examples(st, f, "top", 5)[0])


def test_sample_example_records_image_mode(tmp_path):
    from msae.features import sample_example_records
    from msae.features.samplers import stats_examples

    g = _g14()
    S, N, P = int(g["image_S"]), int(g["image_N"]), int(g["image_P"])
    loc, act = g["image_locations"], g["image_activations"]
    _split_dir(tmp_path, loc, act, N, 2)
    st = _stats_from(loc, act, S, N, "image", 64, pool_len=P)
    assert (st.seg_count > 64).any() and (st.sample_fraction() < 1).any()
    image_ids = g["image_ids"].tolist()
    deduped = 0
    for f in g["image_features"].tolist()[:10]:
        ids, vals = stats_examples(st, f, "quantile", 3)
        assert len(ids) == 30 and set(ids.tolist()) <= set(st.smp_id[f].tolist())
        ex = sample_example_records(str(tmp_path), st, "m", f, "quantile", 3, n_splits=2, seq_len=S)
        assert torch.equal(ex.ids, ids) and torch.equal(ex.values, vals)
        assert ex.tokens.shape == (30, S) and not ex.tokens.any()
        for j, r in enumerate(ex.ids.tolist()):
            sel = (loc[:, 0] == r) & (loc[:, 2] == f)
            dense = np.zeros(S, np.float32)
            dense[loc[sel, 1]] = act[sel]
            assert np.array_equal(ex.activations[j].numpy(), dense)
            assert np.float32(dense[:P].sum(dtype=np.float32) / np.float32(P)) == pytest.approx(ex.values[j].item(), rel=1e-6)
        # with image ids: the first row of every image id, in list order, no padding
        dd = sample_example_records(str(tmp_path), st, "m", f, "quantile", 3, n_splits=2, seq_len=S, image_ids=image_ids)
        seen, want = set(), []
        for r in ids.tolist():
            if image_ids[r] not in seen:
                seen.add(image_ids[r])
                want.append(r)
        assert dd.ids.tolist() == want and len(dd.activations) == len(want)
        deduped += len(want) < 30
    assert deduped > 0


def test_cache_config_sample_flags():
    from msae.config import CacheConfig, parse_cache_config

    assert (CacheConfig().stats_sample, CacheConfig().stats_seed) == (0, 22)
    cfg = parse_cache_config(["m", "d"])
    assert (cfg.stats_sample, cfg.stats_seed, cfg.feature_stats) == (0, 22, False)
    on = parse_cache_config(["m", "d", "--feature_stats", "--stats_sample", "64", "--stats_seed", "7"])
    assert (on.feature_stats, on.stats_sample, on.stats_seed) == (True, 64, 7)
    rest = {k: v for k, v in on.to_dict().items() if k not in ("feature_stats", "stats_sample", "stats_seed")}
    assert rest == {k: v for k, v in cfg.to_dict().items() if k in rest}


def test_launchers_forward_the_sample_options():
    for name in ("cache.py", "cache_image.py"):
        text = (REPO / "multimodal-sae_amd" / "msae" / "launch" / "cache" / name).read_text()
        assert "n_sample=cfg.stats_sample" in text and "sample_seed=cfg.stats_seed" in text, name


def test_cache_passes_the_sample_options_through():
    from msae.features import Cache

    cache = Cache(0, None, batch_size=2, stats=dict(pool="window", window=64, n_sample=64, sample_seed=5))
    assert cache.stats == dict(pool="window", window=64, n_sample=64, sample_seed=5)


def test_c_abi_declares_the_sample_entry_points():
    import ctypes

    from msae import _hip

    assert len(_hip.PROTOTYPES["msae_feature_stats_update_sampled"][1]) == len(_hip.PROTOTYPES["msae_feature_stats_update"][1]) + 1
    assert len(_hip.PROTOTYPES["msae_feature_sample_merge"][1]) == 10
    assert ctypes.sizeof(_hip.MsaeFeatureSample) == 40
    lib = _hip.load()
    # argument errors come back before anything touches a device: n_sample outside 1..256, null tables, a short struct
    tables = (ctypes.c_uint64 * 4)()
    for n_sample, size, ptr in ((0, 40, tables), (257, 40, tables), (8, 40, None), (8, 16, tables)):
        p = ctypes.cast(ptr, ctypes.c_void_p) if ptr is not None else None
        sm = _hip.MsaeFeatureSample(size, n_sample, 22, p, p, p)
        rc = lib.msae_feature_stats_update_sampled(None, None, 1, 4, 2, 1e-5, 4, 1, 1, 2, 0, 64, None, None, None, None, None,
                                                   ctypes.byref(sm), None, 0, None)
        assert rc == -1, (n_sample, size, rc)
    assert lib.msae_feature_sample_merge(4, 0, 22, None, None, None, None, None, None, None) == -1
    assert lib.msae_feature_sample_merge(4, 8, 22, None, None, None, None, None, None, None) == -1


def test_alias_resolves_the_samplers_module():
    import os

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(REPO / "multimodal-sae_amd"),
                                                        str(REPO / "multimodal-sae_amd" / "compat")]))
    code = ("import sae_auto_interp.features.samplers as a, msae.features.samplers as b\n"
            "from sae_auto_interp.features.samplers import train, split_quantiles, sample\n"
            "assert a is b and train is b.train and b.__name__ == 'msae.features.samplers'\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-1500:]
