"""CPU: the feature statistics' rules (feature_stats_ref.py) against the reference's own selections (g14), the merge
rule, the file format, the reader side (top_example_records, the padded dedup, the stats-screened min_examples cut) and
the CacheConfig flags."""
import dataclasses
import subprocess
import sys

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

import feature_stats_ref as ref
from conftest import GOLDEN, REPO

RECIPE = GOLDEN / "make_golden_stats.py"


def _reference_present() -> bool:
    """The recipe knows where the reference lives (make_golden.REF); it is absent on most machines."""
    return subprocess.run([sys.executable, str(RECIPE), "--check-reference"], capture_output=True).returncode == 0


def _g14():
    return np.load(GOLDEN / "g14_feature_stats.npz")


def test_restatement_matches_reference_window_selections():
    g = _g14()
    S, N, W, m = int(g["window_S"]), int(g["window_N"]), int(g["window_W"]), int(g["max_examples"])
    loc, act = g["window_locations"], g["window_activations"]
    cf, cv, ci = ref.candidates(loc[:, 0], loc[:, 1], loc[:, 2], act, S, "window", 0, W=W)
    tv, ti = ref.top_tables(cf, cv, ci, N, 64)
    for i, f in enumerate(g["window_features"].tolist()):
        sel = g["window_selected"][i]
        assert np.array_equal(ti[f][:m][ti[f][:m] >= 0], sel[sel >= 0]), f
        np.testing.assert_allclose(tv[f][:m][sel >= 0], g["window_pooled"][i][sel >= 0], rtol=1e-6)


def test_restatement_matches_reference_image_selections():
    from msae.features.loader import dedup_image_rows

    g = _g14()
    S, N, P, m = int(g["image_S"]), int(g["image_N"]), int(g["image_P"]), int(g["max_examples"])
    loc, act = g["image_locations"], g["image_activations"]
    cf, cv, ci = ref.candidates(loc[:, 0], loc[:, 1], loc[:, 2], act, S, "image", 0, P=P)
    tv, ti = ref.top_tables(cf, cv, ci, N, 64)
    ids = g["image_ids"].tolist()
    for i, f in enumerate(g["image_features"].tolist()):
        got = dedup_image_rows(ti[f][:m + 50][ti[f][:m + 50] >= 0].tolist(), ids, m)
        assert got == g["image_selected"][i].tolist(), f


def test_recipe_regenerates_g14_byte_for_byte(tmp_path):
    if not _reference_present():
        pytest.skip("the reference is not on this machine")
    subprocess.run([sys.executable, str(RECIPE), "--out", str(tmp_path)], check=True, capture_output=True)
    a, b = np.load(tmp_path / "g14_feature_stats.npz"), _g14()
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def _random_side(rng, N, n):
    count = rng.integers(0, 100, N).astype(np.int64)
    mx = rng.standard_normal(N).astype(np.float32)
    sm = rng.standard_normal(N)
    tv = np.zeros((N, n), np.float32)
    ti = np.full((N, n), -1, np.int64)
    for f in range(N):
        c = int(rng.integers(0, n + 1))
        v = rng.integers(1, 8, c).astype(np.float32)          # small grid: exact ties across sides
        i = rng.choice(10_000, c, replace=False)
        o = np.lexsort((i, -v))
        tv[f, :c], ti[f, :c] = v[o], i[o]
    return count, mx, sm, tv, ti


def test_merge_is_associative_and_commutative():
    rng = np.random.default_rng(0)
    N, n = 50, 8
    a, b, c = (_random_side(rng, N, n) for _ in range(3))
    ab_c = ref.merge_tables(ref.merge_tables(a, b, n), c, n)
    a_bc = ref.merge_tables(a, ref.merge_tables(b, c, n), n)
    ba = ref.merge_tables(b, a, n)
    ab = ref.merge_tables(a, b, n)
    for x, y in zip(ab_c, a_bc):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12)    # sums: rounding only
    for i in (0, 1, 3, 4):
        assert np.array_equal(ab[i], ba[i]) and np.array_equal(ab_c[i], a_bc[i])


def test_save_load_round_trip(tmp_path):
    from msae.features import FeatureStats

    st = FeatureStats(300, n_top=60, pool="window", window=32, thresh=1e-5)
    st.count[:] = torch.arange(300)
    st.top_val[5, :3] = torch.tensor([3.0, 2.0, 1.0])
    st.top_id[5, :3] = torch.tensor([7, 1, 9])
    st.tokens_seen, st.windows_per_row = 1234, 4
    st.save(str(tmp_path / "s.safetensors"))
    back = FeatureStats.load(str(tmp_path / "s.safetensors"))
    assert back.metadata() == st.metadata()
    assert (back.pool, back.window, back.n_top, back.thresh, back.tokens_seen) == ("window", 32, 60, 1e-5, 1234)
    for k in ("count", "act_max", "act_sum", "top_val", "top_id"):
        assert torch.equal(getattr(back, k), getattr(st, k)), k
    ids, vals = back.top_examples(5)
    assert ids.tolist() == [7, 1, 9] and vals.tolist() == [3.0, 2.0, 1.0]
    assert torch.allclose(back.density(), torch.arange(300, dtype=torch.float64) / 1234)
    with pytest.raises(ValueError):
        FeatureStats(10, n_top=40)


def _split_dir(tmp_path, loc, act, width, n_splits, module="m"):
    from msae.features.cache import generate_split_indices

    d = tmp_path / module
    d.mkdir(parents=True, exist_ok=True)
    for s, e in generate_split_indices(width, n_splits):
        m = (loc[:, 2] >= s) & (loc[:, 2] < e)
        save_file({"locations": torch.from_numpy(loc[m]), "activations": torch.from_numpy(act[m])},
                  str(d / f"{s}_{e}.safetensors"))
    return d


def _stats_from(loc, act, S, N, mode, n=64, **kw):
    from msae.features import FeatureStats

    st = FeatureStats(N, n_top=n, pool=mode, **kw)
    cf, cv, ci = ref.candidates(loc[:, 0], loc[:, 1], loc[:, 2], act, S, mode, 0, P=kw.get("pool_len", 576),
                                W=kw.get("window", 64))
    tv, ti = ref.top_tables(cf, cv, ci, N, n)
    c, mx, sm = ref.basic_stats(loc[:, 2], act, N)
    st.count, st.act_max, st.act_sum = torch.from_numpy(c), torch.from_numpy(mx), torch.from_numpy(sm)
    st.top_val, st.top_id = torch.from_numpy(tv), torch.from_numpy(ti)
    if mode == "window":
        st.windows_per_row = S // kw["window"]
    return st


def test_top_example_records_window_mode(tmp_path):
    from msae.features.loader import top_example_records

    g = _g14()
    S, N, W, m = int(g["window_S"]), int(g["window_N"]), int(g["window_W"]), int(g["max_examples"])
    loc, act = g["window_locations"], g["window_activations"]
    _split_dir(tmp_path, loc, act, N, 4)
    st = _stats_from(loc, act, S, N, "window", window=W)
    rows = int(loc[:, 0].max()) + 1
    tokens = torch.arange(rows * S).reshape(rows, S)
    for i, f in enumerate(g["window_features"].tolist()[:20]):
        if f in (15, 31, 47, 63):
            continue                                    # the split files drop each split's last feature (reference quirk)
        ex = top_example_records(str(tmp_path), st, "m", f, m, n_splits=4, tokens=tokens)
        sel = g["window_selected"][i]
        assert ex.ids.tolist() == sel[sel >= 0].tolist()
        assert torch.equal(ex.activations.max(dim=1).values, ex.values)
        r, w = ex.ids // (S // W), ex.ids % (S // W)
        assert torch.equal(ex.tokens[:, 0], r * S + w * W)


def test_top_example_records_image_mode_and_padded_dedup(tmp_path):
    from msae.features.loader import dedup_image_rows, top_example_records

    g = _g14()
    S, N, P, m = int(g["image_S"]), int(g["image_N"]), int(g["image_P"]), int(g["max_examples"])
    loc, act = g["image_locations"], g["image_activations"]
    _split_dir(tmp_path, loc, act, N, 2)
    st = _stats_from(loc, act, S, N, "image", pool_len=P)
    ids = g["image_ids"].tolist()
    for i, f in enumerate(g["image_features"].tolist()[:10]):
        ex = top_example_records(str(tmp_path), st, "m", f, m, n_splits=2, image_ids=ids, seq_len=S)
        assert ex.ids.tolist() == g["image_selected"][i].tolist()
        for j, r in enumerate(ex.ids.tolist()):
            sel = (loc[:, 0] == r) & (loc[:, 2] == f)
            dense = np.zeros(S, np.float32)
            dense[loc[sel, 1]] = act[sel]
            assert np.array_equal(ex.activations[j].numpy(), dense)
    # fewer distinct images than max_examples: padded by repeating the first row (the reference raises here)
    assert dedup_image_rows([4, 9, 5, 2], {4: "a", 9: "b", 5: "a", 2: "b"}, 5) == [4, 9, 4, 4, 4]
    assert dedup_image_rows([3, 1, 2], ["x", "y", "y", "z"], 2) == [3, 1]


def test_min_examples_screen_selects_the_same_features(tmp_path):
    from msae.features import FeatureDataset

    g = _g14()
    S, N, W = int(g["window_S"]), int(g["window_N"]), int(g["window_W"])
    loc, act = g["window_locations"], g["window_activations"]
    d = _split_dir(tmp_path, loc, act, N, 4)
    st = _stats_from(loc, act, S, N, "window", window=W)
    sel = {"m": torch.arange(0, N, 2)}
    runs = {}
    for with_stats in (False, True):
        if with_stats:
            st.save(str(d / "feature_stats.safetensors"))
        for feats in (None, sel):
            ds = FeatureDataset(str(tmp_path), N, 4, modules=["m"], features=feats, min_examples=170)
            runs[(with_stats, feats is None)] = [(r.feature, r.locations.tolist()) for r in ds]
    assert runs[(True, True)] == runs[(False, True)] and runs[(True, False)] == runs[(False, False)]
    assert 0 < len(runs[(False, True)]) < N - 4


def test_cache_config_without_the_new_flags():
    from msae.config import CacheConfig, parse_cache_config

    cfg = parse_cache_config(["m", "d", "--n_splits", "3"])
    new = {"feature_stats": False, "stats_top": 64, "example_ctx_len": 64}
    d = cfg.to_dict()
    assert {k: d[k] for k in new} == new
    old = {f.name for f in dataclasses.fields(CacheConfig)} - set(new)
    assert {k: d[k] for k in old}["n_splits"] == 3 and d["model"] == "m" and d["dataset"] == "d"
    on = parse_cache_config(["m", "d", "--feature_stats", "--stats_top", "80", "--example_ctx_len", "32"])
    assert (on.feature_stats, on.stats_top, on.example_ctx_len) == (True, 80, 32)
    assert {k: v for k, v in on.to_dict().items() if k in old and k not in ("model", "dataset")} == \
        {k: v for k, v in parse_cache_config(["m", "d"]).to_dict().items() if k in old and k not in ("model", "dataset")}
