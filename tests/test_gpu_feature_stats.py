"""GPU: per-feature statistics and top-example tables of the cache loop (msae_feature_stats_*, FeatureStats) against the
numpy restatement in feature_stats_ref.py, the records the same run saved, and the reference's own selections (g14)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import fakes
import feature_stats_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _tables(st):
    return (st.count.cpu().numpy(), st.act_max.cpu().numpy(), st.act_sum.cpu().numpy(), st.top_val.cpu().numpy(),
            st.top_id.cpu().numpy())


def _expected(calls, S, N, n, mode, P=576, W=64):
    """calls: [(vals [B*S, k], idx, row_base)] -> restated (count, max, sum, top_val, top_id)."""
    F, V, CF, CV, CI = [], [], [], [], []
    for vals, idx, row_base in calls:
        b, s, f, v = ref.records(vals, idx, S, N=N)
        F.append(f)
        V.append(v)
        cf, cv, ci = ref.candidates(b, s, f, v, S, mode, row_base, P=P, W=W)
        CF.append(cf), CV.append(cv), CI.append(ci)
    count, mx, sm = ref.basic_stats(np.concatenate(F), np.concatenate(V), N)
    tv, ti = ref.top_tables(np.concatenate(CF), np.concatenate(CV), np.concatenate(CI), N, n)
    return count, mx, sm, tv, ti


def _assert_same(got, exp, sum_rtol=1e-9):
    count, mx, sm, tv, ti = got
    assert np.array_equal(count, exp[0])
    assert np.array_equal(mx, exp[1])
    np.testing.assert_allclose(sm, exp[2], rtol=sum_rtol, atol=0)
    assert np.array_equal(ti, exp[4])
    assert np.array_equal(tv.view(np.uint32), exp[3].view(np.uint32))


def _zipf_topk(rng, T, k, N, a=1.2, hot=None):
    """[T, k] distinct feature ids drawn with Zipf-biased usage, nonnegative values with some exact ties."""
    w = 1.0 / np.arange(1, N + 1) ** a
    perm = rng.permutation(N)
    p = np.empty(N)
    p[perm] = w / w.sum()
    idx = np.empty((T, k), np.int64)
    for t in range(T):
        idx[t] = rng.choice(N, size=k, replace=False, p=p)
    if hot is not None:
        has = (idx == hot).any(1)
        idx[~has, 0] = hot
    vals = (rng.integers(0, 64, size=(T, k)) * 0.125).astype(np.float32)   # coarse grid: exact ties, some zeros
    return vals, idx


def _run(calls, S, N, dev, n=64, mode="window", P=576, W=64):
    from msae.features import FeatureStats

    st = FeatureStats(N, n_top=n, pool=mode, pool_len=P, window=W, device=dev)
    for vals, idx, row_base in calls:
        st.update(torch.from_numpy(vals).to(dev).view(-1, S, vals.shape[1]),
                  torch.from_numpy(idx).to(dev).view(-1, S, idx.shape[1]), row_base)
    return st


@pytest.mark.parametrize("k", [32, 256])
def test_counts_max_sum_match_the_saved_records_at_c2_width(dev, k):
    """A cache with stats on, d = 4096, N = 131072, T = 8192: count / act_max exact and act_sum to 1e-9 against the
    unfiltered COO records the same run saved."""
    from msae import Sae, SaeConfig
    from msae.features import Cache

    d, N, B, S = 4096, 131072, 4, 2048
    torch.manual_seed(5)
    sae = Sae(d, SaeConfig(num_latents=N, k=k), device=dev)
    cache = Cache(0, None, batch_size=B, stats=dict(pool="window", window=64))
    for batch in range(2):
        x = torch.randn(B * S, d, device=dev).to(torch.bfloat16)
        with torch.no_grad():
            top = sae.encode(x)
        cache.add_topk(top.top_acts.view(B, S, k), top.top_indices.view(B, S, k), N, batch, "m")
    cache.save()
    loc = cache.feature_locations["m"].numpy()
    act = cache.feature_activations["m"].numpy()
    st = cache.feature_stats["m"]
    assert st.tokens_seen == 2 * B * S
    count, mx, sm = ref.basic_stats(loc[:, 2], act, N)
    assert np.array_equal(st.count.cpu().numpy(), count)
    assert np.array_equal(st.act_max.cpu().numpy(), mx)
    np.testing.assert_allclose(st.act_sum.cpu().numpy(), sm, rtol=1e-9, atol=0)
    assert (count > 0).sum() > 1000


def test_top_tables_image_mode_bit_exact_with_ties(dev):
    """Image mode, P = 576, rows of 2880 tokens; two rows duplicated so their pooled values tie exactly and must
    resolve by ascending row."""
    rng = np.random.default_rng(1)
    N, k, S, rows = 2048, 32, 2880, 6
    vals, idx = _zipf_topk(rng, rows * S, k, N)
    vals[3 * S:4 * S], idx[3 * S:4 * S] = vals[1 * S:2 * S], idx[1 * S:2 * S]     # row 3 == row 1: exact ties
    calls = [(vals[:3 * S], idx[:3 * S], 100), (vals[3 * S:], idx[3 * S:], 103)]
    exp = _expected(calls, S, N, 64, "image")
    got = _tables(_run(calls, S, N, dev, mode="image"))
    _assert_same(got, exp)
    tied = (exp[3][:, :-1] == exp[3][:, 1:]) & (exp[4][:, 1:] >= 0)
    assert tied.sum() > 50


def test_top_tables_window_mode_bit_exact_with_ragged_tail(dev):
    """Window mode, W = 64, rows of 5 windows + a 17-position tail (not pooled), coarse values: exact ties."""
    rng = np.random.default_rng(2)
    N, k, W = 1024, 32, 64
    S = 5 * W + 17
    vals, idx = _zipf_topk(rng, 12 * S, k, N)
    calls = [(vals[r * S:(r + 4) * S], idx[r * S:(r + 4) * S], 7 + r) for r in (0, 4, 8)]
    exp = _expected(calls, S, N, 64, "window", W=W)
    st = _run(calls, S, N, dev, mode="window", W=W)
    _assert_same(_tables(st), exp)
    assert st.windows_per_row == 5
    assert (exp[4] >= 0).sum() > 1000


@pytest.mark.parametrize("mode", ["window", "image"])
def test_chunk_invariance(dev, mode):
    """The same rows fed in calls of 1, 3 and 8 rows: bit-identical tables, act_sum within 1e-12 relative."""
    rng = np.random.default_rng(3)
    N, k = 4096, 32
    S = 640 if mode == "image" else 3 * 64 + 5
    R = 24
    vals, idx = _zipf_topk(rng, R * S, k, N)
    outs = []
    for per in (1, 3, 8):
        calls = [(vals[r * S:(r + per) * S], idx[r * S:(r + per) * S], r) for r in range(0, R, per)]
        outs.append(_tables(_run(calls, S, N, dev, mode=mode)))
    for o in outs[1:]:
        for a, b in zip(o[:2] + o[3:], outs[0][:2] + outs[0][3:]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        np.testing.assert_allclose(o[2], outs[0][2], rtol=1e-12, atol=0)


def test_reference_selections_g14(dev):
    """The kernel on g14's records reproduces the selections of the reference's own constructors."""
    from msae.features.loader import dedup_image_rows

    g = np.load(GOLDEN / "g14_feature_stats.npz")
    for mode in ("window", "image"):
        S, N = int(g[f"{mode}_S"]), int(g[f"{mode}_N"])
        loc, act = g[f"{mode}_locations"], g[f"{mode}_activations"]
        rows = int(loc[:, 0].max()) + 1
        vals = np.zeros((rows * S, 1), np.float32)       # one record per token slot: k = 1 is enough
        slots = {}
        for (r, s, f), v in zip(loc.tolist(), act.tolist()):
            slots.setdefault((r, s), []).append((f, v))
        k = max(len(x) for x in slots.values())
        vals = np.zeros((rows * S, k), np.float32)
        idx = np.tile(np.arange(k, dtype=np.int64) + N, (rows * S, 1))   # out-of-range ids: not kept
        for (r, s), lst in slots.items():
            for j, (f, v) in enumerate(lst):
                vals[r * S + s, j], idx[r * S + s, j] = v, f
        st = _run([(vals, idx, 0)], S, N, dev, mode=mode, P=int(g["image_P"]), W=int(g["window_W"]))
        for i, f in enumerate(g[f"{mode}_features"].tolist()):
            ids, pv = st.top_examples(f)
            if mode == "window":
                m = int(g["max_examples"])
                sel = g["window_selected"][i]
                nw = S // int(g["window_W"])
                assert np.array_equal(ids[:m].numpy(), sel[sel >= 0]), f
                np.testing.assert_allclose(pv[:m].numpy(), g["window_pooled"][i][sel >= 0], rtol=1e-6)
                assert ((ids[:m] // nw) < rows).all()
            else:
                m = int(g["max_examples"])
                got = dedup_image_rows(ids[:m + 50].tolist(), g["image_ids"].tolist(), m)
                assert got == g["image_selected"][i].tolist(), f


def test_hostile_usage(dev):
    """One feature fires on every token, Zipf-biased usage at k = 64, n = 256: everything still matches."""
    rng = np.random.default_rng(4)
    N, k, W = 8192, 64, 64
    S = 8 * W
    vals, idx = _zipf_topk(rng, 16 * S, k, N, a=1.5, hot=77)
    vals[vals == 0] = 0.5
    calls = [(vals[:8 * S], idx[:8 * S], 0), (vals[8 * S:], idx[8 * S:], 8)]
    exp = _expected(calls, S, N, 256, "window", W=W)
    st = _run(calls, S, N, dev, n=256, mode="window", W=W)
    _assert_same(_tables(st), exp)
    assert int(st.count[77]) == 16 * S
    assert int((st.top_id[77] >= 0).sum()) == 16 * 8        # every window of every row holds it
    # image mode of the same tokens, rows of 2 * 576 (hot feature: one candidate per row)
    S2 = 1152
    calls2 = [(vals[:7 * S2], idx[:7 * S2], 0)]
    exp2 = _expected(calls2, S2, N, 256, "image")
    _assert_same(_tables(_run(calls2, S2, N, dev, n=256, mode="image")), exp2)


def _image_cache(dev, g, filters, stats):
    from msae import Sae, SaeConfig
    from msae.features import FeatureImageCache

    d, N = int(g["d"]), 4096
    torch.manual_seed(11)
    sae = Sae(d, SaeConfig(num_latents=N, k=16), device=dev)
    model = fakes.TinyLlava(vocab=int(g["vocab"]), d=d).to(dev)
    module = str(g["module"])
    return module, FeatureImageCache(model, None, {module: sae}, batch_size=2, shard_size=0, filters=filters,
                                     processor=fakes.FakeProcessor(int(g["vocab"])), stats=stats)


def test_no_side_effects_on_the_cache(dev, tmp_path, golden_dir):
    """With a filter, the COO split files are byte-identical with stats on and off, and the stats cover unfiltered
    features; the update itself runs clean under sync debug mode "error"."""
    from msae.features import FeatureStats

    g = np.load(golden_dir / "g9_image_cache.npz")
    images = [{"image": fakes.FakeImage(i)} for i in range(int(g["n_images"]))]
    module = str(g["module"])
    filters = {module: torch.arange(0, 4096, 3)}
    outs = {}
    for on in (False, True):
        _, fic = _image_cache(dev, g, filters, dict(pool="image", pool_len=4) if on else None)
        fic.run(0, images)
        out = tmp_path / ("on" if on else "off")
        fic.save_splits(n_splits=2, save_dir=str(out), rank=0)
        fic.concate_safetensors(n_splits=2, save_dir=str(out))
        outs[on] = (out, fic)
    off_files = sorted(os.listdir(outs[False][0] / module))
    on_files = sorted(os.listdir(outs[True][0] / module))
    assert on_files == sorted(off_files + ["feature_stats.safetensors"])
    for f in off_files:
        assert (outs[False][0] / module / f).read_bytes() == (outs[True][0] / module / f).read_bytes(), f
    st = FeatureStats.load(str(outs[True][0] / module / "feature_stats.safetensors"))
    assert st.tokens_seen == (len(images) // 2) * 2 * 4        # drop_last batches of 2 images, 4 positions each
    fired = np.flatnonzero(st.count.numpy())
    assert (fired % 3 != 0).any()                   # features outside the filter are counted too
    loc = outs[True][1].cache.feature_locations[module].numpy()
    assert np.array_equal(np.bincount(loc[:, 2], minlength=4096)[::3], st.count.numpy()[::3])

    rng = np.random.default_rng(6)
    vals, idx = _zipf_topk(rng, 4 * 96, 32, 4096)
    v, i = torch.from_numpy(vals).to(dev).view(4, 96, 32), torch.from_numpy(idx).to(dev).view(4, 96, 32)
    sst = FeatureStats(4096, pool="window", window=32, device=dev)
    sst.update(v, i, 0)                             # first call: library load, workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sst.update(v, i, 4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(sst.count.sum()) == 2 * int((np.abs(vals) > 1e-5).sum())


def _rank_worker(rank, world, out_dir, S, N, k):
    from msae.features import Cache

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    vals, idx = _zipf_topk(rng, 8 * S, k, N)
    rows_per = 8 // world
    cache = Cache(rank * rows_per, None, batch_size=2, stats=dict(pool="window", window=64, n_top=80))
    for b in range(rows_per // 2):
        r0 = rank * rows_per + 2 * b
        cache.add_topk(torch.from_numpy(vals[r0 * S:(r0 + 2) * S]).to(dev).view(2, S, k),
                       torch.from_numpy(idx[r0 * S:(r0 + 2) * S]).to(dev).view(2, S, k), N, b, "m")
    os.makedirs(os.path.join(out_dir, "m"), exist_ok=True)
    cache.feature_stats["m"].save(os.path.join(out_dir, "m", f"Rank{rank}_feature_stats.safetensors"))


def test_two_ranks_merge_equals_one_process(dev, tmp_path):
    """Two processes cache half the rows each; the rank files merged into feature_stats.safetensors equal a one-process
    run over all rows."""
    from msae.features import FeatureStats
    from msae.features.cache import merge_rank_stats

    S, N, k = 4 * 64, 2048, 32
    mp.spawn(_rank_worker, args=(2, str(tmp_path / "two"), S, N, k), nprocs=2, join=True)
    merged = merge_rank_stats(str(tmp_path / "two" / "m"), dev)
    assert sorted(os.listdir(tmp_path / "two" / "m")) == ["feature_stats.safetensors"]
    _rank_worker(0, 1, str(tmp_path / "one"), S, N, k)
    one = FeatureStats.load(str(tmp_path / "one" / "m" / "Rank0_feature_stats.safetensors"))
    two = FeatureStats.load(merged)
    assert two.tokens_seen == one.tokens_seen == 8 * S
    a, b = _tables(two), _tables(one)
    for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]):
        assert np.array_equal(x, y)
    np.testing.assert_allclose(a[2], b[2], rtol=1e-12, atol=0)
    assert two.metadata() == one.metadata()
