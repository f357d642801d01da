"""GPU: co-activation counters and neighbour lists (msae_coact_*, CoactStats) against the numpy restatement in coact_ref.py.
Everything is exact integer arithmetic plus one IEEE f64 quotient: every comparison is array_equal, bitwise on the f32
scores; there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import coact_ref as ref
import fakes
import synth

pytestmark = pytest.mark.gpu

N_C2, T_C2, K_C2, F_C2 = 131072, 8192, 32, 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _topk(rng, B, S, k, N, reserved=()):
    """[B, S, k] pairs: a token's indices distinct and outside `reserved`; values on a coarse grid, some exactly 0."""
    pool = np.setdiff1d(np.arange(N), np.asarray(reserved, np.int64))
    idx = np.stack([rng.choice(pool, size=k, replace=False) for _ in range(B * S)]).reshape(B, S, k).astype(np.int64)
    vals = (rng.integers(0, 64, size=(B, S, k)) * 0.125).astype(np.float32)
    return vals, idx


def _run(calls, queries, pool, N, dev, P=576, W=64, index_dtype=torch.int64):
    from msae.features import CoactStats

    st = CoactStats(N, queries, pool=pool, pool_len=P, window=W, device=dev)
    for vals, idx in calls:
        st.update(torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev).to(index_dtype))
    return st


def _assert_state(st, exp):
    assert st.counts.dtype == torch.int32 and st.seg_count.dtype == torch.int64
    assert np.array_equal(st.seg_count.cpu().numpy(), exp[1])
    assert np.array_equal(st.counts.cpu().numpy(), exp[0])
    assert st.n_segments == exp[2]


def _case_a():
    """Token pool, B = 3, S = 37, k = 32, N = 4096, F = 17 (unsorted): query 100 fires on every token, query 200 never,
    query 300 only below thresh; member 400 (no query) fires on every token; one negative value, two out-of-range ids."""
    rng = np.random.default_rng(11)
    B, S, k, N = 3, 37, 32, 4096
    vals, idx = _topk(rng, B, S, k, N, reserved=(100, 200, 300, 400))
    idx[:, :, 0], vals[:, :, 0] = 100, 1.5
    idx[:, :, 1], vals[:, :, 1] = 400, 0.25
    idx[:, ::3, 2], vals[:, ::3, 2] = 300, 5e-6
    vals[1, 5, 7] = -2.0
    idx[0, 3, 9], idx[2, 30, 4] = N, -1
    vals[0, 3, 9] = vals[2, 30, 4] = 1.0
    fired = np.unique(idx[(vals > 1e-5) & (idx >= 0) & (idx < N)])
    extra = rng.choice(np.setdiff1d(fired, [100, 400]), size=14, replace=False)
    queries = rng.permutation(np.concatenate([[100, 200, 300], extra])).tolist()
    return [(vals, idx)], queries, N


@pytest.fixture(scope="module")
def case_a():
    calls, queries, N = _case_a()
    return calls, queries, N, ref.run(calls, queries, "token", N)


def _c2_pairs():
    """[8192, 32] pairs at N = 131072 from synth's counter-based streams: feature ids concentrated on the low ids (a cube
    law, so features recur and co-fire; a token may repeat one -- it counts once), positive values."""
    u = np.abs(synth.normalish(77, T_C2 * K_C2)) / np.float32(3.47)
    idx = np.minimum((u.astype(np.float64) ** 3 * N_C2).astype(np.int64), N_C2 - 1).reshape(T_C2, K_C2)
    vals = (np.abs(synth.normalish(78, T_C2 * K_C2)) + np.float32(0.01)).reshape(T_C2, K_C2)
    return vals, idx


@pytest.fixture(scope="module")
def case_c2():
    vals, idx = _c2_pairs()
    freq = np.bincount(idx.reshape(-1), minlength=N_C2)
    top = np.argsort(-freq, kind="stable")[:F_C2 - 2]
    queries = np.random.default_rng(5).permutation(np.concatenate([top, [N_C2 - 1, 70001]])).tolist()
    calls = [(vals.reshape(4, 2048, K_C2), idx.reshape(4, 2048, K_C2))]
    return calls, queries, ref.run(calls, queries, "token", N_C2)


@pytest.fixture(scope="module")
def state_a(dev, case_a):
    calls, queries, N, exp = case_a
    return _run(calls, queries, "token", N, dev)


@pytest.fixture(scope="module")
def state_c2(dev, case_c2):
    calls, queries, exp = case_c2
    return _run(calls, queries, "token", N_C2, dev)


def test_token_pool_case_a(state_a, case_a):
    calls, queries, N, exp = case_a
    _assert_state(state_a, exp)
    sc, c = exp[1], exp[0]
    assert sc[100] == sc[400] == 111 and sc[200] == sc[300] == 0
    assert c[queries.index(100), 400] == 111 and c[queries.index(200)].sum() == 0 and c[queries.index(300)].sum() == 0
    for i, q in enumerate(queries):
        assert c[i, q] == sc[q]


@pytest.mark.parametrize("k", [5, 256])
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_token_pool_other_k(dev, k, index_dtype):
    """k = 5 (a fraction of a wave) and k = 256 (four key slots per lane); a repeated index inside a token counts once."""
    rng = np.random.default_rng(12 + k)
    B, S, N = 2, 19, 4096
    vals, idx = _topk(rng, B, S, k, N)
    idx[0, 4, k - 1], vals[0, 4, k - 1], vals[0, 4, 0] = idx[0, 4, 0], 2.0, 1.0       # a caller's repeat, far apart
    queries = rng.choice(np.unique(idx), size=23, replace=False).tolist() + [int(idx[0, 4, 0])]
    queries = list(dict.fromkeys(queries))
    exp = ref.run([(vals, idx)], queries, "token", N)
    _assert_state(_run([(vals, idx)], queries, "token", N, dev, index_dtype=index_dtype), exp)
    assert exp[0].sum() > 0


def _case_d():
    """Image pool, B = 4, S = 700, P = 576, k = 32, N = 4096: feature 50 on 400 positions of image 1 and on every position
    of image 2, feature 60 only at positions >= P."""
    rng = np.random.default_rng(13)
    B, S, k, N = 4, 700, 32, 4096
    vals, idx = _topk(rng, B, S, k, N, reserved=(50, 60))
    idx[1, :400, 0], vals[1, :400, 0] = 50, 1.0
    idx[2, :, 3], vals[2, :, 3] = 50, 2.0
    idx[:, 576:, 5], vals[:, 576:, 5] = 60, 1.0
    queries = [50, 60] + rng.choice(np.setdiff1d(np.arange(N), [50, 60]), size=15, replace=False).tolist()
    return [(vals, idx)], queries, N


def test_image_pool_case_d(dev):
    calls, queries, N = _case_d()
    exp = ref.run(calls, queries, "image", N, P=576)
    _assert_state(_run(calls, queries, "image", N, dev, P=576), exp)
    assert exp[1][50] == 2 and exp[1][60] == 0 and exp[0][1].sum() == 0 and exp[2] == 4


def test_window_pool_case_e(dev):
    """Window pool, W = 64, S = 200 (a tail of 8 dropped), B = 3; feature 70 only in the tail."""
    rng = np.random.default_rng(14)
    B, S, k, N = 3, 200, 32, 4096
    vals, idx = _topk(rng, B, S, k, N, reserved=(70,))
    idx[:, 192:, 2], vals[:, 192:, 2] = 70, 1.0
    queries = [70] + rng.choice(np.setdiff1d(np.arange(N), [70]), size=16, replace=False).tolist()
    exp = ref.run([(vals, idx)], queries, "window", N, W=64)
    _assert_state(_run([(vals, idx)], queries, "window", N, dev, W=64), exp)
    assert exp[2] == 9 and exp[1][70] == 0 and exp[0].sum() > 0


@pytest.mark.parametrize("pool", ["token", "window", "image"])
def test_one_query_and_an_unsorted_list(dev, pool):
    rng = np.random.default_rng(15)
    B, S, k, N = 3, 50, 16, 1001                            # N % 4 != 0: rows off the 16-byte grid
    vals, idx = _topk(rng, B, S, k, N)
    for queries in ([int(idx[1, 7, 3])], [1000, 5, 400, 17, 3]):
        exp = ref.run([(vals, idx)], queries, pool, N, P=40, W=16)
        st = _run([(vals, idx)], queries, pool, N, dev, P=40, W=16)
        _assert_state(st, exp)
        assert st.queries.tolist() == queries
        ind, val = st.neighbors(k=10)
        ri, rv = ref.neighbors(exp[0], exp[1], queries, 10)
        assert np.array_equal(ind.cpu().numpy(), ri)
        assert np.array_equal(val.cpu().numpy().view(np.uint32), rv.view(np.uint32))


def test_more_query_members_than_one_chunk(dev):
    """Image pool: every active feature of segment 0 is a query (about 2000 of them, in a range of 3200 keys: several
    rounds of the query list, each one full of queries)."""
    rng = np.random.default_rng(16)
    B, S, k, N = 2, 100, 32, 4096
    vals, idx = _topk(rng, B, S, k, N)
    vals[vals == 0] = 0.5
    queries = np.unique(idx[0]).tolist()
    assert len(queries) > 1024
    exp = ref.run([(vals, idx)], queries, "image", N, P=100)
    _assert_state(_run([(vals, idx)], queries, "image", N, dev, P=100), exp)
    assert (np.diagonal(exp[0][:, queries]) >= 1).all()


def test_production_width_token(state_c2, case_c2):
    calls, queries, exp = case_c2
    _assert_state(state_c2, exp)
    assert (exp[0] > 0).sum() > 20000 and exp[2] == T_C2


def test_production_width_image(dev, case_c2):
    calls, queries, _ = case_c2
    vals, idx = calls[0][0].reshape(-1, K_C2)[:5760].reshape(2, 2880, K_C2), calls[0][1].reshape(-1, K_C2)[:5760].reshape(2, 2880, K_C2)
    exp = ref.run([(vals, idx)], queries, "image", N_C2, P=576)
    _assert_state(_run([(vals, idx)], queries, "image", N_C2, dev, P=576), exp)
    assert exp[0].max() == 2 and exp[2] == 2


@pytest.mark.parametrize("pool", ["token", "window", "image"])
def test_cut_order_and_merge_on_the_device(dev, pool):
    rng = np.random.default_rng(17)
    B, S, k, N = 9, 70, 32, 2048
    vals, idx = _topk(rng, B, S, k, N)
    queries = rng.choice(N, size=40, replace=False).tolist()
    kw = dict(P=48, W=16)
    one = _run([(vals, idx)], queries, pool, N, dev, **kw)
    cuts = [(vals[5:], idx[5:]), (vals[:2], idx[:2]), (vals[2:5], idx[2:5])]
    three = _run(cuts, queries, pool, N, dev, **kw)
    assert torch.equal(one.counts, three.counts) and torch.equal(one.seg_count, three.seg_count)
    assert one.n_segments == three.n_segments
    a, b = _run(cuts[:1], queries, pool, N, dev, **kw), _run(cuts[1:], queries, pool, N, dev, **kw)
    a.merge(b)
    assert torch.equal(one.counts, a.counts) and torch.equal(one.seg_count, a.seg_count) and one.n_segments == a.n_segments
    _assert_state(one, ref.run([(vals, idx)], queries, pool, N, **kw))


def _assert_topk(st, counts, sc, queries, m, metric, exclude_self):
    from msae.features.coact import METRICS, _neighbors_host

    ind, val = st.neighbors(k=m, metric=metric, exclude_self=exclude_self)
    ri, rv = ref.neighbors(counts, sc, queries, m, metric, exclude_self)
    assert ind.dtype == torch.int64 and val.dtype == torch.float32
    assert np.array_equal(ind.cpu().numpy(), ri)
    assert np.array_equal(val.cpu().numpy().view(np.uint32), rv.view(np.uint32))
    v32, i32 = torch.ops.msae.coact_topk(st.counts, st.seg_count, st.queries.to(torch.int32), m, METRICS[metric],
                                         exclude_self, False)
    assert i32.dtype == torch.int32 and torch.equal(i32.long(), ind) and torch.equal(v32.view(torch.int32), val.view(torch.int32))
    hi, hv = _neighbors_host(st.counts.cpu(), st.seg_count.cpu(), st.queries.cpu(), m, metric, exclude_self)
    assert torch.equal(hi, ind.cpu()) and torch.equal(hv.view(torch.int32), val.cpu().view(torch.int32))
    return ri


@pytest.mark.parametrize("metric", ["jaccard", "count"])
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("m", [1, 10, 64])
def test_topk_on_case_a_and_planted_ties(dev, state_a, case_a, metric, exclude_self, m):
    from msae.features import CoactStats

    calls, queries, N, exp = case_a
    ri = _assert_topk(state_a, exp[0], exp[1], queries, m, metric, exclude_self)
    assert (ri[queries.index(200)] == -1).all()
    counts, sc, q = ref.planted_state()
    st = CoactStats(counts.shape[1], q, device=dev)
    st.counts.copy_(torch.from_numpy(counts))
    st.seg_count.copy_(torch.from_numpy(sc))
    ri = _assert_topk(st, counts, sc, q, m, metric, exclude_self)
    if metric == "jaccard" and exclude_self and m == 10:
        assert ri[0].tolist() == [30, 2, 7, 11, 17, 25, 12, -1, -1, -1] and ri[1].tolist() == [2, 3] + [-1] * 8


@pytest.mark.parametrize("metric", ["jaccard", "count"])
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("m", [1, 10, 64])
def test_topk_at_production_width(state_c2, case_c2, metric, exclude_self, m):
    calls, queries, exp = case_c2
    ri = _assert_topk(state_c2, exp[0], exp[1], queries, m, metric, exclude_self)
    assert (ri[:, 0] >= 0).sum() >= F_C2 - 2


def test_no_host_sync_and_no_allocation_growth(dev):
    rng = np.random.default_rng(18)
    B, S, k, N = 4, 96, 32, 4096
    vals, idx = _topk(rng, B, S, k, N)
    v, i = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev)
    queries = rng.choice(N, size=30, replace=False).tolist()
    from msae.features import CoactStats

    for pool in ("token", "window", "image"):
        st = CoactStats(N, queries, pool=pool, pool_len=64, window=32, device=dev)
        st.update(v, i)                                     # first call: library load, workspace, slot table
        st.neighbors(k=10)
        torch.cuda.synchronize()
        before = torch.cuda.memory_reserved(dev)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                st.update(v, i)
            ind, val = st.neighbors(k=10)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.cuda.memory_reserved(dev) == before
        exp = ref.run([(vals, idx)] * 4, queries, pool, N, P=64, W=32)
        _assert_state(st, exp)
        assert np.array_equal(ind.cpu().numpy(), ref.neighbors(exp[0], exp[1], queries, 10)[0])


def _image_cache(dev, g, filters, stats, coact):
    from msae import Sae, SaeConfig
    from msae.features import FeatureImageCache

    d, N = int(g["d"]), 4096
    torch.manual_seed(11)
    sae = Sae(d, SaeConfig(num_latents=N, k=16), device=dev)
    model = fakes.TinyLlava(vocab=int(g["vocab"]), d=d).to(dev)
    module = str(g["module"])
    return FeatureImageCache(model, None, {module: sae}, batch_size=2, shard_size=0, filters=filters,
                             processor=fakes.FakeProcessor(int(g["vocab"])), stats=stats, coact=coact)


def test_end_to_end_cache(dev, tmp_path, golden_dir):
    """A FeatureImageCache run over the fake images with coact on: the merged coact.safetensors equals the restatement over
    every batch's top-k; with coact=None the same run writes nothing of it, and its split files are byte-identical.
    feature_stats.safetensors is compared tensor by tensor (its writer does not fix the order of the metadata keys, and
    act_sum is a float atomic sum: 1e-12 relative, as the feature statistics' own tests compare it)."""
    from msae.features import CoactStats, FeatureStats

    g = np.load(golden_dir / "g9_image_cache.npz")
    images = [{"image": fakes.FakeImage(i)} for i in range(int(g["n_images"]))]
    module = str(g["module"])
    filters = {module: torch.arange(0, 4096, 3)}
    outs, seen = {}, []
    for on in (False, True):
        fic = _image_cache(dev, g, filters, dict(pool="image", pool_len=4), dict(pool="image", pool_len=3) if on else None)
        if on:
            inner = fic.cache.add_topk

            def spy(top_acts, top_indices, *a, **kw):
                seen.append((top_acts.cpu().numpy(), top_indices.cpu().numpy()))
                return inner(top_acts, top_indices, *a, **kw)

            fic.cache.add_topk = spy
        fic.run(0, images)
        out = tmp_path / ("on" if on else "off")
        fic.save_splits(n_splits=2, save_dir=str(out), rank=0)
        if on:
            assert "Rank0_coact.safetensors" in os.listdir(out / module)
        fic.concate_safetensors(n_splits=2, save_dir=str(out))
        outs[on] = out / module
        assert (fic.cache.coact_stats == {}) == (not on)
    off_files, on_files = sorted(os.listdir(outs[False])), sorted(os.listdir(outs[True]))
    assert on_files == sorted(off_files + ["coact.safetensors"])
    for f in off_files:
        if f != "feature_stats.safetensors":
            assert (outs[False] / f).read_bytes() == (outs[True] / f).read_bytes(), f
    a, b = (FeatureStats.load(str(outs[x] / "feature_stats.safetensors")) for x in (False, True))
    assert a.metadata() == b.metadata()
    for name in ("count", "act_max", "top_val", "top_id"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    np.testing.assert_allclose(a.act_sum.numpy(), b.act_sum.numpy(), rtol=1e-12, atol=0)
    st = CoactStats.load(str(outs[True] / "coact.safetensors"))
    queries = filters[module].tolist()
    assert st.queries.tolist() == queries and st.pool == "image" and st.pool_len == 3
    assert len(seen) == len(images) // 2
    exp = ref.run(seen, queries, "image", 4096, P=3)
    _assert_state(st, exp)
    assert exp[0].sum() > 0 and (exp[1][np.arange(4096) % 3 != 0] > 0).any()     # the member side is not filtered


def test_two_rank_files_merge_to_the_single_rank_file(dev, tmp_path):
    """The rows split by hand over two ranks, saved as rank files and merged by the cache's concat step: byte-identical to
    the file of one rank that saw every row."""
    from msae.features.cache import merge_rank_coact

    rng = np.random.default_rng(19)
    B, S, k, N = 8, 64, 32, 2048
    vals, idx = _topk(rng, B, S, k, N)
    queries = rng.choice(N, size=50, replace=False).tolist()
    for name, parts in (("two", [(vals[:4], idx[:4]), (vals[4:], idx[4:])]), ("one", [(vals, idx)])):
        os.makedirs(tmp_path / name / "m")
        for r, part in enumerate(parts):
            _run([part], queries, "window", N, dev, W=16).save(str(tmp_path / name / "m" / f"Rank{r}_coact.safetensors"))
        assert merge_rank_coact(str(tmp_path / name / "m"), dev) == str(tmp_path / name / "m" / "coact.safetensors")
        assert os.listdir(tmp_path / name / "m") == ["coact.safetensors"]
    assert (tmp_path / "two" / "m" / "coact.safetensors").read_bytes() == (tmp_path / "one" / "m" / "coact.safetensors").read_bytes()
