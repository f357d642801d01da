"""CPU: the co-activation statistics' contract (include/msae.h msae_coact_*) -- the numpy restatement
against a brute-force set definition, the laws the exact integer sums obey, the CPU neighbour lists, the file format, the
argument checks (all before any device work) and the command-line flags."""
import json

import numpy as np
import pytest
import torch

import coact_ref as ref

N = 40
THRESH = 1e-5


def _tiny():
    """[B=2, S=7, k=4] with every case of the contract: a feature repeated inside a segment (and inside a token),
    entries at and below thresh, negative values above it, a zero-padded list, image positions >= P, a window tail,
    out-of-range indices on both sides."""
    B, S, k = 2, 7, 4
    vals = np.zeros((B, S, k), np.float32)
    idx = np.zeros((B, S, k), np.int64)
    rows = {
        (0, 0): [(1.0, 3), (0.5, 5), (2.0, 3), (0.0, 0)],            # 3 twice in one token
        (0, 1): [(-0.75, 3), (1e-5, 9), (5e-6, 11), (-1e-5, 12)],     # negative kept; at / below thresh dropped
        (0, 2): [(1.0, 5), (1.0, 7), (0.0, 0), (0.0, 0)],             # zero-padded list
        (0, 3): [(1.0, 7), (1.0, N), (1.0, -1), (1.0, N + 100)],      # out of range
        (0, 4): [(1.0, 20), (1.0, 3), (-2e-5, 21), (1.0, 5)],
        (0, 5): [(1.0, 30), (1.0, 31), (1.0, 3), (1.0, 7)],           # image: s >= P = 5
        (0, 6): [(1.0, 32), (1.0, 3), (1.0, 33), (0.0, 0)],           # window tail (W = 3) and s >= P
        (1, 0): [(1.0, 7), (3.0, 8), (0.0, 0), (0.0, 0)],
        (1, 2): [(1.0, 8), (1.0, 3), (1.0, 39), (1.0, 0)],
        (1, 6): [(1.0, 34), (1.0, 7), (0.0, 0), (0.0, 0)],
    }
    for (b, s), lst in rows.items():
        for j, (v, f) in enumerate(lst):
            vals[b, s, j], idx[b, s, j] = v, f
    return vals, idx


QUERIES = [7, 3, 34, 11, 0]      # unsorted; 11 only below thresh; 34 only in tails


@pytest.mark.parametrize("pool", ["token", "window", "image"])
def test_restatement_equals_the_set_definition(pool):
    vals, idx = _tiny()
    rng = np.random.default_rng(1)
    v2 = (rng.integers(-3, 6, size=(3, 11, 5)) * 0.5).astype(np.float32)
    i2 = rng.integers(-2, N + 2, size=(3, 11, 5))
    calls = [(vals, idx), (v2, i2)]
    got = ref.run(calls, QUERIES, pool, N, THRESH, P=5, W=3)
    exp = ref.brute_force(calls, QUERIES, pool, N, THRESH, P=5, W=3)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[2] == exp[2]
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64
    # what the planted cases must give on the first call alone
    c, sc, n = ref.run([(vals, idx)], QUERIES, pool, N, THRESH, P=5, W=3)
    assert n == {"token": 14, "window": 4, "image": 2}[pool]
    assert sc[3] == {"token": 6, "window": 3, "image": 2}[pool]        # the repeat inside a token / segment counts once
    assert sc[9] == sc[11] == sc[12] == 0 and sc[21] == 1               # |v| <= thresh dropped, -2e-5 kept
    assert c[QUERIES.index(11)].sum() == 0
    if pool == "image":
        assert sc[30] == sc[32] == sc[34] == 0                          # only at positions >= P
    if pool == "window":
        assert sc[32] == sc[34] == 0 and sc[30] == 1                    # the tail position 6 is not pooled


@pytest.mark.parametrize("pool", ["token", "window", "image"])
def test_diagonal_and_symmetry(pool):
    rng = np.random.default_rng(2)
    vals = (rng.integers(0, 4, size=(4, 13, 6)) * 0.5).astype(np.float32)
    idx = rng.integers(0, N, size=(4, 13, 6))
    q = [5, 17, 2, 39, 8]
    counts, sc, _ = ref.run([(vals, idx)], q, pool, N, THRESH, P=9, W=4)
    for i, qi in enumerate(q):
        assert counts[i, qi] == sc[qi]
        for j, qj in enumerate(q):
            assert counts[i, qj] == counts[j, qi]
    assert counts.sum() > 0


def _state(st):
    return st.counts.cpu().numpy(), st.seg_count.cpu().numpy(), st.n_segments


def _filled(state, queries, pool="token", **kw):
    """A host CoactStats holding a restated state."""
    from msae.features import CoactStats

    st = CoactStats(state[0].shape[1], queries, pool=pool, **kw)
    st.counts.copy_(torch.from_numpy(state[0]))
    st.seg_count.copy_(torch.from_numpy(state[1]))
    st.n_segments = int(state[2])
    return st


@pytest.mark.parametrize("pool", ["token", "window", "image"])
def test_cut_order_and_merge_laws(pool):
    from msae.features import CoactStats

    rng = np.random.default_rng(3)
    vals = (rng.integers(0, 4, size=(9, 10, 5)) * 0.5).astype(np.float32)
    idx = rng.integers(0, N, size=(9, 10, 5))
    q = [1, 30, 12]
    kw = dict(P=6, W=4)
    one = ref.run([(vals, idx)], q, pool, N, THRESH, **kw)
    cuts = [(vals[5:], idx[5:]), (vals[:2], idx[:2]), (vals[2:5], idx[2:5])]
    three = ref.run(cuts, q, pool, N, THRESH, **kw)
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1]) and one[2] == three[2]
    skw = dict(pool_len=6, window=4)
    a = _filled(ref.run(cuts[:1], q, pool, N, THRESH, **kw), q, pool, **skw)
    b = _filled(ref.run(cuts[1:], q, pool, N, THRESH, **kw), q, pool, **skw)
    m = _state(a.merge(b))
    assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
    with pytest.raises(ValueError):
        a.merge(CoactStats(N, [1, 12, 30], pool=pool, **skw))          # another query order is another list
    with pytest.raises(ValueError):
        a.merge(CoactStats(N, q, pool="token" if pool != "token" else "image", **skw))
    with pytest.raises(ValueError):
        a.merge(CoactStats(N, q, pool=pool, thresh=1e-3, **skw))


_planted = ref.planted_state


@pytest.mark.parametrize("metric", ["jaccard", "count"])
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("m", [1, 10, 64])
def test_neighbors_host_equals_restatement(metric, exclude_self, m):
    counts, sc, q = _planted()
    st = _filled((counts, sc, 10), q)
    ind, val = st.neighbors(k=m, metric=metric, exclude_self=exclude_self)
    ri, rv = ref.neighbors(counts, sc, q, m, metric, exclude_self)
    assert ind.dtype == torch.int64 and val.dtype == torch.float32 and ind.shape == (4, m)
    assert np.array_equal(ind.numpy(), ri)
    assert np.array_equal(val.numpy().view(np.uint32), rv.view(np.uint32))
    assert (ind[2] == -1).all() and (val[2] == 0).all()                 # a query that never fired
    if metric == "jaccard" and exclude_self and m == 10:
        # 30 (1.0), 2 (2/4 = 0.5), then the 1/3 ties by ascending feature -- 25 holds 2/6 --, then 12 (1/4)
        assert ind[0].tolist() == [30, 2, 7, 11, 17, 25, 12, -1, -1, -1]
        assert val[0, 2] == val[0, 5] == np.float32(1.0 / 3.0)
        assert ind[1].tolist() == [2, 3] + [-1] * 8 and val[1].tolist()[2:] == [0.0] * 8
    if metric == "jaccard" and not exclude_self and m == 10:
        assert ind[0].tolist()[:2] == [4, 30]                           # the self tie: ascending feature


def test_file_round_trip_and_get_neighbors_shape(tmp_path):
    from msae.features import CoactStats, coact_neighbors
    from safetensors.torch import load_file, save_file

    counts, sc, q = _planted()
    st = _filled((counts, sc, 10), q, pool="window", window=16)
    p1, p2 = tmp_path / "a.safetensors", tmp_path / "b.safetensors"
    st.save(str(p1))
    back = CoactStats.load(str(p1))
    back.save(str(p2))
    assert p1.read_bytes() == p2.read_bytes()
    assert np.array_equal(back.counts.numpy(), counts) and np.array_equal(back.seg_count.numpy(), sc)
    assert back.n_segments == 10 and back.pool == "window" and back.window == 16 and back.queries.tolist() == q
    raw = load_file(str(p1))
    key = raw["pair_key"].numpy()
    assert raw["pair_key"].dtype == torch.int64 and raw["pair_count"].dtype == torch.int32
    assert (np.diff(key) > 0).all() and np.array_equal(key, np.flatnonzero(counts.reshape(-1)))
    assert np.array_equal(raw["pair_count"].numpy(), counts.reshape(-1)[key])
    assert np.array_equal(st.row(9).numpy(), counts[1])
    with pytest.raises(KeyError):
        st.row(5)
    other = tmp_path / "other.safetensors"
    save_file(raw, str(other), metadata={"format": "msae.feature_stats.v1"})
    with pytest.raises(ValueError):
        CoactStats.load(str(other))

    nd, plf = coact_neighbors({"m": st, "unused": st}, {"m": [9, 4], "unused": []}, k=4)
    assert set(nd) == {"m"} and set(nd["m"]) == {0, 1}
    assert nd["m"][0] == {"indices": [2, 3], "values": [float(np.float32(2 / 3)), 0.5]}
    assert nd["m"][1]["indices"] == [30, 2, 7] and len(nd["m"][1]["values"]) == 3
    assert plf == {"m": [2, 3, 4, 7, 9, 30]}
    with pytest.raises(ValueError):
        coact_neighbors({"m": st}, {"m": [5]}, k=4)


def test_argument_errors_raise_before_any_device_work():
    from msae.features import CoactStats

    with pytest.raises(ValueError):
        CoactStats(N, [1, 2, 1])
    with pytest.raises(ValueError):
        CoactStats(N, [1, N])
    with pytest.raises(ValueError):
        CoactStats(N, [-1])
    with pytest.raises(ValueError):
        CoactStats(N, [])
    with pytest.raises(ValueError):
        CoactStats(262144, list(range(16385)), max_bytes=1 << 40)
    with pytest.raises(ValueError):
        CoactStats(262145, [0])
    with pytest.raises(ValueError):
        CoactStats(N, [1, 2], max_bytes=2 * N * 4 - 1)
    CoactStats(N, [1, 2], max_bytes=2 * N * 4)
    with pytest.raises(ValueError):
        CoactStats(N, [1], pool="row")
    with pytest.raises(ValueError):
        CoactStats(N, [1], pool="image", pool_len=2881)
    with pytest.raises(ValueError):
        CoactStats(N, [1], pool="window", window=0)
    st = CoactStats(N, [1, 2])
    with pytest.raises(ValueError):                                     # k > 256: a host check, the tensors are not touched
        st.update(torch.zeros(1, 2, 257), torch.zeros(1, 2, 257, dtype=torch.int64))
    st.n_segments = (1 << 31) - 6
    with pytest.raises(OverflowError):
        st.update(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int64))
    st.n_segments = (1 << 31) - 8                                       # 6 more segments fit: now the device is asked for
    with pytest.raises(RuntimeError):
        st.update(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int64))
    assert st.n_segments == (1 << 31) - 8
    other = CoactStats(N, [1, 2])
    other.n_segments = 8
    with pytest.raises(OverflowError):
        st.merge(other)
    with pytest.raises(ValueError):
        st.neighbors(k=65)
    with pytest.raises(ValueError):
        st.neighbors(metric="dice")


def test_cache_needs_queries_and_allocates_nothing_when_off():
    from msae.features import Cache

    with pytest.raises(ValueError):
        Cache(0, None, coact=dict(pool="token"))
    off = Cache(0, None)
    assert off.coact is None and off.coact_stats == {}
    on = Cache(0, {"m": torch.tensor([3, 1])}, coact=dict(pool="token"))
    assert on._new_coact("m", N, "cpu").queries.tolist() == [3, 1]
    on = Cache(0, None, coact=dict(pool="image", pool_len=4, queries={"m": [5, 2]}))
    st = on._new_coact("m", N, "cpu")
    assert st.queries.tolist() == [5, 2] and st.pool == "image" and st.pool_len == 4
    with pytest.raises(ValueError):
        on._new_coact("other", N, "cpu")


def test_cli_flags(tmp_path, capsys):
    from msae.config import coact_kwargs, parse_cache_config
    from msae.launch.cache import cache, cache_image
    from msae.launch.features import neighbors

    filt = tmp_path / "f.json"
    filt.write_text(json.dumps({"layers.1": [9, 4]}))
    cfg = parse_cache_config(["model", "data", "--filters_path", str(filt)])
    assert cfg.coact is False and coact_kwargs(cfg, cache.COACT_DEFAULT_POOL) is None
    cfg = parse_cache_config(["model", "data", "--coact", "--filters_path", str(filt)])
    assert coact_kwargs(cfg, cache.COACT_DEFAULT_POOL) == dict(pool="token", window=64, pool_len=576)
    assert coact_kwargs(cfg, cache_image.COACT_DEFAULT_POOL, pool_len=9)["pool"] == "image"
    cfg = parse_cache_config(["model", "data", "--coact", "--coact_pool", "window", "--example_ctx_len", "32",
                              "--coact_features", str(filt)])
    kw = coact_kwargs(cfg, cache_image.COACT_DEFAULT_POOL)
    assert kw["pool"] == "window" and kw["window"] == 32 and kw["queries"]["layers.1"].tolist() == [9, 4]
    with pytest.raises(SystemExit):
        parse_cache_config(["model", "data", "--coact"])
    assert "--coact" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_cache_config(["model", "data", "--coact", "--coact_pool", "row", "--filters_path", str(filt)])
    assert "--coact_pool" in capsys.readouterr().err

    # the neighbours launcher reads a cache's coact.safetensors without a checkpoint or a GPU
    counts, sc, q = _planted()
    st = _filled((counts, sc, 10), q)
    (tmp_path / "save" / "layers.1").mkdir(parents=True)
    st.save(str(tmp_path / "save" / "layers.1" / "coact.safetensors"))
    out = tmp_path / "nb.safetensors"
    neighbors.main(["--coact", str(tmp_path / "save"), "--k", "3", "--device", "cpu", "--out", str(out),
                    "--features", str(filt)])
    from safetensors.torch import load_file

    got = load_file(str(out))
    ri, rv = ref.neighbors(counts, sc, q, 3)
    assert got["features"].tolist() == [9, 4]
    assert np.array_equal(got["indices"].numpy(), ri[[1, 0]]) and np.array_equal(got["values"].numpy(), rv[[1, 0]])
    with pytest.raises(SystemExit):
        neighbors.parse_argument(["--k", "3"])
