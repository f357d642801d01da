"""GPU: the per-feature uniform example sample of the statistics update (msae_feature_stats_update_sampled,
msae_feature_sample_merge, FeatureStats(n_sample=)) bit for bit against the numpy restatement in feature_sample_ref.py, and
the rest of the statistics bit for bit against a run with the sample off."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import feature_sample_ref as sref
import feature_stats_ref as ref

pytestmark = pytest.mark.gpu

SEED = 22


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _topk(rng, T, k, N, lo=1, hi=64, step=0.125, hot=None):
    """[T, k] distinct feature ids per token and values on a coarse grid (exact ties; zeros and signs when lo <= 0)."""
    idx = np.argsort(rng.random((T, N)), axis=1)[:, :k].astype(np.int64)
    if hot is not None:
        idx[~(idx == hot).any(1), 0] = hot
    vals = (rng.integers(lo, hi, size=(T, k)) * step).astype(np.float32)
    return vals, idx


def _run(calls, S, N, dev, n_sample, mode="window", P=576, W=64, seed=SEED, n_top=64):
    from msae.features import FeatureStats

    st = FeatureStats(N, n_top=n_top, pool=mode, pool_len=P, window=W, device=dev, n_sample=n_sample, sample_seed=seed)
    for vals, idx, row_base in calls:
        st.update(torch.from_numpy(vals).to(dev).view(-1, S, vals.shape[1]),
                  torch.from_numpy(idx).to(dev).view(-1, S, idx.shape[1]), row_base)
    return st


def _candidates(calls, S, N, mode, P=576, W=64):
    CF, CV, CI = [], [], []
    for vals, idx, row_base in calls:
        b, s, f, v = ref.records(vals, idx, S, N=N)
        cf, cv, ci = ref.candidates(b, s, f, v, S, mode, row_base, P=P, W=W)
        CF.append(cf), CV.append(cv), CI.append(ci)
    return np.concatenate(CF), np.concatenate(CV), np.concatenate(CI)


def _sample(st):
    return st.seg_count.cpu().numpy(), st.smp_val.cpu().numpy(), st.smp_id.cpu().numpy()


def _assert_sample(got, exp):
    assert np.array_equal(got[0], exp[0])
    assert np.array_equal(got[2], exp[2])
    assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32))


def _assert_rest_equal(a, b):
    """count, act_max, top_val, top_id bit-identical between two FeatureStats."""
    for k in ("count", "act_max", "top_val", "top_id"):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


@pytest.fixture(scope="module")
def window_case():
    """W = 4, S = 6 * 4 + 3, N = 257, k = 8; 40 rows at row_base 2^33 + r in calls of 16 / 16 / 8 rows; feature 256 forced
    onto every token: 96 candidates per 16-row call (two chunks of 64), 240 in all."""
    rng = np.random.default_rng(31)
    W, N, k, rows = 4, 257, 8, 40
    S = 6 * W + 3
    vals, idx = _topk(rng, rows * S, k, N, hot=256)
    calls = [(vals[a * S:b * S], idx[a * S:b * S], 2 ** 33 + a) for a, b in ((0, 16), (16, 32), (32, 40))]
    cand = _candidates(calls, S, N, "window", W=W)
    return dict(W=W, N=N, S=S, calls=calls, cand=cand)


@pytest.fixture(scope="module")
def window_off(window_case, dev):
    c = window_case
    return _run(c["calls"], c["S"], c["N"], dev, 0, W=c["W"])


@pytest.mark.parametrize("n_sample", [1, 16, 64, 256])
def test_window_mode_bit_exact(dev, window_case, window_off, n_sample):
    c = window_case
    cf, cv, ci = c["cand"]
    assert (cf == 256).sum() == 240 and (cf == 0).sum() > 0 and ci.min() >= 2 ** 33 * 6
    exp = sref.sample_tables(cf, cv, ci, c["N"], n_sample, SEED)
    st = _run(c["calls"], c["S"], c["N"], dev, n_sample, W=c["W"])
    _assert_sample(_sample(st), exp)
    _assert_rest_equal(st, window_off)
    assert int(st.seg_count[256]) == 240
    assert int((st.smp_id[256] >= 0).sum()) == min(n_sample, 240)
    frac = st.sample_fraction().cpu().numpy()
    assert np.array_equal(frac, np.minimum(1.0, n_sample / np.maximum(exp[0], 1).astype(np.float64)))
    ids, vals = st.sample_examples(256)
    assert np.array_equal(ids.numpy(), exp[2][256][exp[2][256] >= 0]) and len(vals) == len(ids)


def test_image_mode_bit_exact_with_cancelling_sums(dev):
    """S = 12, P = 8, N = 64, k = 4, 300 rows in calls of 100; signed values on a grid of 1/4: some pooled sums are exactly 0
    and are not candidates."""
    rng = np.random.default_rng(32)
    S, P, N, k, rows = 12, 8, 64, 4, 300
    vals, idx = _topk(rng, rows * S, k, N, lo=-3, hi=4, step=0.25)
    calls = [(vals[a * S:(a + 100) * S], idx[a * S:(a + 100) * S], 1000 + a) for a in (0, 100, 200)]
    cf, cv, ci = _candidates(calls, S, N, "image", P=P)
    # rows whose pooled sum cancels: the feature fired at s < P but is no candidate
    b, s, f, v = ref.records(vals, idx, S, N=N)
    fired = len(set(zip(f[s < P].tolist(), b[s < P].tolist())))
    assert fired - len(cf) > 20
    off = _run(calls, S, N, dev, 0, mode="image", P=P)
    for n_sample in (16, 64):
        exp = sref.sample_tables(cf, cv, ci, N, n_sample, SEED)
        assert exp[0].max() > 64
        st = _run(calls, S, N, dev, n_sample, mode="image", P=P)
        _assert_sample(_sample(st), exp)
        _assert_rest_equal(st, off)


def test_chunk_and_order_invariance(dev, window_case):
    """The same rows in calls of 1, 3 and 8 rows, and the 8-row calls in reverse order: bit-identical samples."""
    c = window_case
    S, N, W = c["S"], c["N"], c["W"]
    vals = np.concatenate([x[0] for x in c["calls"]])[:24 * S]
    idx = np.concatenate([x[1] for x in c["calls"]])[:24 * S]
    outs = []
    for per, rev in ((1, False), (3, False), (8, False), (8, True)):
        calls = [(vals[r * S:(r + per) * S], idx[r * S:(r + per) * S], 2 ** 33 + r) for r in range(0, 24, per)]
        outs.append(_run(calls[::-1] if rev else calls, S, N, dev, 16, W=W))
    exp = sref.sample_tables(*_candidates(calls, S, N, "window", W=W), N, 16, SEED)
    _assert_sample(_sample(outs[0]), exp)
    for o in outs[1:]:
        _assert_sample(_sample(o), _sample(outs[0]))
        _assert_rest_equal(o, outs[0])


def test_prefix_property_on_the_device(dev, window_case):
    c = window_case
    a = _sample(_run(c["calls"], c["S"], c["N"], dev, 16, W=c["W"]))
    b = _sample(_run(c["calls"], c["S"], c["N"], dev, 64, W=c["W"]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2][:, :16])
    assert np.array_equal(a[1].view(np.uint32), b[1][:, :16].view(np.uint32))
    assert (b[2][:, 16:] >= 0).sum() > 100


def test_merge_both_ways_equals_one_state(dev, window_case):
    c = window_case
    S, N, W = c["S"], c["N"], c["W"]
    for n_sample in (16, 256):
        whole = _run(c["calls"], S, N, dev, n_sample, W=W)
        ab = _run(c["calls"][:1], S, N, dev, n_sample, W=W).merge(_run(c["calls"][1:], S, N, dev, n_sample, W=W))
        ba = _run(c["calls"][1:], S, N, dev, n_sample, W=W).merge(_run(c["calls"][:1], S, N, dev, n_sample, W=W))
        for m in (ab, ba):
            _assert_sample(_sample(m), _sample(whole))
            _assert_rest_equal(m, whole)
        _assert_sample(_sample(whole), sref.sample_tables(*c["cand"], N, n_sample, SEED))
    # an empty source and an empty destination
    empty = _run([], S, N, dev, 16, W=W)
    full = _run(c["calls"], S, N, dev, 16, W=W)
    _assert_sample(_sample(_run(c["calls"], S, N, dev, 16, W=W).merge(empty)), _sample(full))
    _assert_sample(_sample(empty.merge(full)), _sample(full))


def _feature_cache(cache, width):
    """A FeatureCache around a filled Cache, without a model: save_splits / concate_safetensors only use these two."""
    from msae.features import FeatureCache

    fc = FeatureCache.__new__(FeatureCache)
    fc.cache, fc.width = cache, width
    return fc


def _rank_worker(rank, world, out_dir, S, N, k, W):
    from msae.features import Cache

    dev = torch.device("cuda:0")
    vals, idx = _topk(np.random.default_rng(33), 8 * S, k, N, hot=5)
    rows_per = 8 // world
    cache = Cache(rank * rows_per, None, batch_size=2, stats=dict(pool="window", window=W, n_sample=16, sample_seed=7))
    for b in range(rows_per // 2):
        r0 = rank * rows_per + 2 * b
        cache.add_topk(torch.from_numpy(vals[r0 * S:(r0 + 2) * S]).to(dev).view(2, S, k),
                       torch.from_numpy(idx[r0 * S:(r0 + 2) * S]).to(dev).view(2, S, k), N, b, "m")
    cache.save()
    _feature_cache(cache, N).save_splits(2, out_dir, rank)


def test_two_ranks_through_save_splits_and_merge_rank_stats(dev, tmp_path):
    from msae.features import FeatureStats
    from msae.features.cache import merge_rank_stats

    S, N, k, W = 4 * 8 + 3, 300, 8, 8
    mp.spawn(_rank_worker, args=(2, str(tmp_path / "two"), S, N, k, W), nprocs=2, join=True)
    merged = merge_rank_stats(str(tmp_path / "two" / "m"), dev)
    assert "Rank0_feature_stats.safetensors" not in os.listdir(tmp_path / "two" / "m")
    _rank_worker(0, 1, str(tmp_path / "one"), S, N, k, W)
    one = FeatureStats.load(str(tmp_path / "one" / "m" / "Rank0_feature_stats.safetensors"))
    two = FeatureStats.load(merged)
    assert (two.n_sample, two.sample_seed) == (16, 7) and two.metadata() == one.metadata()
    _assert_sample(_sample(two), _sample(one))
    _assert_rest_equal(two, one)
    vals, idx = _topk(np.random.default_rng(33), 8 * S, k, N, hot=5)
    exp = sref.sample_tables(*_candidates([(vals, idx, 0)], S, N, "window", W=W), N, 16, 7)
    _assert_sample(_sample(one), exp)
    assert int(one.seg_count[5]) == 8 * 4


def test_end_to_end_cache(dev, tmp_path):
    """A small Sae under Cache(stats=dict(..., n_sample=64)), two batches of 4 x 256 tokens: the split files are
    byte-identical to a run without the sample, and the saved sample is the restatement of the saved, unfiltered records."""
    from msae import Sae, SaeConfig
    from msae.features import Cache, FeatureStats

    d, N, k, B, S, W = 128, 8192, 8, 4, 256, 64
    torch.manual_seed(6)
    sae = Sae(d, SaeConfig(num_latents=N, k=k), device=dev)
    xs = [torch.randn(B * S, d, device=dev).to(torch.bfloat16) for _ in range(2)]
    files = {}
    for n_sample in (0, 64):
        cache = Cache(0, None, batch_size=B, stats=dict(pool="window", window=W, n_sample=n_sample))
        for batch, x in enumerate(xs):
            with torch.no_grad():
                top = sae.encode(x)
            cache.add_topk(top.top_acts.view(B, S, k), top.top_indices.view(B, S, k), N, batch, "m")
        cache.save()
        out = tmp_path / str(n_sample)
        _feature_cache(cache, N).save_splits(2, str(out), 0, include_split_end=True)
        files[n_sample] = out / "m"
        if n_sample:
            loc, act = cache.feature_locations["m"].numpy(), cache.feature_activations["m"].numpy()
    names = sorted(os.listdir(files[0]))
    assert names == sorted(os.listdir(files[64])) and len(names) == 3
    for f in names:
        if f != "Rank0_feature_stats.safetensors":
            assert (files[0] / f).read_bytes() == (files[64] / f).read_bytes(), f
    st = FeatureStats.load(str(files[64] / "Rank0_feature_stats.safetensors"))
    off = FeatureStats.load(str(files[0] / "Rank0_feature_stats.safetensors"))
    assert st.n_sample == 64 and off.n_sample == 0
    _assert_rest_equal(st, off)
    cf, cv, ci = ref.candidates(loc[:, 0], loc[:, 1], loc[:, 2], act, S, "window", 0, W=W)
    _assert_sample(_sample(st), sref.sample_tables(cf, cv, ci, N, 64, 22))
    assert len(cf) > 1000


def test_argument_errors_empty_call_and_no_sync(dev):
    from msae import _hip
    from msae.features import FeatureStats
    from msae.features.stats import feature_stats_update_sampled

    rng = np.random.default_rng(34)
    N, k, S, W = 512, 8, 40, 8
    vals, idx = _topk(rng, 4 * S, k, N)
    v, i = torch.from_numpy(vals).to(dev).view(4, S, k), torch.from_numpy(idx).to(dev).view(4, S, k)
    st = FeatureStats(N, pool="window", window=W, device=dev, n_sample=16)
    st.update(v, i, 0)                               # first call: library load, workspace
    before = [t.clone() for t in (st.count, st.top_id, st.seg_count, st.smp_val, st.smp_id)]
    lib = _hip.load()
    i32 = i.to(torch.int32)
    ws = torch.empty(lib.msae_feature_stats_ws_bytes(4 * S, k, N), dtype=torch.uint8, device=dev)

    def call(n_sample, size, seg, sv, si):
        sm = _hip.MsaeFeatureSample(size, n_sample, 22, seg, sv, si)
        return lib.msae_feature_stats_update_sampled(
            _hip.ptr(v), _hip.ptr(i32), 4, S, k, 1e-5, N, 1, 576, W, 4, 64, _hip.ptr(st.count),
            _hip.ptr(st.act_max), _hip.ptr(st.act_sum), _hip.ptr(st.top_val), _hip.ptr(st.top_id), ctypes.byref(sm),
            _hip.ptr(ws), ws.numel(), _hip.stream_of(v))

    p = (st.seg_count.data_ptr(), st.smp_val.data_ptr(), st.smp_id.data_ptr())
    for bad in ((0, 40) + p, (257, 40) + p, (-1, 40) + p, (16, 8) + p, (16, 40, None, p[1], p[2]), (16, 40, p[0], None, p[2]),
                (16, 40, p[0], p[1], None)):
        assert call(*bad) == -1, bad
    assert lib.msae_feature_sample_merge(N, 0, 22, *[_hip.ptr(t) for t in before[2:]] * 2, None) == -1
    assert lib.msae_feature_sample_merge(N, 257, 22, *[_hip.ptr(t) for t in before[2:]] * 2, None) == -1
    with pytest.raises(RuntimeError):                 # through the op: tables wider than 256
        feature_stats_update_sampled(v, i, 4, 1e-5, 1, 576, W, st.count, st.act_max, st.act_sum, st.top_val, st.top_id, 22,
                                     st.seg_count, torch.zeros(N, 300, device=dev),
                                     torch.full((N, 300), -1, dtype=torch.int64, device=dev))
    st.update(v[:0], i[:0], 4)                        # B * S = 0: a no-op
    torch.cuda.synchronize()
    for t, b in zip((st.count, st.top_id, st.seg_count, st.smp_val, st.smp_id), before):
        assert torch.equal(t, b)                      # nothing was launched by any of the above
    torch.cuda.set_sync_debug_mode("error")
    try:
        st.update(v, i, 4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    exp = sref.sample_tables(*_candidates([(vals, idx, 0), (vals, idx, 4)], S, N, "window", W=W), N, 16, SEED)
    _assert_sample(_sample(st), exp)
