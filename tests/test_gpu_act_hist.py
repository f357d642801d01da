"""GPU: activation histograms and quantile bins (msae_act_hist_*, ActHist) against the numpy restatement in act_hist_ref.py.
Everything is integer counting plus one IEEE f64 multiply: every comparison is array_equal; there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import act_hist_ref as ref
import fakes
import synth

pytestmark = pytest.mark.gpu

N_C2, T_C2, K_C2 = 131072, 8192, 32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _topk(rng, B, S, k, N, reserved=(), positive=False):
    """[B, S, k] pairs: a token's indices distinct and outside `reserved`; values over 2^-18 .. 2^17 (both ends of the
    default bins clamp), some exactly 0, some negative (unless `positive`)."""
    pool = np.setdiff1d(np.arange(N), np.asarray(reserved, np.int64))
    idx = np.stack([rng.choice(pool, size=k, replace=False) for _ in range(B * S)]).reshape(B, S, k).astype(np.int64)
    vals = np.exp2(rng.uniform(-18, 17, size=(B, S, k))).astype(np.float32)
    if not positive:
        u = rng.uniform(size=(B, S, k))
        vals[u < 0.05] = 0.0
        vals[u > 0.95] *= -1.0
    return vals, idx


def _run(calls, pool, N, dev, index_dtype=torch.int64, value_dtype=None, **kw):
    from msae.features import ActHist

    st = ActHist(N, pool=pool, device=dev, **kw)
    for vals, idx in calls:
        v = torch.from_numpy(vals).to(dev)
        st.update(v if value_dtype is None else v.to(value_dtype), torch.from_numpy(idx).to(dev).to(index_dtype))
    return st


def _ref(calls, pool, N, **kw):
    names = dict(pool_len="P", window="W", sub_bits="s", e_lo="e_lo", octaves="E", thresh="thresh")
    return ref.run(calls, pool, N, **{names[k]: v for k, v in kw.items()})


def _assert_state(st, exp):
    assert st.hist.dtype == torch.int32 and st.hist.shape == exp[0].shape
    assert np.array_equal(st.hist.cpu().numpy(), exp[0])
    assert st.n_segments == exp[1]


# ---- token pool: special values ---------------------------------------------------------------------------------------
def _specials():
    e = ref.edges()
    on = e[[0, 1, 8, 127, 128, 129, 255, 256]]                     # octave and sub-bin edges; e[256] = 2^16 clamps
    below = np.nextafter(on, np.float32(0))
    other = np.array([1.2e-5,                                      # in (thresh, 2^e_lo)
                      1e-40,                                       # a subnormal (below thresh: dropped)
                      1e-5,                                        # exactly thresh: dropped (the rule is >)
                      1e6, np.inf, np.nan, -2.0], np.float32)
    return np.concatenate([on, below, other]).astype(np.float32)


def _case_special(k, bf16=False):
    """B = 3, S = 37, N = 4096.  Special value i sits alone on feature 3000 + i, in slot i % k of token 2 i; indices -1 and N
    carry ordinary values; with k >= 2 feature 2990 is named twice by token 100 (it counts twice)."""
    rng = np.random.default_rng(20 + k)
    B, S, N = 3, 37, 4096
    vals, idx = _topk(rng, B, S, k, N, reserved=np.arange(2990, 3100))
    sp = _specials()
    v2, i2 = vals.reshape(B * S, k), idx.reshape(B * S, k)
    for i, x in enumerate(sp):
        v2[2 * i, i % k], i2[2 * i, i % k] = x, 3000 + i
    v2[81, 0], i2[81, 0] = 1.0, -1
    v2[83, k - 1], i2[83, k - 1] = 1.0, N
    if k >= 2:
        v2[100, 0], i2[100, 0], v2[100, k - 1], i2[100, k - 1] = 1.0, 2990, 3.0, 2990
    if bf16:
        vals = torch.from_numpy(vals).to(torch.bfloat16).to(torch.float32).numpy()
    return vals, idx, N, len(sp)


@pytest.mark.parametrize("k", [1, 32, 37, 256])
@pytest.mark.parametrize("variant", ["int32", "int64", "bf16"])
def test_token_pool_special_values(dev, k, variant):
    vals, idx, N, n_sp = _case_special(k, bf16=variant == "bf16")
    exp = _ref([(vals, idx)], "token", N)
    st = _run([(vals, idx)], "token", N, dev, index_dtype=torch.int32 if variant == "int32" else torch.int64,
              value_dtype=torch.bfloat16 if variant == "bf16" else None)
    _assert_state(st, exp)
    assert exp[1] == 3 * 37
    h = exp[0]
    if variant != "bf16":
        # on the edges 0, 1, 8, 127, 128, 129, 255 and 2^16; one below each; the rest
        assert [int(np.flatnonzero(h[3000 + i])[0]) for i in range(8)] == [0, 1, 8, 127, 128, 129, 255, 255]
        assert [int(np.flatnonzero(h[3008 + i])[0]) for i in range(1, 8)] == [0, 7, 126, 127, 128, 254, 255]
        assert h[3008].sum() == 1 and h[3008, 0] == 1              # below 2^-16 but above thresh: bin 0
        assert h[3016, 0] == 1                                     # 1.2e-5
        assert h[3017].sum() == 0 and h[3018].sum() == 0           # the subnormal and thresh itself are dropped
        assert h[3019, 255] == 1 and h[3020, 255] == 1             # 1e6 and +inf
        assert h[3021].sum() == 0 and h[3022].sum() == 0           # NaN and a negative count nowhere
    assert h[3000:3000 + n_sp].sum(axis=1).max() == 1
    if k >= 2:
        assert h[2990].sum() == 2 and h[2990, 128] == 1            # the repeat counts twice


# ---- window and image pool -------------------------------------------------------------------------------------------
def test_window_pool_full_window_and_ragged_tail(dev):
    """S = 150, W = 64: feature 70 fills window 1 of row 0; 71 fires only in the tail (positions >= 128: counts nothing);
    72 fills a window with negative values (pooled < 0); 73 is negative on part of a window (pooled = 0)."""
    rng = np.random.default_rng(31)
    B, S, k, N, W = 3, 150, 16, 4096, 64
    vals, idx = _topk(rng, B, S, k, N, reserved=(70, 71, 72, 73))
    idx[0, 64:128, 2], vals[0, 64:128, 2] = 70, np.exp2(rng.uniform(-3, 3, size=64)).astype(np.float32)
    idx[:, 128:, 3], vals[:, 128:, 3] = 71, 2.0
    idx[1, 0:64, 4], vals[1, 0:64, 4] = 72, -1.5
    idx[2, 70:90, 5], vals[2, 70:90, 5] = 73, -0.5
    exp = _ref([(vals, idx)], "window", N, window=W)
    _assert_state(_run([(vals, idx)], "window", N, dev, window=W), exp)
    h = exp[0]
    assert exp[1] == B * 2 and h[70].sum() == 1 and h[70, ref.bins_of(vals[0, 64:128, 2].max()[None])[0]] == 1
    assert h[71].sum() == 0 and h[72].sum() == 0 and h[73].sum() == 0 and h.sum() > 1000


def test_image_pool_tail_and_summation_order(dev):
    """S = 40, pool_len = 24: feature 60 fires only at s >= 24 (counts nothing).  Feature 61 of row 1 has the summands
    24576 - 2^-9, 2^-11, 2^-11 at ascending positions: added in that order the small ones vanish one by one and the mean
    stays below the bin edge 1024; added small-first they reach 24576 and the mean is 1024, one bin up."""
    rng = np.random.default_rng(32)
    B, S, k, N, P = 3, 40, 16, 4096, 24
    vals, idx = _topk(rng, B, S, k, N, reserved=(60, 61))
    idx[:, 24:, 1], vals[:, 24:, 1] = 60, 3.0
    a, t = np.float32(24576.0) - np.float32(2.0 ** -9), np.float32(2.0 ** -11)
    for s, x in ((3, a), (10, t), (20, t)):
        idx[1, s, 6], vals[1, s, 6] = 61, x
    fwd = np.float32(np.float32(np.float32(a + t) + t) / np.float32(P))
    rev = np.float32(np.float32(np.float32(t + t) + a) / np.float32(P))
    b_fwd, b_rev = int(ref.bins_of(fwd[None])[0]), int(ref.bins_of(rev[None])[0])
    assert rev == 1024.0 and fwd < 1024.0 and b_rev == b_fwd + 1
    exp = _ref([(vals, idx)], "image", N, pool_len=P)
    _assert_state(_run([(vals, idx)], "image", N, dev, pool_len=P), exp)
    h = exp[0]
    assert exp[1] == B and h[60].sum() == 0 and h[61].sum() == 1 and h[61, b_fwd] == 1 and h.sum() > 500


@pytest.mark.parametrize("bins", [dict(sub_bits=0, e_lo=-4, octaves=8), dict(sub_bits=4, e_lo=-16, octaves=32),
                                  dict(sub_bits=2, e_lo=-1, octaves=2), dict(sub_bits=3, e_lo=-126, octaves=60, thresh=0.0)])
@pytest.mark.parametrize("pool", ["token", "window", "image"])
def test_other_bins(dev, bins, pool):
    """1 and 16 bins per octave, 512 bins, a range of two octaves that clamps at both ends, and -- with thresh = 0 -- a
    lowest octave at the bottom of the normal range, where a subnormal lands in bin 0."""
    rng = np.random.default_rng(33)
    B, S, k, N = 3, 50, 8, 1001
    vals, idx = _topk(rng, B, S, k, N, reserved=(5,))
    idx[0, 2, 0], vals[0, 2, 0] = 5, 1e-40
    kw = dict(bins, pool_len=30, window=16)
    exp = _ref([(vals, idx)], pool, N, **kw)
    st = _run([(vals, idx)], pool, N, dev, **kw)
    _assert_state(st, exp)
    assert st.n_bins == bins["octaves"] << bins["sub_bits"] and exp[0][:, 0].sum() > 0
    assert exp[0][:, -1].sum() > 0 or pool == "image"            # a mean over 30 positions does not reach 2^16
    assert np.array_equal(st.edges().cpu().numpy().view(np.uint32),
                          ref.edges(bins["sub_bits"], bins["e_lo"], bins["octaves"]).view(np.uint32))
    if bins.get("thresh") == 0.0 and pool == "token":
        assert exp[0][5, 0] == 1


# ---- cuts, merges, chunks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ["token", "window", "image"])
def test_cut_and_merge_invariance(dev, pool):
    rng = np.random.default_rng(34)
    B, S, k, N = 9, 70, 32, 2048
    vals, idx = _topk(rng, B, S, k, N)
    kw = dict(pool_len=48, window=16)
    one = _run([(vals, idx)], pool, N, dev, **kw)
    cuts = [(vals[5:], idx[5:]), (vals[:2], idx[:2]), (vals[2:5], idx[2:5])]
    three = _run(cuts, pool, N, dev, **kw)
    assert torch.equal(one.hist, three.hist) and one.n_segments == three.n_segments
    a, b = _run(cuts[:1], pool, N, dev, **kw), _run(cuts[1:], pool, N, dev, **kw)
    assert a.merge(b) is a and torch.equal(one.hist, a.hist) and one.n_segments == a.n_segments
    _assert_state(one, _ref([(vals, idx)], pool, N, **kw))


def test_update_chunks_at_the_call_envelope(dev):
    """B * S = 65920 > 65536 in ONE update (1024 rows, then 6): the same bits as three calls of whole rows."""
    rng = np.random.default_rng(35)
    B, S, k, N, W = 1030, 64, 2, 512, 16
    idx = rng.integers(0, N, size=(B, S, k)).astype(np.int64)
    vals = np.exp2(rng.uniform(-6, 6, size=(B, S, k))).astype(np.float32)
    one = _run([(vals, idx)], "window", N, dev, window=W)
    three = _run([(vals[:300], idx[:300]), (vals[300:301], idx[300:301]), (vals[301:], idx[301:])], "window", N, dev, window=W)
    assert torch.equal(one.hist, three.hist) and one.n_segments == three.n_segments == B * 4
    _assert_state(one, _ref([(vals, idx)], "window", N, window=W))


def test_contention_one_feature_one_value_on_every_token(dev):
    rng = np.random.default_rng(36)
    B, S, k, N = 32, 256, 32, 4096
    vals, idx = _topk(rng, B, S, k, N, reserved=(7,), positive=True)
    idx[:, :, 11], vals[:, :, 11] = 7, 1.5
    st = _run([(vals, idx)], "token", N, dev)
    assert int(st.hist[7, 132]) == B * S and int(st.hist[7].sum()) == B * S          # 1.5 = edge(132)
    _assert_state(st, _ref([(vals, idx)], "token", N))


def _c2_pairs():
    """[8192, 32] pairs at N = 131072 from synth's counter-based streams: feature ids concentrated on the low ids (a cube
    law, so features recur; a token may repeat one -- the token pool counts it twice), positive values."""
    u = np.abs(synth.normalish(77, T_C2 * K_C2)) / np.float32(3.47)
    idx = np.minimum((u.astype(np.float64) ** 3 * N_C2).astype(np.int64), N_C2 - 1).reshape(T_C2, K_C2)
    vals = (np.abs(synth.normalish(78, T_C2 * K_C2)) + np.float32(0.01)).reshape(T_C2, K_C2)
    return vals, idx


@pytest.fixture(scope="module")
def c2_pairs():
    return _c2_pairs()


@pytest.fixture(scope="module")
def c2_token(dev, c2_pairs):
    """(the state after the production-width token update, the restatement's) -- computed once, read by two tests."""
    vals, idx = c2_pairs
    calls = [(vals.reshape(4, 2048, K_C2), idx.reshape(4, 2048, K_C2))]
    return _run(calls, "token", N_C2, dev), _ref(calls, "token", N_C2)


def test_production_width_token(c2_token):
    st, exp = c2_token
    _assert_state(st, exp)
    assert exp[0].sum() == T_C2 * K_C2 and exp[1] == T_C2 and (exp[0].sum(axis=1) > 0).sum() > 20000


def test_production_width_image(dev, c2_pairs):
    vals, idx = (a[:5760].reshape(2, 2880, K_C2) for a in c2_pairs)
    exp = _ref([(vals, idx)], "image", N_C2, pool_len=576)
    _assert_state(_run([(vals, idx)], "image", N_C2, dev, pool_len=576), exp)
    assert exp[1] == 2 and exp[0].sum() > 5000


# ---- against the feature statistics' kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("pool,S", [("window", 150), ("image", 40)])
def test_agrees_with_the_feature_statistics(dev, pool, S):
    """The same positive [B, S, k] input into ActHist and FeatureStats: a feature's counted values are its nonzero pooled
    segments (seg_count), and its highest non-empty bin is the bin of its best example (top_val[f, 0])."""
    from msae.features import FeatureStats

    rng = np.random.default_rng(37)
    B, k, N = 4, 16, 2048
    vals, idx = _topk(rng, B, S, k, N, positive=True)
    kw = dict(pool_len=24, window=64)
    st = _run([(vals, idx)], pool, N, dev, **kw)
    fs = FeatureStats(N, pool=pool, device=dev, n_sample=1, **kw)
    fs.update(torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev), 0)
    fired = st.fired().cpu().numpy()
    assert np.array_equal(fired, fs.seg_count.cpu().numpy()) and (fired > 0).sum() > 500
    h = st.hist.cpu().numpy()
    top = fs.top_val[:, 0].cpu().numpy()
    on = fired > 0
    highest = h.shape[1] - 1 - np.argmax(h[:, ::-1] > 0, axis=1)
    assert (top[on] > 0).all() and np.array_equal(highest[on], ref.bins_of(top[on]))


def _case_shared_walk():
    """B = 2, S = 150, k = 4, N = 37 for window 64 (two full windows and a ragged tail of 22) and pool_len 40.  Features
    0 .. 19 are background (a token's four distinct, values +-2^[-6, 6): f32 sums depend on their order, f64 sums are exact in
    any order); 20 .. 27 are planted, each in slots of its own:
      20  a NaN (dropped) and one ordinary entry          21  -0.0 (dropped) and one negative entry
      22  |v| = thresh and below (dropped), one just above  23  (row 1, s = 10) names it twice; also s = 12 and s = 45
      24  row 0: all 64 positions of window 0, negative (cnt == W: the candidate stays negative); 63 positions of window 1,
          negative (the implicit 0 wins); so it also lies on both sides of s = 40
      25  only in the ragged tail (s >= 128)              26  s = 38 .. 41: both sides of pool_len
      27  all of window 1 of row 1, positive
    and two background slots carry the indices -1 and N."""
    rng = np.random.default_rng(42)
    B, S, k, N = 2, 150, 4, 37
    idx = np.stack([rng.choice(20, size=k, replace=False) for _ in range(B * S)]).reshape(B, S, k).astype(np.int64)
    vals = np.exp2(rng.uniform(-6, 6, size=(B, S, k))).astype(np.float32)
    vals[rng.uniform(size=(B, S, k)) < 0.2] *= -1.0
    plant = [((0, 5, 0), 20, np.nan), ((1, 3, 1), 20, 0.75), ((0, 6, 1), 21, -0.0), ((1, 4, 1), 21, -0.5),
             ((0, 7, 0), 22, 1e-5), ((0, 8, 0), 22, 5e-6), ((0, 9, 0), 22, 1.25e-5),
             ((1, 10, 0), 23, 1.5), ((1, 10, 3), 23, 2.25), ((1, 12, 0), 23, -3.0), ((1, 45, 0), 23, 0.625),
             ((0, 20, 1), -1, 1.0), ((1, 70, 2), N, 1.0)]
    plant += [((0, s, 2), 24, -(1.0 + s / 64.0)) for s in range(64)]
    plant += [((0, s, 2), 24, -0.5) for s in range(64, 128) if s != 100]
    plant += [((b, s, 1), 25, 2.0 + b + s / 256.0) for b in range(B) for s in range(130, 141)]
    plant += [((1, s, 0), 26, x) for s, x in ((38, 3.0), (39, 2.0 ** -10), (40, 5.0), (41, -7.0))]
    plant += [((1, s, 3), 27, x) for s, x in zip(range(64, 128), np.exp2(rng.uniform(-3, 3, size=64)))]
    for at, f, x in plant:
        idx[at], vals[at] = f, np.float32(x)
    assert np.signbit(vals[0, 6, 1]) and vals[0, 6, 1] == 0 and vals[0, 7, 0] == np.float32(1e-5)
    return vals, idx, N


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_shared_walk_special_values(dev, index_dtype):
    """Every branch of the walk over a sorted (feature, row, group) run, on the planted input of `_case_shared_walk`:
    FeatureStats bit for bit against feature_stats_ref.py (count, act_max, act_sum, top tables), ActHist bit for bit against
    act_hist_ref.py, and the histogram's row totals equal to the positive candidates the statistics' restatement forms."""
    import feature_stats_ref as fs_ref
    from msae.features import FeatureStats

    vals, idx, N = _case_shared_walk()
    B, S, k = vals.shape
    W, P, row_base, n_top = 64, 40, 11, 64
    v, i = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev).to(index_dtype)
    with np.errstate(invalid="ignore"):
        rb, rs, rf, rv = fs_ref.records(vals.reshape(B * S, k), idx.reshape(B * S, k), S, N=N)
    count, mx, sm = fs_ref.basic_stats(rf, rv, N)
    assert count[24] == 127 and mx[24] == -0.5 and count[23] == 4 and count[25] == 22 and count[22] == 1
    for pool in ("window", "image"):
        cf, cv, ci = fs_ref.candidates(rb, rs, rf, rv, S, pool, row_base, P=P, W=W)
        tv, ti = fs_ref.top_tables(cf, cv, ci, N, n_top)
        fs = FeatureStats(N, n_top=n_top, pool=pool, pool_len=P, window=W, device=dev)
        fs.update(v, i, row_base)
        assert np.array_equal(fs.count.cpu().numpy(), count)
        assert np.array_equal(fs.act_max.cpu().numpy().view(np.uint32), mx.view(np.uint32))
        assert np.array_equal(fs.act_sum.cpu().numpy().view(np.uint64), sm.view(np.uint64))
        assert np.array_equal(fs.top_id.cpu().numpy(), ti)
        assert np.array_equal(fs.top_val.cpu().numpy().view(np.uint32), tv.view(np.uint32))
        exp = _ref([(vals, idx)], pool, N, pool_len=P, window=W)
        st = _run([(vals, idx)], pool, N, dev, index_dtype=index_dtype, pool_len=P, window=W)
        _assert_state(st, exp)
        positive = np.bincount(cf[cv > 0], minlength=N)
        assert np.array_equal(st.fired().cpu().numpy(), positive) and positive.sum() > 20
        assert positive[25] == 0 and 25 not in cf                  # the ragged tail / s >= pool_len: no candidate
        if pool == "window":
            # window 0 of row 0 holds 24 on every position: the negative maximum stands; window 1 misses one: no candidate
            assert cv[cf == 24].tolist() == [-1.0] and ci[cf == 24].tolist() == [row_base * 2] and positive[24] == 0
            assert positive[27] == 1 and positive[23] == 1 and cv[cf == 23].tolist() == [2.25]
            assert positive[20] == 1 and positive[21] == 0 and positive[22] == 1
        else:
            assert positive[24] == 0 and (cv[cf == 24] < 0).all() and positive[27] == 0
            s26 = np.float32(np.float32(3.0) + np.float32(2.0 ** -10))
            assert cv[cf == 26].tolist() == [s26 / np.float32(P)] and cv[cf == 23].tolist() == [np.float32(0.75) / np.float32(P)]


# ---- quantiles -------------------------------------------------------------------------------------------------------
def _planted_hist(rng, N, n_bins):
    hist = (rng.integers(0, 30, size=(N, n_bins)) * (rng.uniform(size=(N, n_bins)) < 0.3)).astype(np.int32)
    hist[np.arange(N), rng.integers(0, n_bins, size=N)] += 1       # no empty row but the planted one
    hist[0] = 0                                                    # an empty row
    hist[1] = 0; hist[1, n_bins // 2] = 1                          # a single count
    hist[2] = 0; hist[2, n_bins - 1] = 1
    hist[3] = 0; hist[3, 0] = 1
    hist[4, 0], hist[4, n_bins // 3], hist[4, n_bins - 1] = (1 << 24) + 1, 3, 1 << 30       # counts beyond a float's integers
    hist[5] = 0; hist[5, 0] = hist[5, n_bins - 1] = (1 << 31) - 1
    hist[N - 1] = 1
    return hist


@pytest.mark.parametrize("bins", [dict(), dict(sub_bits=4), dict(sub_bits=2, e_lo=-1, octaves=2), dict(sub_bits=0, e_lo=0, octaves=1),
                                  dict(sub_bits=3, e_lo=-2, octaves=5), dict(sub_bits=0, e_lo=-40, octaves=65)])
def test_quantile_kernel(dev, bins):
    """256, 512, 8, 1, 40 and 65 bins (one to eight per lane, rows that end inside a lane's share); Q = 1, 7, 64; with and
    without the zeros; the device kernel, the restatement and the CPU path agree."""
    from msae.features import ActHist

    rng = np.random.default_rng(38)
    N = 1003
    st = ActHist(N, device=dev, **bins)
    hist = _planted_hist(rng, N, st.n_bins)
    st.hist.copy_(torch.from_numpy(hist))
    host = ActHist(N, **bins)
    host.hist.copy_(torch.from_numpy(hist))
    for Q in (1, 7, 64):
        qs = [0.5] if Q == 1 else [0.0, 1.0] + np.sort(rng.uniform(0, 1, size=Q - 2)).tolist()
        for zeros, n_seg in ((False, 0), (False, 12345), (True, 0), (True, 4000), (True, (1 << 31) - 1)):
            st.n_segments = host.n_segments = n_seg
            got = st.quantile_bins(qs, zeros=zeros)
            assert got.dtype == torch.int32 and got.shape == (N, Q) and got.device == st.device
            exp = ref.quantile_bins(hist, qs, n_seg, zeros)
            assert np.array_equal(got.cpu().numpy(), exp), (Q, zeros, n_seg)
            assert np.array_equal(host.quantile_bins(qs, zeros=zeros).numpy(), exp)
            if zeros and n_seg:
                assert (exp == -1).any() and (exp >= 0).any()
            else:
                assert (exp[0] == -2).all() and (exp[1:] >= 0).all()
    st.n_segments = host.n_segments = 4000
    val = st.quantile([0.1, 0.9], zeros=True)
    assert torch.equal(val.cpu().view(torch.int32), host.quantile([0.1, 0.9], zeros=True).view(torch.int32))
    assert np.array_equal(val.cpu().numpy().view(np.uint32),
                          ref.quantile(hist, [0.1, 0.9], 4000, True, st.sub_bits, st.e_lo, st.octaves).view(np.uint32))


def test_quantiles_at_production_width(c2_token):
    """All 131072 rows through the kernel; the hot low ids and every 37th row against the restatement."""
    st, exp = c2_token
    qs = [0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99]
    rows = np.unique(np.concatenate([np.arange(4096), np.arange(0, N_C2, 37), [N_C2 - 1]]))
    for zeros in (False, True):
        got = st.quantile_bins(qs, zeros=zeros)
        assert got.shape == (N_C2, len(qs))
        assert np.array_equal(got.cpu().numpy()[rows], ref.quantile_bins(exp[0][rows], qs, T_C2, zeros))


# ---- no host synchronisation ---------------------------------------------------------------------------------------
def test_no_host_sync_and_no_allocation_growth(dev):
    rng = np.random.default_rng(39)
    B, S, k, N = 4, 96, 32, 4096
    vals, idx = _topk(rng, B, S, k, N)
    v, i = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev)
    from msae.features import ActHist

    qs = [0.1, 0.5, 0.9]
    for pool in ("token", "window", "image"):
        st = ActHist(N, pool=pool, pool_len=64, window=32, device=dev)
        st.update(v, i)                                     # first call: library load, workspace, the probabilities
        st.quantile(qs, zeros=True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_reserved(dev)
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(3):
                st.update(v, i)
            bins = st.quantile_bins(qs, zeros=True)
            val = st.quantile(qs, zeros=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.cuda.memory_reserved(dev) == before
        exp = _ref([(vals, idx)] * 4, pool, N, pool_len=64, window=32)
        _assert_state(st, exp)
        assert np.array_equal(bins.cpu().numpy(), ref.quantile_bins(exp[0], qs, exp[1], True))
        assert np.array_equal(val.cpu().numpy().view(np.uint32), ref.quantile(exp[0], qs, exp[1], True).view(np.uint32))


# ---- the caches ------------------------------------------------------------------------------------------------------
def _spy(cache, seen):
    inner = cache.add_topk

    def spy(top_acts, top_indices, *a, **kw):
        seen.append((top_acts.float().cpu().numpy(), top_indices.cpu().numpy()))
        return inner(top_acts, top_indices, *a, **kw)

    cache.add_topk = spy


def _files(root):
    return {f: (root / f).read_bytes() for f in sorted(os.listdir(root))}


def test_image_cache_end_to_end(dev, tmp_path, golden_dir):
    """A FeatureImageCache run over the fake images with hist on: act_hist.safetensors equals the restatement over every
    batch's top-k; with hist=None the same run writes nothing of it and every other file is byte-identical."""
    from msae import Sae, SaeConfig
    from msae.features import ActHist, FeatureImageCache

    g = np.load(golden_dir / "g9_image_cache.npz")
    images = [{"image": fakes.FakeImage(i)} for i in range(int(g["n_images"]))]
    module, d, N = str(g["module"]), int(g["d"]), 4096
    outs, seen = {}, []
    for on in (False, True):
        torch.manual_seed(11)
        sae = Sae(d, SaeConfig(num_latents=N, k=16), device=dev)
        model = fakes.TinyLlava(vocab=int(g["vocab"]), d=d).to(dev)
        fic = FeatureImageCache(model, None, {module: sae}, batch_size=2, shard_size=0,
                                processor=fakes.FakeProcessor(int(g["vocab"])),
                                hist=dict(pool="image", pool_len=3, sub_bits=2) if on else None)
        if on:
            _spy(fic.cache, seen)
        fic.run(0, images)
        out = tmp_path / ("on" if on else "off")
        fic.save_splits(n_splits=2, save_dir=str(out), rank=0)
        if on:
            assert "Rank0_act_hist.safetensors" in os.listdir(out / module)
        fic.concate_safetensors(n_splits=2, save_dir=str(out))
        outs[on] = _files(out / module)
        assert (fic.cache.act_hists == {}) == (not on)
    assert sorted(outs[True]) == sorted(list(outs[False]) + ["act_hist.safetensors"])
    assert all(outs[True][f] == outs[False][f] for f in outs[False])
    st = ActHist.load(str(tmp_path / "on" / module / "act_hist.safetensors"))
    assert st.pool == "image" and st.pool_len == 3 and st.sub_bits == 2 and st.n_bins == 128 and st.device.type == "cpu"
    assert len(seen) == len(images) // 2
    exp = _ref(seen, "image", N, pool_len=3, sub_bits=2)
    _assert_state(st, exp)
    assert exp[0].sum() > 0 and exp[1] == len(images) // 2 * 2


def test_text_cache_end_to_end(dev, tmp_path):
    """A FeatureCache run over token batches with hist on (token pool): the file equals the restatement."""
    from msae import Sae, SaeConfig
    from msae.features import ActHist, FeatureCache

    d, N, module = 64, 4096, "layers.1"
    torch.manual_seed(12)
    sae = Sae(d, SaeConfig(num_latents=N, k=16), device=dev)
    model = fakes.TinyLlava(vocab=40, d=d).to(dev)
    rng = np.random.default_rng(40)
    dataset = [{"input_ids": torch.from_numpy(rng.integers(0, 40, size=7))} for _ in range(6)]
    fc = FeatureCache(model, None, {module: sae}, batch_size=2, shard_size=0, hist=dict(pool="token"))
    seen = []
    _spy(fc.cache, seen)
    fc.run(7, dataset)
    fc.save_splits(n_splits=2, save_dir=str(tmp_path), rank=0)
    fc.concate_safetensors(n_splits=2, save_dir=str(tmp_path))
    assert "act_hist.safetensors" in os.listdir(tmp_path / module)
    assert not [f for f in os.listdir(tmp_path / module) if f.startswith("Rank")]
    st = ActHist.load(str(tmp_path / module / "act_hist.safetensors"))
    exp = _ref(seen, "token", N)
    _assert_state(st, exp)
    assert len(seen) == 3 and exp[1] == 6 * 7 and exp[0].sum() > 0


def test_two_rank_files_merge_to_the_single_rank_file(dev, tmp_path):
    """The rows split by hand over two ranks, saved as rank files and merged by the cache's concat step: byte-identical to
    the file of one rank that saw every row."""
    from msae.features.cache import merge_rank_act_hist

    rng = np.random.default_rng(41)
    B, S, k, N = 8, 64, 32, 2048
    vals, idx = _topk(rng, B, S, k, N)
    for name, parts in (("two", [(vals[:4], idx[:4]), (vals[4:], idx[4:])]), ("one", [(vals, idx)])):
        os.makedirs(tmp_path / name / "m")
        for r, part in enumerate(parts):
            _run([part], "window", N, dev, window=16).save(str(tmp_path / name / "m" / f"Rank{r}_act_hist.safetensors"))
        assert merge_rank_act_hist(str(tmp_path / name / "m"), dev) == str(tmp_path / name / "m" / "act_hist.safetensors")
        assert os.listdir(tmp_path / name / "m") == ["act_hist.safetensors"]
    assert (tmp_path / "two" / "m" / "act_hist.safetensors").read_bytes() == (tmp_path / "one" / "m" / "act_hist.safetensors").read_bytes()
    assert merge_rank_act_hist(str(tmp_path / "one" / "m"), dev) is None
