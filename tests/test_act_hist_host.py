"""CPU: the activation histograms' contract (include/msae.h msae_act_hist_*) -- the bin rule of the
numpy restatement (act_hist_ref.py) against an independent frexp formulation, the quantile rule against order statistics of
the raw values, and everything of `ActHist` that needs no GPU.  Every comparison is exact."""
import math

import numpy as np
import pytest
import torch

import act_hist_ref as ref

BINNINGS = [(3, -16, 32), (0, -4, 8), (4, -16, 32), (2, -3, 5), (1, -126, 254), (0, 127, 1)]


def _bins_frexp(c, s, e_lo, E):
    """The bin by arithmetic: c = m * 2^e with m in [0.5, 1) -> octave e - 1, sub-bin floor((2m - 1) * 2^s).  Exact in f64:
    2m - 1 has at most 24 significant bits, times 2^s."""
    c = np.asarray(c, np.float32).astype(np.float64)
    out = np.empty(c.shape, np.int64)
    fin = np.isfinite(c)
    m, e = np.frexp(c[fin])
    raw = (e.astype(np.int64) - 1 - e_lo) * (1 << s) + np.floor((2.0 * m - 1.0) * (1 << s)).astype(np.int64)
    out[fin] = np.clip(raw, 0, (E << s) - 1)
    out[~fin] = (E << s) - 1                         # +inf
    return out


def _lognormal(rng, n, sigma=4.0):
    return np.exp(rng.normal(0.0, sigma, size=n)).astype(np.float32)


@pytest.mark.parametrize("s,e_lo,E", BINNINGS)
def test_bin_rule_equals_the_frexp_formulation(s, e_lo, E):
    rng = np.random.default_rng(1)
    c = _lognormal(rng, 200000)
    c = c[c > 0]
    e = ref.edges(s, e_lo, E)
    fin = e[np.isfinite(e) & (e > 0)]
    hand = np.concatenate([fin, np.nextafter(fin, np.float32(0)), np.nextafter(fin, np.float32(np.inf)),
                           np.array([1e-5, 1.0, 1.125, 65536.0, np.inf, 1e-45, 1e-40, 1.1754944e-38, 3.4028235e38, 0.99999994],
                                    np.float32)])
    hand = hand[hand > 0]
    for vals in (c, hand):
        assert np.array_equal(ref.bins_of(vals, s, e_lo, E), _bins_frexp(vals, s, e_lo, E))


def test_pinned_bins_and_edges():
    assert ref.bins_of(np.array([1e-5, 1.0, 1.125, 65536.0, np.inf], np.float32)).tolist() == [0, 128, 129, 255, 255]
    e = ref.edges()
    assert e.shape == (257,) and e[0] == 2.0 ** -16 and e[128] == 1.0 and e[129] == 1.125 and e[256] == 65536.0
    assert (np.diff(e.astype(np.float64)) > 0).all()
    assert (e[1:].astype(np.float64) / e[:-1] <= 1.125).all()         # each bin under 12.5 % wide
    assert np.isinf(ref.edges(0, 127, 1)[1]) and ref.edges(1, -126, 254)[0] == np.float32(2.0 ** -126)


@pytest.mark.parametrize("s,e_lo,E", BINNINGS)
def test_unclamped_values_lie_between_their_edges(s, e_lo, E):
    rng = np.random.default_rng(2)
    c = _lognormal(rng, 100000)
    e = ref.edges(s, e_lo, E)
    c = np.concatenate([c, e[:-1], np.nextafter(e[1:], np.float32(0))])
    raw = ref.raw_bins_of(c, s, e_lo, E)
    c = c[(raw >= 0) & (raw < (E << s)) & np.isfinite(c) & (c > 0)]
    assert len(c) > (E << s)
    b = ref.bins_of(c, s, e_lo, E)
    assert (e[b] <= c).all() and (c < e[b + 1]).all()


def _filled(hist, n_segments, **kw):
    from msae.features import ActHist

    st = ActHist(hist.shape[0], **kw)
    st.hist.copy_(torch.from_numpy(hist))
    st.n_segments = int(n_segments)
    return st


def _rows_of_values(rng, N, s, e_lo, E, empty=(3,), single=(5,)):
    """Per feature a list of raw values inside [2^e_lo, 2^(e_lo + E)) (nothing clamps), of very different lengths."""
    rows = []
    for f in range(N):
        n = 0 if f in empty else 1 if f in single else int(rng.integers(1, 400))
        u = rng.uniform(e_lo, e_lo + E, size=n)
        v = np.exp2(u).astype(np.float32)
        lo, hi = np.float32(2.0 ** e_lo), np.nextafter(np.float32(2.0 ** (e_lo + E)), np.float32(0))
        rows.append(np.clip(v, lo, hi))
    return rows


QS = [0.0, 0.01, 0.1, 0.25, 0.5, 1.0 / 3.0, 0.9, 0.999, 1.0]


@pytest.mark.parametrize("s,e_lo,E", [(3, -16, 32), (0, -4, 8), (4, -8, 16)])
def test_quantile_bin_holds_the_order_statistic(s, e_lo, E):
    rng = np.random.default_rng(3)
    N = 40
    rows = _rows_of_values(rng, N, s, e_lo, E)
    hist = np.zeros((N, E << s), np.int32)
    for f, v in enumerate(rows):
        np.add.at(hist[f], ref.bins_of(v, s, e_lo, E), 1)
    st = _filled(hist, 0, sub_bits=s, e_lo=e_lo, octaves=E)
    got = st.quantile_bins(QS).numpy()
    assert got.dtype == np.int32 and np.array_equal(got, ref.quantile_bins(hist, QS))
    e = ref.edges(s, e_lo, E)
    assert np.array_equal(st.edges().numpy().view(np.uint32), e.view(np.uint32))
    val = st.quantile(QS).numpy()
    for f, v in enumerate(rows):
        if len(v) == 0:
            assert (got[f] == -2).all() and np.isnan(val[f]).all()
            continue
        srt = np.sort(v)
        for i, q in enumerate(QS):
            r = min(max(math.ceil(q * float(len(v))), 1), len(v))
            x = srt[r - 1]
            b = got[f, i]
            assert e[b] <= x < e[b + 1], (f, q)
            assert val[f, i] == e[b]
    assert np.array_equal(st.fired().numpy(), np.array([len(v) for v in rows]))


def test_zeros_population_and_threshold_at_rate():
    """Token pool, one value per (segment, feature) at most: the population of a feature is its values and a zero for every
    other segment.  threshold_at_rate against a brute-force count over that population."""
    rng = np.random.default_rng(4)
    N, n_seg = 12, 1000
    fire = [0, 1, 10, 250, 500, 999, 1000, 37, 640, 3, 125, 875]
    pops = []
    hist = np.zeros((N, 256), np.int32)
    for f in range(N):
        v = np.exp2(rng.uniform(-10, 10, size=fire[f])).astype(np.float32)
        np.add.at(hist[f], ref.bins_of(v), 1)
        pops.append(np.sort(np.concatenate([np.zeros(n_seg - fire[f], np.float32), v])))
    st = _filled(hist, n_seg)
    qs = [0.0, 0.3, 0.5, 0.75, 0.999, 1.0]
    got = st.quantile_bins(qs, zeros=True).numpy()
    assert np.array_equal(got, ref.quantile_bins(hist, qs, n_seg, True))
    assert (got[0] == -1).all()                      # never fired: every quantile is a zero
    assert got[1].tolist() == [-1] * 5 + [int(ref.bins_of(pops[1][-1:])[0])]
    assert (got[6] >= 0).all()                       # fired on every segment: no zero in the population
    assert np.array_equal(_filled(hist, 0).quantile_bins(qs, zeros=True).numpy()[0], [-2] * 6)     # nothing seen at all
    assert np.array_equal(st.quantile_bins(qs, zeros=False).numpy()[0], [-2] * 6)
    e = ref.edges()
    val = st.quantile(qs, zeros=True).numpy()
    for f in range(N):
        for i, q in enumerate(qs):
            r = min(max(math.ceil(q * float(n_seg)), 1), n_seg)
            x = pops[f][r - 1]
            assert val[f, i] == (0.0 if x == 0 else e[ref.bins_of(x[None])[0]])
    rates = [0.5, 0.25, 0.1, 0.001, 1.0]
    thr = st.threshold_at_rate(rates).numpy()
    assert thr.shape == (N, len(rates)) and thr.dtype == np.float32
    assert np.array_equal(thr.view(np.uint32), st.quantile([1.0 - r for r in rates], zeros=True).numpy().view(np.uint32))
    for f in range(N):
        for i, rate in enumerate(rates):
            r = min(max(math.ceil((1.0 - rate) * float(n_seg)), 1), n_seg)
            need = n_seg - r + 1                     # segments at or above the r-th smallest value
            t = thr[f, i]
            if t == 0.0:
                assert (pops[f] > 0).sum() < need    # fires on less than that share
            else:
                nxt = e[ref.bins_of(np.array([t], np.float32))[0] + 1]
                assert (pops[f] >= t).sum() >= need > (pops[f] >= nxt).sum()
    assert st.threshold_at_rate(0.5).shape == (N, 1)


def test_host_quantiles_equal_the_restatement_on_big_counts():
    """Counts above 2^24 (a float accumulator would lose them), a single count, an empty row, every Q."""
    rng = np.random.default_rng(5)
    N = 9
    hist = rng.integers(0, 5, size=(N, 256)).astype(np.int32)
    hist[0] = 0
    hist[1] = 0; hist[1, 200] = 1
    hist[2, 7], hist[2, 8], hist[2, 250] = (1 << 24) + 1, 1, (1 << 30)
    hist[3] = 0; hist[3, 0], hist[3, 255] = 2 ** 31 - 1, 2 ** 31 - 1
    for Q in (1, 7, 64):
        qs = np.sort(rng.uniform(0, 1, size=Q)).tolist()
        for zeros, n_seg in ((False, 0), (True, 2 ** 31 - 1), (True, 10)):
            st = _filled(hist, n_seg)
            assert np.array_equal(st.quantile_bins(qs, zeros=zeros).numpy(), ref.quantile_bins(hist, qs, n_seg, zeros))


def test_constructor_validation():
    from msae.features import ActHist

    for kw in (dict(pool="row"), dict(num_latents=0), dict(num_latents=262145), dict(pool="image", pool_len=0),
               dict(pool="image", pool_len=2881), dict(pool="window", window=0), dict(pool="window", window=4097),
               dict(sub_bits=-1), dict(sub_bits=5), dict(octaves=0), dict(e_lo=-127), dict(e_lo=100, octaves=29),
               dict(sub_bits=4, octaves=33)):
        args = dict(num_latents=16)
        args.update(kw)
        with pytest.raises(ValueError):
            ActHist(**args)
    with pytest.raises(ValueError, match=str(131072 * 256 * 4)):
        ActHist(131072, max_bytes=1 << 20)
    st = ActHist(16, sub_bits=4, octaves=32)
    assert st.n_bins == 512 and st.hist.shape == (16, 512) and st.hist.dtype == torch.int32 and st.n_segments == 0
    assert ActHist(5, sub_bits=0, e_lo=127, octaves=1).n_bins == 1
    for qs in ([], [0.5] * 65, [1.5], [-0.1], [float("nan")]):
        with pytest.raises(ValueError):
            st.quantile_bins(qs)


def test_update_checks_shapes_and_the_segment_guard_before_any_device_work():
    from msae.features import ActHist

    st = ActHist(16)
    v, i = torch.ones(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int64)
    with pytest.raises(ValueError):
        st.update(v, i[:1])
    with pytest.raises(ValueError):
        st.update(torch.ones(2, 3, 257), torch.zeros(2, 3, 257, dtype=torch.int64))
    st.update(v[:0], i[:0])                          # empty input: a no-op, on any device
    st.update(v[:, :0], i[:, :0])
    assert st.n_segments == 0 and int(st.hist.sum()) == 0
    with pytest.raises(RuntimeError):
        st.update(v, i)                              # there is no CPU path for the update
    st.n_segments = (1 << 31) - 6
    with pytest.raises(OverflowError):
        st.update(v, i)                              # 6 more token segments reach 2^31: refused before the device check
    assert st.n_segments == (1 << 31) - 6
    win = ActHist(16, pool="window", window=2)
    win.n_segments = (1 << 31) - 2
    with pytest.raises(OverflowError):
        win.update(v, i)                             # 2 rows x (3 // 2) windows


def test_merge_laws_and_kind_mismatch():
    from msae.features import ActHist

    rng = np.random.default_rng(6)
    ha, hb = (rng.integers(0, 9, size=(16, 256)).astype(np.int32) for _ in range(2))
    a, b = _filled(ha, 10), _filled(hb, 7)
    assert a.merge(b) is a and a.n_segments == 17 and np.array_equal(a.hist.numpy(), ha + hb)
    for kw in (dict(pool="window"), dict(thresh=1e-4), dict(sub_bits=2, octaves=64), dict(e_lo=-15)):
        with pytest.raises(ValueError):
            a.merge(ActHist(16, **kw))
    with pytest.raises(ValueError):
        a.merge(ActHist(17))
    with pytest.raises(ValueError):
        ActHist(16, pool="window", window=32).merge(ActHist(16, pool="window", window=64))
    ActHist(16, pool="token", window=32).merge(ActHist(16, pool="token", window=64))     # the window of a token pool is unused
    big = _filled(ha, (1 << 31) - 10)
    with pytest.raises(OverflowError):
        big.merge(a)
    assert big.n_segments == (1 << 31) - 10 and np.array_equal(big.hist.numpy(), ha)


def test_file_round_trip(tmp_path):
    from msae.features import ActHist
    from safetensors import safe_open

    rng = np.random.default_rng(7)
    hist = (rng.integers(0, 50, size=(33, 40)) * (rng.uniform(size=(33, 40)) < 0.2)).astype(np.int32)
    st = _filled(hist, 777, pool="image", pool_len=24, thresh=2e-5, sub_bits=2, e_lo=-3, octaves=10)
    p = str(tmp_path / "act_hist.safetensors")
    st.save(p)
    back = ActHist.load(p)
    assert back._kind() == st._kind() and back.n_segments == 777 and back.device.type == "cpu"
    assert torch.equal(back.hist, st.hist)
    for zeros in (False, True):
        assert torch.equal(back.quantile(QS, zeros).view(torch.int32), st.quantile(QS, zeros).view(torch.int32))
    with safe_open(p, framework="pt") as fh:
        meta = fh.metadata()
        assert list(fh.keys()) == ["hist"]
    assert meta == {"format": "msae.act_hist.v1", "pool": "image", "pool_len": "24", "window": "64", "thresh": "2e-05",
                    "num_latents": "33", "sub_bits": "2", "e_lo": "-3", "octaves": "10", "n_segments": "777"}
    q = str(tmp_path / "again.safetensors")
    back.save(q)
    assert open(p, "rb").read() == open(q, "rb").read()
    with pytest.raises(ValueError):
        ActHist.load(p, max_bytes=64)
    from msae.features import CoactStats

    with pytest.raises(ValueError):
        CoactStats.load(p)


def test_cache_allocates_nothing_when_off():
    from msae.features import Cache

    assert Cache(0).hist is None and Cache(0).act_hists == {}
    c = Cache(0, hist=dict(pool="window", window=8))
    assert c.hist == dict(pool="window", window=8) and c.act_hists == {}


def test_cli_flags(capsys):
    from msae.config import act_hist_kwargs, parse_cache_config
    from msae.launch.cache import cache, cache_image

    cfg = parse_cache_config(["model", "data"])
    assert cfg.act_hist is False and cfg.act_hist_pool is None and cfg.act_hist_bins is None
    assert act_hist_kwargs(cfg, cache.ACT_HIST_DEFAULT_POOL) is None
    cfg = parse_cache_config(["model", "data", "--act_hist"])
    assert act_hist_kwargs(cfg, cache.ACT_HIST_DEFAULT_POOL) == dict(pool="token", window=64, pool_len=576)
    assert act_hist_kwargs(cfg, cache_image.ACT_HIST_DEFAULT_POOL, pool_len=9) == dict(pool="image", window=64, pool_len=9)
    cfg = parse_cache_config(["model", "data", "--act_hist", "--act_hist_pool", "window", "--example_ctx_len", "32",
                              "--act_hist_bins", "4,-8,16"])
    kw = act_hist_kwargs(cfg, cache_image.ACT_HIST_DEFAULT_POOL)
    assert kw == dict(pool="window", window=32, pool_len=576, sub_bits=4, e_lo=-8, octaves=16)
    from msae.features import ActHist

    assert ActHist(64, **kw).n_bins == 256
    for bad in (["--act_hist_pool", "row"], ["--act_hist_bins", "3,-16"], ["--act_hist_bins", "5,-16,32"],
                ["--act_hist_bins", "a,b,c"], ["--act_hist_bins", "4,-16,33"]):
        with pytest.raises(SystemExit):
            parse_cache_config(["model", "data", "--act_hist"] + bad)
        assert bad[0] in capsys.readouterr().err


def test_alias_package_resolves_the_launchers_with_the_new_flags():
    import os
    import subprocess
    import sys

    from conftest import REPO

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(REPO / "multimodal-sae_amd"), str(REPO / "multimodal-sae_amd" / "compat")]))
    code = ("import sae_auto_interp.launch.cache.cache as a, sae_auto_interp.launch.cache.cache_image as b\n"
            "import msae.launch.cache.cache as c\n"
            "assert a is c and a.ACT_HIST_DEFAULT_POOL == 'token' and b.ACT_HIST_DEFAULT_POOL == 'image'\n"
            "from sae_auto_interp.features import ActHist\n"
            "import msae.features\n"
            "assert ActHist is msae.features.ActHist\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-1500:]
