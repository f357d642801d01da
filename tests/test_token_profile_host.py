"""CPU: the token profiles' contract (include/msae.h msae_token_profile_*) -- q(v) of the numpy
restatement (token_profile_ref.py) against the position profiles', the restatement against a state written out by hand, the
plain-torch `top_tokens` against the restatement bit for bit, and everything of `TokenProfile`, the cache wiring and the
launchers that needs no GPU.  Every comparison is exact.  (The cache run itself needs the device -- `Cache.add_topk` has no
CPU path, as for `PosProfile` -- and is in test_gpu_token_profile.py.)"""
import numpy as np
import pytest
import torch

import pos_profile_ref
import token_profile_ref as ref


# ---- q(v) -----------------------------------------------------------------------------------------------------------------
def test_q_equals_the_position_profiles_q():
    f = np.float32
    ulp = 2.0 ** -20
    vs = [f(0.5 * ulp), f(1.5 * ulp), f(2.5 * ulp), np.nextafter(f(0.5 * ulp), f(1)), np.nextafter(f(0.5 * ulp), f(0)), f(1e-40),
          f(1.0), f(1.0) + f(2.0 ** -23), f(3.0 + 2.0 ** -21), f(1e-5), f(2e-5), np.nextafter(f(2.0 ** 40), f(0)), f(2.0 ** 40),
          f(3e38), f(np.inf)]
    rng = np.random.default_rng(1)
    vs += list(np.exp(rng.normal(0.0, 6.0, size=3000)).astype(np.float32))
    vs += list((rng.integers(1, 1 << 12, size=1500) * 2.0 ** -21).astype(np.float32))          # ties among them
    assert [ref.q_of(v) for v in vs] == [pos_profile_ref.q_of(v) for v in vs]
    assert ref.q_of(f(1.0)) == 1 << 20 and ref.q_of(f(2.0 ** -21)) == 0 and ref.q_of(f(3 * 2.0 ** -21)) == 2
    assert ref.q_of(f(np.inf)) == 1 << 60


# ---- the restatement against a state written out by hand ----------------------------------------------------------------------
def _hand_case():
    """B = 2, S = 3, k = 2, N = 6, V = 4, queries (5, 2), offsets (0, 1, -1).
    ids: row 0 = [1, 9, 3] (9 lies outside the vocabulary), row 1 = [0, 0, -1]."""
    nan = np.nan
    vals = np.array([[[1.0, 2.0], [0.5, -1.0], [4.0, nan]],
                     [[1.0, 1e-5], [3.0, 0.0], [2.0, 2.0]]], np.float32)
    idx = np.array([[[5, 2], [5, 2], [5, 2]],
                    [[2, 5], [2, 6], [5, 5]]], np.int64)
    ids = np.array([[1, 9, 3], [0, 0, -1]], np.int64)
    one = 1 << 20
    counts = np.zeros((3, 2, 4), np.int32)
    mass = np.zeros((3, 2, 4), np.uint64)
    # offset 0: row 0: s = 0 token 1: features 5 (1.0) and 2 (2.0); s = 1 token 9: nowhere; s = 2 token 3: feature 5 (4.0), NaN no.
    #           row 1: s = 0 token 0: feature 2 (1.0), feature 5 at 1e-5 is not above thresh; s = 1 token 0: feature 2 (3.0),
    #           index 6 names no feature; s = 2 token -1: nowhere
    counts[0, 0, 1], mass[0, 0, 1] = 1, one
    counts[0, 1, 1], mass[0, 1, 1] = 1, 2 * one
    counts[0, 0, 3], mass[0, 0, 3] = 1, 4 * one
    counts[0, 1, 0], mass[0, 1, 0] = 2, 4 * one
    # offset +1: the token AFTER the firing position.  row 0: s = 0 -> token 9: nowhere; s = 1 -> token 3: feature 5 (0.5), the
    #           -1.0 of feature 2 no; s = 2 -> past the row.  row 1: s = 0 -> token 0: feature 2 (1.0); s = 1 -> token -1; s = 2 past
    counts[1, 0, 3], mass[1, 0, 3] = 1, one // 2
    counts[1, 1, 0], mass[1, 1, 0] = 1, one
    # offset -1: the token BEFORE.  row 0: s = 1 -> token 1: feature 5 (0.5); s = 2 -> token 9.  row 1: s = 1 -> token 0: feature
    #           2 (3.0); s = 2 -> token 0: feature 5 twice (2.0, 2.0: a repeat counts twice)
    counts[2, 0, 1], mass[2, 0, 1] = 1, one // 2
    counts[2, 1, 0], mass[2, 1, 0] = 1, 3 * one
    counts[2, 0, 0], mass[2, 0, 0] = 2, 4 * one
    tok = np.array([[2, 1, 0, 1],        # offset 0: every position with a token inside the vocabulary
                    [1, 0, 0, 1],        # offset +1: the positions s' = 1, 2 of each row
                    [2, 1, 0, 0]],       # offset -1: the positions s' = 0, 1
                   np.int64)
    return vals, idx, ids, counts, mass, tok


def test_restatement_equals_the_hand_written_state():
    vals, idx, ids, counts, mass, tok = _hand_case()
    st = ref.run([(vals, idx, ids)], 6, (5, 2), 4, (0, 1, -1))
    assert np.array_equal(st["counts"], counts) and np.array_equal(st["mass"], mass) and np.array_equal(st["tok_count"], tok)
    assert (st["n_rows"], st["n_positions"]) == (2, 6)
    two = ref.run([(vals[1:], idx[1:], ids[1:]), (vals[:1], idx[:1], ids[:1])], 6, (5, 2), 4, (0, 1, -1))
    assert all(np.array_equal(two[k], st[k]) for k in ("counts", "mass", "tok_count"))
    # a threshold below zero lets the zero through the keep rule; it is still counted nowhere (v > 0)
    low = ref.run([(vals, idx, ids)], 6, (5, 2), 4, (0, 1, -1), thresh=-1.0)
    assert low["counts"][0, 0, 0] == 1 and low["counts"].sum() == counts.sum() + 2       # only the 1e-5 of feature 5 is new (planes 0, 1)


# ---- top tokens: plain torch against the restatement ----------------------------------------------------------------------------
def planted_profile(V, device=None):
    """A `TokenProfile` with F = 7 queries, offsets (0, -1) and hand-placed counters: random rows, ties, rows with fewer
    candidates than any m, counts above 2^24 that round to one float, and masses at and beyond 2^63 (the int64 is negative)."""
    from msae.features import TokenProfile

    rng = np.random.default_rng(100 + V)
    F = 7
    st = TokenProfile(300, [17, 4, 250, 9, 0, 299, 123], V, offsets=(0, -1), mass=True, device=device)
    counts = (rng.integers(1, 40, size=(2, F, V)) * (rng.uniform(size=(2, F, V)) < 0.3)).astype(np.int64)
    counts[:, 1] = 0
    counts[:, 1, [5, 50, 96]] = [[2, 7, 2], [3, 3, 1]]              # three candidates, two of them tied; fewer than min_count 3
    counts[:, 2] = 0                                                # an empty row
    counts[:, 3] = 0
    counts[:, 3, [3, 40, 41, 42, 90]] = [(1 << 24) + 1, (1 << 24), (1 << 24) + 2, (1 << 24) + 3, (1 << 31) - 1]
    counts[:, 4] = 4                                                # every token ties on the count
    counts[0, 5] = np.where(np.arange(V) % 3 == 0, 3, 0)            # ties, a third of the row
    tok = counts.sum(axis=1) + rng.integers(0, 50, size=(2, V))
    tok[:, 7] = counts[:, :, 7].max(axis=1)                         # precision 1 somewhere
    mass = counts * rng.integers(1, 1 << 22, size=(2, F, V))
    mass[:, 4] = 4 * (3 << 19)                                      # equal means: ties on every token
    mass = mass.astype(np.uint64)
    mass[0, 0, np.flatnonzero(counts[0, 0])[:3]] = [1 << 63, (1 << 64) - 1, (1 << 63) + (1 << 10) + 1]
    mass[0, 1, 5] = (1 << 63) + 1024                                # a tie of the f64 conversion: to even
    st.counts.copy_(torch.from_numpy(counts.astype(np.int32)))
    st.mass.copy_(torch.from_numpy(mass.view(np.int64)))
    st.tok_count.copy_(torch.from_numpy(tok))
    st.n_rows, st.n_positions = 11, 11 * 64
    return st, counts.astype(np.int32), mass, tok


_TOP_REF = {}


def top_ref(V, plane, m, metric, min_count):
    """The restatement's lists for `planted_profile(V)`, computed once per (V, plane, metric, min_count) at m = 64."""
    key = (V, plane, metric, min_count)
    if key not in _TOP_REF:
        _, counts, mass, tok = planted_profile(V)
        _TOP_REF[key] = ref.top_tokens(counts[plane], mass[plane], tok[plane], 64, metric, min_count)
    val, tk, tot = _TOP_REF[key]
    return val[:, :m], tk[:, :m], tot


@pytest.mark.parametrize("metric", ["count", "precision", "mean"])
@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("V", [97, 5000])
def test_top_tokens_torch_path_equals_the_restatement(V, min_count, metric):
    st, counts, mass, tok = planted_profile(V)
    for offset, plane in ((0, 0), (-1, 1)):
        for m in (1, 10, 64):
            val, tk, tot = st.top_tokens(m=m, by=metric, offset=offset, min_count=min_count)
            rv, rt, rtot = top_ref(V, plane, m, metric, min_count)
            assert val.dtype == torch.float32 and tk.dtype == torch.int32 and tot.dtype == torch.int64
            assert np.array_equal(val.numpy().view(np.uint32), rv.view(np.uint32)), (offset, m)
            assert np.array_equal(tk.numpy(), rt) and np.array_equal(tot.numpy(), rtot)
    rv, rt, rtot = top_ref(V, 0, 64, metric, min_count)
    assert rt[2].tolist() == [-1] * 64 and rv[2].tolist() == [0.0] * 64 and rtot[2] == 0          # the empty row: all padding
    assert (rt[1] >= 0).sum() == (3 if min_count == 1 else 1)                                     # fewer than m candidates
    if metric == "count":
        # 2^24 + 1 rounds to 2^24 and 2^24 + 3 to 2^24 + 4: the order is that of the f32 score, then the token
        assert rt[3, :5].tolist() == [90, 42, 41, 3, 40] and rv[3, :3].tolist() == [2.0 ** 31, 2.0 ** 24 + 4, 2.0 ** 24 + 2]
        assert rv[3, 3] == rv[3, 4] == 2.0 ** 24 and rtot[3] == 4 * (1 << 24) + 6 + (1 << 31) - 1
        assert rt[4, :10].tolist() == list(range(10))                                             # all tied: ascending tokens
        if min_count == 1:
            assert rt[1, :3].tolist() == [50, 5, 96]
    if metric == "mean" and min_count == 1:
        c0 = np.flatnonzero(counts[0, 0])[:3]
        assert set(rt[0, :3].tolist()) == set(c0.tolist())                                        # the unsigned reading: the largest
        assert float(rv[1, 0]) == float(np.float32(2.0 ** 63 / 2.0 * 2.0 ** -20)) and rt[1, 0] == 5     # 2^63 + 1024 -> 2^63 (even)


def test_top_tokens_of_a_feature_subset_and_row():
    st, counts, _, _ = planted_profile(97)
    val, tk, tot = st.top_tokens(m=10, by="precision", offset=-1)
    sv, stk, stot = st.top_tokens(m=10, by="precision", offset=-1, features=[9, 17, 9])
    assert torch.equal(sv, val[[3, 0, 3]]) and torch.equal(stk, tk[[3, 0, 3]]) and torch.equal(stot, tot[[3, 0, 3]])
    assert np.array_equal(st.row(250).numpy(), counts[0, 2]) and np.array_equal(st.row(9, offset=-1).numpy(), counts[1, 3])
    with pytest.raises(KeyError):
        st.row(5)
    with pytest.raises(KeyError):
        st.top_tokens(features=[17, 5])


def test_top_tokens_argument_errors():
    from msae.features import TokenProfile

    st, *_ = planted_profile(97)
    for kw in (dict(m=0), dict(m=65), dict(by="jaccard"), dict(offset=1), dict(min_count=0)):
        with pytest.raises(ValueError):
            st.top_tokens(**kw)
    with pytest.raises(ValueError, match="mass=True"):
        TokenProfile(8, [1], 5).top_tokens(by="mean")
    with pytest.raises(ValueError):
        st.row(17, offset=3)


def test_single_token_and_decode():
    from msae.features import TokenProfile

    st = TokenProfile(50, [7, 3, 40, 11, 12], 20, offsets=(0, 1))
    c = torch.zeros(2, 5, 20, dtype=torch.int32)
    c[0, 0, 4] = 95; c[0, 0, 5] = 5                        # 95 % on one token
    c[0, 1, 4] = 60; c[0, 1, 9] = 35; c[0, 1, 2] = 5       # 60 % on one, 95 % on two
    c[0, 2, 6] = 9; c[0, 2, 1] = 1                         # exactly 90 %
    c[0, 3, 8] = 1                                         # one fire on one token
    c[1, 1, 0] = 10                                        # row 4 never fired; in the next-token plane only feature 3 did
    st.counts.copy_(c)
    assert st.single_token().tolist() == [7, 40, 11] and st.single_token().dtype == torch.int64
    assert st.single_token(min_fired=2).tolist() == [7, 40] and st.single_token(share=0.91).tolist() == [7, 11]
    assert st.single_token(share=0.95, max_tokens=2).tolist() == [7, 3, 40, 11]
    assert st.single_token(offset=1).tolist() == [3] and st.single_token(share=0.0).tolist() == [7, 3, 40, 11]

    class Tok:
        def convert_ids_to_tokens(self, ids):
            return [f"<{i}>" for i in ids]

    _, tk, _ = st.top_tokens(m=3)
    assert TokenProfile.decode(tk, Tok()) == [["<4>", "<5>"], ["<4>", "<9>", "<2>"], ["<6>", "<1>"], ["<8>"], []]


# ---- the constructor, update's host checks -----------------------------------------------------------------------------------
def test_constructor_validation():
    from msae.features import TokenProfile

    for kw in (dict(num_latents=0), dict(num_latents=262145), dict(queries=[]), dict(queries=[1, 1]), dict(queries=[16]),
               dict(queries=[-1]), dict(queries=list(range(16385)), num_latents=20000), dict(vocab_size=0), dict(offsets=()),
               dict(offsets=(0, 1, 2, 3, 4)), dict(offsets=(1, 1)), dict(offsets=(65,)), dict(offsets=(-65, 0))):
        args = dict(num_latents=16, queries=[3, 1], vocab_size=10)
        args.update(kw)
        with pytest.raises(ValueError):
            TokenProfile(**args)
    with pytest.raises(ValueError, match="2\\^31"):                                # the cell index, whatever max_bytes
        TokenProfile(20000, list(range(16384)), 131072, max_bytes=1 << 50)
    with pytest.raises(ValueError, match=str(3 * 5000 * 32000 * 4 + 3 * 32000 * 8)):      # the guard names the sizes
        TokenProfile(131072, list(range(5000)), 32000, offsets=(-1, 0, 1), max_bytes=1 << 30)
    with pytest.raises(ValueError, match=str(2 * 100 * 12 + 100 * 8)):
        TokenProfile(16, [0, 1], 100, mass=True, max_bytes=1000)
    st = TokenProfile(16, torch.tensor([3, 1]), 10, offsets=(0, -2), mass=True)
    assert st.counts.shape == (2, 2, 10) and st.counts.dtype == torch.int32 and st.mass.dtype == torch.int64
    assert st.tok_count.shape == (2, 10) and st.tok_count.dtype == torch.int64 and st.queries.tolist() == [3, 1]
    assert (st.n_rows, st.n_positions, st.offsets, st.device.type) == (0, 0, (0, -2), "cpu")
    assert TokenProfile(16, [3], 10).mass is None and TokenProfile(16, [3], 10).offsets == (0,)


def test_update_checks_shapes_before_any_device_work():
    from msae.features import TokenProfile

    st = TokenProfile(16, [0, 1], 10)
    v, i, t = torch.ones(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64)
    for bad in (lambda: st.update(v, i[:1], t), lambda: st.update(v, i, t[:1]), lambda: st.update(v, i, t[:, :2]),
                lambda: st.update(v, i, t.reshape(-1)), lambda: st.update(v, i, t.float()),
                lambda: st.update(torch.ones(2, 3, 257), torch.zeros(2, 3, 257, dtype=torch.int64), t)):
        with pytest.raises(ValueError):
            bad()
    st.update(v[:0], i[:0], t[:0])                   # empty input: a no-op, on any device
    assert st.n_positions == 0 and st.n_rows == 0
    with pytest.raises(RuntimeError):
        st.update(v, i, t)                           # there is no CPU path for the update
    assert st.n_positions == 0 and int(st.tok_count.sum()) == 0
    st.n_positions = (1 << 31) - 6
    with pytest.raises(OverflowError):
        st.update(v, i, t)


# ---- merge, files ---------------------------------------------------------------------------------------------------------
def test_merge_laws_and_kind_mismatch():
    from msae.features import TokenProfile

    a, ca, ma, ta = planted_profile(97)
    b, *_ = planted_profile(97)
    b.counts.copy_(b.counts.flip(2)); b.mass.copy_(b.mass.flip(2))
    cb, mb = b.counts.clone(), b.mass.clone()
    assert a.merge(b) is a and a.n_rows == 22 and a.n_positions == 22 * 64
    with np.errstate(over="ignore"):
        assert np.array_equal(a.counts.numpy(), ca + cb.numpy())               # int32 adds wrap, as the counters do
    assert np.array_equal(a.mass.numpy().view(np.uint64), ma + mb.numpy().view(np.uint64))     # the unsigned sum mod 2^64
    assert np.array_equal(a.tok_count.numpy(), 2 * ta)
    q = [17, 4, 250, 9, 0, 299, 123]
    for args, kw in (((301, q, 97), {}), ((300, q, 98), {}), ((300, q[::-1], 97), {}), ((300, q[:6], 97), {}),
                     ((300, q, 97), dict(offsets=(-1, 0))), ((300, q, 97), dict(offsets=(0,))), ((300, q, 97), dict(mass=False)),
                     ((300, q, 97), dict(thresh=1e-4))):
        kw = dict(dict(offsets=(0, -1), mass=True), **kw)
        with pytest.raises(ValueError):
            a.merge(TokenProfile(*args, **kw))
    a.n_positions = (1 << 31) - 10
    with pytest.raises(OverflowError):
        a.merge(b)
    assert a.n_rows == 22


def test_file_round_trip(tmp_path):
    from msae.features import PosProfile, TokenProfile
    from safetensors import safe_open

    st, *_ = planted_profile(97)
    p = str(tmp_path / "token_profile.safetensors")
    st.save(p)
    back = TokenProfile.load(p)
    assert back._kind() == st._kind() and back.kind_hash() == st.kind_hash() and back.device.type == "cpu"
    assert (back.n_rows, back.n_positions) == (11, 11 * 64)
    assert torch.equal(back.counts, st.counts) and torch.equal(back.mass, st.mass) and torch.equal(back.tok_count, st.tok_count)
    with safe_open(p, framework="pt") as fh:
        meta = fh.metadata()
        assert sorted(fh.keys()) == ["cell_count", "cell_key", "cell_mass", "queries", "tok_count"]
    assert meta == {"format": "msae.token_profile.v1", "num_latents": "300", "vocab_size": "97", "offsets": "0,-1", "mass": "1",
                    "thresh": "1e-05", "kind": st.kind_hash(), "n_rows": "11", "n_positions": str(11 * 64)}
    q = str(tmp_path / "again.safetensors")
    back.save(q)
    assert open(p, "rb").read() == open(q, "rb").read()
    val, tk, tot = back.top_tokens(m=10, by="mean", offset=-1)                 # a loaded file reads without a GPU
    rv, rt, rtot = top_ref(97, 1, 10, "mean", 1)
    assert np.array_equal(val.numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(tk.numpy(), rt)
    with pytest.raises(ValueError):
        TokenProfile.load(p, max_bytes=64)
    with pytest.raises(ValueError):
        PosProfile.load(p)
    plain = TokenProfile(12, [3, 5], 9)                                        # without mass: no cell_mass in the file
    plain.counts[0, 1, 4] = 6
    plain.save(q)
    again = TokenProfile.load(q)
    assert again.mass is None and torch.equal(again.counts, plain.counts) and again.kind_hash() == plain.kind_hash()
    assert again.kind_hash() != TokenProfile(12, [5, 3], 9).kind_hash()        # the order of the queries is part of the kind


def test_merge_rank_files_on_the_host(tmp_path):
    from msae.features.cache import merge_rank_token_profile

    a, *_ = planted_profile(97)
    b, *_ = planted_profile(97)
    both, *_ = planted_profile(97)
    both.merge(b)
    a.save(str(tmp_path / "Rank0_token_profile.safetensors"))
    b.save(str(tmp_path / "Rank1_token_profile.safetensors"))
    out = merge_rank_token_profile(str(tmp_path))
    assert out == str(tmp_path / "token_profile.safetensors") and sorted(p.name for p in tmp_path.iterdir()) == ["token_profile.safetensors"]
    both.save(str(tmp_path / "want.safetensors"))
    assert (tmp_path / "token_profile.safetensors").read_bytes() == (tmp_path / "want.safetensors").read_bytes()
    assert merge_rank_token_profile(str(tmp_path)) is None


# ---- the cache wiring -----------------------------------------------------------------------------------------------------
def test_cache_allocates_nothing_when_off_and_checks_its_arguments():
    from msae.features import Cache, FeatureImageCache
    from msae.features.cache import ACCUMULATORS

    assert Cache(0).tokens is None and Cache(0).token_profiles == {}
    assert [k.keyword for k in ACCUMULATORS][-2:] == ["pos", "tokens"] and ACCUMULATORS[-1].stem == "token_profile"
    c = Cache(0, tokens=dict(vocab_size=40, queries=[1, 2]))
    assert c.tokens == dict(vocab_size=40, queries=[1, 2]) and c.token_profiles == {}
    assert Cache(0, filters={"m": torch.tensor([1])}, tokens=dict(vocab_size=40)).token_profiles == {}
    with pytest.raises(ValueError, match="query features"):
        Cache(0, tokens=dict(vocab_size=40))
    with pytest.raises(ValueError, match="vocab"):
        Cache(0, tokens=dict(queries=[1]))
    v, i = torch.ones(1, 2, 3), torch.zeros(1, 2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="token_ids"):
        c.add_topk(v, i, 16, 0, "m")                 # tokens= given, no token_ids: before any device work
    assert c.token_profiles == {}
    with pytest.raises(ValueError, match="no query features for module 'other'"):
        Cache(0, filters={"m": torch.tensor([1])}, tokens=dict(vocab_size=40))._new_token_profile("other", 16, "cpu")
    tp = Cache(0, filters={"m": torch.tensor([5, 1])}, tokens=dict(vocab_size=40, offsets=(0, 1)))._new_token_profile("m", 16, "cpu")
    assert tp.queries.tolist() == [5, 1] and tp.offsets == (0, 1) and tp.vocab_size == 40
    tp = Cache(0, tokens=dict(vocab_size=40, queries={"m": [3]}))._new_token_profile("m", 16, "cpu")
    assert tp.queries.tolist() == [3]
    with pytest.raises(ValueError, match="no token per position"):
        FeatureImageCache(None, None, {}, 2, 0, processor=object(), tokens=dict(vocab_size=40, queries=[1]))


def test_cli_flags(capsys):
    from msae.config import parse_cache_config, token_profile_kwargs
    from msae.launch.cache import cache, cache_image

    cfg = parse_cache_config(["model", "data"])
    assert cfg.token_profile is False and cfg.token_profile_offsets is None and cfg.token_profile_mass is False
    assert token_profile_kwargs(cfg, 100) is None
    cache_image.check_config(cfg)
    cfg = parse_cache_config(["model", "data", "--token_profile", "--filters_path", "f.json"])
    assert token_profile_kwargs(cfg, 100) == dict(vocab_size=100, offsets=(0,), mass=False)
    cfg = parse_cache_config(["model", "data", "--token_profile", "--filters_path", "f.json", "--token_profile_offsets", "-1,0,1",
                              "--token_profile_mass"])
    assert token_profile_kwargs(cfg, 128256) == dict(vocab_size=128256, offsets=(-1, 0, 1), mass=True)
    with pytest.raises(SystemExit):
        parse_cache_config(["model", "data", "--token_profile"])
    assert "--filters_path" in capsys.readouterr().err
    for bad in ("a", "0,0", "65", "-65,0", "0,1,2,3,4", "", "1;2"):
        with pytest.raises(SystemExit):
            parse_cache_config(["model", "data", "--token_profile", "--filters_path", "f.json", "--token_profile_offsets", bad])
        assert "--token_profile_offsets" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cache_image.check_config(cfg)                # the image launcher refuses the flag
    assert "no token per position" in capsys.readouterr().err

    class Tok:
        def __len__(self):
            return 32000

    class S:
        num_latents = 131072

    filters = {"layers.1": torch.arange(5000)}
    assert cache.token_profiles(cfg, Tok(), {"layers.1": S()}, filters) == dict(vocab_size=32000, offsets=(-1, 0, 1), mass=True)
    assert cache.token_profiles(parse_cache_config(["model", "data"]), Tok(), {"layers.1": S()}, filters) is None
    with pytest.raises(SystemExit):                  # 3 x 20000 x 32000 cells pass 2^31: ends like a bad flag
        cache.token_profiles(cfg, Tok(), {"layers.1": S()}, {"layers.1": torch.arange(20000)})
    assert "--token_profile" in capsys.readouterr().err


def test_alias_package_resolves_the_new_names():
    import os
    import subprocess
    import sys

    from conftest import REPO

    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(REPO / "multimodal-sae_amd"), str(REPO / "multimodal-sae_amd" / "compat")]))
    code = ("from sae_auto_interp.features import TokenProfile\n"
            "import sae_auto_interp.features.tokens as t\n"
            "import msae.features\n"
            "assert TokenProfile is msae.features.TokenProfile and t.FORMAT == 'msae.token_profile.v1'\n"
            "print('ok')")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-1500:]
