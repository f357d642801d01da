"""GPU: token profiles and their top-token lists (msae_token_profile_*, TokenProfile) against the numpy restatement in
token_profile_ref.py.  Everything is integer arithmetic, and the scores are one fixed operation sequence each: every
comparison is array_equal (the f32 values by their bits); there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import fakes
import token_profile_ref as ref
from test_token_profile_host import planted_profile, top_ref

pytestmark = pytest.mark.gpu

MSAE_EINVAL = -1
N, V, QUERIES, OFFSETS = 512, 97, (300, 7, 511, 0, 42), (-1, 0, 2)      # the base shape: F = 5, with B = 3, S = 37, k = 4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _batch(rng, B, S, k, n=N, v=V, hot_share=0.5):
    """[B, S, k] pairs and [B, S] ids: about `hot_share` of the entries name a query, a token's indices need not be distinct
    (a repeat counts twice); values over 2^-18 .. 2^17, some exactly 0, some negative."""
    idx = rng.integers(0, n, size=(B, S, k)).astype(np.int64)
    pick = rng.uniform(size=(B, S, k)) < hot_share
    idx[pick] = rng.choice(np.asarray(QUERIES), size=int(pick.sum()))
    vals = np.exp2(rng.uniform(-18, 17, size=(B, S, k))).astype(np.float32)
    u = rng.uniform(size=(B, S, k))
    vals[u < 0.05] = 0.0
    vals[u > 0.95] *= -1.0
    ids = rng.integers(0, v, size=(B, S)).astype(np.int64)
    return vals, idx, ids


def _run(calls, dev, mass=True, idx_dtype=torch.int64, ids_dtype=torch.int64, n=N, v=V, queries=QUERIES, offsets=OFFSETS, **kw):
    from msae.features import TokenProfile

    st = TokenProfile(n, list(queries), v, offsets=offsets, mass=mass, device=dev, **kw)
    for vals, idx, ids in calls:
        st.update(torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev).to(idx_dtype),
                  torch.from_numpy(ids).to(dev).to(ids_dtype))
    return st


def _assert_state(st, exp, mass=True):
    assert st.counts.dtype == torch.int32 and st.tok_count.dtype == torch.int64 and st.counts.shape == exp["counts"].shape
    assert np.array_equal(st.counts.cpu().numpy(), exp["counts"])
    assert np.array_equal(st.tok_count.cpu().numpy(), exp["tok_count"])
    if mass:
        assert st.mass.dtype == torch.int64 and np.array_equal(st.mass.cpu().numpy().view(np.uint64), exp["mass"])
    else:
        assert st.mass is None
    assert (st.n_rows, st.n_positions) == (exp["n_rows"], exp["n_positions"])


def _same(a, b):
    return (torch.equal(a.counts, b.counts) and torch.equal(a.tok_count, b.tok_count)
            and (a.mass is None) == (b.mass is None) and (a.mass is None or torch.equal(a.mass, b.mass))
            and (a.n_rows, a.n_positions) == (b.n_rows, b.n_positions))


# ---- the update: the base shape, every width -----------------------------------------------------------------------------------
def _case_base():
    """B = 3, S = 37, k = 4.  Query 7 fires at EVERY position (slot 0, value 1.5); special values sit on query 42 in slot 1 of
    the first positions; hostile list indices (-7, 2^31 - 1, N) carry ordinary values; ids outside [0, V) and negative ids sit
    at row ends and in the middle, so that every offset meets them."""
    rng = np.random.default_rng(200)
    B, S, k = 3, 37, 4
    vals, idx, ids = _batch(rng, B, S, k)
    idx[:, :, 0], vals[:, :, 0] = 7, 1.5
    f = np.float32
    specials = [np.nan, -1.0, 0.0, -0.0, 1e-5, 9e-6, np.nextafter(f(1e-5), f(1)), 2.0 ** -21, 1.0, 3.0 + 2.0 ** -21, 2.0 ** 40, np.inf,
                -np.inf, 1e-40]
    for i, x in enumerate(specials):
        vals[0, i, 1], idx[0, i, 1] = x, 42
    idx[1, 3, 2], idx[1, 4, 3], idx[1, 5, 1] = -7, 2 ** 31 - 1, N
    vals[1, 3:6, 1:] = 2.0
    ids[0, 0], ids[0, 36], ids[1, 1], ids[1, 17], ids[2, 35], ids[2, 20] = V, -1, V + 1000, -5, 2 ** 31 - 1, -2 ** 31
    return vals, idx, ids


_BASE_REF = {}


def _base_ref():
    if "st" not in _BASE_REF:
        _BASE_REF["st"] = ref.run([_case_base()], N, QUERIES, V, OFFSETS)
    return _BASE_REF["st"]


@pytest.mark.parametrize("mass", [True, False])
@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64])
def test_base_shape_every_width(dev, idx_dtype, ids_dtype, mass):
    exp = _base_ref()
    st = _run([_case_base()], dev, mass=mass, idx_dtype=idx_dtype, ids_dtype=ids_dtype)
    _assert_state(st, exp, mass)
    c = exp["counts"]
    # query 7 (slot 1) fires everywhere: its row of plane 0 is the token histogram of the positions inside the vocabulary
    assert c[1, 1].sum() >= 3 * 37 - 6 and np.array_equal(c[1, 1] >= exp["tok_count"][1], np.ones(V, bool))
    assert exp["tok_count"][1].sum() == 3 * 37 - 6 and exp["tok_count"][0].sum() < 3 * 36 and exp["tok_count"][2].sum() < 3 * 35
    assert c.sum() > 0 and (c[0] != c[1]).any() and (c[2] != c[1]).any()


def test_ids_wider_than_32_bits_are_counted_nowhere(dev):
    """An int64 id of 2^32 + 5 must not alias token 5 (the check is made on all 64 bits)."""
    vals, idx, ids = _case_base()
    ids = ids.copy()
    ids[1, 10], ids[2, 3] = 2 ** 32 + 5, -(2 ** 32) + 5
    _assert_state(_run([(vals, idx, ids)], dev), ref.run([(vals, idx, ids)], N, QUERIES, V, OFFSETS))


def test_hot_cell_one_token_everywhere(dev):
    """Every id is token 11 and query 7 fires at every position: one cell per plane takes every add of the workgroup."""
    vals, idx, ids = _case_base()
    ids = np.full_like(ids, 11)
    exp = ref.run([(vals, idx, ids)], N, QUERIES, V, OFFSETS)
    st = _run([(vals, idx, ids)], dev)
    _assert_state(st, exp)
    assert exp["tok_count"][:, 11].tolist() == [3 * 36, 3 * 37, 3 * 35] and exp["counts"][:, 1, 11].min() >= 3 * 35
    assert int(st.counts.sum()) == int(st.counts[:, :, 11].sum())


def test_a_strided_view_of_a_wider_list(dev):
    """The [:, :, :k] view of a list of 2 k slots (not contiguous) gives what its copy gives."""
    from msae.features import TokenProfile

    rng = np.random.default_rng(201)
    vals, idx, ids = _batch(rng, 3, 37, 8)
    tv, ti, tt = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(ids).to(dev)
    st = TokenProfile(N, list(QUERIES), V, offsets=OFFSETS, mass=True, device=dev)
    assert not tv[:, :, :4].is_contiguous()
    st.update(tv[:, :, :4], ti[:, :, :4], tt)
    _assert_state(st, ref.run([(vals[:, :, :4], idx[:, :, :4], ids)], N, QUERIES, V, OFFSETS))


# ---- rows that straddle workgroup chunks; cuts and merges ------------------------------------------------------------------------
def _case_large():
    rng = np.random.default_rng(202)
    return _batch(rng, 2, 300, 32, hot_share=0.6)


def test_rows_straddle_workgroup_chunks(dev):
    """B = 2, S = 300, k = 32: a workgroup takes 1024 entries = 32 positions, so a row border falls inside a chunk (300 is no
    multiple of 32) and one chunk holds hundreds of distinct cells."""
    vals, idx, ids = _case_large()
    exp = ref.run([(vals, idx, ids)], N, QUERIES, V, OFFSETS)
    st = _run([(vals, idx, ids)], dev)
    _assert_state(st, exp)
    assert (exp["counts"] > 0).sum() > 1000 and exp["tok_count"].sum(axis=1).tolist() == [2 * 299, 2 * 300, 2 * 298]
    _assert_state(_run([(vals, idx, ids)], dev, mass=False, idx_dtype=torch.int32, ids_dtype=torch.int32), exp, mass=False)


def test_cut_and_merge_invariance(dev):
    vals, idx, ids = _case_base()
    one = _run([(vals, idx, ids)], dev)
    cuts = [(vals[b:b + 1], idx[b:b + 1], ids[b:b + 1]) for b in range(3)]
    assert _same(one, _run(cuts, dev)) and _same(one, _run(cuts[::-1], dev))
    a, b = _run(cuts[:1], dev), _run(cuts[1:], dev)
    assert a.merge(b) is a and _same(one, a)
    _assert_state(a, _base_ref())
    lv, li, lt = _case_large()
    big = _run([(lv, li, lt)], dev)
    halves = _run([(lv[:1], li[:1], lt[:1])], dev).merge(_run([(lv[1:], li[1:], lt[1:])], dev))
    assert _same(big, halves)


# ---- no host synchronisation ----------------------------------------------------------------------------------------------------
def test_no_host_sync_and_no_allocation_growth(dev):
    vals, idx, ids = _case_base()
    tv, ti, tt = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(ids).to(dev)
    st = _run([], dev)
    st.update(tv, ti, tt)                            # first call: library load, the slot table
    st.top_tokens(m=10, by="precision", offset=2)
    torch.cuda.synchronize()
    before = torch.cuda.memory_reserved(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            st.update(tv, ti, tt)
        val, tok, tot = st.top_tokens(m=10, by="precision", offset=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_reserved(dev) == before
    exp = ref.run([(vals, idx, ids)] * 4, N, QUERIES, V, OFFSETS)
    _assert_state(st, exp)
    rv, rt, rtot = ref.top_tokens(exp["counts"][2], exp["mass"][2], exp["tok_count"][2], 10, "precision", 1)
    assert np.array_equal(val.cpu().numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(tok.cpu().numpy(), rt)
    assert np.array_equal(tot.cpu().numpy(), rtot)


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------------------
def test_einval_through_the_c_abi_leaves_the_state_alone(dev):
    import ctypes

    from msae import _hip

    lib = _hip.load()
    P_ = _hip.ptr
    vals, idx, ids = _case_base()
    tv, ti, tt = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, torch.int32), torch.from_numpy(ids).to(dev)
    slot_of = torch.full((N,), -1, dtype=torch.int32, device=dev)
    counts = torch.full((3, 5, V), -7, dtype=torch.int32, device=dev)
    mass = torch.full((3, 5, V), -7, dtype=torch.int64, device=dev)
    tok = torch.full((3, V), -7, dtype=torch.int64, device=dev)
    st = _hip.stream_of(tv)

    def call(B=3, S=37, k=4, n=N, F=5, v=V, offs=(-1, 0, 2), bits=64, ids_t=tt, counts_t=counts):
        arr = (ctypes.c_int32 * max(len(offs), 1))(*offs) if offs is not None else None
        return lib.msae_token_profile_update(P_(tv), P_(ti), P_(ids_t), bits, B, S, k, 1e-5, n, P_(slot_of), F, v, arr,
                                             len(offs) if offs is not None else 1, P_(counts_t), P_(mass), P_(tok), st)

    for kw in (dict(B=-1), dict(B=2, S=32769), dict(k=0), dict(k=257), dict(n=0), dict(n=262145), dict(F=0), dict(F=16385),
               dict(v=0), dict(F=16384, v=65536), dict(offs=()), dict(offs=(0, 1, 2, 3, 4)), dict(offs=(0, 0)), dict(offs=(65,)),
               dict(offs=(0, -65)), dict(offs=None), dict(bits=16), dict(ids_t=None), dict(counts_t=None)):
        assert call(**kw) == MSAE_EINVAL, kw
    val = torch.empty(5, 10, dtype=torch.float32, device=dev)
    tk = torch.empty(5, 10, dtype=torch.int32, device=dev)
    tot = torch.empty(5, dtype=torch.int64, device=dev)
    top = lambda F=5, v=V, m=10, metric=0, mc=1, ms=mass: lib.msae_token_profile_topk(
        P_(counts[0]), None if ms is None else P_(ms[0]), P_(tok[0]), F, v, m, metric, mc, P_(val), P_(tk), P_(tot), st)
    for kw in (dict(F=0), dict(F=16385), dict(v=0), dict(m=0), dict(m=65), dict(metric=3), dict(metric=-1), dict(mc=0),
               dict(metric=2, ms=None)):
        assert top(**kw) == MSAE_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((mass == -7).all()) and bool((tok == -7).all())


# ---- top tokens: the kernel against the torch path and the restatement ------------------------------------------------------------
@pytest.mark.parametrize("metric", ["count", "precision", "mean"])
@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("V_", [97, 5000])
def test_top_tokens_kernel_equals_torch_path_and_restatement(dev, V_, min_count, metric):
    st, *_ = planted_profile(V_, device=dev)
    host, *_ = planted_profile(V_)
    for offset, plane in ((0, 0), (-1, 1)):
        for m in (1, 10, 64):
            val, tk, tot = st.top_tokens(m=m, by=metric, offset=offset, min_count=min_count)
            assert val.is_cuda and val.dtype == torch.float32 and tk.dtype == torch.int32 and tot.dtype == torch.int64
            rv, rt, rtot = top_ref(V_, plane, m, metric, min_count)
            assert np.array_equal(val.cpu().numpy().view(np.uint32), rv.view(np.uint32)), (offset, m)
            assert np.array_equal(tk.cpu().numpy(), rt) and np.array_equal(tot.cpu().numpy(), rtot)
            hv, ht, htot = host.top_tokens(m=m, by=metric, offset=offset, min_count=min_count)
            assert torch.equal(val.cpu().view(torch.int32), hv.view(torch.int32)) and torch.equal(tk.cpu(), ht)
            assert torch.equal(tot.cpu(), htot)
    sv, stk, stot = st.top_tokens(m=10, by=metric, min_count=min_count, features=[9, 17])
    val, tk, tot = st.top_tokens(m=10, by=metric, min_count=min_count)
    assert torch.equal(sv, val[[3, 0]]) and torch.equal(stk, tk[[3, 0]]) and torch.equal(stot, tot[[3, 0]])


def test_top_tokens_of_a_row_longer_than_the_candidate_buffer(dev):
    """V = 5000 with EVERY token a candidate, scores ascending along the row: the buffer fills and is cut back four times, and
    each time all of its old keys lose against the new ones."""
    from msae.features import TokenProfile

    Vb = 5000
    st = TokenProfile(8, [3, 5], Vb, device=dev)
    c = torch.stack([torch.arange(1, Vb + 1), torch.arange(Vb, 0, -1)]).to(torch.int32)
    st.counts.copy_(c[None].to(dev))
    st.tok_count.fill_(Vb)
    val, tk, tot = st.top_tokens(m=64, by="count")
    assert tk[0].tolist() == list(range(Vb - 1, Vb - 65, -1)) and tk[1].tolist() == list(range(64))
    assert val[0].tolist() == [float(Vb - i) for i in range(64)] and tot.tolist() == [Vb * (Vb + 1) // 2] * 2
    hv, ht, htot = TokenProfile.top_tokens(_cpu_copy(st), m=64, by="count")
    assert torch.equal(val.cpu(), hv) and torch.equal(tk.cpu(), ht) and torch.equal(tot.cpu(), htot)


def _cpu_copy(st):
    from msae.features import TokenProfile

    out = TokenProfile(st.num_latents, st.queries.cpu(), st.vocab_size, offsets=st.offsets, mass=st.has_mass, thresh=st.thresh)
    out.counts.copy_(st.counts)
    out.tok_count.copy_(st.tok_count)
    if st.has_mass:
        out.mass.copy_(st.mass)
    return out


# ---- the caches -------------------------------------------------------------------------------------------------------------------
def test_cache_add_topk_sequence(dev):
    """`Cache.add_topk(..., token_ids=)` over three batches: the module's profile equals the restatement; the queries default to
    the filter list; with tokens=None no profile is created."""
    from msae.features import Cache

    rng = np.random.default_rng(203)
    calls = [_batch(rng, 2, 19, 4) for _ in range(3)]
    filters = {"m": torch.tensor(QUERIES, device=dev)}
    on = Cache(0, filters, batch_size=2, tokens=dict(vocab_size=V, offsets=OFFSETS, mass=True))
    off = Cache(0, filters, batch_size=2)
    for n, (vals, idx, ids) in enumerate(calls):
        tv, ti, tt = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev), torch.from_numpy(ids).to(dev)
        on.add_topk(tv, ti, N, n, "m", token_ids=tt)
        off.add_topk(tv, ti, N, n, "m", token_ids=tt)          # given and ignored
        off.add_topk(tv, ti, N, n + 3, "m")
    assert off.token_profiles == {} and off.tokens is None and list(on.token_profiles) == ["m"]
    _assert_state(on.token_profiles["m"], ref.run(calls, N, QUERIES, V, OFFSETS))
    with pytest.raises(ValueError, match="token_ids"):
        on.add_topk(tv, ti, N, 9, "m")
    on.flush_pending(); off.flush_pending()


def _files(root):
    return {f: (root / f).read_bytes() for f in sorted(os.listdir(root))}


def test_text_cache_end_to_end(dev, tmp_path):
    """A FeatureCache run over token batches on the stand-in model with tokens on: token_profile.safetensors equals the
    restatement fed every batch's top-k and input ids; with tokens=None the same run writes nothing of it and every other
    file is byte-identical."""
    from msae import Sae, SaeConfig
    from msae.features import FeatureCache, TokenProfile

    d, n, module, vocab = 64, 4096, "layers.1", 40
    rng = np.random.default_rng(204)
    dataset = [{"input_ids": torch.from_numpy(rng.integers(0, vocab, size=7))} for _ in range(6)]
    queries = list(range(0, n, 3))
    outs, seen = {}, []
    for on in (False, True):
        torch.manual_seed(12)
        sae = Sae(d, SaeConfig(num_latents=n, k=16), device=dev)
        model = fakes.TinyLlava(vocab=vocab, d=d).to(dev)
        fc = FeatureCache(model, None, {module: sae}, batch_size=2, shard_size=0,
                          tokens=dict(vocab_size=vocab - 2, queries=queries, offsets=(0, 1), mass=True) if on else None)
        if on:
            inner = fc.cache.add_topk

            def spy(top_acts, top_indices, *a, token_ids=None, **kw):
                seen.append((top_acts.float().cpu().numpy(), top_indices.cpu().numpy(), token_ids.cpu().numpy()))
                return inner(top_acts, top_indices, *a, token_ids=token_ids, **kw)

            fc.cache.add_topk = spy
        fc.run(7, dataset)
        out = tmp_path / ("on" if on else "off")
        fc.save_splits(n_splits=2, save_dir=str(out), rank=0)
        if on:
            assert "Rank0_token_profile.safetensors" in os.listdir(out / module)
        fc.concate_safetensors(n_splits=2, save_dir=str(out))
        outs[on] = _files(out / module)
        assert (fc.cache.token_profiles == {}) == (not on)
    assert sorted(outs[True]) == sorted(list(outs[False]) + ["token_profile.safetensors"])
    assert all(outs[True][f] == outs[False][f] for f in outs[False])
    st = TokenProfile.load(str(tmp_path / "on" / module / "token_profile.safetensors"))
    assert st.device.type == "cpu" and st.offsets == (0, 1) and st.vocab_size == vocab - 2 and st.has_mass
    assert len(seen) == 3 and all(np.array_equal(s[2], np.stack([dataset[2 * i]["input_ids"].numpy(),
                                                                dataset[2 * i + 1]["input_ids"].numpy()]))
                                  for i, s in enumerate(seen))
    exp = ref.run(seen, n, queries, vocab - 2, (0, 1))
    _assert_state(st, exp)
    assert exp["counts"].sum() > 0 and exp["n_positions"] == 6 * 7 and exp["tok_count"][0].sum() <= 42
    val, tk, tot = st.top_tokens(m=5, by="mean")                 # a loaded file, on the CPU
    rv, rt, rtot = ref.top_tokens(exp["counts"][0], exp["mass"][0], exp["tok_count"][0], 5, "mean", 1)
    assert np.array_equal(val.numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(tk.numpy(), rt)
    assert np.array_equal(tot.numpy(), rtot)
