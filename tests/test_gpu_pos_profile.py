"""GPU: position profiles and their summary (msae_pos_profile_*, PosProfile) against the numpy restatement in
pos_profile_ref.py.  Everything is integer arithmetic: every comparison is array_equal; there is no tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fakes
import guarded_ws
import pos_profile_ref as ref
import synth

pytestmark = pytest.mark.gpu

N_C2, T_C2, K_C2 = 131072, 8192, 32
WG_ENTRIES = 1024                  # entries a workgroup of the update takes (csrc/pos_profile.hip: PP_ENTRIES)
MSAE_EINVAL, MSAE_EWS = -1, -3


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _topk(rng, B, S, k, N, reserved=(), positive=False):
    """[B, S, k] pairs: a token's indices distinct and outside `reserved`; values over 2^-18 .. 2^17, some exactly 0, some
    negative (unless `positive`)."""
    pool = np.setdiff1d(np.arange(N), np.asarray(reserved, np.int64))
    idx = np.stack([rng.choice(pool, size=k, replace=False) for _ in range(B * S)]).reshape(B, S, k).astype(np.int64)
    vals = np.exp2(rng.uniform(-18, 17, size=(B, S, k))).astype(np.float32)
    if not positive:
        u = rng.uniform(size=(B, S, k))
        vals[u < 0.05] = 0.0
        vals[u > 0.95] *= -1.0
    return vals, idx


def _run(calls, N, bins, dev, index_dtype=torch.int64, value_dtype=None, **kw):
    from msae.features import PosProfile

    table, tail, P = bins
    st = PosProfile(N, table, tail, P, device=dev, **kw)
    for vals, idx in calls:
        v = torch.from_numpy(vals).to(dev)
        st.update(v if value_dtype is None else v.to(value_dtype), torch.from_numpy(idx).to(dev).to(index_dtype))
    return st


def _ref(calls, N, bins, wide=False, **kw):
    table, tail, P = bins
    return ref.run(calls, N, np.asarray(table), tail, P, wide=wide, **kw)


def _assert_state(st, exp):
    assert st.count.dtype == torch.int32 and st.mass.dtype == torch.int64 and st.count.shape == exp["count"].shape
    assert np.array_equal(st.count.cpu().numpy(), exp["count"])
    assert np.array_equal(st.mass.cpu().numpy().view(np.uint64), exp["mass"])
    assert np.array_equal(st.bin_positions.numpy(), exp["bin_positions"])
    assert (st.n_rows, st.n_positions) == (exp["n_rows"], exp["n_positions"])


def _same(a, b):
    return (torch.equal(a.count, b.count) and torch.equal(a.mass, b.mass) and torch.equal(a.bin_positions, b.bin_positions)
            and (a.n_rows, a.n_positions) == (b.n_rows, b.n_positions))


# ---- special values ---------------------------------------------------------------------------------------------------------
def _specials():
    f = np.float32
    return np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -2.0, -1e-3,           # 0 .. 6: counted nowhere
                     1e-40, 1.1754944e-38,                                      # 7, 8: a denormal, the smallest normal
                     1e-5, np.nextafter(f(1e-5), f(1)),                         # 9, 10: thresh itself (dropped), just above
                     2.0 ** -21, 3 * 2.0 ** -21, 1.0, 1.0 + 2.0 ** -23, 3.0 + 2.0 ** -21,          # 11 .. 15: ties and neighbours
                     np.nextafter(f(2.0 ** 40), f(0)), 2.0 ** 40, 3e38], np.float32)               # 16 .. 18: the saturation


SPECIAL_BINS = ([0, 1, 2, -1, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5], 6, 7)     # L = 20 < S = 37: the tail bin is used


def _case_special(k, bf16=False):
    """B = 3, S = 37, N = 1000.  Special value i sits alone on feature 900 + i, in slot i % k of token 2 i + 1 (positions 1, 3
    -- which has no bin --, 5, .. and, from token 37 on, of the next row); the indices -1, N and 2^31 - 1 carry ordinary
    values; with k >= 2 feature 890 is named twice by token 100 (it counts twice)."""
    rng = np.random.default_rng(50 + k)
    B, S, N = 3, 37, 1000
    vals, idx = _topk(rng, B, S, k, N, reserved=np.arange(890, 1000))
    sp = _specials()
    v2, i2 = vals.reshape(B * S, k), idx.reshape(B * S, k)
    for i, x in enumerate(sp):
        v2[2 * i + 1, i % k], i2[2 * i + 1, i % k] = x, 900 + i
    v2[81, 0], i2[81, 0] = 1.0, -1
    v2[83, k - 1], i2[83, k - 1] = 1.0, N
    v2[85, k // 2], i2[85, k // 2] = 1.0, 2 ** 31 - 1
    if k >= 2:
        v2[100, 0], i2[100, 0], v2[100, k - 1], i2[100, k - 1] = 1.0, 890, 3.0, 890
    if bf16:
        vals = torch.from_numpy(vals).to(torch.bfloat16).to(torch.float32).numpy()
    return vals, idx, N


_SPECIAL_REF = {}


@pytest.mark.parametrize("k", [1, 32, 37, 256])
@pytest.mark.parametrize("variant", ["int32", "int64", "bf16"])
def test_special_values(dev, k, variant):
    bf16 = variant == "bf16"
    vals, idx, N = _case_special(k, bf16)
    if (k, bf16) not in _SPECIAL_REF:
        _SPECIAL_REF[k, bf16] = _ref([(vals, idx)], N, SPECIAL_BINS)
    exp = _SPECIAL_REF[k, bf16]
    st = _run([(vals, idx)], N, SPECIAL_BINS, dev, index_dtype=torch.int32 if variant == "int32" else torch.int64,
              value_dtype=torch.bfloat16 if bf16 else None)
    _assert_state(st, exp)
    assert exp["n_positions"] == 3 * 37 and exp["bin_positions"].tolist() == [3, 3, 3, 12, 24, 12, 51]
    c, m = exp["count"], exp["mass"]
    if not bf16:
        assert c[900:911].sum() == 1 and c[910].sum() == 1 and int(m[910].sum()) == 10        # only "just above thresh" of 0 .. 10
        assert [int(c[900 + i].sum()) for i in range(11, 19)] == [0, 0] + [1] * 6          # 2^-21 and 3 * 2^-21: below thresh
        assert [int(m[900 + i].sum()) for i in range(13, 19)] == [1 << 20, 1 << 20, 3 << 20, (1 << 60) - (1 << 36), 1 << 60,
                                                                  1 << 60]
        assert c[901].sum() == 0                     # +inf sits on token 3: the position without a bin
        assert c[910, 6] == 1 and c[918, 0] == 1     # position 21: the tail bin; token 37 is position 0 of row 1: bin 0
    if k >= 2:
        assert c[890].sum() == 2 and int(m[890].sum()) == 4 << 20              # the repeat counts twice


@pytest.mark.parametrize("thresh", [0.0, -1.0])
def test_special_values_with_a_threshold_at_or_below_zero(dev, thresh):
    """thresh = 0 keeps the denormal and the smallest normal (count 1, mass 0); thresh < 0 lets the zeros through the keep rule
    as well, and they are still counted nowhere (v > 0, not v >= 0)."""
    vals, idx, N = _case_special(32)
    exp = _ref([(vals, idx)], N, SPECIAL_BINS, thresh=thresh)
    _assert_state(_run([(vals, idx)], N, SPECIAL_BINS, dev, thresh=thresh), exp)
    c, m = exp["count"], exp["mass"]
    assert c[907].sum() == 1 and c[908].sum() == 1 and c[909].sum() == 1 and m[907].sum() == 0 and m[908].sum() == 0
    assert c[911].sum() == 1 and m[911].sum() == 0 and c[912].sum() == 1 and m[912].sum() == 2       # the ties, to even
    assert c[900:907].sum() == 0                     # NaN, -0.0, 0.0 and the negatives: nowhere (+inf has no bin here)
    wrong = _ref([(vals, idx)], N, SPECIAL_BINS, thresh=thresh, mutant="ge")
    assert np.array_equal(wrong["count"], c) == (thresh == 0.0)


def test_restatement_mistakes_are_rejected_on_the_device_state(dev):
    vals, idx, N = _case_special(32)
    st = _run([(vals, idx)], N, SPECIAL_BINS, dev)
    wrong = _ref([(vals, idx)], N, SPECIAL_BINS, mutant="lookup")
    assert not np.array_equal(st.count.cpu().numpy(), wrong["count"])


# ---- table edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tail", "long_table", "no_tail", "all_minus_one", "one_bin", "1024_bins"])
def test_table_edges(dev, case):
    rng = np.random.default_rng(60)
    B, S, k, N = 4, 50, 8, 257
    vals, idx = _topk(rng, B, S, k, N)
    lin = lambda L, P: (np.arange(L) * P // L).tolist()
    bins = {"tail": (lin(20, 5), 5, 6),                      # L < S: positions 20 .. 49 fall into the tail bin
            "long_table": (lin(300, 7), 3, 7),               # L > S: the tail bin is never used
            "no_tail": (lin(20, 5), -1, 5),                  # positions past the table are counted nowhere
            "all_minus_one": ([-1] * 64, -1, 3),
            "one_bin": ([0] * 10 + [-1] * 10, 0, 1),
            "1024_bins": (lin(50, 1024), -1, 1024)}[case]
    exp = _ref([(vals, idx)], N, bins, wide=True)
    st = _run([(vals, idx)], N, bins, dev)
    _assert_state(st, exp)
    total = int(exp["count"].sum())
    if case == "all_minus_one":
        assert total == 0 and int(st.mass.abs().sum()) == 0 and exp["bin_positions"].sum() == 0 and st.n_positions == B * S
    else:
        assert total > 0
    if case == "tail":
        assert exp["count"][:, 5].sum() > 0 and exp["bin_positions"][5] == B * 30
    if case == "no_tail":
        assert np.array_equal(exp["count"], _ref([(vals, idx)], N, (bins[0], 5, 6), wide=True)["count"][:, :5])
    if case == "1024_bins":
        assert (exp["count"].sum(axis=0) > 0).sum() == 50 and exp["count"][:, 1023].sum() == 0
    fired, peak = st.summary()
    rf, rp = ref.summary(exp["count"], exp["bin_positions"])
    assert np.array_equal(fired.cpu().numpy(), rf) and np.array_equal(peak.cpu().numpy(), rp)


@pytest.mark.parametrize("k", [32, 37])
@pytest.mark.parametrize("dS", [-1, 0, 1])
def test_rows_around_a_workgroups_share(dev, k, dS):
    """A workgroup takes 1024 consecutive entries -- 32 tokens at k = 32; at k = 37 its borders fall inside a token.  Rows one
    shorter and one longer than that share put every row border at a different place of a workgroup."""
    rng = np.random.default_rng(61)
    B, S, N = 7, WG_ENTRIES // 32 + dS, 300
    vals, idx = _topk(rng, B, S, k, N)
    bins = ((np.arange(S - 2) % 5).tolist(), 5, 6)
    exp = _ref([(vals, idx)], N, bins, wide=True)
    _assert_state(_run([(vals, idx)], N, bins, dev), exp)
    assert exp["count"][:, 5].sum() > 0 and B * S * k > 6 * WG_ENTRIES


# ---- contention -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [1, 36])
def test_contention_one_feature_on_every_token(dev, spread):
    """T = 8192, k = 32: feature 7 with the value 1.5 on every token -- into one bin (as a BOS-like
    feature puts every row's entry into one cell), or spread over 36 bins (a dense feature on a 36-cell grid)."""
    rng = np.random.default_rng(62)
    B, S, k, N = 32, 256, 32, 4096
    vals, idx = _topk(rng, B, S, k, N, reserved=(7,), positive=True)
    idx[:, :, 11], vals[:, :, 11] = 7, 1.5
    bins = ([0] * S, -1, 1) if spread == 1 else ((np.arange(S) % 36).tolist(), -1, 36)
    exp = _ref([(vals, idx)], N, bins, wide=True)
    st = _run([(vals, idx)], N, bins, dev)
    _assert_state(st, exp)
    row = st.count[7].cpu().numpy()
    assert row.sum() == B * S and int(st.mass[7].sum()) == B * S * (3 << 19)
    if spread == 1:
        assert row.tolist() == [B * S]
    else:
        per = np.bincount(np.asarray(bins[0]), minlength=36) * B
        assert np.array_equal(row, per) and (per > 0).all() and per.sum() == B * S


def test_mass_wraps_mod_2_64(dev):
    """16 entries of +inf in one cell: 16 * 2^60 = 0 mod 2^64 (count 16); 5 entries: 5 * 2^60, beyond 2^63."""
    for n, want in ((16, 0), (5, 5 << 60)):
        vals = np.full((n, 1, 1), np.inf, np.float32)
        idx = np.full((n, 1, 1), 2, np.int64)
        st = _run([(vals, idx)], 4, ([0], -1, 1), dev)
        _assert_state(st, _ref([(vals, idx)], 4, ([0], -1, 1)))
        assert int(st.count[2, 0]) == n and int(st.mass[2, 0].cpu().numpy().view(np.uint64)) == want
        assert int(st.count.sum()) == n


# ---- cuts, merges, chunks ---------------------------------------------------------------------------------------------------
def test_cut_and_merge_invariance(dev):
    rng = np.random.default_rng(63)
    B, S, k, N = 9, 70, 32, 2048
    vals, idx = _topk(rng, B, S, k, N)
    bins = ((np.arange(48) // 7).tolist(), 7, 8)
    one = _run([(vals, idx)], N, bins, dev)
    cuts = [(vals[5:], idx[5:]), (vals[:2], idx[:2]), (vals[2:5], idx[2:5])]
    assert _same(one, _run(cuts, N, bins, dev))
    a, b = _run(cuts[:1], N, bins, dev), _run(cuts[1:], N, bins, dev)
    assert a.merge(b) is a and _same(one, a)
    _assert_state(one, _ref([(vals, idx)], N, bins, wide=True))
    fired, peak = a.summary()                        # the device copy of bin_positions is rebuilt after a merge
    rf, rp = ref.summary(a.count.cpu().numpy(), a.bin_positions.numpy())
    assert np.array_equal(fired.cpu().numpy(), rf) and np.array_equal(peak.cpu().numpy(), rp)


@pytest.mark.parametrize("B,S", [(2, 65536), (3, 65535), (3, 32769)])
def test_update_chunks_at_the_call_envelope(dev, B, S):
    """Rows of (nearly) a whole call's positions: one update cuts them into calls of one row (two rows never fit), with a
    table of 65536 positions and 1024 bins -- the same bits as one update per row, in another order."""
    rng = np.random.default_rng(64)
    k, N = 1, 8
    idx = rng.integers(0, N, size=(B, S, k)).astype(np.int64)
    vals = np.exp2(rng.uniform(-6, 6, size=(B, S, k))).astype(np.float32)
    bins = ((np.arange(65536) // 64).tolist(), -1, 1024)
    one = _run([(vals, idx)], N, bins, dev)
    rows = _run([(vals[b:b + 1], idx[b:b + 1]) for b in reversed(range(B))], N, bins, dev)
    assert _same(one, rows)
    _assert_state(one, _ref([(vals, idx)], N, bins, wide=True))
    assert int(one.count.sum()) == B * S and int(one.count[:, (S - 1) // 64].sum()) == B * ((S - 1) % 64 + 1)


# ---- production width -------------------------------------------------------------------------------------------------------
def _c2_pairs():
    """[8192, 32] pairs at N = 131072 from synth's counter-based streams: feature ids concentrated on the low ids (a cube
    law, so features recur; a token may repeat one -- it counts twice), positive values."""
    u = np.abs(synth.normalish(77, T_C2 * K_C2)) / np.float32(3.47)
    idx = np.minimum((u.astype(np.float64) ** 3 * N_C2).astype(np.int64), N_C2 - 1).reshape(T_C2, K_C2)
    vals = (np.abs(synth.normalish(78, T_C2 * K_C2)) + np.float32(0.01)).reshape(T_C2, K_C2)
    return vals, idx


def test_production_width_image_rows(dev):
    """N = 131072, k = 32, two rows of 2880 positions, the image launcher's default bins (24 x 24 grid in cells of 4, and the
    rest): the update against the restatement; the summary kernel over all features against `summary_host`, and against the
    restatement on the hot low ids and every 37th row."""
    from msae.features import PosProfile
    from msae.features.pos import summary_host

    vals, idx = (a[:5760].reshape(2, 2880, K_C2) for a in _c2_pairs())
    table, tail, P, _ = PosProfile.grid_bins()
    bins = (table.tolist(), tail, P)
    exp = _ref([(vals, idx)], N_C2, bins, wide=True)
    st = _run([(vals, idx)], N_C2, bins, dev)
    _assert_state(st, exp)
    assert exp["count"].sum() == 5760 * K_C2 and exp["bin_positions"].tolist() == [32] * 36 + [4608]
    fired, peak = st.summary()
    assert fired.dtype == torch.int64 and peak.dtype == torch.int32 and fired.shape == (N_C2,) and peak.shape == (N_C2, 2)
    hf, hp = summary_host(st.count, st.bin_positions)
    assert torch.equal(fired.cpu(), hf) and torch.equal(peak.cpu(), hp)
    rows = np.unique(np.concatenate([np.arange(2048), np.arange(0, N_C2, 37), [N_C2 - 1]]))
    rf, rp = ref.summary(exp["count"][rows], exp["bin_positions"])
    assert np.array_equal(fired.cpu().numpy()[rows], rf) and np.array_equal(peak.cpu().numpy()[rows], rp)
    assert (rf > 0).sum() > 2000 and (rp[:, 0] == 36).any() and (rp[:, 0] < 36).any() and (rp[:, 0] == -1).any()


# ---- the summary kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5, 37, 64, 65, 1000, 1024])
def test_summary_kernel(dev, P):
    """Fewer bins than lanes, exactly a wave's, one more, and 16 rounds; rate ties inside a lane, across lanes and across
    rounds; empty rows; bins without positions; counts and positions up to 2^31 - 1."""
    from msae.features import PosProfile
    from msae.features.pos import summary_host

    rng = np.random.default_rng(65 + P)
    N = 203
    bp = rng.integers(1, 1 << 31, size=P).astype(np.int64)
    count = (rng.integers(0, 1 << 31, size=(N, P)) * (rng.uniform(size=(N, P)) < 0.2)).astype(np.int32)
    count[0] = 0
    if P >= 5:
        bp[rng.choice(P, size=P // 5, replace=False)] = 0
        on = np.flatnonzero(bp > 0)
        bp[on[: len(on) // 2]] = 1000                    # many bins of one size: equal counts there tie
        count[1] = 0; count[1, on[: len(on) // 2]] = 77  # a tie across all of them: the lowest bin
        count[2] = 7                                     # every bin 7: the smallest bin with positions wins, ties to the lowest
        count[3] = 0; count[3, np.flatnonzero(bp == 0)] = 5       # counts only where no position fell
    count[N - 1] = (1 << 31) - 1
    st = PosProfile(N, [0], n_bins=P, device=dev)
    st.count.copy_(torch.from_numpy(count))
    st.bin_positions.copy_(torch.from_numpy(bp))
    fired, peak = st.summary()
    rf, rp = ref.summary(count, bp)
    assert np.array_equal(fired.cpu().numpy(), rf) and np.array_equal(peak.cpu().numpy(), rp)
    hf, hp = summary_host(st.count, st.bin_positions)
    assert torch.equal(fired.cpu(), hf) and torch.equal(peak.cpu(), hp)
    assert rp[0].tolist() == [-1, 0]
    if P >= 5:
        assert rp[1].tolist() == [int(np.flatnonzero(bp == 1000)[0]), 77] and rp[3].tolist() == [-1, 0] and rf[3] > 0
        assert not np.array_equal(ref.summary(count, bp, mutant="count_peak")[1], rp)


# ---- no host synchronisation ------------------------------------------------------------------------------------------------
def test_no_host_sync_and_no_allocation_growth(dev):
    from msae.features import PosProfile

    rng = np.random.default_rng(66)
    B, S, k, N = 4, 96, 32, 4096
    vals, idx = _topk(rng, B, S, k, N)
    v, i = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev)
    table, tail, P, _ = PosProfile.grid_bins(8, 2)
    st = PosProfile(N, table, tail, P, device=dev)
    st.update(v, i)                                  # first call: library load, workspace, the row's positions per bin
    st.summary()
    torch.cuda.synchronize()
    before = torch.cuda.memory_reserved(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            st.update(v, i)
        fired, peak = st.summary()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_reserved(dev) == before
    exp = _ref([(vals, idx)] * 4, N, (table.tolist(), tail, P), wide=True)
    _assert_state(st, exp)
    rf, rp = ref.summary(exp["count"], exp["bin_positions"])
    assert np.array_equal(fired.cpu().numpy(), rf) and np.array_equal(peak.cpu().numpy(), rp)


# ---- the workspace contract -------------------------------------------------------------------------------------------------
_WS_ZERO = {}


@pytest.mark.parametrize("fill", guarded_ws.FILLS)
def test_update_under_guarded_workspaces(dev, monkeypatch, fill):
    """The update with ops._workspace replaced by the guarded, exact-size allocator: every request is what the sizing helper
    returns (0 bytes: a guarded block with no interior), the guards stay intact, the state equals the restatement and is the
    same bits under the three fills."""
    from msae import _hip, ops

    rng = np.random.default_rng(67)
    B, S, k, N = 3, 50, 8, 1000
    main, alt = _topk(rng, B, S, k, N), _topk(rng, B, S, k, N)
    bins = ((np.arange(40) // 9).tolist(), 5, 6)
    gws = guarded_ws.GuardedWorkspace(fill, dev)
    gws.what = f"msae_pos_profile_update B={B} S={S} k={k} N={N}"
    monkeypatch.setattr(ops, "_workspace", gws)
    if fill == "recycled":
        _run([alt], N, bins, dev)
        gws.check()
    st = _run([main], N, bins, dev)
    gws.check()
    assert gws.requests and {n for _, n in gws.requests} == {_hip.load().msae_pos_profile_ws_bytes(B * S, k, N)}
    _assert_state(st, _ref([main], N, bins, wide=True))
    got = (st.count.cpu(), st.mass.cpu())
    zero = _WS_ZERO.setdefault("state", got)
    assert torch.equal(got[0], zero[0]) and torch.equal(got[1], zero[1])


def test_workspace_refusal_and_helper_through_the_c_abi(dev):
    """The helper returns 0 for every shape the entry refuses.  For a shape it accepts, a workspace one byte short of the
    helper's result, and a missing one, are refused with MSAE_EWS before anything is written -- where the helper asks for
    bytes at all: this kernel keeps its table in LDS and the helper returns 0, so no workspace can be short, and the entry
    must then run with ws = NULL and with a guarded block of 0 bytes."""
    from msae import _hip

    lib = _hip.load()
    P_ = _hip.ptr
    for T, k, N in ((-1, 8, 100), (65537, 8, 100), (100, 0, 100), (100, 257, 100), (100, 8, 0), (100, 8, 262145)):
        assert lib.msae_pos_profile_ws_bytes(T, k, N) == 0
    rng = np.random.default_rng(68)
    B, S, k, N = 3, 50, 8, 1000
    vals, idx = _topk(rng, B, S, k, N)
    tv, ti = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, torch.int32)
    table = torch.tensor((np.arange(40) // 9).tolist(), dtype=torch.int32, device=dev)
    count = torch.full((N, 6), -7, dtype=torch.int32, device=dev)
    mass = torch.full((N, 6), -7, dtype=torch.int64, device=dev)
    st = _hip.stream_of(tv)
    call = lambda ws, n, B_=B, S_=S, k_=k, N_=N, L=40, tail=5, P=6: lib.msae_pos_profile_update(
        P_(tv), P_(ti), B_, S_, k_, 1e-5, N_, P_(table), L, tail, P, P_(count), P_(mass), ws, n, st)
    big = ctypes.c_void_p(tv.data_ptr())             # (never touched: the refusals come before any launch)
    for kw in (dict(B_=-1), dict(B_=2, S_=32769), dict(k_=0), dict(k_=257), dict(N_=0), dict(N_=262145), dict(L=0),
               dict(L=65537), dict(P=0), dict(P=1025), dict(tail=6), dict(tail=-2)):
        assert call(big, 1 << 40, **kw) == MSAE_EINVAL, kw
    need = lib.msae_pos_profile_ws_bytes(B * S, k, N)
    gws = guarded_ws.GuardedWorkspace("word3", dev)
    if need > 0:
        ptr, n, _ = gws.block(need - 1)
        assert call(ctypes.c_void_p(ptr), n) == MSAE_EWS and call(None, need) == MSAE_EWS
        gws.check()
    torch.cuda.synchronize()
    assert bool((count == -7).all()) and bool((mass == -7).all())              # every refusal left the state alone
    count.zero_(); mass.zero_()
    ptr, n, _ = gws.block(need)
    assert call(ctypes.c_void_p(ptr), n) == 0
    gws.check()
    if need == 0:
        assert call(None, 0) == 0
    exp = _ref([(vals, idx)] * (2 if need == 0 else 1), N, (table.tolist(), 5, 6), wide=True)
    assert np.array_equal(count.cpu().numpy(), exp["count"]) and np.array_equal(mass.cpu().numpy().view(np.uint64), exp["mass"])
    fired = torch.empty(N, dtype=torch.int64, device=dev)
    peak = torch.empty(N, 2, dtype=torch.int32, device=dev)
    bp = torch.ones(6, dtype=torch.int64, device=dev)
    for args in ((0, 6), (262145, 6), (N, 0), (N, 1025)):
        assert lib.msae_pos_profile_summary(P_(count), P_(bp), *args, P_(fired), P_(peak), st) == MSAE_EINVAL


def test_a_table_value_outside_the_bins_is_counted_nowhere(dev):
    """The C ABI cannot read the device table back: a value outside [0, P) counts as -1 and nothing is written out of bounds
    (the counters sit between guard rows)."""
    from msae import _hip

    lib = _hip.load()
    P_ = _hip.ptr
    rng = np.random.default_rng(69)
    B, S, k, N = 2, 6, 4, 50
    vals, idx = _topk(rng, B, S, k, N, positive=True)
    tv, ti = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, torch.int32)
    table = torch.tensor([0, 3, 1000, -5, 2, 1 << 30], dtype=torch.int32, device=dev)
    count = torch.zeros(N + 2, 3, dtype=torch.int32, device=dev)
    mass = torch.zeros(N + 2, 3, dtype=torch.int64, device=dev)
    assert lib.msae_pos_profile_update(P_(tv), P_(ti), B, S, k, 1e-5, N, P_(table), 6, -1, 3, P_(count[1:]), P_(mass[1:]), None, 0,
                                       _hip.stream_of(tv)) == 0
    exp = _ref([(vals, idx)], N, ([0, -1, -1, -1, 2, -1], -1, 3))
    assert np.array_equal(count[1:N + 1].cpu().numpy(), exp["count"]) and 0 < exp["count"].sum() <= 2 * B * k
    assert np.array_equal(mass[1:N + 1].cpu().numpy().view(np.uint64), exp["mass"])
    assert int(count[0].abs().sum()) == 0 and int(count[N + 1].abs().sum()) == 0 and int(mass[0].abs().sum()) == 0


# ---- the caches -------------------------------------------------------------------------------------------------------------
def _spy(cache, seen):
    inner = cache.add_topk

    def spy(top_acts, top_indices, *a, **kw):
        seen.append((top_acts.float().cpu().numpy(), top_indices.cpu().numpy()))
        return inner(top_acts, top_indices, *a, **kw)

    cache.add_topk = spy


def _files(root):
    return {f: (root / f).read_bytes() for f in sorted(os.listdir(root))}


def test_image_cache_end_to_end(dev, tmp_path, golden_dir):
    """A FeatureImageCache run over the fake images with pos on: pos_profile.safetensors equals the restatement over every
    batch's top-k; with pos=None the same run writes nothing of it and every other file is byte-identical."""
    from msae import Sae, SaeConfig
    from msae.config import parse_cache_config, pos_profile_kwargs
    from msae.features import FeatureImageCache, PosProfile

    g = np.load(golden_dir / "g9_image_cache.npz")
    images = [{"image": fakes.FakeImage(i)} for i in range(int(g["n_images"]))]
    module, d, N = str(g["module"]), int(g["d"]), 4096
    cfg = parse_cache_config(["model", "data", "--pos_profile", "--pos_profile_bins", "grid:2:1"])
    pos = pos_profile_kwargs(cfg, "grid:24:4", cfg.ctx_len)
    outs, seen = {}, []
    for on in (False, True):
        torch.manual_seed(11)
        sae = Sae(d, SaeConfig(num_latents=N, k=16), device=dev)
        model = fakes.TinyLlava(vocab=int(g["vocab"]), d=d).to(dev)
        fic = FeatureImageCache(model, None, {module: sae}, batch_size=2, shard_size=0,
                                processor=fakes.FakeProcessor(int(g["vocab"])), pos=pos if on else None)
        if on:
            _spy(fic.cache, seen)
        fic.run(0, images)
        out = tmp_path / ("on" if on else "off")
        fic.save_splits(n_splits=2, save_dir=str(out), rank=0)
        if on:
            assert "Rank0_pos_profile.safetensors" in os.listdir(out / module)
        fic.concate_safetensors(n_splits=2, save_dir=str(out))
        outs[on] = _files(out / module)
        assert (fic.cache.pos_profiles == {}) == (not on)
    assert sorted(outs[True]) == sorted(list(outs[False]) + ["pos_profile.safetensors"])
    assert all(outs[True][f] == outs[False][f] for f in outs[False])
    st = PosProfile.load(str(tmp_path / "on" / module / "pos_profile.safetensors"))
    assert st.table.tolist() == [0, 1, 2, 3] and (st.tail_bin, st.n_bins) == (4, 5) and st.device.type == "cpu"
    assert len(seen) == len(images) // 2
    exp = _ref(seen, N, ([0, 1, 2, 3], 4, 5))
    _assert_state(st, exp)
    assert exp["count"].sum() > 0 and exp["n_rows"] == len(images) // 2 * 2
    fired, peak = st.summary()                       # a loaded file, on the CPU
    rf, rp = ref.summary(exp["count"], exp["bin_positions"])
    assert np.array_equal(fired.numpy(), rf) and np.array_equal(peak.numpy(), rp)


def test_text_cache_end_to_end(dev, tmp_path):
    """A FeatureCache run over token batches with the text launcher's default bins (log2 over the context length): the file
    equals the restatement."""
    from msae import Sae, SaeConfig
    from msae.config import parse_cache_config, pos_profile_kwargs
    from msae.features import FeatureCache, PosProfile
    from msae.launch.cache import cache as text_launcher

    d, N, module = 64, 4096, "layers.1"
    torch.manual_seed(12)
    sae = Sae(d, SaeConfig(num_latents=N, k=16), device=dev)
    model = fakes.TinyLlava(vocab=40, d=d).to(dev)
    rng = np.random.default_rng(70)
    dataset = [{"input_ids": torch.from_numpy(rng.integers(0, 40, size=7))} for _ in range(6)]
    cfg = parse_cache_config(["model", "data", "--pos_profile", "--ctx_len", "7"])
    fc = FeatureCache(model, None, {module: sae}, batch_size=2, shard_size=0,
                      pos=pos_profile_kwargs(cfg, text_launcher.POS_PROFILE_DEFAULT_BINS, cfg.ctx_len))
    seen = []
    _spy(fc.cache, seen)
    fc.run(7, dataset)
    fc.save_splits(n_splits=2, save_dir=str(tmp_path), rank=0)
    fc.concate_safetensors(n_splits=2, save_dir=str(tmp_path))
    assert "pos_profile.safetensors" in os.listdir(tmp_path / module)
    assert not [f for f in os.listdir(tmp_path / module) if f.startswith("Rank")]
    st = PosProfile.load(str(tmp_path / module / "pos_profile.safetensors"))
    assert st.table.tolist() == [0, 1, 2, 2, 3, 3, 3] and (st.tail_bin, st.n_bins) == (-1, 4)
    exp = _ref(seen, N, ([0, 1, 2, 2, 3, 3, 3], -1, 4))
    _assert_state(st, exp)
    assert len(seen) == 3 and exp["n_positions"] == 6 * 7 and exp["bin_positions"].tolist() == [6, 6, 12, 18]
    assert exp["count"].sum() > 0


def test_two_rank_files_merge_to_the_single_rank_file(dev, tmp_path):
    """The rows split by hand over two ranks, saved as rank files and merged by the cache's concat step: byte-identical to
    the file of one rank that saw every row."""
    from msae.features.cache import merge_rank_pos_profile

    rng = np.random.default_rng(71)
    B, S, k, N = 8, 64, 32, 2048
    vals, idx = _topk(rng, B, S, k, N)
    bins = ((np.arange(40) // 9).tolist(), 5, 6)
    for name, parts in (("two", [(vals[:4], idx[:4]), (vals[4:], idx[4:])]), ("one", [(vals, idx)])):
        os.makedirs(tmp_path / name / "m")
        for r, part in enumerate(parts):
            _run([part], N, bins, dev).save(str(tmp_path / name / "m" / f"Rank{r}_pos_profile.safetensors"))
        assert merge_rank_pos_profile(str(tmp_path / name / "m"), dev) == str(tmp_path / name / "m" / "pos_profile.safetensors")
        assert os.listdir(tmp_path / name / "m") == ["pos_profile.safetensors"]
    assert ((tmp_path / "two" / "m" / "pos_profile.safetensors").read_bytes()
            == (tmp_path / "one" / "m" / "pos_profile.safetensors").read_bytes())
    assert merge_rank_pos_profile(str(tmp_path / "one" / "m"), dev) is None
