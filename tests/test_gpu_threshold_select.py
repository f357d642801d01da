"""The threshold select of the fused encoder (csrc/topk.hip) through its debug entry msae_kth_value_f32: the streaming kernel
(S % 1024 == 0, S >= 2048, r S / 1024 <= 256) and the register-resident one (every other shape, and MSAE_KTH_STREAM=0).

Reference, in numpy: with the order key of a float (sign-folded bits, -0 onto +0), tau[t] is the float whose key is the r-th
largest key of the row with the low 14 bits cleared, and the pushed set is every (key << 32 | 0x7FFFFFFF - (stride j + off))
with key above that -- nothing when tau <= 0.  tau is compared bit for bit, the lists as sorted sets, cnt exactly (it advances
from whatever it held, and counts the entries a small `cap` dropped as well).  Both kernels run on every input and must agree.

The streaming kernel finishes a row whose survivors (keys >= the rounded r-th largest key of the row's first 1024 values) do
not fit its 512-entry buffer by another route inside the same launch.  Which rows do is read off the reference (count of
keys >= chunk 0's r-th largest): test_both_routes_of_the_streaming_kernel_are_covered asserts that at least a third of the
streamed rows of this file overflow and at least a third do not.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOW = np.uint32((1 << 14) - 1)
BUF = 512                      # survivor buffer of the streaming kernel (KS_CAP)
SHAPES = [2048, 4096, 8192, 256, 1024]
RS = [1, 16, 64]
TS = [1, 5, 37]
KINDS = ["gauss", "equal", "tied40", "chunk0_low", "descending", "ascending", "zeros_inf", "sparse", "negative"]


def streams(S, r):
    """the launcher's rule (msae_kth_value_launch)"""
    return S % 1024 == 0 and S >= 2048 and r * (S // 1024) <= BUF // 2


def order_key(v):
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & 0x80000000, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def make_row(kind, S, r, rng):
    g = rng.standard_normal(S).astype(np.float32)
    if kind == "gauss":
        return g
    if kind == "equal":
        return np.full(S, 1.5, np.float32)
    if kind == "tied40":                       # r - 1 values above 3.0, then 40 copies of it, the rest below
        row = np.minimum(g, 2.5).astype(np.float32)
        pos = rng.permutation(S)[: r - 1 + 40]
        row[pos[: r - 1]] = 5.0 + rng.random(r - 1).astype(np.float32)
        row[pos[r - 1:]] = 3.0
        return row
    if kind == "chunk0_low":                   # the first 1024 values say nothing about the row
        row = (g + 3.0).astype(np.float32)
        row[: min(S, 1024)] = -1.0
        return row
    if kind == "descending":
        return np.linspace(2.0, -1.0, S, dtype=np.float32)
    if kind == "ascending":
        return np.linspace(-1.0, 2.0, S, dtype=np.float32)
    if kind == "zeros_inf":
        row = g.copy()
        pos = rng.permutation(S)[:24]
        row[pos[:8]] = 0.0
        row[pos[8:16]] = -0.0
        row[pos[16:19]] = np.inf
        row[pos[19:24]] = -np.inf
        return row
    if kind == "sparse":                       # +-0 with five positive values behind the first 1024 (or anywhere, S <= 1024)
        row = np.where(rng.random(S) < 0.5, 0.0, -0.0).astype(np.float32)
        lo = 1024 if S > 1024 else 0
        row[lo + rng.permutation(S - lo)[:5]] = 1.0 + rng.random(5).astype(np.float32)
        return row
    if kind == "negative":
        return (-np.abs(g) - 0.1).astype(np.float32)
    raise KeyError(kind)


_ROWS = {}


def rows_of(S, r, T):
    """[T][S] f32: row t of kind KINDS[t % 9]; built once per shape and left unchanged"""
    if (S, r, T) not in _ROWS:
        rng = np.random.default_rng(1000 * S + 10 * r + T)
        _ROWS[S, r, T] = np.stack([make_row(KINDS[t % len(KINDS)], S, r, rng) for t in range(T)])
    return _ROWS[S, r, T]


def reference(rows, r, stride, off):
    """-> tau bits [T] (u32), list of sorted u64 arrays, and per row the survivor counts (exact bound, rounded bound)"""
    taus, sets, surv = [], [], []
    for row in rows:
        key = order_key(row)
        kth = np.sort(key)[::-1][r - 1] & ~LOW
        tau = key_to_float(kth)
        taus.append(tau.view(np.uint32))
        j = np.nonzero(key > kth)[0] if tau > 0 else np.zeros(0, np.int64)
        ent = (key[j].astype(np.uint64) << np.uint64(32)) | (0x7FFFFFFF - (stride * j + off)).astype(np.uint64)
        sets.append(np.sort(ent))
        c0 = np.sort(key[:1024])[::-1][min(r, len(key[:1024])) - 1]
        surv.append((int((key >= c0).sum()), int((key >= (c0 & ~LOW)).sum())))
    return np.array(taus, np.uint32), sets, surv


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    return _hip.load()


def launch(lib, rows_dev, T, S, ld, r, cap, stride, off, cnt0, stream_kernel):
    """-> tau bits [T], cnt [T], cand [T][cap] (u64) of one launch; cnt starts at cnt0[t]"""
    from msae import _hip

    out = torch.full((T,), float("nan"), device=rows_dev.device)
    cnt = torch.from_numpy(cnt0.astype(np.int32)).to(rows_dev.device)
    cand = torch.zeros(T, max(cap, 1), dtype=torch.int64, device=rows_dev.device)
    old = os.environ.get("MSAE_KTH_STREAM")
    if stream_kernel:
        os.environ.pop("MSAE_KTH_STREAM", None)
    else:
        os.environ["MSAE_KTH_STREAM"] = "0"
    try:
        _hip.check(lib.msae_kth_value_f32(_hip.ptr(rows_dev), T, S, ld, r, _hip.ptr(out), _hip.ptr(cnt), _hip.ptr(cand), cap,
                                          stride, off, _hip.stream_of(rows_dev)), "msae_kth_value_f32")
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop("MSAE_KTH_STREAM", None)
        else:
            os.environ["MSAE_KTH_STREAM"] = old
    return (out.cpu().numpy().view(np.uint32), cnt.cpu().numpy(), cand.cpu().numpy().view(np.uint64))


def check(what, got, taus, sets, cnt0, cap):
    tau, cnt, cand = got
    assert np.array_equal(tau, taus), f"{what}: tau differs on rows {np.nonzero(tau != taus)[0].tolist()}"
    for t, want in enumerate(sets):
        assert cnt[t] == cnt0[t] + len(want), f"{what}: row {t} ({KINDS[t % len(KINDS)]}) cnt {cnt[t]} != {cnt0[t]} + {len(want)}"
        have = cand[t, cnt0[t]:min(int(cnt[t]), cap)]
        if cnt[t] <= cap:
            assert np.array_equal(np.sort(have), want), f"{what}: row {t} ({KINDS[t % len(KINDS)]}) pushed set differs"
        else:                                  # the list is cut at cap: distinct members of the reference set
            assert len(np.unique(have)) == len(have) and np.isin(have, want).all(), f"{what}: row {t} entries outside the set"
        assert not cand[t, :cnt0[t]].any() and not cand[t, min(int(cnt[t]), cap):].any(), f"{what}: row {t} wrote outside its slots"


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("S", SHAPES)
def test_threshold_and_pushed_set_equal_reference(lib, S, r):
    dev = torch.device("cuda:0")
    for T in TS:
        rows = rows_of(S, r, T)
        ld = S + 8 if (S, r) == (2048, 16) else S              # a pitch above S once: the padding holds large values
        stride, off = (1, 0) if r == 1 else (32, 13)
        padded = np.full((T, ld), 100.0, np.float32)
        padded[:, :S] = rows
        rows_dev = torch.from_numpy(padded).to(dev)
        taus, sets, _ = reference(rows, r, stride, off)
        cnt0 = np.array([3 if t % 2 else 0 for t in range(T)], np.int64)
        full = S + 4
        new = launch(lib, rows_dev, T, S, ld, r, full, stride, off, cnt0, True)
        old = launch(lib, rows_dev, T, S, ld, r, full, stride, off, cnt0, False)
        check(f"S={S} r={r} T={T} default kernel", new, taus, sets, cnt0, full)
        check(f"S={S} r={r} T={T} MSAE_KTH_STREAM=0", old, taus, sets, cnt0, full)
        assert np.array_equal(new[0], old[0]) and np.array_equal(new[1], old[1])
        assert all(np.array_equal(np.sort(a), np.sort(b)) for a, b in zip(new[2], old[2])), "the two kernels' lists differ"
        # the negative rows: nothing pushed, cnt untouched
        for t in range(T):
            if KINDS[t % len(KINDS)] == "negative":
                assert len(sets[t]) == 0 and new[1][t] == cnt0[t] and old[1][t] == cnt0[t]
        # a cap below the pushed count: cnt still counts everything
        small = 8
        assert r == 1 or any(len(s) + c > small for s, c in zip(sets, cnt0))   # (r = 1 pushes next to nothing)
        for which in (True, False):
            check(f"S={S} r={r} T={T} cap={small} stream={which}", launch(lib, rows_dev, T, S, ld, r, small, stride, off, cnt0, which),
                  taus, sets, cnt0, small)


def test_without_a_list_only_the_threshold_is_written(lib):
    from msae import _hip

    S, r, T = 4096, 16, 37
    rows = rows_of(S, r, T)
    rows_dev = torch.from_numpy(rows).to("cuda:0")
    taus, _, _ = reference(rows, r, 1, 0)
    out = torch.full((T,), float("nan"), device=rows_dev.device)
    _hip.check(lib.msae_kth_value_f32(_hip.ptr(rows_dev), T, S, S, r, _hip.ptr(out), None, None, 0, 1, 0, _hip.stream_of(rows_dev)),
               "msae_kth_value_f32")
    assert np.array_equal(out.cpu().numpy().view(np.uint32), taus)


def test_both_routes_of_the_streaming_kernel_are_covered():
    """From the reference alone: a streamed row overflows for certain when even the keys >= chunk 0's exact r-th largest exceed
    the buffer, and stays inside for certain when the keys >= that bound with its low 14 bits cleared fit."""
    n = over = inside = 0
    for S in SHAPES:
        for r in RS:
            if not streams(S, r):
                continue
            for T in TS:
                _, _, surv = reference(rows_of(S, r, T), r, 1, 0)
                n += len(surv)
                over += sum(exact > BUF for exact, _ in surv)
                inside += sum(rounded <= BUF for _, rounded in surv)
    print(f"\nstreamed rows {n}: overflow {over}, inside the buffer {inside}")
    assert n > 0 and 3 * over >= n and 3 * inside >= n, (n, over, inside)
