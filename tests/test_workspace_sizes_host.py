"""CPU: the workspace sizing helpers (msae_*_ws_bytes) are host code -- what they promise without a GPU.

  - a helper returns 0 for every shape its entry refuses with MSAE_EINVAL because of the sizes the helper sees (zero or negative
    sizes, k above the entry's limit, N above 262144 for the counters), and the entry does refuse those shapes;
  - sizes do not change from call to call (no hidden state);
  - msae_encode_topk_ws_bytes with the feature-major re-score forced on (MSAE_FM=1) is never smaller than with it forced off,
    at the shapes tests/test_gpu_workspace_contract.py runs;
  - the guarded allocator of that module (tests/guarded_ws.py) itself: sizes, fills, and a changed guard byte is reported with
    its offset.
"""
import ctypes
import os

import pytest
import torch

import guarded_ws

MSAE_EINVAL = -1
MAX_T, MAX_N = 65536, 262144


@pytest.fixture(scope="module")
def lib():
    from msae import _hip

    return _hip.load()


def _opts(**kw):
    from msae import _hip

    o = _hip.MsaeOptions()
    _hip.load().msae_options_init(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---- invalid shapes: the helper says 0, the entry says MSAE_EINVAL ------------------------------------------------------
_FAKE = (ctypes.c_char * 64)()            # a non-null pointer for arguments an entry checks before it checks the shape


def _p():
    return ctypes.cast(_FAKE, ctypes.c_void_p)


def _encode_entry(lib, T, d, N, k):
    return lib.msae_encode_topk_i64(_p(), 0, _p(), None, None, _p(), T, d, N, k, -1, 0.0, -1, _p(), _p(), None, _p(), 1 << 40,
                                    None, None)


@pytest.mark.parametrize("T,d,N,k", [(0, 256, 8192, 32), (-1, 256, 8192, 32), (300, 0, 8192, 32), (300, -4, 8192, 32),
                                     (300, 256, 0, 32), (300, 256, -8192, 32), (300, 256, 8192, 0), (300, 256, 8192, -1),
                                     (300, 256, 8192, 8193), (300, 256, 16384, 4097), (40, 50, 1000, 1001)])
def test_encode_topk_helper_is_zero_where_the_entry_refuses(lib, T, d, N, k):
    assert lib.msae_encode_topk_ws_bytes(T, d, N, k, None) == 0
    if T != 0:                                # (T == 0 is an empty batch: the entry returns 0 without reading its workspace)
        assert _encode_entry(lib, T, d, N, k) == MSAE_EINVAL


def test_encode_topk_helper_at_the_limits_of_k(lib):
    assert lib.msae_encode_topk_ws_bytes(300, 256, 8192, 4096, None) > 0       # k = 4096: the entry's largest
    assert lib.msae_encode_topk_ws_bytes(40, 50, 1000, 1000, None) > 0         # k = N


@pytest.mark.parametrize("max_rows,N", [(0, 8192), (-1, 8192), (128, 0), (128, -1)])
def test_encode_topk_rows_helper(lib, max_rows, N):
    assert lib.msae_encode_topk_rows_ws_bytes(max_rows, N) == 0
    if max_rows != 0:
        rc = lib.msae_encode_topk_rows(_p(), 0, _p(), None, None, _p(), _p(), max_rows, 256, N, 8, -1, 0.0, -1, _p(), _p(), None,
                                       _p(), 1 << 40, None)
        assert rc == MSAE_EINVAL


@pytest.mark.parametrize("T,d,N,k,G,C", [(0, 256, 16384, 32, 2, 64), (200, 0, 16384, 32, 2, 64), (200, 256, 0, 32, 2, 64),
                                         (200, 256, 16384, 0, 2, 64), (200, 256, 16384, 32, 0, 64), (200, 256, 16384, 32, 2, 0),
                                         (200, 256, 16384, 257, 2, 256),       # k above the entry's 256
                                         (200, 256, 16, 32, 2, 64),             # k > N
                                         (200, 256, 16384, 32, 2, 8),           # G C < k: the records cannot hold a top-k
                                         (200, 256, 16384, 32, 2, 8192),        # G C > 8192
                                         (200, 200, 16384, 32, 2, 64)])         # d % 64
def test_rescore_candidates_helper(lib, T, d, N, k, G, C):
    assert lib.msae_rescore_candidates_ws_bytes(T, d, N, k, G, C) == 0
    if T != 0:
        rc = lib.msae_rescore_candidates(_p(), 0, _p(), None, None, T, T, d, N, k, G, C, _p(), -1, 0.0, -1, _p(), _p(), None,
                                         _p(), 1 << 40, None, None)
        assert rc == MSAE_EINVAL
    assert lib.msae_rescore_candidates_ws_bytes(200, 256, 16384, 32, 2, 64) > 200 * 256 * 4


def test_shard_candidates_asks_for_the_encode_size(lib):
    """include/msae.h: "ws: msae_encode_topk_ws_bytes(T, d, N/G, k, opts)" -- less is MSAE_EWS before anything is launched,
    although the shard's own plan (a lower threshold rank, no feature-major regions) is smaller."""
    need = lib.msae_encode_topk_ws_bytes(300, 256, 8192, 32, None)
    for C in (8, 64):
        for ws, n in ((_p(), need - 256), (_p(), 0), (None, need)):
            rc = lib.msae_shard_candidates(_p(), 1, None, None, _p(), 300, 256, 8192, 32, 0, C, -1, -1, _p(), ws, n, None, None)
            assert rc == -3, (C, n, rc)


@pytest.mark.parametrize("A,k,N", [(-1, 3, 37), (64, 0, 37), (64, -3, 37), (64, 3, 0), (64, 3, -1)])
def test_decode_bwd_wdec_helper(lib, A, k, N):
    assert lib.msae_decode_bwd_wdec_ws_bytes(A, k, N) == 0
    rc = lib.msae_decode_bwd_wdec_f32(_p(), _p(), _p(), A, k, N, 4, _p(), None, None, None, _p(), 1 << 40, None)
    assert rc == MSAE_EINVAL


_COUNTER_BAD = [(-1, 8, 1000), (MAX_T + 1, 8, 1000), (150, 0, 1000), (150, -8, 1000), (150, 257, 1000), (150, 8, 0),
                (150, 8, -1), (150, 8, MAX_N + 1)]


@pytest.mark.parametrize("T,k,N", _COUNTER_BAD)
def test_counter_helpers_are_zero_outside_the_envelope(lib, T, k, N):
    """feature statistics, co-activation counters, activation histograms: B*S <= 65536, k <= 256, N <= 262144."""
    assert lib.msae_feature_stats_ws_bytes(T, k, N) == 0
    assert lib.msae_coact_ws_bytes(T, k, N) == 0
    assert lib.msae_act_hist_ws_bytes(T, k, N) == 0
    if T < 0:
        return                                 # (B * S cannot be negative with B, S >= 0: the entries refuse B < 0 itself)
    B, S = (1, T) if T <= MAX_T else (2, T // 2 + 1)
    big = 1 << 40
    assert lib.msae_feature_stats_update(_p(), _p(), B, S, k, 1e-5, N, 1, 576, 64, 0, 8, _p(), _p(), _p(), _p(), _p(), _p(), big,
                                         None) == MSAE_EINVAL
    assert lib.msae_coact_update(_p(), _p(), B, S, k, 1e-5, N, 1, 576, 64, _p(), 4, _p(), _p(), _p(), big, None) == MSAE_EINVAL
    assert lib.msae_act_hist_update(_p(), _p(), B, S, k, 1e-5, N, 1, 576, 64, 3, -16, 32, _p(), _p(), big, None) == MSAE_EINVAL


def test_counter_helpers_at_the_envelope(lib):
    for f in (lib.msae_feature_stats_ws_bytes, lib.msae_coact_ws_bytes, lib.msae_act_hist_ws_bytes):
        assert f(MAX_T, 256, MAX_N) > 2 * MAX_T * 256 * 8          # two key buffers at least
        assert f(150, 8, 1000) > 0


# (T, k, N) -> msae_feature_stats_ws_bytes, msae_coact_ws_bytes, msae_act_hist_ws_bytes: 256-byte aligned regions of two key
# buffers (8 B per entry), two value buffers (4 B per entry; not the co-activation counters), starts / ends (4 B per feature /
# per token; not the histograms) and the sort's (8 B per entry + 1 MiB)
_COUNTER_SIZES = {(1, 1, 1): (1050368, 1049856, 1049856),
                  (300, 5, 37): (1097472, 1087232, 1096960),
                  (8192, 32, 131072): (10485760, 7405568, 9437184),
                  (65536, 256, 262144): (540016640, 404226048, 537919488)}


@pytest.mark.parametrize("shape", sorted(_COUNTER_SIZES))
def test_counter_helper_sizes_are_pinned(lib, shape):
    got = (lib.msae_feature_stats_ws_bytes(*shape), lib.msae_coact_ws_bytes(*shape), lib.msae_act_hist_ws_bytes(*shape))
    assert got == _COUNTER_SIZES[shape]


@pytest.mark.parametrize("M,N,k,chunks", [(-1, 1000, 8, 0), (130, 0, 8, 0), (130, 1000, 0, 0), (130, 1000, 65, 0),
                                          (130, 1000, 8, -1), (130, 4, 8, 0),       # k > N
                                          (130, 8192 * 128, 64, 129)])                # chunks * k > 8192
def test_rows_topk_helper(lib, M, N, k, chunks):
    assert lib.msae_rows_topk_ws_bytes(M, N, k, chunks) == 0
    rc = lib.msae_rows_topk_f32(_p(), 1000, _p(), M, _p(), N, 48, None, None, None, k, chunks, _p(), _p(), _p(), 1 << 40, None)
    assert rc == MSAE_EINVAL


@pytest.mark.parametrize("N,d", [(0, 68), (-1, 68), (1000, 0), (1000, -4), (1000, 67)])
def test_weighted_row_sum_helper(lib, N, d):
    assert lib.msae_weighted_row_sum_ws_bytes(N, d) == 0
    assert lib.msae_weighted_row_sum_f32(_p(), _p(), N, d, 1.0, _p(), _p(), 1 << 40, None) == MSAE_EINVAL


# ---- stable sizes ----------------------------------------------------------------------------------------------------------
# (T, d, N, k, options) of every msae_encode_topk case of tests/test_gpu_workspace_contract.py
ENCODE_SHAPES = [(1, 1024, 8192, 32, {}), (5, 1024, 8192, 32, {}), (16, 1024, 8192, 32, {}), (200, 256, 8192, 32, {}),
                 (300, 256, 8192, 8, {}), (300, 256, 8192, 32, {}), (300, 256, 8192, 256, {}), (300, 192, 8192, 32, {}),
                 (300, 256, 8192, 32, dict(coarse_mode=2)), (300, 256, 8192, 32, dict(certified=1)),
                 (512, 1024, 8192, 32, {}), (40, 50, 1000, 8, {})]


def test_sizes_are_stable_across_calls(lib):
    def all_sizes():
        out = [lib.msae_encode_topk_ws_bytes(T, d, N, k, ctypes.byref(_opts(**o))) for T, d, N, k, o in ENCODE_SHAPES]
        out += [lib.msae_encode_topk_rows_ws_bytes(128, 8192), lib.msae_rescore_candidates_ws_bytes(300, 256, 16384, 32, 2, 64),
                lib.msae_decode_bwd_wdec_ws_bytes(64, 3, 8193), lib.msae_feature_stats_ws_bytes(150, 8, 1000),
                lib.msae_coact_ws_bytes(150, 8, 1000), lib.msae_act_hist_ws_bytes(150, 8, 1000),
                lib.msae_rows_topk_ws_bytes(130, 1000, 8, 2), lib.msae_rows_topk_ws_bytes(130, 1000, 8, 4),
                lib.msae_weighted_row_sum_ws_bytes(1000, 68)]
        return out

    first = all_sizes()
    assert all(n > 0 for n in first), first
    for _ in range(3):
        assert all_sizes() == first
    assert all(n % 256 == 0 for n in first[:len(ENCODE_SHAPES) + 6])       # (the layouts that carve 256-B aligned regions)


def test_feature_major_plan_is_never_smaller(lib):
    """MSAE_FM=1 adds the feature-major regions where the shape has the route and changes nothing elsewhere; MSAE_LPR=1 is how
    tests/test_gpu_rescore_followup.py opens the route at T = 512."""
    old = {n: os.environ.get(n) for n in ("MSAE_FM", "MSAE_LPR")}
    sizes = {}
    try:
        for lpr in (None, "1"):
            for fm in ("0", "1"):
                os.environ["MSAE_FM"] = fm
                if lpr is None:
                    os.environ.pop("MSAE_LPR", None)
                else:
                    os.environ["MSAE_LPR"] = lpr
                sizes[(lpr, fm)] = [lib.msae_encode_topk_ws_bytes(T, d, N, k, ctypes.byref(_opts(**o)))
                                    for T, d, N, k, o in ENCODE_SHAPES]
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
    for lpr in (None, "1"):
        off, on = sizes[(lpr, "0")], sizes[(lpr, "1")]
        assert all(a > 0 and b >= a for a, b in zip(off, on)), (lpr, off, on)
    i512 = [s[:2] for s in ENCODE_SHAPES].index((512, 1024))
    assert sizes[("1", "1")][i512] > sizes[("1", "0")][i512], "the forced route adds no region at T = 512, d = 1024"


# ---- the guarded allocator itself (on host tensors) --------------------------------------------------------------------------
@pytest.mark.parametrize("fill", guarded_ws.FILLS)
def test_guarded_allocator_sizes_fills_and_guards(fill):
    G = guarded_ws.GUARD_BYTES
    gws = guarded_ws.GuardedWorkspace(fill, dev="cpu")
    for n in (0, 1, 5, 256, 1001):
        v = gws("cpu", n)
        assert v.dtype == torch.uint8 and v.numel() == n
        if fill == "zero":
            assert not bool(v.any())
        elif fill == "word3" or n == 0:
            assert v.tolist() == [3 if i % 4 == 0 else 0 for i in range(n)]
        gws.check()
    ptr, n, blk = gws.block(1001)
    assert ptr % 256 == 0 and n == 1001 and blk.view.numel() == 1001 and blk.raw.numel() >= 2 * G + 1001
    gws.check()
    # a byte right behind the workspace, one 299 bytes further on (an aligned word of the rear guard), one in the front guard
    for at, where in ((G + 1001, r"\+0 "), (G + 1001 + 299, r"\+299 "), (G - 8, r"-1009 ")):
        ptr, n, blk = gws.block(1001)
        blk.raw[at] = 9
        with pytest.raises(AssertionError, match=f"workspace of 1001 bytes.*byte offset {where}"):
            gws.check()
    gws.check()                                                    # (a failed check drops its blocks)


def test_guarded_allocator_recycles_leftovers():
    gws = guarded_ws.GuardedWorkspace("recycled", dev="cpu")
    gws("cpu", 64).fill_(7)
    assert gws("cpu", 32).tolist() == [7] * 32                     # smaller: the same block, the guard moved up
    gws.check()
    v = gws("cpu", 128)                                            # larger: the old contents in front, word 3 behind
    assert v[:32].tolist() == [7] * 32 and v[64:72].tolist() == [3, 0, 0, 0, 3, 0, 0, 0]
    gws.check()
    assert [n for _, n in gws.requests] == [64, 32, 128]
