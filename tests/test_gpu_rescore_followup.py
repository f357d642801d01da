"""The re-score behind a FEATURE-major first round (select_rescore_kernel PHASE 1 -> counting sort -> fm_dot_kernel -> PHASE 2)
on tokens that need FOLLOW-UP rounds, and the start-of-call zeroing of that route's scratch.

Every result is compared with the exact path (ops.encode_topk(exact=True) on the same inputs) bit for bit: top_acts,
top_indices, and status & 3 resolved on both sides.

The weights are tests/test_gpu_hostile.py's cluster of near-duplicate features: `cluster` rows are copies of one direction
scaled by 1 + 1e-4 j and every token points along it, so the cluster's exact values are closer together than the error band
and a token needs all of them re-scored.  With ~300 of them a tenth of the tokens takes a first round smaller than the
cluster and a follow-up round for the rest (1 .. 40 rows, depending on the token's noise), and the tokens that need more than
r_max = 8 k = 256 rows go to the exact path.  (Clusters of ~120 rows are covered by the first round: no follow-up at all.)
The dither seed is fixed, so every run sees the same candidate lists.  Every test asserts through
msae_options::rows_rescored that the feature-major route ran and that rounds >= 2 occurred.

The pair counters (fm.count) and defer flags (fm.defer) of the route are zeroed by the call's one start-of-call kernel
(zero_call_scratch), not by launches of their own in front of PHASE 1.  Each test therefore encodes twice through the same
workspace: a counter or flag left over from the first call would break the second (fm.count feeds the counting sort's ranks
and slot offsets, fm.defer decides which launch owns a token), and status and statistics of both calls must be equal.
"""
import os

import pytest
import torch

import hostile

pytestmark = pytest.mark.gpu

K = 32
SEED = 12345          # msae_options::dither_seed of the prepare and of every call: the same roundings in every run


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture
def forced_fm():
    """MSAE_FM=1: the feature-major route wherever the shape has it.  MSAE_LPR=1 keeps a lane per row in the first round at
    T = 512 too (rescore_shape would take two: no feature-major route then).  The workspace size depends on both and ops
    memoises it by shape, so the memo is dropped on the way in and out."""
    from msae import ops

    old = {n: os.environ.get(n) for n in ("MSAE_FM", "MSAE_LPR")}
    os.environ["MSAE_FM"] = "1"
    os.environ["MSAE_LPR"] = "1"
    ops._WS_BYTES_CACHE.clear()
    yield
    for n, v in old.items():
        if v is None:
            os.environ.pop(n, None)
        else:
            os.environ[n] = v
    ops._WS_BYTES_CACHE.clear()


_CASES = {}


def _case(dev, d, N, T, cluster, seed=11):
    """(x, W, b, b_dec, prepared) of the cluster construction, built once per shape and left unchanged."""
    from msae import ops

    key = (d, N, T, cluster, seed)
    if key not in _CASES:
        if len(_CASES) >= 2:                       # (d = 12288 holds 0.8 GB of weights)
            _CASES.clear()
            torch.cuda.empty_cache()
        W, b, bd = hostile.weights("gauss", N, d, dev, seed=seed)
        g = torch.Generator(device=dev).manual_seed(77 + cluster)
        base = torch.randn(d, generator=g, device=dev)
        base /= base.norm()
        if cluster:
            rows = torch.randperm(N, generator=g, device=dev)[:cluster]
            scale = 1.0 + 1e-4 * torch.arange(cluster, device=dev, dtype=torch.float32)
            W[rows] = base[None, :] * scale[:, None]
            b[rows] = 0.0
        x = torch.randn(T, d, generator=g, device=dev) + 6.0 * base[None, :]
        x = (x + bd).to(torch.bfloat16)
        W = W.contiguous()
        ops.set_dither("on", seed=SEED)            # (batches of this size are rounded against the PREPARE's dither vectors)
        try:
            _CASES[key] = (x, W, b, bd, ops.prepare_encoder(W))
        finally:
            ops.set_dither("default")
    return _CASES[key]


def _fields(rows):
    """msae_options::rows_rescored -> (feature-major, rounds, first-round rows, rows read)"""
    return (rows >> 30) & 1, (rows >> 24) & 0x3F, (rows >> 12) & 0xFFF, rows & 0xFFF


def _run(ops, case, T, **kw):
    """fused (twice, through the same workspace) against the exact path; -> (status, rows_rescored)"""
    x, W, b, bd, prepared = case
    ev, ei, est = ops.encode_topk(x, W, b, bd, prepared, K, exact=True, **kw)
    rows = torch.zeros(T, dtype=torch.int32, device=x.device)
    for call in range(2):
        rows.zero_()
        with ops.rescore_rows(rows):
            v, i, st = ops.encode_topk(x, W, b, bd, prepared, K, status_detail=True, dither=1, dither_seed=SEED, **kw)
        assert int(((st & 0xFF) >= 2).sum()) == 0, f"call {call}: unresolved tokens"
        assert torch.equal(i, ei), f"call {call}: indices differ on {int((i != ei).any(-1).sum())} tokens"
        assert torch.equal(v.view(torch.int32), ev.view(torch.int32)), f"call {call}: values differ"
        # exact=True reports every token as 1 (recomputed); the fused call 0 (verified) or 1: both resolved, none 2 / 3
        assert bool((((st & 3) == 0) | ((st & 3) == 1)).all()) and bool(((est & 3) == 1).all())
        if call == 0:
            first = (st.clone(), rows.clone())
        else:                                      # nothing of the first call leaked into the second
            assert torch.equal(st, first[0]) and torch.equal(rows, first[1])
    return st, rows


def _summary(what, st, rows):
    fm, rounds, first, done = _fields(rows)
    ver = (st & 0xFF) == 0
    extra = (done - first)[ver & (rounds >= 2)]
    hist = torch.bincount(extra.clamp(max=63), minlength=1).tolist() if extra.numel() else []
    print(f"\n{what}: verified {int(ver.sum())} of {st.numel()}, feature-major {int(fm[ver].sum())}, rounds>=2 "
          f"{int((rounds[ver] >= 2).sum())}, rounds>=3 {int((rounds[ver] >= 3).sum())}, r_max fallbacks "
          f"{int((((st >> 8) & 32) != 0).sum())}, rows past the first round (histogram from 0): {hist}")
    return fm, rounds, first, done, ver


@pytest.mark.parametrize("d,T", [(1024, 1024), (12288, 512), (1152, 1024)])
def test_cluster_300_follow_up_rounds_equal_exact(dev, forced_fm, d, T):
    """300 near-duplicates, r_max = 256: tokens whose coarse statistic asks for fewer rows take a follow-up round, tokens that
    need more than r_max rows go to the exact path.  d = 1024: the follow-up rounds read the activations from LDS (LDSA);
    d = 12288: no room for them, the other instantiation of the full-size launch; d = 1152: a row length that is no multiple
    of the 256-float batch of four lanes per row -- the kernel falls back to two lanes per row."""
    from msae import ops

    N = 16384
    st, rows = _run(ops, _case(dev, d, N, T, 300), T)
    fm, rounds, first, done, ver = _summary(f"cluster300 d={d} T={T}", st, rows)
    assert bool(fm[ver].bool().all()), "the feature-major route was not taken"
    assert int(ver.sum()) >= 0.8 * T
    assert int((rounds[ver] >= 2).sum()) >= 16, "(almost) no follow-up round ran"
    assert bool((done[ver & (rounds >= 2)] > first[ver & (rounds >= 2)]).all())
    assert int((((st >> 8) & 32) != 0).sum()) > 0, "no token hit r_max"


def test_follow_up_targets_off_the_group_sizes(dev, forced_fm):
    """Follow-up rounds of 1, 3, 5 and 17 rows -- no multiples of the lanes that share a row; up to 16 rows take four lanes per
    row, more a lane per row -- occur on some token of clusters of 270 .. 300 rows."""
    from msae import ops

    d, N, T = 1024, 16384, 1024
    seen = set()
    for cluster in (300, 290, 280, 270):
        st, rows = _run(ops, _case(dev, d, N, T, cluster), T)
        fm, rounds, first, done, ver = _summary(f"cluster{cluster}", st, rows)
        two = ver & (rounds >= 2)
        assert bool(fm[ver].bool().all())
        seen.update((done - first)[two].unique().tolist())
    assert {1, 3, 5, 17} <= seen, sorted(seen)


def test_hook_edits_with_follow_up_rounds(dev, forced_fm):
    """set_feature puts one result in front of the re-scored ones (the has_set offset of the result slots), zero_feature
    takes a feature out of the candidate passes: the follow-up rounds must still land every row in its slot."""
    from msae import ops

    d, N, T = 1024, 16384, 1024
    case = _case(dev, d, N, T, 300)
    x, W, b, bd, prepared = case
    hot = int(ops.pre_acts(x[:1], W, b, bd)[0].argmax())     # a member of the cluster
    for kw in (dict(set_feature=77, set_value=10.0), dict(zero_feature=hot), dict(set_feature=77, set_value=10.0, zero_feature=hot)):
        st, rows = _run(ops, case, T, **kw)
        fm, rounds, first, done, ver = _summary(f"edits {kw}", st, rows)
        assert bool(fm[ver].bool().all())
        assert int((rounds[ver] >= 2).sum()) >= 16, "(almost) no follow-up round ran"
