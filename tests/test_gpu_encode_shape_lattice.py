"""GPU: the fused encoder at the widths and batch sizes its kernel families are chosen by -- bit for bit.

csrc/encode_fused.hip picks a route from (T, d, N, k) alone:

    T <= 16      the small path (csrc/encode_small.h) where it has kernels: d_in = 1024, 2048, 4096, and 8192 at T <= 2
    T <= 256     the weight-stream kernel (csrc/gemm_skinny.h: 64- / 128- / 256-token tiles) at d_in % 1024 == 0
    the rest     256-row MFMA tiles (csrc/gemm_mfma.h)

and the suite ran them at power-of-two widths almost only.  Here: every width 1024 ... 8192 at 1 ... 16 tokens (3072, 5120,
6144, 7168, and 8192 from three tokens on, were planned on the small path, which has no kernel for them: the encode raised), the
weight-stream kernel's rotated chunk walk at 3, 5, 6, 10, 12 and 20 chunks, the MFMA tiles at 1, 2, 3, 5, 9, 18 and 24 k-tiles of
128 bytes, the sample widths 256 and 768, and the environment switches that tell the routes apart (MSAE_NO_SMALL_PATH,
MSAE_NO_SKINNY, MSAE_SMALL_DOT4_MAX).

Reference.  <= 16 tokens: oracle.encode_topk (the serial f32 chain in C).  Larger batches: the exact HIP path
ops.topk(ops.pre_acts(...)) for every token (held to the oracle by tests/test_gpu_parity.py) plus the oracle on the first 8.
Edits are applied to the dense latents before the top-k.  Every comparison is of bits; there is no tolerance.

Asserted in every case: the call returns, no token has status 2, every token's values and indices equal the reference.  The
share of tokens the fast path verified (status 0) is a CONDITION that keeps a case from passing with everything on the in-call
exact path, not a measurement: more than 0.9 of the tokens from 32 tokens on (the suite's bar), all but at most one token below
(one token is more than 3 % there) -- tokens built to fall back excepted.
"""
import gc
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from encode_routes import np32, plan_is_small, rand_sae, rand_x, same_bits, small_expected
from oracle import oracle

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
SEED = 0x1A771CE
N0, K0 = 8192, 32
WIDTHS = (1024, 2048, 3072, 4096, 5120, 6144, 7168, 8192)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from msae import _hip

    return _hip.load()


@pytest.fixture(scope="module", autouse=True)
def _pinned_dither_and_caches(dev):
    """The dither seed is fixed for the module (the candidate sets reproduce); weights, operands and references are built once
    per shape and dropped with the module."""
    from msae import ops

    ops.set_dither("on", seed=SEED)
    yield
    ops.set_dither("default")
    _SAES.clear(); _XS.clear(); _REFS.clear()
    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def candidate_pass(request, dev):
    """The candidate pass of the encodes of one test: "int8", "bf16" or "certified", set and restored as the `coarse` fixture
    of tests/test_gpu_parity.py does."""
    from msae import ops

    if request.param == "certified":
        ops.set_certified(True)
    else:
        ops.set_coarse_mode(request.param)
    yield request.param
    ops.set_coarse_mode("int8")
    ops.set_certified(False)


# ---- one encoder per (d, N), one reference per input -----------------------------------------------------------------------
class _Sae:
    def __init__(self, dev, d, N):
        from msae import ops

        self.d, self.N = d, N
        self.W, self.b, self.bd = rand_sae(dev, d, N, seed=1000 + d + N // 8192)
        self.prepared = ops.prepare_encoder(self.W)
        self._np = None

    def np(self):
        if self._np is None:
            self._np = (np32(self.W), np32(self.b), np32(self.bd))
        return self._np


_SAES, _XS, _REFS = {}, {}, {}


def _sae(dev, d, N=N0):
    if (d, N) not in _SAES:
        _SAES[(d, N)] = _Sae(dev, d, N)
    return _SAES[(d, N)]


def _x16(dev, d, dtype=torch.bfloat16):
    """THE 16 tokens of width d (in `dtype`): the cases of <= 16 tokens encode a prefix of them."""
    if (d, dtype) not in _XS:
        _XS[(d, dtype)] = rand_x(dev, 16, d, seed=77 + d, dtype=dtype)
    return _XS[(d, dtype)]


def _ref16(dev, d, N=N0, k=K0, dtype=torch.bfloat16, **kw):
    """oracle.encode_topk of those 16 tokens, once per (shape, k, type, edit) -> (values [16, k], indices int64 [16, k])."""
    key = (d, N, k, dtype, tuple(sorted(kw.items())))
    if key not in _REFS:
        v, i = oracle.encode_topk(np32(_x16(dev, d, dtype)), *_sae(dev, d, N).np(), k, **kw)
        _REFS[key] = (v, i.astype(np.int64))
    return _REFS[key]


def _oracle_rows(s, x, k, **kw):
    v, i = oracle.encode_topk(np32(x), *s.np(), k, **kw)
    return v, i.astype(np.int64)


def _exact(s, pre, k, **kw):
    """The exact HIP path with the edits applied to the dense latents -> numpy (values, indices)."""
    from msae import ops

    lat = pre
    if kw:
        lat = pre.clone()
        if kw.get("set_feature", -1) >= 0:
            lat[:, kw["set_feature"]] = kw["set_value"]
        if kw.get("zero_feature", -1) >= 0:
            lat[:, kw["zero_feature"]] = 0.0
    ev, ei = ops.topk(lat, k)
    return ev.cpu().numpy(), ei.cpu().numpy()


def _check_share(st, what, fall_back=()):
    live = np.ones(st.shape[0], dtype=bool)
    live[list(fall_back)] = False
    fast = st[live] == 0
    if st.shape[0] >= 32:
        assert fast.mean() > 0.9, f"{what}: fast path verified only {fast.mean():.2%} of the tokens"
    else:
        assert (~fast).sum() <= 1, f"{what}: {(~fast).sum()} of {fast.size} tokens went to the exact path"


def _encode(s, x, k, **kw):
    from msae import ops

    v, i, st = ops.encode_topk(x, s.W, s.b, s.bd, s.prepared, k, **kw)
    return v.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()


def _encode_and_check(s, x, k, ref_v, ref_i, what, fall_back=(), **kw):
    """One fused encode: returns, no status 2, every token's bits equal the reference, the share condition -> status."""
    v, i, st = _encode(s, x, k, **kw)
    assert (st != 2).all(), f"{what}: unresolved tokens {np.flatnonzero(st == 2)[:8].tolist()}"
    ok = same_bits(v, ref_v) & same_bits(i, ref_i)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} tokens differ, first {np.flatnonzero(~ok)[:8].tolist()}"
    _check_share(st, what, fall_back)
    return st


def _hot_features(s, x):
    """A hot feature of token 0 and a hot feature of the 1/32 sample (13 + 32 j: its candidates come from the sample pass)."""
    from msae import ops

    pre = ops.pre_acts(x[:1], s.W, s.b, s.bd)
    return int(pre[0].argmax()), 13 + 32 * int(pre[0, 13::32].argmax())


# ---- 1. the small-T lattice --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 2, 3, 4, 5, 16))
@pytest.mark.parametrize("d", WIDTHS)
def test_small_t_lattice(dev, lib, monkeypatch, d, T):
    """Every width 1024 ... 8192 at 1 ... 16 tokens.  The plan is the small path exactly where the route table says (3072,
    5120, 6144, 7168 and 8192 from 3 tokens on: the weight-stream kernel's 64-token tile); the bits are the oracle's."""
    small, _, _ = plan_is_small(lib, monkeypatch, T, d, N0, K0)
    assert small == small_expected(T, d, N0, K0), f"T = {T}, d = {d}: the plan is {'' if small else 'not '}the small path"
    rv, ri = _ref16(dev, d)
    _encode_and_check(_sae(dev, d), _x16(dev, d)[:T], K0, rv[:T], ri[:T], f"T = {T}, d = {d}")


# ---- 2. the small path along its other axes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 16))                       # (the dot4 stream, the MFMA stream)
@pytest.mark.parametrize("k", (1, 64, 65))
@pytest.mark.parametrize("d", (2048, 4096))
def test_small_path_k(dev, lib, monkeypatch, d, k, T):
    """k = 1 and 64 = SMALL_K_MAX stay on the small path, 65 leaves it (the weight-stream kernel).  (d = 2048, k = 64, 16 tokens
    verified 13 of 16 before gemv_mfma_kernel spread its blocks over all workgroups -- 64 workgroups held 128 features each and
    emit 5 per token: a bound among a token's ~100 best values is its tau; 16 of 16 since.)"""
    assert plan_is_small(lib, monkeypatch, T, d, N0, k)[0] == (k <= 64)
    rv, ri = _ref16(dev, d, k=k)
    _encode_and_check(_sae(dev, d), _x16(dev, d)[:T], k, rv[:T], ri[:T], f"T = {T}, d = {d}, k = {k}")


@pytest.mark.parametrize("T", (1, 16))
@pytest.mark.parametrize("dtype", (torch.float32, torch.float16, torch.bfloat16), ids=("f32", "f16", "bf16"))
@pytest.mark.parametrize("d", (2048, 4096))
def test_small_path_activation_types(dev, d, dtype, T):
    rv, ri = _ref16(dev, d, dtype=dtype)
    _encode_and_check(_sae(dev, d), _x16(dev, d, dtype)[:T], K0, rv[:T], ri[:T], f"T = {T}, d = {d}, {dtype}")


@pytest.mark.parametrize("T", (1, 16))
@pytest.mark.parametrize("d", (2048, 4096))
def test_small_path_sample_width_768(dev, lib, monkeypatch, d, T):
    """N = 24576: 12 rows per workgroup of the dot4 stream, 1536 blocks of 16 features for the MFMA stream, sample width 768."""
    N = 24576
    assert plan_is_small(lib, monkeypatch, T, d, N, K0)[0]
    rv, ri = _ref16(dev, d, N=N)
    _encode_and_check(_sae(dev, d, N), _x16(dev, d)[:T], K0, rv[:T], ri[:T], f"T = {T}, d = {d}, N = {N}")


@pytest.mark.parametrize("T", (2, 16))
@pytest.mark.parametrize("d", (2048, 4096))
def test_small_path_hook_edits(dev, d, T):
    """set_feature / zero_feature on the small path: a hot feature, a hot feature of the 1/32 sample, both together."""
    s, x16 = _sae(dev, d), _x16(dev, d)
    hot, hot_s = _hot_features(s, x16)
    assert hot != hot_s
    for kw in (dict(zero_feature=hot), dict(zero_feature=hot_s), dict(set_feature=hot_s, set_value=7.5),
               dict(set_feature=hot_s, set_value=0.5, zero_feature=hot), dict(set_feature=hot, set_value=0.25, zero_feature=hot_s)):
        rv, ri = _ref16(dev, d, **kw)
        _encode_and_check(s, x16[:T], K0, rv[:T], ri[:T], f"T = {T}, d = {d}, {kw}", **kw)


@pytest.mark.parametrize("kind", ("inf", "constant"))
@pytest.mark.parametrize("d", (2048, 4096))
def test_small_path_degenerate_token(dev, d, kind):
    """One token of eight cannot verify: a row holding +inf (its scale is inf), or a constant row of 3e38 (the sum of its squares
    overflows f32: the band, every upper value and the bound tau are +inf, and no k-th value lies above that).  It comes back
    from the in-call exact path (status 1) with the exact path's bits, NaN for NaN; the other seven are the oracle's."""
    from msae import ops

    s, t_bad = _sae(dev, d), 5
    x = _x16(dev, d)[:8].clone()
    if kind == "inf":
        x[t_bad, 7] = float("inf")
    else:
        x[t_bad] = 3e38
    v, i, st = _encode(s, x, K0)
    assert (st != 2).all()
    assert st[t_bad] == 1, st.tolist()
    ev, ei = _exact(s, ops.pre_acts(x[t_bad:t_bad + 1], s.W, s.b, s.bd), K0)
    assert (v[t_bad].view(np.uint32) == ev[0].view(np.uint32)).all() and (i[t_bad] == ei[0]).all()
    rest = [t for t in range(8) if t != t_bad]
    rv, ri = _ref16(dev, d)
    ok = same_bits(v[rest], rv[rest]) & same_bits(i[rest], ri[rest])
    assert ok.all(), f"d = {d}, {kind}: tokens {np.asarray(rest)[~ok].tolist()} differ from the oracle"
    _check_share(st, f"d = {d}, {kind}", fall_back=(t_bad,))


# ---- 3. the small path switched off ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 16))
@pytest.mark.parametrize("d", (1024, 3072, 4096))
def test_weight_stream_tile_nearly_empty(dev, monkeypatch, d, T):
    """MSAE_NO_SMALL_PATH=1: 1 and 16 tokens in the weight-stream kernel's 64-token tile -- the route d_in = 3072 takes anyway."""
    monkeypatch.setenv("MSAE_NO_SMALL_PATH", "1")
    rv, ri = _ref16(dev, d)
    _encode_and_check(_sae(dev, d), _x16(dev, d)[:T], K0, rv[:T], ri[:T], f"no small path, T = {T}, d = {d}")


# ---- 4. the weight-stream kernel at chunk counts that are no power of two ------------------------------------------------------
def _large_case(dev, s, x, k, what, edits, reruns=()):
    """x through the fused encoder, plain and with every edit of `edits`, against the exact path (all tokens) and the oracle
    (first 8); `reruns`: (environment switch, monkeypatch) pairs under which everything runs again -- same bits."""
    from msae import ops

    pre = ops.pre_acts(x, s.W, s.b, s.bd)
    for kw in ({},) + tuple(edits):
        ev, ei = _exact(s, pre, k, **kw)
        ov, oi = _oracle_rows(s, x[:8], k, **kw)
        ok = same_bits(ev[:8], ov) & same_bits(ei[:8], oi)
        assert ok.all(), f"{what} {kw}: the exact path differs from the oracle on tokens {np.flatnonzero(~ok).tolist()}"
        _encode_and_check(s, x, k, ev, ei, f"{what} {kw}", **kw)
        for name, mp in reruns:
            mp.setenv(name, "1")
            try:
                _encode_and_check(s, x, k, ev, ei, f"{what} {kw} {name}=1", **kw)
            finally:
                mp.delenv(name)
    return pre


@pytest.mark.parametrize("d,N,T", [(d, N0, T) for d in (3072, 5120) for T in (17, 64, 65, 128, 129, 256)]
                         + [(3072, 24576, 40), (3072, 24576, 200)])
def test_weight_stream_kernel_odd_chunk_counts(dev, monkeypatch, d, N, T):
    """17 ... 256 tokens at d_in = 3072 and 5120: nchunks = d / KC = 3, 6, 12 and 5, 10, 20 in the rotated walk (b mod nchunks)
    of the 64- / 128- / 256-token tiles, plain and with an edit of a hot sample feature.  d_in = 3072 at 64 and 200 tokens
    again under MSAE_NO_SKINNY=1: the row-major MFMA pass at the same shape (24 k-tiles), same bits."""
    s = _sae(dev, d, N)
    x = rand_x(dev, T, d, seed=200 + T)
    _, hot_s = _hot_features(s, x[T // 3:])
    reruns = ((("MSAE_NO_SKINNY", monkeypatch),) if d == 3072 and T in (64, 200) else ())
    _large_case(dev, s, x, K0, f"T = {T}, d = {d}, N = {N}", (dict(set_feature=5, set_value=0.25, zero_feature=hot_s),), reruns)


# ---- 5. MFMA tiles with few and odd k-tile counts ------------------------------------------------------------------------------
@pytest.mark.parametrize("candidate_pass,d,T",
                         [("int8", d, T) for d in (128, 256, 384, 640, 1152, 2304, 3072) for T in (257, 300)]
                         + [(m, d, T) for m in ("certified", "bf16") for d in (128, 384, 2304) for T in (257, 300)],
                         indirect=["candidate_pass"])
def test_mfma_tiles_few_and_odd_k_tiles(dev, candidate_pass, d, T):
    """257 and 300 tokens (two 256-row tiles, the second nearly empty): 1, 2, 3, 5, 9, 18 and 24 k-tiles of the int8 pass (+ its
    outlier tile), 3 x that of the certified pass, 2, 6 and 36 of the bf16 pass."""
    _large_case(dev, _sae(dev, d), rand_x(dev, T, d, seed=300 + T), K0, f"{candidate_pass}, T = {T}, d = {d}", ())


def test_feature_major_first_round_d2304(dev):
    """d_in = 2304, 1536 tokens, bf16 x.  The cost model (fm_pays: 8.2 tokens per feature, 769 ps gained per pair against its
    bar of 500) sends the first round of the re-score down the FEATURE-major route at this shape, and that is the route that
    ran: the witness (bit 30 of msae_options::rows_rescored) was set on 1536 of 1536 tokens.  The case prints the witness and
    asserts the bits whichever route runs."""
    from msae import ops

    d, T = 2304, 1536
    s = _sae(dev, d)
    x = rand_x(dev, T, d, seed=1536)
    rows = torch.zeros(T, dtype=torch.int32, device=dev)
    with ops.rescore_rows(rows):
        _large_case(dev, s, x, K0, f"T = {T}, d = {d}", ())
    took = ((rows >> 30) & 1).bool()
    print(f"feature-major first round: bit 30 set on {int(took.sum())} of {T} tokens")


# ---- 6. the dot4 stream's kernels for 2 and 4 tokens -----------------------------------------------------------------------------
def test_shipped_dot4_kernels_for_2_and_4_tokens(dev):
    """gemv_small_kernel<., 2> and <., 4> run only where MSAE_SMALL_DOT4_MAX says so, and the knob is read once per process: ONE
    fresh child (tests/small_dot4_runner.py) encodes 2, 3 and 4 tokens at d_in = 1024 and 4096 against the oracle."""
    env = dict(os.environ, MSAE_SMALL_DOT4_MAX="4")
    env.pop("MSAE_NO_SMALL_PATH", None)
    cmd = ["timeout", "-k", "10", "240", sys.executable, str(REPO / "tests" / "small_dot4_runner.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.count("ok:") == 6, r.stdout[-3000:]
