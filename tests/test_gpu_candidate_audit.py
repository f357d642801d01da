"""Every record of the candidate pass audited against the f64 pre-activations of EVERY (token, feature) pair of the shard.

The fused encoders return the exact f32 top-k only if the candidate pass keeps two promises for every pair, not only for the
pairs the verification re-scores:
  * band: the exact pre-activation p lies in [c - z sigma, c + z sigma] (c: the coarse int8 / bf16 value);
  * threshold: a feature left out of a token's candidates has p <= tau (the record's tail).
msae_shard_candidates is the only entry point that exposes the candidate lists; with C >= 8 r they are the single-GPU
encode's own lists cut to the C best (smaller C also covers a shard's reduced r).  Per token:
  P1 format      valid keys first, empty slots (key 0, z sigma 0) last; unique ids inside the shard; z sigma finite and > 0;
                 a full record's upper values >= tail; a +inf tail only with an empty record.
  P2 band        |p - c| <= z sigma (1 + 1e-6) + 4 ulp(|c|) for every recorded pair (c = u - z sigma).
  P3 threshold   p <= tail for every feature of the shard left out of the record.
  P4 complete    (int8, subtractive dither) every feature whose restated c + sqrt(proxy) exceeds the tail is recorded --
                 the band is at least the proxy (tests/test_gpu_band.py).
  P5 definition  (int8, subtractive dither) the recorded c is quant_x_kernel<SD>'s coarse value with the outlier remainder
                 computed EXACTLY (tests/candidate_ref.py), to the f32 evaluation's own error: 2 ulp(u) + 4 x 2^-24 x the sum
                 of the magnitudes of its terms (one operand integer off by one step is ~10x that).
  P6 unbounded   empty record and tail +inf for tokens the pass cannot bound: all-zero rows under negative biases in the bf16
                 pass (zero band, tau <= 0), outlier multipliers above 1040, and every token of a dithered call on a buffer
                 prepared without the dither.
"""
from __future__ import annotations

import contextlib
import gc

import numpy as np
import pytest
import torch

import hostile
from candidate_ref import band_proxy, coarse_all, decode_records, exact_pre, restate_int8_sd

pytestmark = pytest.mark.gpu

Z = 7.0                               # the library's default band width (msae_options::guard_z)
SEED = 0xC0A2D17E
N8 = 8192


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_after():
    yield
    from msae import ops

    ops.set_coarse_mode("default")
    ops.set_dither("default")
    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _mode(mode: str):
    """"sd": int8 with the subtractive dither (the default pass), "rtn": int8 rounded to nearest, "bf16": the bf16 pass,
    "i8-bf16": the int8 mode at a width the int8 pass does not take (d % 128 != 0: the bf16 pass runs)."""
    from msae import ops

    ops.set_coarse_mode("bf16" if mode == "bf16" else "int8")   # ("i8-bf16": int8 with the dither, like "sd")
    ops.set_dither("off" if mode == "rtn" else "on", seed=SEED)
    try:
        yield
    finally:
        ops.set_coarse_mode("default")
        ops.set_dither("default")


def _ulp(v: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def audit(dev, x, W, b, bd, k, C, *, mode, row_offset=0, set_feature=-1, zero_feature=-1, prepared=None, unbounded=(),
          label=""):
    """shard_candidates on (x, shard W) -> P1 ... P6 (P4 / P5 for mode "sd"); returns the decoded record and statistics."""
    from msae import ops

    T, N = x.shape[0], W.shape[0]
    with _mode(mode):
        if prepared is None:
            prepared = ops.prepare_encoder(W)
        recs = ops.shard_candidates(x, b, bd, prepared, N, k, row_offset, C, set_feature=set_feature,
                                    zero_feature=zero_feature)
    R = decode_records(recs, C)
    valid, u, zs, tail = R["valid"], R["u"], R["zs"], R["tail"]
    lf = R["feat"] - row_offset
    skip = [f - row_offset for f in (set_feature, zero_feature) if row_offset <= f < row_offset + N]

    # P1: the record's format
    nv = valid.sum(axis=1)
    assert (valid == (np.arange(C)[None, :] < nv[:, None])).all(), "P1: valid keys first, empty slots last"
    assert (R["keys"][~valid] == 0).all() and (zs[~valid] == 0).all(), "P1: empty slots are zero"
    assert ((lf[valid] >= 0) & (lf[valid] < N)).all(), "P1: ids inside [row_offset, row_offset + N_shard)"
    srt = np.sort(np.where(valid, lf, -1 - np.arange(C)[None, :]), axis=1)
    assert (np.diff(srt, axis=1) != 0).all(), "P1: duplicate ids in a record"
    assert np.isfinite(zs[valid]).all() and (zs[valid] > 0).all(), "P1: z sigma finite and > 0"
    assert not np.isnan(tail).any()
    full = nv == C
    assert (u[full] >= tail[full, None]).all(), "P1: a full record holds the C best: every u >= tail"
    unb = np.isinf(tail)
    assert (tail[unb] > 0).all() and (nv[unb] == 0).all(), "P1: +inf tail only with an empty record"
    for f in skip:
        assert not (valid & (lf == f)).any(), f"hook edit: feature {f + row_offset} in its owner's record"
    # P6: the tokens the pass cannot bound
    unbounded = np.asarray(unbounded, dtype=np.int64)
    if unbounded.size:
        assert unb[unbounded].all() and (nv[unbounded] == 0).all(), \
            f"P6: bounded tokens {unbounded[~unb[unbounded]].tolist()[:8]} that the pass cannot bound"

    # P2 / P3 against the f64 pre-activations of every pair
    p = exact_pre(x, W, b, bd)
    tt, jj = np.nonzero(valid)
    ff = lf[tt, jj]
    tt_d, ff_d = torch.from_numpy(tt).to(dev), torch.from_numpy(ff).to(dev)
    pv = p[tt_d, ff_d].cpu().numpy()
    c = u[tt, jj].astype(np.float64) - zs[tt, jj]
    z64 = zs[tt, jj].astype(np.float64)
    dev2 = np.abs(pv - c) - (z64 * (1 + 1e-6) + 4 * _ulp(c))
    if dev2.size and dev2.max() > 0:
        i = int(dev2.argmax())
        raise AssertionError(f"P2 {label}: token {tt[i]} feature {ff[i] + row_offset}: p {pv[i]:.9g} c {c[i]:.9g} "
                             f"z sigma {z64[i]:.6g} ({int((dev2 > 0).sum())} pairs outside their band)")
    ratio = float((np.abs(pv - c) / z64).max()) if c.size else 0.0
    inrec = torch.zeros(T, N, dtype=torch.bool, device=dev)
    inrec[tt_d, ff_d] = True
    for f in skip:
        inrec[:, f] = True
    tail_d = torch.from_numpy(tail.astype(np.float64)).to(dev)[:, None]
    tol3 = torch.from_numpy(4 * _ulp(tail) + 1e-6 * np.abs(tail)).to(dev)[:, None]
    fin = torch.isfinite(tail_d)
    over = (p - tail_d).masked_fill(inrec | ~fin, -np.inf)
    worst = float(over.max())
    bad = over > tol3
    if bool(bad.any()):
        t_b, n_b = (int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"P3 {label}: token {t_b} feature {n_b + row_offset} left out with p {float(p[t_b, n_b]):.9g} > "
                             f"tail {tail[t_b]:.9g} ({int(bad.sum())} pairs)")
    st = {"ratio": ratio, "over": worst, "full": int(full.sum()), "unbounded": int(unb.sum()), "pairs": int(c.size)}

    if mode == "sd":   # P4 / P5 from the restated operands
        rs = restate_int8_sd(x, bd, prepared, W)
        assert rs["dseed"] == SEED
        ok = rs["restated"] & ~rs["ambiguous"] & ~unb
        ok_d = torch.from_numpy(ok).to(dev)[:, None]
        call, mag = coarse_all(rs, b, dev, with_mag=True)
        c_em = call[tt_d, ff_d].cpu().numpy()
        tol5 = 2 * _ulp(u[tt, jj]) + 4 * 2.0 ** -24 * mag[tt_d, ff_d].cpu().numpy()
        del mag
        sel = ok[tt]
        err = np.abs(c - c_em) / tol5              # (in units of the tolerance)
        if sel.any() and err[sel].max() > 1.0:
            i = int(np.argmax(np.where(sel, err, -1)))
            raise AssertionError(f"P5 {label}: token {tt[i]} (m {rs['m'][tt[i]]}) feature {ff[i] + row_offset}: recorded c "
                                 f"{c[i]:.9g} != restated {c_em[i]:.9g} ({err[i]:.3g} x the f32 rounding bound "
                                 f"{tol5[i]:.3g}; {int((err[sel] > 1.0).sum())} pairs)")
        reach = call + band_proxy(rs, W, Z, dev).sqrt() * (1 - 1e-5) - 2e-5 * call.abs().clamp_min(1.0)
        miss = (reach > tail_d) & ~inrec & ok_d
        for f in skip:
            miss[:, f] = False
        if bool(miss.any()):
            t_b, n_b = (int(v) for v in torch.nonzero(miss)[0])
            raise AssertionError(f"P4 {label}: token {t_b} feature {n_b + row_offset} reaches {float(reach[t_b, n_b]):.9g} > "
                                 f"tail {tail[t_b]:.9g} but is not recorded ({int(miss.sum())} pairs)")
        st.update(p5=float(err[sel].max()) if sel.any() else 0.0, restated=int(ok.sum()), m_max=int(rs["m"].max()),
                  n_out=int(rs["out"].sum()))
        R["restate"] = rs
        del call, reach, miss
    del p, inrec, over
    st["peak_gib"] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    print(f"\n[{mode}] {label}: T={T} N={N} C={C} k={k}: {st}")
    R["stats"] = st
    return R


def _x(T, d, dev, seed, dtype=torch.bfloat16):
    return hostile.activations(T, d, dev, seed=seed).to(dtype)


# ---- the passes: weight-stream tiles (64 / 128 / 256 rows), row-major and tile-major MFMA ------------------------------------
@pytest.mark.parametrize("T,kind,dtype,k,C", [
    (1, "gauss", torch.float16, 32, 256),
    (16, "spiky0.2x100", torch.bfloat16, 32, 256),
    (64, "lognorm", torch.float32, 32, 256),
    (65, "spiky1x20n", torch.bfloat16, 32, 256),
    (200, "dup", torch.bfloat16, 8, 32),
], ids=["ws64-T1-f16", "ws64-T16", "ws64-T64-f32", "ws128-T65", "ws256-T200-dup-C32"])
def test_weight_stream_tiles(dev, T, kind, dtype, k, C):
    """d % 1024 == 0, T <= 256: csrc/gemm_skinny.h (64-, 128- and 256-row tiles); the shard sits at row_offset = 7 x 8192."""
    W, b, bd = hostile.weights(kind, N8, 1024, dev, seed=T)
    R = audit(dev, _x(T, 1024, dev, 100 + T, dtype), W, b, bd, k, C, mode="sd", row_offset=7 * N8, label=f"ws T={T} {kind}")
    if C == 32:   # more survivors than C: the tail is the best candidate left behind, not tau
        assert R["stats"]["full"] >= 0.9 * T


def test_row_major_mfma_pass_d512(dev):
    """T <= 256 with d % 1024 != 0: the 256 x 256-tile MFMA pass on row-major operands."""
    W, b, bd = hostile.weights("trained_like", N8, 512, dev, seed=3)
    audit(dev, _x(200, 512, dev, 4), W, b, bd, 32, 256, mode="sd", label="row-major d=512")


def test_row_major_mfma_pass_no_skinny(dev, monkeypatch):
    """The same pass at d = 1024 with the weight-stream kernel switched off, on round-to-nearest operands."""
    monkeypatch.setenv("MSAE_NO_SKINNY", "1")
    W, b, bd = hostile.weights("lognorm", N8, 1024, dev, seed=5)
    audit(dev, _x(100, 1024, dev, 6), W, b, bd, 32, 256, mode="rtn", row_offset=N8, label="row-major no-skinny")


@pytest.mark.parametrize("T,kind", [(257, "spiky5x20"), (4097, "trained_like")])
def test_tile_major_mfma_pass(dev, T, kind):
    """T > 256: the tile-major MFMA pass, with a partial last 256-row tile."""
    W, b, bd = hostile.weights(kind, N8, 1024, dev, seed=T)
    audit(dev, _x(T, 1024, dev, T + 1), W, b, bd, 32, 256, mode="sd", row_offset=7 * N8, label=f"tile-major T={T}")


def test_tau_tail_zero_rows_and_f32_input(dev):
    """C = 1024 > the survivors: the tail is tau.  The input is f32 that bf16 cannot represent, with all-zero rows (the int8
    pass gives them a one-unit scale, so their band is wide and tau > 0: they stay bounded and P2 / P3 hold on them)."""
    T, d = 300, 1024
    W, b, _ = hostile.weights("gauss", N8, d, dev, seed=7)
    b = -b.abs()
    bd = torch.zeros(d, device=dev)
    x = hostile.activations(T, d, dev, seed=8).float() * (1 + torch.rand(T, d, device=dev, generator=torch.Generator(
        device=dev).manual_seed(9)) * 2 ** -10)
    assert not torch.equal(x, x.to(torch.bfloat16).float())
    zero = [0, 131, 299]
    x[zero] = 0.0
    R = audit(dev, x, W, b, bd, 32, 1024, mode="sd", label="tau tail")
    nv = R["valid"].sum(axis=1)
    assert ((nv > 0) & (nv < 1024)).sum() >= 0.9 * (T - len(zero)), "the tail should come from tau here"


# ---- d: 128, 192 (the bf16 pass under the int8 mode), 12288 (quant_x_kernel's non-resident branch) ------------------------
@pytest.mark.parametrize("d,T", [(128, 300), (192, 300), (12288, 257)])
def test_widths(dev, d, T):
    W, b, bd = hostile.weights("lognorm", N8, d, dev, seed=d)
    mode = "i8-bf16" if d % 128 else "sd"   # (d % 128 != 0: the int8 mode runs the bf16 pass; its records have no restatement)
    with _mode("sd"):
        from msae import ops

        prepared = ops.prepare_encoder(W)
    audit(dev, _x(T, d, dev, d + 1), W, b, bd, 32, 256, mode=mode, prepared=prepared, row_offset=N8, label=f"d={d}")


# ---- operand modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,T,dtype", [("bf16", 300, torch.bfloat16), ("bf16", 64, torch.float16),
                                          ("rtn", 512, torch.bfloat16), ("rtn", 200, torch.float32)])
def test_operand_modes(dev, mode, T, dtype):
    """The bf16 pass and int8 rounded to nearest.  bf16, T = 300: all-zero rows under negative biases -- their coarse values
    are the biases with a zero band, tau <= 0, and the pass cannot bound them (P6)."""
    W, b, bd = hostile.weights("gauss", N8, 1024, dev, seed=T)
    x, zero = _x(T, 1024, dev, T + 2, dtype), []
    if mode == "bf16" and T == 300:
        b, bd, zero = -b.abs(), torch.zeros_like(bd), [0, 77, 299]
        x[zero] = 0
    audit(dev, x, W, b, bd, 32, 256, mode=mode, row_offset=2 * N8, unbounded=zero, label=f"{mode} T={T}")


def test_production_shard(dev):
    """d = 4096, T = 8192, one shard of G = 8 at the production width N = 131072 (N_shard = 16384), C = 32."""
    from msae.parallel import default_candidates

    C = default_candidates(32, 8)
    W, b, bd = hostile.weights("trained_like", 16384, 4096, dev, seed=11)
    audit(dev, _x(8192, 4096, dev, 12), W, b, bd, 32, C, mode="sd", row_offset=5 * 16384, label="production shard")


# ---- a batch with the full 128 outlier dims and every kind of multiplier -------------------------------------------------
def test_wide_outliers(dev):
    """128 outlier dims, per-token multipliers 2, 128, 200, 252 (remainder plane), 253 (coarse outlier steps) and 1100 (over
    M_MAX = 1040: no bound).  f32 input; the restated outlier set has exactly 128 dims and P5 checks the exact remainder."""
    T, d = 257, 4096
    W, b, _ = hostile.weights("gauss", N8, d, dev, seed=13)
    bd = torch.zeros(d, device=dev)
    g = torch.Generator(device=dev).manual_seed(14)
    x = (torch.rand(T, d, generator=g, device=dev) * 2 - 1) * torch.exp(torch.randn(T, 1, generator=g, device=dev))
    odim = torch.randperm(d, generator=g, device=dev)[:128]
    x[:, odim] = 0.0
    inmax = x.abs().max(dim=1).values
    ms = torch.randint(2, 253, (T,), generator=g, device=dev).float()
    pick = {2: 1, 128: 2, 200: 3, 252: 4, 253: 5, 1100: 6}
    for mv, t in pick.items():
        ms[t] = mv
    ms[7:20] = 252.0
    sign = torch.where(torch.rand(T, 128, generator=g, device=dev) < 0.5, -1.0, 1.0)
    mag = ms[:, None] - 1 + torch.rand(T, 128, generator=g, device=dev) * 0.9     # max over the row: m - 0.1 .. m - 1
    mag[:, 0] = ms - 0.05
    x[:, odim] = sign * mag * inmax[:, None]
    R = audit(dev, x, W, b, bd, 32, 256, mode="sd", unbounded=[pick[1100]], label="wide outliers")
    rs = R["restate"]
    assert int(rs["out"].sum()) == 128 and set(np.nonzero(rs["out"])[0]) == set(odim.cpu().numpy().tolist())
    for mv, t in pick.items():
        assert int(rs["m"][t]) == min(mv, 1040), (t, int(rs["m"][t]))
    assert rs["m_over"][pick[1100]] and not rs["restated"][pick[253]]
    assert R["stats"]["restated"] >= T - 10


# ---- hook edits, the stale-dither fallback, C above the list capacity --------------------------------------------------------
@pytest.mark.parametrize("inside", ["set", "zero"])
def test_hook_edits(dev, inside):
    """set_feature / zero_feature are global ids: the owning shard leaves the feature out, the others ignore it."""
    T, d, ro = 300, 1024, 3 * N8
    W, b, bd = hostile.weights("spiky0.1x1000", N8, d, dev, seed=15)
    x = _x(T, d, dev, 16)
    base = audit(dev, x, W, b, bd, 32, 256, mode="sd", row_offset=ro, label="no edit")
    ids, counts = np.unique(base["feat"][base["valid"]], return_counts=True)
    f_in = int(ids[counts.argmax()])                    # the feature the most records hold without the edit
    assert counts.max() > T // 10
    f_out = ro - 5
    sf, zf = (f_in, f_out) if inside == "set" else (f_out, f_in)
    audit(dev, x, W, b, bd, 32, 256, mode="sd", row_offset=ro, set_feature=sf, zero_feature=zf, label=f"edit {inside} inside")


def test_buffer_prepared_without_dither(dev):
    """A buffer prepared with the dither off has no shared dither vectors (dseed 0): a dithered call bounds no token."""
    from msae import ops

    T, d = 300, 1024
    W, b, bd = hostile.weights("gauss", N8, d, dev, seed=17)
    with _mode("rtn"):
        prepared = ops.prepare_encoder(W)
    R = audit(dev, _x(T, d, dev, 18), W, b, bd, 32, 256, mode="rtn", prepared=prepared, label="rtn buffer")
    assert R["stats"]["unbounded"] < T
    with _mode("sd"):
        recs = ops.shard_candidates(_x(T, d, dev, 18), b, bd, prepared, N8, 32, 0, 256)
    R = decode_records(recs, 256)
    assert np.isinf(R["tail"]).all() and not R["valid"].any(), "P6: dseed == 0 under a dithering call"


def test_C_above_capacity_is_not_implemented(dev):
    from msae import ops
    from msae._hip import MsaeNotImplemented

    W, b, bd = hostile.weights("gauss", N8, 1024, dev, seed=19)
    prepared = ops.prepare_encoder(W)
    with pytest.raises(MsaeNotImplemented):
        ops.shard_candidates(_x(300, 1024, dev, 20), b, bd, prepared, N8, 32, 0, 4096)   # cap = 2048 at k = 32
