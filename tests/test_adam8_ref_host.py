"""tests/adam8_ref.py on the CPU: the e4m3 codec against its own table and against torch's float8_e4m3fn cast, the step
restatement against a plain float64 Adam on the dequantised state, an independent float32 evaluation of the 8-bit step inside
the acceptance check on every case the GPU file runs (test_gpu_adam8.py) -- and each of a list of nearly-correct 8-bit optimisers
rejected by that same check."""
import math

import numpy as np
import pytest
import torch

import adam8_ref as a8
import train_ref as tr

F32 = np.float32


# ---- the codec -----------------------------------------------------------------------------------------------------------------------
def test_codec_round_trip_over_all_codes():
    codes = np.arange(256, dtype=np.uint8)
    nan = (codes & 0x7F) == 0x7F
    assert np.isnan(a8.DECODE[nan]).all() and np.isfinite(a8.DECODE[~nan]).all()
    assert a8.DECODE[0x7E] == 448.0 and a8.DECODE[0x01] == 2.0 ** -9 and a8.DECODE[0x08] == 2.0 ** -6 and a8.DECODE[0x38] == 1.0
    assert (np.diff(a8.POS) > 0).all()
    assert np.array_equal(a8.DECODE.astype(F32).astype(np.float64)[~nan], a8.DECODE[~nan])         # every value is a float32
    back = a8.encode(a8.DECODE[~nan])
    assert np.array_equal(back, codes[~nan])                     # -0 (0x80) keeps its sign bit
    # the cells: the inside of a cell rounds to its code, a midpoint to the even neighbour, beyond 448 clamps
    for c in range(127):
        lo, hi = a8.LO[c], a8.HI[c]
        inside = np.nextafter(lo, np.inf) if c else 0.0, (np.nextafter(hi, 0) if np.isfinite(hi) else 1e9)
        assert list(a8.encode(np.array(inside))) == [c, c]
        if c < 126:
            assert int(a8.encode(np.array([hi]))[0]) == (c if c % 2 == 0 else c + 1)
            assert int(a8.encode(np.array([-hi]))[0]) == 0x80 | (c if c % 2 == 0 else c + 1)


def test_codec_equals_torch_float8_e4m3fn():
    """An independent check: the table is torch's uint8 -> float8_e4m3fn -> float, the encoder is torch's CPU cast on 200k
    in-range values with every code and every midpoint among them."""
    codes = torch.arange(256, dtype=torch.uint8)
    table = codes.view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    nan = np.isnan(a8.DECODE)
    assert np.array_equal(np.isnan(table), nan) and np.array_equal(table[~nan], a8.DECODE[~nan])
    gen = tr._gen("adam8codec")
    x = torch.cat([(torch.rand(100_000, generator=gen) * 2 - 1) * 448, torch.randn(99_000, generator=gen) * 0.05,
                   torch.from_numpy(np.concatenate([a8.POS, -a8.POS, a8.MID, -a8.MID])).float()])
    got = a8.encode(x.double().numpy())
    ref = x.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert a8.same_codes(got, ref).all()


def test_quantize_restatement_on_the_planted_blocks():
    for kind in a8.PLANTED:
        M, V, R = a8.planted(kind)
        st = a8.quantize(M, V)
        m, v = a8.dequantize(st)
        blk = slice(0, a8.BLOCK)
        assert not ((st.M8 & 0x7F) == 0x7F).any() and not ((st.R8 & 0x7F) == 0x7F).any()
        if kind == "zero_block":
            assert not st.SM.reshape(8, 2)[:, 0].any() and not st.M8[:, blk].any() and not st.R8[:, blk].any()
        if kind == "every_code":                                  # exact values come back bit for bit
            assert np.array_equal(m[:, blk], M[:, blk]) and np.array_equal(v[:, blk], V[:, blk])
            assert np.array_equal(st.R8[0, :127], np.arange(127, dtype=np.uint8))
        if kind == "midpoints":                                   # ties to the even code
            assert ((st.M8[:, :125] & 0x7F) % 2 == 0).all() and (st.R8[:, 1:125] % 2 == 0).all()
            assert np.array_equal(st.M8[0, :125] & 0x7F, np.arange(125) + (np.arange(125) % 2))
            assert (st.R8[:, 0] == 1).all()                       # the tie between 0 and code 1: a positive sqrt(v) stays code 1
        if kind == "clamp1":
            assert (st.R8[:, 9] == 1).all() and (R[:, 9] > 0).all()
        assert ((st.R8 & 0x7F)[R > 0] > 0).all(), "a positive sqrt(v) was lost"
        a8.assert_quantized_exactly(st, M, V, kind)


# ---- float32 restatements of the 8-bit step: plain torch sums, the codec above, and the ways to get it nearly right ----------------
def _encode_f32(x, am, mutant=None):
    """codes of the [rows, bpr, 256] float32 blocks x at block absmax am [rows, bpr]."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.where(am > 0, F32(448) / am, F32(0)).astype(F32)
        q = np.clip((x * inv[:, :, None]).astype(F32), F32(-448), F32(448)).astype(np.float64)
    if mutant == "truncate":
        c = np.searchsorted(a8.POS, np.abs(q), side="right") - 1
        return (c | np.where(np.signbit(q), 0x80, 0)).astype(np.uint8)
    if mutant == "ties_away":
        a = np.abs(q)
        c = np.searchsorted(a8.MID, a, side="right")              # a == MID[c] goes up
        return (c | np.where(np.signbit(q), 0x80, 0)).astype(np.uint8)
    return a8.encode(q)


def quantize_f32(m, r, old: a8.State, mutant=None) -> a8.State:
    """m, r = sqrt(v) float32 [rows, d] -> State, with one thing wrong if `mutant` names it."""
    rows, d = m.shape
    out = []
    for x, keep_positive, name in ((m, False, "M"), (r, True, "R")):
        if mutant == "v_not_sqrt" and name == "R":
            x = (x * x).astype(F32)
        xb = a8._blocked(x.astype(F32))
        am = np.abs(xb).max(axis=2)
        am_q = am
        if mutant == "row_absmax":
            am = am_q = np.broadcast_to(am.max(axis=1, keepdims=True), am.shape)
        elif mutant == "block128":                                # codes at the absmax of each half, one scale per 256
            h = np.abs(xb.reshape(rows, -1, 2, 128)).max(axis=3)
            codes = _encode_f32(xb.reshape(rows, -1, 128), h.reshape(rows, -1)).reshape(rows, -1, 256)
        elif mutant == "prev_scale":
            am = am_q = (getattr(old, "S" + name).reshape(rows, -1) * F32(448)).astype(F32)
        elif mutant == "sm_for_r" and name == "R":
            am_q = np.abs(a8._blocked(m.astype(F32))).max(axis=2)
        if mutant != "block128":
            codes = _encode_f32(xb, am_q, mutant)
        if keep_positive and mutant != "no_clamp1":
            codes = np.where((xb > 0) & ((codes & 0x7F) == 0), np.uint8(1), codes)
        out.append((codes.reshape(rows, -1)[:, :d].copy(), (am / F32(448)).astype(F32).reshape(-1)))
    return a8.State(out[0][0], out[1][0], out[0][1], out[1][1])


def adam8_f32(W, G, st: a8.State, step, lr, betas=(0.9, 0.999), eps=1e-8, total_sumsq=None, max_norm=1.0, project=False,
              mutant=None):
    """-> (W' float32 tensor [rows, d], State)."""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    rows, d = st.M8.shape
    m0, v0 = (torch.from_numpy(x) for x in a8.dequantize(st))
    W, G = W.reshape(rows, d), G.reshape(rows, d)
    c = t(1.0)
    if total_sumsq is not None:
        c = torch.minimum(t(max_norm) / (torch.sqrt(total_sumsq.reshape(()).float()) + t(1e-6)), t(1.0))
    g = G * c
    if project:
        g = g - (g * W).sum(1, keepdim=True) * W
    m1 = m0 + (g - m0) * (t(1.0) - t(betas[0]))
    v1 = t(betas[1]) * v0 + (t(1.0) - t(betas[1])) * g * g
    new = quantize_f32(m1.numpy(), torch.sqrt(v1).numpy(), st, mutant)
    if mutant == "update_from_requantized":
        m1, v1 = (torch.from_numpy(x) for x in a8.dequantize(new))
    bc1 = t(1.0 - float(t(betas[0])) ** step)
    bc2s = t(math.sqrt(1.0 - float(t(betas[1])) ** step))
    w1 = W - (t(lr) / bc1) * (m1 / (torch.sqrt(v1) / bc2s + t(eps)))
    return w1, new


def _run(case, mutant=None):
    W, G, st, S = a8.inputs(case)
    ref = a8.adam8_rows(W, G, st, case.step, case.lr, total_sumsq=S, **case.kwargs())
    w1, new = adam8_f32(W, G, st, case.step, case.lr, total_sumsq=S, mutant=mutant, **case.kwargs())
    return a8.accept(w1, new, ref, f"{case.name} {mutant or ''}")


_ALL = a8.CASES + [a8.CLAMP_CASE]


def test_restatement_equals_plain_float64_adam_on_the_dequantised_state():
    case = next(c for c in a8.CASES if c.name == "project_off-7x1000")
    W, G, st, _ = a8.inputs(case)
    S = float((G.double() ** 2).sum())        # (the cases carry S rounded to float32, as the kernel reads it; here: the exact one)
    ref = a8.adam8_rows(W, G, st, case.step, case.lr, total_sumsq=S, **case.kwargs())
    m0, v0 = (torch.from_numpy(x).double() for x in a8.dequantize(st))
    p = torch.nn.Parameter(W.double().clone())
    opt = torch.optim.Adam([p], lr=tr.f32(case.lr), betas=tuple(tr.f32(b) for b in case.betas), eps=tr.f32(case.eps))
    opt.state[p] = {"step": torch.tensor(float(case.step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    p.grad = G.double().clone()
    torch.nn.utils.clip_grad_norm_([p], tr.f32(case.max_norm))
    opt.step()
    close = lambda a, r: torch.testing.assert_close(a, r, rtol=1e-9, atol=0.0)
    close(ref["W"], p.data); close(ref["m"], opt.state[p]["exp_avg"]); close(ref["v"], opt.state[p]["exp_avg_sq"])
    close(ref["r"], opt.state[p]["exp_avg_sq"].sqrt())
    # the dequantised state is within half a cell of what was quantised
    _, _, M, V, _ = tr.adam_inputs(case)
    assert float((m0 - M.double()).abs().max()) <= float(M.abs().max()) / 16 * 1.01


@pytest.mark.parametrize("case", _ALL, ids=[c.name for c in _ALL])
def test_float32_evaluation_passes_the_acceptance_check(case):
    ratios = _run(case)
    print(f"\nadam8 f32 {case.name}: max err/bound W {ratios['W']:.3f} SM {ratios['SM']:.3f} SR {ratios['SR']:.3f}")


_ON = ["step2-7x1000", "shape4x1028", "shape8x512", "shape3x8188", "shape4096"]
_MUTANTS = {
    "truncate": _ON,
    "block128": _ON,
    "row_absmax": _ON,                        # (every one of these rows is longer than a block)
    "prev_scale": _ON + ["sumsq_zero-7x1000"],
    "v_not_sqrt": _ON,
    "sm_for_r": _ON,
    "no_clamp1": ["clamp1-7x1000"],
    "update_from_requantized": _ON,
}


@pytest.mark.parametrize("mutant", list(_MUTANTS))
def test_acceptance_check_rejects(mutant):
    by_name = {c.name: c for c in _ALL}
    for name in _MUTANTS[mutant]:
        with pytest.raises(AssertionError):
            _run(by_name[name], mutant)
        _run(by_name[name])                   # ... and accepts the same case done right


def test_ties_away_from_zero_is_rejected_on_the_planted_midpoints():
    """A tie can only be told from its neighbours where q is exact: the planted midpoints of the conversion kernel's check."""
    M, V, R = a8.planted("midpoints")
    good = quantize_f32(M, R, None)
    a8.assert_quantized_exactly(good, M, V, "midpoints")
    bad = quantize_f32(M, R, None, "ties_away")
    with pytest.raises(AssertionError):
        a8.assert_quantized_exactly(bad, M, V, "midpoints ties_away")
    with pytest.raises(AssertionError):
        a8.assert_quantized_exactly(quantize_f32(M, R, None, "truncate"), M, V, "midpoints truncate")
    M, V, R = a8.planted("clamp1")
    with pytest.raises(AssertionError):
        a8.assert_quantized_exactly(quantize_f32(M, R, None, "no_clamp1"), M, V, "clamp1 no_clamp1")


def test_shape_rules():
    for sh in a8.SHAPES:
        assert sh == (3072,) or a8.supported(sh), sh
    for sh in a8.UNSUPPORTED:
        assert not a8.supported(sh), sh
    assert {c.shape for c in a8.CASES} >= set(a8.SHAPES)
