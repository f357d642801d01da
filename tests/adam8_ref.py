"""Restatement of the blockwise 8-bit Adam moments (the "adam8" format of include/msae.h, csrc/train.hip: msae_adam8_rows_f32,
msae_adam8_quantize_f32, msae_adam8_dequantize_f32), the acceptance check the GPU tests and the host tests share, and their cases.
It builds on train_ref.py and changes nothing there.

The codec.  A code is OCP e4m3fn: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 is subnormal (mantissa * 2^-9),
0x7F / 0xFF are NaN and never written, the largest value is 448 (0x7E).  DECODE is the table, encode() rounds a float64 to the
nearest code, ties to the even code, after clamping to +-448.  Every code c has a rounding CELL [LO[c], HI[c]] in units of the
block's scale: the midpoints to its neighbours; the top code's cell is open upwards (the clamp), code 0's is [-HI[0], HI[0]].
For R8 (codes of sqrt(v), which never loses a positive value) code 0 holds only 0 and code 1's cell reaches down to 0 exclusive.

quantize() / dequantize() restate the two conversion kernels in numpy float32, operation for operation (one float32 division
for the scale and one for its inverse, one multiplication, the clamp, the rounding; three separate multiplications to decode):
the conversion kernels are compared with them bit for bit (+-0 codes count as equal).

adam8_rows() is one optimiser step: the state dequantised in numpy float32 (the bits the kernel sees), train_ref.adam_rows on
them (float64 W', m', v' with the derived bounds dW, dm, dv), r' = sqrt(v') with _sqrt_interval's bound dr.

accept() is the check of a kernel's result (W, M8, R8, SM, SR).  Every element, none excluded:
    W'       train_ref.assert_within
    scale    |S - absmax_ref / 448| <= max_block(dx) / 448 + 3 u S
    code c   with the kernel's OWN scale S, the reference value x satisfies  LO[c] S (1 - 4u) - dx <= x <= HI[c] S (1 + 4u) + dx
             (the kernel's q = x * fl(448 / absmax) and its S = fl(absmax / 448) are three roundings apart: 4 u covers them)
i.e. "this code is what correct rounding gives for some value inside the bound" -- no list of exempt elements."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

import train_ref as tr

BLOCK = 256
QMAX = 448.0
U = tr.U
F32 = np.float32


def _decode_table() -> np.ndarray:
    t = np.empty(256, np.float64)
    for c in range(256):
        s, e, m = (-1.0 if c & 0x80 else 1.0), (c >> 3) & 0xF, c & 7
        t[c] = np.nan if (e == 0xF and m == 7) else s * (m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return t


DECODE = _decode_table()                      # [256] float64; every value is a float32 too
POS = DECODE[:0x7F]                           # the 127 non-negative values, ascending: codes 0 .. 0x7E
MID = (POS[:-1] + POS[1:]) / 2                # MID[c]: the midpoint between codes c and c + 1
LO = np.concatenate([[0.0], MID])             # cell of magnitude code c: [LO[c], HI[c]]
HI = np.concatenate([MID, [np.inf]])


def encode(q) -> np.ndarray:
    """float64 -> uint8: clamp to +-448, nearest code, ties to the even code (subnormals included).  A negative value that
    rounds to zero keeps its sign bit (0x80), as the float32 -> e4m3 casts do."""
    q = np.asarray(q, np.float64)
    a = np.minimum(np.abs(q), QMAX)
    c = np.searchsorted(MID, a, side="left")              # a in (MID[c - 1], MID[c]]
    tie = (c < 126) & (a == MID[np.minimum(c, 125)])
    c = np.where(tie & (c % 2 == 1), c + 1, c)
    return (c | np.where(np.signbit(q), 0x80, 0)).astype(np.uint8)


def blocks_per_row(d: int) -> int:
    return -(-d // BLOCK)


def supported(shape) -> bool:
    """The shapes that get 8-bit moments (msae_adam8_blocks != 0)."""
    rows, d = tr.kernel_rows(shape)
    return d % 4 == 0 and d <= 8192 and rows * d >= 4096 and not (rows == 1 and d % 1024 != 0)


def _blocked(x: np.ndarray) -> np.ndarray:
    """[rows, d] -> [rows, bpr, 256], the partial last block padded with zeros."""
    rows, d = x.shape
    bpr = blocks_per_row(d)
    out = np.zeros((rows, bpr * BLOCK), x.dtype)
    out[:, :d] = x
    return out.reshape(rows, bpr, BLOCK)


def per_element(S: np.ndarray, rows: int, d: int) -> np.ndarray:
    """[nb] block values -> [rows, d]."""
    return np.repeat(np.asarray(S).reshape(rows, blocks_per_row(d)), BLOCK, axis=1)[:, :d]


@dataclasses.dataclass
class State:
    """An adam8 state on the host: codes uint8 [rows, d], scales float32 [nb]."""
    M8: np.ndarray
    R8: np.ndarray
    SM: np.ndarray
    SR: np.ndarray


def _quantize_one(x: np.ndarray, keep_positive: bool):
    """float32 [rows, d] -> (codes, scales): per block absmax / 448 and the codes of x * (448 / absmax), all in float32."""
    rows, d = x.shape
    xb = _blocked(x.astype(F32))
    am = np.abs(xb).max(axis=2)                                             # [rows, bpr] float32
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(am > 0, F32(QMAX) / am, F32(0)).astype(F32)
        S = (am / F32(QMAX)).astype(F32)
        q = np.clip((xb * inv[:, :, None]).astype(F32), F32(-QMAX), F32(QMAX))
    codes = encode(q.astype(np.float64))
    if keep_positive:
        codes = np.where((xb > 0) & ((codes & 0x7F) == 0), np.uint8(1), codes)
    return codes.reshape(rows, -1)[:, :d].copy(), S.reshape(-1)


def quantize(M, V) -> State:
    """The restatement of msae_adam8_quantize_f32, bit for bit: M, V float32 [rows, d] (V >= 0)."""
    M, V = np.asarray(M, F32), np.asarray(V, F32)
    M8, SM = _quantize_one(M, False)
    R8, SR = _quantize_one(np.sqrt(V).astype(F32), True)
    return State(M8, R8, SM, SR)


def dequantize(st: State):
    """-> (m, v) float32 [rows, d]: m = dec(M8) * SM, r = dec(R8) * SR, v = r * r -- three float32 multiplications."""
    rows, d = st.M8.shape
    dec = DECODE.astype(F32)
    m = (dec[st.M8] * per_element(st.SM, rows, d).astype(F32)).astype(F32)
    r = (dec[st.R8] * per_element(st.SR, rows, d).astype(F32)).astype(F32)
    return m, (r * r).astype(F32)


def same_codes(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: equal codes, 0x80 (-0) and 0x00 counting as the same."""
    z = lambda c: np.where((c & 0x7F) == 0, 0, c)
    return z(np.asarray(a)) == z(np.asarray(b))


def assert_quantized_exactly(got: State, M, V, what: str = "") -> None:
    """The conversion kernel against quantize(): the same codes and the same scale bits."""
    ref = quantize(M, V)
    for n in ("SM", "SR"):
        g, r = getattr(got, n), getattr(ref, n)
        assert g.shape == r.shape and np.array_equal(g.view(np.uint32), r.view(np.uint32)), f"{what} {n}: scale bits differ"
    for n in ("M8", "R8"):
        bad = ~same_codes(getattr(got, n), getattr(ref, n))
        assert not bad.any(), (f"{what} {n}: {int(bad.sum())} codes differ, first at {tuple(np.argwhere(bad)[0])}: "
                               f"got {getattr(got, n)[bad][0]:#x} ref {getattr(ref, n)[bad][0]:#x}")


# ---- one optimiser step ----------------------------------------------------------------------------------------------------------
def adam8_rows(W, G, st: State, step: int, lr: float, **kw):
    """-> dict(W, m, v, r, dW, dm, dv, dr): float64 [rows, d] tensors, from the float32 dequantised state."""
    rows, d = st.M8.shape
    m0, v0 = dequantize(st)
    shape = W.shape
    (W1, m1, v1), (dW, dm, dv) = tr.adam_rows(W, G, torch.from_numpy(m0).reshape(shape), torch.from_numpy(v0).reshape(shape),
                                              step, lr, **kw)
    W1, m1, v1, dW, dm, dv = (t.reshape(rows, d) for t in (W1, m1, v1, dW, dm, dv))
    r1, dr = tr._sqrt_interval(v1, dv)
    return dict(W=W1, m=m1, v=v1, r=r1, dW=dW, dm=dm, dv=dv, dr=dr)


def check_scales(S, x, dx, what: str) -> float:
    """Each scale against absmax_ref / 448 -> the largest ratio of error to bound."""
    rows, d = x.shape
    S = np.asarray(S, np.float64)
    assert S.shape == (rows * blocks_per_row(d),), f"{what}: {S.shape} scales for {rows * blocks_per_row(d)} blocks"
    assert np.isfinite(S).all() and (S >= 0).all(), f"{what}: a scale is negative or not finite"
    ref = np.abs(_blocked(x)).max(axis=2).reshape(-1) / QMAX
    bound = _blocked(dx).max(axis=2).reshape(-1) / QMAX + 3 * U * S
    err = np.abs(S - ref)
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} scales outside their bound; block {int(np.argmax(err - bound))}: "
                           f"got {S[np.argmax(err - bound)]!r} ref {ref[np.argmax(err - bound)]!r}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check_codes(codes, S, x, dx, keep_positive: bool, what: str) -> None:
    """Each code, read at the kernel's own scale, is what correct rounding gives for some value within dx of x."""
    rows, d = x.shape
    codes = np.asarray(codes)
    assert codes.shape == (rows, d) and codes.dtype == np.uint8
    k = (codes & 0x7F).astype(np.int64)
    assert not (k == 0x7F).any(), f"{what}: a NaN code was written"
    Se = per_element(np.asarray(S, np.float64), rows, d)
    neg = codes >= 0x80
    if keep_positive:
        assert not (neg & (k > 0)).any(), f"{what}: a negative code for a square root"
    sx = np.where(neg & (k > 0), -x, x)                       # x along the code's sign
    top = np.isinf(HI[k])                                     # the top code's cell is open upwards
    lower = LO[k] * Se * (1 - 4 * U) - dx
    upper = np.where(top, np.inf, np.where(top, 0.0, HI[k]) * Se * (1 + 4 * U) + dx)
    zero = k == 0
    if keep_positive:                                         # code 0 holds only 0; code 1 reaches down to 0 exclusive
        ok = np.where(zero, np.abs(x) <= dx, ((sx >= lower) | (k == 1)) & (sx <= upper))
        ok &= ~((k == 1) & (x + dx <= 0))
    else:
        ok = np.where(zero, np.abs(x) <= upper, (sx >= lower) & (sx <= upper))
    ok &= ~((Se == 0) & ~zero)                                # an all-zero block: scale 0 AND codes 0
    if not ok.all():
        i = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} codes are not a correct rounding; first at {i}: code "
                             f"{int(codes[i]):#x} scale {Se[i]!r} ref {x[i]!r} +- {dx[i]:.3e} cell [{LO[k[i]]}, {HI[k[i]]}] * scale")


def accept(got_W, got: State, ref: dict, what: str = "") -> dict:
    """The acceptance check of one step's result -> the error / bound ratios of W and of the two scale arrays."""
    n = lambda t: t.numpy()
    out = {"W": tr.assert_within(got_W, ref["W"], ref["dW"], f"{what} W")}
    out["SM"] = check_scales(got.SM, n(ref["m"]), n(ref["dm"]), f"{what} SM")
    out["SR"] = check_scales(got.SR, n(ref["r"]), n(ref["dr"]), f"{what} SR")
    check_codes(got.M8, got.SM, n(ref["m"]), n(ref["dm"]), False, f"{what} M8")
    check_codes(got.R8, got.SR, n(ref["r"]), n(ref["dr"]), True, f"{what} R8")
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# the shapes of the GPU file: each is the smallest that reaches its edge of the kernel
SHAPES = [(8, 512),            # the smallest matrix that gets 8-bit moments
          (7, 1000),           # a partial block of 232
          (4, 1028),           # a second trip whose block has 4 elements
          (3, 8188), (3, 8192),    # the KEEP window
          (1, 4096),           # one row
          (4096,), (3072,)]    # the [rows, 1024] view of a vector ((3072,) lies below the 4096-element floor: policy, not the kernel's)
UNSUPPORTED = [(2, 8196), (5, 50), (4100,)]


def _cases():
    by_shape = {}
    for c in tr.ADAM_CASES:
        by_shape.setdefault(c.shape, []).append(c)
    out = list(by_shape[(7, 1000)])                                          # every hyper-parameter case
    for sh in SHAPES + [s for s in by_shape if supported(s) and s not in SHAPES]:
        if sh == (7, 1000):
            continue
        out += by_shape.get(sh) or [tr.AdamCase(name="shape" + "x".join(map(str, sh)), shape=sh)]
    return out


CASES = _cases()
# the code-1 clamp inside a step: see inputs()
CLAMP_CASE = tr.AdamCase(name="clamp1-7x1000", shape=(7, 1000), project=False, sumsq="none", norm_ratio=None)
CLAMP_AT, CLAMP_BIG = (0, 5), (0, 3)


def inputs(case):
    """-> W, G (float32 tensors shaped case.shape), the warm State (train_ref.adam_inputs' M, V through quantize()), S.
    CLAMP_CASE plants, in block 0 of row 0: one gradient of 0.1 (the block's new absmax of sqrt(v) is ten times the old one)
    and one element with no gradient, a normal m and the smallest stored sqrt(v) (code 1): its new sqrt(v) is 2e-7 of the
    block's absmax and rounds to code 0 unless it is kept at code 1, while its m' = 0.9 m is far from flushed."""
    W, G, M, V, S = tr.adam_inputs(case)
    rows, d = tr.kernel_rows(case.shape)
    M2, V2 = M.reshape(rows, d).clone(), V.reshape(rows, d).clone()
    if case is CLAMP_CASE:
        G = G.clone()
        G[CLAMP_BIG], G[CLAMP_AT] = 0.1, 0.0
        M2[CLAMP_AT] = 1e-4
        V2[CLAMP_AT] = float(V2[0, :BLOCK].max()) * 1e-14
    st = quantize(M2.numpy(), V2.numpy())
    if case is CLAMP_CASE:
        assert st.R8[CLAMP_AT] == 1
    return W, G, st, S


def planted(kind: str):
    """Planted blocks for the conversion kernels -> (M, V, R = sqrt(V)) float32 [8, 512]: block 0 of every row is the planted
    one, block 1 is random."""
    gen = tr._gen("adam8" + kind)
    rows, d = 8, 512
    M = (torch.randn(rows, d, generator=gen) * 1e-4).numpy()
    R = (torch.rand(rows, d, generator=gen) * 3e-4 + 1e-6).numpy()
    pos = POS.astype(F32)
    if kind == "zero_block":
        M[:, :BLOCK], R[:, :BLOCK] = 0.0, 0.0
    elif kind == "one_nonzero":
        M[:, :BLOCK], R[:, :BLOCK] = 0.0, 0.0
        M[:, 17], R[:, 200] = -3e-5, 2e-4
    elif kind == "all_equal":
        M[:, :BLOCK], R[:, :BLOCK] = -7e-5, 1.5e-4
    elif kind in ("every_code", "subnormals", "midpoints"):
        # absmax = 448 * 2^-k: the scale and its inverse are powers of two, q = x * 2^k is exact
        for r in range(rows):
            s = F32(2.0 ** -(10 + r))
            if kind == "every_code":
                vals = pos                                             # 127 values: must round-trip bit for bit
            elif kind == "subnormals":
                vals = np.concatenate([np.linspace(0, 2.0 ** -6, 120, dtype=F32), [F32(QMAX)]])     # 0 .. the first normal binade
            else:
                vals = np.concatenate([MID[:125].astype(F32), [F32(QMAX)]])    # every midpoint (exact in float32): ties to even
            blk = np.zeros(BLOCK, F32)
            blk[:len(vals)] = vals * s
            R[r, :BLOCK] = blk
            sign = np.where(np.arange(BLOCK) % 2 == 0, 1, -1).astype(F32)
            sign[len(vals) - 1] = 1
            M[r, :BLOCK] = blk * sign
    elif kind == "clamp1":
        R[:, 9] = R[:, :BLOCK].max(axis=1) * F32(1e-7)               # sqrt(v) at 1e-7 of its block's absmax: code 1, not 0
        M[:, 9] = 1e-4
    else:
        raise ValueError(kind)
    return M.astype(F32), (R.astype(F32) ** 2).astype(F32), R.astype(F32)


PLANTED = ["zero_block", "one_nonzero", "all_equal", "every_code", "midpoints", "subnormals", "clamp1"]
