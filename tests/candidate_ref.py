"""Restatements of the int8 / bf16 candidate pass for the tests that audit its records (tests/test_gpu_band.py,
tests/test_gpu_candidate_audit.py, and the host-only checks in tests/test_host_properties.py).

The feature-sharded engine's sender (msae_shard_candidates) writes, per token, the C best candidates of its shard as
(upper value u = c + z sigma, band z sigma) and a tail: the largest upper value left out of the record, else the threshold
tau every non-candidate stayed below, else +inf when the shard cannot bound the token.  These helpers decode that record,
restate the prepared buffer's tables (csrc/encode_defs.h struct Prepared), restate quant_x_kernel<SD> with the outlier
remainder computed EXACTLY, and compute the exact f64 pre-activations and the restated coarse value of every pair.

Only `exact_pre` and `coarse_all` need a device (f64 GEMMs, in chunks); everything else is numpy.
"""
from __future__ import annotations

import numpy as np
import torch

MAX_OUT = 128               # csrc/encode_prep.h: outlier dims of a batch
SD_M_EXACT = 252            # csrc/encode_defs.h: largest multiplier with a remainder plane
M_MAX = 1040                # quant_x_kernel: larger multipliers are clamped and the token guarded
AMBIGUOUS = 2.0 ** -14      # a remainder this close to a floor boundary may round to either neighbour


# ---- the prepared buffer and the records ----------------------------------------------------------------------------------
def _header(prepared: torch.Tensor) -> dict:
    """csrc/encode_defs.h struct Prepared, as prepare_impl copies it to the head of the buffer."""
    raw = prepared[:256].cpu().numpy().tobytes()
    u32 = np.frombuffer(raw, dtype=np.uint32)
    u64 = np.frombuffer(raw, dtype=np.uint64)
    names = ["off_wb", "off_ws", "off_wstat", "off_wstat_s", "off_colbf", "off_colbf_s", "off_wq", "off_wqs", "off_wqp",
             "off_wqsp", "off_wqf", "off_wqsf", "bytes"]
    h = {"magic": int(u32[0]), "N": int(u32[1]), "d": int(u32[2]), "S": int(u32[3]), "valid": int(u32[30])}
    for i, n in enumerate(names):
        h[n] = int(u64[2 + i])
    h["dseed"], h["off_ds"], h["off_sdtab"] = int(u64[16]), int(u64[17]), int(u64[18])
    return h


def _view(prepared: torch.Tensor, off: int, nbytes: int, dtype) -> np.ndarray:
    return np.frombuffer(prepared[off:off + nbytes].cpu().numpy().tobytes(), dtype=dtype)


def decode_records(recs: torch.Tensor, C: int) -> dict:
    """records uint8 [T, 12 C + 8] -> valid [T, C] bool, u f32, feat int64 (global ids), zs f32 (z sigma), tail f32 [T]
    (tail[0] of the record: the shard's bound on everything it left out), keys uint64."""
    raw = recs.cpu().numpy()
    T = raw.shape[0]
    keys = np.frombuffer(raw[:, :8 * C].tobytes(), dtype=np.uint64).reshape(T, C)
    zs = np.frombuffer(raw[:, 8 * C:12 * C].tobytes(), dtype=np.float32).reshape(T, C)
    tail = np.frombuffer(raw[:, 12 * C:12 * C + 8].tobytes(), dtype=np.float32).reshape(T, 2)[:, 0]
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    bits = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi).astype(np.uint32)
    u = bits.view(np.float32)
    feat = (0x7FFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int64)
    return {"valid": keys != 0, "u": u, "feat": feat, "zs": zs, "tail": tail.copy(), "keys": keys}


def _records(recs: torch.Tensor, C: int):
    r = decode_records(recs, C)
    return r["valid"], r["u"], r["feat"], r["zs"]


# ---- the outlier remainder: three evaluations of A - m hi (A = v / scale, in steps) --------------------------------------
def remainder_f32(v, scale, m, hi) -> np.ndarray:
    """The evaluation before the fix: (v * inv) - m hi in f32, rounded at |A| up to 127 m."""
    inv = (np.float32(1.0) / np.asarray(scale, np.float32)).astype(np.float32)
    sv = (np.asarray(v, np.float32) * inv).astype(np.float32)
    return (sv - (np.asarray(m).astype(np.float32) * np.asarray(hi, np.float32)).astype(np.float32)).astype(np.float32)


def remainder_fma(v, scale, m, hi) -> np.ndarray:
    """quant_x_kernel<SD>: fmaf(-(m hi), scale, v) * inv.  The f64 product and difference are exact (m hi < 2^15, scale and
    v are f32: at most 40 significant bits), so rounding them to f32 once is the fused multiply-add."""
    scale = np.asarray(scale, np.float32)
    inv = (np.float32(1.0) / scale).astype(np.float32)
    mh = np.asarray(m).astype(np.float64) * np.asarray(hi, np.float64)
    f = (np.asarray(v, np.float32).astype(np.float64) - mh * scale.astype(np.float64)).astype(np.float32)
    return (f * inv).astype(np.float32)


def remainder_exact(v, scale, m, hi) -> np.ndarray:
    return (np.asarray(v, np.float32).astype(np.float64) / np.asarray(scale, np.float32).astype(np.float64)
            - np.asarray(m).astype(np.float64) * np.asarray(hi, np.float64))


def floor_exact(rem: np.ndarray, r: np.ndarray):
    """floor(rem + r) of the exact remainder -> (q int64, ambiguous: closer than 2^-14 step to the floor boundary)."""
    s = np.asarray(rem, np.float64) + np.asarray(r, np.float64)
    q = np.floor(s)
    frac = s - q
    return q.astype(np.int64), np.minimum(frac, 1.0 - frac) < AMBIGUOUS


# ---- quant_x_kernel<SD> restated ----------------------------------------------------------------------------------------
def outlier_dims(a: np.ndarray) -> np.ndarray:
    """pick_outliers_kernel: column max > 8 x the mean column max, threshold x1.5 until at most 128 qualify."""
    colmax = np.abs(a).max(axis=0)
    thr = np.float32(8.0) * colmax.sum(dtype=np.float32) / np.float32(a.shape[1])
    while (colmax > thr).sum() > MAX_OUT:
        thr = np.float32(thr * np.float32(1.5))
    return colmax > thr


def _a32(x: torch.Tensor, b_dec) -> np.ndarray:
    a = x.float().cpu()
    if b_dec is not None:
        a = a - b_dec.float().cpu()
    return a.numpy().astype(np.float32)


def _sd_tables(prepared: torch.Tensor, h: dict, d: int):
    tab = _view(prepared, h["off_sdtab"], d * 4, np.int32).astype(np.int64) & 0xFFFFFFFF
    F = int(_view(prepared, h["off_sdtab"] + ((d + 1) & ~1) * 4, 8, np.int64)[0])
    hx, hw = tab >> 16, tab & 0xFFFF
    rx = (2 * hx + 1).astype(np.float32) * np.float32(1.0 / 131072.0)
    rw = (2 * hw + 1).astype(np.float32) * np.float32(1.0 / 131072.0)
    return tab, F, rx, rw, 2 * hx + 1 - 65536, 2 * hw + 1 - 65536


def _quant_tokens(a: np.ndarray, out: np.ndarray, rx: np.ndarray, gw: np.ndarray, F: int, remainder: str):
    T, d = a.shape
    aa = np.abs(a)
    m_in = np.where(out[None, :], 0, aa).max(axis=1)
    m_out = np.where(out[None, :], aa, 0).max(axis=1) if out.any() else np.zeros(T, np.float32)
    scale = np.where(m_in > 0, m_in / np.float32(127.0),
                     np.where(m_out > 0, m_out / np.float32(127.0), np.float32(1.0))).astype(np.float32)
    m_raw = np.ceil((m_out / (np.float32(127.0) * scale)).astype(np.float32)).astype(np.int64)
    m_over = m_raw > M_MAX
    m = np.clip(m_raw, 1, M_MAX)
    coarse = m > SD_M_EXACT
    inv = (np.float32(1.0) / scale).astype(np.float32)
    inv_o = (np.float32(1.0) / (scale * m.astype(np.float32))).astype(np.float32)
    sv = (a * inv[:, None]).astype(np.float32)
    q = np.clip(np.floor((sv + rx[None, :]).astype(np.float32)), -127, 127).astype(np.int64)
    amb = np.zeros((T, d), bool)
    hi = np.zeros((T, d), np.int64)
    oc = np.nonzero(out)[0]
    if oc.size:
        v = a[:, oc]
        h = np.clip(np.rint((v * inv_o[:, None]).astype(np.float32)), -127, 127)
        mm = m[:, None]
        if remainder == "exact":
            qo, ao = floor_exact(remainder_exact(v, scale[:, None], mm, h), rx[oc][None, :])
        else:
            f = remainder_fma if remainder == "fma" else remainder_f32
            qo = np.floor((f(v, scale[:, None], mm, h) + rx[oc][None, :]).astype(np.float32)).astype(np.int64)
            ao = np.zeros_like(qo, dtype=bool)
        qo = np.clip(qo, -127, 127)
        cz = coarse[:, None]
        q[:, oc] = np.where(cz, 0, qo)
        amb[:, oc] = ao & ~cz
        hi[:, oc] = np.where(cz, 0, h.astype(np.int64))   # (coarse tokens: a dithered tile entry, not restated)
    Aq = q + m[:, None] * hi
    E = np.rint((Aq @ gw).astype(np.float64) / 131072.0 - float(F) / 131072.0 ** 2).astype(np.int64)
    return Aq, scale, m, m_over, coarse, E, amb


def _emulate(x: torch.Tensor, bd: torch.Tensor, tab: np.ndarray, F: int, remainder: str = "exact"):
    """quant_x_kernel<SD> restated: -> (a f32 [T, d], Aq int64 [T, d], sx f32 [T], m int [T], E int64 [T], g_x, outliers)."""
    a = _a32(x, bd)
    out = outlier_dims(a)
    assert out.sum() <= MAX_OUT
    hx, hw = tab >> 16, tab & 0xFFFF
    rx = (2 * hx + 1).astype(np.float32) * np.float32(1.0 / 131072.0)
    Aq, scale, m, _, _, E, _ = _quant_tokens(a, out, rx, 2 * hw + 1 - 65536, F, remainder)
    return a, Aq, scale, m, E, 2 * hx + 1 - 65536, out


def restate_int8_sd(x: torch.Tensor, b_dec, prepared: torch.Tensor, W: torch.Tensor | None = None,
                    remainder: str = "exact") -> dict:
    """The int8 subtractive-dither pass's operands restated from the prepared buffer's own tables:
    Aq int64 [T, d] (outlier dims: m hi + floor(exact remainder + r_x)), sx f32 [T], m int64 [T], E int64 [T], Wq int64 [N, d],
    sw f64 [N], Ds f64 [N] (= sw D), the outlier set, and per token: `restated` (the multiplier has a remainder plane and is not
    clamped), `ambiguous` (an outlier element within 2^-14 step of a floor boundary: its integer is either neighbour).
    With W given, the weights' side is checked against its definition (Wq = floor(W / sw + r_w), Ds = sw sum Wq g_x)."""
    h = _header(prepared)
    N, d = h["N"], h["d"]
    tab, F, rx, rw, gx, gw = _sd_tables(prepared, h, d)
    Wq = _view(prepared, h["off_wq"], N * d, np.int8).reshape(N, d).astype(np.int64)
    wstat = _view(prepared, h["off_wstat"], N * 16, np.float32).reshape(N, 4)
    ds = _view(prepared, h["off_ds"], N * 4, np.float32).astype(np.float64)
    sw32 = wstat[:, 0]
    if W is not None:
        Wn = W.float().cpu().numpy()
        with np.errstate(divide="ignore"):   # (an all-zero row: sw = 0, inv = 0, Wq = floor(r_w) = 0)
            inv_w = np.where(sw32 > 0, np.float32(1.0) / sw32, np.float32(0.0)).astype(np.float32)
        Wq_em = np.clip(np.floor(((Wn * inv_w[:, None]).astype(np.float32) + rw[None, :]).astype(np.float32)), -127, 127)
        assert np.array_equal(Wq_em.astype(np.int64), Wq), "row_stats_quant_row: shared dither r_w(c)"
        D = (Wq @ gx).astype(np.float64) / 131072.0
        assert np.allclose(ds, sw32.astype(np.float64) * D, rtol=2e-6, atol=1e-7), "Ds != sw D"
    a = _a32(x, b_dec)
    out = outlier_dims(a)
    Aq, sx, m, m_over, coarse, E, amb = _quant_tokens(a, out, rx, gw, F, remainder)
    return {"a": a, "Aq": Aq, "sx": sx, "m": m, "m_over": m_over, "E": E, "Wq": Wq, "sw": sw32.astype(np.float64), "Ds": ds,
            "out": out, "restated": ~coarse & ~m_over, "ambiguous": amb.any(axis=1), "dseed": h["dseed"]}


# ---- f64 references on the device ---------------------------------------------------------------------------------------
def exact_pre(x: torch.Tensor, W: torch.Tensor, b_enc, b_dec, chunk: int = 16384) -> torch.Tensor:
    """p [T, N] f64 on x's device: (x - b_dec in f32, as every kernel forms it) . W_n + b_n in f64."""
    a = x.float()
    if b_dec is not None:
        a = a - b_dec.float()
    a = a.double()
    N = W.shape[0]
    p = torch.empty(a.shape[0], N, dtype=torch.float64, device=x.device)
    for n0 in range(0, N, chunk):
        n1 = min(N, n0 + chunk)
        torch.matmul(a, W[n0:n1].double().T, out=p[:, n0:n1])
        if b_enc is not None:
            p[:, n0:n1] += b_enc[n0:n1].double()
    return p


def coarse_all(rs: dict, b_enc, dev, chunk: int = 8192, with_mag: bool = False):
    """The restated coarse value of EVERY pair, c = ((Aq . Wq_n - E_t) sw_n - Ds_n) sx_t + b_n, [T, N] f64 on `dev`.  The
    integer accumulator runs as an f64 GEMM: exact, since |Aq| 127 d < 2^53.  with_mag: also the sum of the magnitudes of the
    terms the kernel adds in f32, |acc - E| sw sx + |Ds| sx + |b| -- its rounding error is a few 2^-24 of that."""
    Aq = torch.from_numpy(rs["Aq"]).to(dev, torch.float64)
    assert float(Aq.abs().max()) * 127.0 * Aq.shape[1] < 2.0 ** 53
    E = torch.from_numpy(rs["E"]).to(dev, torch.float64)[:, None]
    sx = torch.from_numpy(rs["sx"].astype(np.float64)).to(dev)[:, None]
    N = rs["Wq"].shape[0]
    c = torch.empty(Aq.shape[0], N, dtype=torch.float64, device=dev)
    mag = torch.empty_like(c) if with_mag else None
    for n0 in range(0, N, chunk):
        n1 = min(N, n0 + chunk)
        wq = torch.from_numpy(rs["Wq"][n0:n1]).to(dev, torch.float64)
        sw = torch.from_numpy(rs["sw"][n0:n1]).to(dev)[None, :]
        ds = torch.from_numpy(rs["Ds"][n0:n1]).to(dev)[None, :]
        acc = Aq @ wq.T
        c[:, n0:n1] = ((acc - E) * sw - ds) * sx
        if with_mag:
            mag[:, n0:n1] = (acc - E).abs() * sw * sx + ds.abs() * sx
        if b_enc is not None:
            bb = b_enc[n0:n1].to(dev, torch.float64)[None, :]
            c[:, n0:n1] += bb
            if with_mag:
                mag[:, n0:n1] += bb.abs()
        del acc
    return (c, mag) if with_mag else c


def band_proxy(rs: dict, W: torch.Tensor, z: float, dev) -> torch.Tensor:
    """Lower bound of the subtractive pass's (z sigma)^2 of every pair, [T, N] f64: z^2 / 12 (sw_n^2 sum_c (|a_c| + sx / 2)^2
    + sx^2 |W_n|^2) -- the per-element variance of both roundings with the cross term inside (tests/test_gpu_band.py)."""
    a64 = torch.from_numpy(rs["a"]).to(dev, torch.float64)
    sx = torch.from_numpy(rs["sx"].astype(np.float64)).to(dev)
    xs = ((a64.abs() + 0.5 * sx[:, None]) ** 2).sum(dim=1)
    wn2 = (W.double() ** 2).sum(dim=1)
    sw = torch.from_numpy(rs["sw"]).to(dev)
    return z * z / 12.0 * (sw[None, :] ** 2 * xs[:, None] + sx[:, None] ** 2 * wn2[None, :])
