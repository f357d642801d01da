"""The error band of the large-batch int8 candidate pass, checked ELEMENT BY ELEMENT (round-5 verdict, items 1 and 2).

Round 6 made the pass's dither SUBTRACTIVE (csrc/encode_defs.h "subtractive dither"): both operands are rounded against
per-dim vectors shared by all tokens / all features, and the pass subtracts the dither again through a per-feature constant
D_n and a per-token integer E_t.  The residual of every operand element is then exactly uniform on (-1/2, 1/2] step,
whatever the data, and the band may use the uniform's own variance 1/12 where Hoeffding's worst case needed 1/4.

These tests restate the quantisation in numpy from the prepared buffer's own tables and check, pair by pair, against what
the kernels report through the feature-sharded engine's candidate records (upper value u and band z sigma of the best C
candidates of every token):
  * the coarse value c = u - z sigma IS  ((sum_c Aq_c Wq_c - E_t) sw_n - sw_n D_n) sx_t + b_n  -- i.e. D and E are the
    corrections the derivation says they are (a wrong sign would be a 1-sigma discrepancy on every pair);
  * (z sigma)^2 >= z^2 / 12 * sum_c [ sw^2 (|a_c| + sx / 2)^2 + sx^2 w_c^2 ]  -- the per-element variance proxy INCLUDING the
    cross term of the two roundings (the weights' residuals multiply the dequantised activation), and not more than 5 % above it;
  * the measured (p - c) / sigma over 50-130 k pairs has standard deviation ~1 and no outlier: 1/12 is the residuals' variance.
Reference semantics of the quantity being selected: /root/reference/sae_auto_interp/sae/sae.py:172-185.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import hostile
from candidate_ref import _emulate, _header, _records, _view

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("T,d", [(512, 512), (200, 1024)], ids=["mfma-tiles", "weight-stream"])
def test_subtractive_dither_band_is_the_elementwise_bound(dev, T, d):
    """(512 tokens: the 256 x 256-tile MFMA pass, csrc/gemm_mfma.h; 200 tokens at d % 1024 == 0: the weight-stream pass of
    17 ... 256 tokens, csrc/gemm_skinny.h -- both subtract the dither.)"""
    from msae import ops

    N, k, C, z = 8192, 32, 256, 7.0
    W, b, bd = hostile.weights("lognorm", N, d, dev, seed=41)
    x = hostile.activations(T, d, dev, seed=42)            # four x20 dims: the outlier tile and the remainder plane are in play
    ops.set_dither("on", seed=0xD17E5EED)
    try:
        prepared = ops.prepare_encoder(W)
        recs = ops.shard_candidates(x, b, bd, prepared, N, k, 0, C)
    finally:
        ops.set_dither("default")
    h = _header(prepared)
    assert h["dseed"] == 0xD17E5EED and h["N"] == N and h["d"] == d
    tab = _view(prepared, h["off_sdtab"], d * 4, np.int32).astype(np.int64) & 0xFFFFFFFF
    F = int(_view(prepared, h["off_sdtab"] + ((d + 1) & ~1) * 4, 8, np.int64)[0])
    Wq = _view(prepared, h["off_wq"], N * d, np.int8).reshape(N, d).astype(np.int64)
    wstat = _view(prepared, h["off_wstat"], N * 16, np.float32).reshape(N, 4)
    ds = _view(prepared, h["off_ds"], N * 4, np.float32)
    sw = wstat[:, 0].astype(np.float64)
    a, Aq, sx, m, E, gx, out = _emulate(x, bd, tab, F)     # (the outlier remainder restated exactly: candidate_ref.py)
    assert 1 <= out.sum() <= 4 and int(m.max()) <= 252 and int(m.max()) > 1

    # the weights' side of the tables: Wq = floor(W / sw + r_w) and Ds = sw D
    Wn = W.cpu().numpy()
    hw = tab & 0xFFFF
    rw = ((2 * hw + 1).astype(np.float32) * np.float32(1.0 / 131072.0))
    sw32 = wstat[:, 0]
    inv_w = (np.float32(1.0) / sw32).astype(np.float32)
    Wq_em = np.clip(np.floor(((Wn * inv_w[:, None]).astype(np.float32) + rw[None, :]).astype(np.float32)), -127, 127).astype(np.int64)
    assert np.array_equal(Wq_em, Wq), "row_stats_quant_row: shared dither r_w(c)"
    D = (Wq @ gx).astype(np.float64) / 131072.0
    assert np.allclose(ds, sw * D, rtol=2e-6, atol=1e-7)

    ok, u, feat, zs = _records(recs, C)
    assert ok.mean() > 0.95
    tt, jj = np.nonzero(ok)
    ff = feat[tt, jj]
    acc = np.einsum("ij,ij->i", Aq[tt], Wq[ff])
    bias = b.cpu().numpy().astype(np.float64)
    c_em = ((acc - E[tt]) * sw[ff] - ds[ff].astype(np.float64)) * sx[tt].astype(np.float64) + bias[ff]
    c_gpu = u[tt, jj].astype(np.float64) - zs[tt, jj].astype(np.float64)
    err = np.abs(c_gpu - c_em) / np.maximum(1.0, np.abs(c_em))
    assert err.max() < 2e-5, f"coarse value != its definition: {err.max():.3g}"

    # the band against the per-element variance proxy (cross term inside)
    a64, W64 = a.astype(np.float64), Wn.astype(np.float64)
    xs = ((np.abs(a64) + 0.5 * sx[:, None].astype(np.float64)) ** 2).sum(axis=1)          # sum_c (|a_c| + sx / 2)^2
    wn2 = (W64 ** 2).sum(axis=1)
    proxy = z * z / 12.0 * (sw[ff] ** 2 * xs[tt] + sx[tt].astype(np.float64) ** 2 * wn2[ff])
    band2 = zs[tt, jj].astype(np.float64) ** 2
    assert (band2 >= proxy * (1 - 1e-5)).all(), float((band2 / proxy).min())
    assert (band2 <= proxy * 1.05).all(), float((band2 / proxy).max())

    # the residuals themselves: uniform, variance 1/12 -- (p - c) / sigma has unit variance and Gaussian-like tails
    p = np.einsum("ij,ij->i", a64[tt], W64[ff]) + bias[ff]
    ratio = (p - c_em) / (np.sqrt(proxy) / z)
    print(f"\nsubtractive dither: {ratio.size} pairs, (p - c) / sigma: mean {ratio.mean():+.4f}, std {ratio.std():.4f}, "
          f"max |.| {np.abs(ratio).max():.2f}; band / proxy {float((band2 / proxy).min()):.4f} .. {float((band2 / proxy).max()):.4f}")
    assert 0.9 < ratio.std() < 1.04 and abs(ratio.mean()) < 0.05 and np.abs(ratio).max() < 6.0


@pytest.mark.parametrize("T,d", [(512, 512), (200, 1024)], ids=["mfma-tiles", "weight-stream"])
def test_token_with_a_huge_outlier_multiplier_keeps_the_coarse_outlier_steps(dev, T, d):
    """A token whose massive dims exceed its ordinary ones by more than SD_M_EXACT = 252 has no remainder plane (it would not
    fit int8): its outlier dims keep coarse steps and their own band term (M_t = sqrt(3) m).  Its coarse values still lie inside
    their band, and the encode is exact on it and on its neighbours."""
    from msae import ops

    N, k, C = 8192, 32, 256
    W, b, bd = hostile.weights("gauss", N, d, dev, seed=43)
    x = hostile.activations(T, d, dev, seed=44).float()
    big = [7, 150]
    for t in big:                                           # ~400x its ordinary dims' maximum, on two of the batch's outlier dims
        x[t, 13] = 2000.0 * x[t].abs().median()
        x[t, (977 + 13) % d] = -1900.0 * x[t].abs().median()
    x = x.to(torch.bfloat16)
    prepared = ops.prepare_encoder(W)
    recs = ops.shard_candidates(x, b, bd, prepared, N, k, 0, C)
    ok, u, feat, zs = _records(recs, C)
    a64 = (x.float().cpu() - bd.cpu()).numpy().astype(np.float64)
    W64, bias = W.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    for t in big:
        sel = ok[t]
        assert sel.sum() > k
        p = a64[t] @ W64[feat[t, sel]].T + bias[feat[t, sel]]
        c = u[t, sel].astype(np.float64) - zs[t, sel]
        assert (np.abs(p - c) <= zs[t, sel] * 1.0001).all()
    v, i, st = ops.encode_topk(x, W, b, bd, prepared, k, coarse_mode=1)
    ve, ie, _ = ops.encode_topk(x, W, b, bd, prepared, k, exact=True)
    assert torch.equal(i, ie) and torch.equal(v, ve)
    assert int(st[big[0]]) == 0 and int(st[big[1]]) == 0, "verified by the fast path, not recomputed"
