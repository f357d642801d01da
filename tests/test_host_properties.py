"""Property tests (hypothesis) of the host-side logic around the hot path: the canonical order key,
the merge of per-shard TopK lists, the k_loc truncation rule and the split-index rule of the cache
writer.  CPU only."""
from __future__ import annotations

import numpy as np
import torch
from hypothesis import given, settings, strategies as st

from oracle import oracle
from msae.parallel import canonical_key, merge_topk, token_slice
from msae.features.cache import FeatureCache

finite = st.floats(min_value=-1e6, max_value=1e6, allow_nan=False, allow_infinity=False, width=32)


@settings(max_examples=200, deadline=None)
@given(st.lists(finite, min_size=2, max_size=40), st.data())
def test_canonical_key_orders_by_value_then_index(vals, data):
    idx = data.draw(st.lists(st.integers(0, 2 ** 31 - 2), min_size=len(vals), max_size=len(vals), unique=True))
    v, i = torch.tensor(vals, dtype=torch.float32), torch.tensor(idx, dtype=torch.int64)
    key = canonical_key(v, i)
    order = torch.argsort(key, descending=True).tolist()
    for a, b in zip(order, order[1:]):
        va, vb = float(v[a]), float(v[b])
        assert va > vb or (va == vb and idx[a] < idx[b])       # -0.0 == +0.0 ties break by index


@settings(max_examples=100, deadline=None)
@given(st.integers(1, 6), st.integers(1, 8), st.integers(1, 5), st.integers(0, 2 ** 31 - 1))
def test_merge_of_shard_topk_equals_global_topk(G, k, T, seed):
    """global top-k (value desc, index asc) == merge of the per-shard top-k lists."""
    rng = np.random.default_rng(seed)
    n_loc = k + int(rng.integers(0, 5))
    # few distinct values: plenty of ties inside and across shards
    dense = rng.choice(np.array([0.0, 0.5, 1.0, 1.5, 2.0], dtype=np.float32), size=(T, G * n_loc))
    ref_v, ref_i = oracle.topk(dense, k)
    sv, si = [], []
    for g in range(G):
        v, i = oracle.topk(np.ascontiguousarray(dense[:, g * n_loc:(g + 1) * n_loc]), k)
        sv.append(torch.from_numpy(v)); si.append(torch.from_numpy(i.astype(np.int64)) + g * n_loc)
    mv, mi = merge_topk(torch.cat(sv, 1), torch.cat(si, 1), k)
    assert np.array_equal(mv.numpy(), ref_v) and np.array_equal(mi.numpy().astype(np.int32), ref_i)


@settings(max_examples=200, deadline=None)
@given(st.integers(1, 10 ** 6), st.integers(1, 64))
def test_token_slices_partition_the_batch(T, world):
    covered = 0
    for r in range(world):
        lo, hi, per = token_slice(T, r, world)
        assert lo == min(r * per, T) and lo <= hi <= T
        covered += hi - lo
    assert covered == T


@settings(max_examples=200, deadline=None)
@given(st.integers(2, 1 << 19), st.integers(1, 256))
def test_split_indices_follow_the_reference_rule(width, n_splits):
    """boundaries = linspace(0, width, n+1).long(); split i = (b[i], b[i+1] - 1)
    (sae_auto_interp/features/cache.py:243-247)."""
    fc = FeatureCache.__new__(FeatureCache)
    fc.width = width
    got = fc._generate_split_indices(n_splits)
    b = torch.linspace(0, width, steps=n_splits + 1).long()
    assert [(int(s), int(e)) for s, e in got] == list(zip(b[:-1].tolist(), (b[1:] - 1).tolist()))


def test_subtractive_dither_identities_and_residual_distribution():
    """The arithmetic behind the large-batch int8 pass's band (csrc/encode_defs.h "subtractive dither"),
    restated in numpy -- no GPU: (1) with shared dither vectors the subtracted product equals the integer accumulator minus a
    per-feature constant D_n, a per-token constant E_t, plus a scalar F -- exactly, in integers of 2^-34; (2) the residual of a
    subtractively dithered element is uniform on (-1/2, 1/2] WHATEVER the value is (here: values chosen adversarially at
    k + 1/2, where round to nearest is worst and stochastic rounding has its largest variance); (3) the error of a coarse value
    is exactly sum_c (A_c + delta_c) eps_c + delta_c W_c -- the cross term of the two roundings sits inside the first sum; (4) its
    standard deviation is that of the band's sigma (1/12 per rounding)."""
    import numpy as np

    rng = np.random.default_rng(7)
    d, T, N = 2048, 48, 64
    hx, hw = rng.integers(0, 1 << 16, d), rng.integers(0, 1 << 16, d)
    gx, gw = 2 * hx + 1 - (1 << 16), 2 * hw + 1 - (1 << 16)            # units of 2^-17: the dither minus one half
    rx, rw = (2 * hx + 1) / 131072.0, (2 * hw + 1) / 131072.0
    A = rng.normal(0, 30, (T, d))
    A[0] = np.floor(A[0]) + 0.5                                        # adversarial token: every element half way between two steps
    W = rng.normal(0, 30, (N, d))
    q = np.floor(A + rx).astype(np.int64)
    w = np.floor(W + rw).astype(np.int64)
    acc = q @ w.T
    D = (w @ gx)                                                       # [N], units 2^-17
    E = (q @ gw)                                                       # [T], units 2^-17
    F = int((gx * gw).sum())                                           # units 2^-34
    # (1) the identity, in exact integer arithmetic (everything scaled by 2^34)
    lhs = ((q * 131072 - gx).astype(object) @ (w * 131072 - gw).astype(object).T)
    rhs = acc.astype(object) * (1 << 34) - D.astype(object)[None, :] * (1 << 17) - E.astype(object)[:, None] * (1 << 17) + F
    assert (lhs == rhs).all()
    # (2) residuals: in (-1/2, 1/2], mean ~0, variance 1/12 -- also on the adversarial token
    delta = q - (rx - 0.5) - A
    eps = w - (rw - 0.5) - W
    for r in (delta, delta[0], eps):
        assert r.min() > -0.5 - 1e-9 and r.max() <= 0.5 + 1e-9
        assert abs(r.mean()) < 0.02 and abs(r.var() - 1.0 / 12.0) < 0.01
    # (3) the error decomposition, to float accuracy
    coarse = lhs.astype(np.float64) / float(1 << 34)
    exact = A @ W.T
    err = coarse - exact
    pred = (A + delta) @ eps.T + delta @ W.T
    assert np.allclose(err, pred, rtol=0, atol=1e-6 * np.abs(exact).max())
    # (4) its scale: sigma^2 = (|A + delta|^2 + |W|^2) / 12 per pair
    sig = np.sqrt((((A + delta) ** 2).sum(1)[:, None] + (W ** 2).sum(1)[None, :]) / 12.0)
    ratio = err / sig
    assert 0.9 < ratio.std() < 1.1 and np.abs(ratio).max() < 5.0
    # non-subtractive stochastic rounding of the SAME adversarial token: variance 1/4 per element, three times as much
    assert abs((q[0] - A[0]).var() - 0.25) < 0.01


def test_outlier_remainder_restatements():
    """The remainder plane of quant_x_kernel<SD>: an outlier dim's A = v / scale is split into m hi (the outlier tile) and
    lo = floor(A - m hi + r_x) in its own column.  Evaluated as (v * inv) - m hi in f32, A - m hi carries the rounding of
    v * inv at |A| up to 127 m: about 1e-3 step, and floor() picks the wrong integer for a few 1e-4 of the elements.  With ONE
    rounding, fmaf(-(m hi), scale, v) * inv, the error drops to ~1e-5 step and floor() agrees with the exact remainder except
    right next to an integer (tests/candidate_ref.py accepts either neighbour there)."""
    import numpy as np

    import candidate_ref as cr

    rng = np.random.default_rng(11)
    n = 1_000_000
    for lo, hi_, f32_flips in ((2, 127, (3e-5, 5e-4)), (128, 252, (1.5e-4, 8e-4))):
        m = rng.integers(lo, hi_ + 1, n)
        scale = (np.float32(2.0) ** rng.uniform(-12, 6, n)).astype(np.float32)
        v = (rng.uniform(-127, 127, n) * m * scale).astype(np.float32)
        inv_o = (np.float32(1.0) / (scale * m.astype(np.float32))).astype(np.float32)
        h = np.rint((v * inv_o).astype(np.float32))
        r = ((2 * rng.integers(0, 1 << 16, n) + 1) / 131072.0).astype(np.float32)
        exact = cr.remainder_exact(v, scale, m, h)
        assert np.abs(exact).max() <= m.max() / 2 + 1                # |lo| <= m / 2 + 1 <= 127: the column holds it
        q_ex, amb = cr.floor_exact(exact, r)
        assert 5e-5 < amb.mean() < 2e-4                             # 2 x 2^-14 of the elements sit in the undecidable band
        old = cr.remainder_f32(v, scale, m, h)
        q_old = np.floor((old + r).astype(np.float32)).astype(np.int64)
        assert np.abs(old - exact).max() > 5e-4, "the f32 evaluation's error this test exists for"
        assert f32_flips[0] < (q_old != q_ex).mean() < f32_flips[1]
        new = cr.remainder_fma(v, scale, m, h)
        q_new = np.floor((new + r).astype(np.float32)).astype(np.int64)
        assert np.abs(new - exact).max() < 3e-5
        assert not ((q_new != q_ex) & ~amb).any(), "one rounding: floor() agrees away from the boundary"
        assert (q_new != q_ex).mean() < 1e-5
    # the outlier set: 8 x the mean column max, the threshold raised by 1.5 until at most 128 dims qualify
    a = rng.normal(0, 1, (64, 4096)).astype(np.float32)
    a[3, :200] = np.float32(1e3) * (1 + np.arange(200, dtype=np.float32) / 100)
    out = cr.outlier_dims(a)
    assert out.sum() <= cr.MAX_OUT and out[:200].sum() == out.sum() and out[199]
