"""GPU parity of the training forward's AuxK / Multi-TopK branch at production width (C2: d = 4096, N = 131072).

When `Sae.forward` gets a `dead_mask`, or Multi-TopK asks for more than 256 latents, `ops._SparseEncode` leaves the fused
encoder: dense pre_acts, then `msae_topk_f32` three times -- top-k, the AuxK top-k_aux of the dead latents (k_aux =
min(d // 2, num_dead) = 2048 at C2, up to 16384 by design) and top-4k -- and the backward sends one [T, k + k_aux + 4k]
pair matrix (2208 wide at C2) through the weight-gradient kernel.  This module checks that branch kernel by kernel at
those widths and end to end against dense torch restatements of the reference (sae.py:193-247, trainer.py:347-408):

  1. msae_topk_f32 over its whole k range (the > 64 KiB LDS launch, non-power-of-two k, thousands of rows, rows of
     -inf, ties at 0, signed zeros) against a float64 canonical top-k and the C oracle;
  2. decode / decode_bwd at AuxK widths (k = 2048 .. 4096, the 2208-wide pair matrix with features every token picks);
  3. Sae.forward with AuxK and Multi-TopK: losses and gradients;
  4. one SaeTrainStep.step with auxk_alpha = 1/32: parameters and the fired bookkeeping.

Every test frees its dense [T, N] buffers (_free_after): the module stays within the peak of the other C2 tests.
"""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hostile
from oracle import oracle

pytestmark = pytest.mark.gpu

D, N_C2 = 4096, 131072
U = 2.0 ** -24                                     # unit roundoff of f32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_after():
    yield
    from msae import ops

    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. msae_topk_f32 over k in (2048, 16384] ------------------------------------------------------------------------
def _canonical_topk(lat, k, rows=256):
    """Canonical top-k in float64, independent of the kernel and of the oracle's heap: a stable sort of -value keeps equal
    values in ascending index order (lexsort by (-value, index)).  -0.0 is mapped to +0.0 first so the two rank as equal;
    the values returned are the stored ones (gathered from `lat`)."""
    T = lat.shape[0]
    vals = torch.empty(T, k, dtype=lat.dtype, device=lat.device)
    idx = torch.empty(T, k, dtype=torch.int64, device=lat.device)
    for r0 in range(0, T, rows):
        blk = lat[r0:r0 + rows]
        key = blk.double()
        key = torch.where(key == 0, torch.zeros_like(key), key)
        order = torch.sort(-key, dim=-1, stable=True).indices[:, :k]
        idx[r0:r0 + rows] = order
        vals[r0:r0 + rows] = blk.gather(1, order)
        del key, order
    return vals, idx


ROW_KINDS = ["auxk_mask", "dead_exactly_k", "ties", "signed_zeros", "digit1", "digit2", "digit3", "digit3_negative"]


def _hostile_rows(out, k, dev, seed):
    """Fills out [T, N] with one row kind per row (row t: ROW_KINDS[t % 8]), each aimed at a way the radix select / collect
    / bitonic sort of topk_rows_kernel can go wrong at large k."""
    T, N = out.shape
    g = torch.Generator(device=dev).manual_seed(seed)
    nk = len(ROW_KINDS)
    for kind, name in enumerate(ROW_KINDS):
        R = len(range(kind, T, nk))
        if R == 0:
            continue
        if name == "auxk_mask":
            # torch.where(dead_mask, pre, -inf) with more dead latents than k (sae.py:217-220): -inf outside a dead set of
            # ~1.5 k; about half of the dead latents are post-ReLU zeros, so the pivot is 0 and the r lowest-index zeros win
            dead = torch.rand(R, N, generator=g, device=dev) < min(1.0, 1.5 * k / N)
            v = torch.relu(torch.randn(R, N, generator=g, device=dev))
            rows = torch.where(dead, v, torch.full_like(v, -torch.inf))
        elif name == "dead_exactly_k":
            # a dead set of exactly k latents (num_dead == k_aux), a quarter of them 0: every finite entry is selected
            pos = torch.rand(R, N, generator=g, device=dev).topk(k, dim=1).indices
            v = torch.randn(R, k, generator=g, device=dev).abs()
            v[torch.rand(R, k, generator=g, device=dev) < 0.25] = 0.0
            rows = torch.full((R, N), -torch.inf, device=dev).scatter_(1, pos, v)
        elif name == "ties":
            # ~25 distinct values: thousands of copies of the pivot value straddle position k
            rows = torch.round(torch.randn(R, N, generator=g, device=dev) * 4) / 4
        elif name == "signed_zeros":
            # fewer than k positives, the rest +0.0 / -0.0 at random (and a few negatives): the zeros that fill the top-k
            # rank as equal whatever their sign and come back in ascending index with their stored bits
            u = torch.rand(R, N, generator=g, device=dev)
            mag = torch.randn(R, N, generator=g, device=dev).abs() + 1e-3
            zero = torch.where(torch.rand(R, N, generator=g, device=dev) < 0.5, 0.0, -0.0)
            p_pos = 0.6 * k / N
            rows = torch.where(u < p_pos, mag, torch.where(u > 1.0 - 0.05 * (1.0 - p_pos), -mag, zero))
        elif name == "digit1":
            # values over many binades: the pivot is told apart in the top 12 key bits
            rows = torch.randn(R, N, generator=g, device=dev) * torch.exp(2.0 * torch.randn(R, N, generator=g, device=dev))
        elif name == "digit2":
            # one binade, 2^20 patterns: all keys share bits 31..20, the pivot is decided by bits 19..8
            b = torch.randint(0, 1 << 20, (R, N), generator=g, device=dev, dtype=torch.int32) + 0x3F800000
            rows = b.view(torch.float32)
        elif name == "digit3":
            # 256 patterns: keys share bits 31..8, the pivot is decided by the last 8 bits (N / 256 copies of each value)
            b = torch.randint(0, 256, (R, N), generator=g, device=dev, dtype=torch.int32) + 0x3F800000
            rows = b.view(torch.float32)
        else:  # digit3_negative: the same below zero (order key = ~bits)
            b = torch.randint(0, 256, (R, N), generator=g, device=dev, dtype=torch.int32) + 0x3F800000
            rows = -b.view(torch.float32)
        out[kind::nk] = rows
        del rows
    return out


def _check_topk(lat, k, what, oracle_rows=8):
    from msae import ops

    v, i = ops.topk(lat, k)
    assert v.shape == (lat.shape[0], k) and i.dtype == torch.int64
    rv, ri = _canonical_topk(lat, k)
    bad = (i != ri).any(dim=1)
    assert not bad.any(), (what, "indices differ on rows", torch.nonzero(bad).flatten()[:8].tolist(),
                           [ROW_KINDS[int(t) % len(ROW_KINDS)] for t in torch.nonzero(bad).flatten()[:8]])
    assert torch.equal(_bits(v), _bits(rv)), (what, "values differ (bits)")
    # the C oracle (a heap) on the first rows: one of every kind
    n = min(oracle_rows, lat.shape[0])
    lat_np = lat[:n].contiguous().cpu().numpy()
    ov, oi = oracle.topk(lat_np, k)
    assert np.array_equal(i[:n].cpu().numpy().astype(np.int32), oi), (what, "indices differ from the oracle")
    assert np.array_equal(v[:n].cpu().numpy(), ov), (what, "values differ from the oracle")
    return v, i


@pytest.mark.parametrize("T,N,k", [(256, N_C2, 2049), (256, N_C2, 4096), (128, N_C2, 8191), (128, N_C2, 16384),
                                   (8192, N_C2, 2048), (16, 16384, 16384)],
                         ids=["k2049", "k4096", "k8191", "k16384", "T8192_k2048", "full_sort_N16384"])
def test_topk_large_k_bit_exact_vs_float64_canonical(dev, T, N, k):
    """The AuxK shape: one workgroup per row, grid = T, k up to the 16384 DESIGN.md promises (~144 KiB of dynamic LDS,
    hipFuncSetAttribute), non-power-of-two k (the next_pow2 padding keys must sort last), k = N (a full sort)."""
    lat = torch.empty(T, N, device=dev)
    _hostile_rows(lat, k, dev, seed=k + T)
    _check_topk(lat, k, f"T={T} N={N} k={k}")
    del lat


@pytest.mark.parametrize("N,k,offset", [(131071, 8191, 0), (N_C2, 16384, 1), (16383, 16383, 0)],
                         ids=["N_odd_k8191", "misaligned_k16384", "N_odd_full_sort"])
def test_topk_scalar_kernel_at_large_k(dev, N, k, offset):
    """topk_rows_kernel<false> (element loads): rows of N % 4 != 0, or a row view 4 bytes off a 16-byte boundary."""
    T = 64
    buf = torch.empty(T * N + offset, device=dev)
    lat = buf[offset:].view(T, N)
    assert (lat.data_ptr() % 16 != 0) == (offset != 0)
    _hostile_rows(lat, k, dev, seed=7 * k + offset)
    _check_topk(lat, k, f"N={N} k={k} offset={offset}")
    del buf, lat


# ---- 2. decode and its backward at AuxK widths -----------------------------------------------------------------------
def _decoder(dev, seed):
    """W_dec [N_C2, D] with rows of norm ~1, b_dec [D]."""
    g = torch.Generator(device=dev).manual_seed(seed)
    W = torch.randn(N_C2, D, generator=g, device=dev) * (1.0 / 64)
    return W, torch.randn(D, generator=g, device=dev) * 0.1


@pytest.mark.parametrize("A,k", [(64, 2048), (32, 4096), (48, 2047)], ids=["k2048", "k4096", "k2047_tail"])
def test_decode_at_auxk_widths_bit_exact_vs_oracle(dev, A, k):
    """msae_decode_f32 / msae_decode_i64_f32 at (A, k = 2048 / 4096 / 2047 (a tail after the unroll of 8), N = 131072,
    d = 4096) against oracle.decode: one f32 fma chain per output in selection order, bit for bit.  Half the activations are
    post-ReLU zeros, which contribute nothing (kernels.py:277): a decoder row of NaN picked only with activation 0 must
    leave no trace."""
    from msae import ops

    W, b = _decoder(dev, seed=300 + k)
    g = torch.Generator(device=dev).manual_seed(301 + k)
    idx = torch.rand(A, N_C2, generator=g, device=dev).topk(k, dim=1).indices     # distinct per row, any order
    idx[0, 0], idx[-1, -1] = 0, N_C2 - 1                                           # both ends of the table
    acts = torch.relu(torch.randn(A, k, generator=g, device=dev))
    poison = 12345
    W[poison] = float("nan")
    acts[idx == poison] = 0.0
    idx[:, k // 2] = poison                                                        # every token, activation 0
    acts[:, k // 2] = 0.0
    assert float((acts == 0).float().mean()) > 0.4
    out64 = ops.decode(idx, acts, W, b)
    out32 = ops.decode(idx.to(torch.int32), acts, W, b)
    rows = W[idx.reshape(-1)].cpu().numpy()                 # the oracle needs only the gathered rows
    ref = oracle.decode(np.arange(A * k, dtype=np.int32).reshape(A, k), acts.cpu().numpy(), rows, b.cpu().numpy())
    del rows
    assert np.isfinite(ref).all()
    for name, out in (("int64 indices", out64), ("int32 indices", out32)):
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
            (name, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
    del W


def test_decode_bwd_acts_at_k2048_vs_float64(dev):
    """msae_decode_bwd_acts_f32 at (A = 64, k = 2048, N = 131072, d = 4096): g_acts[a, j] = <grad_out[a], W_dec[idx[a, j]]>
    against float64.  The kernel is a 64-term fma chain per lane (d / 64 products) and a 6-level reduction across the wave,
    so each result is within gamma_70 sum_c |g_c w_c| of the exact dot (gamma_n ~ n u, the classic bound of a summation
    of depth n); bar: 72 u sum |g w|."""
    from msae import ops

    A, k = 64, 2048
    W, _ = _decoder(dev, seed=310)
    g = torch.Generator(device=dev).manual_seed(311)
    idx = torch.randint(0, N_C2, (A, k), generator=g, device=dev)
    idx[:, 0] = 0
    idx[:, -1] = N_C2 - 1
    gout = torch.randn(A, D, generator=g, device=dev) * torch.exp(torch.randn(A, 1, generator=g, device=dev))
    ga, _ = ops.decode_bwd(idx, torch.rand(A, k, generator=g, device=dev), W, gout, True, False)
    for a0 in range(0, A, 8):                               # 8 tokens x 2048 rows of float64 at a time
        rows = W[idx[a0:a0 + 8]].double()                  # [8, k, D]
        gd = gout[a0:a0 + 8, None, :].double()
        ref = (rows * gd).sum(-1)
        bound = 72 * U * (rows.abs() * gd.abs()).sum(-1)
        err = (ga[a0:a0 + 8].double() - ref).abs()
        assert bool((err <= bound).all()), (a0, float(err.max()), float((err / bound).max()))
        del rows, gd, ref, bound, err
    del W


def test_decode_bwd_wdec_with_the_auxk_pair_matrix_vs_float64_index_add(dev):
    """msae_decode_bwd_wdec_f32 with the pair matrix of a C2 Multi-TopK + AuxK step: [A = 4096, 32 + 2048 + 128 = 2208],
    N = 131072, d = 4096.  300 "dead" features sit in every token's AuxK block (num_dead <= d / 2: every dead latent is in
    every token's selection), so their rows have L = A pairs (the in-place global sort); the rest of the AuxK block makes
    ~58 pairs per feature on average (the register and LDS sorts); the Multi-TopK block repeats the top-k (the same
    (token, feature) pair twice in one row).  Against a chunked float64 index_add_ with the error model of
    test_decode_bwd_wdec_at_c2_vs_float64_index_add; two calls give the same bits; collect_wgrad_sumsq's row norms and the
    row_act_sum output (the encoder-bias gradient of _SparseEncode.backward) against float64."""
    from msae import ops

    A, kt, ka, km = 4096, 32, 2048, 128
    k = kt + ka + km
    n_dead = 300
    g = torch.Generator(device=dev).manual_seed(320)
    dead = torch.randperm(N_C2 - 16, generator=g, device=dev)[:n_dead] + 16
    top = torch.randint(0, N_C2, (A, kt), generator=g, device=dev)
    aux_dead = dead[torch.rand(A, n_dead, generator=g, device=dev).argsort(dim=1)]     # every token, in its own order
    aux_rest = torch.randint(0, N_C2, (A, ka - n_dead), generator=g, device=dev)
    multi = torch.cat([top, torch.randint(0, N_C2, (A, km - kt), generator=g, device=dev)], 1)
    idx = torch.cat([top, aux_dead, aux_rest, multi], 1).contiguous()
    idx[idx == 5] = 6                                        # feature 5: no pair at all
    assert idx.shape == (A, k)
    acts = torch.rand(A, k, generator=g, device=dev) + 0.05
    acts[::9, kt + n_dead + 3] = 0.0                         # pairs that carry nothing (relu' = 0)
    acts[:, kt + ka + 5] = 0.0
    gout = torch.randn(A, D, generator=g, device=dev)
    W = torch.empty(N_C2, D, device=dev)                     # only its shape is read
    wkey = W.data_ptr()
    prev = ops._WGRAD_ROWSUM
    try:
        ops._WGRAD_ROWSUM = []
        with ops.collect_wgrad_sumsq() as coll:
            _, gw = ops.decode_bwd(idx, acts, W, gout, False, True)
        rowsum = ops._WGRAD_ROWSUM[0]
        ops._WGRAD_ROWSUM = []
        _, gw2 = ops.decode_bwd(idx, acts, W, gout, False, True)
        rowsum2 = ops._WGRAD_ROWSUM[0]
    finally:
        ops._WGRAD_ROWSUM = prev
    assert torch.equal(gw, gw2) and torch.equal(rowsum, rowsum2), "weight gradient is not bit-reproducible"
    del gw2, rowsum2, W
    calls, ptr, rowsq = coll[wkey]
    assert calls == 1 and ptr == gw.data_ptr()

    flat_i = idx.reshape(-1)
    live = acts.reshape(-1) != 0
    L = torch.bincount(flat_i[live], minlength=N_C2)
    assert int(L[dead].min()) >= A, "the dead features must have a live pair in every token"
    assert int(((L > 64) & (L <= 1024)).sum()) > 1000 and int((L <= 64).sum()) > 1000   # all three sort paths
    ref = torch.zeros(N_C2, D, dtype=torch.float64, device=dev)
    mag = torch.zeros(N_C2, dtype=torch.float64, device=dev)   # sum |act| per row: scale of the rounding bound
    step = max(1, (1 << 27) // (k * D))                        # ~1 GiB of float64 products per chunk
    for a0 in range(0, A, step):
        sl = slice(a0, min(A, a0 + step))
        src = acts[sl].reshape(-1, 1).double() * gout[sl].double().repeat_interleave(k, 0)
        ref.index_add_(0, idx[sl].reshape(-1), src)
        mag.index_add_(0, idx[sl].reshape(-1), acts[sl].reshape(-1).double())
        del src
    Lc = torch.clamp(L.double(), min=1.0)
    worst = 0.0
    for r0 in range(0, N_C2, 16384):
        sl = slice(r0, r0 + 16384)
        err = (gw[sl].double() - ref[sl]).abs().amax(dim=1)
        # an f32 chain of L terms a_i g_i: |error| <~ sqrt(L) eps sum|a_i g_i| (worst case L eps ...); |g| < 6 here
        tol = 2e-7 * mag[sl] * 6.0 * Lc[sl].sqrt() + 1e-12
        worst = max(worst, float((err / tol).max()))
    assert worst <= 1.0, worst
    # per-row squared norms, from the rows the kernel had in registers
    assert torch.allclose(rowsq.double(), (gw.double() ** 2).sum(1), rtol=1e-5, atol=1e-12)
    del ref
    # row_act_sum: lane-strided chains of ceil(L / 64) terms, then a 6-level tree: gamma_{ceil(L/64)+6} sum |a|
    ref_s = torch.zeros(N_C2, dtype=torch.float64, device=dev).index_add_(0, flat_i, acts.reshape(-1).double())
    bound = (torch.ceil(L.double() / 64) + 7) * U * mag
    assert bool(((rowsum.double() - ref_s).abs() <= bound).all()), float((rowsum.double() - ref_s).abs().max())
    assert float(rowsum[L == 0].abs().max()) == 0.0
    del gw


# ---- 3. Sae.forward with AuxK and Multi-TopK at C2 width -------------------------------------------------------------
class _Spy:
    """Records what Sae.forward asked of ops.sparse_encode (k, k_aux, k_multi) and the selections it got back, and which
    encoder branch ran (fused encode_topk or dense pre_acts + topk)."""

    def __init__(self, monkeypatch):
        from msae import ops

        self.calls, self.branches = [], []
        real_se, real_enc, real_pre = ops.sparse_encode, ops.encode_topk, ops.pre_acts

        def sparse_encode(x, W_enc, b_enc, b_dec, k, dead_mask=None, k_aux=0, k_multi=0, **kw):
            out = real_se(x, W_enc, b_enc, b_dec, k, dead_mask, k_aux, k_multi, **kw)
            self.calls.append({"k": k, "k_aux": k_aux, "k_multi": k_multi,
                               "sel": [(a.detach(), i.detach()) for a, i in out]})
            return out

        def encode_topk(*a, **kw):
            self.branches.append("fused")
            return real_enc(*a, **kw)

        def pre_acts(*a, **kw):
            self.branches.append("dense")
            return real_pre(*a, **kw)

        monkeypatch.setattr(ops, "sparse_encode", sparse_encode)
        monkeypatch.setattr(ops, "encode_topk", encode_topk)
        monkeypatch.setattr(ops, "pre_acts", pre_acts)


def _c2_sae(dev, k, seed, T):
    """Sae(d = 4096, N = 131072, k, multi_topk) with trained-like encoder rows, the tied decoder of the reference's
    initialisation (unit rows), and T residual-stream-like tokens in f32."""
    from msae import Sae, SaeConfig

    W, b, bd = hostile.weights("trained_like", N_C2, D, dev, seed=seed)
    sae = Sae(D, SaeConfig(num_latents=N_C2, k=k, multi_topk=True), device=dev)
    with torch.no_grad():
        sae.encoder.weight.copy_(W)
        sae.encoder.bias.copy_(b)
        sae.b_dec.copy_(bd)
        sae.W_dec.copy_(W)
    del W, b, bd
    sae.set_decoder_norm_to_unit_norm()
    x = hostile.activations(T, D, dev, seed=seed).float()
    return sae, x


def _dead_mask(n_dead, dev, seed):
    if n_dead is None:
        return None
    m = torch.zeros(N_C2, dtype=torch.bool, device=dev)
    m[torch.randperm(N_C2, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)[:n_dead]] = True
    return m


def _assert_topk_of(lat, scale, vals, idx, m, what):
    """(vals, idx) [T, m] is a top-m of the dense latents `lat` [T, N] up to the summation order of the GEMM: the selected
    latents equal the dense ones within tol = 2e-5 |row max| (`scale`), and no latent is larger than the smallest selected
    one by more than tol unless it is selected.  (Ties at 0 carry no value and no gradient: any tie choice gives the same
    loss.)"""
    assert idx.shape == (lat.shape[0], m), (what, tuple(idx.shape), m)
    s = torch.sort(idx, dim=1).values
    assert not bool((s[:, 1:] == s[:, :-1]).any()), (what, "an index is selected twice")
    tol = (2e-5 * scale)[:, None]
    got = lat.gather(1, idx)
    assert bool(((got - vals).abs() <= tol).all()), (what, float((got - vals).abs().max()))
    kth = got.min(dim=1, keepdim=True).values
    above = (lat > kth + tol).sum(1)
    assert int(above.max()) <= m - 1, (what, "not a top-k of the dense latents", int(above.max()), m)


def _restate_forward(params, x, sel, k, dead_mask, k_aux, scale, multi):
    """Reference Sae.forward (sae.py:193-247) in dense torch on the HIP side's selections `sel` ([(acts, idx)] in
    sparse_encode's order): relu(F.linear), where(dead_mask, pre, -inf), decode by gather (embedding_bag, the selected
    latents as per-sample weights), and e, the total variance, fvu, auxk_loss, multi_topk_fvu in float64.  -> (leaves,
    [fvu, auxk_loss, multi_topk_fvu]) with the losses differentiable w.r.t. the leaves (We, be, Wd, bd, x)."""
    We, be, Wd, bd = (torch.nn.Parameter(p.detach().clone()) for p in params)
    xr = x.detach().clone().requires_grad_(x.requires_grad)
    pre = torch.relu(F.linear(xr - bd, We, be))                                  # [T, N] f32, dense
    with torch.no_grad():
        row_scale = pre.abs().amax(dim=1)
    xd = xr.double()
    total_variance = (xd - xd.mean(0)).pow(2).sum()

    def decode(lat, idx):
        return F.embedding_bag(idx, Wd, per_sample_weights=lat.gather(1, idx), mode="sum") + bd

    (a0, i0) = sel[0]
    with torch.no_grad():
        _assert_topk_of(pre, row_scale, a0, i0, k, "top-k")
    e = decode(pre, i0).double() - xd
    fvu = e.pow(2).sum() / total_variance
    j = 1
    if k_aux > 0:
        a1, i1 = sel[j]
        j += 1
        dead_pre = torch.where(dead_mask[None], pre, -torch.inf)                  # sae.py:217-220
        with torch.no_grad():
            assert bool(dead_mask[i1].all()), "AuxK picked a live latent"
            _assert_topk_of(dead_pre, row_scale, a1, i1, k_aux, "AuxK top-k_aux")
        e_hat = decode(dead_pre, i1).double()
        auxk_loss = scale * (e_hat - e).pow(2).sum() / total_variance
        del dead_pre
    else:
        auxk_loss = torch.zeros((), dtype=torch.float64, device=x.device)
    if multi:
        a2, i2 = sel[j]
        j += 1
        with torch.no_grad():
            _assert_topk_of(pre, row_scale, a2, i2, 4 * k, "Multi-TopK top-4k")
        multi_fvu = (decode(pre, i2).double() - xd).pow(2).sum() / total_variance
    else:
        multi_fvu = torch.zeros((), dtype=torch.float64, device=x.device)
    assert j == len(sel), (j, len(sel))
    return (We, be, Wd, bd, xr), [fvu, auxk_loss, multi_fvu]


def _expected_aux(n_dead, d):
    """k_aux and scale of sae.py:207-213, stated independently of msae."""
    if not n_dead:
        return 0, 0.0
    return min(d // 2, n_dead), min(n_dead / (d // 2), 1.0)


FORWARD_CASES = {
    # name: (k, num_dead or None = no dead_mask, x.requires_grad)
    "dead_over_half": (32, 5000, False),        # k_aux = 2048, scale = 1
    "dead_over_half_x_grad": (32, 5000, True),  # ... the non-lean path (plain expressions), with x.grad
    "dead_under_half": (32, 300, False),        # k_aux = num_dead = 300: every dead latent in every token's selection
    "dead_one": (32, 1, False),                 # k_aux = 1, scale = 1 / 2048
    "dead_none": (32, 0, False),                # an all-False mask: no AuxK term, the fused encoder
    "multi_k64": (64, None, False),             # 4k = 256: the fused encoder's largest selection
    "multi_k65": (65, None, False),             # 4k = 260: the dense branch
    "multi_k65_x_grad": (65, None, True),
}


@pytest.mark.parametrize("case", list(FORWARD_CASES))
def test_training_forward_auxk_and_multi_topk_at_c2_vs_dense_restatement(dev, monkeypatch, case):
    """Sae.forward(x, dead_mask) at d = 4096, N = 131072, T = 2048, multi_topk: the three loss terms, and after backward of
    fvu + auxk_loss / 32 + multi_topk_fvu / 8 (trainer.py:379-384) the gradients of W_enc, b_enc, W_dec, b_dec (and x), against
    the dense float64-loss restatement on the HIP side's selections, each of which is first checked to be a valid top-k
    of the dense latents of its width."""
    k, n_dead, x_grad = FORWARD_CASES[case]
    T = 2048
    sae, x = _c2_sae(dev, k, seed=400 + k, T=T)
    dead_mask = _dead_mask(n_dead, dev, seed=401)
    k_aux, scale = _expected_aux(n_dead, D)
    spy = _Spy(monkeypatch)
    x = x.requires_grad_(x_grad)
    params = (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)

    out = sae(x, dead_mask)
    loss = out.fvu + out.auxk_loss / 32 + out.multi_topk_fvu / 8
    loss.backward()
    got_losses = [float(t.detach()) for t in (out.fvu, out.auxk_loss, out.multi_topk_fvu)]
    grads = [p.grad for p in params] + ([x.grad] if x_grad else [])
    assert len(spy.calls) == 1
    call = spy.calls[0]
    assert (call["k"], call["k_aux"], call["k_multi"]) == (k, k_aux, 4 * k), call
    expect_branch = "fused" if k_aux == 0 and 4 * k <= 256 else "dense"
    assert spy.branches == [expect_branch], (spy.branches, expect_branch)
    sel = call["sel"]
    assert torch.equal(out.latent_indices, sel[-1][1])        # the reference returns the Multi-TopK selection
    if k_aux == 0:
        assert float(out.auxk_loss) == 0.0
    for p in params:
        p.grad = None
    del out, loss

    leaves, losses = _restate_forward(params, x, sel, k, dead_mask, k_aux, scale, multi=True)
    for name, got, ref in zip(("fvu", "auxk_loss", "multi_topk_fvu"), got_losses, losses):
        ref = float(ref.detach())
        assert abs(got - ref) <= 2e-5 * abs(ref), (name, got, ref)
    if k_aux > 0:
        assert losses[1].item() > 0.0
    (losses[0] + losses[1] / 32 + losses[2] / 8).backward()
    del losses
    names = ("W_enc", "b_enc", "W_dec", "b_dec", "x")
    for name, got, leaf in zip(names, grads, leaves):
        ref = leaf.grad
        err = (got - ref).abs().max().item()
        assert err <= 2e-4 * ref.abs().max().item() + 1e-9, (name, err, ref.abs().max().item())
    del sae, leaves, grads, sel, spy


# ---- 4. one optimisation step with AuxK at C2 ------------------------------------------------------------------------
def test_train_step_with_auxk_at_c2_matches_dense_restatement(dev, monkeypatch):
    """SaeTrainStep.step with auxk_alpha = 1/32 and 1500 dead features (num_tokens_since_fired > threshold), multi_topk, at
    d = 4096, N = 131072, T = 2048, against the reference trainer's step order (trainer.py:347-401) restated densely:
    forward on the HIP selections, backward of fvu + auxk_loss / 32 + multi_topk_fvu / 8, clip_grad_norm_(1.0), the
    decoder-parallel projection, torch.optim.Adam.  Then the fired bookkeeping (trainer.py:387, 404-408): exactly the
    features of out.latent_indices -- the Multi-TopK selection -- are reset to 0; a feature only the AuxK selection picked
    has not fired."""
    from msae.train import SaeTrainStep

    T, k, n_dead = 2048, 32, 1500
    lr = 2e-4 / (N_C2 / 2 ** 14) ** 0.5
    sae, x = _c2_sae(dev, k, seed=500, T=T)
    dead_mask = _dead_mask(n_dead, dev, seed=501)
    k_aux, scale = _expected_aux(n_dead, D)
    params = (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)
    params0 = [p.detach().clone() for p in params]
    ts = SaeTrainStep(sae, lr=lr, auxk_alpha=1.0 / 32, dead_feature_threshold=0)
    ts.num_tokens_since_fired[dead_mask] = 1
    spy = _Spy(monkeypatch)
    stats = ts.step(x)
    assert len(spy.calls) == 1 and spy.calls[0]["k_aux"] == k_aux == n_dead
    sel = spy.calls[0]["sel"]

    leaves, losses = _restate_forward(params0, x, sel, k, dead_mask, k_aux, scale, multi=True)
    We, be, Wd, bd, _ = leaves
    for name, ref in (("fvu", losses[0]), ("auxk_loss", losses[1]), ("multi_topk_fvu", losses[2])):
        ref = float(ref.detach())
        assert abs(float(stats[name]) - ref) <= 1e-4 * ref, (name, float(stats[name]), ref)
    (losses[0] + losses[1] / 32 + losses[2] / 8).backward()
    del losses
    torch.nn.utils.clip_grad_norm_([We, be, Wd, bd], 1.0)
    with torch.no_grad():
        Wd.grad -= (Wd.grad * Wd.data).sum(dim=1, keepdim=True) * Wd.data
    torch.optim.Adam([We, be, Wd, bd], lr=lr).step()
    if ts.fuse_next_step:
        # the Adam pass has already applied the NEXT step's set_decoder_norm_to_unit_norm (trainer.py:352, sae.py:249-255)
        assert ts._normed_version == sae.W_dec._version
        with torch.no_grad():
            Wd.data /= Wd.data.norm(dim=1, keepdim=True) + torch.finfo(torch.float32).eps
    for name, p, ref, p0 in zip(("W_enc", "b_enc", "W_dec", "b_dec"), params, (We, be, Wd, bd), params0):
        diff = (p.detach() - ref.data).abs()
        # Adam's first update is lr * g / (|g| + eps): ill-conditioned only where |g| ~ 1e-8 (see
        # _close_but_for_adam_sign_flips in test_gpu_parity.py)
        bad = diff > 2e-6 + 1e-5 * ref.data.abs() + 0.02 * lr
        assert bad.float().mean().item() < 1e-4, (name, int(bad.sum()), bad.numel())
        assert diff.max().item() <= 2.1 * lr, (name, diff.max().item())
        moved = (p.detach() - p0).abs().max().item()
        assert moved > 0.5 * lr, (name, "the step did not move the parameter")
        del diff, bad

    fired = torch.zeros(N_C2, dtype=torch.bool, device=dev)
    fired[sel[-1][1].reshape(-1)] = True
    aux_only = torch.zeros(N_C2, dtype=torch.bool, device=dev)
    aux_only[sel[1][1].reshape(-1)] = True
    aux_only &= ~fired
    assert int(aux_only.sum()) > 0, "the case must have dead features that only the AuxK selection picks"
    assert torch.equal(ts.num_tokens_since_fired == 0, fired)
    cnt = ts.num_tokens_since_fired
    assert bool((cnt[aux_only] == 1 + T).all())
    assert bool((cnt[~fired & ~dead_mask] == T).all())
    del sae, ts, We, be, Wd, bd, params0, leaves, sel, spy
