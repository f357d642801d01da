"""The kernels built on the shared device helpers (csrc/sortsel.h: the LDS bitonic sort; csrc/wave_ops.h: the workgroup
scan) at the smallest shapes that reach their seams: tile edges of the three scan kernels, the sort's padding and thread
counts, every optional output of the one merge kernel.  References are CPU computations in torch / numpy; equality is exact
unless a test says otherwise."""
import numpy as np
import pytest
import torch

import edits_ref as eref
from oracle import oracle

pytestmark = pytest.mark.gpu

MSAE_EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


# ---- compact_flags: 1024 flags per tile ------------------------------------------------------------------------------
@pytest.mark.parametrize("T,p", [(0, 0.3), (1, 0.3), (63, 0.3), (64, 0.3), (65, 0.3), (1023, 0.3), (1024, 0.3), (1025, 0.3),
                                 (2049, 0.3), (5000, 0.3), (2049, 1.0), (2049, 0.0)])
def test_compact_flags_across_tiles(dev, T, p):
    from msae import ops

    g = torch.Generator().manual_seed(T + 1)
    flags = (torch.rand(T, generator=g) < p).to(torch.int32)
    if T == 1:
        flags[0] = 1
    rows, n = ops.compact_flags(flags.to(dev))
    want = torch.nonzero(flags).flatten().to(torch.int32)
    assert int(n) == want.numel()
    assert torch.equal(rows[: want.numel()].cpu(), want)


# ---- sparsify: 1024 tokens per scan tile, 64-thread sort of next_pow2(k) keys ---------------------------------------------
@pytest.mark.parametrize("B,S", [(1, 1023), (1, 1024), (1, 1025), (3, 700)])
def test_sparsify_across_scan_tiles(dev, B, S):
    from msae import ops

    k, N, thresh, row_base = 5, 64, 1e-5, 17
    g = torch.Generator().manual_seed(B * 10000 + S)
    vals = torch.randn(B, S, k, generator=g)
    vals[torch.rand(B, S, k, generator=g) < 0.2] = 5e-6                      # below the threshold: dropped
    idx = torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(B * S)]).reshape(B, S, k)
    bitmap = (torch.arange(N) % 3 != 0).to(torch.uint8)                      # a third of the features filtered out
    keep = (vals.abs() > thresh) & bitmap[idx].bool()
    tok = torch.arange(B * S).reshape(B, S, 1).expand(B, S, k)
    order = torch.sort((tok * N + idx)[keep], stable=True).indices         # (row, pos, feature): features are distinct per token
    t_k, f_k, v_k = tok[keep][order], idx[keep][order], vals[keep][order]
    ref_loc = torch.stack((row_base + t_k // S, t_k % S, f_k), 1).to(torch.int64)
    args = (vals.to(dev), idx.to(dev), N)
    loc, act = ops.sparsify(*args, row_base=row_base, thresh=thresh, filter_bitmap=bitmap.to(dev), sync=True)
    assert torch.equal(loc.cpu(), ref_loc) and torch.equal(act.cpu(), v_k)
    loc, act, nnz = ops.sparsify(*args, row_base=row_base, thresh=thresh, filter_bitmap=bitmap.to(dev), sync=False)
    assert int(nnz) == ref_loc.shape[0]
    assert torch.equal(loc[: int(nnz)].cpu(), ref_loc) and torch.equal(act[: int(nnz)].cpu(), v_k)


# ---- weight-gradient scan: 8192 counts per tile, eight per thread ---------------------------------------------------------
@pytest.mark.parametrize("N", [7, 8, 8191, 8192, 8193, 16391])
def test_wgrad_scan_tile_edges(dev, N):
    """ops.decode_bwd(..., False, True) at d = 4, A = 64, k = 3 against a float64 index_add_ within
    2e-7 * sum|act| * max|g| * sqrt(L) + 1e-12 (an f32 chain of L terms; test_decode_bwd_wdec_at_c2_vs_float64_index_add's
    bound); bit-identical twice; rows without a pair exactly zero, rows with one pair exactly the rounded product."""
    from msae import ops

    d, A, k = 4, 64, 3
    g = torch.Generator().manual_seed(N)
    idx = torch.randint(0, N, (A, k), generator=g)
    forced = [f for f in (0, N - 1, 8191, 8192) if 0 <= f < N]
    for j, f in enumerate(forced):
        idx[j, 0] = f
    acts = torch.rand(A, k, generator=g) + 0.05
    gout = torch.randn(A, d, generator=g)
    W = torch.empty(N, d, device=dev)                                        # only its shape is read
    _, gw = ops.decode_bwd(idx.to(dev), acts.to(dev), W, gout.to(dev), False, True)
    _, gw2 = ops.decode_bwd(idx.to(dev), acts.to(dev), W, gout.to(dev), False, True)
    assert torch.equal(gw, gw2)
    gw = gw.cpu()
    flat = idx.reshape(-1)
    ref = torch.zeros(N, d, dtype=torch.float64)
    ref.index_add_(0, flat, acts.reshape(-1, 1).double() * gout.double().repeat_interleave(k, 0))
    mag = torch.zeros(N, dtype=torch.float64).index_add_(0, flat, acts.reshape(-1).double())
    counts = torch.bincount(flat, minlength=N)
    tol = 2e-7 * mag * float(gout.abs().max()) * counts.clamp(min=1).double().sqrt() + 1e-12
    err = (gw.double() - ref).abs().amax(dim=1)
    print("wgrad scan N", N, "worst err/tol", float((err / tol).max()))
    assert (err <= tol).all()
    assert (counts[forced] >= 1).all()
    assert (gw[counts == 0] == 0).all()
    single = torch.nonzero(counts == 1).flatten()
    pos = torch.full((N,), -1, dtype=torch.long)
    pos[flat] = torch.arange(A * k)
    p = pos[single]
    assert torch.equal(gw[single], acts.reshape(-1)[p].unsqueeze(1) * gout[p // k])


# ---- the merge kernel through the C ABI: every optional argument --------------------------------------------------------
def _gathered(T, G, kl):
    g = torch.Generator().manual_seed(T * 7 + G)
    vals = torch.relu(torch.randn(G, T, kl, generator=g)).sort(dim=-1, descending=True).values
    vals[:, : max(1, T // 2)] = torch.round(vals[:, : max(1, T // 2)] * 2) / 2          # ties across shards
    vals = vals.sort(dim=-1, descending=True).values
    idx = torch.stack([torch.stack([torch.randperm(2000, generator=g)[:kl] + 2000 * s for _ in range(T)])
                       for s in range(G)]).to(torch.int32)
    gathered = torch.stack((vals.view(torch.int32), idx), 1).reshape(G * 2, T, kl).contiguous()
    return vals, idx, gathered


@pytest.mark.parametrize("T,G,kl,k", [(9, 3, 5, 7), (4, 1, 64, 64), (3, 8, 1024, 32)])
def test_merge_kernel_every_output(dev, T, G, kl, k):
    from msae import _hip
    from msae.parallel import canonical_key, merge_topk

    lib = _hip.load()
    vals, idx, gathered = _gathered(T, G, kl)
    gd = gathered.to(dev)
    st = _hip.stream_of(gd)
    av, ai = vals.permute(1, 0, 2), idx.permute(1, 0, 2).long()
    rv, ri = merge_topk(av.reshape(T, -1), ai.reshape(T, -1), k)
    if kl < k:
        kth = canonical_key(rv[:, -1], ri[:, -1])
        rf = (canonical_key(av[:, :, -1], ai[:, :, -1]) >= kth[:, None]).any(dim=1)
    else:
        rf = torch.zeros(T, dtype=torch.bool)

    def fresh():
        return (torch.full((T, k), -7.0, device=dev), torch.full((T, k), -7, dtype=torch.int32, device=dev),
                torch.full((T, k), -7, dtype=torch.int64, device=dev))

    v, i32, _ = fresh()
    fl = torch.full((T,), -7, dtype=torch.int32, device=dev)
    assert lib.msae_merge_topk(_hip.ptr(gd), T, G, kl, k, _hip.ptr(v), _hip.ptr(i32), _hip.ptr(fl), st) == 0
    assert torch.equal(v.cpu(), rv) and torch.equal(i32.cpu().long(), ri) and torch.equal(fl.cpu().bool(), rf)
    assert ((fl == 0) | (fl == 1)).all()

    mask = (torch.arange(T) % 2 == 0).to(torch.int32)                        # mixed: T >= 3 everywhere
    on, off = mask.bool(), ~mask.bool()
    for use32, use64 in ((True, False), (False, True), (True, True)):
        v, i32, i64 = fresh()
        rc = lib.msae_merge_topk_masked(_hip.ptr(gd), T, G, kl, k, _hip.ptr(mask.to(dev)), _hip.ptr(v),
                                        _hip.ptr(i32) if use32 else None, _hip.ptr(i64) if use64 else None, st)
        assert rc == 0
        v, i32, i64 = v.cpu(), i32.cpu(), i64.cpu()
        assert torch.equal(v[on], rv[on]) and (v[off] == -7.0).all()
        assert torch.equal(i32[on].long(), ri[on]) if use32 else (i32 == -7).all()
        assert torch.equal(i64[on], ri[on]) if use64 else (i64 == -7).all()
        assert (i32[off] == -7).all() and (i64[off] == -7).all()
    v, i32, i64 = fresh()
    zero = torch.zeros(T, dtype=torch.int32, device=dev)
    assert lib.msae_merge_topk_masked(_hip.ptr(gd), T, G, kl, k, _hip.ptr(zero), _hip.ptr(v), _hip.ptr(i32), _hip.ptr(i64),
                                      st) == 0
    assert (v == -7.0).all() and (i32 == -7).all() and (i64 == -7).all()


@pytest.mark.parametrize("G,kl,k", [(1, 8193, 32), (1, 4, 8)])
def test_merge_entry_points_refuse_bad_sizes(dev, G, kl, k):
    """G * kl = 8193 (one more than the LDS sort holds) and G * kl < k: MSAE_EINVAL from both entry points, nothing launched."""
    from msae import _hip

    lib, T = _hip.load(), 1
    gd = torch.zeros(G * 2 * T * kl, dtype=torch.int32, device=dev)
    v = torch.zeros(T, k, device=dev)
    i32 = torch.zeros(T, k, dtype=torch.int32, device=dev)
    fl = torch.ones(T, dtype=torch.int32, device=dev)
    st = _hip.stream_of(gd)
    assert lib.msae_merge_topk(_hip.ptr(gd), T, G, kl, k, _hip.ptr(v), _hip.ptr(i32), _hip.ptr(fl), st) == MSAE_EINVAL
    assert lib.msae_merge_topk_masked(_hip.ptr(gd), T, G, kl, k, _hip.ptr(fl), _hip.ptr(v), _hip.ptr(i32), None,
                                      st) == MSAE_EINVAL


# ---- edit_topk: 64 threads up to 128 keys, n_sort / 2 threads up to 2048 keys, 1024 beyond ----------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("k,E", [(30, 1), (56, 36), (120, 8), (1000, 10), (1960, 40), (2000, 40)])
def test_edit_topk_thread_count_seam(dev, k, E, wide):
    """k + 2 E = 32 and 128 (one wave), 136 (128 threads), 1020 (512), 2040 and 2080 (1024 threads, 2048 and 4096 keys)
    against the definition: dense latents, edits applied, canonical top-k (edits_ref.dense_topk)."""
    from msae import ops

    T, N = 3, 4096
    rng = np.random.default_rng(k * 100 + E)
    L = np.maximum(rng.standard_normal((T, N)).astype(np.float32), 0)       # half zeros: ties broken by index
    L[:, ::7] = np.round(L[:, ::7] * 4) / 4                                    # ties among positive values
    v0, i0 = oracle.topk(L, k + E)
    hot = i0[0, : E // 2]                                                      # features inside the list ...
    cold = np.setdiff1d(np.arange(N), i0.reshape(-1))[: E - E // 2]            # ... and outside every list
    feats_all = np.concatenate([hot, cold])
    n_set = (E + 1) // 2
    set_vals = np.where(np.arange(n_set) % 2 == 0, 9.5, 0.25).astype(np.float32)
    feats, vals, kinds = eref.merge((feats_all[:n_set], set_vals), feats_all[n_set:])
    assert len(feats) == E
    idx_in = torch.from_numpy(i0.astype(np.int64 if wide else np.int32)).to(dev)
    gv, gi = ops.edit_topk(torch.from_numpy(v0).to(dev), idx_in, torch.from_numpy(feats).to(dev),
                           torch.from_numpy(vals).to(dev), torch.from_numpy(kinds).to(dev), N, k)
    assert gi.dtype == (torch.int64 if wide else torch.int32)
    ref_v, ref_i = eref.dense_topk(L, k, feats, vals, kinds)
    assert np.array_equal(gi.cpu().numpy(), ref_i)
    assert np.array_equal(eref.bits(gv.cpu().numpy()), eref.bits(ref_v))
