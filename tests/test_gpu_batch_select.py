"""The batch-level selection on the HIP path (csrc/batch_select.hip; include/msae.h, "batch-level selection"; DESIGN.md
section 7n) against the sorting restatement tests/batch_select_ref.py.  Every comparison is on BITS: there is no tolerance
anywhere in this file.

  * msae_batch_kth_f32: shapes that fill no wave / workgroup / vector and one that needs many workgroups, a strided view,
    value sets on which every radix pass decides something, special values, the edges of K, the workspace contract.
  * msae_list_filter_f32 / _i64_f32: the one-wave and the workgroup kernel, scalar and table mode, both index types.
  * msae_decode_prefix_f32 / _i64_f32: the same bits as ops.decode on the filtered list, and the slots behind the length
    are never read (they hold NaN activations and indices past N here).
  * Sae.forward / Sae.encode of a "batchtopk" Sae against the restatement applied to the project's own exact pre_acts, with
    and without saturated rows, under torch.cuda.set_sync_debug_mode("error").
  * three training steps with the new ops against the same steps with ops.batch_select and the lengths= decode replaced by
    torch and existing-kernel restatements: parameters, Adam moments, threshold and dead-feature counters bit-equal.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import batch_select_ref as ref
import guarded_ws
import synth

pytestmark = pytest.mark.gpu

MSAE_EINVAL, MSAE_EWS = -1, -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), what


def _relu_lists(rng, T, C, N, zeros=0.3):
    pre = rng.standard_normal((T, N)).astype(np.float32)
    pre[rng.random((T, N)) < zeros] = 0.0
    return ref.canonical_lists(np.maximum(pre, 0), C)


def _kth(vals_np, K, dev):
    from msae import ops

    th, n_pos = ops.batch_kth(torch.from_numpy(vals_np).to(dev), K)
    return th, n_pos


def _check_kth(vals_np, K, dev, what):
    th, n_pos = _kth(vals_np, K, dev)
    rt, rn = ref.theta(vals_np, K)
    _same_bits(th, rt, f"{what}: theta, K = {K}")
    assert int(n_pos) == rn, what


# ---- msae_batch_kth_f32 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(1, 1), (37, 13), (300, 32), (4096, 64)])
def test_batch_kth_shapes(dev, T, C):
    rng = np.random.default_rng(T + C)
    vals, _ = _relu_lists(rng, T, C, max(C, 96))
    n_pos = int(ref.positive(vals).sum())
    for K in sorted({1, max(n_pos // 3, 1), T * max(C // 4, 1), max(n_pos, 1), n_pos + 1, T * C + 5}):
        _check_kth(vals, K, dev, f"T = {T}, C = {C}")


def test_batch_kth_reads_a_view_of_a_wider_list_in_place(dev):
    from msae import ops

    rng = np.random.default_rng(7)
    vals, _ = _relu_lists(rng, 37, 20, 96)
    vals[:, 13:] += 50.0                                            # the columns outside the view would change every answer
    full = torch.from_numpy(vals).to(dev)
    for K in (1, 100, 37 * 13):
        th, n_pos = ops.batch_kth(full[:, :13], K)
        rt, rn = ref.theta(vals[:, :13], K)
        _same_bits(th, rt, f"view, K = {K}")
        assert int(n_pos) == rn


def test_batch_kth_values_on_which_every_pass_decides(dev):
    # all equal: every K gives that value
    _check_kth(np.full((9, 7), 2.5, np.float32), 1, dev, "equal")
    _check_kth(np.full((9, 7), 2.5, np.float32), 40, dev, "equal")
    _check_kth(np.full((9, 7), 2.5, np.float32), 63, dev, "equal")
    # 256 values that differ in their last 8 mantissa bits only: the first three passes see one bin, the last decides
    low = (np.uint32(0x3F800000) | np.random.default_rng(1).permutation(256).astype(np.uint32)).view(np.float32).reshape(16, 16)
    for K in (1, 2, 100, 255, 256, 257):
        _check_kth(low, K, dev, "low byte")
    # ... and 256 x 3 values spread over every byte: each pass splits
    rng = np.random.default_rng(2)
    spread = rng.integers(1, 0x7F800000, 768, dtype=np.uint32).view(np.float32).reshape(24, 32)
    for K in (1, 77, 400, 768):
        _check_kth(spread, K, dev, "spread")


def test_batch_kth_special_values(dev):
    v = np.array([[np.nan, -0.0, -3.0, 0.0, 1e-45, 3e-39], [np.inf, -np.inf, 2.0, -1e-40, np.float32(3.4e38), 1.0]], np.float32)
    assert int(ref.positive(v).sum()) == 6
    for K in range(1, 9):
        _check_kth(v, K, dev, "specials")
    assert float(_kth(v, 1, dev)[0]) == np.inf and np.float32(float(_kth(v, 6, dev)[0])) == np.float32(1e-45)


def test_batch_kth_edges_of_k(dev):
    rng = np.random.default_rng(3)
    vals, _ = _relu_lists(rng, 37, 13, 40, zeros=0.6)
    P = int(ref.positive(vals).sum())
    assert 1 < P < 37 * 13
    smallest = np.sort(vals[ref.positive(vals)])[0]
    for K in (1, P, P + 1, 37 * 13 + 1, 10 ** 12):
        _check_kth(vals, K, dev, "edges")
    _same_bits(_kth(vals, P + 1, dev)[0], smallest, "K = |P| + 1 gives min P")
    _same_bits(_kth(vals, 10 ** 12, dev)[0], smallest, "K > T * C gives min P")
    empty = np.array([[0.0, -1.0, np.nan], [-0.0, -np.inf, 0.0]], np.float32)
    th, n_pos = _kth(empty, 2, dev)
    assert float(th) == np.inf and int(n_pos) == 0


_KTH_FILLS = {}


@pytest.mark.parametrize("fill", guarded_ws.FILLS)
def test_batch_kth_under_guarded_workspaces(dev, monkeypatch, fill):
    """ops._workspace replaced by the guarded, exact-size allocator: the request is what the helper returns, the guards stay
    intact, and the result is the restatement's -- the same bits under the three fills (nothing is read before written)."""
    from msae import _hip, ops

    rng = np.random.default_rng(5)
    T, C = 300, 32
    vals, _ = _relu_lists(rng, T, C, 96)
    alt, _ = _relu_lists(rng, T, C, 96)
    gws = guarded_ws.GuardedWorkspace(fill, dev)
    gws.what = f"msae_batch_kth_f32 T={T} C={C}"
    monkeypatch.setattr(ops, "_workspace", gws)
    if fill == "recycled":
        _kth(alt, 999, dev)
        gws.check()
    got = []
    for K in (1, T * 8, 10 ** 9):
        th, n_pos = _kth(vals, K, dev)
        gws.check()
        rt, rn = ref.theta(vals, K)
        _same_bits(th, rt, f"{fill}, K = {K}")
        assert int(n_pos) == rn
        got.append(_bits(th).item())
    assert {n for _, n in gws.requests} == {_hip.load().msae_batch_kth_ws_bytes(T, C)}
    assert _KTH_FILLS.setdefault("theta", got) == got


def test_batch_kth_refuses_a_short_workspace_and_bad_shapes(dev):
    from msae import _hip

    lib = _hip.load()
    P_ = _hip.ptr
    T, C = 37, 13
    vals = torch.rand(T, C, device=dev)
    theta = torch.full((), -7.0, device=dev)
    n_pos = torch.full((), -7, dtype=torch.int32, device=dev)
    st = _hip.stream_of(vals)
    need = lib.msae_batch_kth_ws_bytes(T, C)
    gws = guarded_ws.GuardedWorkspace("word3", dev)
    call = lambda ws, n, T_=T, C_=C, ld=C, K=5: lib.msae_batch_kth_f32(P_(vals), T_, C_, ld, K, P_(theta), P_(n_pos), ws, n, st)
    big = ctypes.c_void_p(vals.data_ptr())                          # (never touched: the refusals come before any launch)
    for kw in (dict(T_=0), dict(C_=0), dict(T_=4097, C_=4096, ld=4096), dict(ld=C - 1), dict(K=0), dict(K=-3)):
        assert call(big, 1 << 40, **kw) == MSAE_EINVAL, kw
    ptr, n, blk = gws.block(need - 1)
    before = blk.view.clone()
    assert call(ctypes.c_void_p(ptr), n) == MSAE_EWS and call(None, need) == MSAE_EWS
    gws.check()
    assert float(theta) == -7.0 and int(n_pos) == -7 and torch.equal(blk.view, before)      # outputs and workspace untouched
    ptr, n, _ = gws.block(need)
    assert call(ctypes.c_void_p(ptr), n) == 0
    gws.check()
    rt, rn = ref.theta(vals.cpu().numpy(), 5)
    _same_bits(theta, rt, "exact-size workspace")
    assert int(n_pos) == rn


# ---- msae_list_filter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True], ids=["scalar", "table"])
@pytest.mark.parametrize("C", [1, 3, 32, 64, 65, 256, 300])
def test_list_filter(dev, C, table):
    from msae import ops

    rng = np.random.default_rng(100 + C + table)
    T, N = 41, 512
    pre = np.abs(rng.standard_normal((T, N))).astype(np.float32)   # ~410 positive values a row: C = 300 can saturate
    pre[rng.random((T, N)) < 0.2] = 0.0
    vals, idx = ref.canonical_lists(pre, C)
    idx[5, C // 2] = N + 3                                          # outside [0, N): dropped in table mode, never looked up
    idx[6, 0] = -2
    if C >= 3:
        vals[2, 1] = np.nan                                         # a row that is no longer descending: the partition moves it
    tf = rng.random(N).astype(np.float32) * np.float32(1.2) if table else None
    thetas = [np.float32(tf.min())] if table else [np.float32(0.7), np.float32(np.inf), np.float32(0.0),
                                                   np.float32(vals[:, -1].max())]
    seen_sat = set()
    for th in thetas:
        rv, ri, rl, rs = ref.list_filter(vals, idx, th, tf)
        seen_sat |= set(rs.tolist())
        for dt in (torch.int32, torch.int64):
            v, i = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, dt)
            tft = None if tf is None else torch.from_numpy(tf).to(dev)
            acc = torch.full((), 11, dtype=torch.int32, device=dev)
            vo, io, ln, n_sat = ops.list_filter(v, i, torch.tensor(th, device=dev), tft, n_saturated=acc)
            ops.list_filter(v, i, float(th), tft, n_saturated=acc)                   # the counter accumulates over calls
            what = f"C = {C}, theta = {th}, {dt}"
            _same_bits(vo, rv, what)
            assert io.dtype == dt and np.array_equal(io.cpu().numpy(), ri.astype(io.cpu().numpy().dtype)), what
            assert np.array_equal(ln.cpu().numpy(), rl) and ln.dtype == torch.int32, what
            assert n_sat is acc and int(acc) == 11 + 2 * int(rs.sum()), what
        # the [:, :C] view of a wider list is read in place
        wide_v = torch.from_numpy(np.concatenate([vals, np.full((T, 5), 9.0, np.float32)], 1)).to(dev)
        wide_i = torch.from_numpy(np.concatenate([idx, np.zeros((T, 5), np.int64)], 1)).to(dev)
        vo, io, ln, _ = ops.list_filter(wide_v[:, :C], wide_i[:, :C], float(th), None if tf is None else torch.from_numpy(tf).to(dev))
        _same_bits(vo, rv, f"C = {C}: view")
        assert np.array_equal(io.cpu().numpy(), ri) and np.array_equal(ln.cpu().numpy(), rl)
    if not table:
        assert seen_sat == {True, False}, "the case needs saturated and unsaturated rows"


def test_list_filter_refusals(dev):
    from msae import _hip

    lib = _hip.load()
    P_ = _hip.ptr
    v = torch.rand(4, 8, device=dev)
    i = torch.zeros(4, 8, dtype=torch.int32, device=dev)
    th = torch.zeros((), device=dev)
    ln = torch.full((4,), -7, dtype=torch.int32, device=dev)
    vo, io = torch.full_like(v, -7.0), torch.full_like(i, -7)
    st = _hip.stream_of(v)
    call = lambda T=4, C=8, ld=8, theta=th, tf=None, N=0: lib.msae_list_filter_f32(
        P_(v), P_(i), T, C, ld, P_(theta), P_(tf), N, P_(vo), P_(io), P_(ln), None, st)
    for kw in (dict(T=-1), dict(C=0), dict(C=4097, ld=4097), dict(ld=7), dict(theta=None), dict(tf=th, N=0)):
        assert call(**kw) == MSAE_EINVAL, kw
    assert call(T=0) == 0
    torch.cuda.synchronize()
    assert bool((ln == -7).all()) and bool((vo == -7).all()) and bool((io == -7).all())


# ---- msae_decode_prefix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 128, 1000, 1002, 1028])
def test_decode_prefix_equals_decode_on_the_filtered_list(dev, d):
    """d = 1002 is no multiple of 4 and takes the one-column-per-lane kernel; 1028 needs a second column slab of 1024."""
    from msae import ops

    rng = np.random.default_rng(d)
    N, C = 64, 16
    lens = np.array([0, 1, 7, 8, 9, C, C + 5, -3, 15, 16, 2], np.int32)
    T = lens.size
    eff = np.clip(lens, 0, C)
    vals = (rng.random((T, C)).astype(np.float32) + np.float32(0.1))
    idx = np.stack([rng.permutation(N)[:C] for _ in range(T)]).astype(np.int64)
    live = np.arange(C)[None] < eff[:, None]
    filtered = np.where(live, vals, np.float32(0.0))
    poison_v = np.where(live, vals, np.float32(np.nan))
    poison_i = np.where(live, idx, N + 1 + idx)
    W = torch.from_numpy(rng.standard_normal((N, d)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rng.standard_normal(d).astype(np.float32)).to(dev)
    ln = torch.from_numpy(lens).to(dev)
    was = ops._DEBUG_BOUNDS
    ops.set_debug_bounds(True)                                       # an index past N that IS read would raise here
    try:
        for dt in (torch.int32, torch.int64):
            for bias in (b, None):
                want = ops.decode(torch.from_numpy(idx).to(dev, dt), torch.from_numpy(filtered).to(dev), W, bias)
                got = ops.decode(torch.from_numpy(poison_i).to(dev, dt), torch.from_numpy(poison_v).to(dev), W, bias, ln)
                _same_bits(got, want, f"d = {d}, {dt}, bias {bias is not None}")
                clean = ops.decode(torch.from_numpy(idx).to(dev, dt), torch.from_numpy(filtered).to(dev), W, bias, ln)
                _same_bits(clean, want, f"d = {d}: filtered list with lengths")
    finally:
        ops.set_debug_bounds(was)
    assert np.isfinite(got.cpu().numpy()).all()
    # the gradient: the kept slots' equals the plain decode's, the slots behind the length get exactly 0
    a1 = torch.from_numpy(filtered).to(dev).requires_grad_()
    a2 = torch.from_numpy(poison_v).to(dev).requires_grad_()
    W1, W2 = W.clone().requires_grad_(), W.clone().requires_grad_()
    g = torch.from_numpy(rng.standard_normal((T, d)).astype(np.float32)).to(dev)
    ops.decode(torch.from_numpy(idx).to(dev), a1, W1, b).backward(g)
    ops.decode(torch.from_numpy(poison_i).to(dev), a2, W2, b, ln).backward(g)
    _same_bits(a2.grad, np.where(live, a1.grad.cpu().numpy(), np.float32(0.0)), "activation gradient")
    _same_bits(W2.grad, W1.grad, "decoder gradient")


# ---- Sae level --------------------------------------------------------------------------------------------------------------
D_, N_, K_ = 128, 8192, 8


def _sae(dev, cap=0, activation="batchtopk"):
    from msae import Sae, SaeConfig

    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(D_, N_, seed=21)
    sae = Sae(D_, SaeConfig(num_latents=N_, k=K_, activation=activation, batch_cap=cap), device=dev)
    with torch.no_grad():
        for p, a in ((sae.encoder.weight, W_enc), (sae.encoder.bias, b_enc), (sae.W_dec, W_dec), (sae.b_dec, b_dec)):
            p.copy_(torch.from_numpy(a))
    sae.invalidate_prepared()
    return sae


_PRE = {}


def _restated(dev, T, n_outlier, C):
    """x, and the restatement applied to the project's own exact pre_acts (computed once per shape, never modified)"""
    key = (T, n_outlier, C)
    if key not in _PRE:
        x = torch.from_numpy(synth.activations(T, D_, seed=22, n_outlier=n_outlier)).to(dev)
        with torch.no_grad():
            pre = _sae(dev, C).pre_acts(x).cpu().numpy()
        vals, idx = ref.canonical_lists(pre, C)
        _PRE[key] = (x, pre, vals, idx, ref.batch_select(vals, idx, K_))
    return _PRE[key]


@pytest.mark.parametrize("T", [300, 40])
@pytest.mark.parametrize("n_outlier,C", [(4, 32), (0, 64)], ids=["saturated", "unsaturated"])
def test_sae_forward_and_encode_against_the_restatement(dev, T, n_outlier, C):
    x, pre, vals, idx, (rv, ri, rl, rt, rs) = _restated(dev, T, n_outlier, C)
    if n_outlier:
        assert rs.any() and not rs.all(), "the case needs saturated and unsaturated rows"
        print(f"T = {T}, C = {C}: {int(rs.sum())} of {T} rows saturated, theta = {rt}")
    else:
        assert not rs.any(), "the case needs a batch without a saturated row"
        th_dense, keep = ref.dense_batchtopk(pre, K_)
        print(f"T = {T}, C = {C}: no row saturated, longest row {int(rl.max())}, {int((vals == rt).sum())} value(s) at theta")
    sae = _sae(dev, 0 if C == 32 else C)
    assert sae.cfg.cap == C
    sae.train()
    sae(x)                                                          # warm: library load, operand preparation, workspaces
    with torch.no_grad():
        sae.encode(x, threshold=1.0)
    with no_sync():
        out = sae(x)
        with torch.no_grad():
            enc, lengths = sae.encode(x, threshold=out.theta, return_lengths=True)
            recon = sae.decode(enc.top_acts, enc.top_indices, lengths)
    what = f"T = {T}, C = {C}"
    _same_bits(out.theta, rt, what)
    _same_bits(out.latent_acts, rv, what)
    assert np.array_equal(out.latent_indices.cpu().numpy(), idx) and np.array_equal(out.lengths.cpu().numpy(), rl), what
    assert int(out.n_saturated) == int(rs.sum()) and out.latent_acts.shape == (T, C)
    # the threshold encode with this batch's theta is the same selection, and its decode the forward's reconstruction
    _same_bits(enc.top_acts, rv, what)
    assert np.array_equal(enc.top_indices.cpu().numpy(), ri) and np.array_equal(lengths.cpu().numpy(), rl)
    _same_bits(recon, out.sae_out, what)
    with torch.no_grad():
        _same_bits(sae.decode(out.latent_acts, out.latent_indices), out.sae_out, f"{what}: decode without lengths")
    if not n_outlier:
        # no saturated row: exactly the uncapped BatchTopK over the dense latents
        _same_bits(out.theta, th_dense, what)
        dense = np.zeros_like(pre)
        np.put_along_axis(dense, out.latent_indices.cpu().numpy(), out.latent_acts.detach().cpu().numpy(), 1)
        _same_bits(dense, np.where(keep, pre, np.float32(0.0)), f"{what}: dense BatchTopK")
    # the learned threshold: an error while it is -1, then the buffer is what encode uses
    with pytest.raises(RuntimeError, match="not learned"), torch.no_grad():
        sae.encode(x)
    sae.set_threshold(float(rt))
    with no_sync(), torch.no_grad():
        again = sae.encode(x)
    _same_bits(again.top_acts, rv, f"{what}: learned threshold")


def test_threshold_table_on_a_topk_sae(dev):
    """"top-k, then drop what lies below its feature's threshold" on a TopK Sae, with a per-feature table."""
    T = 300
    x, pre, _, _, _ = _restated(dev, T, 4, 32)
    sae = _sae(dev, activation="topk")
    sae.eval()
    rng = np.random.default_rng(4)
    table = (rng.random(N_) * 20).astype(np.float32)
    vals, idx = ref.canonical_lists(pre, K_)
    rv, ri, rl, _ = ref.list_filter(vals, idx, table.min(), table)
    assert 0 < rl.sum() < T * K_
    with torch.no_grad():
        plain = sae.encode(x)
        enc, lengths = sae.encode(x, threshold=torch.from_numpy(table).to(dev), return_lengths=True)
    assert np.array_equal(plain.top_indices.cpu().numpy(), idx)
    _same_bits(enc.top_acts, rv, "table")
    assert np.array_equal(enc.top_indices.cpu().numpy(), ri) and np.array_equal(lengths.cpu().numpy(), rl)
    assert enc.top_acts.shape == (T, K_)


# ---- training ---------------------------------------------------------------------------------------------------------------
def _batch_select_torch(acts, idx, k):
    """ops.batch_select in torch ops: a sort for theta, a where for the mask (its autograd is the mask's)."""
    C = acts.shape[-1]
    flat = acts.detach().reshape(-1, C)
    P = torch.sort(flat[flat > 0], descending=True).values
    theta = P[min(flat.shape[0] * k, P.numel()) - 1].clone() if P.numel() else torch.full((), float("inf"), device=acts.device)
    keep = (acts.detach() > 0) & (acts.detach() >= theta)
    lengths = keep.sum(-1).to(torch.int32)
    return (torch.where(keep, acts, torch.zeros((), device=acts.device)), lengths, theta,
            (lengths == C).sum().to(torch.int32))


def _train_run(dev, monkeypatch, restated: bool):
    from msae import ops
    from msae.train import SaeTrainStep

    with monkeypatch.context() as m:
        if restated:
            plain_decode = ops.decode
            m.setattr(ops, "batch_select", _batch_select_torch)
            m.setattr(ops, "decode", lambda i, a, W, b, lengths=None: plain_decode(i, a, W, b))
        sae = _sae(dev)
        ts = SaeTrainStep(sae, lr=1e-3, auxk_alpha=1 / 32, dead_feature_threshold=250, micro_acc_steps=2)
        snaps = []
        for s in range(3):
            x = torch.from_numpy(synth.activations(301, D_, seed=60 + s)).to(dev)      # chunks of 151 and 150 tokens
            dead = int((ts.num_tokens_since_fired > ts.dead_feature_threshold).sum())
            res = ts.step(x)
            snaps.append(dict(dead=dead, theta=res["theta"].clone(), n_sat=res["n_saturated"].clone(),
                              thr=sae.threshold.clone(), since=ts.num_tokens_since_fired.clone(),
                              params=[p.detach().clone() for p in ts.params], m=[t.clone() for t in ts.exp_avg],
                              v=[t.clone() for t in ts.exp_avg_sq], fvu=res["fvu"].clone(), aux=res["auxk_loss"].clone()))
    return snaps


def test_three_training_steps_equal_the_restated_ops_bit_for_bit(dev, monkeypatch):
    new = _train_run(dev, monkeypatch, restated=False)
    old = _train_run(dev, monkeypatch, restated=True)
    assert new[0]["dead"] == 0 and new[1]["dead"] > 0, "steps 2 and 3 must run the AuxK term with a dead mask"
    assert float(new[2]["aux"]) > 0 and float(new[0]["thr"]) > 0
    for s, (a, b) in enumerate(zip(new, old)):
        assert a["dead"] == b["dead"], s
        for name in ("theta", "thr", "fvu", "aux"):
            _same_bits(a[name], b[name], f"step {s}: {name}")
        assert torch.equal(a["n_sat"], b["n_sat"]) and torch.equal(a["since"], b["since"]), s
        for kind in ("params", "m", "v"):
            for j, (p, q) in enumerate(zip(a[kind], b[kind])):
                _same_bits(p, q, f"step {s}: {kind}[{j}]")
    assert not torch.equal(new[0]["params"][0], new[2]["params"][0])                   # (the steps moved something)
