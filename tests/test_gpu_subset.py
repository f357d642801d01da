"""GPU checks of the exact encode over a feature subset (include/msae.h): msae_pre_acts_features_f32
and msae_topk_map_i64_f32 against the numpy restatement on the C oracle (tests/subset_ref.py), ops.topk_within across
chunk seams, and `auxk_path="subset"` of Sae.forward / SaeTrainStep against the dense branch it replaces.  Every
comparison of activations is on the int32 views of the floats, element for element."""
import copy
import gc

import numpy as np
import pytest
import torch

import hostile
import subset_ref
from oracle import oracle

pytestmark = pytest.mark.gpu

N1 = 1024
T_ALL, M_ALL = (1, 129, 257), (1, 127, 128, 129, 300)        # tile tails on the token side / the column tile edge (128)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got: torch.Tensor, ref: np.ndarray) -> bool:
    return np.array_equal(got.contiguous().cpu().numpy().view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))


_PROBLEMS: dict = {}


def _problem(d, T=257, N=N1):
    """Host operands of one d, drawn once: x [T, d], W [N, d], b_enc [N], b_dec [d], and an unsorted feature list of 300
    entries with repeats (its prefixes are the shorter lists: a column does not depend on the rest of the list)."""
    if (d, T, N) not in _PROBLEMS:
        rng = np.random.default_rng(100 + d)
        x = rng.standard_normal((T, d)).astype(np.float32)
        W = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
        b = (0.1 * rng.standard_normal(N)).astype(np.float32)
        bd = (0.1 * rng.standard_normal(d)).astype(np.float32)
        f = rng.integers(0, N, 300).astype(np.int32)
        f[:4] = (N - 1, 0, 5, 5)
        _PROBLEMS[(d, T, N)] = (x, W, b, bd, f)
    return _PROBLEMS[(d, T, N)]


_TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


# ---- msae_pre_acts_features_f32 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(_TORCH_DT))
@pytest.mark.parametrize("d", [64, 100, 70])
def test_pre_acts_features_bit_exact_vs_restatement(dev, d, dt):
    """d = 64: whole k-tiles; 100: the last k-tile ends early on the vector path; 70: d % 4 != 0, the generic staging path.
    Every T x M of the tile-edge sets, lists unsorted with repeats (prefixes of one list), against ONE reference."""
    from msae import ops

    x, W, b, bd, f = _problem(d)
    xt = torch.from_numpy(x).to(dev, _TORCH_DT[dt])
    ref = subset_ref.pre_acts_features(xt.float().cpu().numpy(), W, b, bd, f)            # [257, 300]
    Wt, bt, bdt, ft = (torch.from_numpy(a).to(dev) for a in (W, b, bd, f))
    for T in T_ALL:
        for M in M_ALL:
            out = ops.pre_acts_features(xt[:T], Wt, bt, bdt, ft[:M])
            assert out.shape == (T, M) and out.dtype == torch.float32
            assert out.stride(0) == (M + 3) // 4 * 4, "rows are M rounded up to 4 floats apart"
            assert _same_bits(out, ref[:T, :M]), (d, dt, T, M)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_pre_acts_features_at_the_production_row_length(dev, dt):
    """d = 4096 (a 16-KB row of W_enc per list entry), T = 129, M = 129: 128 k-tiles, one tail tile on both sides."""
    from msae import ops

    x, W, b, bd, f = _problem(4096, T=129)
    xt = torch.from_numpy(x).to(dev, _TORCH_DT[dt])
    ref = subset_ref.pre_acts_features(xt.float().cpu().numpy(), W, b, bd, f[:129])
    out = ops.pre_acts_features(xt, *(torch.from_numpy(a).to(dev) for a in (W, b, bd, f[:129])))
    assert _same_bits(out, ref)


def test_pre_acts_features_optional_operands_clamping_and_empty_list(dev):
    from msae import _hip, ops

    d, T = 100, 129
    x, W, b, bd, f = _problem(d)
    x = x[:T]
    xt, Wt, bt, bdt = (torch.from_numpy(a).to(dev) for a in (x, W, b, bd))
    f = f[:129]
    ft = torch.from_numpy(f).to(dev)
    # b_enc / b_dec each None once
    assert _same_bits(ops.pre_acts_features(xt, Wt, None, bdt, ft), subset_ref.pre_acts_features(x, W, None, bd, f))
    assert _same_bits(ops.pre_acts_features(xt, Wt, bt, None, ft), subset_ref.pre_acts_features(x, W, b, None, f))
    # entries outside [0, N) are clamped, never fault
    g = np.array([-1, N1 + 5, 7, -2 ** 31, 2 ** 31 - 1], dtype=np.int32)
    got = ops.pre_acts_features(xt, Wt, bt, bdt, torch.from_numpy(g).to(dev))
    assert _same_bits(got, subset_ref.pre_acts_features(x, W, b, bd, g))
    assert _same_bits(got, oracle.pre_acts(x, W, b, bd)[:, [0, N1 - 1, 7, 0, N1 - 1]])
    # M = 0: an empty result, no launch
    empty = ops.pre_acts_features(xt, Wt, bt, bdt, torch.empty(0, dtype=torch.int32, device=dev))
    assert empty.shape == (T, 0) and empty.dtype == torch.float32
    # relu = 0 through the C ABI, into a pitch wider than M (the columns beyond M are not written)
    M, ld = f.size, 140
    out = torch.full((T, ld), -7.0, device=dev)
    lib = _hip.load()
    with torch.cuda.device(dev):
        _hip.check(lib.msae_pre_acts_features_f32(_hip.ptr(xt), 0, _hip.ptr(Wt), _hip.ptr(bt), _hip.ptr(bdt), _hip.ptr(ft),
                                                  M, T, d, N1, 0, _hip.ptr(out), ld, _hip.stream_of(xt)), "features")
    raw = subset_ref.pre_acts_features(x, W, b, bd, f, relu=False)
    assert (raw < 0).any() and _same_bits(out[:, :M], raw)
    assert bool((out[:, M:] == -7.0).all())
    assert lib.msae_pre_acts_features_f32(_hip.ptr(xt), 0, _hip.ptr(Wt), None, None, _hip.ptr(ft), M, T, d, N1, 0,
                                          _hip.ptr(out), M - 1, None) != 0          # ld_out < M is refused


def test_pre_acts_features_unaligned_input_takes_the_generic_path(dev):
    """x starts one element into its buffer: 4 bytes off a 16-byte boundary with d % 4 == 0."""
    from msae import ops

    d, T = 64, 129
    x, W, b, bd, f = _problem(d)
    buf = torch.empty(T * d + 1, device=dev)
    xt = buf[1:].view(T, d)
    xt.copy_(torch.from_numpy(x[:T]))
    assert xt.data_ptr() % 16 == 4 and xt.is_contiguous()
    out = ops.pre_acts_features(xt, *(torch.from_numpy(a).to(dev) for a in (W, b, bd, f[:129])))
    assert _same_bits(out, subset_ref.pre_acts_features(x[:T], W, b, bd, f[:129]))


def test_pre_acts_features_equals_the_dense_op_columns(dev):
    from msae import ops

    x, W, b, bd, f = _problem(100)
    xt, Wt, bt, bdt, ft = (torch.from_numpy(a).to(dev) for a in (x, W, b, bd, f))
    dense = ops.pre_acts(xt, Wt, bt, bdt)
    sub = ops.pre_acts_features(xt, Wt, bt, bdt, ft)
    assert sub.shape == (257, 300)
    assert torch.equal(_bits(dense[:, ft.long()]), _bits(sub))


# ---- msae_topk_map_i64_f32 -------------------------------------------------------------------------------------------
def _topk_map(dev, lat: np.ndarray, col_map: np.ndarray, k: int, ld: int):
    from msae import _hip

    T, M = lat.shape
    buf = torch.zeros(T, ld, device=dev)
    buf[:, :M] = torch.from_numpy(lat)
    cm = torch.from_numpy(col_map.astype(np.int32)).to(dev)
    vals = torch.empty(T, k, device=dev)
    idx = torch.empty(T, k, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_topk_map_i64_f32(_hip.ptr(buf), T, M, k, ld, _hip.ptr(cm), _hip.ptr(vals), _hip.ptr(idx),
                                                     _hip.stream_of(buf)), "msae_topk_map_i64_f32")
    return vals, idx


@pytest.mark.parametrize("k", [1, 37, 300])
def test_topk_map_vs_restatement(dev, k):
    """T = 5, M = 300: a random post-ReLU row, an all-zero row, a row with exactly k - 1 positive values (the k-th winner
    is the first zero by position), a row of few distinct values (ties straddle k), a row with negatives.  An ascending
    map and a non-monotone one: ties resolve by POSITION, whatever the map says."""
    M = 300
    rng = np.random.default_rng(7 + k)
    lat = np.maximum(rng.standard_normal((5, M)), 0).astype(np.float32)
    lat[1] = 0.0
    lat[2] = 0.0
    lat[2, rng.permutation(M)[:k - 1]] = rng.random(k - 1).astype(np.float32) + 0.5
    assert int((lat[2] > 0).sum()) == k - 1
    lat[3] = np.round(rng.standard_normal(M) * 2) / 2
    lat[4] = rng.standard_normal(M)
    asc = np.sort(rng.permutation(5000)[:M])
    perm = rng.permutation(5000)[:M]
    assert (np.diff(perm) < 0).any()
    for name, cm in (("ascending", asc), ("non-monotone", perm)):
        rv, ri = subset_ref.topk_map(lat, cm, k)
        v, i = _topk_map(dev, lat, cm, k, ld=M)
        assert np.array_equal(i.cpu().numpy(), ri), (name, k)
        assert _same_bits(v, rv), (name, k)
    # ties by position: the all-zero row returns the map's first k entries in list order
    assert np.array_equal(_topk_map(dev, lat, perm, k, ld=M)[1][1].cpu().numpy(), perm[:k])
    # M % 4 != 0 in a pitch of M rounded up to 4 (what ops.topk_within hands over): element loads, same answer
    if k < M:
        rv, ri = subset_ref.topk_map(lat[:, :M - 1], perm[:M - 1], k)
        v, i = _topk_map(dev, lat[:, :M - 1], perm[:M - 1], k, ld=M)
        assert np.array_equal(i.cpu().numpy(), ri) and _same_bits(v, rv)


# ---- ops.topk_within ---------------------------------------------------------------------------------------------------
def test_topk_within_chunks_agree_with_one_chunk_and_the_restatement(dev):
    from msae import ops

    d, T, M, k = 100, 300, 129, 37
    x, W, b, bd, _ = _problem(d, T=T)
    f = np.sort(np.random.default_rng(5).permutation(N1)[:M]).astype(np.int32)
    xt, Wt, bt, bdt, ft = (torch.from_numpy(a).to(dev) for a in (x, W, b, bd, f))
    cap = 128 * 132 * 4                                         # one 128-row chunk of ld = 132: 128 + 128 + 44 rows
    assert ops.rows_per_chunk(T, M, cap) == 128 and ops.rows_per_chunk(T, M) == T
    v1, i1 = ops.topk_within(xt, Wt, bt, bdt, ft, k)
    v3, i3 = ops.topk_within(xt, Wt, bt, bdt, ft, k, max_ws_bytes=cap)
    assert i1.dtype == torch.int64 and v1.shape == (T, k)
    assert torch.equal(i1, i3) and torch.equal(_bits(v1), _bits(v3))
    rv, ri = subset_ref.topk_within(x, W, b, bd, f, k)
    assert np.array_equal(i1.cpu().numpy(), ri) and _same_bits(v1, rv)
    with pytest.raises(ValueError):
        ops.topk_within(xt, Wt, bt, bdt, ft, M + 1)


# ---- AuxK end to end ---------------------------------------------------------------------------------------------------
D2, N2, K2, T2 = 256, 8192, 8, 200


@pytest.fixture(scope="module")
def auxk_model(dev):
    """Sae(d = 256, N = 8192, k = 8, multi_topk: 4k = 32) with trained-like weights, residual-like bf16 -> f32 tokens."""
    from msae import Sae, SaeConfig

    W, b, bd = hostile.weights("trained_like", N2, D2, dev, seed=3)
    sae = Sae(D2, SaeConfig(num_latents=N2, k=K2, multi_topk=True), device=dev)
    with torch.no_grad():
        sae.encoder.weight.copy_(W)
        sae.encoder.bias.copy_(b)
        sae.b_dec.copy_(bd)
        sae.W_dec.copy_(W)
    sae.set_decoder_norm_to_unit_norm()
    x = hostile.activations(T2, D2, dev, seed=3).float()
    yield sae, x
    from msae import ops

    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


def _dead_mask(n_dead, N, dev, seed=11):
    m = torch.zeros(N, dtype=torch.bool, device=dev)
    m[torch.randperm(N, generator=torch.Generator(device=dev).manual_seed(seed), device=dev)[:n_dead]] = True
    return m


def _capture(monkeypatch):
    """Wraps ops.sparse_encode: -> the list its selections are appended to, one entry per call."""
    from msae import ops

    real, calls = ops.sparse_encode, []

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append([(v.detach().clone(), i.detach().clone()) for v, i in out])
        return out

    monkeypatch.setattr(ops, "sparse_encode", spy)
    return calls


def _forward_backward(sae, x, dead_mask, path):
    params = (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)
    for p in params:
        p.grad = None
    out = sae(x, dead_mask, auxk_path=path)
    (out.fvu + out.auxk_loss / 32 + out.multi_topk_fvu / 8).backward()
    losses = [t.detach().clone() for t in (out.fvu, out.auxk_loss, out.multi_topk_fvu)]
    grads = [p.grad.detach().clone() for p in params]
    for p in params:
        p.grad = None
    return losses, grads


def _assert_within_run_to_run(name, got, a, b):
    """`got` (subset mode) against dense run `a`, within the difference of the two dense runs `a` and `b` on the same
    inputs; zero difference -> the comparison is torch.equal."""
    spread = (a.double() - b.double()).abs().max().item() if a.numel() else 0.0
    print(f"{name}: dense run-to-run {spread:.3e}, subset - dense {(got.double() - a.double()).abs().max().item():.3e}")
    if spread == 0.0:
        assert torch.equal(got, a), name
    else:
        assert (got.double() - a.double()).abs().max().item() <= spread, (name, spread)


@pytest.mark.parametrize("n_dead", [1, 100, 128, 500])
def test_auxk_subset_forward_matches_the_dense_branch(dev, auxk_model, monkeypatch, n_dead):
    """k_aux = min(d / 2, num_dead) = 1, 100, 128, 128.  All three selections bit-identical to the dense branch's, every
    AuxK index dead, the AuxK term alive, losses and the four parameter gradients within the dense branch's own run-to-run
    difference."""
    sae, x = auxk_model
    dead = _dead_mask(n_dead, N2, dev)
    calls = _capture(monkeypatch)
    la, ga = _forward_backward(sae, x, dead, "dense")
    lb, gb = _forward_backward(sae, x, dead, "dense")
    ls, gs = _forward_backward(sae, x, dead, "subset")
    assert len(calls) == 3
    sel_d, sel_s = calls[0], calls[2]
    assert [v.shape[-1] for v, _ in sel_s] == [K2, min(D2 // 2, n_dead), 4 * K2] == [v.shape[-1] for v, _ in sel_d]
    for j, ((vd, id_), (vs, is_)) in enumerate(zip(sel_d, sel_s)):
        assert is_.dtype == torch.int64 and torch.equal(id_, is_), ("indices of selection", j)
        assert torch.equal(_bits(vd), _bits(vs)), ("values of selection", j)
    assert bool(dead[sel_s[1][1]].all()), "AuxK picked a live latent"
    assert float(ls[1]) > 0.0
    for name, s, a, b in zip(("fvu", "auxk_loss", "multi_topk_fvu"), ls, la, lb):
        _assert_within_run_to_run(name, s, a, b)
    for name, s, a, b in zip(("W_enc.grad", "b_enc.grad", "W_dec.grad", "b_dec.grad"), gs, ga, gb):
        _assert_within_run_to_run(name, s, a, b)


def test_auxk_subset_never_builds_the_dense_latents(dev, auxk_model, monkeypatch):
    from msae import ops

    sae, x = auxk_model
    dead = _dead_mask(100, N2, dev)

    def boom(*a, **kw):
        raise AssertionError("ops.pre_acts was called in subset mode")

    monkeypatch.setattr(ops, "pre_acts", boom)
    out = sae(x, dead, auxk_path="subset")
    assert float(out.auxk_loss.detach()) > 0.0
    sae.auxk_path = "subset"                       # the attribute is what `None` reads
    try:
        out2 = sae(x, dead)
    finally:
        del sae.auxk_path
    assert sae.auxk_path == "dense" and torch.equal(out2.auxk_loss, out.auxk_loss)
    with pytest.raises(AssertionError, match="subset mode"):
        sae(x, dead)                               # the control: the default branch does call it


def test_auxk_subset_peak_memory_stays_below_the_dense_latents(dev):
    """T = 512, N = 16384, d = 256, 200 dead: across forward + backward, after a warm-up call per mode, the peak above the
    resting allocation is below T N 4 bytes (one dense [T, N] f32 tensor) in subset mode and at least that in dense mode.
    The two weight matrices are frozen for this measurement: each of their gradients is an [N, d] f32 buffer of N d 4 =
    16 MiB in either mode -- together T N 4 = 32 MiB at this shape, before autograd's temporaries of the three decodes --
    and would mask the quantity the bound is about; the biases keep their gradients, so the encoder node's backward runs."""
    from msae import Sae, SaeConfig, ops

    T, N, d, n_dead = 512, 16384, 256, 200
    W, b, bd = hostile.weights("trained_like", N, d, dev, seed=4)
    sae = Sae(d, SaeConfig(num_latents=N, k=K2, multi_topk=True), device=dev)
    with torch.no_grad():
        sae.encoder.weight.copy_(W)
        sae.encoder.bias.copy_(b)
        sae.b_dec.copy_(bd)
        sae.W_dec.copy_(W)
    del W, b, bd
    sae.set_decoder_norm_to_unit_norm()
    sae.encoder.weight.requires_grad_(False)
    sae.W_dec.requires_grad_(False)
    x = hostile.activations(T, d, dev, seed=4).float()
    dead = _dead_mask(n_dead, N, dev)
    peak = {}
    for path in ("subset", "dense"):
        for measured in (False, True):             # one warm-up call per mode (workspaces, operand buffers)
            sae.encoder.bias.grad = sae.b_dec.grad = None
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            out = sae(x, dead, auxk_path=path)
            (out.fvu + out.auxk_loss / 32 + out.multi_topk_fvu / 8).backward()
            torch.cuda.synchronize()
            if measured:
                peak[path] = torch.cuda.max_memory_allocated(dev) - base
            assert sae.encoder.bias.grad is not None and sae.b_dec.grad is not None
            del out
    print(f"peak above rest: subset {peak['subset']} B, dense {peak['dense']} B, T N 4 = {T * N * 4} B")
    ops.release_workspaces()
    assert peak["subset"] < T * N * 4
    assert peak["dense"] >= T * N * 4


# ---- one optimisation step -----------------------------------------------------------------------------------------------
def test_train_step_subset_matches_its_dense_twin(dev, auxk_model, monkeypatch):
    """SaeTrainStep.step with auxk_alpha = 1/32, dead_feature_threshold = 0 and 100 features marked dead, in subset mode
    against twins built from the same state in dense mode: parameters and num_tokens_since_fired after the step, within
    the difference of two dense twins; a feature only the AuxK selection picked has not fired.

    The twins run with the gradient clip out of reach (max_grad_norm = 1e30: the coefficient is exactly 1).  The step's
    gradient-norm pass adds its per-workgroup partial sums with float atomics, so with the clip active the coefficient of
    IDENTICAL gradients can differ in its last bit from one run to the next, in either mode, and two dense runs that happen
    to agree would then hold the subset run to a difference the dense mode does not keep itself.  With the coefficient
    pinned, everything the step computes from the selections is fixed-order, and the comparison is exact."""
    from msae.train import SaeTrainStep

    sae0, x = auxk_model
    dead = _dead_mask(100, N2, dev, seed=12)
    calls = _capture(monkeypatch)

    def run(path):
        sae = copy.deepcopy(sae0)
        ts = SaeTrainStep(sae, lr=1e-3, auxk_alpha=1.0 / 32, dead_feature_threshold=0, auxk_path=path)
        ts.num_tokens_since_fired[dead] = 1
        ts.max_grad_norm = 1e30
        ts.step(x)
        return [p.detach().clone() for p in (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)], \
            ts.num_tokens_since_fired.clone()

    pa, ca = run("dense")
    pb, cb = run("dense")
    ps, cs = run("subset")
    for name, s, a, b in zip(("W_enc", "b_enc", "W_dec", "b_dec"), ps, pa, pb):
        _assert_within_run_to_run(name, s, a, b)
        assert not torch.equal(s, dict(zip(("W_enc", "b_enc", "W_dec", "b_dec"), (sae0.encoder.weight, sae0.encoder.bias,
                                                                                  sae0.W_dec, sae0.b_dec)))[name]), name
    assert torch.equal(ca, cb) and torch.equal(cs, ca)
    sel = calls[2]
    assert sel[1][0].shape[-1] == 100
    fired = torch.zeros(N2, dtype=torch.bool, device=dev)
    fired[sel[-1][1].reshape(-1)] = True
    aux_only = torch.zeros(N2, dtype=torch.bool, device=dev)
    aux_only[sel[1][1].reshape(-1)] = True
    aux_only &= ~fired
    assert int(aux_only.sum()) > 0, "the case must have dead features that only the AuxK selection picks"
    assert torch.equal(cs == 0, fired)
    assert bool((cs[aux_only] == 1 + T2).all())


# ---- no host synchronisation ---------------------------------------------------------------------------------------------
def test_subset_calls_do_not_synchronise(dev, auxk_model, monkeypatch):
    """ops.pre_acts_features, ops.topk_within, Sae.pre_acts(features=) and the subset forward under
    torch.cuda.set_sync_debug_mode("error"); the forward's one documented host read -- the length of the dead list
    (Sae._dead_list, in place of int(dead_mask.sum())) -- is let through, counted, and is the only one."""
    from msae import Sae, ops

    sae, x = auxk_model
    dead = _dead_mask(100, N2, dev)
    feats = torch.nonzero(dead).flatten().to(torch.int32)
    W, b, bd = sae.encoder.weight.detach(), sae.encoder.bias.detach(), sae.b_dec.detach()
    real, reads = Sae._dead_list, []

    def dead_list(mask):
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("default")
        try:
            reads.append(1)
            return real(mask)
        finally:
            torch.cuda.set_sync_debug_mode(prev)

    monkeypatch.setattr(Sae, "_dead_list", staticmethod(dead_list))
    with torch.no_grad():                                       # (library load, kernel attributes, workspaces)
        ops.topk_within(x, W, b, bd, feats, 100)
        sae.pre_acts(x, features=[3, 1, 2])
    sae(x, dead, auxk_path="subset")
    reads.clear()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                       # the control: the mode does raise on a host read
            torch.nonzero(dead)
        with torch.no_grad():
            a = ops.pre_acts_features(x, W, b, bd, feats)
            v, i = ops.topk_within(x, W, b, bd, feats, 100, max_ws_bytes=128 * 100 * 4)
            c = sae.pre_acts(x, features=[3, 1, 2])
        out = sae(x, dead, auxk_path="subset")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert reads == [1]
    assert a.shape == (T2, 100) and v.shape == (T2, 100) and i.shape == (T2, 100) and c.shape == (T2, 3)
    assert float(out.auxk_loss.detach()) > 0.0
