"""The Matryoshka kernels on the HIP path (include/msae.h, "nested decode") against the CPU restatement
tests/nested_ref.py: BIT FOR BIT where the contract defines bits (out, E, the combine, the grouped backward against the
plain backward kernels), inside derived bounds elsewhere (sq: recon_ref.bound; gradients: nested_ref.grad_bound).  The
autograd node, the composed expression and Sae.forward run under torch.cuda.set_sync_debug_mode("error") (of the AuxK
case the backward alone: its forward reads the dead list's length on the host, as documented)."""
import contextlib

import numpy as np
import pytest
import torch

import nested_ref as ref
import recon_ref
import synth

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


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


def _inputs(c, dev):
    bv, bi = torch.from_numpy(c.buf_vals).to(dev), torch.from_numpy(c.buf_idx).to(dev)
    v, i = bv[:, :c.k], bi[:, :c.k]
    assert v.is_contiguous() != c.view or c.T == 1
    ln = None if c.lengths is None else torch.from_numpy(c.lengths).to(dev)
    return (torch.from_numpy(c.x).to(dev, TDT[c.dtype]), v, i, torch.from_numpy(c.W_dec).to(dev), torch.from_numpy(c.b_dec).to(dev),
            c.bounds, ln)


def _eq(a, b) -> bool:
    """Bit equality of two f32 arrays."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- forward, on bits ------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_what_it_must():
    cs = ref.CASES
    assert {c.d for c in cs} == {4, 128, 1000, 1002, 1028} and {c.k for c in cs} >= {1, 8, 9, 65, 300}
    assert {c.T for c in cs} == {1, 37, 300} and {c.G for c in cs} == {1, 2, 5, 8} and ref.BOUNDS[8][0] == 1
    assert {c.kind for c in cs} == set(ref.KINDS) and {c.dtype for c in cs} == {"f32", "bf16", "f16"}
    assert {c.wide for c in cs} == {True, False} and {c.view for c in cs} == {True, False}
    assert sum(c.lengths is not None for c in cs) >= 3
    for d in (4, 128, 1000, 1002, 1028):
        assert {c.k for c in cs if c.d == d} >= {1, 8, 9, 65, 300}, d


@pytest.mark.parametrize("i", range(len(ref.CASES)), ids=lambda i: ref.CASES[i].id)
def test_forward_against_the_restatement(dev, i):
    from msae import ops

    c = ref.CASES[i]
    exp = ref.expected(i)
    args = _inputs(c, dev)
    out, sq, E = ops.nested_decode(*args, want_residuals=True)
    assert out.shape == (c.T, c.d) and sq.shape == (c.T, c.G) and E.shape == (c.G, c.T, c.d)
    assert _eq(out.cpu().numpy(), exp["out"]), c.id
    assert _eq(E.cpu().numpy(), exp["E"]), c.id
    got = sq.double().cpu().numpy()
    lim = recon_ref.bound(exp["sq_abs"], c.d)
    print(f"{c.id}: worst sq error / bound = {ref.worst(got, exp['sq'], lim):.3e}")
    assert ref.inside(got, exp["sq"], lim), c.id
    # without the residual planes: the same out and sq, bit for bit
    out2, sq2, E2 = ops.nested_decode(*args)
    assert E2 is None and torch.equal(out2, out) and torch.equal(sq2, sq)
    if c.G == 1 and c.lengths is None:
        assert torch.equal(out, ops.decode(args[2], args[1], args[3], args[4]))


def test_a_token_is_the_same_bits_alone_and_in_a_batch(dev):
    from msae import ops

    c = next(c for c in ref.CASES if c.T == 300 and c.G > 1)
    x, v, i, W, b, bounds, ln = _inputs(c, dev)
    out, sq, E = ops.nested_decode(x, v, i, W, b, bounds, ln, want_residuals=True)
    o1, s1, E1 = ops.nested_decode(x[41:42], v[41:42], i[41:42], W, b, bounds, None, want_residuals=True)
    assert torch.equal(o1, out[41:42]) and torch.equal(s1, sq[41:42]) and torch.equal(E1, E[:, 41:42])


def test_out_of_range_indices_set_status_and_are_skipped(dev):
    import ctypes

    from msae import _hip, ops

    c = next(c for c in ref.CASES if c.d == 128 and c.k == 8 and c.G == 5 and c.kind == "mixed" and c.lengths is None)
    x, v, i, W, b, bounds, _ = _inputs(c, dev)
    i = i.clone()
    i[3, 2], i[5, 0], i[7, 7] = ref.N, -1, 2 ** 31 - 1
    idx_np = i.cpu().numpy()
    exp = ref.forward(c.x, c.vals, idx_np, c.W_dec, c.b_dec, bounds)
    assert exp["flagged"]
    out, sq, E = ops.nested_decode(x, v, i, W, b, bounds, want_residuals=True)
    assert _eq(out.cpu().numpy(), exp["out"]) and _eq(E.cpu().numpy(), exp["E"])
    lib = _hip.load()
    for bad, want in ((i, 1), (_inputs(c, dev)[2], 0)):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        o = torch.empty(c.T, c.d, device=dev)
        s = torch.empty(c.T, c.G, device=dev)
        bh = (ctypes.c_int32 * c.G)(*bounds)
        fn = lib.msae_nested_decode_i64_f32 if bad.dtype == torch.int64 else lib.msae_nested_decode_f32
        bad = bad.contiguous()
        rc = fn(_hip.ptr(x), _hip.DTYPE_CODE[x.dtype], _hip.ptr(v.contiguous()), _hip.ptr(bad), c.k, None, bh, c.G, _hip.ptr(W),
                _hip.ptr(b), c.T, c.k, ref.N, c.d, _hip.ptr(o), None, _hip.ptr(s), _hip.ptr(status), _hip.stream_of(x))
        assert rc == 0 and int(status.item()) == want


def test_without_residuals_nothing_is_written_outside_out_and_sq(dev):
    """E = NULL: out and sq carved out of one guard-filled arena; every float around them keeps the guard's bits."""
    import ctypes

    from msae import _hip

    c = next(c for c in ref.CASES if c.d == 1002 and c.G == 5)
    x, v, i, W, b, bounds, _ = _inputs(c, dev)
    v, i = v.contiguous(), i.contiguous()
    n_out, n_sq, pad = c.T * c.d, c.T * c.G, 4096
    arena = torch.full((pad + n_out + pad + n_sq + pad,), -7.25, device=dev)
    o, s = arena[pad:pad + n_out], arena[2 * pad + n_out:2 * pad + n_out + n_sq]
    lib = _hip.load()
    fn = lib.msae_nested_decode_i64_f32 if i.dtype == torch.int64 else lib.msae_nested_decode_f32
    rc = fn(_hip.ptr(x), _hip.DTYPE_CODE[x.dtype], _hip.ptr(v), _hip.ptr(i), c.k, None, (ctypes.c_int32 * c.G)(*bounds), c.G, _hip.ptr(W),
            _hip.ptr(b), c.T, c.k, ref.N, c.d, _hip.ptr(o), None, _hip.ptr(s), None, _hip.stream_of(x))
    assert rc == 0
    exp = ref.expected(ref.CASES.index(c))
    assert _eq(o.view(c.T, c.d).cpu().numpy(), exp["out"])
    for lo, hi in ((0, pad), (pad + n_out, 2 * pad + n_out), (2 * pad + n_out + n_sq, arena.numel())):
        assert bool((arena[lo:hi] == -7.25).all())


# ---- combine, on bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,d", [(37, 1002), (300, 1002), (37, 1028), (1, 4)])       # T d % 4 != 0: the one-element path
@pytest.mark.parametrize("with_full", [True, False])
def test_combine_bits(dev, T, d, with_full):
    from msae import ops

    rng = np.random.default_rng([T, d])
    G = 5
    E = rng.standard_normal((G, T, d)).astype(np.float32)
    coef = (2 * rng.uniform(-1, 1, G)).astype(np.float32)
    gf = rng.standard_normal((T, d)).astype(np.float32) if with_full else None
    Et = torch.from_numpy(E).to(dev)
    S = ops.nested_combine_(Et, torch.from_numpy(coef).to(dev), None if gf is None else torch.from_numpy(gf).to(dev))
    assert S.data_ptr() == Et.data_ptr()
    assert _eq(S.cpu().numpy(), ref.combine_f32(E, coef, gf))


# ---- grouped backward, on bits, against the plain kernels ------------------------------------------------------------------
def _pair_counts_fixture(T=1100, k=32, seed=3):
    """Features 0 .. 5 with T (more than 1024), 1024, 65, 64, 1 and 0 pairs -- every way wgrad_accum_kernel holds a segment --
    when T = 1100 (min(T, .) otherwise); the rest spread over [6, N), 2 % of them with a zero activation."""
    rng = np.random.default_rng(seed)
    idx = np.stack([6 + rng.permutation(ref.N - 6)[:k] for _ in range(T)])
    vals = rng.uniform(0.05, 3.0, (T, k)).astype(np.float32)
    vals[rng.random((T, k)) < 0.02] = 0.0
    want = {f: min(T, n) for f, n in ((0, T), (1, 1024), (2, 65), (3, 64), (4, 1))}
    for f, n in want.items():
        rows = rng.permutation(T)[:n]
        idx[rows, f] = f
        vals[rows, f] = rng.uniform(0.05, 3.0, n).astype(np.float32)
    counts = np.bincount(idx[vals != 0], minlength=ref.N)
    assert counts[5] == 0 and all(counts[f] == n for f, n in want.items())
    return idx.astype(np.int32), vals


@pytest.mark.parametrize("d,T", [(128, 1100), (1002, 37)])
def test_grouped_backward_equals_the_plain_kernels_plane_by_plane(dev, d, T):
    from msae import ops

    G, bounds = 5, ref.BOUNDS[5]
    idx, vals = _pair_counts_fixture(T)
    k = idx.shape[1]
    rng = np.random.default_rng([d, T])
    W = torch.from_numpy((rng.standard_normal((ref.N, d)) / np.sqrt(d)).astype(np.float32)).to(dev)
    S = torch.from_numpy(rng.standard_normal((G, T, d)).astype(np.float32)).to(dev)
    it, vt = torch.from_numpy(idx).to(dev), torch.from_numpy(vals).to(dev)

    def run(fn):
        prev, ops._WGRAD_ROWSUM = ops._WGRAD_ROWSUM, []
        try:
            with ops.collect_wgrad_sumsq() as rec:
                ga, gw = fn()
            return ga, gw, rec[W.data_ptr()][2], ops._WGRAD_ROWSUM[0]
        finally:
            ops._WGRAD_ROWSUM = prev

    ga, gw, rowsq, rowsum = run(lambda: ops.nested_decode_bwd(it, vt, W, S, bounds, True, True))
    grp_pair = torch.bucketize(it.long(), torch.tensor(bounds, device=dev), right=True)
    grp_row = torch.bucketize(torch.arange(ref.N, device=dev), torch.tensor(bounds, device=dev), right=True)
    assert set(grp_row.unique().tolist()) == set(range(G))
    for g in range(G):
        pa, pw, psq, psum = run(lambda: ops.decode_bwd(it, vt, W, S[g].contiguous(), True, True))
        assert torch.equal(ga[grp_pair == g], pa[grp_pair == g]), g
        rows = grp_row == g
        assert torch.equal(gw[rows], pw[rows]) and torch.equal(rowsq[rows], psq[rows]) and torch.equal(rowsum[rows], psum[rows]), g
    assert bool((gw[5] == 0).all()) and float(rowsq[5]) == 0.0
    # one plane: the grouped entry points are the plain ones
    g1a, g1w, _, _ = run(lambda: ops.nested_decode_bwd(it, vt, W, S[:1].contiguous(), (ref.N,), True, True))
    pa, pw, _, _ = run(lambda: ops.decode_bwd(it, vt, W, S[0].contiguous(), True, True))
    assert torch.equal(g1a, pa) and torch.equal(g1w, pw)


# ---- the autograd node against the composed expression and the float64 restatement -------------------------------------------
NODE = dict(T=300, d=128, k=32, G=5)


def _node_case(lengths: bool, seed=11):
    T, d, k, G = NODE["T"], NODE["d"], NODE["k"], NODE["G"]
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((ref.N, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.5 * rng.standard_normal(d)).astype(np.float32)
    vals = -np.sort(-rng.uniform(0.05, 3.0, (T, k)).astype(np.float32), axis=1)
    idx = np.stack([rng.permutation(ref.N)[:k] for _ in range(T)]).astype(np.int64)
    ln = None
    if lengths:
        ln = rng.integers(0, k + 1, T).astype(np.int32)
        vals[np.arange(k)[None] >= ln[:, None]] = 0.0          # a filtered list: +0.0 behind the kept prefix
    x = rng.standard_normal((T, d)).astype(np.float32)
    gf = (rng.standard_normal((T, d)) / T).astype(np.float32)
    w = rng.uniform(0.1, 1.0, G).astype(np.float32)
    return dict(W_dec=W, b_dec=b, vals=vals, idx=idx, lengths=ln, x=x, grad_full=gf, w=w, bounds=ref.BOUNDS[G], T=T, d=d, k=k)


def _run_node(c, dev, fused: bool, with_full: bool):
    from msae import ops

    x = torch.from_numpy(c["x"]).to(dev)
    v = torch.from_numpy(c["vals"]).to(dev).requires_grad_()
    i = torch.from_numpy(c["idx"]).to(dev)
    W = torch.from_numpy(c["W_dec"]).to(dev).requires_grad_()
    b = torch.from_numpy(c["b_dec"]).to(dev).requires_grad_()
    ln = None if c["lengths"] is None else torch.from_numpy(c["lengths"]).to(dev)
    w, gf = torch.from_numpy(c["w"]).to(dev), torch.from_numpy(c["grad_full"]).to(dev)
    torch.cuda.synchronize()
    with no_sync():
        if fused:
            out, sq_sum = ops.nested_reconstruct(x, v, i, W, b, c["bounds"], ln)
            assert type(out.grad_fn).__name__.startswith("_NestedReconstruct")
        else:
            out, sq = ops.nested_composed(x, v, i, W, b, c["bounds"], ln)[:2]
            sq_sum = sq.sum(0)
        loss = (sq_sum * w).sum() + ((out * gf).sum() if with_full else 0.0)
        loss.backward()
    return out.detach(), sq_sum.detach(), v.grad, W.grad, b.grad


@pytest.mark.parametrize("lengths", [False, True], ids=["topk", "lengths"])
@pytest.mark.parametrize("with_full", [False, True], ids=["sq_only", "with_grad_full"])
def test_node_against_the_composed_expression_and_float64(dev, lengths, with_full):
    c = _node_case(lengths)
    G, d = len(c["bounds"]), c["d"]
    f_out, f_sq, f_ga, f_gw, f_gb = _run_node(c, dev, True, with_full)
    c_out, c_sq, c_ga, c_gw, c_gb = _run_node(c, dev, False, with_full)
    assert torch.equal(f_out, c_out), "sae_out must match the composed expression on bits"
    fwd = ref.forward(c["x"], c["vals"], c["idx"], c["W_dec"], c["b_dec"], c["bounds"], c["lengths"])
    assert _eq(f_out.cpu().numpy(), fwd["out"])
    S, S_abs = ref.combine(fwd["E"], 2.0 * c["w"].astype(np.float64), c["grad_full"] if with_full else None)
    exp = ref.backward(c["vals"], c["idx"], c["W_dec"], c["bounds"], S, S_abs, c["lengths"])
    pairs = np.bincount(c["idx"][c["vals"] != 0], minlength=ref.N).max()
    assert pairs <= d and np.log2(c["T"]) + 2 <= d                  # the depth the bound's derivation assumes
    for name, fused, comp in (("g_acts", f_ga, c_ga), ("g_W", f_gw, c_gw), ("g_b", f_gb, c_gb)):
        lim = ref.grad_bound(exp[name + "_abs"], d, G)
        for who, got in (("fused", fused), ("composed", comp)):
            got = got.double().cpu().numpy()
            print(f"{name} {who}: worst error / bound = {ref.worst(got, exp[name], lim):.3e}")
            assert ref.inside(got, exp[name], lim), (name, who)
    # power: the wrong combines are outside the bound
    for variant in ref.VARIANTS_BWD:
        if variant == "grad_full_last_only" and not with_full:
            continue
        Sv, _ = ref.combine(fwd["E"], 2.0 * c["w"].astype(np.float64), c["grad_full"] if with_full else None, variant=variant)
        wrong = ref.backward(c["vals"], c["idx"], c["W_dec"], c["bounds"], Sv, S_abs, c["lengths"])
        assert not ref.inside(f_ga.double().cpu().numpy(), wrong["g_acts"], ref.grad_bound(exp["g_acts_abs"], d, G)), variant


def test_node_is_replaced_by_the_composed_expression_where_it_must(dev):
    from msae import ops

    c = _node_case(False)
    x = torch.from_numpy(c["x"]).to(dev)
    v = torch.from_numpy(c["vals"]).to(dev).requires_grad_()
    i, W, b = (torch.from_numpy(c[n]).to(dev) for n in ("idx", "W_dec", "b_dec"))
    for xx in (x.clone().requires_grad_(), x.to(torch.bfloat16)):
        out, sq_sum = ops.nested_reconstruct(xx, v, i, W, b, c["bounds"])
        assert not type(out.grad_fn).__name__.startswith("_NestedReconstruct")
    xg = x.clone().requires_grad_()
    out, sq_sum = ops.nested_reconstruct(xg, v, i, W, b, c["bounds"])
    sq_sum.sum().backward()
    assert xg.grad is not None and bool(xg.grad.abs().sum() > 0)
    with torch.no_grad():                                              # no gradient needed: no residual planes kept
        out2, sq2 = ops.nested_reconstruct(x, v, i, W, b, c["bounds"])
    assert torch.equal(out2, out.detach()) and out2.grad_fn is None


# ---- Sae.forward: the fused node against the composed expression, encoder included ----------------------------------------------
def _sae(dev, activation, seed=21):
    from msae import Sae, SaeConfig

    d, N, k = NODE["d"], ref.N, NODE["k"]
    kw = dict(activation="batchtopk", batch_cap=64) if activation == "batchtopk" else {}
    sae = Sae(d, SaeConfig(num_latents=N, k=k, normalize_decoder=False, matryoshka=list(ref.BOUNDS[5]),
                           matryoshka_weights=[0.3, 0.25, 0.2, 0.15, 0.1], **kw), device=dev)
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, N, seed=seed)
    with torch.no_grad():
        for p, a in ((sae.encoder.weight, W_enc), (sae.encoder.bias, b_enc), (sae.W_dec, W_dec), (sae.b_dec, b_dec)):
            p.copy_(torch.from_numpy(a))
    return sae


@contextlib.contextmanager
def composed_node():
    """ops.nested_reconstruct replaced by the composed expression under ordinary autograd."""
    from msae import ops

    real = ops.nested_reconstruct

    def composed(x, top_acts, top_indices, W_dec, b_dec, bounds, lengths=None):
        out, sq, _ = ops.nested_composed(x, top_acts, top_indices, W_dec, b_dec, tuple(bounds), lengths)
        return out, sq.sum(0)

    ops.nested_reconstruct = composed
    try:
        yield
    finally:
        ops.nested_reconstruct = real


def _forward_backward(sae, x, dead_mask=None, auxk_alpha=0.0, scale=1.0, zero=True):
    """One forward + backward of (nested_loss + alpha auxk_loss) * scale -> (out, {"grad_full": the gradient that reached
    sae_out, "g_acts": the one that left towards latent_acts, "aux": the AuxK selection (acts, indices) or None}).  Under "no
    host sync"; with a dead mask the FORWARD runs outside it (Sae._dead_list sizes its result on the host: the forward's one
    documented read) and the backward inside."""
    from msae import ops

    grabbed = {"aux": None}
    if zero:
        for p in sae.parameters():
            p.grad = None
    real = ops.sparse_encode

    def spy(*a, **kw):
        sel = real(*a, **kw)
        if dead_mask is not None and len(sel) > 1:
            grabbed["aux"] = (sel[1][0].detach(), sel[1][1].detach())
        return sel

    ops.sparse_encode = spy
    try:
        torch.cuda.synchronize()
        with (no_sync() if dead_mask is None else contextlib.nullcontext()):
            out = sae(x, dead_mask, auxk_path="subset") if dead_mask is not None else sae(x)
    finally:
        ops.sparse_encode = real
    out.sae_out.register_hook(lambda g: grabbed.__setitem__("grad_full", g.detach().clone()))
    out.latent_acts.register_hook(lambda g: grabbed.__setitem__("g_acts", g.detach().clone()))
    loss = (out.nested_loss + auxk_alpha * out.auxk_loss) * scale
    with no_sync():
        loss.backward()
    return out, grabbed


def _grads(sae):
    return {n: p.grad.detach().clone() for n, p in sae.named_parameters()}


def _restate(sae, x, out, hook, scale=1.0):
    """The float64 restatement of EVERY parameter's gradient for one forward of `sae` on x -> (exp: the node's own float64
    gradients, lim_a: the bound of g_acts, {parameter: (float64 gradient, elementwise bound)}).

    The node: nested_ref.backward from what reached it -- coef = 2 * weight / total_variance * scale as the device forms it
    (from the f32 total variance of the forward; those two roundings sit inside d + G + 2 with the reduction depth to spare)
    and grad_full as captured.  AuxK (hook["aux"]): with q = -grad_full the gradient of the AuxK decode's output (e_hat and
    sae_out - x enter the AuxK loss with opposite signs; q is taken as the f32 data it is), that decode adds sum_pairs v q[t]
    to W_dec, sum_t q[t] to b_dec and latent gradients q[t] . W_dec[i] to the encoder.  The encoder: nested_ref.
    encoder_backward over the main list and the AuxK list side by side.  Bounds, all single-sided against float64:
    gamma_{d+G+2} sum |term| for W_dec (with AuxK: G + 2 + the longest pair chain of a feature + 1 where that exceeds d),
    nested_ref.encoder_depths for the encoder's three."""
    d, G, bounds = NODE["d"], 5, ref.BOUNDS[5]
    T = x.shape[0]
    vals, idx = out.latent_acts.detach().cpu().numpy(), out.latent_indices.cpu().numpy()
    ln = None if out.lengths is None else out.lengths.cpu().numpy()
    W, b = sae.W_dec.detach().cpu().numpy(), sae.b_dec.detach().cpu().numpy()
    W_enc = sae.encoder.weight.detach().cpu().numpy()
    xn = x.cpu().numpy()
    fwd = ref.forward(xn, vals, idx, W, b, bounds, ln)
    assert _eq(out.sae_out.detach().cpu().numpy(), fwd["out"])
    tv32 = float(torch.var(x, dim=0, correction=0).sum() * T)
    coef = 2.0 * np.asarray(sae.cfg.nested_weights) / tv32 * scale
    gf = hook.get("grad_full")
    gf = None if gf is None else gf.double().cpu().numpy()
    S, S_abs = ref.combine(fwd["E"], coef, gf)
    exp = ref.backward(vals, idx, W, bounds, S, S_abs, ln)
    lim_a = ref.grad_bound(exp["g_acts_abs"], d, G)
    g_W, g_W_abs, g_b, g_b_abs = exp["g_W"].copy(), exp["g_W_abs"].copy(), exp["g_b"].copy(), exp["g_b_abs"].copy()
    e_idx, e_acts, e_g, e_gabs = idx, vals, exp["g_acts"], exp["g_acts_abs"]
    if ln is not None:                                          # the slots behind a row's length carry no gradient
        keep = np.arange(vals.shape[1])[None] < ln[:, None]
        e_acts = np.where(keep, vals, np.float32(0.0))
    pairs_dec = int(np.bincount(idx[vals != 0], minlength=ref.N).max())
    if hook.get("aux") is not None:
        av, ai = (t.cpu().numpy() for t in hook["aux"])
        q, W64 = -gf, W.astype(np.float64)
        flat = ai.reshape(-1).astype(np.int64)
        np.add.at(g_W, flat, (av.astype(np.float64)[:, :, None] * q[:, None, :]).reshape(-1, d))
        np.add.at(g_W_abs, flat, (np.abs(av.astype(np.float64))[:, :, None] * np.abs(q)[:, None, :]).reshape(-1, d))
        g_b, g_b_abs = g_b + q.sum(0), g_b_abs + np.abs(q).sum(0)
        e_idx, e_acts = np.concatenate([idx, ai], 1), np.concatenate([e_acts, av], 1)
        e_g = np.concatenate([e_g, np.einsum("td,tjd->tj", q, W64[ai])], 1)
        e_gabs = np.concatenate([e_gabs, np.einsum("td,tjd->tj", np.abs(q), np.abs(W64[ai]))], 1)
        pairs_dec = int(np.bincount(np.concatenate([idx[vals != 0], ai[av != 0]]), minlength=ref.N).max())
    # gamma_{d+G+2} has room for a chain over at most d of a feature's pairs; where AuxK piles more of them on one dead
    # feature (and adds its share to the node's: + 1) the chain's own length takes d's place -- the depth that does hold
    depth_W = G + 2 + max(d, pairs_dec + 1)
    assert np.log2(T) + 2 <= d and (hook.get("aux") is not None or depth_W == d + G + 2)
    enc = ref.encoder_backward(e_idx, e_acts, e_g, e_gabs, xn, b, W_enc)
    depth = ref.encoder_depths(d, G, enc["pairs"], ref.N)
    params = {
        "W_dec": (g_W, ref.grad_bound(g_W_abs, d, G, depth_W)),
        "encoder.weight": (enc["g_W_enc"], ref.grad_bound(enc["g_W_enc_abs"], d, G, depth["g_W_enc"])),
        "encoder.bias": (enc["g_b_enc"], ref.grad_bound(enc["g_b_enc_abs"], d, G, depth["g_b_enc"])),
        "b_dec": (g_b + enc["g_bd"], ref.grad_bound(g_b_abs + enc["g_bd_abs"], d, G, depth["b_dec"])),
    }
    return exp, lim_a, params


@pytest.mark.parametrize("mode", ["topk", "batchtopk", "auxk"])
def test_sae_forward_fused_against_composed(dev, mode):
    """Every gradient of Sae.forward, on the fused node and on the composed expression, single-sided against float64: g_acts
    and W_dec inside gamma_{d+G+2} sum |term|, the encoder's three inside the depth nested_ref.encoder_depths derives (the
    encoder backward reduces a second time, over a feature's pairs)."""
    sae = _sae(dev, "batchtopk" if mode == "batchtopk" else "topk")
    T, d, G = NODE["T"], NODE["d"], 5
    x = torch.from_numpy(synth.activations(T, d, seed=23, bf16=False)).to(dev)
    dead, alpha = None, 0.0
    if mode == "auxk":
        dead = torch.zeros(ref.N, dtype=torch.bool, device=dev)
        dead[torch.arange(1, ref.N, 2, device=dev)] = True     # (1024 dead features: a feature's AuxK and main pairs stay below d)
        alpha = 1 / 32
    f_out, f_hook = _forward_backward(sae, x, dead, alpha)
    f_g = _grads(sae)
    with composed_node():
        c_out, c_hook = _forward_backward(sae, x, dead, alpha)
    c_g = _grads(sae)
    assert type(f_out).__name__ == "NestedForwardOutput" and f_out.bounds == ref.BOUNDS[5]
    assert torch.equal(f_out.sae_out, c_out.sae_out) and torch.equal(f_out.latent_indices, c_out.latent_indices)
    assert torch.equal(f_out.latent_acts, c_out.latent_acts) and torch.equal(f_out.auxk_loss, c_out.auxk_loss)
    assert f_out.nested_fvu.shape == (G,) and torch.equal(f_out.fvu, f_out.nested_fvu[-1])
    # sq_sum: a sum of T d squares on either side, each within gamma_{T + d} of the exact sum of the same f32 residuals
    assert torch.allclose(f_out.nested_fvu, c_out.nested_fvu, rtol=2 * ref.gamma(T + d), atol=0)
    if mode == "batchtopk":
        assert f_out.lengths is not None and f_out.theta is not None and f_out.n_saturated is not None
        assert int(f_out.lengths.min()) < int(f_out.lengths.max())
    if mode == "auxk":
        assert bool(f_out.auxk_loss > 0) and bool(f_hook["grad_full"].abs().sum() > 0) and f_hook["aux"] is not None
        assert torch.equal(f_hook["grad_full"], c_hook["grad_full"])
    else:
        assert "grad_full" not in f_hook                       # nothing but the squared errors feeds the node
    exp, lim_a, params = _restate(sae, x, f_out, f_hook)
    for who, hook, grads in (("fused", f_hook, f_g), ("composed", c_hook, c_g)):
        got = hook["g_acts"].double().cpu().numpy()
        print(f"{mode} g_acts {who}: worst error / bound = {ref.worst(got, exp['g_acts'], lim_a):.3e}")
        assert ref.inside(got, exp["g_acts"], lim_a), who
        for name, (want, lim) in params.items():
            got = grads[name].double().cpu().numpy()
            print(f"{mode} {name} {who}: worst error / bound = {ref.worst(got, want, lim):.3e}")
            assert ref.inside(got, want, lim), (name, who)
            assert np.abs(got).sum() > 0


# ---- training --------------------------------------------------------------------------------------------------------------
def _adam_interval(W, G, dG, M, V, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """Elementwise bound on |W'(G1) - W'(G2)| of one Adam step (train_ref.adam_rows' formulas, no clipping: the test lifts
    max_grad_norm) for any two gradients inside G +- dG, by interval arithmetic: the numerator m' is increasing in g, the
    denominator depends on g^2 alone."""
    import train_ref as tr

    W, G, dG, M, V = (torch.as_tensor(t, dtype=torch.float64) for t in (W, G, dG, M, V))
    b1, b2, lr_, eps_ = tr.f32(betas[0]), tr.f32(betas[1]), tr.f32(lr), tr.f32(eps)
    bc1, bc2 = 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5
    m_lo, m_hi = M + (G - dG - M) * (1 - b1), M + (G + dG - M) * (1 - b1)
    g2_lo = torch.clamp(G.abs() - dG, min=0.0) ** 2
    g2_hi = (G.abs() + dG) ** 2
    den_lo = torch.sqrt(b2 * V + (1 - b2) * g2_lo) / bc2 + eps_
    den_hi = torch.sqrt(b2 * V + (1 - b2) * g2_hi) / bc2 + eps_
    cands = torch.stack([m_lo / den_lo, m_lo / den_hi, m_hi / den_lo, m_hi / den_hi])
    return lr_ / bc1 * (cands.max(0).values - cands.min(0).values)


def test_three_training_steps_fused_against_composed(dev):
    """Three SaeTrainStep steps, two uneven micro-chunks each, the fused node against the composed expression IN LOCK STEP: before
    every step the fused trainer takes over the composed trainer's parameters and moments, so each step starts from one
    state and the bound is that of ONE Adam step.  Both trainers' gradients lie within the single-sided float64 bounds of
    _restate (summed over the chunks, + u |G| for the f32 accumulation) of the FLOAT64 gradient G; the parameters may differ
    by the width of the Adam update over G +- that bound, plus train_ref.adam_rows' rounding bound of the pass on each side.
    Clipping is lifted (max_grad_norm = 1e9) so that the update is elementwise."""
    import train_ref
    from msae.train import SaeTrainStep

    T, lr = 301, 1e-3                                           # 151 + 150
    x = torch.from_numpy(synth.activations(T, NODE["d"], seed=29, bf16=False)).to(dev)
    trainers = {}
    for who in ("fused", "composed"):
        sae = _sae(dev, "topk", seed=31)
        trainers[who] = SaeTrainStep(sae, lr=lr, micro_acc_steps=2, fuse_next_step=False)
        trainers[who].max_grad_norm = 1e9
    tf, tc = trainers["fused"], trainers["composed"]
    for step in (1, 2, 3):
        with torch.no_grad():                                   # lock step
            for pf, pc in zip(tf.params, tc.params):
                pf.copy_(pc)
            for mf, mc in zip(tf.exp_avg + tf.exp_avg_sq, tc.exp_avg + tc.exp_avg_sq):
                mf.copy_(mc)
        before = {n: p.detach().clone() for n, p in tc.sae.named_parameters()}
        moments = {n: (m.clone(), v.clone()) for (n, _), m, v in zip(tc.sae.named_parameters(), tc.exp_avg, tc.exp_avg_sq)}
        # the float64 gradient of this step and its bound, from the state both sides start from: one restated forward per chunk
        G64, dG64 = {}, {}
        for chunk in x.chunk(2):
            out, hook = _forward_backward(tc.sae, chunk, scale=0.5)
            _, _, params = _restate(tc.sae, chunk, out, hook, scale=0.5)
            for n, (want, lim) in params.items():
                G64[n] = G64.get(n, 0.0) + want
                dG64[n] = dG64.get(n, 0.0) + lim
        for p in tc.params:
            p.grad = None
        rf = tf.step(x)
        with composed_node():
            rc = tc.step(x)
        assert rf["stepped"] and rc["stepped"] and rf["nested_fvu"].shape == (5,)
        assert torch.allclose(rf["nested_fvu"], rc["nested_fvu"], rtol=2 * ref.gamma(T + NODE["d"])) and torch.allclose(rf["fvu"], rf["nested_fvu"][-1])
        for (n, pf), (_, pc) in zip(tf.sae.named_parameters(), tc.sae.named_parameters()):
            G = torch.from_numpy(np.asarray(G64[n])).reshape(pc.shape)
            dG = torch.from_numpy(np.asarray(dG64[n])).reshape(pc.shape) + ref.U * G.abs()
            M, V = (t.double().cpu() for t in moments[n])
            W = before[n].double().cpu()
            spread = _adam_interval(W, G, dG, M, V, step, lr)
            _, (dw, _, _) = train_ref.adam_rows(before[n].cpu(), G.float(), M.float(), V.float(), step, lr, total_sumsq=None)
            lim = spread + 2 * dw.reshape(spread.shape)
            err = (pf.detach().double().cpu() - pc.detach().double().cpu()).abs()
            moved = float((pc.detach().cpu() - before[n].cpu()).abs().max())
            print(f"step {step} {n}: worst |fused - composed| / bound = {float((err / lim.clamp(min=1e-300)).max()):.3e}; moved {moved:.3e}")
            assert bool((err <= lim).all()), (step, n)
            assert moved > 0.5 * lr, f"{n} did not move"


# ---- Sae.nested_error and Sae.truncate on the device ---------------------------------------------------------------------------
def test_nested_error_and_truncate(dev):
    from msae import ops

    sae = _sae(dev, "topk")
    x = torch.from_numpy(synth.activations(37, NODE["d"], seed=5)).to(dev, torch.bfloat16)
    with torch.no_grad(), no_sync():
        ne = sae.nested_error(x)
        top = sae.encode(x)
        _, sq, _ = ops.nested_decode(x, top.top_acts, top.top_indices, sae.W_dec, sae.b_dec, sae.cfg.matryoshka)
        ne2 = sae.nested_error(x, [1024, ref.N], top=top)
    assert ne.bounds == ref.BOUNDS[5] and torch.equal(ne.err2, sq) and ne.fvu.shape == (5,) and ne.fvu.dtype == torch.float64
    # other bounds are another chain order, hence other bits than `ne`: held to the op with the same bounds, on bits
    with torch.no_grad():
        _, sq2, _ = ops.nested_decode(x, top.top_acts, top.top_indices, sae.W_dec, sae.b_dec, [1024, ref.N])
    assert ne2.bounds == (1024, ref.N) and torch.equal(ne2.err2, sq2)
    # the full prefix agrees with recon_error's last checkpoint, bit for bit (the same chain order when the list is one group)
    one = sae.nested_error(x, [ref.N], top=top)
    rc = sae.recon_error(x, [sae.cfg.k], top=top)
    assert torch.equal(one.err2[:, 0], rc.err2[:, 0])
    # truncate: a working Sae over the first 512 features, sharing storage; it re-selects among them
    t = sae.truncate(512)
    assert t.W_dec.data_ptr() == sae.W_dec.data_ptr() and t.cfg.matryoshka == [128, 256, 512]
    from oracle import oracle
    with torch.no_grad():
        tt = t.encode(x)
        full = sae.encode(x, exact=True)
    assert int(tt.top_indices.max()) < 512
    # exactly the project's oracle encode over the first 512 rows (the contract smoke() holds the encoder to)
    ref_v, ref_i = oracle.encode_topk(x.float().cpu().numpy(), sae.encoder.weight.detach()[:512].cpu().numpy(),
                                      sae.encoder.bias.detach()[:512].cpu().numpy(), sae.b_dec.detach().cpu().numpy(), sae.cfg.k)
    assert np.array_equal(tt.top_indices.cpu().numpy(), ref_i) and np.array_equal(tt.top_acts.cpu().numpy(), ref_v)
    assert not torch.equal(tt.top_indices, full.top_indices)
    out = t(x.float())
    assert out.nested_fvu.shape == (3,)
