"""Reconstruction error against sparsity on the HIP path (ops.recon_curve, Sae.recon_error, ReconStats, the cache loop)
against the CPU restatement tests/recon_ref.py within the bound derived there, and BIT FOR BIT where the contract
(include/msae.h, "reconstruction error against sparsity") defines bits.  Fixtures and their power: tests/recon_ref.py,
tests/test_recon_host.py.  The device calls of the statistics run under torch.cuda.set_sync_debug_mode("error")."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

import fakes
import recon_ref as ref
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


def _x_on(c, dev):
    x = torch.from_numpy(c.x).to(dev, TDT[c.dtype])
    if not c.offset:
        return x
    buf = torch.empty(c.T * c.d + 1, dtype=x.dtype, device=dev)
    out = buf[1:].view(c.T, c.d)
    out.copy_(x)
    assert out.is_contiguous() and out.data_ptr() % (4 * out.element_size()) != 0
    return out


def _inputs(c, dev):
    bv, bi = torch.from_numpy(c.buf_vals).to(dev), torch.from_numpy(c.buf_idx).to(dev)
    v, i = bv[:, :c.k], bi[:, :c.k]
    assert v.is_contiguous() != c.view or c.T == 1
    return _x_on(c, dev), v, i, torch.from_numpy(c.W_dec).to(dev), torch.from_numpy(c.b_dec).to(dev)


def _assert_inside(mom, xx, exp, d, what):
    e_mom, e_xx, e_mom_abs, e_xx_abs, _ = exp
    got_m, got_x = mom.double().cpu().numpy(), xx.double().cpu().numpy()
    err, lim = np.abs(got_m - e_mom), ref.bound(e_mom_abs, d)
    print(f"{what}: worst moment error / bound = {np.nanmax(err / lim):.3e}; xx {np.max(np.abs(got_x - e_xx) / ref.bound(e_xx_abs, d)):.3e}")
    assert not ref.outside(got_m, e_mom, e_mom_abs, d).any(), what
    assert (np.abs(got_x - e_xx) <= ref.bound(e_xx_abs, d)).all(), what


# ---- the op against the restatement ----------------------------------------------------------------------------------------
def test_the_case_list_covers_what_it_must():
    cs = ref.CASES
    assert {c.d for c in cs} >= set(ref.EDGE_D) and {c.k for c in cs} == {1, 4, 32, 256} and {c.T for c in cs} == {1, 5, 300}
    for d in ref.EDGE_D:
        assert {c.dtype for c in cs if c.d == d} == set(ref.DTYPES), d
    assert {c.wide for c in cs} == {True, False} and {c.view for c in cs} == {True, False} and any(c.offset for c in cs)
    kinds = {tuple(c.ks) for c in cs}
    assert (0,) in kinds and (0, 1, 32) in kinds and tuple(range(16)) in kinds and (1, 2, 4, 8, 16, 32) in kinds
    assert any(c.ks == [c.k] for c in cs)


@pytest.mark.parametrize("i", range(len(ref.CASES)), ids=lambda i: ref.CASES[i].id)
def test_op_against_the_restatement(dev, i):
    from msae import ops

    c = ref.CASES[i]
    mom, xx = ops.recon_curve(*_inputs(c, dev), c.ks)
    assert mom.shape == (c.T, len(c.ks), 3) and xx.shape == (c.T,) and mom.dtype == xx.dtype == torch.float32
    _assert_inside(mom, xx, ref.expected(i), c.d, c.id)


# ---- bit-level structure ---------------------------------------------------------------------------------------------------
STRUCT = [i for i, c in enumerate(ref.CASES) if c.T == 300 and len(c.ks) > 1][:4] + \
         [i for i, c in enumerate(ref.CASES) if c.offset and c.T == 300][:1]


@pytest.mark.parametrize("i", STRUCT, ids=lambda i: ref.CASES[i].id)
def test_prefix_token_and_repeat_bits(dev, i):
    """A checkpoint is the same call with k = kappa on the truncated list; token t of the batch is the T = 1 call on row t;
    two calls give the same bits."""
    from msae import ops

    c = ref.CASES[i]
    x, v, idx, W, b = _inputs(c, dev)
    mom, xx = ops.recon_curve(x, v, idx, W, b, c.ks)
    again = ops.recon_curve(x, v, idx, W, b, c.ks)
    assert torch.equal(mom, again[0]) and torch.equal(xx, again[1])
    for ci, kappa in enumerate(c.ks):
        if kappa == 0:
            continue
        m1, x1 = ops.recon_curve(x, v[:, :kappa].contiguous(), idx[:, :kappa].contiguous(), W, b, [kappa])
        assert torch.equal(m1[:, 0], mom[:, ci]) and torch.equal(x1, xx), kappa
    for t in (0, 137, c.T - 1):
        assert (x[t:t + 1].data_ptr() % (4 * x.element_size()) != 0) == c.offset     # the batch's own load path
        mt, xt = ops.recon_curve(x[t:t + 1], v[t:t + 1], idx[t:t + 1], W, b, c.ks)
        assert torch.equal(mt[0], mom[t]) and torch.equal(xt[0], xx[t]), t


def test_recon_error_does_not_depend_on_the_chunking(dev):
    from msae import Sae, SaeConfig

    c = ref.CASES[[c.id for c in ref.CASES].index("d4096-k32-T300-pow2-bf16-i64")]
    x, v, idx, W, b = _inputs(c, dev)
    sae = Sae(c.d, SaeConfig(num_latents=ref.N, k=c.k), device=dev)
    with torch.no_grad():
        sae.W_dec.copy_(W)
        sae.b_dec.copy_(b)
    whole = sae.recon_error(x.view(3, 100, c.d), top=(v.view(3, 100, c.k), idx.view(3, 100, c.k)))
    assert whole.ks == (1, 2, 4, 8, 16, 32) and whole.err2.shape == (3, 100, 6) and whole.xnorm2.shape == (3, 100)
    for chunk in (1, 7, 299, 300, 1000):
        part = sae.recon_error(x, top=(v, idx), chunk=chunk)
        for name in ("err2", "dot", "rnorm2", "xnorm2"):
            assert torch.equal(getattr(part, name).reshape(-1), getattr(whole, name).reshape(-1)), (chunk, name)
        assert torch.equal(part.total_variance, whole.total_variance)
    _assert_inside(torch.stack([whole.err2, whole.dot, whole.rnorm2], -1).view(300, 6, 3), whole.xnorm2.view(300),
                   ref.expected(ref.CASES.index(c)), c.d, "recon_error")


# ---- hostile lists -----------------------------------------------------------------------------------------------------------
def test_hostile_lists(dev):
    """+0 / -0 values (in front of a non-finite decoder row), a repeated feature, features N, -1 and 2^31 - 1: skipped, flagged
    exactly as ops.decode flags them, no fault; a non-finite x row poisons its own token alone."""
    from msae import ops

    h = ref.hostile_case()
    on = {n: torch.from_numpy(h[n]).to(dev) for n in ("x", "vals", "idx", "W_dec", "b_dec")}
    exp = ref.moments(h["x"], h["vals"], h["idx"], h["W_dec"], h["b_dec"], h["ks"], ref.N)
    assert exp[4]
    for idx in (on["idx"], on["idx"].to(torch.int32)):
        mom, xx = ops.recon_curve(on["x"], on["vals"], idx, on["W_dec"], on["b_dec"], h["ks"])
        got = mom.double().cpu().numpy()
        assert not np.isfinite(got[5][:, :2]).any() and np.isinf(float(xx[5]))      # (|r|^2 does not see x)
        assert np.isfinite(got[5][:, 2]).all() and np.isfinite(np.delete(got, 5, 0)).all()
        keep = np.arange(h["T"]) != 5
        assert not ref.outside(got[keep], exp[0][keep], exp[2][keep], h["d"]).any()
        clean = on["x"].clone()
        clean[5] = 0
        m2, x2 = ops.recon_curve(clean, on["vals"], idx, on["W_dec"], on["b_dec"], h["ks"])
        kt = torch.from_numpy(keep).to(dev)
        assert torch.equal(m2[kt], mom[kt]) and torch.equal(x2[kt], xx[kt]) and torch.equal(m2[5, :, 2], mom[5, :, 2])
        # the decoder agrees bit for bit about what a hostile list reconstructs: kappa = 8 is the whole list
        r = ops.decode(idx, on["vals"], on["W_dec"], on["b_dec"])
        ed, xd, rd = (r - clean).double(), clean.double(), r.double()
        for m, term in enumerate((ed * ed, xd * rd, rd * rd)):
            s64 = term.sum(1).cpu().numpy()
            a64 = term.abs().sum(1).cpu().numpy()
            assert (np.abs(m2[:, -1, m].double().cpu().numpy() - s64) <= ref.bound(a64, h["d"])).all(), m
    ops.set_debug_bounds(True)
    try:
        good = slice(0, 3)                                  # tokens 0 .. 2: zero values and a repeat, every feature in range
        ops.decode(on["idx"][good], on["vals"][good], on["W_dec"], on["b_dec"])
        ops.recon_curve(on["x"][good], on["vals"][good], on["idx"][good], on["W_dec"], on["b_dec"], h["ks"])
        for t in (3, 4, 6):
            with pytest.raises(IndexError):
                ops.decode(on["idx"][t:t + 1], on["vals"][t:t + 1], on["W_dec"], on["b_dec"])
            with pytest.raises(IndexError):
                ops.recon_curve(on["x"][t:t + 1], on["vals"][t:t + 1], on["idx"][t:t + 1], on["W_dec"], on["b_dec"], h["ks"])
    finally:
        ops.set_debug_bounds(False)


# ---- production width --------------------------------------------------------------------------------------------------------
def test_prefix_property_at_production_width_and_fvu(dev):
    """d = 4096, N = 131072, T = 300, the list from Sae.encode with k = 32: checkpoint 8 equals, bit for bit, recon_error of an
    Sae over the same weights with cfg.k = 8; and .fvu against the float64 restatement of e.pow(2).sum() / total_variance."""
    from msae import Sae, SaeConfig

    d, N, T = 4096, 131072, 300
    torch.manual_seed(3)
    sae = Sae(d, SaeConfig(num_latents=N, k=32), device=dev)
    with torch.no_grad():
        sae.b_dec.copy_(0.1 * torch.randn(d, device=dev))
    sae.eval()
    sae8 = copy.copy(sae)
    sae8.cfg = SaeConfig(num_latents=N, k=8)
    x = torch.from_numpy(synth.activations(T, d, seed=31)).to(dev, torch.bfloat16)
    top = sae.encode(x)
    out32 = sae.recon_error(x, ks=[8])
    out8 = sae8.recon_error(x, ks=[8])
    assert out8.err2.shape == (T, 1)
    for name in ("err2", "dot", "rnorm2", "xnorm2"):
        assert torch.equal(getattr(out32, name), getattr(out8, name)), name
    full = sae.recon_error(x, top=top)
    assert full.ks == (1, 2, 4, 8, 16, 32) and torch.equal(full.err2[:, 3], out8.err2[:, 0])
    # the same numbers from the decoder: sae.decode over the truncated list, then the reference's expressions in float64
    xf = x.float()
    tv = ref.total_variance_direct(xf.cpu().numpy())
    assert abs(float(full.total_variance) - tv) <= 1e-12 * tv
    for ci, kappa in enumerate(full.ks):
        with torch.no_grad():
            r = sae.decode(top.top_acts[:, :kappa].contiguous(), top.top_indices[:, :kappa].contiguous())
        e = (r - xf).double()
        s64, a64 = e.pow(2).sum(1).cpu().numpy(), e.pow(2).sum(1).cpu().numpy()
        assert (np.abs(full.err2[:, ci].double().cpu().numpy() - s64) <= ref.bound(a64, d)).all(), kappa
        fvu = s64.sum() / tv
        assert abs(float(full.fvu[ci]) - fvu) <= ref.gamma(d) * fvu + 1e-12 * fvu, kappa
    assert torch.allclose(full.mse, full.err2.double() / d) and full.cosine.shape == (T, 6)


# ---- ReconStats --------------------------------------------------------------------------------------------------------------
def _batches(rng, n, B, S, d, k, N, b):
    out = []
    for _ in range(n):
        x = ref.to_dtype((rng.standard_normal((B, S, d)) + b).astype(np.float32), "bf16")
        vals = -np.sort(-rng.uniform(0.1, 2.0, (B, S, k)).astype(np.float32), -1)
        out.append((x, vals, rng.integers(0, N, (B, S, k))))
    return out


def _assert_stats(st, exp, kernel_exp, d):
    """`exp`: the full restatement (per-token bound gamma_d on every term, then the float64 accumulation); `kernel_exp`: the
    float64 sums of the kernel's own per-token outputs (the float64 accumulation bound alone)."""
    for g in range(st.num_groups):
        n = exp[g]["n"]
        assert st.n[g] == n == kernel_exp[g]["n"]
        got = st.sums[g].cpu().numpy()
        acc = ref.stats_bound(n, kernel_exp[g]["sums_abs"])
        assert (np.abs(got - kernel_exp[g]["sums"]) <= acc).all(), g
        assert (np.abs(got - exp[g]["sums"]) <= ref.gamma(d) * exp[g]["terms_abs"] + n * d * 2.0 ** -149 + acc).all(), g
        assert abs(float(st.xx_sum[g]) - kernel_exp[g]["xx_sum"]) <= ref.stats_bound(n, kernel_exp[g]["xx_sum"])
        cs = st.cos_sum[g].cpu().numpy()
        assert (np.abs(cs - kernel_exp[g]["cos_sum"]) <= (2 * n + 8) * 2.0 ** -53 * n).all(), g       # |cos| <= 1 + eps per token
        xs = st.x_sum[g].cpu().numpy()
        assert (np.abs(xs - exp[g]["x_sum"]) <= 2 * n * 2.0 ** -53 * (np.abs(exp[g]["x_sum"]) + 8.0 * n)).all(), g


def test_recon_stats_cuts_merge_file_and_no_sync(dev, tmp_path):
    from msae import Sae, SaeConfig, ops
    from msae.features import ReconStats

    rng = np.random.default_rng(41)
    B, S, d, k, N = 4, 20, 100, 8, ref.N
    W = (rng.standard_normal((N, d)) / 10).astype(np.float32)
    b = (0.3 * rng.standard_normal(d)).astype(np.float32)
    sae = Sae(d, SaeConfig(num_latents=N, k=k), device=dev)
    with torch.no_grad():
        sae.W_dec.copy_(torch.from_numpy(W))
        sae.b_dec.copy_(torch.from_numpy(b))
    ks, all_ks, edges = [1, 4, 8], [0, 1, 4, 8], (0, 7)
    batches = _batches(rng, 3, B, S, d, k, N, b)
    on = [(torch.from_numpy(x).to(dev, torch.bfloat16), torch.from_numpy(v).to(dev), torch.from_numpy(i).to(dev))
          for x, v, i in batches]
    exp = ref.stats(batches, W, b, all_ks, edges)

    def kernel_mom(x2, v2, i2):
        m, xx = ops.recon_curve(torch.from_numpy(x2).to(dev, torch.bfloat16), torch.from_numpy(v2).to(dev),
                                torch.from_numpy(i2).to(dev), sae.W_dec, sae.b_dec, all_ks)
        return m.cpu().numpy(), xx.cpu().numpy()

    kernel_exp = ref.stats(batches, W, b, all_ks, edges, mom_of=kernel_mom)
    halves = ReconStats(d, ks, edges, device=dev)
    first, second = ReconStats(d, ks, edges, device=dev), ReconStats(d, ks, edges, device=dev)
    whole = ReconStats(d, ks, edges, b_dec=sae.b_dec, device=dev)
    with no_sync():
        for x, v, i in on:
            whole.update(x, v, i, sae)
            for a in (0, 2):
                halves.update(x[a:a + 2], v[a:a + 2], i[a:a + 2], sae)
        first.update(*on[0], sae)
        first.update(on[1][0][:2], on[1][1][:2], on[1][2][:2], sae)
        second.update(on[1][0][2:], on[1][1][2:], on[1][2][2:], sae)
        second.update(*on[2], sae)
    for st in (whole, halves, copy.deepcopy(first).merge(second)):
        _assert_stats(st, exp, kernel_exp, d)
    path = str(tmp_path / "recon_stats.safetensors")
    whole.save(path)
    back = ReconStats.load(path)                                                   # on the CPU
    assert back.device.type == "cpu" and back.n == whole.n and torch.equal(back.sums, whole.sums.cpu())
    direct = [ref.total_variance_direct(np.concatenate([x[:, a:e].reshape(-1, d) for x, _, _ in batches]))
              for a, e in ((0, 7), (7, S))]
    for g in (0, 1):
        assert torch.equal(back.fvu(g), whole.fvu(g)) and torch.equal(back.cosine(g), whole.cosine(g))
        fvu = exp[g]["sums"][1:, 0] / direct[g]
        assert np.allclose(whole.fvu(g).numpy(), fvu, rtol=4 * ref.gamma(d), atol=0), g
        assert np.allclose(whole.nmse(g).numpy(), exp[g]["sums"][1:, 0] / exp[g]["xx_sum"], rtol=4 * ref.gamma(d), atol=0)
        assert np.allclose(whole.mse(g).numpy(), exp[g]["sums"][1:, 0] / (exp[g]["n"] * d), rtol=2 * ref.gamma(d), atol=0)
    all_x = np.concatenate([x.reshape(-1, d) for x, _, _ in batches])
    tot = sum(e["sums"][1:, 0] for e in exp)
    assert np.allclose(whole.fvu().numpy(), tot / ref.total_variance_direct(all_x), rtol=4 * ref.gamma(d), atol=0)


def test_one_call_replays_from_a_graph_with_identical_bits(dev):
    """A single chain: the op's allocations and its one kernel, no parallel branches."""
    from msae import ops

    c = ref.CASES[[c.id for c in ref.CASES].index("d4096-k32-T300-pow2-bf16-i64")]
    x, v, idx, W, b = _inputs(c, dev)
    eager = ops.recon_curve(x, v, idx, W, b, c.ks)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.recon_curve(x, v, idx, W, b, c.ks)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mom, xx = ops.recon_curve(x, v, idx, W, b, c.ks)
    for _ in range(2):
        mom.zero_()
        xx.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mom, eager[0]) and torch.equal(xx, eager[1])


# ---- the cache loop ----------------------------------------------------------------------------------------------------------
def _image_cache(dev, g, recon):
    from msae import Sae, SaeConfig
    from msae.features import FeatureImageCache

    d, N = int(g["d"]), 4096
    torch.manual_seed(11)
    sae = Sae(d, SaeConfig(num_latents=N, k=16), device=dev)
    with torch.no_grad():
        sae.b_dec.copy_(0.2 * torch.randn(d, device=dev))
    model = fakes.TinyLlava(vocab=int(g["vocab"]), d=d).to(dev)
    module = str(g["module"])
    return sae, FeatureImageCache(model, None, {module: sae}, batch_size=2, shard_size=0,
                                  processor=fakes.FakeProcessor(int(g["vocab"])), recon=recon)


def test_end_to_end_cache(dev, tmp_path, golden_dir):
    """A FeatureImageCache run over the fake images with recon on: recon_stats.safetensors equals the restatement over the
    hidden states the loop held; the split files are byte-identical to a run without it, which writes nothing else; two rank
    files merge to the one-rank result within the float64 bound."""
    from msae.features import ReconStats
    from msae.features.cache import merge_rank_recon

    g = np.load(golden_dir / "g9_image_cache.npz")
    images = [{"image": fakes.FakeImage(i)} for i in range(int(g["n_images"]))]
    module, d = str(g["module"]), int(g["d"])
    ks, edges = [0, 1, 4, 16], (0, 2)
    outs, seen = {}, []
    for on in (False, True):
        sae, fic = _image_cache(dev, g, dict(ks=ks, position_edges=edges) if on else None)
        if on:
            inner = fic.cache.add_recon

            def spy(hidden, top_acts, top_indices, *a, **kw):
                seen.append((hidden.float().cpu().numpy(), top_acts.cpu().numpy(), top_indices.cpu().numpy()))
                return inner(hidden, top_acts, top_indices, *a, **kw)

            fic.cache.add_recon = spy
        fic.run(0, images)
        assert (fic.cache.recon_stats == {}) == (not on)
        out = tmp_path / ("on" if on else "off")
        fic.save_splits(n_splits=2, save_dir=str(out), rank=0)
        if on:
            assert "Rank0_recon_stats.safetensors" in os.listdir(out / module)
        fic.concate_safetensors(n_splits=2, save_dir=str(out))
        outs[on] = out / module
    off_files, on_files = sorted(os.listdir(outs[False])), sorted(os.listdir(outs[True]))
    assert on_files == sorted(off_files + ["recon_stats.safetensors"]) and len(off_files) == 2
    for f in off_files:
        assert (outs[False] / f).read_bytes() == (outs[True] / f).read_bytes(), f
    st = ReconStats.load(str(outs[True] / "recon_stats.safetensors"))
    assert st.ks == tuple(ks) and st.position_edges == edges and len(seen) == len(images) // 2
    assert seen[0][0].shape == (2, 4, d)                                            # BOS dropped: the positions the cache records
    W, b = sae.W_dec.detach().cpu().numpy(), sae.b_dec.detach().cpu().numpy()
    assert torch.equal(st.b_dec, sae.b_dec.detach().cpu())
    exp = ref.stats(seen, W, b, ks, edges)
    for gi in range(2):
        n = exp[gi]["n"]
        assert st.n[gi] == n == 2 * 2 * 2
        lim = ref.gamma(d) * exp[gi]["terms_abs"] + n * d * 2.0 ** -149 + ref.stats_bound(n, exp[gi]["sums_abs"])
        assert (np.abs(st.sums[gi].numpy() - exp[gi]["sums"]) <= lim).all(), gi
        assert (np.abs(st.x_sum[gi].numpy() - exp[gi]["x_sum"]) <= 2 * n * 2.0 ** -53 * np.abs(seen[0][0]).max() * n).all()
    assert torch.isfinite(st.fvu()).all() and (st.fvu() > 0).all()
    # two ranks, a batch each, merged by the concat step's helper
    os.makedirs(tmp_path / "two")
    for r, (x, v, i) in enumerate(seen):
        rs = ReconStats(d, ks, edges, b_dec=sae.b_dec, device=dev)
        rs.update(torch.from_numpy(x).to(dev, torch.float16), torch.from_numpy(v).to(dev), torch.from_numpy(i).to(dev), sae)
        rs.save(str(tmp_path / "two" / f"Rank{r}_recon_stats.safetensors"))
    merged = ReconStats.load(merge_rank_recon(str(tmp_path / "two"), dev))
    assert os.listdir(tmp_path / "two") == ["recon_stats.safetensors"] and merged.n == st.n
    for name in ("sums", "xx_sum", "cos_sum", "x_sum"):
        p, q = getattr(merged, name).numpy(), getattr(st, name).numpy()
        assert (np.abs(p - q) <= ref.stats_bound(8, np.abs(q) * 4 + 8)).all(), name
