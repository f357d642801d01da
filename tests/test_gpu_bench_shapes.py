"""EVERY token of the shapes behind the benchmark's numbers, on the object the benchmark times.

bench.py's headline (d = 4096, N = 131072, T = 8192, k = 32) and its --full records (k256, t2880, t65536, zipf, coarse_fp8,
dither_off, exact_modes.certified) run `bench.HipRuntime().engine(...)` -- ShardedSae(world = 1) with reuse_buffers -- over
`bench.make_inputs` weights and batches, one process-wide workspace serving calls of changing T and k.  The tests below take
weights, biases, batches, seeds and the engine from bench.py itself and check each call's (top_acts, top_indices, sae_out)
on three levels (tests/bench_shapes_ref.py): A every token bit for bit against the exact HIP path, B every token against
float64 in plain torch with the derived bound gamma_{d+1} (sum |a W| + |b|), C a token sample bit for bit against the C oracle.
A call is checked before the next one is issued.  What a case adds beyond "the outputs are right":

  1 headline loop   the four rotated batches, two laps on one engine: lap 2 (other dither seeds drawn per call, and the
                    per-token re-score statistics on, as bench.py's instrumented pass) returns lap 1's bits
  2 k = 256         the same batches on a k = 256 engine
  3 changing T      8192 -> 2880 -> 65536 -> 8192 on one engine and one workspace; the last call returns the first call's bits
  4 zipf            bench.zipf_bias as the encoder bias: a handful of dense features, heavy-tailed usage
  5 modes           coarse = "fp8", dither = "off", certified -- set as HipRuntime.options sets them, engines created where
                    bench.py creates them; "same exact outputs" as a test
  6 lifetimes       a reconstruction handed out by call i is unchanged after call i + 1 (the streaming contract of
                    reuse_buffers; parallel.py::_gather_recon), and without reuse_buffers it never aliases the engine's ring

Each call prints one "bench-shape-parity:" line: T, k, mode; main / sample output tiles per persistent workgroup of the candidate
GEMM (bench_shapes_ref.tiles_per_workgroup: GEMM_BM x GEMM_BN = 256 x 256 tiles of csrc/encode_fused.hip's GemmCfg, SAMPLE_STRIDE
= 32 of csrc/encode_defs.h, the grid of csrc/gemm_mfma.h gemm_launch = the device's CUs); rows of W_enc re-scored per token
(ops.rescore_rows); tokens verified / exact fallback / unresolved / verified-and-wrong; the largest |v - P| / B and the largest
reconstruction error over its bound; tokens whose f64 gap exceeds 2 B and how many of them match the f64 set (information);
oracle rows.  profiles/bench_shape_parity.txt holds the lines of one run.

The exact-fallback cap is test_gpu_hostile._compare's: 0.03 of the tokens, 1.0 under `certified` (deterministic bands widen on
the batches' four x20 dims).
"""
import contextlib
import gc

import pytest
import torch

import bench
import bench_shapes_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu

D, N, T_BENCH = bench.D_MODEL, bench.WIDTH, 8192
SAMPLE_SEED = 20250


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


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(dev):
    """The benchmark's SAE (seed 0) and its four rotated batches, once per module; host copies for the oracle; the f64 copies."""
    assert (D, N) == (4096, 131072)
    c = _Ctx()
    c.dev, c.rt = dev, bench.HipRuntime()
    W_enc, b_enc, W_dec, b_dec, x0 = bench.make_inputs(dev, T_BENCH, D, N, seed=0)
    c.weights = (W_enc, b_enc, W_dec, b_dec)
    c.xs = [x0] + [bench.make_inputs(dev, T_BENCH, D, min(N, 8192), seed=7919 * j)[4] for j in range(1, 4)]   # more_batches
    c.host = tuple(t.cpu().numpy() for t in c.weights)
    c.f64 = ref.F64Reference(W_enc, b_enc, b_dec, W_dec)
    c.rows_buf = torch.zeros(65536, dtype=torch.int32, device=dev)
    c.n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    yield c
    c.__dict__.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _tokens_batch(c, T, j=0):
    """bench.py run_tokens: the batches of the t2880 / t65536 records."""
    return bench.make_inputs(c.dev, T, D, min(N, 8192), seed=101 + 7919 * j)[4]


def _step(c, eng, x, stats):
    """One step as bench.py's timed loop issues it; stats: inside ops.rescore_rows, as its instrumented pass.
    -> (out, mean rows of W_enc re-scored per verified token or None)"""
    from msae import ops

    if stats:
        c.rows_buf.zero_()
    with (ops.rescore_rows(c.rows_buf) if stats else contextlib.nullcontext()):
        out = eng.forward(x, async_gather=eng.collective, gather=True)
    eng.synchronize()
    rows = None
    if stats:
        got = c.rows_buf[: x.shape[0]]
        got = got[got > 0]
        rows = float((got & 0xFFF).float().mean()) if got.numel() else float("nan")
    return out, rows


def _check(c, x, out, k, what, mode="int8", b_enc=None, max_fallback=0.03, rows=None):
    """Levels A, B, C on one call's outputs, then the coverage line."""
    from msae import ops

    W_enc, b_enc0, W_dec, b_dec = c.weights
    T = x.shape[0]
    be, f64, host = b_enc0, c.f64, c.host
    if b_enc is not None:
        be, f64, host = b_enc, c.f64.with_bias(b_enc), (c.host[0], b_enc.cpu().numpy(), c.host[2], c.host[3])
    assert out["top_acts"].shape == (T, k) and out["top_indices"].shape == (T, k) and out["sae_out"].shape == (T, D)
    assert out["status"].shape == (T,) and out["top_indices"].dtype == torch.int64
    exact = ref.exact_path(ops, x, W_enc, be, b_dec, W_dec, k, chunk=2048)
    hist = ref.level_a(out, exact, what, max_fallback=max_fallback)
    del exact
    enc = f64.check_encode(x, out["top_acts"], out["top_indices"], what)
    dec = f64.check_decode(out["top_acts"], out["top_indices"], out["sae_out"], what)
    sample = ref.sample_rows(T, out["status"].cpu().numpy(), seed=SAMPLE_SEED)
    n_oracle = ref.level_c(oracle, host, x, out, sample, k, what)
    main, samp = ref.tiles_per_workgroup(T, N, c.n_cu, mode)
    print(f"\nbench-shape-parity: {what}: T={T} k={k} mode={mode} tiles/workgroup main={main} sample={samp} "
          f"rows/token={'n/a' if rows is None else format(rows, '.1f')} verified={hist['verified']} fallback={hist['fallback']} "
          f"unresolved={hist['unresolved']} wrong={hist['wrong']} max|v-P|/B={enc['max_ratio']:.4f} "
          f"max_recon_err/bound={dec['max_ratio_recon']:.4f} gap>2B={enc['wide_gap']} matched_f64_set={enc['wide_gap_matched']} "
          f"oracle_rows={n_oracle}", flush=True)
    return hist


def _keep(out):
    """What a later call is compared with (`status` depends on the dither seeds drawn per call: compared only as "no code >= 2",
    which level A asserts)."""
    return {n: out[n] for n in ("top_acts", "top_indices", "sae_out")}


def test_headline_loop_two_laps(ctx):
    """Case 1.  Lap 1 runs un-instrumented (the headline pass), lap 2 with the re-score statistics on (the instrumented pass)."""
    W_enc, b_enc, W_dec, b_dec = ctx.weights
    eng = ctx.rt.engine(W_enc, b_enc, W_dec, b_dec, 32)
    assert eng.reuse_buffers and not eng.collective and eng.world == 1
    first = {}
    for lap in range(2):
        for j, x in enumerate(ctx.xs):
            out, rows = _step(ctx, eng, x, stats=(lap == 1))
            _check(ctx, x, out, 32, f"headline lap {lap + 1} batch {j}", rows=rows)
            if lap == 0:
                first[j] = _keep(out)
            else:
                assert ref.same_bits(out, first[j]), f"lap 2 batch {j}: outputs differ from lap 1 (dither seeds / stale state)"
            del out
    del eng, first


def test_k256_engine(ctx):
    """Case 2: the k256 record's engine on the same batches."""
    W_enc, b_enc, W_dec, b_dec = ctx.weights
    eng = ctx.rt.engine(W_enc, b_enc, W_dec, b_dec, 256)
    for j, x in enumerate(ctx.xs):
        out, rows = _step(ctx, eng, x, stats=True)
        _check(ctx, x, out, 256, f"k256 batch {j}", rows=rows)
        del out
    del eng


def test_changing_T_on_one_engine_and_one_workspace(ctx):
    """Case 3: the headline engine sees the t2880 and t65536 records' calls between two headline batches."""
    W_enc, b_enc, W_dec, b_dec = ctx.weights
    eng = ctx.rt.engine(W_enc, b_enc, W_dec, b_dec, 32)
    calls = [("T 8192 first", ctx.xs[0]), ("T 2880", _tokens_batch(ctx, 2880)), ("T 65536", _tokens_batch(ctx, 65536)),
             ("T 8192 again", ctx.xs[0])]
    first = None
    for n, (what, x) in enumerate(calls):
        out, rows = _step(ctx, eng, x, stats=True)
        _check(ctx, x, out, 32, "changing " + what, rows=rows)
        if n == 0:
            first = _keep(out)
        if n == 3:
            assert ref.same_bits(out, first), "8192 tokens after the 2880- and 65536-token calls: outputs differ from the first call"
        del out
    del eng, first, calls


def test_zipf_bias(ctx):
    """Case 4: the zipf record -- bench.zipf_bias(xs[0], ...) as the encoder bias."""
    W_enc, _, W_dec, b_dec = ctx.weights
    bz = bench.zipf_bias(ctx.xs[0], b_dec, N, 32, ctx.dev)
    eng = ctx.rt.engine(W_enc, bz, W_dec, b_dec, 32)
    out, rows = _step(ctx, eng, ctx.xs[0], stats=True)
    _check(ctx, ctx.xs[0], out, 32, "zipf", b_enc=bz, rows=rows)
    del eng, out


@pytest.mark.parametrize("mode", ["coarse_fp8", "dither_off", "certified"])
def test_modes_with_the_same_exact_outputs(ctx, mode):
    """Case 5: bench.py's run_fp8 / run_dither_off create their engine INSIDE the option (operands prepared under it); run_modes
    runs the headline engine, created under the defaults, inside `certified`."""
    from msae import ops

    W_enc, b_enc, W_dec, b_dec = ctx.weights
    x = ctx.xs[0]
    d0 = ops._defaults
    prev = (d0.exact, d0.coarse, d0.dither, d0.dither_seed, d0.certified)
    try:
        if mode == "certified":
            eng = ctx.rt.engine(W_enc, b_enc, W_dec, b_dec, 32)
            with ctx.rt.options(certified=True):
                out, rows = _step(ctx, eng, x, stats=True)
        else:
            kw = {"coarse_fp8": dict(coarse="fp8"), "dither_off": dict(dither="off")}[mode]
            with ctx.rt.options(**kw):
                eng = ctx.rt.engine(W_enc, b_enc, W_dec, b_dec, 32)
                out, rows = _step(ctx, eng, x, stats=True)
    finally:
        ops.set_exact(prev[0])
        ops.set_coarse_mode(prev[1])
        ops.set_dither(prev[2], prev[3])
        ops.set_certified(prev[4])
    gemm = {"coarse_fp8": "fp8", "dither_off": "dither_off", "certified": "certified"}[mode]
    _check(ctx, x, out, 32, mode, mode=gemm, max_fallback=1.0 if mode == "certified" else 0.03, rows=rows)
    del eng, out


def test_reconstruction_of_call_i_survives_call_i_plus_1(ctx):
    """Case 6 on the benchmark's object (reuse_buffers = True): call i's outputs, kept by the caller, are checked on all three
    levels AFTER call i + 1 has run."""
    W_enc, b_enc, W_dec, b_dec = ctx.weights
    eng = ctx.rt.engine(W_enc, b_enc, W_dec, b_dec, 32)
    assert eng.reuse_buffers
    out0, _ = _step(ctx, eng, ctx.xs[0], stats=False)
    snap = out0["sae_out"].clone()
    out1, _ = _step(ctx, eng, ctx.xs[1], stats=False)
    assert not ref.token_bit_mismatch(out0["sae_out"], snap).any(), "call i's sae_out changed during call i + 1"
    assert out0["sae_out"].data_ptr() != out1["sae_out"].data_ptr()
    _check(ctx, ctx.xs[0], out0, 32, "lifetime call i, checked after call i+1")
    _check(ctx, ctx.xs[1], out1, 32, "lifetime call i+1")
    del eng, out0, out1, snap


@pytest.mark.parametrize("reuse", [True, False])
def test_reconstruction_ring_lifetimes(ctx, monkeypatch, reuse):
    """Case 6 on the ring itself.  A single-GPU engine decodes without the ring; the gathered decode of a group does
    (_gather_recon: two send / receive pairs per shape).  Here the group has one rank and its all-gather is a device copy
    -- the ring, its indexing and the reuse_buffers rule are the engine's own.
      reuse_buffers = True : the view handed out by call i is unchanged after call i + 1 and holds the exact path's bits; call
                             i + 2 takes its slot (the documented lifetime: the two-deep ring);
      reuse_buffers = False: the returned tensor is the caller's -- unchanged after two more calls, no ring buffer behind it."""
    from msae import ops, parallel

    W_enc, b_enc, W_dec, b_dec = ctx.weights

    def all_gather_one_rank(full, pad, group=None, async_op=False):
        assert not async_op and full.shape == pad.shape
        full.copy_(pad)

    monkeypatch.setattr(parallel.dist, "all_gather_into_tensor", all_gather_one_rank)
    eng = ctx.rt.engine(W_enc, b_enc, W_dec, b_dec, 32)
    eng.reuse_buffers = reuse
    tops, want = [], []
    for x in ctx.xs[:3]:
        o, _ = _step(ctx, eng, x, stats=False)
        tops.append((o["top_acts"], o["top_indices"]))
        want.append(o["sae_out"])                       # the un-gathered decode of the same latents (checked by the cases above)
    eng.collective = True                               # from here on decode() goes through _gather_recon
    r0 = eng.decode(*tops[0])
    assert not ref.token_bit_mismatch(r0, want[0]).any()
    r1 = eng.decode(*tops[1])
    assert not ref.token_bit_mismatch(r1, want[1]).any()
    assert not ref.token_bit_mismatch(r0, want[0]).any(), "the reconstruction of call i changed during call i + 1"
    ctx.f64.check_decode(*tops[0], r0, "ring call i after call i+1")
    r2 = eng.decode(*tops[2])
    assert not ref.token_bit_mismatch(r2, want[2]).any() and not ref.token_bit_mismatch(r1, want[1]).any()
    ring = [buf for pair in next(iter(eng._recon_bufs.values()))[:2] for buf in pair]
    assert len(eng._recon_bufs) == 1 and len(ring) == 4
    ring_ptrs = {b.data_ptr() for b in ring}
    if reuse:
        assert r0.data_ptr() in ring_ptrs and r1.data_ptr() in ring_ptrs and r0.data_ptr() != r1.data_ptr()
        assert r2.data_ptr() == r0.data_ptr(), "a two-deep ring: call i + 2 takes call i's slot"
    else:
        for r, w in zip((r0, r1, r2), want):
            assert r.data_ptr() not in ring_ptrs
            assert not ref.token_bit_mismatch(r, w).any(), "a returned reconstruction changed under later calls"
    del eng, tops, want, r0, r1, r2, ring
