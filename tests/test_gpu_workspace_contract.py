"""GPU: the workspace contract of include/msae.h, entry by entry, with exact-size, guarded and dirty scratch buffers.

The product hands every entry a slice of one grow-only buffer of at least 1 MiB (ops._workspace): a layout that under-counts
a region, or a kernel that walks past its last one, lands in slack, and what a kernel reads of stale scratch depends on the
order the tests ran.  Here ops._workspace is replaced by tests/guarded_ws.py: every request gets exactly the bytes the sizing
helper returned, between two 1 MiB guards, filled with zeros ("zero"), with the 32-bit word 3 ("word3"), or left as the call
before -- the same entry on OTHER inputs of the same shape -- left it ("recycled").  Every case runs under the three fills
and asserts

  (a) return code 0 (the host layer raises otherwise) and every guard word unchanged;
  (b) outputs and state against the entry's independent reference (oracle.*, coact_ref, act_hist_ref, feature_stats_ref /
      feature_sample_ref, neighbors_ref, train_ref, candidate_ref), with the equality or the bound of the entry's own test;
  (c) the three fills give bit-identical outputs -- all but act_sum of the feature statistics (f64 atomics, compared by (b)).

Read-before-write audit (done on the launch code before any dirty buffer ran; the GPU run confirms it).  For every region a
kernel of the call may read: who writes it first, in the same call.

  entry                         region                           first writer in the call
  ----------------------------  -------------------------------  ---------------------------------------------------------
  msae_encode_topk[_i64]        dense [T][N] (shapes without     msae_pre_acts_launch, every element of the T rows
   (make_plan)                    the fused pass)
    large batch (run_fast /     cnt [T] (+ segcnt [T][8])        zero_call_scratch
     run_cert)                  flagged [T] | count 64 | passes  zero_call_scratch (flag_words); pass counts:
                                                                 fallback_counts_kernel, only when fb_chunks > 1
                                colmax [d][parts]                zero_call_scratch (int8 / fp8), then prep_colmax_kernel
                                fmcount [N + 1], fmdefer [2 T]   zero_call_scratch (plans with the feature-major route);
                                                                 block sums behind fmcount: fm_blocksum_kernel
                                odims, is_out                    pick_outliers_kernel
                                a32 [T][d]                       prep_colmax_kernel / prep_x_kernel (a shard: never read)
                                xq, xqo, rowc, rowe (Tp rows)    quant_x_kernel / cert_quant_x_kernel / quant_x_fp8_kernel:
                                                                 one workgroup per row of the PADDED tile, rows >= T zero;
                                                                 bf16: prep_x_kernel (xb, padded rows zero) + row_p4_kernel
                                                                 (rowc of rows < T; the epilogues read rowc[t] for t < T)
                                colc, colc_s, colc_p, cds*,      gather_wo_kernel / gather_wo_fp8_kernel, every column
                                 wqo, wqos
                                refs                             band_refs_kernel
                                sample [T][S]                    the sample GEMM's epilogue (t < T)
                                tauv [T][r] column r - 1         kth_value kernels (the one column read); generic shapes:
                                 (taui)                          msae_topk_launch writes all r columns
                                cand / segcand [T][cap]          the GEMM epilogue and the sample push append below the
                                                                 zeroed counters; readers stop at min(cnt, cap);
                                                                 compact_candidates_kernel joins the segments
                                fmtarget, fmkeys, fmpre/rank     phase1_emit for EVERY token (the LEAN launch or the full
                                                                 one that takes what it deferred); fmpre: fm_dot_kernel
                                fmpairs                          pad slots: fm_scan_kernel; pair slots: fm_scatter_kernel;
                                                                 fm_dot_kernel reads fmcount[N] slots
                                fallback dense [fb_cap][N]       msae_pre_acts_launch for the listed rows
    small batch (run_small)     viol [T] | done [T], flagged     prep_small_kernel (its workgroup 0), a launch before any
                                                                 reader
                                a32, xhi, xlo, rowc              prep_small_kernel
                                surv, bound                      gemv_small_kernel / gemv_mfma_kernel, every slot
                                                                 select_small_kernel is told to read (n_surv, n_bound)
                                scand [T][128], stau             select_small_kernel
                                skeys (exact) [T][128]           rescore_small_kernel, every slot (0 for an empty one)
    exact = 1                   flagged list                     iota_list_kernel (list, count, zeros behind)
  msae_encode_topk_rows         pass counts                      fallback_counts_kernel, only when fb_chunks > 1 (read then)
   (make_plan_rows)             dense                            msae_pre_acts_launch
  msae_shard_candidates         make_plan's regions as above; a32 is neither written nor read, no re-score regions.  The
                                plan (shard_C = C) is never larger than the helper's (shard_C = 0): C only lowers the
                                threshold rank r, hence cap, tau_n and the segment count, and drops the fm regions.
  msae_rescore_candidates       flagged [T] | count | passes     zero_i32_kernel (flag_words)
   (make_plan_ext)              a32                              prep_x_kernel (T_valid rows, the rows read)
                                fallback dense                   msae_pre_acts_launch
  msae_decode_bwd_wdec_f32      counts [N + 1]                   wgrad_zero_kernel
                                offsets, cursor [N + 1]          wgrad_scan_kernel (no pairs: wgrad_zero_kernel on offsets)
                                perm [A k]                       wgrad_fill_kernel: the slots offsets[] delimits, no others
  msae_feature_stats_update     keys0, vals0                     fs_keys_kernel, all M
   [_sampled] (fs_layout)       keys1, vals1, sort               rocPRIM (its own temporaries); the candidates over the dead
                                                                 value buffer: fs_group_kernel
                                ends [N]                         hipMemsetAsync
                                starts [N]                       fs_group_kernel; read only where ends[f] != 0
  msae_coact_update             keys0                            coact_keys_kernel, all M
   (co_layout)                  keys1, sort                      rocPRIM
                                ends [nseg]                      hipMemsetAsync
                                starts [nseg]                    coact_heads_kernel, with ends; read only where ends != 0
                                (token mode uses no workspace)
  msae_act_hist_update          keys0, vals0                     ah_keys_kernel, all M
   (ah_layout)                  keys1, vals1, sort               rocPRIM
                                (token mode uses no workspace)
  msae_rows_topk_f32            rows [M], ones [M]               clamp_rows_kernel
   (head_bytes + lists)         lists [C][2][M][k]               rows_topk_kernel, every chunk's k entries per row
  msae_weighted_row_sum_f32     part [groups][d]                 weighted_rows_part_kernel, every group (all-zero too)
                                mid [n_mid][d]                   weighted_rows_sum_kernel

No region is read uninitialised.  What the audit and the host tests did find, fixed with this module: msae_rows_topk_*
answered a missing or short workspace with MSAE_EINVAL instead of MSAE_EWS, and the sizing helpers of the feature statistics,
the fused encode, the candidate re-score, the row sums and the neighbours returned a size for shapes their entries refuse.

Out of reach of a small shape: more than one pass of the in-call exact fallback (fb_chunks > 1, the only reader of the
per-pass counts) needs T above 4 GiB / (4 N) rows -- 131072 tokens at N = 8192.  Its counts are written by
fallback_counts_kernel in the same call; no case here runs it.

msae_rescore_candidates refuses G C < k (the records cannot hold a top-k): at G = 2, k = 32 the C = 8 case runs the shard
call alone, checks its records, and asserts that refusal.
"""
import contextlib
import ctypes
import gc

import numpy as np
import pytest
import torch

import act_hist_ref
import candidate_ref
import coact_ref
import feature_sample_ref as sref
import feature_stats_ref as fref
import guarded_ws
import neighbors_ref as nref
import synth
import train_ref as tr
from oracle import oracle

pytestmark = pytest.mark.gpu

MSAE_EINVAL, MSAE_EWS = -1, -3
SEED = 12345                  # msae_options::dither_seed of every prepare and encode: the same roundings in every run
N_FAST = 8192                 # the smallest width with the fused pass
FILL_IDS = [f"fill_{f}" for f in guarded_ws.FILLS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(params=guarded_ws.FILLS, ids=FILL_IDS)
def fill(request):
    return request.param


@pytest.fixture(autouse=True)
def _free_after():
    yield
    from msae import ops

    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def install(monkeypatch, dev):
    """install(fill, what) -> the GuardedWorkspace now standing in for ops._workspace"""
    from msae import ops

    def _install(fill, what):
        gws = guarded_ws.GuardedWorkspace(fill, dev)
        gws.what = what
        monkeypatch.setattr(ops, "_workspace", gws)
        return gws

    return _install


@contextlib.contextmanager
def _seeded():
    from msae import ops

    ops.set_dither("on", seed=SEED)
    try:
        yield
    finally:
        ops.set_dither("default")


def _np(t):
    return t.detach().cpu().numpy()


def _np_all(outs):
    return tuple(np.ascontiguousarray(_np(o)) for o in outs)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))
        raise AssertionError(f"{what}: {bad.size} bytes differ, first in element {bad[0] // a.itemsize} of {a.size}")


_ZERO = {}        # case -> the outputs of its run on zeroed workspaces, shared by the three fills of the case


def _three_fills(install, fill, case, run, verify, bits=None):
    """The case under `fill`.  run(alt) -> tensors (alt: other inputs of the same shape, the call a "recycled" buffer is left
    over from); verify(outputs as numpy arrays): (b); bits: the outputs (c) compares, all when None."""
    gws = install(fill, case)
    if fill == "recycled":
        run(True)
        gws.check()
    out = _np_all(run(False))
    gws.check()
    assert gws.requests, f"{case}: the call asked for no workspace"
    verify(out)
    if fill == "zero":
        _ZERO[case] = out
    elif case not in _ZERO:                     # (this fill run on its own: the zeroed run is made here)
        g0 = install("zero", case)
        _ZERO[case] = _np_all(run(False))
        g0.check()
    for j, (a, b) in enumerate(zip(out, _ZERO[case])):
        if bits is None or j in bits:
            _same_bits(a, b, f"{case}: output {j} under fill {fill!r} against the zeroed workspace")
    return gws


# ---- inputs, built once and left unchanged ----------------------------------------------------------------------------------------
_WEIGHTS, _DEVICE, _ENC_REF = {}, {}, {}


def _weights(d, N):
    if (d, N) not in _WEIGHTS:
        _WEIGHTS[(d, N)] = synth.sae_weights(d, N, seed=21)
    return _WEIGHTS[(d, N)]


def _on_device(dev, d, N, mode="int8"):
    """(W, b_enc, b_dec, prepared) on the device; `mode`: the coarse mode the operands were prepared under"""
    from msae import ops

    key = (d, N, mode)
    if key not in _DEVICE:
        W, b, _, bd = (torch.from_numpy(a).to(dev) for a in _weights(d, N))
        old = ops._defaults.coarse
        ops.set_coarse_mode(mode)
        try:
            with _seeded():
                prepared = ops.prepare_encoder(W)
        finally:
            ops.set_coarse_mode(old)
        _DEVICE[key] = (W, b, bd, prepared)
    return _DEVICE[key]


def _x(T, d, seed, dtype, dev):
    """(numpy f32 values, device tensor of `dtype`): the values the device tensor holds, which is what the references get"""
    xt = torch.from_numpy(synth.activations(T, d, seed=seed, bf16=dtype != torch.float32)).to(dev, dtype)
    return np.ascontiguousarray(_np(xt.float())), xt


# ---- msae_encode_topk_i64 -------------------------------------------------------------------------------------------------------
ENCODE = {
    # small path (<= 16 tokens, d % 1024 == 0): the dot4 weight stream and the MFMA stream
    "small_dot4_T1": dict(T=1, d=1024, k=32),
    "small_mfma_T5": dict(T=5, d=1024, k=32),
    "small_mfma_T16": dict(T=16, d=1024, k=32),
    # int8 pass with segmented candidate lists (T <= 256, cap >= 1024) ...
    "int8_segmented_T200": dict(T=200, d=256, k=32),
    # ... and without: r = 8 (k = 8), r = 16, r = 32 with cap 4096 (k = 256)
    "int8_T300_k8": dict(T=300, d=256, k=8),
    "int8_T300_k32": dict(T=300, d=256, k=32),
    "int8_T300_k256": dict(T=300, d=256, k=256),
    "bf16_pass_d192": dict(T=300, d=192, k=32),
    "coarse_fp8": dict(T=300, d=256, k=32, mode="fp8"),
    "certified": dict(T=300, d=256, k=32, certified=True),
    "feature_major_forced": dict(T=512, d=1024, k=32, fm=True),
    "exact_path_N1000": dict(T=40, d=50, k=8, N=1000),
    "x_f32": dict(T=300, d=256, k=32, dtype=torch.float32),
    "x_f16": dict(T=300, d=256, k=32, dtype=torch.float16),
    "hook_edits": dict(T=300, d=256, k=32, edits=True),
}


def _encode_ref(name, c, x, W, b, bd, kw):
    if name not in _ENC_REF:
        _ENC_REF[name] = oracle.encode_topk(x, W, b, bd, c["k"], kw.get("set_feature", -1), kw.get("set_value", 0.0),
                                            kw.get("zero_feature", -1))
    return _ENC_REF[name]


@pytest.mark.parametrize("name", list(ENCODE))
def test_encode_topk(dev, install, monkeypatch, fill, name):
    from msae import _hip, ops

    c = ENCODE[name]
    T, d, k, N = c["T"], c["d"], c["k"], c.get("N", N_FAST)
    dtype, mode = c.get("dtype", torch.bfloat16), c.get("mode", "int8")
    Wn, bn, _, bdn = _weights(d, N)
    W, b, bd, prepared = _on_device(dev, d, N, mode)
    xn, xt = _x(T, d, 22, dtype, dev)
    _, xt_alt = _x(T, d, 122, dtype, dev)
    kw = {}
    if c.get("edits"):
        hot = int(oracle.encode_topk(xn[:1], Wn, bn, bdn, k)[1][0, 0])         # a feature that IS in the top-k: zero it
        kw = dict(set_feature=77, set_value=10.0, zero_feature=hot)
    if mode == "fp8":
        kw["coarse_mode"] = 2
    if c.get("certified"):
        kw["certified"] = True
    rows = None
    if c.get("fm"):            # the route forced on as tests/test_gpu_rescore_followup.py's forced_fm does
        monkeypatch.setenv("MSAE_FM", "1")
        monkeypatch.setenv("MSAE_LPR", "1")
        ops._WS_BYTES_CACHE.clear()
        rows = torch.zeros(T, dtype=torch.int32, device=dev)
    ref_v, ref_i = _encode_ref(name, c, xn, Wn, bn, bdn, kw)

    def run(alt):
        with _seeded(), (ops.rescore_rows(rows) if rows is not None else contextlib.nullcontext()):
            return ops.encode_topk(xt_alt if alt else xt, W, b, bd, prepared, k, **kw)

    def verify(out):
        v, i, st = out
        assert int(((st & 0xFF) >= 2).sum()) == 0, "unresolved tokens"
        assert np.array_equal(i, ref_i), f"indices differ on {int((i != ref_i).any(-1).sum())} of {T} tokens"
        _same_bits(v, ref_v, "top_acts against the oracle")

    try:
        gws = _three_fills(install, fill, f"msae_encode_topk_i64 {name} T={T} d={d} N={N} k={k}", run, verify)
        want = _hip.load().msae_encode_topk_ws_bytes(T, d, N, k, ops._opts(**{"coarse_mode": kw.get("coarse_mode", -1)}).ref()) \
            if not c.get("certified") else None
        if want is not None:
            assert {n for _, n in gws.requests} == {want}, (gws.requests, want)
        if rows is not None:
            ver = _np(rows) != 0
            assert ver.sum() >= T // 2 and bool(((_np(rows)[ver] >> 30) & 1).all()), "the feature-major route did not run"
    finally:
        if c.get("fm"):
            ops._WS_BYTES_CACHE.clear()


# ---- msae_encode_topk_rows ------------------------------------------------------------------------------------------------------
def test_encode_topk_rows(dev, install, fill):
    from msae import _hip, ops

    T, d, N, k = 128, 256, N_FAST, 32           # max_rows = 128
    Wn, bn, _, bdn = _weights(d, N)
    W, b, bd, _ = _on_device(dev, d, N)
    xn, xt = _x(T, d, 31, torch.bfloat16, dev)
    _, xt_alt = _x(T, d, 131, torch.bfloat16, dev)
    listed = [3, 77, 0, 127, 64]
    ref_v, ref_i = oracle.encode_topk(xn[listed], Wn, bn, bdn, k)

    def run(alt):
        rows = torch.zeros(T, dtype=torch.int32, device=dev)
        rows[:5] = torch.tensor(listed, dtype=torch.int32)
        n = torch.tensor([5], dtype=torch.int32, device=dev)
        vals = torch.full((T, k), -7.0, device=dev)
        idx = torch.full((T, k), -7, dtype=torch.int64, device=dev)
        st = torch.full((T,), -7, dtype=torch.int32, device=dev)
        ops.encode_topk_rows_(xt_alt if alt else xt, W, b, bd, rows, n, k, vals, idx, st)
        return vals, idx, st

    def verify(out):
        v, i, st = out
        assert np.array_equal(i[listed], ref_i) and np.array_equal(st[listed], np.ones(5, np.int32))
        _same_bits(v[listed], ref_v, "listed rows against the oracle")
        rest = np.setdiff1d(np.arange(T), listed)
        assert (v[rest] == -7.0).all() and (i[rest] == -7).all() and (st[rest] == -7).all(), "an unlisted row was written"

    gws = _three_fills(install, fill, f"msae_encode_topk_rows max_rows={T} N={N} d={d} k={k}", run, verify)
    assert {n for _, n in gws.requests} == {_hip.load().msae_encode_topk_rows_ws_bytes(T, N)}


# ---- msae_shard_candidates + msae_rescore_candidates ----------------------------------------------------------------------------
def _canonical_records(recs, C):
    """(keys [T, C] descending, their z sigma, the tail): a record holds its entries in the order the candidate list was
    appended in (atomics: it varies from run to run; the owner sorts), so records are compared entry set by entry set"""
    keys = recs[:, :8 * C].contiguous().view(torch.int64)
    zs = recs[:, 8 * C:12 * C].contiguous().view(torch.float32)
    order = torch.argsort(keys, dim=1, descending=True)
    return keys.gather(1, order), zs.gather(1, order), recs[:, 12 * C:12 * C + 8].contiguous().view(torch.float32)


@pytest.mark.parametrize("C", ["default", 8])
@pytest.mark.parametrize("T", [200, 300])
def test_shard_candidates_and_rescore(dev, install, fill, T, C):
    from msae import _hip, ops
    from msae.parallel import default_candidates

    G, n_loc, d, k = 2, N_FAST, 256, 32
    N = G * n_loc
    C = default_candidates(k, G) if C == "default" else C
    lib = _hip.load()
    Wn, bn, _, bdn = _weights(d, N)
    W, b, bd, prepared = _on_device(dev, d, N)
    key = ("shards", d, N)
    if key not in _DEVICE:
        with _seeded():
            _DEVICE[key] = [(W[g * n_loc:(g + 1) * n_loc].contiguous(), b[g * n_loc:(g + 1) * n_loc].contiguous(),
                             ops.prepare_encoder(W[g * n_loc:(g + 1) * n_loc].contiguous())) for g in range(G)]
    shards = _DEVICE[key]
    xn, xt = _x(T, d, 41, torch.bfloat16, dev)
    _, xt_alt = _x(T, d, 141, torch.bfloat16, dev)
    rkey = ("shard_ref", T)
    if rkey not in _ENC_REF:
        _ENC_REF[rkey] = oracle.encode_topk(xn, Wn, bn, bdn, k)
    ref_v, ref_i = _ENC_REF[rkey]
    can_rescore = G * C >= k
    shard_bytes = lib.msae_encode_topk_ws_bytes(T, d, n_loc, k, None)      # the header's contract for the shard call

    def run(alt):
        x = xt_alt if alt else xt
        with _seeded():
            recs = [ops.shard_candidates(x, bs, bd, ps, n_loc, k, g * n_loc, C) for g, (_, bs, ps) in enumerate(shards)]
            canon = [a for r in recs for a in _canonical_records(r, C)]
            if not can_rescore:
                return (*recs, *canon)
            v, i, st = ops.rescore_candidates(x, W, b, bd, k, torch.stack(recs).contiguous(), C)
            ev, ei, _ = ops.encode_topk(x, W, b, bd, prepared, k)
        return (*recs, *canon, v, i, st, ev, ei)

    def verify(out):
        # the records against f64 pre-activations: a listed pair's upper value bounds its exact value, the tail bounds every
        # feature the record left out (7 sigma bands: 1e-12 per pair against 5e6 pairs; fixed seeds: the same pairs every run)
        finite = 0
        for g, (Ws, bs, _) in enumerate(shards):
            r = candidate_ref.decode_records(torch.from_numpy(out[g]), C)
            p = _np(candidate_ref.exact_pre(xt, Ws, bs, bd))
            loc = r["feat"] - g * n_loc
            assert ((loc >= 0) & (loc < n_loc))[r["valid"]].all(), "a record names a feature outside its shard"
            tt = np.broadcast_to(np.arange(T)[:, None], loc.shape)
            assert (r["u"][r["valid"]].astype(np.float64) >= p[tt[r["valid"]], loc[r["valid"]]]).all()
            left = np.ones((T, n_loc), bool)
            left[tt[r["valid"]], loc[r["valid"]]] = False
            worst = np.where(left, p, -np.inf).max(axis=1)
            assert (worst <= r["tail"].astype(np.float64)).all(), "a feature outside the record lies above its tail"
            finite += int(np.isfinite(r["tail"]).sum())
        assert finite >= G * T // 2, "most records do not bound what they left out: the check above is vacuous"
        if can_rescore:
            v, i, st, ev, ei = out[4 * G:]
            assert int((st >= 2).sum()) == 0
            assert np.array_equal(i, ref_i) and np.array_equal(ei, ref_i)
            _same_bits(v, ref_v, "re-scored candidates against the oracle")
            _same_bits(ev, ref_v, "single-GPU encode against the oracle")

    gws = _three_fills(install, fill, f"msae_shard_candidates + msae_rescore_candidates T={T} C={C} G={G}", run, verify,
                       bits=set(range(G, 4 * G + 5)))         # (the raw records: compared in canonical order)
    asked = [n for who, n in gws.requests if who == "shard_candidates"]
    assert asked and set(asked) == {shard_bytes}, (asked, shard_bytes)
    if not can_rescore:                          # G C < k: the owner-side call refuses the records
        recs = torch.zeros(G, T, lib.msae_shard_record_bytes(C), dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match=r"code -1"):
            ops.rescore_candidates(xt, W, b, bd, k, recs, C)
        assert lib.msae_rescore_candidates_ws_bytes(T, d, N, k, G, C) == 0


# ---- msae_decode_bwd_wdec_f32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,k,N,d", [(64, 3, 37, 4), (64, 3, 8193, 8)])
def test_decode_bwd_wdec(dev, install, fill, A, k, N, d):
    """tests/test_gpu_shared_helpers.py::test_wgrad_scan_tile_edges's shapes, reference and bound (an f32 chain of L terms:
    2e-7 sum|act| max|g| sqrt(L) + 1e-12), with feature 5 picked by every token (a segment of exactly 64 pairs)."""
    from msae import _hip, ops

    def inputs(seed):
        g = torch.Generator().manual_seed(seed)
        idx = torch.randint(0, N, (A, k), generator=g)
        idx[:, 1] = 5
        idx[idx[:, 0] == 5, 0] = 6
        idx[idx[:, 2] == 5, 2] = 7
        idx[0, 0], idx[1, 0] = 0, N - 1
        acts = torch.rand(A, k, generator=g) + 0.05
        acts[::9, 2] = 0.0                       # pairs that carry nothing
        return idx, acts, torch.randn(A, d, generator=g)

    idx, acts, gout = inputs(N)
    alt = inputs(N + 1)
    Wshape = torch.empty(N, d, device=dev)       # only its shape is read

    def run(a):
        i, v, g = alt if a else (idx, acts, gout)
        return (ops.decode_bwd(i.to(dev), v.to(dev), Wshape, g.to(dev), False, True)[1],)

    def verify(out):
        gw = torch.from_numpy(out[0])
        flat = idx.reshape(-1)
        ref = torch.zeros(N, d, dtype=torch.float64)
        ref.index_add_(0, flat, acts.reshape(-1, 1).double() * gout.double().repeat_interleave(k, 0))
        mag = torch.zeros(N, dtype=torch.float64).index_add_(0, flat, acts.reshape(-1).double())
        counts = torch.bincount(flat, minlength=N)
        tol = 2e-7 * mag * float(gout.abs().max()) * counts.clamp(min=1).double().sqrt() + 1e-12
        assert ((gw.double() - ref).abs().amax(dim=1) <= tol).all()
        assert int(counts[5]) == A and (gw[counts == 0] == 0).all()

    gws = _three_fills(install, fill, f"msae_decode_bwd_wdec_f32 A={A} k={k} N={N} d={d}", run, verify)
    assert {n for _, n in gws.requests} == {_hip.load().msae_decode_bwd_wdec_ws_bytes(A, k, N)}


# ---- the counters of the cache loop: feature statistics (+ sample), co-activation, histograms ------------------------------------------
# (pool, B, S, k, N, window, pool_len): window mode with a ragged tail, image mode, and both at B S k = 300 000 for rocPRIM's
# temporary storage against the layouts' *_sort_bound
COUNTER_CASES = {"window": ("window", 3, 50, 8, 1000, 16, 576), "image": ("image", 3, 50, 8, 1000, 64, 32),
                 "window_300k": ("window", 3, 3125, 32, 1000, 64, 576), "image_300k": ("image", 3, 3125, 32, 1000, 64, 576)}
_PAIRS, _COUNTER_REF = {}, {}


def _pairs(B, S, k, N, seed):
    """[B, S, k] values on a coarse grid (exact ties, some zeros: below the threshold) and distinct features per token"""
    key = (B, S, k, N, seed)
    if key not in _PAIRS:
        rng = np.random.default_rng(seed)
        idx = np.argsort(rng.random((B * S, N), dtype=np.float32), axis=1)[:, :k].astype(np.int64).reshape(B, S, k)
        vals = (rng.integers(0, 64, size=(B, S, k)) * 0.125).astype(np.float32)
        _PAIRS[key] = (vals, idx)
    return _PAIRS[key]


def _counter_inputs(case, dev):
    pool, B, S, k, N, W, P = COUNTER_CASES[case]
    vals, idx = _pairs(B, S, k, N, 7)
    av, ai = _pairs(B, S, k, N, 8)
    to = lambda a: torch.from_numpy(a).to(dev)
    return (pool, B, S, k, N, W, P), (vals, idx), (to(vals), to(idx)), (to(av), to(ai))


def _ref(key, make):
    if key not in _COUNTER_REF:
        _COUNTER_REF[key] = make()
    return _COUNTER_REF[key]


@pytest.mark.parametrize("n_sample", [0, 16])
@pytest.mark.parametrize("case", list(COUNTER_CASES))
def test_feature_stats_update(dev, install, fill, case, n_sample):
    """msae_feature_stats_update (n_sample = 0) and _update_sampled: tests/test_gpu_feature_stats.py's comparison (tables bit for
    bit, act_sum to 1e-9 relative) and tests/test_gpu_feature_sample.py's (the sample bit for bit)."""
    from msae import _hip
    from msae.features import FeatureStats

    (pool, B, S, k, N, W, P), (vals, idx), main, alt = _counter_inputs(case, dev)
    row_base, n_top = 2 ** 33 + 5, 64

    def expected():
        b, s, f, v = fref.records(vals.reshape(B * S, k), idx.reshape(B * S, k), S, N=N)
        cf, cv, ci = fref.candidates(b, s, f, v, S, pool, row_base, P=P, W=W)
        return fref.basic_stats(f, v, N) + fref.top_tables(cf, cv, ci, N, n_top) + (cf, cv, ci)

    count, mx, sm, tv, ti, cf, cv, ci = _ref(("fs", case), expected)

    def run(a):
        st = FeatureStats(N, n_top=n_top, pool=pool, pool_len=P, window=W, device=dev, n_sample=n_sample, sample_seed=22)
        st.update(*(alt if a else main), row_base)
        out = (st.count, st.act_max, st.act_sum, st.top_val, st.top_id)
        return out + ((st.seg_count, st.smp_val, st.smp_id) if n_sample else ())

    def verify(out):
        assert np.array_equal(out[0], count) and np.array_equal(out[1], mx)
        np.testing.assert_allclose(out[2], sm, rtol=1e-9, atol=0)
        assert np.array_equal(out[4], ti)
        _same_bits(out[3], tv, "top_val")
        if n_sample:
            seg, sv, si = sref.sample_tables(cf, cv, ci, N, n_sample, 22)
            assert np.array_equal(out[5], seg) and np.array_equal(out[7], si)
            _same_bits(out[6], sv, "smp_val")

    gws = _three_fills(install, fill, f"msae_feature_stats_update{'_sampled' if n_sample else ''} {case} B={B} S={S} k={k} "
                       f"N={N}", run, verify, bits={0, 1, 3, 4, 5, 6, 7})
    assert {n for _, n in gws.requests} == {_hip.load().msae_feature_stats_ws_bytes(B * S, k, N)}


@pytest.mark.parametrize("case", list(COUNTER_CASES))
def test_coact_update(dev, install, fill, case):
    from msae import _hip
    from msae.features import CoactStats

    (pool, B, S, k, N, W, P), (vals, idx), main, alt = _counter_inputs(case, dev)
    queries = [5, 999, 0, 123, 500, 77, 640, 311]
    counts, seg_count, nseg = _ref(("co", case), lambda: coact_ref.run([(vals, idx)], queries, pool, N, P=P, W=W))

    def run(a):
        st = CoactStats(N, queries, pool=pool, pool_len=P, window=W, device=dev)
        st.update(*(alt if a else main))
        assert a or st.n_segments == nseg
        return st.counts, st.seg_count

    def verify(out):
        assert np.array_equal(out[1], seg_count) and np.array_equal(out[0], counts) and counts.sum() > 0

    gws = _three_fills(install, fill, f"msae_coact_update {case} B={B} S={S} k={k} N={N}", run, verify)
    assert {n for _, n in gws.requests} == {_hip.load().msae_coact_ws_bytes(B * S, k, N)}


@pytest.mark.parametrize("case", list(COUNTER_CASES))
def test_act_hist_update(dev, install, fill, case):
    from msae import _hip
    from msae.features import ActHist

    (pool, B, S, k, N, W, P), (vals, idx), main, alt = _counter_inputs(case, dev)
    hist, nseg = _ref(("ah", case), lambda: act_hist_ref.run([(vals, idx)], pool, N, P=P, W=W))

    def run(a):
        st = ActHist(N, pool=pool, pool_len=P, window=W, device=dev)
        st.update(*(alt if a else main))
        assert a or st.n_segments == nseg
        return (st.hist,)

    def verify(out):
        assert np.array_equal(out[0], hist) and hist.sum() > 0

    gws = _three_fills(install, fill, f"msae_act_hist_update {case} B={B} S={S} k={k} N={N}", run, verify)
    assert {n for _, n in gws.requests} == {_hip.load().msae_act_hist_ws_bytes(B * S, k, N)}


def test_token_mode_with_an_empty_workspace(dev, fill):
    """MSAE_POOL_TOKEN of the co-activation counters and the histograms uses none of its workspace: a guarded block of 0 bytes."""
    from msae import _hip

    lib = _hip.load()
    B, S, k, N = 3, 50, 8, 1000
    vals, idx = _pairs(B, S, k, N, 7)
    queries = [5, 999, 0, 123, 500, 77, 640, 311]
    tv, ti = torch.from_numpy(vals).to(dev), torch.from_numpy(idx).to(dev, torch.int32)
    slot_of = torch.full((N,), -1, dtype=torch.int32, device=dev)
    slot_of[torch.tensor(queries, device=dev)] = torch.arange(len(queries), dtype=torch.int32, device=dev)
    counts = torch.zeros(len(queries), N, dtype=torch.int32, device=dev)
    seg_count = torch.zeros(N, dtype=torch.int64, device=dev)
    hist = torch.zeros(N, 256, dtype=torch.int32, device=dev)
    gws = guarded_ws.GuardedWorkspace(fill, dev)
    gws.what = f"token mode B={B} S={S} k={k} N={N}"
    stream = _hip.stream_of(tv)
    ptr, n, _ = gws.block(0)
    assert n == 0 and ptr % 256 == 0
    assert lib.msae_coact_update(_hip.ptr(tv), _hip.ptr(ti), B, S, k, 1e-5, N, 2, 576, 64, _hip.ptr(slot_of), len(queries),
                                 _hip.ptr(counts), _hip.ptr(seg_count), ctypes.c_void_p(ptr), 0, stream) == 0
    ptr, n, _ = gws.block(0)
    assert lib.msae_act_hist_update(_hip.ptr(tv), _hip.ptr(ti), B, S, k, 1e-5, N, 2, 576, 64, 3, -16, 32, _hip.ptr(hist),
                                    ctypes.c_void_p(ptr), 0, stream) == 0
    gws.check()
    rc, rs, _ = _ref(("co", "token"), lambda: coact_ref.run([(vals, idx)], queries, "token", N))
    rh, _ = _ref(("ah", "token"), lambda: act_hist_ref.run([(vals, idx)], "token", N))
    assert np.array_equal(_np(counts), rc) and np.array_equal(_np(seg_count), rs) and np.array_equal(_np(hist), rh)


# ---- msae_rows_topk_f32 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [0, 1, 2, 4])         # 1: no merge buffers, the row list alone
def test_rows_topk(dev, install, fill, chunks):
    """tests/test_gpu_neighbors.py::test_grid's comparison (oracle dots, canonical ranking: bit for bit) at M = 130 listed rows."""
    from msae import _hip, ops

    M, N, d, k = 130, 1000, 48, 8
    key = ("nb", N, d)
    if key not in _COUNTER_REF:
        rng = np.random.default_rng(1000 + d + N)
        centers = rng.standard_normal((32, d)).astype(np.float32)
        Wn = centers[rng.integers(0, 32, N)] * np.float32(0.7) + rng.standard_normal((N, d)).astype(np.float32)
        rows = rng.integers(0, N, M)
        rows[5] = rows[77]
        _COUNTER_REF[key] = (np.ascontiguousarray(Wn), rows, nref.rank(nref.dots(Wn, Wn, rows), k), rng.integers(0, N, M))
    Wn, rows, (ref_v, ref_i), rows_alt = _COUNTER_REF[key]
    Wt = torch.from_numpy(Wn).to(dev)
    rt, rt_alt = (torch.from_numpy(r.astype(np.int32)).to(dev) for r in (rows, rows_alt))

    def run(a):
        return ops.rows_topk(Wt, Wt, k, q_rows=rt_alt if a else rt, chunks=chunks)

    def verify(out):
        assert np.array_equal(out[1], ref_i)
        _same_bits(out[0], ref_v, "values")

    gws = _three_fills(install, fill, f"msae_rows_topk_i64_f32 M={M} N={N} d={d} k={k} chunks={chunks}", run, verify)
    want = _hip.load().msae_rows_topk_ws_bytes(M, N, k, chunks)
    assert {n for _, n in gws.requests} == {want}
    # the two row lists [M], and behind them the merge buffers [chunks][2][M][k] of more than one chunk
    assert chunks == 0 or want == 2 * 768 + (chunks * 2 * M * k * 4 if chunks > 1 else 0)


# ---- msae_weighted_row_sum_f32 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["dense", "group_zero"])
def test_weighted_row_sum(dev, install, fill, pattern):
    """tests/test_gpu_train_passes.py::test_weighted_row_sum_within_float64_bounds's reference and bound at N = 1000, d = 68;
    group_zero: a whole 64-row group whose partial row must still be written."""
    from msae import _hip, ops

    N, d, scale = 1000, 68, -1.0
    W0, s0 = tr.wrs_inputs(N, d, pattern)
    W1, s1 = tr.wrs_inputs(N, d, "two_thirds_zero")
    ref, bnd = tr.weighted_row_sum(W0, s0, scale)
    dW = [(W0.to(dev), s0.to(dev)), (W1.to(dev), s1.to(dev))]

    def run(a):
        return (ops.weighted_row_sum(*dW[1 if a else 0], scale),)

    def verify(out):
        tr.assert_within(torch.from_numpy(out[0]), ref, bnd, f"weighted_row_sum {N}x{d} {pattern}")
        assert out[0].any()

    gws = _three_fills(install, fill, f"msae_weighted_row_sum_f32 N={N} d={d} {pattern}", run, verify)
    assert {n for _, n in gws.requests} == {_hip.load().msae_weighted_row_sum_ws_bytes(N, d)}


# ---- a workspace that is too small, or missing, is refused before any write ------------------------------------------------------
def _interior_untouched(blk, fill):
    v = blk.view
    if fill == "zero":
        return not bool(v.any())
    want = torch.where(torch.arange(v.numel(), device=v.device) % 4 == 0, guarded_ws.FILL_WORD, 0).to(torch.uint8)
    return torch.equal(v, want)


def _refusal_entries(dev):
    """(name, bytes the helper asks for, call(ws pointer or None, ws_bytes) -> return code, outputs and state) of every entry"""
    from msae import _hip, ops

    lib = _hip.load()
    P = _hip.ptr
    S7 = lambda *shape, dtype=torch.float32: torch.full(shape, 249 if dtype == torch.uint8 else -7, dtype=dtype, device=dev)
    T, d, N, k = 300, 256, N_FAST, 32
    W, b, bd, prepared = _on_device(dev, d, N)
    _, xt = _x(T, d, 22, torch.bfloat16, dev)
    st = _hip.stream_of(xt)
    out = []

    vals, idx, status = S7(T, k), S7(T, k, dtype=torch.int64), S7(T, dtype=torch.int32)
    out.append(("msae_encode_topk_i64", lib.msae_encode_topk_ws_bytes(T, d, N, k, None),
                lambda ws, n: lib.msae_encode_topk_i64(P(xt), 1, P(W), P(b), P(bd), P(prepared), T, d, N, k, -1, 0.0, -1, P(vals),
                                                       P(idx), P(status), ws, n, None, st), [vals, idx, status]))
    rows = torch.arange(128, dtype=torch.int32, device=dev)
    n_rows = torch.tensor([5], dtype=torch.int32, device=dev)
    rv, ri, rs = S7(128, k), S7(128, k, dtype=torch.int64), S7(128, dtype=torch.int32)
    out.append(("msae_encode_topk_rows", lib.msae_encode_topk_rows_ws_bytes(128, N),
                lambda ws, n: lib.msae_encode_topk_rows(P(xt), 1, P(W), P(b), P(bd), P(rows), P(n_rows), 128, d, N, k, -1, 0.0, -1,
                                                        P(rv), P(ri), P(rs), ws, n, st), [rv, ri, rs]))
    C = 64
    recs = S7(2, T, lib.msae_shard_record_bytes(C), dtype=torch.uint8)
    out.append(("msae_shard_candidates", lib.msae_encode_topk_ws_bytes(T, d, N, k, None),
                lambda ws, n: lib.msae_shard_candidates(P(xt), 1, P(b), P(bd), P(prepared), T, d, N, k, 0, C, -1, -1, P(recs), ws, n,
                                                        None, st), [recs]))
    W2, b2 = torch.cat([W, W]), torch.cat([b, b])
    cv, ci, cs = S7(T, k), S7(T, k, dtype=torch.int64), S7(T, dtype=torch.int32)
    out.append(("msae_rescore_candidates", lib.msae_rescore_candidates_ws_bytes(T, d, 2 * N, k, 2, C),
                lambda ws, n: lib.msae_rescore_candidates(P(xt), 1, P(W2), P(b2), P(bd), T, T, d, 2 * N, k, 2, C, P(recs), -1, 0.0,
                                                          -1, P(cv), P(ci), P(cs), ws, n, None, st), [cv, ci, cs, W2, b2]))
    A, wk, wN, wd = 64, 3, 8193, 8
    g = torch.Generator().manual_seed(3)
    widx = torch.randint(0, wN, (A, wk), generator=g).to(dev, torch.int32)
    wacts, wgout, gw = torch.rand(A, wk, generator=g).to(dev), torch.randn(A, wd, generator=g).to(dev), S7(wN, wd)
    out.append(("msae_decode_bwd_wdec_f32", lib.msae_decode_bwd_wdec_ws_bytes(A, wk, wN),
                lambda ws, n: lib.msae_decode_bwd_wdec_f32(P(widx), P(wacts), P(wgout), A, wk, wN, wd, P(gw), None, None, None, ws, n,
                                                           st), [gw, widx, wacts, wgout]))
    B, S, ck, cN = 3, 50, 8, 1000
    pv, pi = _pairs(B, S, ck, cN, 7)
    tv, ti = torch.from_numpy(pv).to(dev), torch.from_numpy(pi).to(dev, torch.int32)
    count, amax, asum = S7(cN, dtype=torch.int64), S7(cN), S7(cN, dtype=torch.float64)
    tval, tid = S7(cN, 64), S7(cN, 64, dtype=torch.int64)
    fs_args = lambda: (P(tv), P(ti), B, S, ck, 1e-5, cN, 1, 576, 16, 0, 64, P(count), P(amax), P(asum), P(tval), P(tid))
    out.append(("msae_feature_stats_update", lib.msae_feature_stats_ws_bytes(B * S, ck, cN),
                lambda ws, n: lib.msae_feature_stats_update(*fs_args(), ws, n, st), [count, amax, asum, tval, tid, tv, ti]))
    seg, sval, sid = S7(cN, dtype=torch.int64), S7(cN, 16), S7(cN, 16, dtype=torch.int64)
    sample = _hip.MsaeFeatureSample(ctypes.sizeof(_hip.MsaeFeatureSample), 16, 22, seg.data_ptr(), sval.data_ptr(), sid.data_ptr())
    out.append(("msae_feature_stats_update_sampled", lib.msae_feature_stats_ws_bytes(B * S, ck, cN),
                lambda ws, n: lib.msae_feature_stats_update_sampled(*fs_args(), ctypes.byref(sample), ws, n, st),
                [count, amax, asum, tval, tid, seg, sval, sid]))
    slot_of = torch.full((cN,), -1, dtype=torch.int32, device=dev)
    slot_of[:4] = torch.arange(4, dtype=torch.int32, device=dev)
    cc, csc = S7(4, cN, dtype=torch.int32), S7(cN, dtype=torch.int64)
    out.append(("msae_coact_update", lib.msae_coact_ws_bytes(B * S, ck, cN),
                lambda ws, n: lib.msae_coact_update(P(tv), P(ti), B, S, ck, 1e-5, cN, 1, 576, 16, P(slot_of), 4, P(cc), P(csc), ws, n,
                                                    st), [cc, csc, slot_of]))
    hist = S7(cN, 256, dtype=torch.int32)
    out.append(("msae_act_hist_update", lib.msae_act_hist_ws_bytes(B * S, ck, cN),
                lambda ws, n: lib.msae_act_hist_update(P(tv), P(ti), B, S, ck, 1e-5, cN, 1, 576, 16, 3, -16, 32, P(hist), ws, n, st),
                [hist]))
    M, nN, nd, nk = 130, 1000, 48, 8
    Q = torch.randn(nN, nd, generator=g).to(dev)
    qrows = torch.randint(0, nN, (M,), generator=g).to(dev, torch.int32)
    nv, ni = S7(M, nk), S7(M, nk, dtype=torch.int32)
    for chunks in (0, 4):
        out.append((f"msae_rows_topk_f32 chunks={chunks}", lib.msae_rows_topk_ws_bytes(M, nN, nk, chunks),
                    lambda ws, n, c=chunks: lib.msae_rows_topk_f32(P(Q), nN, P(qrows), M, P(Q), nN, nd, None, None, None, nk, c,
                                                                   P(nv), P(ni), ws, n, st), [nv, ni, Q, qrows]))
    sW, ss, so = torch.randn(1000, 68, generator=g).to(dev), torch.randn(1000, generator=g).to(dev), S7(68)
    out.append(("msae_weighted_row_sum_f32", lib.msae_weighted_row_sum_ws_bytes(1000, 68),
                lambda ws, n: lib.msae_weighted_row_sum_f32(P(sW), P(ss), 1000, 68, -1.0, P(so), ws, n, st), [so, sW, ss]))
    return out


def test_too_small_or_missing_workspace_is_refused_before_any_write(dev):
    """Every entry, straight through the C ABI: ws_bytes one byte short (256 bytes short where the helper's result is a multiple
    of 256), and ws = NULL with the full size: MSAE_EWS, outputs and state (pre-filled with -7) unchanged, the short block
    and its guards unchanged."""
    gws = guarded_ws.GuardedWorkspace("word3", dev)
    for name, need, call, tensors in _refusal_entries(dev):
        assert need > 0, name
        before = [t.clone() for t in tensors]
        short = need - 256 if need % 256 == 0 else need - 1
        gws.what = f"{name} with {short} of {need} bytes"
        ptr, n, blk = gws.block(short)
        assert call(ctypes.c_void_p(ptr), n) == MSAE_EWS, f"{name}: {short} of {need} bytes"
        assert call(None, need) == MSAE_EWS, f"{name}: ws = NULL"
        gws.check()
        assert _interior_untouched(blk, "word3"), f"{name}: the refused call wrote into the short workspace"
        for t, t0 in zip(tensors, before):
            assert torch.equal(t, t0), f"{name}: a refused call changed an output"


# ---- the cache loop on one shared buffer ----------------------------------------------------------------------------------------
def test_cache_loop_on_one_recycled_buffer(dev, install):
    """Two batches of Sae.encode -> Cache.add_topk with FeatureStats, CoactStats and ActHist attached, every op on the block the
    op before it left behind (as on the product's one shared buffer) -- against the references, and against the same loop on
    zeroed blocks."""
    from msae import Sae, SaeConfig
    from msae.features import Cache

    d, N, B, S, k = 256, N_FAST, 2, 64, 32
    Wn, bn, Wdn, bdn = _weights(d, N)
    sae = Sae(d, SaeConfig(num_latents=N, k=k), device=dev).eval().requires_grad_(False)
    with torch.no_grad():
        for p, a in ((sae.encoder.weight, Wn), (sae.encoder.bias, bn), (sae.W_dec, Wdn), (sae.b_dec, bdn)):
            p.copy_(torch.from_numpy(a))
    xs = [_x(B * S, d, 51 + j, torch.bfloat16, dev) for j in range(2)]
    tops = [oracle.encode_topk(xn, Wn, bn, bdn, k) for xn, _ in xs]
    queries = sorted({int(f) for f in tops[0][1][:4, :3].reshape(-1)})
    Wn_, Pn = 16, 48

    def loop(fill):
        gws = install(fill, f"cache loop, fill {fill}")
        cache = Cache(0, None, batch_size=B, stats=dict(pool="window", window=Wn_), coact=dict(pool="image", pool_len=Pn,
                      queries=queries), hist=dict(pool="window", window=Wn_))
        for j, (_, xt) in enumerate(xs):
            with torch.no_grad():
                top = sae.encode(xt)
            cache.add_topk(top.top_acts.view(B, S, k), top.top_indices.view(B, S, k), N, j, "m")
            gws.check()
        cache.save()
        fs, co, ah = cache.feature_stats["m"], cache.coact_stats["m"], cache.act_hists["m"]
        callers = {who for who, _ in gws.requests}
        assert {"encode_topk", "feature_stats_update", "coact_update", "act_hist_update"} <= callers, callers
        return _np_all((cache.feature_locations["m"], cache.feature_activations["m"], fs.count, fs.act_max, fs.act_sum, fs.top_val,
                        fs.top_id, co.counts, co.seg_count, ah.hist))

    got, zero = loop("recycled"), loop("zero")
    for j, (a, z) in enumerate(zip(got, zero)):
        if j != 4:                               # (act_sum: f64 atomics, compared with the reference below)
            _same_bits(a, z, f"cache loop output {j}: recycled blocks against zeroed blocks")
    loc, act = zip(*[oracle.sparsify(v, i, B, S, row_base=j * B) for j, (v, i) in enumerate(tops)])
    assert np.array_equal(got[0], np.concatenate(loc))
    _same_bits(got[1], np.concatenate(act), "records' activations")
    F, V, CF, CV, CI = [], [], [], [], []
    for j, (v, i) in enumerate(tops):
        b_, s_, f_, v_ = fref.records(v, i, S, N=N)
        cf, cv, ci = fref.candidates(b_, s_, f_, v_, S, "window", j * B, W=Wn_)
        F.append(f_), V.append(v_), CF.append(cf), CV.append(cv), CI.append(ci)
    count, mx, sm = fref.basic_stats(np.concatenate(F), np.concatenate(V), N)
    tv, ti = fref.top_tables(np.concatenate(CF), np.concatenate(CV), np.concatenate(CI), N, 64)
    assert np.array_equal(got[2], count) and np.array_equal(got[3], mx) and np.array_equal(got[6], ti)
    np.testing.assert_allclose(got[4], sm, rtol=1e-9, atol=0)
    _same_bits(got[5], tv, "top_val")
    calls = [(v.reshape(B, S, k), i.reshape(B, S, k).astype(np.int64)) for v, i in tops]
    cc, csc, _ = coact_ref.run(calls, queries, "image", N, P=Pn)
    assert np.array_equal(got[7], cc) and np.array_equal(got[8], csc) and cc.sum() > 0
    assert np.array_equal(got[9], act_hist_ref.run(calls, "window", N, W=Wn_)[0])


# ---- one training step ------------------------------------------------------------------------------------------------------------
def test_one_training_step_under_dirty_guarded_workspaces(dev, install):
    """SaeTrainStep.step at N = 8192, d = 256, T = 256, k = 32, auxk_alpha = 1/32 with every workspace exact-size, guarded and
    filled with word 3: the fused encoder inside autograd, both weight-gradient sorts and weighted_row_sum.  The dense torch
    restatement and every bound are tests/test_gpu_config_sizes.py::test_train_step_at_c2_matches_dense_torch_restatement's
    (no feature is dead in a first step, so the AuxK term is zero on both sides)."""
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    D, N, T, k = 256, N_FAST, 256, 32
    lr = 2e-4 / (N / 2 ** 14) ** 0.5
    gws = install("word3", f"SaeTrainStep.step N={N} d={D} T={T} k={k}")
    sae = Sae(D, SaeConfig(num_latents=N, k=k), device=dev)
    g = torch.Generator(device=dev).manual_seed(91)
    with torch.no_grad():
        w = torch.randn(N, D, generator=g, device=dev)
        sae.encoder.weight.copy_(w / w.norm(dim=1, keepdim=True))
        sae.W_dec.copy_(sae.encoder.weight)
        sae.encoder.bias.copy_(torch.randn(N, generator=g, device=dev) * 0.01)
        sae.b_dec.copy_(torch.randn(D, generator=g, device=dev) * 0.05)
    sae.set_decoder_norm_to_unit_norm()
    x = torch.randn(T, D, generator=g, device=dev) + 0.25 * torch.randn(D, generator=g, device=dev)
    params0 = [p.detach().clone() for p in (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)]

    out = sae(x)
    out.fvu.backward()
    gws.check()
    grads = [p.grad.detach().clone() for p in (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)]
    idx_hip, acts_hip, fvu_hip = out.latent_indices.detach(), out.latent_acts.detach(), float(out.fvu.detach())
    for p in sae.parameters():
        p.grad = None
    del out
    callers = {who for who, _ in gws.requests}
    assert {"encode_topk", "decode_bwd", "weighted_row_sum"} <= callers, callers

    We, be, Wd, bd = (torch.nn.Parameter(p.clone()) for p in params0)
    pre = torch.relu(torch.nn.functional.linear(x - bd, We, be))
    with torch.no_grad():
        kth = pre.gather(1, idx_hip).min(dim=1).values
        above = (pre > (kth * (1 + 1e-5) + 1e-6)[:, None]).sum(1)
        assert int(above.max()) <= k, "the HIP selection is not a top-k of the dense latents"
    acts = pre.gather(1, idx_hip)
    assert (acts.detach() - acts_hip).abs().max().item() <= 1e-4
    recon = (acts[:, :, None] * Wd[idx_hip]).sum(1) + bd
    fvu = (recon - x).pow(2).sum() / (x - x.mean(0)).pow(2).sum()
    assert abs(float(fvu.detach()) - fvu_hip) <= 1e-4 * abs(fvu_hip)
    fvu.backward()
    for name, got, ref in zip(("W_enc", "b_enc", "W_dec", "b_dec"), grads, (We.grad, be.grad, Wd.grad, bd.grad)):
        err = (got - ref).abs().max().item()
        assert err <= 2e-4 * ref.abs().max().item() + 1e-9, (name, err, ref.abs().max().item())
    torch.nn.utils.clip_grad_norm_([We, be, Wd, bd], 1.0)
    with torch.no_grad():
        Wd.grad -= (Wd.grad * Wd.data).sum(dim=1, keepdim=True) * Wd.data
    torch.optim.Adam([We, be, Wd, bd], lr=lr).step()

    ts = SaeTrainStep(sae, lr=lr, auxk_alpha=1.0 / 32)
    stats = ts.step(x)
    gws.check()
    assert float(stats["auxk_loss"]) == 0.0
    assert abs(float(stats["fvu"]) - float(fvu.detach())) <= 1e-4 * float(fvu.detach())
    if ts.fuse_next_step:
        assert ts._normed_version == sae.W_dec._version
        with torch.no_grad():
            Wd.data /= Wd.data.norm(dim=1, keepdim=True) + torch.finfo(torch.float32).eps
    for name, p, ref, p0 in zip(("W_enc", "b_enc", "W_dec", "b_dec"),
                                (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec), (We, be, Wd, bd), params0):
        diff = (p.detach() - ref.data).abs()
        bad = diff > 2e-6 + 1e-5 * ref.data.abs() + 0.02 * lr
        assert bad.float().mean().item() < 1e-4, (name, int(bad.sum()), bad.numel())
        assert diff.max().item() <= 2.1 * lr, (name, diff.max().item())
        assert (p.detach() - p0).abs().max().item() > 0.5 * lr, (name, "the step did not move the parameter")
    fired = torch.zeros(N, dtype=torch.bool, device=dev)
    fired[idx_hip.reshape(-1)] = True
    assert torch.equal(ts.num_tokens_since_fired == 0, fired)
