"""Transcoders on the GPU against tests/transcoder_ref.py.

  kernel        msae_gemm_nt_acc_f32 bit for bit against oracle.pre_acts(..., relu=False) plus ONE float32 add, over
                M x P x K = {1, 127, 129, 300} x {1, 100, 128, 130} x {4, 33, 64, 100} (33: the generic staging path), f32 /
                bf16 / f16 `a`, both `accumulate` values, ld_c > P with poisoned padding that must survive, bases offset by one
                float, C_in holding -0.0, inf and NaN, and the MSAE_EINVAL cases;
  forward       d_in = 256, d_out in {256, 192}, N = 8192, k = 32, T in {1, 5, 300}: indices equal the restatement's selection
                outside the undecided tokens (at most 1 %), yhat inside the derived bound n u sum |terms| (transcoder_ref), and
                without a skip connection bit-identical to ops.decode on the same list;
  gradients     every parameter and x inside |delta| <= 2e-3 max|ref| + 1e-8; W_skip's gradient non-zero, b_dec's the decoder
                side's alone;
  trajectories  six optimiser steps of five scenarios under the trajectory criterion of transcoder_ref (selections, the
                gradients handed to the optimiser, the update, a decoder that is not unit-norm), the steps running under
                torch.cuda.set_sync_debug_mode("error"); `skip_auxk_dead` (auxk_path="subset") lets the forward's one documented
                host read through -- the length of the dead list, Sae._dead_list -- counts it, and asserts it is the only one;
  hook          transcoder_hook on the fake model equals sae.transcode(input) bit for bit, edits on prefill only, S = 1 eager."""
import ctypes
import gc
import itertools

import numpy as np
import pytest
import torch

import transcoder_ref as R

pytestmark = pytest.mark.gpu


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


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
MS, PS, KS = (1, 127, 129, 300), (1, 100, 128, 130), (4, 33, 64, 100)
POISON = np.float32(-7.25e30)


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_gemm_nt_acc_bit_for_bit(dev, dtype, accumulate):
    from msae import _hip
    from oracle import oracle

    lib = _hip.load()
    rng = np.random.default_rng(11 + accumulate)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for n_case, (M, P, K) in enumerate(itertools.product(MS, PS, KS)):
        offset = n_case % 3 == 1                     # every third shape: all three bases one element off their alignment
        a = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).to(dtype)
        B = rng.standard_normal((P, K)).astype(np.float32)
        ld = P + 3
        C_in = np.full((M, ld), POISON, dtype=np.float32)
        C_in[:, :P] = rng.standard_normal((M, P)).astype(np.float32)
        flat = C_in[:, :P].reshape(-1)               # (a copy when P < ld: written back below)
        for j, v in enumerate((-0.0, np.inf, -np.inf, np.nan)):
            flat[(j * 7919) % flat.size] = v
        C_in[:, :P] = flat.reshape(M, P)
        s = oracle.pre_acts(a.float().numpy(), B, None, None, relu=False)
        with np.errstate(invalid="ignore"):
            want = C_in.copy()
            want[:, :P] = (C_in[:, :P] + s) if accumulate else s

        def on_dev(arr, td):
            buf = torch.empty(arr.numel() + 1, dtype=td, device=dev)
            view = buf[1:] if offset else buf[:-1]
            view.copy_(arr.reshape(-1))
            return buf, view
        ka, va = on_dev(a, dtype)
        kb, vb = on_dev(torch.from_numpy(B), torch.float32)
        kc, vc = on_dev(torch.from_numpy(C_in), torch.float32)
        rc = lib.msae_gemm_nt_acc_f32(ctypes.c_void_p(va.data_ptr()), _hip.DTYPE_CODE[dtype], ctypes.c_void_p(vb.data_ptr()),
                                      M, K, P, ctypes.c_void_p(vc.data_ptr()), ld, accumulate, stream)
        assert rc == 0, (M, P, K, rc)
        got = vc.cpu().numpy().reshape(M, ld)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (M, P, K, "NaN positions")
        assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), (M, P, K, offset, int((_bits(got) != _bits(want))[~nan].sum()))
        assert np.all(got[:, P:] == POISON), (M, P, K, "the padding was written")


def test_gemm_nt_acc_argument_errors_and_the_op(dev):
    from msae import _hip, ops

    lib = _hip.load()
    a = torch.randn(5, 8, device=dev)
    B = torch.randn(3, 8, device=dev)
    C = torch.zeros(5, 3, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    EINVAL = -1
    assert lib.msae_gemm_nt_acc_f32(None, 0, p(B), 5, 8, 3, p(C), 3, 0, st) == EINVAL
    assert lib.msae_gemm_nt_acc_f32(p(a), 0, None, 5, 8, 3, p(C), 3, 0, st) == EINVAL
    assert lib.msae_gemm_nt_acc_f32(p(a), 0, p(B), 5, 8, 3, None, 3, 0, st) == EINVAL
    assert lib.msae_gemm_nt_acc_f32(p(a), 3, p(B), 5, 8, 3, p(C), 3, 0, st) == EINVAL          # a dtype code outside the three
    assert lib.msae_gemm_nt_acc_f32(p(a), 0, p(B), 5, 0, 3, p(C), 3, 0, st) == EINVAL
    assert lib.msae_gemm_nt_acc_f32(p(a), 0, p(B), 5, 8, 0, p(C), 3, 0, st) == EINVAL
    assert lib.msae_gemm_nt_acc_f32(p(a), 0, p(B), -1, 8, 3, p(C), 3, 0, st) == EINVAL
    assert lib.msae_gemm_nt_acc_f32(p(a), 0, p(B), 5, 8, 3, p(C), 2, 0, st) == EINVAL          # ld_c < P
    assert lib.msae_gemm_nt_acc_f32(None, 0, None, 0, 8, 3, None, 3, 0, st) == 0               # M == 0: nothing to do
    assert not bool(C.any())
    # the op: in place, twice, equals the one-shot chain plus one add each; a column-sliced C keeps its neighbours
    wide = torch.full((5, 6), 2.0, device=dev)
    s = ops._dense_gemm_nt(a, B)
    ops.gemm_nt_add_(wide[:, :3], a, B)
    ops.gemm_nt_add_(wide[:, :3], a, B)
    assert torch.equal(wide[:, :3], (2.0 + s) + s) and torch.equal(wide[:, 3:], torch.full((5, 3), 2.0, device=dev))
    assert torch.equal(ops.gemm_nt_add_(torch.full((5, 3), 9.0, device=dev), a, B, accumulate=False), s)


# ---- forward -------------------------------------------------------------------------------------------------------------------------
def _sae_for(sc, dev, P=None):
    from msae import Sae, SaeConfig

    P = R.make_params(sc) if P is None else P
    sae = Sae(sc.d_in, SaeConfig(num_latents=sc.N, k=sc.k, transcode=True, skip_connection=sc.skip, multi_topk=sc.multi_topk,
                                 activation=sc.activation, batch_cap=sc.cap), device=dev, d_out=sc.d_out)
    with torch.no_grad():
        sae.encoder.weight.copy_(P["W_enc"]); sae.encoder.bias.copy_(P["b_enc"])
        sae.W_dec.copy_(P["W_dec"]); sae.b_dec.copy_(P["b_dec"])
        if sc.skip:
            sae.W_skip.copy_(P["W_skip"])
    sae.invalidate_prepared()
    return sae


def _alive_decoder(sc, P):
    P["W_dec"] = (torch.randn(sc.N, sc.d_out, generator=torch.Generator().manual_seed(sc.seed + 9)) * 0.05).float()
    return P


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
@pytest.mark.parametrize("d_out", [256, 192])
@pytest.mark.parametrize("T", [1, 5, 300])
def test_forward_against_the_restatement(dev, T, d_out, skip):
    from msae import ops

    sc = R.dataclasses.replace(R.SCENARIOS["skip" if skip else "transcoder"], T=T, d_out=d_out)
    P = _alive_decoder(sc, R.make_params(sc))
    sae = _sae_for(sc, dev, P)
    x, y = R.make_batches(sc)[0]
    out = sae(x.to(dev), y=y.to(dev))
    with torch.no_grad():
        tc = sae.transcode(x.to(dev))
    P64 = {n: R.d64(v) for n, v in P.items()}
    own = R.forward(P64, R.d64(x), R.d64(y), sc.k)
    und = R.undecided_tokens(own.pre, R.encoder_bound(P64, R.d64(x)), sc.k)
    share = R.judge_selection(out.latent_indices, own.idx, und, f"T={T}") if T >= 100 else float(und.double().mean())
    if T < 100:                                       # (one token of five is 20 %: such shapes need every token decided)
        assert share == 0.0 and torch.equal(torch.sort(out.latent_indices.cpu(), 1).values, torch.sort(own.idx, 1).values)
    # the float32 list itself: its activations within the encoder's bound of the float64 latents, then yhat within
    # n u sum |terms| of the float64 decode of THAT list -- the issue's bound, nothing added
    idx, acts = out.latent_indices.cpu(), out.latent_acts.detach().cpu()
    fw = R.forward(P64, R.d64(x), R.d64(y), sc.k, idx=idx)
    act_ratio = R.acts_within_encoder_bound(P64, R.d64(x), acts, idx)
    bound = R.yhat_bound(P64, R.d64(x), acts, idx)
    err = (out.sae_out.detach().cpu().double() - R.decode64(P64, R.d64(x), acts, idx)).abs()
    assert bool((err <= bound)[~und].all()), float((err / bound)[~und].max())
    print(f"\nT={T} d_out={d_out} skip={skip}: yhat max err/bound {float((err / bound)[~und].max()):.4f}, activations "
          f"{act_ratio:.4f} of the encoder bound, undecided {share:.4f}")
    if T > 1:                                         # (one token has no variance: fvu is 0 / 0 there, as in the reference)
        assert abs(float(out.fvu.detach()) - float(fw.fvu)) <= 1e-4 * float(fw.fvu)
    assert out.sae_out.shape == (T, d_out) and out.sae_out.dtype == torch.float32
    dec = ops.decode(out.latent_indices, out.latent_acts.detach(), sae.W_dec.detach(), sae.b_dec.detach())
    if not skip:
        assert torch.equal(out.sae_out.detach(), dec), "without a skip connection yhat IS ops.decode on the same list"
    else:
        assert torch.equal(out.sae_out.detach(), ops.gemm_nt_add_(dec, x.to(dev), sae.W_skip.detach()))
    assert torch.equal(tc, out.sae_out.detach()), "Sae.transcode and the forward's reconstruction are the same bits"


# ---- gradients -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["transcoder", "skip", "skip_auxk_dead", "skip_batchtopk"])
def test_gradients_against_float64_autograd(dev, name):
    sc = R.SCENARIOS[name]
    P = _alive_decoder(sc, R.make_params(sc))
    sae = _sae_for(sc, dev, P)
    x, y = R.make_batches(sc)[0]
    dead = R.initial_counts(sc) > sc.dead_feature_threshold if sc.auxk_alpha else None
    P64 = {n: R.d64(v) for n, v in P.items()}
    kw = dict(multi_topk=sc.multi_topk, dead_mask=dead, auxk_alpha=sc.auxk_alpha, activation=sc.activation, cap=sc.cap)
    # the tokens float64 leaves undecided are left out of the batch (at most 1 %), so that both sides select alike.  A
    # batch-level threshold moves whenever a token leaves, so "batchtopk" keeps its batch: the float64 side adopts the lists
    # and kept lengths of the GPU, which must equal its own outside the undecided tokens (at most 1 % again)
    width, T0 = sc.k if sc.activation == "topk" else sc.cap, x.shape[0]
    for _ in range(8):
        own = R.forward(P64, R.d64(x), R.d64(y), sc.k, **kw)
        bound = R.encoder_bound(P64, R.d64(x))
        und = R.undecided_tokens(own.pre, bound, width)
        if sc.multi_topk:
            und = und | R.undecided_tokens(own.pre, bound, 4 * sc.k)
        if sc.activation == "batchtopk":
            raw, b = torch.gather(own.pre, 1, own.idx), torch.gather(bound, 1, own.idx)
            und = ((raw > 0) & ((raw - own.theta).abs() <= 2 * b)).any(1) | ((own.lengths == width) & und)
        if not bool(und.any()) or sc.activation == "batchtopk":
            break
        x, y = x[~und], y[~und]
    if sc.activation == "batchtopk":
        assert float(und.double().mean()) <= R.TIE_CAP, float(und.double().mean())
    else:
        assert not bool(und.any()) and T0 - x.shape[0] <= R.TIE_CAP * T0, (T0, x.shape[0])
    xg = x.to(dev).requires_grad_(True)
    out = sae(xg, None if dead is None else dead.to(dev), y=y.to(dev))
    (out.fvu + sc.auxk_alpha * out.auxk_loss + out.multi_topk_fvu / 8).backward()
    if sc.activation == "batchtopk":
        idx, lengths = out.latent_indices.cpu(), out.lengths.cpu().long()
        assert torch.equal(torch.sort(idx, 1).values[~und], torch.sort(own.idx, 1).values[~und])
        assert torch.equal(lengths[~und], own.lengths[~und])
        kw.update(idx=idx, keep=torch.arange(width)[None] < lengths[:, None])
    fw, g, gx = R.gradients(P64, R.d64(x), R.d64(y), sc.k, want_x=True, **kw)
    got = {"W_enc": sae.encoder.weight.grad, "b_enc": sae.encoder.bias.grad, "W_dec": sae.W_dec.grad, "b_dec": sae.b_dec.grad}
    if sc.skip:
        got["W_skip"] = sae.W_skip.grad
        assert float(got["W_skip"].abs().max()) > 0
    worst = {n: R.grads_close(got[n], ref, f"{name} {n}") for n, ref in g.items()}
    worst["x"] = R.grads_close(xg.grad, gx, f"{name} x")
    print(f"\n{name}: gradient max err/tol " + " ".join(f"{n} {v:.4f}" for n, v in worst.items()))
    # b_dec gets nothing from the encoder side: its gradient is the decoder side's alone, sum_t dL/dyhat (+ the AuxK decode's)
    if not sc.auxk_alpha:
        e = fw.yhat.detach() - R.d64(y)
        tv = float((R.d64(y) - R.d64(y).mean(0)).pow(2).sum())
        R.grads_close(got["b_dec"], 2 * e.sum(0) / tv, f"{name} b_dec is the decoder side's alone")


# ---- trajectories --------------------------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self, monkeypatch):
        from msae import ops

        self.adam, self.sel, self.bsel = [], [], []
        real_adam, real_se, real_bs = ops.adam_rows_, ops.sparse_encode, ops.batch_select

        def adam_rows_(p, g, m, v, step, lr, **kw):
            rec = {"ptr": p.data_ptr(), "before": tuple(t.detach().clone() for t in (p, g, m, v)), "step": step, "lr": lr,
                   "project": kw.get("project"), "renorm_eps": kw.get("renorm_eps")}
            real_adam(p, g, m, v, step, lr, **kw)
            rec["after"] = p.detach().clone()
            self.adam.append(rec)

        def sparse_encode(x, W_enc, b_enc, b_dec, k, dead_mask=None, k_aux=0, k_multi=0, **kw):
            assert b_dec is None, "the encoder of a transcoder must not see b_dec"
            out = real_se(x, W_enc, b_enc, b_dec, k, dead_mask, k_aux, k_multi, **kw)
            self.sel.append({"sel": [i.detach().clone() for _, i in out], "k_aux": k_aux, "k_multi": k_multi})
            return out

        def batch_select(acts, idx, k):
            out = real_bs(acts, idx, k)
            self.bsel.append(out[1].detach().clone())            # the lengths
            return out

        monkeypatch.setattr(ops, "adam_rows_", adam_rows_)
        monkeypatch.setattr(ops, "sparse_encode", sparse_encode)
        monkeypatch.setattr(ops, "batch_select", batch_select)

    def clear(self):
        self.adam, self.sel, self.bsel = [], [], []


@pytest.mark.parametrize("name", sorted(R.SCENARIOS))
def test_trajectory(dev, monkeypatch, name):
    from msae import Sae
    from msae.train import SaeTrainStep

    sc = R.SCENARIOS[name]
    sae = _sae_for(sc, dev)
    ts = SaeTrainStep(sae, lr=sc.lr, auxk_alpha=sc.auxk_alpha, dead_feature_threshold=sc.dead_feature_threshold,
                      grad_acc_steps=sc.grad_acc_steps, micro_acc_steps=sc.micro_acc_steps, auxk_path="subset")
    # every step runs under sync-debug "error".  The forward's one documented host read with a dead mask -- the length of the
    # dead list (Sae._dead_list) -- is let through, counted, and must be the only one (tests/test_gpu_subset.py's pattern)
    real_dead_list, reads = Sae._dead_list, []

    def dead_list(mask):
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("default")
        try:
            reads.append(1)
            return real_dead_list(mask)
        finally:
            torch.cuda.set_sync_debug_mode(prev)

    monkeypatch.setattr(Sae, "_dead_list", staticmethod(dead_list))
    ts.num_tokens_since_fired.copy_(R.initial_counts(sc))
    gpu = {"W_enc": sae.encoder.weight, "b_enc": sae.encoder.bias, "W_dec": sae.W_dec, "b_dec": sae.b_dec}
    if sc.skip:
        gpu["W_skip"] = sae.W_skip
    assert len(ts.params) == len(gpu)
    name_of = {p.data_ptr(): n for n, p in gpu.items()}
    slot = {n: next(i for i, q in enumerate(ts.params) if q is p) for n, p in gpu.items()}
    ref = R.Loop(sc, R.make_params(sc))
    spy = _Spy(monkeypatch)
    worst = {"gradient": 0.0, "update": 0.0, "undecided": 0.0}
    width = sc.k if sc.activation == "topk" else sc.cap
    dead_seen = []
    batches = [(x.to(dev), y.to(dev)) for x, y in R.make_batches(sc)]
    for b, (x, y) in enumerate(batches):
        if b % sc.grad_acc_steps == 0:
            ref.load_state(gpu, {n: ts.exp_avg[slot[n]] for n in gpu}, {n: ts.exp_avg_sq[slot[n]] for n in gpu})
        moments = {n: (ts.exp_avg[slot[n]].clone(), ts.exp_avg_sq[slot[n]].clone()) for n in gpu}
        spy.clear()
        torch.cuda.synchronize()
        reads.clear()
        torch.cuda.set_sync_debug_mode("error")
        try:
            res = ts.step(x, y)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert reads == ([1] * sc.micro_acc_steps if sc.auxk_alpha else []), (name, b, reads)
        what = f"{name} batch {b}"
        # (a) the selections, chunk by chunk: judged against the float64 loop's own, then adopted
        assert len(spy.sel) == sc.micro_acc_steps and len(spy.bsel) == (sc.micro_acc_steps if sc.activation == "batchtopk" else 0)
        given = []
        for ci, c in enumerate(spy.sel):
            sel = [i.cpu() for i in c["sel"]]
            gv = {"idx": sel[0]}
            if c["k_aux"]:
                gv["aux_idx"] = sel[1]
            if c["k_multi"]:
                gv["multi_idx"] = sel[-1]
            if sc.activation == "batchtopk":
                gv["keep"] = torch.arange(width)[None] < spy.bsel[ci].cpu().reshape(-1, 1)
            given.append(gv)
        ref_dead = ref.counts > sc.dead_feature_threshold                 # the mask this batch's forward ran with
        want = ref.batch(x.cpu(), y.cpu(), selections=given)
        und_all = []
        for ci, (gv, sw) in enumerate(zip(given, want.sel)):
            und = sw["undecided"]
            if sc.multi_topk:
                und = und | R.undecided_tokens(sw["pre"], sw["bound"], 4 * sc.k)
            own = R.canonical_topk(sw["pre"], width)[1]
            wrong = (torch.sort(gv["idx"], 1).values != torch.sort(own, 1).values).any(1) & ~und
            assert not bool(wrong.any()), (what, ci, "main selection", int(wrong.sum()))
            if "multi_idx" in gv:
                own4 = R.canonical_topk(sw["pre"], 4 * sc.k)[1]
                wrong = (torch.sort(gv["multi_idx"], 1).values != torch.sort(own4, 1).values).any(1) & ~und
                assert not bool(wrong.any()), (what, ci, "Multi-TopK selection", int(wrong.sum()))
            if "aux_idx" in gv:
                # AuxK: over the dead set; ties at zero carry neither value nor gradient, so the float64 VALUES of the adopted
                # list must be the float64 top values within the two entries' bounds
                dead = ref_dead
                assert bool(dead[gv["aux_idx"]].all()), (what, ci, "an AuxK entry is not dead")
                masked = torch.where(dead[None], sw["pre"], torch.full((), -float("inf"), dtype=R.F64))
                top = R.canonical_topk(masked, gv["aux_idx"].shape[1])[0]
                mine = torch.sort(torch.gather(sw["pre"], 1, gv["aux_idx"]), 1, descending=True).values
                assert bool(((top - mine).abs() <= 2 * sw["bound"].max(1, keepdim=True).values).all()), (what, ci, "AuxK selection")
            if sc.activation == "batchtopk":
                keep64, _ = R.batch_keep(torch.gather(sw["pre"], 1, own), sc.k)
                assert torch.equal(keep64.sum(1)[~und], gv["keep"].sum(1)[~und]), (what, ci, "kept lengths")
            und_all.append(und)
        share = float(torch.cat(und_all).double().mean())
        assert share <= R.TIE_CAP, (what, "undecided share", share)
        worst["undecided"] = max(worst["undecided"], share)
        dead_seen.append(want.num_dead)
        assert bool(res["stepped"]) == want.stepped and ts.t == ref.t, what
        # (b), (c)
        if want.stepped:
            assert sorted(name_of[c["ptr"]] for c in spy.adam) == sorted(gpu), what
            for c in spy.adam:       # the decoder of a transcoder is never projected or renormalised, whatever the config says
                assert not c["project"] and c["renorm_eps"] is None and c["step"] == ref.t, (what, name_of[c["ptr"]])
            rec = {name_of[c["ptr"]]: c for c in spy.adam}
            w = R.judge_step({n: rec[n]["before"][1] for n in gpu}, {n: rec[n]["before"][0] for n in gpu},
                             {n: rec[n]["after"] for n in gpu}, moments, want, ref.t, sc.lr, what)
            for key in w:
                worst[key] = max(worst[key], w[key])
        else:
            assert not spy.adam, what
            for n, p in gpu.items():
                worst["gradient"] = max(worst["gradient"], R.grads_close(p.grad, want.G[n] * want.clip, f"{what} {n}.grad after the clip"))
    norms = sae.W_dec.detach().norm(dim=1)
    assert float(norms.max()) > 0 and not bool(((norms - 1).abs() < 1e-3).any()), "W_dec must not hold unit-norm rows"
    if sc.auxk_alpha:
        assert 0 < dead_seen[0] < sc.d_out // 2 < dead_seen[-1], dead_seen
    print(f"\n{name}: max err/tol " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()) + f"; dead {dead_seen}")


# ---- the hook ------------------------------------------------------------------------------------------------------------------------
def test_hook_on_the_fake_model(dev):
    from fakes import TinyLlava
    from msae import Sae, SaeConfig
    from msae.features import FeatureEdits, transcoder_hook

    d, N, k = 64, 8192, 32
    model = TinyLlava(d=d).to(dev)
    layer = model.language_model.layers[1]
    sae = Sae(d, SaeConfig(num_latents=N, k=k, transcode=True, skip_connection=True), device=dev)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        sae.W_dec.copy_(torch.randn(N, d, generator=g) * 0.05)
        sae.W_skip.copy_(torch.randn(d, d, generator=g) * 0.05)
        sae.b_dec.copy_(torch.randn(d, generator=g))
    sae.eval()
    seen = []
    probe = layer.register_forward_hook(lambda m, i, o: seen.append(i[0].detach().clone()))
    ids = torch.tensor([[1, 5, 9, 4, 7, 3]], device=dev)
    edits = FeatureEdits(N, set={3: 50.0}, device=dev)
    with torch.no_grad():
        plain_handles = transcoder_hook(sae, layer)
        out_plain = model(input_ids=ids)["last_hidden_state"]
        assert torch.equal(out_plain, sae.transcode(seen[-1]).to(torch.float16))
        for h in plain_handles:
            h.remove()
        handles = transcoder_hook(sae, layer, edits=edits)
        assert handles[0].step_graph is None
        out = model(input_ids=ids)["last_hidden_state"]
        assert torch.equal(out, sae.transcode(seen[-1], edits=edits).to(torch.float16)) and not torch.equal(out, out_plain)
        step = model(input_ids=ids[:, :1])["last_hidden_state"]                       # S = 1: no edit, eager
        assert step.shape == (1, 1, d) and torch.equal(step, sae.transcode(seen[-1]).to(torch.float16))
    for h in handles:
        h.remove()
    probe.remove()


# ---- the threshold modes: Sae.transcode's kept-length branch, and a "jump" transcoder in training -----------------------------------------
@pytest.mark.parametrize("activation", ["batchtopk", "jump"])
def test_transcode_and_training_steps_of_the_threshold_modes(dev, activation):
    """Sae.transcode of a "batchtopk" / "jump" skip transcoder is, bit for bit, encode(return_lengths) -> decode(lengths) ->
    the in-place skip term; Sae.forward(x, y=) returns the mode's own output type with gradients for every parameter
    (log_threshold included); three SaeTrainStep.step(hiddens, targets) calls run under sync-debug "error" and move every
    parameter, the decoder staying un-normalised."""
    from msae import Sae, SaeConfig, ops
    from msae.train import SaeTrainStep

    sc = R.dataclasses.replace(R.SCENARIOS["skip"], k=16, steps=3)
    P = _alive_decoder(sc, R.make_params(sc))
    sae = Sae(sc.d_in, SaeConfig(num_latents=sc.N, k=sc.k, transcode=True, skip_connection=True, activation=activation,
                                 batch_cap=64, jump_init=0.1, jump_bandwidth=0.05), device=dev, d_out=sc.d_out)
    with torch.no_grad():
        sae.encoder.weight.copy_(P["W_enc"]); sae.encoder.bias.copy_(P["b_enc"])
        sae.W_dec.copy_(P["W_dec"]); sae.b_dec.copy_(P["b_dec"]); sae.W_skip.copy_(P["W_skip"])
    sae.invalidate_prepared()
    if activation == "batchtopk":
        sae.set_threshold(0.1)
    batches = [(x.to(dev), y.to(dev)) for x, y in R.make_batches(sc)]
    x, y = batches[0]
    with torch.no_grad():
        got = sae.transcode(x)
        enc, lengths = sae.encode(x, return_lengths=True)
        want = ops.gemm_nt_add_(ops.decode(enc.top_indices, enc.top_acts, sae.W_dec, sae.b_dec, lengths), x, sae.W_skip)
    assert got.shape == (sc.T, sc.d_out) and torch.equal(got, want)
    assert bool((lengths > 0).any()) and bool((lengths < 64).any()), "the kept lengths must vary for the branch to mean anything"
    out = sae(x, y=y)
    assert type(out).__name__ == ("JumpForwardOutput" if activation == "jump" else "BatchForwardOutput")
    (out.fvu + (0.01 * out.l0 if activation == "jump" else 0.0)).backward()
    for n, p in sae.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    sae.zero_grad(set_to_none=True)
    ts = SaeTrainStep(sae, lr=sc.lr, l0_alpha=0.01 if activation == "jump" else 0.0)
    assert len(ts.params) == (6 if activation == "jump" else 5)
    before = {n: p.detach().clone() for n, p in sae.named_parameters()}
    ts.step(*batches[0])                                   # (workspaces and operand buffers exist before the strict steps)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for xb, yb in batches[1:]:
            res = ts.step(xb, yb)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(res["stepped"]) and bool(torch.isfinite(res["fvu"])) and (activation != "jump" or float(res["l0"]) > 0)
    for n, p in sae.named_parameters():
        assert not torch.equal(p.detach(), before[n]) and bool(torch.isfinite(p).all()), n
    norms = sae.W_dec.detach().norm(dim=1)
    assert not bool(((norms - 1).abs() < 1e-3).any())
