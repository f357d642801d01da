"""Transcoders without a GPU: the configuration and the files, every refusal, the float64 restatement
(tests/transcoder_ref.py) against a hand-computed case, Sae.forward(x, y=) and its gradients on the host through the two seams
the other host tests use (a dense encoder for ops.sparse_encode, a dense decoder_impl; the skip term's host route is a
float32 matmul, so the comparison is inside derived bounds, not bit for bit), the hook on the fake model, and the power of
the trajectory criterion: three wrong trainers are rejected, the right one passes."""
import contextlib
import json

import pytest
import torch

import transcoder_ref as R

F64 = torch.float64


def _dense_seams(monkeypatch, subtract_b_dec_probe=None):
    """ops.sparse_encode and the decoder seam in dense torch ops (float32, autograd through torch)."""
    from msae import ops
    from msae.sae import utils as seam

    def sparse_encode(x, W_enc, b_enc, b_dec, k, dead_mask=None, k_aux=0, k_multi=0, **kw):
        if subtract_b_dec_probe is not None:
            subtract_b_dec_probe.append(b_dec)
        pre = torch.relu((x if b_dec is None else x - b_dec) @ W_enc.T + b_enc)
        out = [tuple(t[:, :k] for t in torch.sort(pre, dim=1, descending=True, stable=True))]
        if k_aux:
            dead = torch.where(dead_mask[None], pre, torch.full((), -torch.inf))
            out.append(tuple(t[:, :k_aux] for t in torch.sort(dead, dim=1, descending=True, stable=True)))
        if k_multi:
            out.append(tuple(t[:, :k_multi] for t in torch.sort(pre, dim=1, descending=True, stable=True)))
        return out

    monkeypatch.setattr(ops, "sparse_encode", sparse_encode)
    monkeypatch.setattr(seam, "decoder_impl", lambda idx, acts, W_T: (acts[..., None] * W_T.mT[idx]).sum(-2))


def _load(sae, P):
    with torch.no_grad():
        sae.encoder.weight.copy_(P["W_enc"]); sae.encoder.bias.copy_(P["b_enc"])
        sae.W_dec.copy_(P["W_dec"]); sae.b_dec.copy_(P["b_dec"])
        if P.get("W_skip") is not None:
            sae.W_skip.copy_(P["W_skip"])


def _sae_for(sc, device="cpu"):
    from msae import Sae, SaeConfig

    sae = Sae(sc.d_in, SaeConfig(num_latents=sc.N, k=sc.k, transcode=True, skip_connection=sc.skip, multi_topk=sc.multi_topk,
                                 activation=sc.activation, batch_cap=sc.cap), device=device, d_out=sc.d_out)
    _load(sae, R.make_params(sc))
    return sae


# ---- configuration and files ------------------------------------------------------------------------------------------------------
def test_config_validation_and_round_trip():
    from msae import SaeConfig

    assert SaeConfig().to_dict() == {"expansion_factor": 32, "normalize_decoder": True, "num_latents": 0, "k": 32,
                                     "multi_topk": False, "signed": False}
    with pytest.raises(ValueError, match="transcode"):
        SaeConfig(skip_connection=True)
    with pytest.raises(ValueError, match="follow-up"):
        SaeConfig(transcode=True, num_latents=64, matryoshka=[16, 64])
    with pytest.raises(ValueError, match="bool"):
        SaeConfig(transcode=1)
    for kw in (dict(transcode=True), dict(transcode=True, skip_connection=True),
               dict(transcode=True, skip_connection=True, activation="batchtopk", k=4, batch_cap=8),
               dict(transcode=True, activation="jump", k=4)):
        cfg = SaeConfig(num_latents=64, **kw)
        d = cfg.to_dict()
        assert d["transcode"] is True and ("skip_connection" in d) == bool(kw.get("skip_connection"))
        assert SaeConfig.from_dict(json.loads(json.dumps(d))) == cfg


def test_files_of_a_plain_sae_are_untouched_and_a_transcoder_round_trips(tmp_path):
    from safetensors.torch import load_file

    from msae import Sae, SaeConfig

    plain = Sae(16, SaeConfig(num_latents=64, k=4))
    assert sorted(plain.state_dict()) == ["W_dec", "b_dec", "encoder.bias", "encoder.weight"] and plain.d_out == 16
    plain.save_to_disk(tmp_path / "plain")
    assert json.loads((tmp_path / "plain" / "cfg.json").read_text()) == {
        "expansion_factor": 32, "normalize_decoder": True, "num_latents": 64, "k": 4, "multi_topk": False, "signed": False,
        "d_in": 16}
    with pytest.raises(ValueError, match="transcode"):
        Sae(16, SaeConfig(num_latents=64, k=4), d_out=12)

    tc = Sae(16, SaeConfig(num_latents=64, k=4, transcode=True, skip_connection=True), d_out=12)
    assert tc.W_dec.shape == (64, 12) and tc.b_dec.shape == (12,) and tc.W_skip.shape == (12, 16) and tc.d_out == 12
    assert not tc.W_dec.any() and not tc.W_skip.any() and tc.W_skip.dtype == torch.float32     # zeros, NOT normalised
    with torch.no_grad():
        for p in tc.parameters():
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    tc.save_to_disk(tmp_path / "tc")
    cfg = json.loads((tmp_path / "tc" / "cfg.json").read_text())
    assert cfg["transcode"] is True and cfg["skip_connection"] is True and cfg["d_out"] == 12 and cfg["d_in"] == 16
    assert sorted(load_file(tmp_path / "tc" / "sae.safetensors")) == ["W_dec", "W_skip", "b_dec", "encoder.bias", "encoder.weight"]
    back = Sae.load_from_disk(tmp_path / "tc")
    assert back.cfg == tc.cfg and back.d_out == 12 and back.d_in == 16
    for (n, a), (_, b) in zip(tc.named_parameters(), back.named_parameters()):
        assert torch.equal(a, b), n
    no_skip = Sae(16, SaeConfig(num_latents=64, k=4, transcode=True))
    assert not hasattr(no_skip, "W_skip") and "W_skip" not in no_skip.state_dict() and no_skip.d_out == 16


def test_every_path_that_cannot_serve_a_transcoder_says_so():
    from msae import Sae, SaeConfig
    from msae.features import FeatureEdits, hooks
    from msae.features.patching.utils import sae_splice_hook
    from msae.parallel import ShardedSae

    sae = Sae(16, SaeConfig(num_latents=64, k=4, transcode=True, skip_connection=True), d_out=12)
    mod = torch.nn.Identity()
    x = torch.randn(3, 16)
    names = "transcode.*(transcoder_hook|Sae.transcode)"
    for fn in (lambda: hooks.sae_reconstruct(sae, x), lambda: hooks.clamp_features_max(sae, 3, mod),
               lambda: hooks.clamp_features_rows(sae, [1, 2], mod), lambda: hooks.attribution_sae_hook({"m": sae}, {mod: "m"}, {}),
               lambda: sae_splice_hook({"m": sae}, {mod: "m"}, {})):
        with pytest.raises(ValueError, match=names):
            fn()
    edits = FeatureEdits(64, zero=[3], device="cpu")
    for fn in (lambda: sae.intervene(x, edits), lambda: sae.recon_error(x), lambda: sae.nested_error(x, bounds=[16, 64]),
               lambda: sae.truncate(32), lambda: ShardedSae.from_sae(sae)):
        with pytest.raises(NotImplementedError, match=names):
            fn()
    # the cache loop's reconstruction statistics compare with the encoder's input as well
    import types

    from msae.features import ReconStats
    from msae.features import cache as cache_mod

    stats = ReconStats(16, [0, 2, 4], device="cpu")
    with pytest.raises(NotImplementedError, match=names):
        stats.update(torch.randn(1, 3, 16), torch.rand(1, 3, 4), torch.zeros(1, 3, 4, dtype=torch.long), sae)
    with pytest.raises(NotImplementedError, match=names):
        cache_mod._new_recon(types.SimpleNamespace(recon={}), "m", types.SimpleNamespace(sae=sae, device="cpu"))
    with pytest.raises(ValueError, match="y="):
        sae(x)
    plain = Sae(16, SaeConfig(num_latents=64, k=4))
    with pytest.raises(ValueError, match="transcode"):
        plain(x, y=x)
    with pytest.raises(ValueError, match="transcode"):
        plain.transcode(x)
    with pytest.raises(ValueError, match="transcode"):
        hooks.transcoder_hook(plain, mod)
    with pytest.raises(ValueError, match="d_out|20"):
        sae(x, y=torch.randn(3, 20))

    from msae.train import SaeTrainStep

    with pytest.raises(ValueError, match="targets"):
        SaeTrainStep(sae, lr=1e-3).step(x)
    with pytest.raises(ValueError, match="targets"):
        SaeTrainStep(plain, lr=1e-3).step(x, x)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_the_restatement_equals_the_hand_computed_case():
    h = R.hand_case()
    fw = R.forward(h["P"], h["x"], h["y"], h["k"])
    assert torch.equal(fw.pre, h["pre"]) and torch.equal(fw.idx, h["idx"]) and torch.equal(fw.acts, h["acts"])
    assert torch.equal(fw.yhat, h["with_skip"]) and float(fw.fvu) == h["sq_err"] / h["tv"]
    no_skip = {**h["P"], "W_skip": None}
    fw = R.forward(no_skip, h["x"], h["y"], h["k"])
    assert torch.equal(fw.yhat, h["plain"]) and float(fw.fvu) == h["sq_err_plain"] / h["tv"]
    # subtracting the (large) b_dec in front of the encoder is another function: the power tests rely on that
    assert not torch.equal(R.forward(h["P"], h["x"], h["y"], h["k"], mutate=["subtract_b_dec"]).idx, h["idx"])
    # gradients by hand: d fvu / d W_skip = 2 e^T x / tv, d fvu / d b_dec = 2 sum_t e / tv; b_dec gets nothing from the encoder
    _, g, gx = R.gradients(h["P"], h["x"], h["y"], h["k"], want_x=True)
    e = h["with_skip"] - h["y"]
    assert torch.allclose(g["W_skip"], 2 * e.T @ h["x"] / h["tv"], rtol=1e-14, atol=0)
    assert torch.allclose(g["b_dec"], 2 * e.sum(0) / h["tv"], rtol=1e-14, atol=0)
    assert float(g["W_skip"].abs().max()) > 0 and float(gx.abs().max()) > 0
    # the first selected latent of token 0 is feature 0 with activation 2: d fvu / d W_dec[0] gets 2 * 2 e[0] / tv from it
    assert torch.allclose(g["W_dec"][0], 2 * 2 * e[0] / h["tv"], rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", sorted(R.SCENARIOS))
def test_the_scenarios_meet_their_preconditions_in_float64_alone(name):
    """What the GPU tests assume of the seeds, from the restatement alone: under 1 % undecided tokens in every batch, every
    parameter's gradient alive (the encoder's from the second step: W_dec starts at zero), the dead count on both sides of
    k_aux, and a decoder that is not unit-norm at the end."""
    sc = R.SCENARIOS[name]
    loop, recs = R.run_standalone(sc)
    for b, r in enumerate(recs):
        share = float(torch.cat([s["undecided"] for s in r.sel]).double().mean())
        assert share <= R.TIE_CAP, (name, b, share)
        for n, g in r.G.items():
            assert float(g.abs().max()) > 0 or (b < sc.grad_acc_steps and n in ("W_enc", "b_enc")), (name, b, n)
    if sc.auxk_alpha:
        k_aux = sc.d_out // 2
        assert 0 < recs[0].num_dead < k_aux < recs[-1].num_dead, [r.num_dead for r in recs]
    if sc.grad_acc_steps > 1:
        assert [r.stepped for r in recs] == [False, True] * sc.steps and sc.T % 2 == 1
    norms = loop.p["W_dec"].norm(dim=1)
    assert float(norms.max()) < 0.5 and float(norms.max()) > 0


# ---- Sae.forward on the host -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["transcoder", "skip", "skip_auxk_dead", "skip_batchtopk"])
def test_forward_and_gradients_on_the_host_against_the_restatement(monkeypatch, name):
    sc = R.small(R.SCENARIOS[name])
    probe = []
    _dense_seams(monkeypatch, probe)
    sae = _sae_for(sc)
    P = R.make_params(sc)
    with torch.no_grad():                      # a decoder away from zero, so that every gradient is alive
        sae.W_dec.copy_(torch.randn(sc.N, sc.d_out, generator=torch.Generator().manual_seed(3)) * 0.05)
    P["W_dec"] = sae.W_dec.detach().clone()
    x, y = R.make_batches(sc)[0]
    dead = R.initial_counts(sc) > sc.dead_feature_threshold if sc.auxk_alpha else None
    xg = x.clone().requires_grad_(True)
    out = sae(xg, dead, y=y)
    assert probe and all(b is None for b in probe), "the encoder of a transcoder must not see b_dec"
    P64 = {n: R.d64(v) for n, v in P.items()}
    kw = dict(multi_topk=sc.multi_topk, dead_mask=dead, auxk_alpha=sc.auxk_alpha, activation=sc.activation, cap=sc.cap)
    fw, g, gx = R.gradients(P64, R.d64(x), R.d64(y), sc.k, want_x=True, **kw)
    und = R.undecided_tokens(fw.pre.detach(), R.encoder_bound(P64, R.d64(x)), sc.k if sc.activation == "topk" else sc.cap)
    assert not bool(und.any())
    if not sc.multi_topk:                      # (with Multi-TopK the forward returns the 4k selection, as the reference does)
        assert torch.equal(out.latent_indices, fw.idx)
        acts = out.latent_acts.detach()
        live = None if fw.lengths is None else torch.arange(acts.shape[1])[None] < fw.lengths[:, None]
        R.acts_within_encoder_bound(P64, R.d64(x), acts, fw.idx, live)
        bound = R.yhat_bound(P64, R.d64(x), acts, fw.idx)
        assert bool(((out.sae_out.detach().double() - R.decode64(P64, R.d64(x), acts, fw.idx)).abs() <= bound).all())
    assert out.sae_out.shape == (sc.T, sc.d_out)
    for got, want in ((out.fvu, fw.fvu), (out.auxk_loss, fw.auxk), (out.multi_topk_fvu, fw.multi_fvu)):
        assert abs(float(got) - float(want)) <= 1e-4 * abs(float(want)) + 1e-12
    (out.fvu + sc.auxk_alpha * out.auxk_loss + out.multi_topk_fvu / 8).backward()
    got = {"W_enc": sae.encoder.weight.grad, "b_enc": sae.encoder.bias.grad, "W_dec": sae.W_dec.grad, "b_dec": sae.b_dec.grad}
    if sc.skip:
        got["W_skip"] = sae.W_skip.grad
        assert float(got["W_skip"].abs().max()) > 0
    for n, ref in g.items():
        R.grads_close(got[n], ref, f"{name} {n}")
    R.grads_close(xg.grad, gx, f"{name} x")


def test_skip_add_accumulates_into_an_existing_grad_and_needs_no_x_grad():
    from msae import ops

    g = torch.Generator().manual_seed(1)
    x, W = torch.randn(7, 5, generator=g), torch.randn(3, 5, generator=g).requires_grad_(True)
    seen = []
    W.register_hook(lambda grad: seen.append(grad is not None))
    for n in range(3):
        # the default route is autograd's own (a hook sees the gradient); inside skip_grad_in_place a backward that finds
        # W.grad adds into it with the GEMM and hands autograd None
        base = torch.zeros(7, 3, requires_grad=True)
        out = ops.skip_add(base * 1.0, x, W)
        with (ops.skip_grad_in_place() if n == 1 else contextlib.nullcontext()):
            out.pow(2).sum().backward()
    assert seen == [True, False, True], seen
    want = 3 * 2 * (x @ W.detach().T).T @ x
    assert torch.allclose(W.grad, want, rtol=1e-5, atol=1e-6) and torch.allclose(base.grad, 2 * x @ W.detach().T, rtol=1e-5, atol=1e-6)
    C = torch.full((4, 6), 7.0)
    ops.gemm_nt_add_(C[:, :3], torch.ones(4, 2), torch.ones(3, 2))
    assert torch.equal(C[:, :3], torch.full((4, 3), 9.0)) and torch.equal(C[:, 3:], torch.full((4, 3), 7.0))
    with pytest.raises(ValueError):
        ops.gemm_nt_add_(C.t(), torch.ones(6, 2), torch.ones(4, 2))


# ---- the hook ----------------------------------------------------------------------------------------------------------------------
def test_the_hook_replaces_the_output_by_the_transcoded_input_and_edits_on_prefill_only(monkeypatch):
    from fakes import TinyLlava
    from msae import Sae, SaeConfig
    from msae.features import FeatureEdits, transcoder_hook

    model = TinyLlava(d=64)
    layer = model.language_model.layers[1]
    sae = Sae(64, SaeConfig(num_latents=256, k=4, transcode=True, skip_connection=True))
    calls = []

    def transcode(x, *, edits=None, edit_group=None, exact=False):
        calls.append((tuple(x.shape), edits))
        return x.float() * 2.0 + (1.0 if edits is not None else 0.0)

    monkeypatch.setattr(sae, "transcode", transcode)
    edits = FeatureEdits(256, set={3: 5.0}, device="cpu")
    seen = {}
    probe = layer.register_forward_hook(lambda m, i, o: (seen.setdefault("x", i[0]), seen.setdefault("old", o)) and None)
    handles = transcoder_hook(sae, layer, edits=edits)
    ids = torch.tensor([[1, 5, 9, 4]])
    out = model(input_ids=ids)["last_hidden_state"]
    assert calls[-1] == ((1, 4, 64), edits) and out.dtype == torch.float16
    assert torch.equal(out, (seen["x"].float() * 2.0 + 1.0).to(torch.float16))
    model(input_ids=ids[:, :1])                                    # an S = 1 step: no edits, still replaced, eager
    assert calls[-1] == ((1, 1, 64), None) and handles[0].step_graph is None
    for h in handles:
        h.remove()
    probe.remove()
    assert torch.equal(model(input_ids=ids)["last_hidden_state"], seen["old"][0])


# ---- the power of the trajectory criterion -----------------------------------------------------------------------------------------
def _judge_loops(sc, under_test: R.Loop):
    """`under_test` (a float64 loop, possibly a wrong one) judged by the right loop, batch by batch, from shared state."""
    ref = R.Loop(sc, R.make_params(sc))
    failures = {}
    for b, (x, y) in enumerate(R.make_batches(sc)):
        if b % sc.grad_acc_steps == 0:
            ref.load_state(under_test.p, under_test.m, under_test.v)
        before = {n: v.clone() for n, v in under_test.p.items()}
        moments = {n: (under_test.m[n].clone(), under_test.v[n].clone()) for n in before}
        got = under_test.batch(x, y)
        want = ref.batch(x, y)
        # every check of every batch runs (the shared state makes each batch its own judgement); the first failure of
        # each KIND is kept, so that a wrong trainer can be held to the check that is meant to catch it
        for ci, (sg, sw) in enumerate(zip(got.sel, want.sel)):
            try:
                R.judge_selection(sg["idx"], sw["idx"], sw["undecided"], f"batch {b} chunk {ci}")
            except AssertionError as e:
                failures.setdefault("selection", str(e))
        try:
            R.judge_step(got.G, before, got.params, moments, want, ref.t, sc.lr, f"batch {b}")
        except AssertionError as e:
            failures.setdefault("step", str(e))
    norms = under_test.p["W_dec"].norm(dim=1)
    if bool(((norms - 1).abs() < 1e-3).any()):
        failures.setdefault("decoder", "W_dec holds unit-norm rows: a transcoder's decoder is never normalised")
    assert not failures, " | ".join(f"[{k}] {v}" for k, v in failures.items())


@pytest.mark.parametrize("mutation, caught_by", [(None, None), ("subtract_b_dec", r"\[selection\].*another selection"),
                                                 ("normalize_decoder", r"\[decoder\].*unit-norm rows"),
                                                 ("drop_skip_grad", r"\[step\].*gradient of W_skip")])
def test_the_trajectory_criterion_rejects_wrong_trainers(mutation, caught_by):
    sc = R.small(R.SCENARIOS["skip"])
    sc = R.dataclasses.replace(sc, d_out=sc.d_in)              # (b_dec can only be subtracted from x where the widths agree)
    loop = R.Loop(sc, R.make_params(sc), [mutation] if mutation else [])
    if mutation is None:
        _judge_loops(sc, loop)
        return
    with pytest.raises(AssertionError, match=caught_by):
        _judge_loops(sc, loop)


@pytest.mark.parametrize("name", ["skip", "skip_accumulate"])
def test_the_trainer_on_the_host_passes_the_trajectory_criterion(monkeypatch, name):
    """SaeTrainStep.step(hiddens, targets) itself -- chunking of the targets, no renormalisation, W_skip among the parameters,
    the in-place accumulation of its gradient -- in float32 on the host (dense seams, torch's Adam formula as the update)."""
    from msae.train import SaeTrainStep

    sc = R.small(R.SCENARIOS[name])
    _dense_seams(monkeypatch)
    sae = _sae_for(sc)

    class HostStep(SaeTrainStep):
        def _update(self, lr):
            self.seen = {id(p): p.grad.detach().clone() for p in self.params}
            torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
            with torch.no_grad():
                for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq):
                    p1, m1, v1 = R.adam(p, p.grad, m, v, self.t, lr)
                    p.copy_(p1); m.copy_(m1); v.copy_(v1)
                    p.grad = None

    ts = HostStep(sae, lr=sc.lr, grad_acc_steps=sc.grad_acc_steps, micro_acc_steps=sc.micro_acc_steps)
    assert any(p is sae.W_skip for p in ts.params) and not ts.normalize_decoder
    gpu = {"W_enc": sae.encoder.weight, "b_enc": sae.encoder.bias, "W_dec": sae.W_dec, "b_dec": sae.b_dec, "W_skip": sae.W_skip}
    slot = {n: next(i for i, q in enumerate(ts.params) if q is p) for n, p in gpu.items()}
    ref = R.Loop(sc, R.make_params(sc))
    for b, (x, y) in enumerate(R.make_batches(sc)):
        if b % sc.grad_acc_steps == 0:
            ref.load_state(gpu, {n: ts.exp_avg[slot[n]] for n in gpu}, {n: ts.exp_avg_sq[slot[n]] for n in gpu})
        before = {n: p.detach().clone() for n, p in gpu.items()}
        moments = {n: (ts.exp_avg[slot[n]].clone(), ts.exp_avg_sq[slot[n]].clone()) for n in gpu}
        res = ts.step(x, y)
        want = ref.batch(x, y)
        assert bool(res["stepped"]) == want.stepped
        if want.stepped:
            G = {n: ts.seen[id(p)] for n, p in gpu.items()}
            R.judge_step(G, before, {n: p.detach() for n, p in gpu.items()}, moments, want, ref.t, sc.lr, f"{name} batch {b}")
        else:
            for n, p in gpu.items():
                R.grads_close(p.grad, want.G[n] * want.clip, f"{name} batch {b} {n}.grad after the clip")
    assert float(sae.W_dec.norm(dim=1).max()) < 0.5


# ---- a "jump" transcoder -----------------------------------------------------------------------------------------------------------
def _jump_sae(sc, device="cpu"):
    from msae import Sae, SaeConfig

    sae = Sae(sc.d_in, SaeConfig(num_latents=sc.N, k=sc.k, transcode=True, skip_connection=True, activation="jump", batch_cap=12,
                                 jump_init=0.2, jump_bandwidth=0.1), device=device, d_out=sc.d_out)
    P = R.make_params(sc)
    P["W_dec"] = torch.randn(sc.N, sc.d_out, generator=torch.Generator().manual_seed(3)) * 0.05
    _load(sae, P)
    return sae, P


def test_a_jump_transcoder_forward_and_gradients_on_the_host(monkeypatch):
    """Sae.forward(x, y=) of a "jump" skip transcoder (float32, dense seams) against the same composition on float64 leaves:
    the partitioned lists exactly, yhat, fvu and every gradient -- log_threshold's and W_skip's alive, b_dec unseen by the
    encoder."""
    from msae import ops

    sc = R.small(R.SCENARIOS["skip"])
    probe = []
    _dense_seams(monkeypatch, probe)
    sae, P = _jump_sae(sc)
    x, y = R.make_batches(sc)[0]
    out = sae(x, y=y)
    assert type(out).__name__ == "JumpForwardOutput" and probe and all(b is None for b in probe)
    assert bool((out.lengths > 0).any()) and bool((out.reach > out.lengths).any()) and bool((out.lengths < 12).any())
    (out.fvu + 0.02 * out.l0).backward()

    L = {n: R.d64(v).requires_grad_(True) for n, v in P.items()}
    lt = sae.log_threshold.detach().double().requires_grad_(True)
    x64, y64 = R.d64(x), R.d64(y)
    pre = torch.relu(x64 @ L["W_enc"].T + L["b_enc"])
    acts, idx = (t[:, :12] for t in torch.sort(pre, dim=1, descending=True, stable=True))
    kept, io, ln, reach, l0, _ = ops.jump_select(acts, idx, lt.exp(), sae.cfg.jump_bandwidth)
    yhat = (kept[..., None] * L["W_dec"][io]).sum(1) + L["b_dec"] + x64 @ L["W_skip"].T
    fvu = (yhat - y64).pow(2).sum() / (y64 - y64.mean(0)).pow(2).sum()
    (fvu + 0.02 * l0 / x.shape[0]).backward()
    assert torch.equal(out.latent_indices, io) and torch.equal(out.lengths, ln) and torch.equal(out.reach, reach)
    assert abs(float(out.fvu) - float(fvu)) <= 1e-4 * float(fvu)
    assert float((out.sae_out.detach().double() - yhat.detach()).abs().max()) <= 1e-4 * float(yhat.detach().abs().max())
    got = {"W_enc": sae.encoder.weight.grad, "b_enc": sae.encoder.bias.grad, "W_dec": sae.W_dec.grad, "b_dec": sae.b_dec.grad,
           "W_skip": sae.W_skip.grad}
    for n in got:
        R.grads_close(got[n], L[n].grad, f"jump {n}")
    R.grads_close(sae.log_threshold.grad, lt.grad, "jump log_threshold")
    assert float(lt.grad.abs().max()) > 0 and float(L["W_skip"].grad.abs().max()) > 0
