"""SaeTrainStep(optimizer="lion").step over several batches against tests/lion_trainer_ref.py, the float64 restatement of the
training loop with the sign-momentum optimiser.  The method is test_gpu_train_trajectory.py's: a spy records every
ops.lion_rows_ call (clones of p, g, m before it, lr, the keywords; p, m after it), every selection ops.sparse_encode returns
with the dead mask it was given, and which of ops.sum_into_ / ops.grad_sumsq_ built the gradient norm; ops.adam_rows_ must
never be called.  Before every optimiser window the restatement takes the GPU's float32 parameters and momentum; its
bookkeeping is never synchronised.  Per batch:

  a. selections   each recorded selection is a valid top-k of the float64 pre-activations within b_t and is adopted; the share
                  of near-ties is at most 1 % (test_lion_trainer_ref_host.py shows the scenarios meet that from float64 alone
                  at lion_trainer_ref.LION_LR);
  b. arguments    lr and betas of every lion_rows_ call equal the float32 value of the restatement's scheduled lr and the
                  configured betas; project / renorm_eps / refresh / tokens_next are what the configuration implies;
  c. gradients    every recorded g (on a batch that does not step: p.grad after the in-place clip) within dG of G64;
  d. norm         ts._sumsq within train_ref.grad_sumsq's bound of sum G_gpu^2, by the expected ops calls;
  e. update       every pass, fed the GPU's own G and norm, passes lion_ref's acceptance rule: W' bit-equal to
                  float32(w - lr s) with s = sign(u64) wherever float64 decides it, M' within its bound, the undecided share
                  under the cap.  The signs of a pass with fused tails are read from a run of ops.lion_rows_ WITHOUT tails
                  on clones of the recorded inputs (test_gpu_lion.py shows the two give the same bits): its M' must equal
                  the recorded M' bit for bit, its W' the recorded one (operand refresh) or, with the renorm, the recorded W'
                  lies within train_ref._renorm's bound of the renormalised adopted rows;
  f. bookkeeping  num_tokens_since_fired, t, global_step, `stepped` and the dead mask equal the restatement's exactly; the
                  statistics within their propagated bounds.

Every scenario asserts its preconditions on the restatement's values and prints its largest error / bound per check."""
import gc

import pytest
import torch

import lion_ref as L
import lion_trainer_ref as LR
import train_ref as tr
import trainer_ref as R

pytestmark = pytest.mark.gpu

EPS32 = float(torch.finfo(torch.float32).eps)


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


class _Spy:
    def __init__(self, monkeypatch):
        from msae import ops

        self.lion, self.sel, self.norm_calls = [], [], []
        self.real_lion = ops.lion_rows_
        real_se, real_sum, real_gss = ops.sparse_encode, ops.sum_into_, ops.grad_sumsq_

        def lion_rows_(p, g, m, lr, **kw):
            rec = {"ptr": p.data_ptr(), "before": tuple(t.detach().clone() for t in (p, g, m)), "lr": lr,
                   "kw": {k: val for k, val in kw.items() if k not in ("total_sumsq", "refresh")},
                   "has_sumsq": kw.get("total_sumsq") is not None, "refresh": kw.get("refresh") is not None}
            self.real_lion(p, g, m, lr, **kw)
            rec["after"] = tuple(t.detach().clone() for t in (p, m))
            self.lion.append(rec)

        def adam_rows_(*a, **kw):
            raise AssertionError("ops.adam_rows_ was called under optimizer='lion'")

        def sparse_encode(x, W_enc, b_enc, b_dec, k, dead_mask=None, k_aux=0, k_multi=0, **kw):
            out = real_se(x, W_enc, b_enc, b_dec, k, dead_mask, k_aux, k_multi, **kw)
            self.sel.append({"sel": [(a.detach().cpu(), i.detach().cpu()) for a, i in out],
                             "dead_mask": None if dead_mask is None else dead_mask.detach().cpu()})
            return out

        def sum_into_(accum, v):
            self.norm_calls.append("sum_into_")
            return real_sum(accum, v)

        def grad_sumsq_(accum, g):
            self.norm_calls.append("grad_sumsq_")
            return real_gss(accum, g)

        monkeypatch.setattr(ops, "lion_rows_", lion_rows_)
        monkeypatch.setattr(ops, "adam_rows_", adam_rows_)
        monkeypatch.setattr(ops, "adam8_rows_", adam_rows_)
        monkeypatch.setattr(ops, "sparse_encode", sparse_encode)
        monkeypatch.setattr(ops, "sum_into_", sum_into_)
        monkeypatch.setattr(ops, "grad_sumsq_", grad_sumsq_)

    def clear(self):
        self.lion, self.sel, self.norm_calls = [], [], []


def _run(dev, monkeypatch, sc: R.Scenario, fuse: bool = True):
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    cfg = sc.cfg
    init = R.make_params(sc)
    sae = Sae(sc.d, SaeConfig(num_latents=sc.N, k=cfg.k, multi_topk=cfg.multi_topk, normalize_decoder=cfg.normalize_decoder),
              device=dev)
    gpu = {"W_enc": sae.encoder.weight, "b_enc": sae.encoder.bias, "W_dec": sae.W_dec, "b_dec": sae.b_dec}
    with torch.no_grad():
        for n in R.NAMES:
            gpu[n].copy_(init[n])
    sae.invalidate_prepared()
    ts = SaeTrainStep(sae, lr=cfg.lr, auxk_alpha=cfg.auxk_alpha, dead_feature_threshold=cfg.dead_feature_threshold,
                      grad_acc_steps=cfg.grad_acc_steps, micro_acc_steps=cfg.micro_acc_steps,
                      lr_warmup_steps=cfg.lr_warmup_steps, total_steps=cfg.total_steps, fuse_next_step=fuse,
                      optimizer="lion", betas=cfg.betas)
    assert all(v is None for v in ts.exp_avg_sq)
    ts.num_tokens_since_fired.copy_(R.initial_counts(sc))
    name_of = {p.data_ptr(): n for n, p in gpu.items()}
    slot = {n: next(i for i, q in enumerate(ts.params) if q is p) for n, p in gpu.items()}
    ref = LR.LionTrainerRef(cfg, init)
    ref.num_tokens_since_fired = R.initial_counts(sc)
    spy = _Spy(monkeypatch)
    worst = {c: 0.0 for c in ("selection", "gradient", "norm", "M", "W_renorm", "undecided", "stats")}
    results, norm_calls = [], []

    for b, x in enumerate(R.make_batches(sc)):
        if b % cfg.grad_acc_steps == 0:
            ref.load_state({n: p.detach() for n, p in gpu.items()}, {n: ts.exp_avg[slot[n]] for n in R.NAMES})
        spy.clear()
        out = ts.step(x.to(dev))
        what = f"{sc.name} batch {b}"

        # (a) the selections, chunk by chunk; the restatement adopts them
        chunks = x.chunk(cfg.micro_acc_steps)
        assert len(spy.sel) == len(chunks), (what, len(spy.sel))
        r = ref.batch(x, [c["sel"] for c in spy.sel], update=False)
        results.append(r)
        worst["selection"] = max(worst["selection"], r.sel_ratio)
        assert r.tie_share <= LR.TIE_CAP, (what, "share of near-ties", r.tie_share)
        for c in spy.sel:
            if cfg.auxk_alpha > 0:
                assert torch.equal(c["dead_mask"], r.dead_mask), (what, "dead mask")
            else:
                assert c["dead_mask"] is None

        # (f) bookkeeping, never synchronised
        assert bool(out["stepped"]) == r.stepped and ts.global_step == r.global_step == b + 1, what
        assert ts.t == ref.t, (what, ts.t, ref.t)
        assert torch.equal(ts.num_tokens_since_fired.cpu(), r.num_tokens_since_fired), (what, "num_tokens_since_fired")
        for n in ("fvu", "auxk_loss", "multi_topk_fvu"):
            worst["stats"] = max(worst["stats"], tr.assert_within(out[n], r.stats[n], r.dstats[n], f"{what} {n}"))

        if not r.stepped:
            assert not spy.lion, what
            for n in R.NAMES:                                       # (c) .grad after the in-place clip
                worst["gradient"] = max(worst["gradient"],
                                        tr.assert_within(gpu[n].grad, r.G[n], r.dG[n], f"{what} {n}.grad after the clip", dev))
            continue

        # (b) the arguments of the four optimiser passes
        assert sorted(name_of[c["ptr"]] for c in spy.lion) == sorted(R.NAMES), what
        last_chunk = chunks[-1].shape[0]
        for c in spy.lion:
            n = name_of[c["ptr"]]
            assert tr.f32(c["lr"]) == tr.f32(r.lr), (what, n, "lr", c["lr"], r.lr)
            kw = c["kw"]
            assert c["has_sumsq"] and kw["max_norm"] == cfg.max_norm and tuple(kw["betas"]) == cfg.betas and "eps" not in kw
            assert kw["project"] == (cfg.normalize_decoder and n == "W_dec"), (what, n, "project")
            assert kw.get("renorm_eps") == (EPS32 if fuse and cfg.normalize_decoder and n == "W_dec" else None), (what, n)
            assert c["refresh"] == (fuse and n == "W_enc"), (what, n, "refresh")
            assert kw.get("tokens_next", 0) == (last_chunk if fuse and n == "W_enc" else 0), (what, n, "tokens_next")

        # (c) the gradients handed to the optimiser passes
        for c in spy.lion:
            n = name_of[c["ptr"]]
            worst["gradient"] = max(worst["gradient"], tr.assert_within(c["before"][1], r.G[n], r.dG[n], f"{what} grad of {n}", dev))

        # (d) the clip's total against the GPU's own gradients, in the order _update accumulates it
        S, bound = 0.0, 0.0
        for c in sorted(spy.lion, key=lambda c: slot[name_of[c["ptr"]]]):
            S, bnd = tr.grad_sumsq(c["before"][1], S)
            bound += bnd
        S_gpu = float(ts._sumsq)
        worst["norm"] = max(worst["norm"], tr.assert_within(S_gpu, S, bound, f"{what} total squared gradient norm"))
        norm_calls.append(list(spy.norm_calls))

        # (e) the update, from the GPU's own inputs
        sumsq = ts._sumsq.detach().clone()
        for c in spy.lion:
            n = name_of[c["ptr"]]
            W, G, M = c["before"]
            W_after, M_after = c["after"]
            project, renorm_eps = c["kw"]["project"], c["kw"].get("renorm_eps")
            (_, M1, u, _), bnd = L.lion_rows(W.cpu(), G.cpu(), M.cpu(), r.lr, betas=cfg.betas, total_sumsq=S_gpu,
                                             max_norm=cfg.max_norm, project=project)
            Wp, Mp = W.clone(), M.clone()                            # the same pass without tails: its bits carry the signs
            spy.real_lion(Wp, G, Mp, c["lr"], total_sumsq=sumsq, max_norm=cfg.max_norm, betas=cfg.betas, project=project)
            assert torch.equal(Mp, M_after), (what, n, "the momentum of the pass with tails differs from the pass without")
            s, share = L.check_w(Wp.cpu(), W.cpu(), r.lr, u, bnd.du, f"{what} {n} W")
            assert share <= L.UNDECIDED_CAP, (what, n, "undecided share", share)
            worst["undecided"] = max(worst["undecided"], share)
            worst["M"] = max(worst["M"], tr.assert_within(M_after.cpu(), M1, bnd.dM, f"{what} {n} M after the pass"))
            if renorm_eps is None:
                assert torch.equal(Wp, W_after), (what, n, "W of the pass with tails differs from the pass without")
            else:
                want, wb = L.renorm_of(W.cpu(), s, r.lr, renorm_eps)
                worst["W_renorm"] = max(worst["W_renorm"],
                                        tr.assert_within(W_after.cpu(), want, wb, f"{what} {n} W after the renorm"))
            assert torch.equal(W_after, gpu[n].detach()), (what, n, "the parameter was touched after its pass")

    print(f"\nlion {sc.name} fuse={fuse}: max err/bound " + " ".join(f"{k} {v:.4g}" for k, v in worst.items()) +
          f"; clip {[round(r.clip, 3) for r in results]} near-tie share {max(r.tie_share for r in results):.4f}")
    LR.assert_preconditions(sc, results, ref.num_tokens_since_fired)
    return results, norm_calls, ts


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_lion_plain_trajectory(dev, monkeypatch, fuse):
    """T = 512, 5 steps, warm-up of 2 and decay to step 6: a first step at lr 0 (the momentum moves, the parameters keep their
    bits), the schedule's three regimes, the weight-gradient short-cut of the norm, the skipped renormalisation and the
    operand hand-over of the fused pass."""
    sc = LR.scenario("plain")
    results, norm_calls, _ = _run(dev, monkeypatch, sc, fuse)
    assert all(calls.count("sum_into_") == 2 and calls.count("grad_sumsq_") == 2 for calls in norm_calls), norm_calls


def test_lion_accumulate_trajectory(dev, monkeypatch):
    """T = 515 in two micro-chunks and two batches per optimiser step: the in-place clip on the odd batches, the clip inside
    the sign pass on the even ones; the norm's short-cut must NOT be taken."""
    sc = LR.scenario("accumulate")
    assert sc.tokens[0] == 515
    results, norm_calls, _ = _run(dev, monkeypatch, sc)
    assert all(calls == ["grad_sumsq_"] * 4 for calls in norm_calls), norm_calls


def test_lion_dead_feature_trajectory(dev, monkeypatch):
    """auxk_alpha = 1 / 32, Multi-TopK, dead_feature_threshold = 2 T: 50 features start above the threshold, a hundred more
    cross it during the run; did_fire comes from the 4k selection."""
    sc = LR.scenario("dead")
    results, _, ts = _run(dev, monkeypatch, sc)
    start = R.start_dead_features(sc)
    assert bool((ts.num_tokens_since_fired.cpu()[start] > sc.cfg.dead_feature_threshold).any())
