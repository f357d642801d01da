"""SaeTrainStep.step over several batches against tests/trainer_ref.py, the float64 restatement of the reference training
loop with derived bounds.  The kernels under the step are pinned one by one elsewhere; this module checks the code in
msae/train.py that strings them together, where every other multi-step test compares the step with itself.

A spy records every ops.adam_rows_ call (clones of p, g, m, v before it, step, lr, the keywords; p, m, v after it), every
selection ops.sparse_encode returns (main, AuxK, Multi-TopK) with the dead mask it was given, and which of ops.sum_into_ /
ops.grad_sumsq_ built the gradient norm.  Before every optimiser step the restatement takes the GPU's float32 parameters and
moments, so each step is judged from identical inputs; its bookkeeping (t, global_step, num_tokens_since_fired, did_fire,
num_tokens_in_step) is NEVER synchronised.  Per batch:

  a. selections   each recorded selection is a valid top-k of the float64 pre-activations (AuxK: over the dead set) within
                  b_t, and is then adopted by the restatement; the share of tokens with a float64 gap at rank k below 2 b_t
                  is at most 1 % (test_trainer_ref_host.py shows the seeds meet that from float64 alone).  This is also what
                  catches a stale operand buffer after the fused refresh;
  b. arguments    step and lr of every adam_rows_ call equal the restatement's t and the float32 value of its scheduled lr,
                  exactly; project / renorm_eps / refresh / tokens_next are what the configuration implies;
  c. gradients    every recorded g (and, on a batch that does not step, p.grad after the in-place clip) within dG of G64;
  d. norm         ts._sumsq within train_ref.grad_sumsq's bound of sum G_gpu^2, with the weight-gradient short-cut taken
                  (plain) and not taken (accumulate);
  e. update       parameters and moments after the pass within train_ref.adam_rows' bounds, fed the GPU's own G and norm;
  f. bookkeeping  num_tokens_since_fired, t, global_step, `stepped` and the dead mask equal the restatement's, exactly; fvu,
                  auxk_loss and multi_topk_fvu within their propagated bounds.

BatchTopK (SaeConfig(activation="batchtopk")) and Matryoshka (SaeConfig(matryoshka=...), section 7o) run
through the same checks, with these on top.  The spy also records what ops.batch_select returned per chunk, and sae.threshold
and the step's nested_fvu are read after every batch:

  a'. batch selection   theta, the kept values, the lengths and n_saturated equal, bit for bit, the sorting restatement
                  (tests/batch_select_ref.py) of the float32 top-C list; over the whole chunk the kept entries are a valid
                  batch-level selection of the float64 latents within b_t and at least min(T k, positives) are kept; the
                  keep mask is then adopted.  The near-tie share of this mode counts the kept slots float64 leaves undecided
                  (trainer_ref._batch_tie_share), at most 1 % as before;
  f'. bookkeeping  n_saturated, the lengths and num_tokens_since_fired under the kept-prefix rule, exactly; theta (the float32
                  mean over the chunks), sae.threshold (folded per chunk, never synchronised), nested_fvu, and fvu against
                  nested_fvu[-1], within their derived bounds;
  d'. norm         which of ops.sum_into_ / ops.grad_sumsq_ built the norm, per scenario (`_norm_pattern`).

Every scenario asserts its preconditions on the restatement's values (clip active in one batch and inactive in another, both
sides of k_aux, a feature dead from start to end) and prints its largest error / bound per check.

Behaviour that differs from the reference on purpose: with fuse_next_step the Adam pass leaves W_dec renormalised (msae/train.py,
"Between steps `W_dec` therefore holds unit-norm rows"), so the step's own renormalisation is skipped; the restatement
renormalises at the top of the batch as the reference does and carries the difference of the two as an input interval.

Out of scope: optim_bits=8 (test_gpu_adam8.py has its own restatement), init_b_dec (an iterative median whose trip count
depends on the precision) and data parallelism."""
import gc

import pytest
import torch

import train_ref as tr
import trainer_ref as R

pytestmark = pytest.mark.gpu

TIE_CAP = 0.01
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

        self.adam, self.sel, self.norm_calls, self.bsel = [], [], [], []
        real_adam, real_se, real_sum, real_gss = ops.adam_rows_, ops.sparse_encode, ops.sum_into_, ops.grad_sumsq_
        real_bs = ops.batch_select

        def adam_rows_(p, g, m, v, step, lr, **kw):
            rec = {"ptr": p.data_ptr(), "before": tuple(t.detach().clone() for t in (p, g, m, v)), "step": step, "lr": lr,
                   "kw": {k: val for k, val in kw.items() if k not in ("total_sumsq", "refresh")},
                   "has_sumsq": kw.get("total_sumsq") is not None, "refresh": kw.get("refresh") is not None}
            real_adam(p, g, m, v, step, lr, **kw)
            rec["after"] = tuple(t.detach().clone() for t in (p, m, v))
            self.adam.append(rec)

        def sparse_encode(x, W_enc, b_enc, b_dec, k, dead_mask=None, k_aux=0, k_multi=0, **kw):
            out = real_se(x, W_enc, b_enc, b_dec, k, dead_mask, k_aux, k_multi, **kw)
            self.sel.append({"sel": [(a.detach().cpu(), i.detach().cpu()) for a, i in out],
                             "dead_mask": None if dead_mask is None else dead_mask.detach().cpu(),
                             "auxk_path": kw.get("auxk_path", "dense")})
            return out

        def batch_select(acts, idx, k):
            out = real_bs(acts, idx, k)
            assert k == self.k, ("batch_select was asked for k =", k)
            self.bsel.append(tuple(t.detach().cpu() for t in out))          # kept values, lengths, theta, n_saturated
            return out

        def sum_into_(accum, v):
            self.norm_calls.append("sum_into_")
            return real_sum(accum, v)

        def grad_sumsq_(accum, g):
            self.norm_calls.append("grad_sumsq_")
            return real_gss(accum, g)

        monkeypatch.setattr(ops, "adam_rows_", adam_rows_)
        monkeypatch.setattr(ops, "sparse_encode", sparse_encode)
        monkeypatch.setattr(ops, "sum_into_", sum_into_)
        monkeypatch.setattr(ops, "grad_sumsq_", grad_sumsq_)
        monkeypatch.setattr(ops, "batch_select", batch_select)
        self.k = None

    def clear(self):
        self.adam, self.sel, self.norm_calls, self.bsel = [], [], [], []


def _run(dev, monkeypatch, sc: R.Scenario, fuse: bool, auxk_path: str = "dense"):
    """The scenario on the GPU and in the restatement, batch by batch, with the checks (a)-(f) -> the per-batch results of
    the restatement and the spy's norm calls per stepping batch."""
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    cfg = sc.cfg
    init = R.make_params(sc)
    batch = cfg.activation == "batchtopk"
    sae = Sae(sc.d, SaeConfig(num_latents=sc.N, k=cfg.k, multi_topk=cfg.multi_topk, normalize_decoder=cfg.normalize_decoder,
                              activation=cfg.activation, batch_cap=cfg.cap, matryoshka=list(cfg.matryoshka),
                              matryoshka_weights=list(cfg.matryoshka_weights)), device=dev)
    assert sae.cfg.cap == cfg.width
    gpu = {"W_enc": sae.encoder.weight, "b_enc": sae.encoder.bias, "W_dec": sae.W_dec, "b_dec": sae.b_dec}
    with torch.no_grad():
        for n in R.NAMES:
            gpu[n].copy_(init[n])
    sae.invalidate_prepared()
    ts = SaeTrainStep(sae, lr=cfg.lr, auxk_alpha=cfg.auxk_alpha, dead_feature_threshold=cfg.dead_feature_threshold,
                      grad_acc_steps=cfg.grad_acc_steps, micro_acc_steps=cfg.micro_acc_steps,
                      lr_warmup_steps=cfg.lr_warmup_steps, total_steps=cfg.total_steps, fuse_next_step=fuse,
                      auxk_path=auxk_path, threshold_lr=cfg.threshold_lr)
    ts.num_tokens_since_fired.copy_(R.initial_counts(sc))
    name_of = {p.data_ptr(): n for n, p in gpu.items()}
    slot = {n: next(i for i, q in enumerate(ts.params) if q is p) for n, p in gpu.items()}
    ref = R.TrainerRef(cfg, init)
    ref.num_tokens_since_fired = R.initial_counts(sc)
    spy = _Spy(monkeypatch)
    spy.k = cfg.k
    worst = {c: 0.0 for c in ("selection", "gradient", "norm", "W", "M", "V", "stats")}
    if batch:
        worst.update(theta=0.0, threshold=0.0)
    if cfg.matryoshka:
        worst.update(nested_fvu=0.0)
    results, norm_calls = [], []

    for b, x in enumerate(R.make_batches(sc)):
        if b % cfg.grad_acc_steps == 0:
            ref.load_state({n: p.detach() for n, p in gpu.items()}, {n: ts.exp_avg[slot[n]] for n in R.NAMES},
                           {n: ts.exp_avg_sq[slot[n]] for n in R.NAMES})
        spy.clear()
        out = ts.step(x.to(dev))
        what = f"{sc.name} batch {b}"

        # (a) the selections, chunk by chunk; the restatement adopts them
        chunks = x.chunk(cfg.micro_acc_steps)
        assert len(spy.sel) == len(chunks), (what, len(spy.sel))
        # (a') "batchtopk": what ops.batch_select returned per chunk is checked bit for bit against the sorting restatement of
        # the float32 list and for validity against the float64 latents (trainer_ref._adopt_batch), then adopted
        assert len(spy.bsel) == (len(chunks) if batch else 0), (what, len(spy.bsel))
        r = ref.batch(x, [c["sel"] for c in spy.sel], update=False, batch_selects=spy.bsel if batch else None)
        results.append(r)
        worst["selection"] = max(worst["selection"], r.sel_ratio)
        assert r.tie_share <= TIE_CAP, (what, "share of near-ties", r.tie_share)
        for c in spy.sel:
            assert c["auxk_path"] == auxk_path or cfg.auxk_alpha == 0
            if cfg.auxk_alpha > 0:                                   # (f) the dead mask the forward ran with
                assert torch.equal(c["dead_mask"], r.dead_mask), (what, "dead mask")
            else:
                assert c["dead_mask"] is None

        # (f) bookkeeping, never synchronised
        assert bool(out["stepped"]) == r.stepped and ts.global_step == r.global_step == b + 1, what
        assert ts.t == ref.t, (what, ts.t, ref.t)
        assert torch.equal(ts.num_tokens_since_fired.cpu(), r.num_tokens_since_fired), (what, "num_tokens_since_fired")
        for n in ("fvu", "auxk_loss", "multi_topk_fvu"):
            worst["stats"] = max(worst["stats"], tr.assert_within(out[n], r.stats[n], r.dstats[n], f"{what} {n}"))
        # (f') the bookkeeping of the two modes: counts exact, the float32 means and the folded threshold within their bounds
        if batch:
            assert int(out["n_saturated"]) == r.n_saturated, (what, "n_saturated", int(out["n_saturated"]), r.n_saturated)
            assert torch.equal(torch.cat([c[1].reshape(-1) for c in spy.bsel]).to(torch.int32), r.lengths), (what, "lengths")
            worst["theta"] = max(worst["theta"], tr.assert_within(out["theta"], r.theta, r.dtheta, f"{what} theta"))
            worst["threshold"] = max(worst["threshold"],
                                     tr.assert_within(sae.threshold, r.threshold, r.dthreshold, f"{what} threshold"))
        else:
            assert "theta" not in out and not hasattr(sae, "threshold")
        if cfg.matryoshka:
            got = out["nested_fvu"].detach().cpu()
            assert tuple(got.shape) == (len(cfg.matryoshka),), (what, tuple(got.shape))
            for g in range(len(cfg.matryoshka)):
                worst["nested_fvu"] = max(worst["nested_fvu"], tr.assert_within(got[g], r.nested_fvu[g], r.dnested_fvu[g],
                                                                                f"{what} nested_fvu[{g}]"))
            tr.assert_within(out["fvu"], r.nested_fvu[-1], r.dnested_fvu[-1], f"{what} fvu against nested_fvu[-1]")
        else:
            assert "nested_fvu" not in out

        if not r.stepped:
            assert not spy.adam, what
            for n in R.NAMES:                                       # (c) .grad after the in-place clip
                worst["gradient"] = max(worst["gradient"],
                                        tr.assert_within(gpu[n].grad, r.G[n], r.dG[n], f"{what} {n}.grad after the clip", dev))
            continue

        # (b) the arguments of the four optimiser passes
        assert sorted(name_of[c["ptr"]] for c in spy.adam) == sorted(R.NAMES), what
        last_chunk = chunks[-1].shape[0]
        for c in spy.adam:
            n = name_of[c["ptr"]]
            assert c["step"] == r.t, (what, n, "step", c["step"], r.t)
            assert tr.f32(c["lr"]) == tr.f32(r.lr), (what, n, "lr", c["lr"], r.lr)
            kw = c["kw"]
            assert c["has_sumsq"] and kw["max_norm"] == cfg.max_norm and tuple(kw["betas"]) == cfg.betas and kw["eps"] == cfg.eps
            assert kw["project"] == (cfg.normalize_decoder and n == "W_dec"), (what, n, "project")
            assert kw.get("renorm_eps") == (EPS32 if fuse and cfg.normalize_decoder and n == "W_dec" else None), (what, n)
            assert c["refresh"] == (fuse and n == "W_enc"), (what, n, "refresh")
            assert kw.get("tokens_next", 0) == (last_chunk if fuse and n == "W_enc" else 0), (what, n, "tokens_next")

        # (c) the gradients handed to the optimiser passes
        for c in spy.adam:
            n = name_of[c["ptr"]]
            worst["gradient"] = max(worst["gradient"], tr.assert_within(c["before"][1], r.G[n], r.dG[n], f"{what} grad of {n}", dev))

        # (d) the clip's total against the GPU's own gradients, in the order _update accumulates it
        S, bound = 0.0, 0.0
        for c in sorted(spy.adam, key=lambda c: slot[name_of[c["ptr"]]]):
            S, bnd = tr.grad_sumsq(c["before"][1], S)
            bound += bnd
        S_gpu = float(ts._sumsq)
        worst["norm"] = max(worst["norm"], tr.assert_within(S_gpu, S, bound, f"{what} total squared gradient norm"))
        norm_calls.append(list(spy.norm_calls))

        # (e) the update, from the GPU's own inputs
        for c in spy.adam:
            n = name_of[c["ptr"]]
            W, G, M, V = c["before"]
            (W1, M1, V1), (dW, dM, dV) = tr.adam_rows(W, G, M, V, r.t, r.lr, betas=cfg.betas, eps=cfg.eps, total_sumsq=S_gpu,
                                                      max_norm=cfg.max_norm, project=c["kw"]["project"],
                                                      renorm_eps=c["kw"].get("renorm_eps"), device=dev)
            for key, got, want, bnd in zip("WMV", c["after"], (W1, M1, V1), (dW, dM, dV)):
                worst[key] = max(worst[key], tr.assert_within(got, want, bnd, f"{what} {n} {key} after the pass", dev))
            assert torch.equal(c["after"][0], gpu[n].detach()), (what, n, "the parameter was touched after its pass")

    print(f"\n{sc.name} fuse={fuse} normalize={cfg.normalize_decoder} auxk_path={auxk_path}: max err/bound " +
          " ".join(f"{k} {v:.4f}" for k, v in worst.items()) +
          f"; clip {[round(r.clip, 3) for r in results]} near-tie share {max(r.tie_share for r in results):.4f}" +
          (f"; saturated rows {[r.n_saturated for r in results]} threshold {float(sae.threshold):.6f}" if batch else ""))
    assert any(r.clip < 1 for r in results) and any(r.clip == 1 for r in results), "the clip must be active and inactive in a run"
    return results, norm_calls, ts


def _norm_pattern(cfg: R.TrainerConfig, auxk_active: bool):
    """(d') The ops calls that build the clip's norm on a stepping batch, from msae/train.py's _update: the per-row sums a
    weight-gradient kernel recorded (ops.sum_into_) stand for a weight gradient only when `single` holds (one chunk per
    optimiser step, so .grad IS the one recorded tensor) and ops.collect_wgrad_sumsq counted exactly ONE kernel call for that
    weight.  W_enc always has one call (the encoder backward runs once over all lists side by side).  W_dec has one call per
    decode: the plain decode, the length-aware decode and the grouped call of the nested node are one each, and an active
    AuxK term adds its own decode, which makes two and rules the short-cut out for W_dec.  With accumulation (micro-chunks
    or windows) .grad is a sum of several calls' outputs: every parameter is read again.  The two biases always are."""
    if cfg.grad_acc_steps * cfg.micro_acc_steps != 1:
        return ["grad_sumsq_"] * 4
    taken = 1 if auxk_active else 2
    return sorted(["sum_into_"] * taken + ["grad_sumsq_"] * (4 - taken))


def _mode_preconditions(sc, results):
    cfg = sc.cfg
    if cfg.matryoshka:
        assert all(min(r.groups_min) > 0 for r in results), "every group holds live entries in every chunk"
        assert any(r.empty_first > 0 for r in results), "some token has an empty first group"
        assert 0.0 in cfg.matryoshka_weights and any(m % 64 for m in cfg.matryoshka) and len(cfg.matryoshka) >= 3


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_batchtopk_trajectory(dev, monkeypatch, fuse):
    """k = 16 over top-64 lists, T = 512, the plain schedule: theta and the kept prefixes of five batches, rows of length 0
    (the length-aware decode's empty row) and none at the cap, the threshold folded once per batch, the fused operand refresh
    with the next encode at width C = 64 in place of k, the norm's short-cut on the length-aware decode's one call."""
    sc = R.scenario("batchtopk")
    assert sc.cfg.cap == 64 and sc.cfg.k == 16
    results, norm_calls, ts = _run(dev, monkeypatch, sc, fuse)
    assert all(bool((r.lengths == 0).any()) and r.n_saturated == 0 for r in results)
    assert all(sorted(calls) == _norm_pattern(sc.cfg, False) for calls in norm_calls), norm_calls
    assert float(ts.sae.threshold) > 0


@pytest.mark.parametrize("auxk_path", ["dense", "subset"])
def test_batchtopk_saturated_trajectory(dev, monkeypatch, auxk_path):
    """C = 32 = 2 k: saturated and unsaturated rows in one chunk; T = 515 in two uneven chunks (258 / 257, each with its own
    theta and fold of the threshold) and two batches per optimiser step; AuxK on the residual of the KEPT reconstruction;
    240 features start one token into their count, and those that window 1 names in dropped slots only must be dead in
    window 2 (test_trainer_ref_host.py shows the kept-prefix rule decides that mask)."""
    sc = R.scenario("batchtopk_saturated")
    assert sc.tokens[0] == 515 and sc.cfg.cap == 32
    results, norm_calls, _ = _run(dev, monkeypatch, sc, True, auxk_path)
    assert [r.stepped for r in results] == [False, True] * 2
    for r in results:
        first = r.lengths[:258]
        assert bool((first == 32).any()) and bool((first < 32).any()) and r.n_saturated > 0
    k_aux = sc.d // 2
    assert results[0].num_dead == sc.start_dead < k_aux < results[-1].num_dead
    old = torch.zeros(sc.N, dtype=torch.bool)
    old[R.start_old_features(sc)] = True
    assert bool((results[-1].dead_mask & old).any()) and bool((~results[-1].dead_mask & old).any())
    assert all(calls == _norm_pattern(sc.cfg, True) for calls in norm_calls), norm_calls


@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "no_normalize"])
def test_matryoshka_trajectory(dev, monkeypatch, normalize):
    """Prefixes (300, 2049, 8192) with weights (0.5, 0, 0.25), fused: the descent on the weighted prefix FVUs (fvu a
    statistic), the combine with a zero coefficient, the grouped weight gradient feeding the norm's short-cut, then the clip,
    the decoder projection and the skipped renormalisation of the fused pass."""
    sc = R.scenario("matryoshka", normalize_decoder=normalize)
    assert sc.cfg.matryoshka == (300, 2049, 8192)
    results, norm_calls, _ = _run(dev, monkeypatch, sc, True)
    _mode_preconditions(sc, results)
    assert all(sorted(calls) == _norm_pattern(sc.cfg, False) for calls in norm_calls), norm_calls


def test_matryoshka_auxk_trajectory(dev, monkeypatch):
    """The same prefixes with auxk_alpha = 1 / 32 and 50 features dead from start to end: the AuxK term's gradient enters the
    combine as grad_full, its target is the residual of the full reconstruction; W_dec's gradient is the sum of two kernel
    calls, so its norm is read again."""
    sc = R.scenario("matryoshka_auxk")
    results, norm_calls, _ = _run(dev, monkeypatch, sc, True)
    _mode_preconditions(sc, results)
    assert all(r.num_dead == sc.start_dead and 0 < r.scale < 1 for r in results)
    assert all(sorted(calls) == _norm_pattern(sc.cfg, True) for calls in norm_calls), norm_calls


def test_matryoshka_batchtopk_trajectory(dev, monkeypatch):
    """Both modes, T = 515 in two uneven chunks: a prefix sees kept entries only, nested_fvu and theta are means over uneven
    chunks, the threshold is folded twice per batch."""
    sc = R.scenario("matryoshka_batchtopk")
    assert sc.tokens[0] == 515 and sc.cfg.activation == "batchtopk" and sc.cfg.matryoshka
    results, norm_calls, _ = _run(dev, monkeypatch, sc, True)
    _mode_preconditions(sc, results)
    assert all(bool((r.lengths == 0).any()) for r in results)
    assert all(calls == _norm_pattern(sc.cfg, False) for calls in norm_calls), norm_calls


@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "no_normalize"])
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
def test_plain_trajectory(dev, monkeypatch, fuse, normalize):
    """T = 512, 5 steps, warm-up of 2 and decay to step 6: the schedule's three regimes, the bias-correction step, the
    weight-gradient short-cut of the norm (both weight gradients come out of one kernel call each), the skipped
    renormalisation and the operand hand-over of the fused pass."""
    sc = R.scenario("plain", normalize_decoder=normalize)
    results, norm_calls, _ = _run(dev, monkeypatch, sc, fuse)
    lrs = [r.lr for r in results]
    assert lrs[0] == 0.0 and lrs[2] == sc.cfg.lr and lrs[4] < lrs[3] < lrs[2], lrs
    assert all(calls.count("sum_into_") == 2 and calls.count("grad_sumsq_") == 2 for calls in norm_calls), norm_calls


def test_accumulate_trajectory(dev, monkeypatch):
    """T = 515 in two micro-chunks (258 / 257) and two batches per optimiser step: the in-place clip on the odd batches, the
    clip inside the Adam pass on the even ones, chunk losses weighted by 1 / acc_steps, _tokens_in_step over a window; the
    norm's short-cut must NOT be taken."""
    sc = R.scenario("accumulate")
    assert sc.tokens[0] == 515
    results, norm_calls, _ = _run(dev, monkeypatch, sc, True)
    assert [r.stepped for r in results] == [False, True] * 3
    assert any(r.clip < 1 for r in results if not r.stepped) and any(r.clip == 1 for r in results if not r.stepped)
    assert all(calls == ["grad_sumsq_"] * 4 for calls in norm_calls), norm_calls


@pytest.mark.parametrize("auxk_path", ["dense", "subset"])
def test_dead_feature_trajectory(dev, monkeypatch, auxk_path):
    """auxk_alpha = 1 / 32, Multi-TopK, dead_feature_threshold = 2 T: 50 features start above the threshold (num_dead < k_aux,
    scale < 1), a hundred more cross it during the run (> against >=, scale capped at 1), did_fire comes from the 4k
    selection."""
    sc = R.scenario("dead")
    results, _, ts = _run(dev, monkeypatch, sc, True, auxk_path)
    k_aux = sc.d // 2
    assert results[0].num_dead == 50 < k_aux and 0 < results[0].scale < 1
    assert any(r.num_dead > k_aux and r.scale == 1.0 for r in results)
    start = R.start_dead_features(sc)
    assert bool((results[-1].num_tokens_since_fired[start] > sc.cfg.dead_feature_threshold).any())
    assert bool((ts.num_tokens_since_fired.cpu()[start] > sc.cfg.dead_feature_threshold).any())


def test_batch_size_trajectory(dev, monkeypatch):
    """d = 1024 with T = 512, 200, 512, 8, 300: every encode follows an optimiser pass that prepared the operands for
    another size class (and the small-T path follows the large one): a buffer trusted wrongly shows as an invalid top-k."""
    sc = R.scenario("batch_sizes")
    assert sc.tokens == (512, 200, 512, 8, 300)
    _run(dev, monkeypatch, sc, True)
