"""Host tests of tests/trainer_ref.py, the float64 restatement of the reference training loop that
test_gpu_train_trajectory.py judges SaeTrainStep against.  No GPU, nothing of msae.

  1. The restatement (hand-written forward and backward, own bookkeeping) against a LITERAL dense loop: autograd,
     torch.optim.Adam, a LambdaLR with the same multiplier, clip_grad_norm_, in float64, on the `accumulate` and `dead`
     settings scaled down to d = 32, N = 256 -- agreement to 1e-12 relative.
  2. The tie cap of the GPU scenarios holds for their seeds from float64 alone, and so do their other preconditions (clip
     active and inactive, both sides of k_aux, an initially dead feature still dead at the end).
  3. The checks have power: each mutation of the restatement moves a checked quantity of the scenario meant to catch it by
     at least 4 times its bound (exact checks: at all)."""
import functools

import pytest
import torch

import train_ref as tr
import trainer_ref as R
from train_ref import F64

EPS32 = float(torch.finfo(torch.float32).eps)


# ---- 1. against torch ---------------------------------------------------------------------------------------------------------
def _literal_loop(sc: R.Scenario):
    """trainer.py:347-414 and sae.py:193-271, line by line, on float64 leaves."""
    cfg = sc.cfg
    P = {n: torch.nn.Parameter(v.to(F64)) for n, v in R.make_params(sc).items()}
    We, be, Wd, bd = (P[n] for n in R.NAMES)
    opt = torch.optim.Adam([We, be, Wd, bd], lr=cfg.lr, betas=cfg.betas, eps=cfg.eps)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda s: R.linear_schedule_with_warmup(s, cfg.lr_warmup_steps, cfg.total_steps))
    counts = R.initial_counts(sc)
    did_fire = torch.zeros(sc.N, dtype=torch.bool)
    num_tokens_in_step, global_step = 0, 0
    log = []

    def decode(acts, idx):
        return (acts[:, :, None] * Wd[idx]).sum(1) + bd

    for x in R.make_batches(sc):
        x = x.to(F64)
        num_tokens_in_step += x.shape[0]
        if cfg.normalize_decoder:
            with torch.no_grad():
                Wd.data /= torch.norm(Wd.data, dim=1, keepdim=True) + EPS32
        acc_steps = cfg.grad_acc_steps * cfg.micro_acc_steps
        stats = [0.0, 0.0, 0.0]
        chunks = x.chunk(cfg.micro_acc_steps)
        for chunk in chunks:
            dead_mask = counts > cfg.dead_feature_threshold if cfg.auxk_alpha > 0 else None
            pre_acts = torch.relu(torch.nn.functional.linear(chunk - bd, We, be))
            top_acts, top_indices = pre_acts.topk(cfg.k, sorted=False)
            sae_out = decode(top_acts, top_indices)
            e = sae_out - chunk
            total_variance = (chunk - chunk.mean(0)).pow(2).sum()
            if dead_mask is not None and (num_dead := int(dead_mask.sum())) > 0:
                k_aux = chunk.shape[-1] // 2
                scale = min(num_dead / k_aux, 1.0)
                k_aux = min(k_aux, num_dead)
                auxk_latents = torch.where(dead_mask[None], pre_acts, -torch.inf)
                auxk_acts, auxk_indices = auxk_latents.topk(k_aux, sorted=False)
                e_hat = decode(auxk_acts, auxk_indices)
                auxk_loss = scale * (e_hat - e).pow(2).sum() / total_variance
            else:
                auxk_loss = sae_out.new_tensor(0.0)
            fvu = e.pow(2).sum() / total_variance
            if cfg.multi_topk:
                top_acts, top_indices = pre_acts.topk(4 * cfg.k, sorted=False)
                sae_out = decode(top_acts, top_indices)
                multi_topk_fvu = (sae_out - chunk).pow(2).sum() / total_variance
            else:
                multi_topk_fvu = sae_out.new_tensor(0.0)
            loss = fvu + cfg.auxk_alpha * auxk_loss + multi_topk_fvu / 8
            loss.div(acc_steps).backward()
            for i, s in enumerate((fvu, auxk_loss, multi_topk_fvu)):
                stats[i] += float(s.detach()) / len(chunks)
            did_fire[top_indices.flatten()] = True
        torch.nn.utils.clip_grad_norm_([We, be, Wd, bd], cfg.max_norm)
        step, substep = divmod(global_step + 1, cfg.grad_acc_steps)
        if substep == 0:
            if cfg.normalize_decoder:
                with torch.no_grad():
                    Wd.grad -= (Wd.grad * Wd.data).sum(1, keepdim=True) * Wd.data
            opt.step()
            opt.zero_grad()
            sched.step()
            counts += num_tokens_in_step
            counts[did_fire] = 0
            num_tokens_in_step = 0
            did_fire.zero_()
        global_step += 1
        log.append((stats, counts.clone(), substep == 0))
    moments = {n: (opt.state[P[n]]["exp_avg"], opt.state[P[n]]["exp_avg_sq"]) for n in R.NAMES}
    return {n: p.detach() for n, p in P.items()}, moments, log


@pytest.mark.parametrize("name", ["accumulate", "dead"])
def test_restatement_equals_a_literal_torch_loop(name):
    sc = R.scenario(name, small=True)
    ref, results, _ = R.run_standalone(sc, f32_hyper=False)
    params, moments, log = _literal_loop(sc)
    assert any(r.clip < 1 for r in results) and any(r.clip == 1 for r in results)
    if name == "dead":
        k_aux = sc.d // 2
        assert any(0 < r.num_dead < k_aux for r in results) and any(r.num_dead > k_aux for r in results)
    for r, (stats, counts, stepped) in zip(results, log):
        assert r.stepped == stepped
        assert torch.equal(r.num_tokens_since_fired, counts)
        for i, n in enumerate(("fvu", "auxk_loss", "multi_topk_fvu")):
            assert abs(r.stats[n] - stats[i]) <= 1e-12 * abs(stats[i]), (n, r.stats[n], stats[i])
    for n in R.NAMES:
        for what, got, want in (("param", ref.p[n], params[n]), ("exp_avg", ref.m[n], moments[n][0]),
                                ("exp_avg_sq", ref.v[n], moments[n][1])):
            err = float((got - want).abs().max())
            assert err <= 1e-12 * float(want.abs().max()), (n, what, err)


# ---- 2. the preconditions of the GPU scenarios, from float64 alone -----------------------------------------------------
SCENARIOS = [("plain", True), ("plain", False), ("accumulate", True), ("dead", True), ("batch_sizes", True)]
TIE_CAP = 0.01


@functools.lru_cache(maxsize=None)
def _baseline(name: str, normalize: bool):
    sc = R.scenario(name, normalize_decoder=normalize)
    return (sc,) + R.run_standalone(sc)


@pytest.mark.parametrize("name,normalize", SCENARIOS, ids=[f"{n}{'' if z else '-no_norm'}" for n, z in SCENARIOS])
def test_gpu_scenarios_meet_their_preconditions(name, normalize):
    sc, ref, results, _ = _baseline(name, normalize)
    print(f"\n{name}: tie share per batch {[round(r.tie_share, 4) for r in results]}, clip {[round(r.clip, 3) for r in results]}, "
          f"dead {[r.num_dead for r in results]}")
    assert max(r.tie_share for r in results) <= TIE_CAP
    assert any(r.clip < 1 for r in results) and any(r.clip == 1 for r in results)
    if name == "plain":            # the schedule reaches its decay
        lrs = [r.lr for r in results]
        assert lrs[0] == 0.0 and lrs[2] == sc.cfg.lr and lrs[4] < lrs[3] < lrs[2]
    if name == "dead":
        k_aux = sc.d // 2
        assert results[0].num_dead == sc.start_dead < k_aux and 0 < results[0].scale < 1
        assert any(r.num_dead > k_aux for r in results)
        assert bool((ref.num_tokens_since_fired[R.start_dead_features(sc)] > sc.cfg.dead_feature_threshold).any())


# ---- 3. the checks have power -------------------------------------------------------------------------------------------
MUTANTS = [("bias_correction_t_plus_1", "plain"), ("lr_of_next_step", "plain"), ("no_clip_on_non_stepping", "accumulate"),
           ("dead_ge_threshold", "dead"), ("did_fire_from_k", "dead"), ("chunk_weight_by_token_share", "accumulate"),
           ("tokens_in_step_reset_every_batch", "accumulate"), ("scale_uncapped", "dead"), ("project_before_clip", "plain"),
           ("no_renorm", "plain")]
EXACT = {"bias_correction_t_plus_1": "t", "lr_of_next_step": "lr", "dead_ge_threshold": "dead_mask",
         "did_fire_from_k": "num_tokens_since_fired", "tokens_in_step_reset_every_batch": "num_tokens_since_fired"}


def test_every_mutation_is_listed():
    assert sorted(m for m, _ in MUTANTS) == sorted(R.MUTATIONS)


@pytest.mark.parametrize("mutation,name", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_mutation_moves_a_checked_quantity(mutation, name):
    """The mutant runs like the GPU side: parameters and moments synchronised to the correct run before every optimiser
    step, bookkeeping never.  Checked quantities per batch: t and lr of the optimiser pass, the dead mask, the counts
    (exact); every gradient against dG; the clip's total against the gradients handed over (grad_sumsq's bound)."""
    sc, _, base, states = _baseline(name, True)
    _, mut, _ = R.run_standalone(sc, (mutation,), sync_to=states)
    moved, worst = False, 0.0
    for b, (r, q) in enumerate(zip(base, mut)):
        if mutation in EXACT:
            a, c = getattr(r, EXACT[mutation]), getattr(q, EXACT[mutation])
            moved |= (not torch.equal(a, c)) if torch.is_tensor(a) else (tr.f32(a) != tr.f32(c) if EXACT[mutation] == "lr" else a != c)
            continue
        if mutation == "project_before_clip":
            if q.stepped:
                S, bound = 0.0, 0.0
                for n in R.NAMES:
                    S, b = tr.grad_sumsq(q.G[n], S)
                    bound += b
                worst = max(worst, abs(q.sumsq - S) / bound)
            continue
        for n in R.NAMES:
            pos = r.dG[n] > 0
            worst = max(worst, float(((q.G[n] - r.G[n]).abs()[pos] / r.dG[n][pos]).max()))
    print(f"\n{mutation} on {name}: " + ("an exact check moved" if mutation in EXACT else f"largest move / bound {worst:.1f}"))
    assert moved if mutation in EXACT else worst >= 4.0
