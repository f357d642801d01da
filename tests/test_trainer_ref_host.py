"""Host tests of tests/trainer_ref.py, the float64 restatement of the reference training loop that
test_gpu_train_trajectory.py judges SaeTrainStep against.  No GPU, nothing of msae.

  1. The restatement (hand-written forward and backward, own bookkeeping) against a LITERAL dense loop: autograd,
     torch.optim.Adam, a LambdaLR with the same multiplier, clip_grad_norm_, in float64, on the `accumulate` and `dead`
     settings and the five BatchTopK / Matryoshka ones (a keep mask from a sorted theta, prefix reconstructions by masking)
     scaled down to d = 32, N = 256 -- agreement to 1e-12 relative, theta, threshold, nested_fvu and the counts included.
  2. The tie cap of the GPU scenarios holds for their seeds from float64 alone, and so do their other preconditions (clip
     active and inactive, both sides of k_aux, an initially dead feature still dead at the end; a row of length 0 and none
     saturated; saturated and unsaturated rows in one chunk and a dead mask the kept-prefix rule decides; every group
     non-empty, a token with an empty first group, a zero-weight prefix).
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
    batch, bounds, weights = cfg.activation == "batchtopk", cfg.matryoshka, cfg.matryoshka_weights
    threshold = -1.0

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
        thetas, lengths, n_saturated, nested = [], [], 0, [0.0] * len(bounds)
        for chunk in chunks:
            dead_mask = counts > cfg.dead_feature_threshold if cfg.auxk_alpha > 0 else None
            pre_acts = torch.relu(torch.nn.functional.linear(chunk - bd, We, be))
            total_variance = (chunk - chunk.mean(0)).pow(2).sum()
            if batch:
                # BatchTopK: the mask of the top-C lists from a sorted theta, the (T k)-th largest positive list entry
                top_acts, top_indices = pre_acts.topk(cfg.cap, sorted=True)
                positive = top_acts.detach()[top_acts.detach() > 0].sort(descending=True).values
                theta = float(positive[min(chunk.shape[0] * cfg.k, positive.numel()) - 1]) if positive.numel() else float("inf")
                keep = (top_acts.detach() > 0) & (top_acts.detach() >= theta)
                n_saturated += int(keep[:, -1].sum())
                lengths.append(keep.sum(1).to(torch.int32))
                thetas.append(theta)
                if theta == theta and abs(theta) != float("inf"):
                    threshold = theta if threshold < 0 else threshold + cfg.threshold_lr * (theta - threshold)
                top_acts = top_acts * keep
                fired = top_indices[keep]
            else:
                top_acts, top_indices = pre_acts.topk(cfg.k, sorted=False)
                fired = top_indices.flatten()
            sae_out = decode(top_acts, top_indices)
            e = sae_out - chunk
            if bounds:
                # Matryoshka: prefix reconstructions by masking; the descent is on their weighted FVUs
                prefix_fvu = [(decode(top_acts * (top_indices < m), top_indices) - chunk).pow(2).sum() / total_variance
                              for m in bounds]
                main = sum(w * f for w, f in zip(weights, prefix_fvu))
                for g, f in enumerate(prefix_fvu):
                    nested[g] += float(f.detach()) / len(chunks)
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
            loss = (main if bounds else fvu) + cfg.auxk_alpha * auxk_loss + multi_topk_fvu / 8
            loss.div(acc_steps).backward()
            for i, s in enumerate((fvu, auxk_loss, multi_topk_fvu)):
                stats[i] += float(s.detach()) / len(chunks)
            if cfg.multi_topk:
                fired = top_indices.flatten()
            did_fire[fired] = True
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
        log.append((stats, counts.clone(), substep == 0,
                    dict(theta=sum(thetas) / len(chunks) if batch else 0.0, threshold=threshold, n_saturated=n_saturated,
                         lengths=torch.cat(lengths) if batch else None, nested_fvu=nested)))
    moments = {n: (opt.state[P[n]]["exp_avg"], opt.state[P[n]]["exp_avg_sq"]) for n in R.NAMES}
    return {n: p.detach() for n, p in P.items()}, moments, log


NEW = ["batchtopk", "batchtopk_saturated", "matryoshka", "matryoshka_auxk", "matryoshka_batchtopk"]


@pytest.mark.parametrize("name", ["accumulate", "dead"] + NEW)
def test_restatement_equals_a_literal_torch_loop(name):
    sc = R.scenario(name, small=True)
    ref, results, _ = R.run_standalone(sc, f32_hyper=False)
    params, moments, log = _literal_loop(sc)
    assert any(r.clip < 1 for r in results) and any(r.clip == 1 for r in results)
    if name == "dead":
        k_aux = sc.d // 2
        assert any(0 < r.num_dead < k_aux for r in results) and any(r.num_dead > k_aux for r in results)
    for r, (stats, counts, stepped, more) in zip(results, log):
        assert r.stepped == stepped
        assert torch.equal(r.num_tokens_since_fired, counts)
        for i, n in enumerate(("fvu", "auxk_loss", "multi_topk_fvu")):
            assert abs(r.stats[n] - stats[i]) <= 1e-12 * abs(stats[i]), (n, r.stats[n], stats[i])
        if sc.cfg.activation == "batchtopk":
            assert abs(r.theta - more["theta"]) <= 1e-12 * abs(more["theta"]), (r.theta, more["theta"])
            assert abs(r.threshold - more["threshold"]) <= 1e-12 * abs(more["threshold"]), (r.threshold, more["threshold"])
            assert r.n_saturated == more["n_saturated"] and torch.equal(r.lengths, more["lengths"])
        assert len(r.nested_fvu) == len(sc.cfg.matryoshka)
        for got, want in zip(r.nested_fvu, more["nested_fvu"]):
            assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    for n in R.NAMES:
        for what, got, want in (("param", ref.p[n], params[n]), ("exp_avg", ref.m[n], moments[n][0]),
                                ("exp_avg_sq", ref.v[n], moments[n][1])):
            err = float((got - want).abs().max())
            assert err <= 1e-12 * float(want.abs().max()), (n, what, err)


# ---- 2. the preconditions of the GPU scenarios, from float64 alone -----------------------------------------------------
SCENARIOS = [("plain", True), ("plain", False), ("accumulate", True), ("dead", True), ("batch_sizes", True),
             ("batchtopk", True), ("batchtopk_saturated", True), ("matryoshka", True), ("matryoshka", False),
             ("matryoshka_auxk", True), ("matryoshka_batchtopk", True)]
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
    cfg = sc.cfg
    if cfg.activation == "batchtopk":
        print(f"  rows of length 0 {[int((r.lengths == 0).sum()) for r in results]}, longest {[int(r.lengths.max()) for r in results]}, "
              f"saturated {[r.n_saturated for r in results]}, theta {[round(r.theta, 5) for r in results]}")
    if name == "batchtopk":        # the length-aware decode's empty row, and no row at the cap
        assert all(bool((r.lengths == 0).any()) and r.n_saturated == 0 for r in results)
    if name == "batchtopk_saturated":
        for r in results:          # saturated and unsaturated rows in ONE chunk (the first of the two, 258 rows)
            first = r.lengths[:-(sc.tokens[0] // 2)]
            assert bool((first == cfg.cap).any()) and bool((first < cfg.cap).any()) and r.n_saturated > 0
        k_aux = sc.d // 2
        assert results[0].num_dead == sc.start_dead < k_aux and any(r.num_dead > k_aux for r in results)
        # the kept-prefix rule DECIDES a dead mask: an old feature that window 1 names in dropped slots only is dead in
        # window 2, and alive there under the rule "every listed feature has fired"
        _, listed, _ = R.run_standalone(sc, ("fired_from_listed_slots",))
        old = torch.zeros(sc.N, dtype=torch.bool)
        old[R.start_old_features(sc)] = True
        decided = results[-1].dead_mask & ~listed[-1].dead_mask & old
        print(f"  dead in the last batch {results[-1].num_dead}, under the listed rule {listed[-1].num_dead}, decided by the rule "
              f"{int(decided.sum())}")
        assert int(decided.sum()) > 0 and not bool((listed[-1].dead_mask & ~results[-1].dead_mask).any())
    if cfg.matryoshka:
        print(f"  fewest live entries per group {[r.groups_min for r in results]}, tokens with an empty first group "
              f"{[r.empty_first for r in results]}, nested fvu {[tuple(round(v, 4) for v in r.nested_fvu) for r in results]}")
        assert all(min(r.groups_min) > 0 for r in results) and any(r.empty_first > 0 for r in results)
        assert 0.0 in cfg.matryoshka_weights and len(set(cfg.matryoshka_weights)) == len(cfg.matryoshka) >= 3
        assert any(m % 64 for m in cfg.matryoshka)
        assert all(r.stats["fvu"] == r.nested_fvu[-1] for r in results)


# ---- 3. the checks have power -------------------------------------------------------------------------------------------
MUTANTS = [("bias_correction_t_plus_1", "plain"), ("lr_of_next_step", "plain"), ("no_clip_on_non_stepping", "accumulate"),
           ("dead_ge_threshold", "dead"), ("did_fire_from_k", "dead"), ("chunk_weight_by_token_share", "accumulate"),
           ("tokens_in_step_reset_every_batch", "accumulate"), ("scale_uncapped", "dead"), ("project_before_clip", "plain"),
           ("no_renorm", "plain"),
           ("fired_from_listed_slots", "batchtopk_saturated"), ("theta_rank_plus_1", "batchtopk"),
           ("keep_strictly_above_theta", "batchtopk"), ("threshold_folded_once_per_batch", "matryoshka_batchtopk"),
           ("threshold_first_value_averaged", "batchtopk"), ("descend_on_full_fvu", "matryoshka"),
           ("prefix_boundary_off_by_one", "matryoshka"), ("suffix_as_prefix", "matryoshka"),
           ("nested_coef_without_weight", "matryoshka"), ("auxk_target_ignores_kept_mask", "batchtopk_saturated")]
THRESHOLD = ("threshold_folded_once_per_batch", "threshold_first_value_averaged")      # moves `threshold` against its bound
EXACT = {"fired_from_listed_slots": "dead_mask", "theta_rank_plus_1": "theta", "keep_strictly_above_theta": "lengths",
         "bias_correction_t_plus_1": "t", "lr_of_next_step": "lr", "dead_ge_threshold": "dead_mask",
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
        if mutation in THRESHOLD:
            worst = max(worst, abs(q.threshold - r.threshold) / r.dthreshold if r.dthreshold > 0 else
                        (float("inf") if q.threshold != r.threshold else 0.0))
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
