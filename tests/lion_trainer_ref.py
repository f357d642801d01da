"""tests/trainer_ref.py with the sign-momentum optimiser in place of Adam: SaeTrainStep(optimizer="lion") is judged against
this by test_gpu_lion_trajectory.py, and test_lion_trainer_ref_host.py holds it against a literal autograd loop.  Everything
but the optimiser step -- forward, backward, clip, projection, schedule, dead-feature bookkeeping, the bounds of the gradients
and of the statistics -- is TrainerRef's, unchanged; the optimiser carries one moment and no second one.

The scenarios are trainer_ref.scenario's `plain`, `accumulate` and `dead` with betas (0.9, 0.99) and LION_LR.

LION_LR = 2e-5.  A sign step moves EVERY element of a row that has a gradient by lr, where Adam at the scenarios' 2e-4 moves
an element by about lr m / sqrt(v): the 0.002 noise floor of the 256 coordinates a feature does not read takes the same step as
the one coordinate it does.  The scenarios' preconditions are statements about float64 (the share of tokens whose gap at rank
k is below 2 b_t stays under 1 %, the clip is active in one batch and inactive in another, the dead-feature counts cross
k_aux), so the value was chosen with this restatement alone, starting from 2e-5 as a tenth of the Adam value: over five
optimiser steps the features move by at most 1e-4 per coordinate, a twentieth of the noise floor, and
test_lion_trainer_ref_host.py shows that every precondition then holds as it does for Adam (largest near-tie share of a batch:
0.39 % in `plain` and `dead`, 0.78 % in `accumulate`, printed there; the cap is 1 %), so the first value tried was kept.
Nothing about the value comes from a GPU run."""
from __future__ import annotations

import dataclasses
from typing import Sequence

import torch

import train_ref as tr
import trainer_ref as R

LION_LR = 2e-5
LION_BETAS = (0.9, 0.99)
SCENARIOS = ("plain", "accumulate", "dead")
TIE_CAP = 0.01


class LionTrainerRef(R.TrainerRef):
    """TrainerRef whose optimiser step is Lion: u = m + (g - m)(1 - b1), p -= lr sign(u), m += (g - m)(1 - b2)."""

    def __init__(self, cfg, params, mutate: Sequence[str] = (), f32_hyper: bool = True):
        super().__init__(cfg, params, mutate, f32_hyper)
        self.v = None                                  # no second moment

    def load_state(self, params, exp_avg, exp_avg_sq=None) -> None:
        assert self.G is None, "state is synchronised between optimiser steps, not inside a window"
        assert exp_avg_sq is None or all(v is None for v in exp_avg_sq.values()), "a sign optimiser has no second moment"
        for n in R.NAMES:
            self.p[n], self.m[n] = tr._d(params[n]).clone(), tr._d(exp_avg[n]).clone()
        self.dWd = torch.zeros_like(self.p["W_dec"])

    def _adam(self, step: int, lr: float) -> None:
        """The sign-momentum step on the (clipped, projected) window gradients; `step` plays no part (no bias correction)."""
        b1, b2, lr = self._h(self.cfg.betas[0]), self._h(self.cfg.betas[1]), self._h(lr)
        for n in R.NAMES:
            g, m = self.G[n], self.m[n]
            u = m + (g - m) * (1.0 - b1)
            self.p[n] = self.p[n] - lr * torch.sign(u)
            self.m[n] = m + (g - m) * (1.0 - b2)
        self.dWd = torch.zeros_like(self.p["W_dec"])


def scenario(name: str, small: bool = False, lr: float = LION_LR) -> R.Scenario:
    assert name in SCENARIOS, name
    sc = R.scenario(name, small=small)
    return dataclasses.replace(sc, cfg=dataclasses.replace(sc.cfg, lr=lr, betas=LION_BETAS))


def run_standalone(sc: R.Scenario, f32_hyper: bool = True):
    """The restatement on its own selections over the scenario's batches -> (LionTrainerRef, [BatchResult])."""
    ref = LionTrainerRef(sc.cfg, R.make_params(sc), (), f32_hyper)
    ref.num_tokens_since_fired = R.initial_counts(sc)
    return ref, [ref.batch(x) for x in R.make_batches(sc)]


def assert_preconditions(sc: R.Scenario, results, counts_at_end) -> None:
    """What test_trainer_ref_host.py asserts of the Adam scenarios, on a run of the Lion ones (either side's results)."""
    assert max(r.tie_share for r in results) <= TIE_CAP, [r.tie_share for r in results]
    assert any(r.clip < 1 for r in results) and any(r.clip == 1 for r in results), [r.clip for r in results]
    if sc.name == "plain":
        lrs = [r.lr for r in results]
        assert lrs[0] == 0.0 and lrs[2] == sc.cfg.lr and lrs[4] < lrs[3] < lrs[2], lrs
    if sc.name == "accumulate":
        assert [r.stepped for r in results] == [False, True] * 3
        assert any(r.clip < 1 for r in results if not r.stepped) and any(r.clip == 1 for r in results if not r.stepped)
    if sc.name == "dead":
        k_aux = sc.d // 2
        assert results[0].num_dead == sc.start_dead < k_aux and 0 < results[0].scale < 1
        assert any(r.num_dead > k_aux and r.scale == 1.0 for r in results)
        assert bool((counts_at_end[R.start_dead_features(sc)] > sc.cfg.dead_feature_threshold).any())
