"""Host tests of tests/lion_trainer_ref.py, the float64 restatement test_gpu_lion_trajectory.py judges
SaeTrainStep(optimizer="lion") against.  No GPU, nothing of msae.

  1. In the `small=True` forms of `plain`, `accumulate` and `dead` the subclass equals the LITERAL loop of
     test_trainer_ref_host.py (autograd, LambdaLR, clip_grad_norm_, in float64) driven by a literal Lion written as a
     torch.optim.Optimizer in the paper's form -- agreement to 1e-12 relative, the counts exactly.
  2. At the GPU sizes and lion_trainer_ref.LION_LR every precondition of the scenarios holds from float64 alone."""
import pytest
import torch

import lion_trainer_ref as LR
import trainer_ref as R
from test_trainer_ref_host import _literal_loop


class _LiteralLion(torch.optim.Optimizer):
    """Lion as Chen et al. write it: u = b1 m + (1 - b1) g; p -= lr sign(u); m = b2 m + (1 - b2) g.  No weight decay.  (It
    answers to the constructor call and the state keys the literal loop uses for torch.optim.Adam.)"""

    def __init__(self, params, lr, betas, eps=None):
        super().__init__(params, dict(lr=lr, betas=betas))

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                st = self.state[p]
                if not st:
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), None
                m = st["exp_avg"]
                u = b1 * m + (1 - b1) * p.grad
                p.add_(torch.sign(u), alpha=-group["lr"])
                m.mul_(b2).add_(p.grad, alpha=1 - b2)


@pytest.mark.parametrize("name", LR.SCENARIOS)
def test_subclass_equals_a_literal_autograd_and_lion_loop(name, monkeypatch):
    sc = LR.scenario(name, small=True)
    ref, results = LR.run_standalone(sc, f32_hyper=False)
    monkeypatch.setattr(torch.optim, "Adam", _LiteralLion)
    params, moments, log = _literal_loop(sc)
    assert ref.v is None
    assert any(r.clip < 1 for r in results) and any(r.clip == 1 for r in results)
    for r, (stats, counts, stepped, _) in zip(results, log):
        assert r.stepped == stepped and torch.equal(r.num_tokens_since_fired, counts)
        for i, n in enumerate(("fvu", "auxk_loss", "multi_topk_fvu")):
            assert abs(r.stats[n] - stats[i]) <= 1e-12 * abs(stats[i]), (n, r.stats[n], stats[i])
    moved = 0.0
    init = R.make_params(sc)
    for n in R.NAMES:
        for what, got, want in (("param", ref.p[n], params[n]), ("exp_avg", ref.m[n], moments[n][0])):
            err = float((got - want).abs().max())
            assert err <= 1e-12 * float(want.abs().max()), (n, what, err)
        assert moments[n][1] is None
        moved = max(moved, float((ref.p[n] - init[n].double()).abs().max()))
    assert moved >= sc.cfg.lr, "the optimiser took no step"


@pytest.mark.parametrize("name", LR.SCENARIOS)
def test_gpu_scenarios_meet_their_preconditions_at_the_chosen_lr(name):
    sc = LR.scenario(name)
    assert sc.cfg.lr == LR.LION_LR and sc.cfg.betas == LR.LION_BETAS and (sc.d, sc.N) == (256, 8192)
    ref, results = LR.run_standalone(sc)
    print(f"\n{name} at lr {sc.cfg.lr}: near-tie share per batch {[round(r.tie_share, 4) for r in results]}, "
          f"clip {[round(r.clip, 3) for r in results]}, dead {[r.num_dead for r in results]}")
    LR.assert_preconditions(sc, results, ref.num_tokens_since_fired)
