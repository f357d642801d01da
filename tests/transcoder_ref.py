"""Float64 restatement of a transcoder and of a skip transcoder (SaeConfig(transcode=True, skip_connection=...); DESIGN.md
section 7u): the forward, the losses, every gradient through float64 autograd, and a literal float64 training loop -- the
same kind of judge as tests/lion_trainer_ref.py, with nothing of msae in it.  tests/test_transcoder_host.py holds the forward
to a hand-computed 3 x 4 x 6 case and shows that the trajectory criterion rejects three wrong trainers;
tests/test_gpu_transcoder.py judges the HIP path against it.

Definition (x [T, d_in] the module's input, y [T, d_out] its output):
    pre  = relu(x W_enc^T + b_enc)                       b_dec is NOT subtracted: it is an output bias of length d_out
    z    = the selection of pre ("topk": k per token, value descending, index ascending among equals;
           "batchtopk": of every token's top-C list the entries at or above the (T k)-th largest positive value of the batch)
    yhat = z W_dec + b_dec (+ x W_skip^T)                W_dec [N, d_out], W_skip [d_out, d_in]
    fvu  = sum (yhat - y)^2 / sum (y - mean_t y)^2
    AuxK = scale * sum (e_hat - (yhat - y))^2 / tv       e_hat = the top-k_aux dead latents decoded + b_dec, NO skip term;
                                                         k_aux = d_out // 2 (capped at the dead count), scale = min(dead / k_aux, 1)
    Multi-TopK = fvu of the top-4k reconstruction (with the skip term) / 8 in the loss

The bounds.  u = 2^-24.  A float32 pre-activation is an ascending fma chain of d_in products and the bias: d_in + 1 rounded
operations, so |pre32 - pre64| <= (d_in + 1) u (sum_j |x_j W_nj| + |b_n|) =: b[t, n] (first order, evaluated in float64).  A token
whose float64 k-th and (k+1)-th latents lie closer than the sum of their two bounds is UNDECIDED: float32 may legitimately pick
either, so such tokens are left out of the selection and of the yhat comparison, and their share is capped at TIE_CAP = 1 %,
the cap the project's trajectory tests keep.  yhat: the float32 activations of the list under test are first held to
b[t, n] of their float64 latents, then decoded in float64 as they are, and yhat must lie within n u sum |terms| of that, with n
the count of rounded operations on an output element's path (k + 1 for the decode chain and the bias, d_in for the skip chain,
1 for the join) and the terms the decode's products, b_dec and the skip products.  Nothing else is added to the bound.

The gradient criterion is the project's (tests/test_gpu_value_edits._assert_grads_close): |delta| <= 2e-3 max|ref| + 1e-8.

The trajectory criterion (`judge_step`), per optimiser step, from a state both sides share (the float64 loop is handed the
float32 parameters and moments of the trainer under test before every optimiser window, as tests/test_gpu_train_trajectory.py
does: six steps of a sign-like optimiser amplify one undecided element into a full lr step, which says nothing about the code):
  a. selections   exact outside the undecided tokens, whose share is at most TIE_CAP; the float64 loop then adopts them;
  b. gradients    what the trainer hands its optimiser, for EVERY parameter, inside the gradient criterion;
  c. parameters   after the step inside the gradient criterion of the float64 Adam step taken from the trainer's own
                  gradient: |delta| <= 2e-3 max|ref update| + 1e-8 with the UPDATE p' - p as the reference (the parameter
                  itself would hide an lr-sized error behind max|p| ~ 1);
  d. the decoder  W_dec's rows are not unit-norm when the run ends."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
TIE_CAP = 0.01
NAMES = ("W_enc", "b_enc", "W_dec", "b_dec", "W_skip")
RTOL, ATOL = 2e-3, 1e-8


def d64(t) -> torch.Tensor:
    return torch.as_tensor(t).detach().to("cpu", F64)


def grads_close(got, ref, what: str = "") -> float:
    """The project's gradient criterion -> the largest |delta| / (2e-3 max|ref| + 1e-8); raises AssertionError beyond 1."""
    got, ref = d64(got), d64(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    tol = RTOL * float(ref.abs().max()) + ATOL if ref.numel() else ATOL
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= tol, f"{what}: max |delta| {err:.3e} > {tol:.3e} (max |ref| {float(ref.abs().max()):.3e})"
    return err / tol


def canonical_topk(lat: torch.Tensor, k: int):
    """value descending, index ascending among equals"""
    v, i = torch.sort(lat, dim=-1, descending=True, stable=True)
    return v[..., :k], i[..., :k]


def pre_acts(P: Dict[str, torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    return torch.relu(x @ P["W_enc"].T + P["b_enc"])


def encoder_bound(P, x) -> torch.Tensor:
    """b[t, n] of the module docstring"""
    d_in = x.shape[1]
    return (d_in + 1) * U * (x.abs() @ P["W_enc"].abs().T + P["b_enc"].abs())


def undecided_tokens(pre: torch.Tensor, bound: torch.Tensor, k: int) -> torch.Tensor:
    """bool [T]: the float64 gap between rank k and rank k + 1 is below the two entries' bounds (or the row has fewer than
    k + 1 positive latents, where the tail is a tie at zero)."""
    v, i = canonical_topk(pre, k + 1)
    b = torch.gather(bound, 1, i)
    return (v[:, k - 1] - v[:, k] <= b[:, k - 1] + b[:, k]) | ~(v[:, k] > 0)


@dataclasses.dataclass
class Forward:
    yhat: torch.Tensor
    acts: torch.Tensor
    idx: torch.Tensor
    fvu: torch.Tensor
    auxk: torch.Tensor
    multi_fvu: torch.Tensor
    pre: torch.Tensor
    lengths: Optional[torch.Tensor] = None
    theta: Optional[float] = None
    loss: Optional[torch.Tensor] = None


def batch_keep(acts: torch.Tensor, k: int):
    """capped BatchTopK on [T, C] lists -> (keep mask, theta): the entries at or above the (T k)-th largest positive value"""
    pos = acts[acts > 0]
    if pos.numel() == 0:
        return torch.zeros_like(acts, dtype=torch.bool), float("inf")
    theta = float(torch.sort(pos, descending=True).values[min(acts.shape[0] * k, pos.numel()) - 1])
    return (acts > 0) & (acts >= theta), theta


def forward(P: Dict[str, torch.Tensor], x, y, k: int, *, multi_topk: bool = False, dead_mask: Optional[torch.Tensor] = None,
            auxk_alpha: float = 0.0, activation: str = "topk", cap: int = 0, idx=None, aux_idx=None, multi_idx=None,
            keep=None, mutate: Sequence[str] = ()) -> Forward:
    """The definition above on float64 tensors (leaves that require grad give gradients through autograd).  idx / aux_idx /
    multi_idx / keep: ADOPTED selections (index tensors, and for "batchtopk" the keep mask of the [T, C] lists) in place of
    this restatement's own.  `mutate` (the wrong trainers of the power tests): "subtract_b_dec" (d_out == d_in only)."""
    skip = P.get("W_skip") is not None
    xin = x - P["b_dec"] if "subtract_b_dec" in mutate else x
    pre = torch.relu(xin @ P["W_enc"].T + P["b_enc"])
    width = k if activation == "topk" else cap
    if idx is None:
        _, idx = canonical_topk(pre.detach(), width)
    acts = torch.gather(pre, 1, idx)
    lengths = theta = None
    if activation == "batchtopk":
        if keep is None:
            keep, theta = batch_keep(acts.detach(), k)
        acts = torch.where(keep, acts, torch.zeros((), dtype=acts.dtype))
        lengths = keep.sum(1)
    yhat = (acts[..., None] * P["W_dec"][idx]).sum(1) + P["b_dec"]
    if skip:
        yhat = yhat + x @ P["W_skip"].T
    tv = (y - y.mean(0)).pow(2).sum()
    e = yhat - y
    fvu = e.pow(2).sum() / tv
    auxk = yhat.new_zeros(())
    if dead_mask is not None and int(dead_mask.sum()) > 0:
        nd = int(dead_mask.sum())
        k_aux = y.shape[1] // 2
        scale = min(nd / k_aux, 1.0)
        k_aux = min(k_aux, nd)
        if aux_idx is None:
            _, aux_idx = canonical_topk(torch.where(dead_mask[None], pre.detach(), torch.full((), -float("inf"), dtype=pre.dtype)), k_aux)
        e_hat = (torch.gather(pre, 1, aux_idx)[..., None] * P["W_dec"][aux_idx]).sum(1) + P["b_dec"]       # no skip term
        auxk = scale * (e_hat - e).pow(2).sum() / tv
    multi = yhat.new_zeros(())
    if multi_topk:
        if multi_idx is None:
            _, multi_idx = canonical_topk(pre.detach(), 4 * k)
        ym = (torch.gather(pre, 1, multi_idx)[..., None] * P["W_dec"][multi_idx]).sum(1) + P["b_dec"]
        if skip:
            ym = ym + x @ P["W_skip"].T
        multi = (ym - y).pow(2).sum() / tv
    return Forward(yhat, acts, idx, fvu, auxk, multi, pre, lengths, theta, fvu + auxk_alpha * auxk + multi / 8)


def decode64(P, x, acts, idx) -> torch.Tensor:
    """yhat in float64 from GIVEN activations (the float32 list of the code under test, read exactly): sum_j acts_j W_dec[idx_j]
    + b_dec (+ x W_skip^T)."""
    out = (d64(acts)[..., None] * P["W_dec"][idx]).sum(1) + P["b_dec"]
    if P.get("W_skip") is not None:
        out = out + x @ P["W_skip"].T
    return out


def yhat_bound(P, x, acts, idx) -> torch.Tensor:
    """[T, d_out]: n u sum |terms| for yhat decoded from the given list -- n = k + 1 (the decode chain and the bias), with a
    skip connection + d_in (the skip chain) + 1 (the join); the terms are the decode's products, b_dec and the skip products.
    Nothing of the encoder enters: the activations are the float32 ones on both sides, and `acts_within_encoder_bound` judges
    them on their own."""
    k, d_in = idx.shape[1], x.shape[1]
    terms = (d64(acts).abs()[..., None] * P["W_dec"][idx].abs()).sum(1) + P["b_dec"].abs()
    n = k + 1
    if P.get("W_skip") is not None:
        terms = terms + x.abs() @ P["W_skip"].abs().T
        n += d_in + 1
    return n * U * terms


def acts_within_encoder_bound(P, x, acts, idx, live=None) -> float:
    """Every float32 activation of the list within b[t, n] of the float64 latent (slots outside `live`, a bool mask, must hold
    zero) -> the largest error / bound."""
    got = d64(acts)
    want, b = torch.gather(pre_acts(P, x), 1, idx), torch.gather(encoder_bound(P, x), 1, idx)
    if live is not None:
        assert not bool(got[~live].any()), "a dropped slot holds a value"
        want, b = torch.where(live, want, torch.zeros((), dtype=F64)), torch.where(live, b, torch.zeros((), dtype=F64))
    err = (got - want).abs()
    assert bool((err <= b).all()), f"an activation is off by {float((err / b.clamp_min(1e-300)).max()):.3f} encoder bounds"
    return float((err / b.clamp_min(1e-300)).max())


def gradients(P: Dict[str, torch.Tensor], x, y, k: int, want_x: bool = False, **kw):
    """-> (Forward, {name: dloss/dname} [, dloss/dx]) through float64 autograd, the loss being fvu + auxk_alpha auxk + multi / 8"""
    leaves = {n: p.detach().clone().requires_grad_(True) for n, p in P.items() if p is not None}
    xl = x.detach().clone().requires_grad_(want_x)
    fw = forward(leaves, xl, y, k, **kw)
    fw.loss.backward()
    g = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in leaves.items()}
    return (fw, g, xl.grad) if want_x else (fw, g)


# ---- the hand-computed case (test_transcoder_host.py): T = 3, d_in = 4, N = 6, d_out = 4, k = 2 ---------------------------------
def hand_case():
    """Small integers and halves: every product and sum below is exact in binary, so the expected values are literals."""
    W_enc = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0], [0, 0, 1, -1]], dtype=F64)
    b_enc = torch.tensor([0, 0, 0, 0, -1, 0.5], dtype=F64)
    W_dec = torch.tensor([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0], [0, 0, 0.5, 0.5]], dtype=F64)
    b_dec = torch.tensor([10, 0, 0, 0], dtype=F64)               # large: subtracting it in front of the encoder shows at once
    W_skip = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0.5, 0, 0, 0]], dtype=F64)
    x = torch.tensor([[2, 1, 0, 0], [0, 0, 3, 1], [1, 4, 0, 2]], dtype=F64)
    y = torch.tensor([[12, 0, 0, 0], [10, 0, 3, 2], [10, 8, 0, 3]], dtype=F64)
    P = dict(W_enc=W_enc, b_enc=b_enc, W_dec=W_dec, b_dec=b_dec, W_skip=W_skip)
    # pre (by hand): token 0: [2, 1, 0, 0, 2, .5]; token 1: [0, 0, 3, 1, 0, 2.5]; token 2: [1, 4, 0, 2, 4, 0]
    pre = torch.tensor([[2, 1, 0, 0, 2, 0.5], [0, 0, 3, 1, 0, 2.5], [1, 4, 0, 2, 4, 0]], dtype=F64)
    # top-2, value descending, index ascending among equals: token 0: (0: 2), (4: 2); token 1: (2: 3), (5: 2.5); token 2: (1: 4), (4: 4)
    idx = torch.tensor([[0, 4], [2, 5], [1, 4]])
    acts = torch.tensor([[2, 2], [3, 2.5], [4, 4]], dtype=F64)
    # decode + b_dec: token 0: 2 e0 + 2 (e0 + e1) + 10 e0 = [14, 2, 0, 0]; token 1: 3 e2 + 2.5 (.5 e2 + .5 e3) + 10 e0 = [10, 0, 4.25, 1.25];
    # token 2: 4 * 2 e1 + 4 (e0 + e1) + 10 e0 = [14, 12, 0, 0]
    plain = torch.tensor([[14, 2, 0, 0], [10, 0, 4.25, 1.25], [14, 12, 0, 0]], dtype=F64)
    # skip: yhat[:, 3] += .5 x[:, 0] -> + [1, 0, .5]
    with_skip = plain + torch.tensor([[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0.5]], dtype=F64)
    # errors with the skip: token 0: [2, 2, 0, 1] -> 9; token 1: [0, 0, 1.25, -.75] -> 2.125; token 2: [4, 4, 0, -2.5] -> 38.25: 49.375
    # total variance: column means [32/3, 8/3, 1, 5/3]: sums of squares 8/3, 128/3, 6, 14/3 -> 56
    return dict(P=P, x=x, y=y, k=2, pre=pre, idx=idx, acts=acts, plain=plain, with_skip=with_skip, sq_err=49.375,
                sq_err_plain=4 + 4 + 0 + 0 + 1.5625 + 0.5625 + 16 + 16 + 9, tv=56.0)


# ---- scenarios -----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Scenario:
    name: str
    d_in: int = 256
    d_out: int = 192
    N: int = 8192
    k: int = 32
    T: int = 300
    steps: int = 6
    skip: bool = False
    lr: float = 2e-4
    auxk_alpha: float = 0.0
    multi_topk: bool = False
    dead_feature_threshold: int = 10_000_000
    start_dead: int = 0
    grad_acc_steps: int = 1
    micro_acc_steps: int = 1
    activation: str = "topk"
    cap: int = 0
    seed: int = 5
    nnz: int = 10                      # nonzero coordinates per token
    weak: int = 150                    # features (the last ones) too short ever to fire

    @property
    def batches(self) -> int:
        return self.steps * self.grad_acc_steps


SCENARIOS = {
    "transcoder": Scenario("transcoder"),
    "skip": Scenario("skip", skip=True, seed=6),
    "skip_auxk_dead": Scenario("skip_auxk_dead", skip=True, auxk_alpha=1 / 32, multi_topk=True, start_dead=50,
                               dead_feature_threshold=600, seed=7),
    "skip_accumulate": Scenario("skip_accumulate", skip=True, T=301, grad_acc_steps=2, micro_acc_steps=2, seed=6),
    "skip_batchtopk": Scenario("skip_batchtopk", skip=True, activation="batchtopk", k=16, cap=64, seed=6),
}


def small(sc: Scenario) -> Scenario:
    """The host tests' size of a scenario: the same schedule on a dictionary a CPU trains in a second."""
    return dataclasses.replace(sc, d_in=24, d_out=24 if sc.name == "transcoder" else 20, N=256, k=4 if sc.activation == "topk" else 3,
                               cap=0 if sc.activation == "topk" else 12, T=sc.T // 4, start_dead=min(sc.start_dead, 6),
                               dead_feature_threshold=sc.dead_feature_threshold // 4, nnz=6, weak=24)


def make_params(sc: Scenario) -> Dict[str, torch.Tensor]:
    """float32 values.  The encoder is tests/trainer_ref.py's construction: feature n reads coordinate n % d_in, N / d_in
    features per coordinate alternating in sign, their lengths a jittered geometric ladder, plus dense noise of 0.002 -- with
    tokens of few nonzero coordinates every pre-activation is ONE dominant product, so the encoder bound stays small against
    the gap at rank k: that is what holds the undecided share under TIE_CAP.  The last `weak` features are 1000 times shorter
    and never reach a top-k (the dead-feature scenario starts its dead features there).  W_dec starts at zero (the module's
    initialisation); b_dec and, with a skip connection, W_skip start away from zero so that the first step's gradients of
    every parameter are alive and a b_dec subtracted in front of the encoder changes the selection."""
    g = torch.Generator().manual_seed(sc.seed)
    N, d = sc.N, sc.d_in
    n = torch.arange(N)
    rung = (n // d) // 2
    sign = 1.0 - 2.0 * ((n // d) % 2).to(F64)
    length = 0.25 * 0.9 ** rung.to(F64) * (1.0 + 0.06 * (torch.rand(N, generator=g, dtype=F64) - 0.5))
    We = torch.randn(N, d, generator=g, dtype=F64) * 0.002
    We[n, n % d] += sign * length
    We[N - sc.weak:] *= 1e-3
    P = {"W_enc": We.float().contiguous(), "b_enc": (torch.randn(N, generator=g) * 2e-4).float(),
         "W_dec": torch.zeros(N, sc.d_out), "b_dec": (torch.randn(sc.d_out, generator=g) * 0.5).float()}
    if sc.skip:
        P["W_skip"] = (torch.randn(sc.d_out, sc.d_in, generator=g) * (0.1 / d ** 0.5)).float()
    return P


def make_batches(sc: Scenario):
    """[(x [T, d_in], y [T, d_out])] float32: tokens with `nnz` nonzero coordinates (standard normal); y is a fixed random
    linear map of x plus a nonlinearity of it and noise, so both the sparse and the dense path have something to learn."""
    g = torch.Generator().manual_seed(sc.seed + 1)
    A = torch.randn(sc.d_out, sc.d_in, generator=g, dtype=F64) / sc.nnz ** 0.5
    out = []
    for _ in range(sc.batches):
        x = torch.zeros(sc.T, sc.d_in, dtype=F64)
        pos = torch.rand(sc.T, sc.d_in, generator=g).topk(sc.nnz, dim=1).indices
        x.scatter_(1, pos, torch.randn(sc.T, sc.nnz, generator=g, dtype=F64))
        h = x @ A.T
        out.append((x.float(), (torch.relu(h) + 0.25 * h + 0.05 * torch.randn(sc.T, sc.d_out, generator=g, dtype=F64)).float()))
    return out


def initial_counts(sc: Scenario) -> torch.Tensor:
    c = torch.zeros(sc.N, dtype=torch.long)
    if sc.start_dead:
        c[sc.N - sc.weak + torch.arange(sc.start_dead) * (sc.weak // sc.start_dead)] = sc.dead_feature_threshold + 1
    return c


# ---- the literal float64 loop --------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class StepRecord:
    sel: List[dict]                       # per chunk: idx, aux_idx, multi_idx, keep (what was selected), undecided [T_chunk]
    G: Dict[str, torch.Tensor]            # the accumulated gradients handed to the optimiser (before the clip)
    stepped: bool
    params: Optional[Dict[str, torch.Tensor]] = None      # after the optimiser step
    clip: float = 1.0
    num_dead: int = 0


class Loop:
    """SaeTrainStep's loop for a transcoder, literally, on float64 tensors: micro-chunks weighted 1 / acc_steps, gradients
    accumulated over grad_acc_steps batches, clip_grad_norm_(1.0) on every batch, NO decoder normalisation and NO projection,
    Adam (betas 0.9 / 0.999, eps 1e-8, constant lr), dead-feature counts for the AuxK mask."""

    def __init__(self, sc: Scenario, params: Dict[str, torch.Tensor], mutate: Sequence[str] = ()):
        self.sc, self.mutate = sc, tuple(mutate)
        self.p = {n: d64(v).clone() for n, v in params.items()}
        self.m = {n: torch.zeros_like(v) for n, v in self.p.items()}
        self.v = {n: torch.zeros_like(v) for n, v in self.p.items()}
        self.G: Optional[Dict[str, torch.Tensor]] = None
        self.t = 0
        self.global_step = 0
        self.counts = initial_counts(sc)
        self.did_fire = torch.zeros(sc.N, dtype=torch.bool)
        self.tokens_in_step = 0

    def load_state(self, params, exp_avg, exp_avg_sq) -> None:
        assert self.G is None, "state is synchronised between optimiser steps, not inside a window"
        for n in self.p:
            self.p[n], self.m[n], self.v[n] = d64(params[n]).clone(), d64(exp_avg[n]).clone(), d64(exp_avg_sq[n]).clone()

    def batch(self, x, y, selections: Optional[List[dict]] = None) -> StepRecord:
        sc = self.sc
        x, y = d64(x), d64(y)
        dead = self.counts > sc.dead_feature_threshold if sc.auxk_alpha > 0 else None
        acc = sc.grad_acc_steps * sc.micro_acc_steps
        xs, ys = x.chunk(sc.micro_acc_steps), y.chunk(sc.micro_acc_steps)
        sel_out = []
        if "normalize_decoder" in self.mutate:
            self.p["W_dec"] = self.p["W_dec"] / (self.p["W_dec"].norm(dim=1, keepdim=True) + float(torch.finfo(torch.float32).eps))
        for ci, (xc, yc) in enumerate(zip(xs, ys)):
            given = selections[ci] if selections is not None else {}
            fw, g = gradients(self.p, xc, yc, sc.k, multi_topk=sc.multi_topk, dead_mask=dead, auxk_alpha=sc.auxk_alpha,
                              activation=sc.activation, cap=sc.cap, idx=given.get("idx"), aux_idx=given.get("aux_idx"),
                              multi_idx=given.get("multi_idx"), keep=given.get("keep"),
                              mutate=[m for m in self.mutate if m == "subtract_b_dec"])
            if "drop_skip_grad" in self.mutate and "W_skip" in g:
                g["W_skip"] = torch.zeros_like(g["W_skip"])
            if self.G is None:
                self.G = {n: torch.zeros_like(v) for n, v in self.p.items()}
            for n in self.G:
                self.G[n] += g[n] / acc
            width = sc.k if sc.activation == "topk" else sc.cap
            bound = encoder_bound(self.p, xc)
            if sc.activation == "topk":
                und = undecided_tokens(fw.pre.detach(), bound, width)
            else:
                # the batch-level selection: an entry within its bound (and theta's own: twice) of theta64 may fall on either
                # side; the gap at rank C forks something only in a row that keeps all C slots
                b = torch.gather(bound, 1, fw.idx)
                raw = torch.gather(fw.pre.detach(), 1, fw.idx)
                theta = fw.theta if fw.theta is not None else float(raw[given["keep"]].min())     # (adopted: the smallest kept)
                und = ((raw > 0) & ((raw - theta).abs() <= 2 * b)).any(1) | \
                    ((fw.lengths == width) & undecided_tokens(fw.pre.detach(), bound, width))
            kept = fw.idx if fw.lengths is None else fw.idx[torch.arange(width)[None] < fw.lengths[:, None]]
            fired = kept if not sc.multi_topk else canonical_topk(fw.pre.detach(), 4 * sc.k)[1] if given.get("multi_idx") is None \
                else given["multi_idx"]
            self.did_fire[fired.reshape(-1)] = True
            sel_out.append({"idx": fw.idx, "lengths": fw.lengths, "theta": fw.theta, "undecided": und, "pre": fw.pre.detach(), "bound": bound,
                            "acts": fw.acts.detach()})
        self.tokens_in_step += x.shape[0]
        self.global_step += 1
        stepped = self.global_step % sc.grad_acc_steps == 0
        total = float(sum(float(g.pow(2).sum()) for g in self.G.values())) ** 0.5
        clip = min(1.0, 1.0 / (total + 1e-6))
        rec = StepRecord(sel_out, {n: g.clone() for n, g in self.G.items()}, stepped, clip=clip,
                         num_dead=0 if dead is None else int(dead.sum()))
        for n in self.G:
            self.G[n] = self.G[n] * clip
        if stepped:
            self.t += 1
            for n in self.p:
                self.p[n], self.m[n], self.v[n] = adam(self.p[n], self.G[n], self.m[n], self.v[n], self.t, sc.lr)
            self.G = None
            self.counts += self.tokens_in_step
            self.counts[self.did_fire] = 0
            self.tokens_in_step = 0
            self.did_fire.zero_()
            rec.params = {n: v.clone() for n, v in self.p.items()}
        return rec


def adam(p, g, m, v, t: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
    """torch.optim.Adam's step -> (p', m', v')"""
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    return p - lr * (m / (1 - betas[0] ** t)) / ((v / (1 - betas[1] ** t)).sqrt() + eps), m, v


def run_standalone(sc: Scenario, mutate: Sequence[str] = ()):
    loop = Loop(sc, make_params(sc), mutate)
    return loop, [loop.batch(x, y) for x, y in make_batches(sc)]


# ---- the trajectory criterion ----------------------------------------------------------------------------------------------------
def judge_selection(got_idx, ref_idx, undecided, what: str = "") -> float:
    """Rows equal as SETS outside the undecided tokens (inside a row the float32 order of near-equal values is its own) ->
    the share of undecided tokens, at most TIE_CAP."""
    got, ref = torch.sort(torch.as_tensor(got_idx).cpu().long(), dim=1).values, torch.sort(ref_idx.long(), dim=1).values
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    wrong = (got != ref).any(1) & ~undecided
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} decided tokens with another selection, first {int(wrong.nonzero()[0])}"
    share = float(undecided.double().mean())
    assert share <= TIE_CAP, f"{what}: {share:.4f} of the tokens are undecided in float64 (cap {TIE_CAP})"
    return share


def judge_step(got_G: Dict[str, torch.Tensor], got_before: Dict[str, torch.Tensor], got_after: Optional[Dict[str, torch.Tensor]],
               got_moments, ref: StepRecord, t: int, lr: float, what: str = "") -> Dict[str, float]:
    """(b) and (c) of the module docstring for one batch: got_G the gradients the trainer hands its optimiser (unclipped),
    got_before / got_after its parameters around the step (None on a batch that does not step), got_moments = {name: (m, v)}
    before the step -> the largest error / tolerance per check."""
    worst = {"gradient": 0.0, "update": 0.0}
    for n, g in ref.G.items():
        # (W_dec starts at zero: at the first step nothing depends on the encoder yet, and its two gradients are exactly zero)
        assert float(g.abs().max()) > 0 or (t == 1 and n in ("W_enc", "b_enc")), \
            f"{what}: the reference gradient of {n} is zero: the scenario checks nothing"
        worst["gradient"] = max(worst["gradient"], grads_close(got_G[n], g, f"{what} gradient of {n}"))
    if got_after is not None:
        total = float(sum(float(d64(g).pow(2).sum()) for g in got_G.values())) ** 0.5
        clip = min(1.0, 1.0 / (total + 1e-6))
        for n in ref.G:
            m, v = got_moments[n]
            p1, _, _ = adam(d64(got_before[n]), d64(got_G[n]) * clip, d64(m), d64(v), t, lr)
            worst["update"] = max(worst["update"], grads_close(d64(got_after[n]) - d64(got_before[n]), p1 - d64(got_before[n]),
                                                               f"{what} update of {n}"))
    return worst
