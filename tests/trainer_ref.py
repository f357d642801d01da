"""Float64 restatement of the reference TRAINING LOOP for one hookpoint (train/sae/sae/trainer.py:347-414: renormalise, forward
and backward per micro-chunk, clip_grad_norm_ on every batch, and on every grad_acc_steps-th batch the removal of the
decoder-parallel gradient, Adam, the scheduler step and the dead-feature update; sae.py:193-271 for the forward with AuxK and
Multi-TopK, the unit norm and the parallel-gradient removal; transformers' get_linear_schedule_with_warmup as its
documentation states it) with DERIVED bounds on what a correct float32 evaluation may differ by.  It imports nothing from
msae, runs on the CPU, and no number in it is fitted to what a GPU produced.  tests/train_ref.py is the template: the same
error model (U, SAFETY, one safety factor at the end), the same `assert_within`, its `adam_rows` / `unit_norm_rows`.

The forward and backward are written out by hand (dense [T, N] pre-activations, the rest over the selected pairs, no
autograd), because every intermediate carries a value AND a bound; test_trainer_ref_host.py holds the hand-written
gradients against a literal autograd loop driven by torch.optim.Adam, LambdaLR and clip_grad_norm_ to 1e-12.

State: params, exp_avg, exp_avg_sq, t (optimiser = scheduler steps), global_step (batches), num_tokens_since_fired, did_fire,
num_tokens_in_step, and the gradients accumulated inside a window.  `TrainerRef.batch(x, selections)` takes one batch and
returns a `BatchResult`: per parameter the float64 gradient G as the optimiser pass receives it (stepping batch: accumulated,
NOT yet clipped -- the port clips inside its Adam pass) or as it is left in .grad (other batches: clipped in place), the
elementwise bound dG on |G_f32 - G|, the three statistics with bounds, and the bookkeeping.

Selections.  With `selections=None` the restatement takes its own torch.topk of the float64 latents (standalone mode).
Otherwise the caller hands over, per micro-chunk, the [(values, indices)] the float32 side selected (main, AuxK, Multi-TopK);
each is checked to be a valid top-k of the float64 latents within the bound b_t of one pre-activation

    b_t = SAFETY (d + 2) u (sum_c |a_c| |w_c| + |b|)          (a = x - b_dec: one rounding; d products, d adds, the bias)

(values within b_t; min over selected + b_t >= max over unselected - b_t, over the dead set for AuxK), and is then ADOPTED, with
the float32 side's ReLU mask where |p64| <= b_t (elsewhere the masks must agree), so that a near-tie cannot fork the
trajectory.  `tie_share` is the share of tokens whose float64 gap at rank k is below 2 b_t (ties among zeros aside: they
carry neither value nor gradient).

BatchTopK (TrainerConfig.activation = "batchtopk"; msae: SaeConfig(activation="batchtopk")).  The main
selection has the list width C = cap.  Standalone: the float64 top-C lists; theta64 = the (T_chunk k)-th largest positive list
entry (the smallest positive one when there are fewer, +inf when none); an entry is kept iff v > 0 and v >= theta.  Adopting: the
caller also hands over, per chunk, what ops.batch_select returned for the list (kept values, lengths, theta, n_saturated).  (i)
the list passes `_adopt` with kk = C; (ii) the four results equal, BIT FOR BIT, batch_select_ref.batch_select of the float32
list (the list itself must descend); (iii) over the whole chunk min over kept (lat64 + b_t) >= max over dropped positive list
entries (lat64 - b_t), and at least min(T k, positives) entries are kept; (iv) the keep mask and the ReLU mask are adopted.
The decode, every gradient, the statistics and did_fire see the kept entries only; AuxK's target is the residual of the kept
reconstruction.  Per CHUNK theta is folded into `threshold` (from -1: the first finite theta is copied, then thr +=
threshold_lr (theta - thr); a non-finite theta is skipped); per batch BatchResult carries theta (the mean over the chunks),
threshold, n_saturated and lengths.  `tie_share` of this selection is the share of the chunk's T k kept slots that float64
leaves undecided: positive list entries within 2 b_t of theta64, plus rows saturated in float64 whose gap at rank C is below
2 b_t (a tie at rank C of an unsaturated row forks nothing -- its tail is dropped -- and does not count).

Matryoshka (TrainerConfig.matryoshka / matryoshka_weights).  out_g decodes the selected (kept) entries
with idx < bounds[g], e_g = out_g - x, nested_fvu[g] = sum e_g^2 / tv; the descended main term is sum_g w_g nested_fvu[g] and
fvu = nested_fvu[-1] is a statistic.  The decode output of group h receives S_h = grad_full + sum_{g >= h} c_g e_g with
c_g = weight 2 w_g / tv (nested_ref's combine); W_dec row n gets sum v S_group(n)[t], a latent S_group(i)[t] . W_dec[i], b_dec
sum_t S_0[t]; grad_full is the AuxK term's gradient into the full reconstruction.

Error model (u = 2^-24; to first order, ONE factor SAFETY at the end).  Every intermediate is a pair (value, bound):
  * an elementwise float32 operation adds u |result|; a scalar coefficient built from a handful of float32 scalar operations
    (2 / total_variance / acc_steps, alpha, scale, 1 / 8) carries 6 u plus the relative bound of the total variance;
  * a float32 sum adds depth * u * sum |terms| on top of the propagated input intervals.  `depth` where the order is ours:
        decode (sae_out, e_hat)        k + 1        the j-ordered fma chain and the bias add, csrc/decode.hip:33-79
        decode of a kept prefix        len + 1      decode_prefix_v4_kernel walks the first len entries of a row, one fma each,
                                                    then the bias add (csrc/batch_select.hip:229-277): <= C + 1
        prefix decode r_g              n_g + 1      the live entries of the groups 0 .. g in group-major order, one fma each
                                                    (nd_walk, csrc/nested_decode.hip:79, walked to the checkpoint s_ck[g],
                                                    :162-169) and the bias add (:173); e_g = r_g - x is one subtract (:174)
        combine S_h                    G + 1        one fma per plane from the last plane down, from grad_full or +0
                                                    (csrc/nested_decode.hip:247-255; nested_ref states the same G + 1)
        decoder backward, g_acts       d / 64 + 7   the lane's fma chain (d / 64 terms, own product), 6 shuffle levels,
                                                    csrc/decode.hip:131-143
        weight gradients (both)        L + 1        wgrad_accum_kernel's ascending pair order: one fma chain over the row's L
                                                    pairs, csrc/decode.hip:308-341 (L counts every selected pair of the call;
                                                    "batchtopk": the KEPT pairs -- wgrad_count_kernel and wgrad_fill_kernel
                                                    leave a pair with activation 0 out of the segment, csrc/decode.hip:177,
                                                    235, and a dropped slot reaches them as 0).  The grouped forms
                                                    (csrc/decode.hip:138, 276) only choose the plane a row is read from
        b_dec through the encoder      train_ref.weighted_row_sum's depth (csrc/train.hip, msae_weighted_row_sum_f32)
    and depth = the number of terms where the order is not ours (valid for ANY order):
        encoder bias gradient          L            (row_act_sum, csrc/decode.hip:355-358, is shallower: ceil(L / 64) + 6)
        b_dec through a decode         T            grad_out.sum(0), a torch reduction
        total variance                 T + d + 8    torch.var over the tokens, the sum over d, the product with T
        squared-error sums             T d          torch.linalg.vector_norm; the nested node's sq (lane fma chain, wave
                                                    butterfly, four waves, slabs: csrc/nested_decode.hip:175-187, then
                                                    sq.sum(0) over the tokens) is one order among those
        theta's mean, the threshold    chunks; 4    the float32 running sum of the chunks' thetas and its division; one fold is a
                                                    subtract, a product with the float32 rate and an add: 4 u (|thr| + |theta|)
                                                    per fold on top of the state's own bound (msae/train.py, _fold_threshold)
        clip_grad_norm_'s total        all parameter elements (torch._foreach_norm and the norm of the four norms)
    autograd adding two contributions of one parameter (the three decodes, the chunks of a window) is one u each;
  * W_dec as the float32 side holds it after its own renormalisation differs from the float64 renormalisation by
    train_ref._renorm's bound, carried as an input interval.

Mutations (`mutate`): the wrong restatements test_trainer_ref_host.py proves the checks reject -- MUTATIONS below."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import train_ref as tr
from train_ref import F64, SAFETY, U, f32

NAMES = ("W_enc", "b_enc", "W_dec", "b_dec")

MUTATIONS = ("bias_correction_t_plus_1", "lr_of_next_step", "no_clip_on_non_stepping", "dead_ge_threshold",
             "did_fire_from_k", "chunk_weight_by_token_share", "tokens_in_step_reset_every_batch", "scale_uncapped",
             "project_before_clip", "no_renorm",
             # "batchtopk"  and matryoshka (section 7o)
             "fired_from_listed_slots", "theta_rank_plus_1", "keep_strictly_above_theta", "threshold_folded_once_per_batch",
             "threshold_first_value_averaged", "descend_on_full_fvu", "prefix_boundary_off_by_one", "suffix_as_prefix",
             "nested_coef_without_weight", "auxk_target_ignores_kept_mask")


def linear_schedule_with_warmup(step: int, warmup: int, total: Optional[int]) -> float:
    """The multiplier get_linear_schedule_with_warmup documents: linear 0 -> 1 over `warmup` scheduler steps, then linear
    1 -> 0 at `total` (never below 0); constant 1 after the warm-up when there is no total."""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    if total is None:
        return 1.0
    return max(0.0, float(total - step) / float(max(1, total - warmup)))


@dataclass(frozen=True)
class TrainerConfig:
    k: int
    lr: float
    multi_topk: bool = False
    normalize_decoder: bool = True
    auxk_alpha: float = 0.0
    dead_feature_threshold: int = 10_000_000
    grad_acc_steps: int = 1
    micro_acc_steps: int = 1
    lr_warmup_steps: int = 0
    total_steps: Optional[int] = None
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    max_norm: float = 1.0
    activation: str = "topk"                  # "topk" or "batchtopk"
    cap: int = 0                              # "batchtopk": the list width C of the main selection
    threshold_lr: float = 0.01                # "batchtopk": the rate every chunk's theta is folded into the threshold at
    matryoshka: Tuple[int, ...] = ()          # prefix sizes, the last one N; empty: the plain loss
    matryoshka_weights: Tuple[float, ...] = ()    # one loss weight per prefix, explicit

    def __post_init__(self):
        assert self.activation in ("topk", "batchtopk"), self.activation
        if self.multi_topk and (self.activation == "batchtopk" or self.matryoshka):
            raise ValueError("multi_topk goes with neither activation='batchtopk' nor matryoshka")
        if self.activation == "batchtopk" and not self.k <= self.cap:
            raise ValueError(f"cap must be at least k = {self.k}, got {self.cap}")
        if len(self.matryoshka_weights) != len(self.matryoshka):
            raise ValueError("matryoshka_weights holds one weight per prefix size")
        if any(a >= b for a, b in zip(self.matryoshka, self.matryoshka[1:])):
            raise ValueError(f"matryoshka prefix sizes must ascend strictly, got {self.matryoshka}")

    @property
    def width(self) -> int:
        """The width of the main selection's lists."""
        return self.cap if self.activation == "batchtopk" else self.k


@dataclass
class BatchResult:
    stepped: bool
    t: int                         # the bias-correction step of this batch's optimiser pass (stepping batches)
    lr: float                      # the learning rate of this batch's optimiser pass
    global_step: int
    G: Dict[str, torch.Tensor]
    dG: Dict[str, torch.Tensor]
    sumsq: float                   # what the clip's norm is the square root of
    dsumsq: float
    clip: float                    # c = min(1, max_norm / (sqrt(sumsq) + 1e-6))
    stats: Dict[str, float]        # fvu, auxk_loss, multi_topk_fvu averaged over the chunks
    dstats: Dict[str, float]
    dead_mask: torch.Tensor        # the mask this batch ran with
    num_dead: int
    scale: float
    tie_share: float               # worst selection of the batch
    sel_ratio: float               # largest |float32 value - float64 latent| / b_t over the adopted selections
    num_tokens_since_fired: torch.Tensor = field(default=None)    # after the batch
    theta: float = 0.0             # "batchtopk": the mean of the chunks' thresholds, and the bound of its float32 mean
    dtheta: float = 0.0
    threshold: float = -1.0        # "batchtopk": the folded threshold state after the batch
    dthreshold: float = 0.0
    n_saturated: int = 0           # "batchtopk": rows that kept all C slots, summed over the chunks
    lengths: torch.Tensor = field(default=None)                   # "batchtopk": the kept prefix of every row, chunks in order
    nested_fvu: Tuple[float, ...] = ()                            # matryoshka: the FVU of every prefix, averaged like stats
    dnested_fvu: Tuple[float, ...] = ()
    groups_min: Tuple[int, ...] = ()                              # matryoshka: per group the fewest live entries of a chunk
    empty_first: int = 0                                          # matryoshka: tokens whose first group holds no live entry


class TrainerRef:
    def __init__(self, cfg: TrainerConfig, params: Dict[str, torch.Tensor], mutate: Sequence[str] = (),
                 f32_hyper: bool = True):
        """params: W_enc [N, d], b_enc [N], W_dec [N, d], b_dec [d].  f32_hyper: evaluate Adam at the float32 values of
        lr, betas, eps and max_norm (what reaches a kernel as C floats, as train_ref does); False: at the Python doubles
        (what torch.optim.Adam in float64 does)."""
        assert set(mutate) <= set(MUTATIONS), mutate
        self.cfg, self.mut, self.f32_hyper = cfg, frozenset(mutate), f32_hyper
        self.p = {n: tr._d(params[n]).clone() for n in NAMES}
        self.N, self.d = self.p["W_enc"].shape
        self.m = {n: torch.zeros_like(v) for n, v in self.p.items()}
        self.v = {n: torch.zeros_like(v) for n, v in self.p.items()}
        self.t = 0
        self.global_step = 0
        self.num_tokens_since_fired = torch.zeros(self.N, dtype=torch.long)
        self.did_fire = torch.zeros(self.N, dtype=torch.bool)
        self.num_tokens_in_step = 0
        self.G: Optional[Dict[str, torch.Tensor]] = None      # the window's accumulated gradients and their raw bounds
        self.dG: Optional[Dict[str, torch.Tensor]] = None
        self.dWd = torch.zeros_like(self.p["W_dec"])           # |float32 W_dec - self.p["W_dec"]| (raw)
        self.threshold, self.dthreshold = -1.0, 0.0            # "batchtopk": the folded theta and its raw bound
        if cfg.matryoshka:
            assert cfg.matryoshka[-1] == self.N, (cfg.matryoshka, self.N)

    # ---- synchronisation with the side under test ---------------------------------------------------------------------------
    def load_state(self, params, exp_avg, exp_avg_sq) -> None:
        """Take the float32 parameters and moments (dicts by NAMES) as exact inputs of the next optimiser step."""
        assert self.G is None, "state is synchronised between optimiser steps, not inside a window"
        for n in NAMES:
            self.p[n], self.m[n], self.v[n] = tr._d(params[n]).clone(), tr._d(exp_avg[n]).clone(), tr._d(exp_avg_sq[n]).clone()
        self.dWd = torch.zeros_like(self.p["W_dec"])

    # ---- pieces ---------------------------------------------------------------------------------------------------------------
    def _h(self, x: float) -> float:
        return f32(x) if self.f32_hyper else float(x)

    @property
    def current_lr(self) -> float:
        step = self.t + 1 if "lr_of_next_step" in self.mut else self.t
        return self.cfg.lr * linear_schedule_with_warmup(step, self.cfg.lr_warmup_steps, self.cfg.total_steps)

    def dead_mask(self) -> torch.Tensor:
        if "dead_ge_threshold" in self.mut:
            return self.num_tokens_since_fired >= self.cfg.dead_feature_threshold
        return self.num_tokens_since_fired > self.cfg.dead_feature_threshold

    def _renorm(self) -> None:
        eps = float(torch.finfo(torch.float32).eps)
        self.p["W_dec"], self.dWd = tr._renorm(self.p["W_dec"], self.dWd, eps, self.d)

    @staticmethod
    def _tie_share(lat, bt, k: int, universe: Optional[torch.Tensor]) -> float:
        if universe is not None:
            lat = torch.where(universe[None], lat, torch.full_like(lat, -torch.inf))
            if int(universe.sum()) <= k:
                return 0.0
        elif lat.shape[1] <= k:
            return 0.0
        v, i = lat.topk(k + 1, dim=1)
        b = bt.gather(1, i[:, k - 1:k + 1]).amax(1)
        near = (v[:, k - 1] - v[:, k] < 2 * b) & (v[:, k - 1] > 0)
        return float(near.double().mean())

    def _adopt(self, pre, bt, idx, vals32, universe: Optional[torch.Tensor], what: str):
        """Check the float32 side's selection (vals32, idx) against the float64 pre-activations, return (mask, ratio)."""
        T, N = pre.shape
        idx = idx.to("cpu", torch.long)
        vals32 = tr._d(vals32)
        lat = torch.relu(pre)
        chosen = torch.zeros(T, N, dtype=torch.bool).scatter_(1, idx, True)
        assert int(chosen.sum()) == idx.numel(), f"{what}: a feature is selected twice"
        if universe is not None:
            assert bool(universe[idx].all()), f"{what}: a feature outside the dead set is selected"
        p_sel, b_sel = pre.gather(1, idx), bt.gather(1, idx)
        err = (vals32 - torch.relu(p_sel)).abs()
        assert bool((err <= b_sel).all()), f"{what}: a selected value is off by {float((err / b_sel.clamp_min(1e-300)).max()):.3f} b_t"
        rest = ~chosen if universe is None else (~chosen & universe[None])
        lo_sel = torch.where(chosen, lat + bt, torch.full_like(lat, torch.inf)).amin(1)
        hi_rest = torch.where(rest, lat - bt, torch.full_like(lat, -torch.inf)).amax(1)
        bad = lo_sel < hi_rest
        assert not bool(bad.any()), (f"{what}: not a top-{idx.shape[1]} of the float64 latents within 2 b_t on "
                                     f"{int(bad.sum())} tokens, first {int(bad.nonzero()[0])}")
        m64, m32, near = p_sel > 0, vals32 > 0, p_sel.abs() <= b_sel
        assert bool(((m64 == m32) | near).all()), f"{what}: the ReLU masks differ where |p| > b_t"
        pos = b_sel > 0
        return torch.where(near, m32, m64), float((err[pos] / b_sel[pos]).max()) if bool(pos.any()) else 0.0

    # ---- "batchtopk": the batch-level selection over the top-C lists ----------------------------------------------------------
    def _theta64(self, v, K: int) -> float:
        """The K-th largest positive entry of the lists v; the smallest positive one when there are fewer, +inf when none."""
        pos = v[v > 0]
        if pos.numel() == 0:
            return float("inf")
        if "theta_rank_plus_1" in self.mut:
            K = K + 1
        return float(pos.sort(descending=True).values[min(K, pos.numel()) - 1])

    def _keep64(self, v, theta: float):
        if "keep_strictly_above_theta" in self.mut:
            return (v > 0) & (v > theta)
        return (v > 0) & (v >= theta)

    def _batch_tie_share(self, lat, bt) -> float:
        """The share of the chunk's T k kept slots that float64 leaves undecided: positive list entries within 2 b_t of
        theta64, and rows saturated in float64 whose gap at rank C is below 2 b_t.  A tie at rank C of an unsaturated row
        forks nothing (its tail is dropped) and does not count."""
        T, N = lat.shape
        C, K = self.cfg.cap, T * self.cfg.k
        v, i = lat.topk(min(C + 1, N), dim=1)
        b = bt.gather(1, i)
        vC, bC = v[:, :C], b[:, :C]
        theta = self._theta64(vC, K)
        undecided = int(((vC > 0) & ((vC - theta).abs() < 2 * bC)).sum())
        if N > C:
            saturated = (vC[:, -1] > 0) & (vC[:, -1] >= theta)
            undecided += int((saturated & (v[:, C - 1] - v[:, C] < 2 * b[:, C - 1:C + 1].amax(1))).sum())
        return undecided / K

    def _select_batch64(self, lat):
        """Standalone mode -> (idx [T, C], keep [T, C], theta64, lengths, n_saturated) from the float64 top-C lists."""
        v, idx = lat.topk(self.cfg.cap, dim=1)
        theta = self._theta64(v, lat.shape[0] * self.cfg.k)
        keep = self._keep64(v, theta)
        sat = (v[:, -1] > 0) & (v[:, -1] >= theta)
        return idx, keep, theta, keep.sum(1).to(torch.int32), int(sat.sum())

    def _adopt_batch(self, pre, bt, vals32, idx, returned, what: str):
        """Adopting mode.  (vals32, idx): the top-C list ops.sparse_encode returned (already through _adopt); returned:
        (kept values, lengths, theta, n_saturated) of ops.batch_select for it.  (ii) those four equal, bit for bit,
        batch_select_ref.batch_select of the float32 list; (iii) the kept set is a valid batch-level selection of the float64
        latents: over the whole chunk min over kept (lat64 + b_t) >= max over dropped positive list entries (lat64 - b_t), and
        at least min(T k, positives) entries are kept.  -> (keep [T, C], theta as a float, lengths, n_saturated)."""
        import batch_select_ref as bs

        T, C = idx.shape
        kept32, lengths, theta32, n_sat = returned
        v_np = vals32.detach().cpu().float().numpy()
        assert bool((v_np[:, :-1] >= v_np[:, 1:]).all()), f"{what}: a top-C list is not in descending order"
        vo, io, ln, th, sat = bs.batch_select(v_np, idx.cpu().numpy(), self.cfg.k)
        kept32 = kept32.detach().cpu().float().reshape(T, C)
        lengths = lengths.detach().cpu().to(torch.int32).reshape(T)
        theta32 = float(theta32)
        assert theta32 == float(th), f"{what}: theta {theta32!r} is not the restated {float(th)!r}"
        assert torch.equal(lengths, torch.from_numpy(ln)), f"{what}: lengths differ from the restated filter"
        assert torch.equal(kept32, torch.from_numpy(vo)) and bool((io == idx.cpu().numpy()).all()), \
            f"{what}: kept values differ from the restated filter"
        assert int(n_sat) == int(sat.sum()), f"{what}: n_saturated {int(n_sat)} against {int(sat.sum())}"
        keep = torch.arange(C)[None, :] < lengths[:, None].long()
        lat_sel, b_sel = torch.relu(pre).gather(1, idx), bt.gather(1, idx)
        lo_kept = float(torch.where(keep, lat_sel + b_sel, torch.full_like(lat_sel, torch.inf)).min())
        dropped = ~keep & (lat_sel > 0)
        hi_drop = float(torch.where(dropped, lat_sel - b_sel, torch.full_like(lat_sel, -torch.inf)).max())
        assert lo_kept >= hi_drop, f"{what}: a dropped entry lies more than 2 b_t above a kept one in float64"
        positives = int((tr._d(vals32) > 0).sum())
        assert int(keep.sum()) >= min(T * self.cfg.k, positives), f"{what}: {int(keep.sum())} entries kept of {positives} positive"
        return keep, theta32, lengths, int(n_sat)

    # ---- forward and backward of one micro-chunk ----------------------------------------------------------------------------
    def _chunk(self, x, weight: float, dead: Optional[torch.Tensor], num_dead: int, sel, bsel=None):
        """-> (G, dG raw, stats, dstats raw, fired indices, tie share, selection ratio, k_aux, scale, extra) of `weight` *
        loss on chunk x.  extra: theta, lengths, n_saturated ("batchtopk"), nested_fvu with raw bounds and the live entries
        per group (matryoshka)."""
        cfg, d, N = self.cfg, self.d, self.N
        batch, nested = cfg.activation == "batchtopk", bool(cfg.matryoshka)
        extra = {}
        We, be, Wd, bd = (self.p[n] for n in NAMES)
        dWd = self.dWd
        T = x.shape[0]
        aWe, aWd = We.abs(), Wd.abs()
        a = x - bd
        da = U * a.abs()
        pre = a @ We.T + be
        bt = SAFETY * (d + 2) * U * (a.abs() @ aWe.T + be.abs())
        lat = torch.relu(pre)

        k_aux, scale = 0, 0.0
        if dead is not None and num_dead > 0:
            k_aux = d // 2
            scale = num_dead / k_aux if "scale_uncapped" in self.mut else min(num_dead / k_aux, 1.0)
            k_aux = min(k_aux, num_dead)
        widths = [(cfg.width, None)] + ([(k_aux, dead)] if k_aux else []) + ([(4 * cfg.k, None)] if cfg.multi_topk else [])
        picks, tie, ratio = [], 0.0, 0.0
        fire_main = listed_mask = None
        if sel is not None:
            assert len(sel) == len(widths), ("selections handed over", len(sel), "expected", len(widths))
            assert (bsel is not None) == batch, "what ops.batch_select returned goes with activation='batchtopk', and only with it"
        for j, (kk, universe) in enumerate(widths):
            main_batch = batch and j == 0
            tie = max(tie, self._batch_tie_share(lat, bt) if main_batch else self._tie_share(lat, bt, kk, universe))
            if sel is None:
                if main_batch:
                    idx, keep, theta, lengths, n_sat = self._select_batch64(lat)
                else:
                    src = lat if universe is None else torch.where(universe[None], lat, torch.full_like(lat, -torch.inf))
                    idx = src.topk(kk, dim=1, sorted=False).indices
                mask = pre.gather(1, idx) > 0
            else:
                vals32, idx = sel[j]
                assert tuple(idx.shape) == (T, kk), (tuple(idx.shape), (T, kk))
                idx = idx.to("cpu", torch.long)
                mask, r = self._adopt(pre, bt, idx, vals32, universe, f"selection {j} (k = {kk})")
                ratio = max(ratio, r)
                if main_batch:
                    keep, theta, lengths, n_sat = self._adopt_batch(pre, bt, vals32, idx, bsel, "batch selection")
            depth = kk + 1
            if main_batch:
                # the decode, every gradient and the statistics see the kept entries only; the decode's chain has one fma per
                # kept entry and the bias add behind it: len + 1 <= C + 1 (csrc/batch_select.hip:229-277)
                extra.update(theta=theta, lengths=lengths, n_saturated=n_sat)
                fire_main = idx[keep]
                listed_mask = mask
                mask = mask & keep
                depth = mask.sum(1, keepdim=True).to(F64) + 1
            v = pre.gather(1, idx) * mask
            dv = bt.gather(1, idx) / SAFETY * mask
            picks.append((idx, mask, v, dv, depth))

        # three sparse products, each as a dense [T, N] matmul (wide selections) or over the selected pairs (narrow ones)
        def dense(idx):
            return idx.shape[1] * 128 >= N

        def spread(idx, coef):
            return torch.zeros(T, N, dtype=F64).scatter_add_(1, idx, coef)

        def lin(idx, coef, M):                # [T, .]: sum_j coef[t, j] M[idx[t, j], :]
            return spread(idx, coef) @ M if dense(idx) else (coef[:, :, None] * M[idx]).sum(1)

        def dots(idx, g, M):                  # [T, kk]: <g[t, :], M[idx[t, j], :]>
            return (g @ M.T).gather(1, idx) if dense(idx) else (g[:, None, :] * M[idx]).sum(2)

        def pair_sum(idx, coef, rows):        # [N, .]: sum over the pairs (t, j) with idx[t, j] = n of coef[t, j] rows[t, :]
            if dense(idx):
                return spread(idx, coef).T @ rows
            return torch.zeros(N, rows.shape[1], dtype=F64).index_add_(
                0, idx.reshape(-1), (coef[:, :, None] * rows[:, None, :]).reshape(-1, rows.shape[1]))

        def decode_of(idx, v, dv, depth):     # sum_j v_j W_dec[idx_j] + b_dec, a chain of `depth` rounded operations
            av = v.abs()
            return (lin(idx, v, Wd) + bd,
                    lin(idx, dv, aWd) + lin(idx, av, dWd) + depth * U * (lin(idx, av, aWd) + bd.abs()))

        def decode(pick):
            idx, _, v, dv, depth = pick
            return decode_of(idx, v, dv, depth)

        mean = x.mean(0)
        tv = float(((x - mean) ** 2).sum())
        dtv = (T + d + 8) * U * float(((x.abs() + mean.abs()) ** 2).sum())
        rc = 6 * U + dtv / tv                                     # relative bound of a loss coefficient
        cf = weight * 2.0 / tv

        nterm = T * d

        def sq_stat(r, dr, coef):
            s = float((r * r).sum())
            val = coef * s / tv
            return val, abs(coef) * (float((2 * r.abs() * dr + dr * dr).sum()) + nterm * U * s) / tv + abs(val) * rc

        stats, dstats = {}, {}
        idx0, mask0, v0, dv0, _ = picks[0]
        if nested:
            # every prefix g decodes the live entries with idx < bounds[g]: group-major, one fma per live entry of the groups
            # 0 .. g and the bias add (csrc/nested_decode.hip:79, 167-173), e_g = r_g - x one subtract (:174)
            Gn = len(cfg.matryoshka)
            grp = torch.searchsorted(torch.tensor(cfg.matryoshka, dtype=torch.long), idx0,
                                     right="prefix_boundary_off_by_one" not in self.mut)
            E, dE, nf, dnf = [], [], [], []
            for g in range(Gn):
                mg = mask0 & ((grp >= Gn - 1 - g) if "suffix_as_prefix" in self.mut else (grp <= g))
                out_g, dout_g = decode_of(idx0, v0 * mg, dv0 * mg, mg.sum(1, keepdim=True).to(F64) + 1)
                e_g = out_g - x
                E.append(e_g)
                dE.append(dout_g + U * e_g.abs())
                val, dval = sq_stat(E[-1], dE[-1], 1.0)
                nf.append(val)
                dnf.append(dval)
            e, de = E[-1], dE[-1]
            stats["fvu"], dstats["fvu"] = nf[-1], dnf[-1]         # a statistic only: the descent is on sum_g w_g nested_fvu[g]
            live_g = [mask0 & (grp == h) for h in range(Gn)]
            extra.update(nested_fvu=nf, dnested_fvu=dnf, groups=[int(m.sum()) for m in live_g],
                         empty_first=int((live_g[0].sum(1) == 0).sum()))
        else:
            out0, dout0 = decode(picks[0])
            e = out0 - x
            de = dout0 + U * e.abs()
            stats["fvu"], dstats["fvu"] = sq_stat(e, de, 1.0)
        g_outs = [None] * len(picks)          # (g_out, dg_out) of each decode
        gf = cf * e
        dgf = abs(cf) * de + (rc + U) * gf.abs()
        j = 1
        stats["auxk_loss"], dstats["auxk_loss"] = 0.0, 0.0
        ga = dga = None
        if k_aux:
            out1, dout1 = decode(picks[1])
            e_t, de_t = e, de                 # AuxK's target: the residual of the (kept) reconstruction
            if batch and "auxk_target_ignores_kept_mask" in self.mut:
                o, do = decode_of(idx0, pre.gather(1, idx0) * listed_mask, bt.gather(1, idx0) / SAFETY * listed_mask, cfg.cap + 1)
                e_t = o - x
                de_t = do + U * e_t.abs()
            r = out1 - e_t
            dr = dout1 + de_t + U * r.abs()
            stats["auxk_loss"], dstats["auxk_loss"] = sq_stat(r, dr, scale)
            ca = cf * cfg.auxk_alpha * scale
            ga = ca * r
            dga = abs(ca) * dr + (rc + 3 * U) * ga.abs()
            g_outs[1] = (ga, dga)
            g0 = gf - ga
            g_outs[0] = (g0, dgf + dga + U * g0.abs())
            j = 2
        else:
            g_outs[0] = (gf, dgf)
        S = None
        if nested:
            # the combine (csrc/nested_decode.hip:247-255): S_h = grad_full + sum_{g >= h} c_g e_g, one fma per plane from the
            # last plane down, from grad_full = the AuxK term's gradient into the full reconstruction (or +0): a chain of at
            # most G + 1 rounded operations.  c_g = weight 2 w_g / tv: the loss coefficient's handful of float32 operations,
            # the float32 value of w_g and the product with it
            w = list(cfg.matryoshka_weights)
            if "descend_on_full_fvu" in self.mut:
                w = [0.0] * (Gn - 1) + [1.0]
            s = torch.zeros_like(e) if ga is None else -ga
            ds = torch.zeros_like(e) if ga is None else dga
            sabs = s.abs()
            S = [None] * Gn
            for g in range(Gn - 1, -1, -1):
                cg = cf if "nested_coef_without_weight" in self.mut else cf * w[g]
                term = cg * E[g]
                s = s + term
                ds = ds + abs(cg) * dE[g] + (rc + 2 * U) * term.abs()
                sabs = sabs + term.abs()
                S[g] = (s, ds + (Gn + 1) * U * sabs)
        stats["multi_topk_fvu"], dstats["multi_topk_fvu"] = 0.0, 0.0
        if cfg.multi_topk:
            out2, dout2 = decode(picks[j])
            e2 = out2 - x
            de2 = dout2 + U * e2.abs()
            stats["multi_topk_fvu"], dstats["multi_topk_fvu"] = sq_stat(e2, de2, 1.0)
            gm = cf / 8.0 * e2
            g_outs[j] = (gm, abs(cf) / 8.0 * de2 + (rc + 2 * U) * gm.abs())

        G, dG = {}, {}

        def add(n, g, dg):                    # autograd accumulating a contribution: one rounded add after the first
            if n in G:
                G[n] = G[n] + g
                dG[n] = dG[n] + dg + U * G[n].abs()
            else:
                G[n], dG[n] = g, dg

        def wgrad(idx, v, dv, rows, drows, Lrow):
            """sum over the pairs of v[t, j] rows[t, :] into row idx[t, j] of an [N, d] gradient, with its bound: the pair
            coefficient and the row known to within dv and drows, one fma chain of Lrow[n] pairs per gradient row."""
            av, ar = v.abs(), rows.abs()
            if dense(idx):
                return (pair_sum(idx, v, rows),
                        pair_sum(idx, dv, ar) + pair_sum(idx, av, drows) + (Lrow[:, None] + 1) * U * pair_sum(idx, av, ar))
            live, inv = torch.unique(idx.reshape(-1), return_inverse=True)       # the rows that have a pair at all

            def ps(coef, r):
                src = (coef[:, :, None] * r[:, None, :]).reshape(-1, d)
                return torch.zeros(live.numel(), d, dtype=F64).index_add_(0, inv, src)

            g = torch.zeros(N, d, dtype=F64).index_copy_(0, live, ps(v, rows))
            return g, torch.zeros(N, d, dtype=F64).index_copy_(
                0, live, ps(dv, ar) + ps(av, drows) + (Lrow[live][:, None] + 1) * U * ps(av, ar))

        depth_acts = -(-d // 64) + 7
        L = torch.zeros(N, dtype=F64)
        idx_all, gc_all, dgc_all = [], [], []
        for pj, ((idx, mask, v, dv, _), (g, dg)) in enumerate(zip(picks, g_outs)):
            ag = g.abs()
            if batch and pj == 0:
                # a dropped slot reaches the weight-gradient kernels as activation 0, and wgrad_count_kernel / wgrad_fill_kernel
                # leave a zero activation out of the row's segment (csrc/decode.hip:177, 235): the chain counts kept pairs
                Ls = torch.bincount(idx.reshape(-1), weights=mask.reshape(-1).to(F64), minlength=N).to(F64)
            else:
                Ls = torch.bincount(idx.reshape(-1), minlength=N).to(F64)
            if nested and pj == 0:
                # the grouped backward kernels (csrc/decode.hip:138, 276): feature n reads plane group(n), the chains are
                # those of the plain kernels.  A row of W_dec lies in ONE group: the per-group sums meet no rounded add
                gw, dgw = torch.zeros(N, d, dtype=F64), torch.zeros(N, d, dtype=F64)
                gc, dgc = torch.zeros(T, idx.shape[1], dtype=F64), torch.zeros(T, idx.shape[1], dtype=F64)
                for h, (sh, dsh) in enumerate(S):
                    mh = (grp == h).to(F64)
                    gw_h, dgw_h = wgrad(idx, v * mh, dv * mh, sh, dsh, Ls)
                    gw, dgw = gw + gw_h, dgw + dgw_h
                    ash = sh.abs()
                    gc = gc + dots(idx, sh, Wd) * mask * mh
                    dgc = dgc + (dots(idx, dsh, aWd) + dots(idx, ash, dWd) + depth_acts * U * dots(idx, ash, aWd)) * mask * mh
                add("W_dec", gw, dgw)
                s0, ds0 = S[0]
                add("b_dec", s0.sum(0), ds0.sum(0) + T * U * s0.abs().sum(0))
            else:
                add("W_dec", *wgrad(idx, v, dv, g, dg, Ls))
                add("b_dec", g.sum(0), dg.sum(0) + T * U * ag.sum(0))
                gc = dots(idx, g, Wd) * mask
                dgc = (dots(idx, dg, aWd) + dots(idx, ag, dWd) + depth_acts * U * dots(idx, ag, aWd)) * mask
            idx_all.append(idx); gc_all.append(gc); dgc_all.append(dgc)
            L += Ls
        idx_cat, gc, dgc = torch.cat(idx_all, 1), torch.cat(gc_all, 1), torch.cat(dgc_all, 1)
        agc = gc.abs()
        add("W_enc", *wgrad(idx_cat, gc, dgc, a, da, L))
        flat = idx_cat.reshape(-1)
        s = torch.zeros(N, dtype=F64).index_add_(0, flat, gc.reshape(-1))
        ds = (torch.zeros(N, dtype=F64).index_add_(0, flat, dgc.reshape(-1))
              + L * U * torch.zeros(N, dtype=F64).index_add_(0, flat, agc.reshape(-1)))
        add("b_enc", s, ds)
        # b_dec through the encoder: -(s^T W_enc) over the rows with s != 0, in msae_weighted_row_sum_f32's order
        _, wrs_bound = tr.weighted_row_sum(We, s, -1.0)
        add("b_dec", -(s @ We), (ds + U * s.abs()) @ aWe + wrs_bound / SAFETY)
        fire = picks[0][0] if ("did_fire_from_k" in self.mut or not cfg.multi_topk) else picks[-1][0]
        if batch and "fired_from_listed_slots" not in self.mut:
            fire = fire_main                  # a dropped slot still names a feature: only the kept entries have fired
        return G, dG, stats, dstats, fire, tie, ratio, k_aux, scale, extra

    # ---- one batch --------------------------------------------------------------------------------------------------------------
    def batch(self, x, selections=None, update: bool = True, batch_selects=None) -> BatchResult:
        """x: [T, d] float32 (or float64 holding float32 values).  selections: None, or per micro-chunk the list of
        (values, indices) pairs the float32 side selected; batch_selects ("batchtopk", with selections): per micro-chunk what
        ops.batch_select returned for the main list (kept values, lengths, theta, n_saturated).  update=False: a caller that
        hands the parameters and moments over before every optimiser step (load_state) skips the restatement's own Adam
        arithmetic; t, the schedule and the dead-feature bookkeeping advance all the same."""
        cfg = self.cfg
        x = tr._d(x)
        if cfg.normalize_decoder and "no_renorm" not in self.mut:
            self._renorm()
        dead = self.dead_mask() if cfg.auxk_alpha > 0 else None
        num_dead = int(dead.sum()) if dead is not None else 0
        acc_steps = cfg.grad_acc_steps * cfg.micro_acc_steps
        chunks = x.chunk(cfg.micro_acc_steps)
        if selections is not None:
            assert len(selections) == len(chunks), (len(selections), len(chunks))
        stats = {n: 0.0 for n in ("fvu", "auxk_loss", "multi_topk_fvu")}
        dstats = dict(stats)
        tie = ratio = scale = 0.0
        batch_mode, Gn = cfg.activation == "batchtopk", len(cfg.matryoshka)
        th_sum = dth_sum = 0.0
        n_sat, lengths = 0, []
        nf, dnf = [0.0] * Gn, [0.0] * Gn
        groups_min, empty_first = [x.shape[0] * cfg.width] * Gn, 0
        for ci, chunk in enumerate(chunks):
            weight = 1.0 / acc_steps
            if "chunk_weight_by_token_share" in self.mut:
                weight = chunk.shape[0] / x.shape[0] / cfg.grad_acc_steps
            G, dG, st, dst, fire, tie_c, ratio_c, _, scale, extra = self._chunk(
                chunk, weight, dead, num_dead, None if selections is None else selections[ci],
                None if batch_selects is None else batch_selects[ci])
            tie, ratio = max(tie, tie_c), max(ratio, ratio_c)
            if batch_mode:
                th = extra["theta"]
                th_sum += th
                dth_sum += U * abs(th_sum)                      # the float32 running sum of the chunks' thetas
                n_sat += extra["n_saturated"]
                lengths.append(extra["lengths"])
                if "threshold_folded_once_per_batch" not in self.mut:
                    self._fold(th)
            for g in range(Gn):
                nf[g] += extra["nested_fvu"][g]
                dnf[g] += extra["dnested_fvu"][g] + U * abs(nf[g])
                groups_min[g] = min(groups_min[g], extra["groups"][g])
            if Gn:
                empty_first += extra["empty_first"]
            for n in stats:
                stats[n] += st[n]
                dstats[n] += dst[n] + U * abs(stats[n])
            if self.G is None:
                self.G, self.dG = G, dG
            else:
                for n in NAMES:
                    self.G[n] = self.G[n] + G[n]
                    self.dG[n] = self.dG[n] + dG[n] + U * self.G[n].abs()
            self.did_fire[fire.reshape(-1)] = True
        for n in stats:
            stats[n] /= len(chunks)
            dstats[n] = SAFETY * (dstats[n] / len(chunks) + U * abs(stats[n]))
        for g in range(Gn):
            nf[g] /= len(chunks)
            dnf[g] = SAFETY * (dnf[g] / len(chunks) + U * abs(nf[g]))
        theta = th_sum / len(chunks) if batch_mode else 0.0
        if batch_mode and "threshold_folded_once_per_batch" in self.mut:
            self._fold(theta)
        if "tokens_in_step_reset_every_batch" in self.mut:
            self.num_tokens_in_step = 0
        self.num_tokens_in_step += x.shape[0]
        self.global_step += 1
        stepped = self.global_step % cfg.grad_acc_steps == 0

        # clip_grad_norm_(max_norm) on every batch (trainer.py:391)
        proj_first = stepped and cfg.normalize_decoder and "project_before_clip" in self.mut
        G_in, dG_in = dict(self.G), dict(self.dG)                  # what the optimiser pass of the port receives
        if proj_first:
            self._project()
        n_all = sum(g.numel() for g in self.G.values())
        S = float(sum((g * g).sum() for g in self.G.values()))
        dS = float(sum((2 * g.abs() * dg + dg * dg).sum() for g, dg in zip(self.G.values(), self.dG.values()))) + n_all * U * S
        mn = self._h(cfg.max_norm)
        c_raw = mn / (S ** 0.5 + 1e-6)
        c = min(1.0, c_raw)
        c_lo = min(1.0, mn / ((S + dS) ** 0.5 + 1e-6) * (1 - 8 * U))
        c_hi = min(1.0, mn / (max(S - dS, 0.0) ** 0.5 + 1e-6) * (1 + 8 * U))
        dc = max(c - c_lo, c_hi - c)
        skip_clip = not stepped and "no_clip_on_non_stepping" in self.mut
        if not skip_clip:
            for n in NAMES:
                g = c * self.G[n]
                self.dG[n] = c * self.dG[n] + self.G[n].abs() * dc + (U * g.abs() if c < 1.0 or dc > 0 else 0.0)
                self.G[n] = g
        res = BatchResult(stepped=stepped, t=0, lr=0.0, global_step=self.global_step, G={}, dG={}, sumsq=S,
                          dsumsq=SAFETY * dS, clip=c, stats=stats, dstats=dstats,
                          dead_mask=dead if dead is not None else torch.zeros(self.N, dtype=torch.bool), num_dead=num_dead,
                          scale=scale, tie_share=tie, sel_ratio=ratio)
        if batch_mode:
            res.theta, res.dtheta = theta, SAFETY * (dth_sum / len(chunks) + U * abs(theta))
            res.threshold, res.dthreshold = self.threshold, SAFETY * self.dthreshold
            res.n_saturated, res.lengths = n_sat, torch.cat(lengths)
        if Gn:
            res.nested_fvu, res.dnested_fvu = tuple(nf), tuple(dnf)
            res.groups_min, res.empty_first = tuple(groups_min), empty_first
        if stepped:
            res.G, res.dG = G_in, {n: SAFETY * g for n, g in dG_in.items()}
            if cfg.normalize_decoder and not proj_first and update:
                self._project()
            res.lr = self.current_lr
            self.t += 1
            res.t = self.t + 1 if "bias_correction_t_plus_1" in self.mut else self.t
            if update:
                self._adam(res.t, res.lr)
            self.G = self.dG = None
            self.num_tokens_since_fired += self.num_tokens_in_step
            self.num_tokens_since_fired[self.did_fire] = 0
            self.num_tokens_in_step = 0
            self.did_fire.zero_()
        else:
            res.G = dict(self.G)
            res.dG = {n: SAFETY * g for n, g in self.dG.items()}
        res.num_tokens_since_fired = self.num_tokens_since_fired.clone()
        return res

    def _fold(self, theta: float) -> None:
        """One chunk's theta into the threshold state: the first finite theta is copied (the state starts at -1), after that
        thr += threshold_lr * (theta - thr); a non-finite theta is skipped.  Bound: the subtract, the product with the float32
        value of the rate and the add are one rounding each, 4 u (|thr| + |theta|) on top of the state's own bound (which
        the update contracts by 1 - rate: carried uncontracted)."""
        if theta != theta or theta in (float("inf"), float("-inf")):
            return
        if self.threshold < 0 and "threshold_first_value_averaged" not in self.mut:
            self.threshold, self.dthreshold = theta, 0.0
            return
        thr = self.threshold + self.cfg.threshold_lr * (theta - self.threshold)
        self.dthreshold += 4 * U * (abs(thr) + abs(theta) + abs(self.threshold))
        self.threshold = thr

    def _project(self) -> None:
        """remove_gradient_parallel_to_decoder_directions (sae.py:257-271) on the window's W_dec gradient."""
        g, w = self.G["W_dec"], self.p["W_dec"]
        self.G["W_dec"] = g - (g * w).sum(1, keepdim=True) * w

    def _adam(self, step: int, lr: float) -> None:
        """torch.optim.Adam's step on the (clipped, projected) window gradients."""
        b1, b2, eps, lr = self._h(self.cfg.betas[0]), self._h(self.cfg.betas[1]), self._h(self.cfg.eps), self._h(lr)
        bc1, bc2 = 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5
        for n in NAMES:
            g = self.G[n]
            self.m[n] = self.m[n] + (g - self.m[n]) * (1.0 - b1)
            self.v[n] = b2 * self.v[n] + (1.0 - b2) * g * g
            self.p[n] = self.p[n] - (lr / bc1) * self.m[n] / (self.v[n].sqrt() / bc2 + eps)
        self.dWd = torch.zeros_like(self.p["W_dec"])


# ---- the scenarios both test files use ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Scenario:
    name: str
    d: int
    N: int
    cfg: TrainerConfig
    tokens: Tuple[int, ...]            # tokens of every batch
    scales: Tuple[float, ...]          # input scale of every batch (chosen so that the clip is active in some, not in others)
    seed: int
    nnz: int = 8                       # nonzero coordinates per token
    weak: int = 0                      # features (the last ones) too short ever to fire
    start_dead: int = 0                # of those, how many start above the dead threshold
    start_old: int = 0                 # ordinary features that start ONE token into their count: one silent window kills them


def make_params(sc: Scenario) -> Dict[str, torch.Tensor]:
    """Float32 initial parameters from the scenario's seed.  Feature n reads coordinate n % d: N / d features per coordinate,
    alternating in sign, their lengths a jittered geometric ladder (0.25 * 0.9^j), plus dense noise of 0.002.  A token with
    few nonzero coordinates then has pre-activations that are ONE dominant product each, so b_t (which scales with
    sum |a| |w|) stays small against the gap at rank k, and the ladder keeps neighbouring latents several percent apart:
    that is what holds the share of near-ties under the cap.  The last `weak` features are 1000 times shorter: they never
    reach a top-k, which the dead-feature scenario needs.  The decoder is the encoder, unit rows when configured."""
    g = torch.Generator().manual_seed(sc.seed)
    N, d = sc.N, sc.d
    n = torch.arange(N)
    rung = (n // d) // 2
    sign = 1.0 - 2.0 * ((n // d) % 2).to(F64)
    length = 0.25 * 0.9 ** rung.to(F64) * (1.0 + 0.06 * (torch.rand(N, generator=g, dtype=F64) - 0.5))
    We = torch.randn(N, d, generator=g, dtype=F64) * 0.002
    We[n, n % d] += sign * length
    if sc.weak:
        We[N - sc.weak:] *= 1e-3
    Wd = We / We.norm(dim=1, keepdim=True) if sc.cfg.normalize_decoder else We
    be = torch.randn(N, generator=g) * 2e-4
    bd = torch.randn(d, generator=g) * 2e-4
    return {"W_enc": We.float().contiguous(), "b_enc": be.float(), "W_dec": Wd.float().contiguous(), "b_dec": bd.float()}


def make_batches(sc: Scenario) -> List[torch.Tensor]:
    """Float32 batches: tokens with `nnz` nonzero coordinates (standard normal), scaled per batch."""
    g = torch.Generator().manual_seed(sc.seed + 1)
    out = []
    for T, s in zip(sc.tokens, sc.scales):
        x = torch.zeros(T, sc.d, dtype=F64)
        pos = torch.rand(T, sc.d, generator=g).topk(sc.nnz, dim=1).indices
        x.scatter_(1, pos, torch.randn(T, sc.nnz, generator=g, dtype=F64))
        out.append((x * s).float())
    return out


def start_dead_features(sc: Scenario) -> torch.Tensor:
    """The features that start with num_tokens_since_fired above the threshold: drawn from the weak ones."""
    g = torch.Generator().manual_seed(sc.seed + 2)
    return sc.N - sc.weak + torch.randperm(sc.weak, generator=g)[:sc.start_dead]


def start_old_features(sc: Scenario) -> torch.Tensor:
    """Ordinary (not weak) features whose count starts at 1: with dead_feature_threshold = one window's tokens they cross it
    after the first optimiser step unless they fire before it -- while a feature that starts at 0 needs two silent windows."""
    g = torch.Generator().manual_seed(sc.seed + 3)
    return torch.randperm(sc.N - sc.weak, generator=g)[:sc.start_old]


def _sc(name, d, N, tokens, scales, seed, nnz, weak, start_dead=0, start_old=0, **cfg) -> Scenario:
    cfg.setdefault("k", 16)
    cfg.setdefault("lr", 2e-4)
    return Scenario(name, d, N, TrainerConfig(**cfg), tuple(tokens), tuple(scales), seed, nnz, weak, start_dead, start_old)


def scenario(name: str, normalize_decoder: bool = True, small: bool = False) -> Scenario:
    """The GPU scenarios (tests/test_gpu_train_trajectory.py) and, with small=True, their scaled-down forms (d = 32,
    N = 256) for the comparison with torch on the host.  The per-batch input scales put the clip on both sides of 1: the
    bias gradients grow as 1 / scale while the weight gradients do not depend on it."""
    d, N, T, k = (32, 256, 64, 4) if small else (256, 8192, 512, 16)
    weak, nnz = (24, 4) if small else (150, 6)
    if name == "plain":
        return _sc(name, d, N, [T] * 5, [1, 0.03, 1, 1, 0.03], 101, nnz, weak, k=k, lr_warmup_steps=2, total_steps=6,
                   normalize_decoder=normalize_decoder)
    if name == "accumulate":
        Ta = T + 3
        return _sc(name, d, N, [Ta] * 6, [0.004, 1, 1, 1, 0.004, 0.004], 202, nnz, weak, k=k, grad_acc_steps=2,
                   micro_acc_steps=2, lr_warmup_steps=1, total_steps=4)
    if name == "dead":
        return _sc(name, d, N, [T] * 5, [1, 1, 0.03, 1, 0.03], 303, nnz, weak, start_dead=5 if small else 50, k=k,
                   auxk_alpha=1.0 / 32, multi_topk=True, dead_feature_threshold=2 * T, lr_warmup_steps=2, total_steps=6)
    if name == "batch_sizes":
        assert not small
        return _sc(name, 1024, 8192, [512, 200, 512, 8, 300], [1, 0.03, 1, 1, 1], 404, 8, 40, k=k)
    # "batchtopk" and matryoshka.  The small forms keep the ratios: C = 4 k and C = 2 k, bounds off the multiples of 64
    bounds, wts = ((20, 65, N), (0.5, 0.0, 0.25)) if small else ((300, 2049, N), (0.5, 0.0, 0.25))
    if name == "batchtopk":
        return _sc(name, d, N, [T] * 5, [1, 0.03, 1, 1, 0.03], 101, nnz, weak, k=k, lr_warmup_steps=2, total_steps=6,
                   activation="batchtopk", cap=4 * k)
    if name == "batchtopk_saturated":
        Ta = T + 3
        return _sc(name, d, N, [Ta] * 4, [1, 0.03, 0.03, 1], 303, nnz, weak, start_dead=5 if small else 50,
                   start_old=12 if small else 240, k=k, activation="batchtopk", cap=2 * k, auxk_alpha=1.0 / 32,
                   dead_feature_threshold=2 * Ta, micro_acc_steps=2, grad_acc_steps=2, lr_warmup_steps=1, total_steps=4)
    if name == "matryoshka":
        return _sc(name, d, N, [T] * 5, [1, 0.03, 1, 1, 0.03], 101, nnz, weak, k=k, lr_warmup_steps=2, total_steps=6,
                   normalize_decoder=normalize_decoder, matryoshka=bounds, matryoshka_weights=wts)
    if name == "matryoshka_auxk":
        return _sc(name, d, N, [T] * 5, [1, 1, 0.03, 1, 0.03], 303, nnz, weak, start_dead=5 if small else 50, k=k,
                   auxk_alpha=1.0 / 32, dead_feature_threshold=8 * T, lr_warmup_steps=2, total_steps=6, matryoshka=bounds,
                   matryoshka_weights=wts)
    if name == "matryoshka_batchtopk":
        Ta = T + 3
        return _sc(name, d, N, [Ta] * 6, [1, 0.01, 1, 1, 0.01, 1], 202, nnz, weak, k=k, micro_acc_steps=2, grad_acc_steps=2,
                   lr_warmup_steps=1, total_steps=4, activation="batchtopk", cap=4 * k, matryoshka=bounds,
                   matryoshka_weights=wts)
    raise ValueError(name)


def initial_counts(sc: Scenario) -> torch.Tensor:
    """num_tokens_since_fired at the start: one batch above the threshold on the features that start dead (three batches'
    worth where the threshold is two), 1 on the old ones."""
    c = torch.zeros(sc.N, dtype=torch.long)
    if sc.start_dead:
        c[start_dead_features(sc)] = sc.cfg.dead_feature_threshold + sc.tokens[0]
    if sc.start_old:
        c[start_old_features(sc)] = 1
    return c


def run_standalone(sc: Scenario, mutate: Sequence[str] = (), f32_hyper: bool = True, sync_to=None):
    """The restatement on its own selections over the scenario's batches -> (TrainerRef, [BatchResult], [state before each
    batch]).  sync_to: the states of another run; the parameters and moments (never the bookkeeping) are taken from it at
    the start of every accumulation window, as the GPU test does with the float32 side's."""
    ref = TrainerRef(sc.cfg, make_params(sc), mutate, f32_hyper)
    ref.num_tokens_since_fired = initial_counts(sc)
    results, states = [], []
    for b, x in enumerate(make_batches(sc)):
        if sync_to is not None and b % sc.cfg.grad_acc_steps == 0:
            ref.load_state(*sync_to[b])
        states.append(tuple({n: t.clone() for n, t in s.items()} for s in (ref.p, ref.m, ref.v)))
        results.append(ref.batch(x))
    return ref, results, states
