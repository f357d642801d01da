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

Error model (u = 2^-24; to first order, ONE factor SAFETY at the end).  Every intermediate is a pair (value, bound):
  * an elementwise float32 operation adds u |result|; a scalar coefficient built from a handful of float32 scalar operations
    (2 / total_variance / acc_steps, alpha, scale, 1 / 8) carries 6 u plus the relative bound of the total variance;
  * a float32 sum adds depth * u * sum |terms| on top of the propagated input intervals.  `depth` where the order is ours:
        decode (sae_out, e_hat)        k + 1        the j-ordered fma chain and the bias add, csrc/decode.hip:33-79
        decoder backward, g_acts       d / 64 + 7   the lane's fma chain (d / 64 terms, own product), 6 shuffle levels,
                                                    csrc/decode.hip:131-143
        weight gradients (both)        L + 1        wgrad_accum_kernel's ascending pair order: one fma chain over the row's L
                                                    pairs, csrc/decode.hip:308-341 (L counts every selected pair of the call)
        b_dec through the encoder      train_ref.weighted_row_sum's depth (csrc/train.hip, msae_weighted_row_sum_f32)
    and depth = the number of terms where the order is not ours (valid for ANY order):
        encoder bias gradient          L            (row_act_sum, csrc/decode.hip:355-358, is shallower: ceil(L / 64) + 6)
        b_dec through a decode         T            grad_out.sum(0), a torch reduction
        total variance                 T + d + 8    torch.var over the tokens, the sum over d, the product with T
        squared-error sums             T d          torch.linalg.vector_norm
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
             "project_before_clip", "no_renorm")


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

    # ---- forward and backward of one micro-chunk ----------------------------------------------------------------------------
    def _chunk(self, x, weight: float, dead: Optional[torch.Tensor], num_dead: int, sel):
        """-> (G, dG raw, stats, dstats raw, fired indices, tie share, selection ratio) of `weight` * loss on chunk x."""
        cfg, d, N = self.cfg, self.d, self.N
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
        widths = [(cfg.k, None)] + ([(k_aux, dead)] if k_aux else []) + ([(4 * cfg.k, None)] if cfg.multi_topk else [])
        picks, tie, ratio = [], 0.0, 0.0
        if sel is not None:
            assert len(sel) == len(widths), ("selections handed over", len(sel), "expected", len(widths))
        for j, (kk, universe) in enumerate(widths):
            tie = max(tie, self._tie_share(lat, bt, kk, universe))
            if sel is None:
                src = lat if universe is None else torch.where(universe[None], lat, torch.full_like(lat, -torch.inf))
                idx = src.topk(kk, dim=1, sorted=False).indices
                mask = pre.gather(1, idx) > 0
            else:
                vals32, idx = sel[j]
                assert tuple(idx.shape) == (T, kk), (tuple(idx.shape), (T, kk))
                idx = idx.to("cpu", torch.long)
                mask, r = self._adopt(pre, bt, idx, vals32, universe, f"selection {j} (k = {kk})")
                ratio = max(ratio, r)
            v = pre.gather(1, idx) * mask
            dv = bt.gather(1, idx) / SAFETY * mask
            picks.append((idx, mask, v, dv, kk))

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

        def decode(pick):                     # sum_j v_j W_dec[idx_j] + b_dec
            idx, _, v, dv, kk = pick
            av = v.abs()
            return (lin(idx, v, Wd) + bd,
                    lin(idx, dv, aWd) + lin(idx, av, dWd) + (kk + 1) * U * (lin(idx, av, aWd) + bd.abs()))

        mean = x.mean(0)
        tv = float(((x - mean) ** 2).sum())
        dtv = (T + d + 8) * U * float(((x.abs() + mean.abs()) ** 2).sum())
        rc = 6 * U + dtv / tv                                     # relative bound of a loss coefficient
        cf = weight * 2.0 / tv

        out0, dout0 = decode(picks[0])
        e = out0 - x
        de = dout0 + U * e.abs()
        nterm = T * d

        def sq_stat(r, dr, coef):
            s = float((r * r).sum())
            val = coef * s / tv
            return val, abs(coef) * (float((2 * r.abs() * dr + dr * dr).sum()) + nterm * U * s) / tv + abs(val) * rc

        stats, dstats = {}, {}
        stats["fvu"], dstats["fvu"] = sq_stat(e, de, 1.0)
        g_outs = [None] * len(picks)          # (g_out, dg_out) of each decode
        gf = cf * e
        dgf = abs(cf) * de + (rc + U) * gf.abs()
        j = 1
        stats["auxk_loss"], dstats["auxk_loss"] = 0.0, 0.0
        if k_aux:
            out1, dout1 = decode(picks[1])
            r = out1 - e
            dr = dout1 + de + U * r.abs()
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
        for (idx, mask, v, dv, kk), (g, dg) in zip(picks, g_outs):
            ag = g.abs()
            Ls = torch.bincount(idx.reshape(-1), minlength=N).to(F64)
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
        return G, dG, stats, dstats, fire, tie, ratio, k_aux, scale

    # ---- one batch --------------------------------------------------------------------------------------------------------------
    def batch(self, x, selections=None, update: bool = True) -> BatchResult:
        """x: [T, d] float32 (or float64 holding float32 values).  selections: None, or per micro-chunk the list of
        (values, indices) pairs the float32 side selected.  update=False: a caller that hands the parameters and moments
        over before every optimiser step (load_state) skips the restatement's own Adam arithmetic; t, the schedule and
        the dead-feature bookkeeping advance all the same."""
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
        for ci, chunk in enumerate(chunks):
            weight = 1.0 / acc_steps
            if "chunk_weight_by_token_share" in self.mut:
                weight = chunk.shape[0] / x.shape[0] / cfg.grad_acc_steps
            G, dG, st, dst, fire, tie_c, ratio_c, _, scale = self._chunk(
                chunk, weight, dead, num_dead, None if selections is None else selections[ci])
            tie, ratio = max(tie, tie_c), max(ratio, ratio_c)
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


def _sc(name, d, N, tokens, scales, seed, nnz, weak, start_dead=0, **cfg) -> Scenario:
    cfg.setdefault("k", 16)
    cfg.setdefault("lr", 2e-4)
    return Scenario(name, d, N, TrainerConfig(**cfg), tuple(tokens), tuple(scales), seed, nnz, weak, start_dead)


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
    raise ValueError(name)


def initial_counts(sc: Scenario) -> torch.Tensor:
    """num_tokens_since_fired at the start: three batches' worth on the features that start dead."""
    c = torch.zeros(sc.N, dtype=torch.long)
    if sc.start_dead:
        c[start_dead_features(sc)] = 3 * sc.tokens[0]
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
