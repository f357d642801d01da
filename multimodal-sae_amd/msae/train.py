"""SAE optimisation steps on streamed activations (BASELINE configs[3]).

Mirrors the inner loop of the reference trainer (train/sae/sae/trainer.py:316-414) for one hookpoint:
first-step `b_dec` = geometric median of the batch (`:325-332`, sae/utils.py:37-62), decoder
renormalisation, forward in `micro_acc_steps` chunks (FVU + AuxK + Multi-TopK, `Sae.forward`), backward
through the HIP kernels (sparse encoder backward, decoder gather/scatter backward), data-parallel
gradient averaging (what DDP does, `:338-345`), `clip_grad_norm_(1.0)` every step, and every
`grad_acc_steps` steps: removal of the decoder-parallel gradient component, Adam with the linear
warm-up / linear decay schedule (`get_linear_schedule_with_warmup`, `:155-157`), dead-latent
bookkeeping (`did_fire` MAX-reduced, `:387-388,404-408`).

MI355X-side design:
  * clip, parallel-component removal and Adam run as ONE pass per parameter (csrc/train.hip: ~38 GB of HBM
    traffic per step at C2 instead of ~67 GB of separate torch ops); the global gradient norm stays on the
    device, so a step never synchronises with the host (statistics are returned as device tensors);
  * passes that would re-read a matrix another kernel has just produced are folded into the producer
    (`fuse_next_step`, round 4): the squared gradient norm of the two weight gradients is accumulated per row by
    the weight-gradient kernel itself (row in registers; a fixed-order 512-KB sum replaces two 2-GiB reads), the
    NEXT step's decoder renormalisation and the next encode's int8 / bf16 operands of the encoder are produced
    by the Adam pass from the row it has just updated (same bits as the separate passes; ~11 GB less traffic per
    step).  Between steps `W_dec` therefore holds unit-norm rows (the reference renormalises at the top of the
    next step, trainer.py:352 -- the same values one kernel later; a checkpoint written between steps differs from
    the reference's by that normalisation, ~1e-5 relative);
  * `optim_bits=8` (the reference takes bitsandbytes' Adam8bit when it can import it, trainer.py:139-147): the Adam
    moments of every parameter the format takes are carried as blockwise 8-bit codes (ops.Adam8State) --
    2 bytes per element instead of 8, and 16 instead of 28 bytes moved per element by the Adam pass;
  * `optimizer="lion"` / `"signum"` (no reference counterpart): a sign-momentum update in the same fused pass --
    one moment instead of two (4 bytes of state per element, 20 instead of 28 bytes moved per element), a step of +-lr per
    element; same clip, projection, renorm and operand refresh.  The default stays Adam;
  * data parallel: each parameter's gradient all-reduce (RCCL, ReduceOp.AVG -- no division pass) is
    launched ASYNCHRONOUSLY from a post-accumulate-grad hook the moment autograd has finished that
    parameter, so the 2 GiB W_dec exchange over xGMI overlaps the encoder backward, and the W_enc
    exchange overlaps the gradient-norm pass of W_dec; the four parameters are their own buckets (two
    of 2 GiB, two tiny).  A ring all-reduce of 2 x 2 GiB moves ~7 GiB per GPU per step over the 7 xGMI
    links -- of the order of the 18 ms compute of a T = 8192 step, so `grad_acc_steps` / larger per-GPU
    batches are what make the 8-GPU step compute-bound, exactly as in the reference.
The LLM forward that produces `hiddens`, dataset plumbing, wandb and checkpointing are the reference
trainer's outer loop and out of scope.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Tuple

import torch
import torch.distributed as dist
from torch import Tensor

from . import ops
from .sae import Sae


@torch.no_grad()
def geometric_median(points: Tensor, max_iter: int = 100, tol: float = 1e-5) -> Tensor:
    """Weiszfeld iterations from the mean (sae/utils.py:37-62); initialises the decoder bias."""
    guess = points.mean(dim=0)
    for _ in range(max_iter):
        prev = guess
        weights = 1 / torch.norm(points - guess, dim=1)
        weights /= weights.sum()
        guess = (weights.unsqueeze(1) * points).sum(dim=0)
        if torch.norm(guess - prev) < tol:
            break
    return guess


def linear_schedule_with_warmup(step: int, warmup_steps: int, total_steps: Optional[int]) -> float:
    """LR multiplier of transformers.get_linear_schedule_with_warmup at scheduler step `step`."""
    if step < warmup_steps:
        return step / max(1, warmup_steps)
    if total_steps is None:
        return 1.0
    return max(0.0, (total_steps - step) / max(1, total_steps - warmup_steps))


OPTIMIZERS = ("adam", "lion", "signum")
# "lion": Chen et al. 2023 (arXiv:2302.06675); "signum" (Bernstein et al. 2018) is its beta1 == beta2 case
_DEFAULT_BETAS = {"adam": (0.9, 0.999), "lion": (0.9, 0.99), "signum": (0.9, 0.9)}


class SaeTrainStep:
    def __init__(self, sae: Sae, lr: Optional[float] = None, auxk_alpha: float = 0.0,
                 dead_feature_threshold: int = 10_000_000, group=None, grad_acc_steps: int = 1,
                 micro_acc_steps: int = 1, lr_warmup_steps: int = 0, total_steps: Optional[int] = None,
                 init_b_dec: bool = False, fuse_next_step: bool = True, optim_bits: int = 32, auxk_path: str = "dense",
                 threshold_lr: float = 0.01, optimizer: str = "adam", betas: Optional[Tuple[float, float]] = None,
                 l0_alpha: float = 0.0, l0_warmup_steps: int = 0):
        from .parallel import _unpinned

        group = _unpinned(group)          # (the default group is addressed as None: nothing here keeps it alive past its destroy)
        self.sae, self.auxk_alpha, self.group = sae, auxk_alpha, group
        self.dead_feature_threshold = dead_feature_threshold
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        self.optimizer = optimizer
        sign = optimizer != "adam"         # "lion" / "signum": one moment, a step of +-lr per element
        if sign and lr is None:
            raise ValueError(f"optimizer={optimizer!r} needs an explicit lr: the default 2e-4 / sqrt(N / 2^14) is the reference's "
                             "Adam value (trainer.py:131), and there is no sign-optimiser value to inherit from it")
        if sign and optim_bits == 8:
            raise ValueError(f"optim_bits=8 is the 8-bit Adam format; optimizer={optimizer!r} keeps a float32 momentum "
                             "(an 8-bit momentum for the sign optimisers is a follow-up, DESIGN.md section 8)")
        if betas is None:
            betas = _DEFAULT_BETAS[optimizer]
        betas = (float(betas[0]), float(betas[1]))
        if optimizer == "signum" and betas[0] != betas[1]:
            raise ValueError(f"optimizer='signum' is Lion with beta1 == beta2, got betas={betas}; use optimizer='lion'")
        if lr is None:  # trainer.py:131: 2e-4 scaled by 1/sqrt(N / 2^14)
            lr = 2e-4 / (sae.num_latents / (2 ** 14)) ** 0.5
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, 1e-8, 1.0
        self.grad_acc_steps, self.micro_acc_steps = grad_acc_steps, micro_acc_steps
        self.lr_warmup_steps, self.total_steps, self.init_b_dec = lr_warmup_steps, total_steps, init_b_dec
        self.params = [p for p in sae.parameters()]
        assert all(p.dtype == torch.float32 for p in self.params), "the SAE trains in fp32 (trainer.py:190)"
        if optim_bits not in (8, 32):
            raise ValueError(f"optim_bits is 32 or 8, not {optim_bits}")
        if optim_bits == 8 and not sae.W_dec.is_cuda:
            raise ValueError("optim_bits=8 needs the Sae on a HIP device: the 8-bit moments exist in the HIP kernels only")
        self.optim_bits = optim_bits
        if auxk_path not in ops.AUXK_PATHS:
            raise ValueError(f"auxk_path must be one of {ops.AUXK_PATHS}, got {auxk_path!r}")
        self.auxk_path = auxk_path        # how Sae.forward builds the AuxK selection ("subset": no dense [T, N] latents)
        # "batchtopk" (DESIGN.md section 7n): every micro-chunk's theta is folded into sae.threshold at this rate (a
        # hyper-parameter: the running average inference will encode with), on the device
        self.batch_topk = sae.cfg.activation == "batchtopk"
        self.threshold_lr = threshold_lr
        # "jump" (DESIGN.md section 7s): the loss adds l0_alpha * warm(t) * out.l0, warm linear from 0 to 1 over l0_warmup_steps
        # optimiser steps; log_threshold is one more 1-D entry of self.params (clip, row passes and DDP hooks as the biases)
        self.jump = sae.cfg.activation == "jump"
        if not (float(l0_alpha) >= 0.0 and float(l0_alpha) != float("inf")) or int(l0_warmup_steps) < 0:
            raise ValueError(f"l0_alpha must be finite and not negative and l0_warmup_steps not negative, got {l0_alpha}, "
                             f"{l0_warmup_steps}")
        self.l0_alpha, self.l0_warmup_steps = float(l0_alpha), int(l0_warmup_steps)
        # a transcoder: step(hiddens, targets); the decoder starts at zero and is never normalised or
        # projected, whatever cfg.normalize_decoder says; W_skip is one more 2-D entry of self.params
        self.transcode = sae.cfg.transcode
        self.normalize_decoder = sae.cfg.normalize_decoder and not self.transcode
        # per parameter: an ops.Adam8State where the 8-bit format takes the shape, else None and float32 moments
        self.state8 = [ops.adam8_state(p) if optim_bits == 8 else None for p in self.params]
        self.exp_avg = [torch.zeros_like(p) if s8 is None else None for p, s8 in zip(self.params, self.state8)]   # torch.optim.Adam state
        self.exp_avg_sq = [torch.zeros_like(p) if s8 is None and not sign else None for p, s8 in zip(self.params, self.state8)]
        self.t = 0                     # optimizer steps taken (= lr scheduler steps)
        self.global_step = 0           # batches seen (trainer.py:394)
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=sae.device)
        self.num_tokens_since_fired = torch.zeros(sae.num_latents, dtype=torch.long, device=sae.device)
        self._did_fire = torch.zeros(sae.num_latents, dtype=torch.bool, device=sae.device)
        self._tokens_in_step = torch.zeros((), dtype=torch.long, device=sae.device)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self._pending, self._reduce_now = [], False
        # round 4: gradient norm from the weight-gradient kernels, next step's renorm + encoder operands from the Adam pass
        self.fuse_next_step = fuse_next_step
        self._normed_version = None        # W_dec._version whose rows the Adam pass left unit-norm
        self._wgrad_sumsq: dict = {}
        self._chunk_tokens = 0
        self._avg_op = None
        if self.world > 1:
            # AVG exists on nccl (RCCL) only; gloo (CPU tests) sums and divides
            self._avg_op = dist.ReduceOp.AVG if dist.get_backend(group) == "nccl" else None
            for p in self.params:
                p.register_post_accumulate_grad_hook(self._grad_ready)

    @property
    def current_lr(self) -> float:
        return self.lr * linear_schedule_with_warmup(self.t, self.lr_warmup_steps, self.total_steps)

    @property
    def current_l0_weight(self) -> float:
        """l0_alpha * warm(t): the weight of the L0 term in the batches of the optimiser step that comes next."""
        warm = min(1.0, self.t / self.l0_warmup_steps) if self.l0_warmup_steps > 0 else 1.0
        return self.l0_alpha * warm

    @property
    def optimizer_state_bytes(self) -> int:
        """Bytes of optimiser moments held (float32 tensors and 8-bit states together)."""
        f32 = sum(t.numel() * t.element_size() for t in self.exp_avg + self.exp_avg_sq if t is not None)
        return f32 + sum(s8.nbytes for s8 in self.state8 if s8 is not None)

    def state_dict(self) -> dict:
        sd = {"step": self.t, "global_step": self.global_step, "exp_avg": self.exp_avg,
              "exp_avg_sq": self.exp_avg_sq, "num_tokens_since_fired": self.num_tokens_since_fired}
        if self.optim_bits == 8:        # (a float32 state dict is what it always was)
            sd["optim_bits"] = 8
            sd["adam8"] = [None if s8 is None else {"m8": s8.m8, "r8": s8.r8, "sm": s8.sm, "sr": s8.sr} for s8 in self.state8]
        if self.optimizer != "adam":    # (an Adam state dict carries no optimiser key: it is what it always was)
            sd["optimizer"], sd["betas"] = self.optimizer, self.betas
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Takes a checkpoint of either precision: float32 moments are quantised into an 8-bit state, an 8-bit state is
        dequantised into float32 moments, per parameter.  A checkpoint of another optimiser is refused: the moments of
        Adam and of a sign optimiser do not mean the same thing."""
        theirs = sd.get("optimizer", "adam")
        if theirs != self.optimizer:
            raise ValueError(f"the checkpoint holds the state of optimizer={theirs!r}, this object runs "
                             f"optimizer={self.optimizer!r}: nothing is converted between them")
        self.t = int(sd["step"])
        self.global_step = int(sd.get("global_step", self.t * self.grad_acc_steps))
        saved8 = sd.get("adam8") or [None] * len(self.params)
        for i, (m, v) in enumerate(zip(sd["exp_avg"], sd["exp_avg_sq"])):
            src8 = None if saved8[i] is None else ops.Adam8State(**saved8[i])
            if self.state8[i] is None:
                if src8 is not None:
                    m, v = ops.adam8_dequantize(ops.Adam8State(*(t.to(self.params[i].device) for t in src8.tensors())))
                self.exp_avg[i].copy_(m)
                if self.exp_avg_sq[i] is not None:
                    self.exp_avg_sq[i].copy_(v)
            else:
                if src8 is None:
                    dev = self.params[i].device
                    src8 = ops.adam8_quantize(m.to(dev, torch.float32).contiguous(), v.to(dev, torch.float32).contiguous())
                for dst, src in zip(self.state8[i].tensors(), src8.tensors()):
                    dst.copy_(src)
        self.num_tokens_since_fired.copy_(sd["num_tokens_since_fired"])

    # ---- data-parallel plumbing -------------------------------------------------------------------------
    def _grad_ready(self, p: Tensor) -> None:
        """post-accumulate-grad hook: this parameter's gradient is final for this backward -> start its
        all-reduce now (asynchronously) if this is the step's last micro-batch."""
        if self._reduce_now:
            op = self._avg_op if self._avg_op is not None else dist.ReduceOp.SUM
            self._pending.append((dist.all_reduce(p.grad, op=op, group=self.group, async_op=True), p))

    def _join_reductions(self) -> None:
        for work, p in self._pending:
            work.wait()
            if self._avg_op is None:
                p.grad.div_(self.world)
        self._pending = []

    def _all_reduce(self, t: Tensor, op=None) -> Tensor:
        if self.world > 1:
            dist.all_reduce(t, op=op or dist.ReduceOp.SUM, group=self.group)
        return t

    # ---- BatchTopK bookkeeping (device work only: nothing is read back) -----------------------------------------
    @torch.no_grad()
    def _fold_threshold(self, theta: Tensor) -> Tensor:
        """This chunk's theta, averaged over the ranks (each takes it from its local batch, as data-parallel BatchTopK does),
        into sae.threshold: the first value is copied, after that thr += lr * (theta - thr); a non-finite theta (an empty
        or overflowed batch) is skipped.  Returns the averaged theta."""
        th = theta.detach().to(torch.float32).clone()
        if self.world > 1:
            self._all_reduce(th).div_(self.world)
        thr = self.sae.threshold
        moved = torch.where(thr < 0, th, thr + self.threshold_lr * (th - thr))
        thr.copy_(torch.where(torch.isfinite(th), moved, thr))
        return th

    @torch.no_grad()
    def _note_fired(self, out) -> None:
        """did_fire of one chunk.  TopK: every listed feature, as the reference.  BatchTopK: a dropped slot still names a
        feature, so only the kept prefix of every row counts -- an integer index_add_ of the keep mask (repeated indices add
        up in integers: deterministic, and no host read)."""
        idx = out.latent_indices
        lengths = getattr(out, "lengths", None)
        if lengths is None:
            self._did_fire.index_fill_(0, idx.flatten().long(), True)    # (an indexed assignment copies its scalar to the device)
            return
        C = idx.shape[-1]
        keep = torch.arange(C, device=idx.device) < lengths.reshape(-1, 1)
        hits = torch.zeros(self._did_fire.shape[0], dtype=torch.int32, device=idx.device)
        hits.index_add_(0, idx.reshape(-1).long(), keep.reshape(-1).to(torch.int32))
        self._did_fire |= hits > 0

    # ---- compute (overridden with torch-CPU restatements by the gloo tests) ----------------------------------
    def _forward(self, hiddens: Tensor, dead_mask: Optional[Tensor], targets: Optional[Tensor] = None):
        if targets is not None:
            return self.sae(hiddens, dead_mask, y=targets, auxk_path=self.auxk_path)
        return self.sae(hiddens, dead_mask, auxk_path=self.auxk_path)

    def _renorm_decoder(self) -> None:
        W = self.sae.W_dec
        if self._normed_version is not None and W._version == self._normed_version:
            return                          # the previous step's Adam pass has already normalised these rows
        self.sae.set_decoder_norm_to_unit_norm()

    def _clip_in_place(self) -> None:
        """clip_grad_norm_(1.0) on accumulated gradients that are NOT consumed by an optimizer step now."""
        torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)

    def _update(self, lr: float) -> None:
        """clip_grad_norm_(1.0) -> remove_gradient_parallel_to_decoder_directions -> Adam (or the sign update), fused."""
        sae = self.sae
        self._sumsq.zero_()
        # the squared norm of a weight gradient that came out of exactly ONE weight-gradient kernel call and was not
        # touched since (no accumulation, no all-reduce) is what that kernel recorded per row
        single = self.world == 1 and self.grad_acc_steps * self.micro_acc_steps == 1
        for p in self.params:
            if p.grad is None:
                continue
            ent = self._wgrad_sumsq.get(p.data_ptr()) if single else None
            if ent is not None and ent[0] == 1 and ent[1] == p.grad.data_ptr():
                ops.sum_into_(self._sumsq, ent[2])
            else:
                ops.grad_sumsq_(self._sumsq, p.grad)
        self._wgrad_sumsq = {}
        fuse = self.fuse_next_step and sae.W_dec.is_cuda
        for p, m, v, s8 in zip(self.params, self.exp_avg, self.exp_avg_sq, self.state8):
            if p.grad is None:
                continue
            kw = {}
            is_dec = p is sae.W_dec
            is_enc = p is sae.encoder.weight
            if fuse and is_dec and self.normalize_decoder:
                kw["renorm_eps"] = torch.finfo(p.dtype).eps          # sae.py:252
            if fuse and is_enc and self._chunk_tokens > 0 and ops.coarse_in_force() != "fp8":   # (the fused pass builds int8 / bf16 operands; MSAE_COARSE=fp8 in the environment counts: ADVICE r5)
                kw["refresh"], kw["tokens_next"] = ops.train_operand_buffer(p), self._chunk_tokens
            kw.update(total_sumsq=self._sumsq, max_norm=self.max_grad_norm, betas=self.betas,
                      project=self.normalize_decoder and is_dec)
            if self.optimizer != "adam":
                ops.lion_rows_(p.data, p.grad, m, lr, **kw)
            elif s8 is None:
                ops.adam_rows_(p.data, p.grad, m, v, self.t, lr, eps=self.eps, **kw)
            else:
                ops.adam8_rows_(p.data, p.grad, s8, self.t, lr, eps=self.eps, **kw)
            p.grad = None
            torch.autograd.graph.increment_version(p)    # p changed behind autograd's back: caches keyed on it go stale
            if "renorm_eps" in kw:
                self._normed_version = p._version
            if "refresh" in kw:
                ops.mark_train_operands_fresh(p, self._chunk_tokens)

    # ---- one batch ---------------------------------------------------------------------------------------------
    def step(self, hiddens: Tensor, targets: Optional[Tensor] = None) -> dict:
        """One global step (one batch of activations of this rank).  Returns device tensors (no host
        synchronisation): {"fvu", "auxk_loss", "multi_topk_fvu"} averaged over micro-batches and ranks,
        "stepped": whether the optimizer moved (every `grad_acc_steps`-th call).  A Matryoshka Sae (cfg.matryoshka) descends on
        the forward's `nested_loss` in place of its fvu and adds "nested_fvu" ([G], averaged like the others).  A
        "batchtopk" Sae adds "theta" (the mean of
        the micro-chunks' rank-averaged thresholds) and "n_saturated" (this rank's rows that kept all C slots), device tensors
        as well.  A "jump" Sae adds "l0" (the mean number of latents kept per token, averaged like the others) and
        "n_saturated", device tensors too, and descends on fvu + ... + l0_alpha * warm(t) * l0.

        `targets` (a transcoder, SaeConfig.transcode: required; a ValueError otherwise): what the dictionary predicts from
        `hiddens`, [T, d_out] over the same tokens; cut into micro-chunks with the same cuts.  `init_b_dec` then takes its
        geometric median from the targets: b_dec is an output bias."""
        sae = self.sae
        if self.transcode:
            if targets is None:
                raise ValueError("SaeTrainStep.step: a transcoder (SaeConfig.transcode) needs its targets: step(hiddens, targets)")
            if targets.dim() != 2 or targets.shape[0] != hiddens.shape[0] or targets.shape[1] != sae.d_out:
                raise ValueError(f"SaeTrainStep.step: targets must be [{hiddens.shape[0]}, {sae.d_out}], got "
                                 f"{tuple(targets.shape)}")
        elif targets is not None:
            raise ValueError("SaeTrainStep.step: targets= belongs to a transcoder (SaeConfig.transcode); an auto-encoder's "
                             "target is its input")
        if self.global_step == 0 and self.init_b_dec:            # trainer.py:325-332
            pts = (targets if self.transcode else hiddens).float()
            if self.world > 1:
                parts = [torch.empty_like(pts) for _ in range(self.world)]
                dist.all_gather(parts, pts, group=self.group)
                pts = torch.cat(parts)
            sae.b_dec.data.copy_(geometric_median(pts).to(sae.b_dec.dtype))
        if self.normalize_decoder:
            self._renorm_decoder()
        dead_mask = (self.num_tokens_since_fired > self.dead_feature_threshold) if self.auxk_alpha > 0 else None
        acc_steps = self.grad_acc_steps * self.micro_acc_steps
        stats = torch.zeros(3, dtype=torch.float32, device=hiddens.device)
        chunks = hiddens.chunk(self.micro_acc_steps)
        tchunks = targets.chunk(self.micro_acc_steps) if self.transcode else None
        theta_sum = n_saturated = nested_sum = l0_sum = 0
        l0_weight = self.current_l0_weight if self.jump else 0.0
        for ci, chunk in enumerate(chunks):
            self._reduce_now = self.world > 1 and ci == len(chunks) - 1
            self._chunk_tokens = chunk.shape[0]
            out = self._forward(chunk, dead_mask, tchunks[ci]) if self.transcode else self._forward(chunk, dead_mask)
            # a Matryoshka Sae descends on the weighted sum of its prefixes' FVUs; fvu stays a statistic
            nested_loss = getattr(out, "nested_loss", None)
            main = out.fvu if nested_loss is None else nested_loss
            loss = main + self.auxk_alpha * out.auxk_loss + out.multi_topk_fvu / 8
            if self.jump:
                loss = loss + l0_weight * out.l0
            # (a single rank: W_skip's gradient of a later chunk is added into .grad by the GEMM's own epilogue; with more
            # ranks the post-accumulate hooks must fire, so autograd accumulates)
            in_place = ops.skip_grad_in_place() if self.world == 1 else contextlib.nullcontext()
            if hiddens.is_cuda:
                with ops.collect_wgrad_sumsq() as self._wgrad_sumsq, in_place:
                    loss.div(acc_steps).backward()
            else:
                with in_place:
                    loss.div(acc_steps).backward()
            stats += torch.stack([out.fvu.detach(), out.auxk_loss.detach(), out.multi_topk_fvu.detach()])
            if nested_loss is not None:
                nested_sum = nested_sum + out.nested_fvu.detach().to(torch.float32)
            self._note_fired(out)
            if self.batch_topk:
                theta_sum = theta_sum + self._fold_threshold(out.theta)
                n_saturated = n_saturated + out.n_saturated
            if self.jump:
                l0_sum = l0_sum + out.l0.detach()
                n_saturated = n_saturated + out.n_saturated
        self._reduce_now = False
        if self.world > 1:
            fired = self._did_fire.to(torch.int32)
            self._all_reduce(fired, dist.ReduceOp.MAX)             # max is boolean "any"
            self._did_fire = fired.bool()
            self._join_reductions()                               # DDP semantics: gradients averaged over the ranks
        n_tok = torch.full((), hiddens.shape[0], dtype=torch.long, device=hiddens.device)   # (a fill: no host-to-device copy)
        self._tokens_in_step += self._all_reduce(n_tok)
        self.global_step += 1
        stepped = self.global_step % self.grad_acc_steps == 0
        if stepped:
            lr = self.current_lr
            self.t += 1
            self._update(lr)
            self.num_tokens_since_fired += self._tokens_in_step
            self.num_tokens_since_fired[self._did_fire] = 0
            self._tokens_in_step.zero_()
            self._did_fire.zero_()
        else:
            self._clip_in_place()                                  # trainer.py:391: clipped every batch
        stats /= len(chunks)
        if self.world > 1:
            self._all_reduce(stats).div_(self.world)
        res = {"fvu": stats[0], "auxk_loss": stats[1], "multi_topk_fvu": stats[2], "stepped": stepped}
        if self.batch_topk:
            res.update(theta=theta_sum / len(chunks), n_saturated=n_saturated)
        if self.jump:
            l0_mean = l0_sum / len(chunks)
            if self.world > 1:
                self._all_reduce(l0_mean).div_(self.world)
            res.update(l0=l0_mean, n_saturated=n_saturated)
        if isinstance(nested_sum, Tensor):
            nested_sum = nested_sum / len(chunks)
            if self.world > 1:
                self._all_reduce(nested_sum).div_(self.world)
            res["nested_fvu"] = nested_sum
        return res
