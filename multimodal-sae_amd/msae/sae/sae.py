"""Drop-in `Sae` module backed by the gfx950 HIP kernels.

Same constructor, attributes, state-dict keys (`encoder.weight [N,d]`, `encoder.bias [N]`,
`W_dec [N,d]`, `b_dec [d]`), checkpoint layout (`<dir>/cfg.json` + `<dir>/sae.safetensors`) and
methods as the reference module (sae_auto_interp/sae/sae.py:44-271), so the hooks in
features/cache.py, features/steering.py, features/patching/utils.py and tools/*.py keep working
unchanged.  What differs is underneath:

* `pre_acts`      -> torch.ops.msae.pre_acts   (exact f32 MFMA GEMM, dense output for legacy callers)
* `select_topk`   -> torch.ops.msae.topk       (canonical order: value desc, index asc)
* `encode`        -> torch.ops.msae.encode_topk (fused: the dense [T, N] latents never reach HBM)
* `decode`        -> torch.ops.msae.decode     (coalesced gather-matmul over W_dec rows, autograd)
* `probe`         -> torch.ops.msae.pooled_acts + topk + probe_maps (tools/probe_activations.py:109-126 without the
                     dense latents: new)
* `pre_acts(x, features=[...])` -> torch.ops.msae.pre_acts_features (the listed columns of `pre_acts` without the dense
                     latents); `forward(..., auxk_path="subset")` builds the AuxK selection on it
* `neighbors`, `top_logits` -> torch.ops.msae.row_inv_norms + rows_topk (features/stats.py:12-47,76-120 as one fused
                     f32 GEMM + per-row top-k: DESIGN.md section 7c)
* `SaeConfig(activation="batchtopk")` -> ops.batch_select + ops.decode(lengths=): the T*k largest latents of the batch in
                     `forward`, a learned or given threshold in `encode(threshold=)` (new, opt-in: DESIGN.md section 7n)

* `SaeConfig(activation="jump")` -> ops.jump_select + ops.decode(lengths=reach): JumpReLU with a learned threshold per feature
                     (`log_threshold`), trained through straight-through estimators (new, opt-in: DESIGN.md section 7s)

* `SaeConfig(transcode=True[, skip_connection=True])` -> a transcoder: `forward(x, y=)` predicts ANOTHER tensor (a module's output
                     from its input), W_dec [N, d_out], b_dec [d_out] an output bias the encoder does not subtract, and a dense
                     skip term x W_skip^T through ops.skip_add (new, opt-in: DESIGN.md section 7u)

SAE math is f32 whatever dtype the LLM hands over, as in the reference (sae.py:140,174).
There is no CPU implementation: calling a compute method with CPU tensors raises.
"""
from __future__ import annotations

import json
import math
import os
import re
from fnmatch import fnmatch
from pathlib import Path
from typing import NamedTuple, Optional, Union

import torch
from torch import Tensor, nn

from .. import ops
from . import probe as _probe
from . import utils as _seam
from .config import SaeConfig
from .probe import ProbeOutput


class EncoderOutput(NamedTuple):
    top_acts: Tensor
    """Activations of the top-k latents."""
    top_indices: Tensor
    """Indices of the top-k features."""


class ForwardOutput(NamedTuple):
    sae_out: Tensor
    latent_acts: Tensor
    latent_indices: Tensor
    fvu: Tensor
    auxk_loss: Tensor
    multi_topk_fvu: Tensor


class BatchForwardOutput(ForwardOutput):
    """The ForwardOutput of a "batchtopk" Sae: the same six fields -- latent_acts / latent_indices are the [T, C] lists, the
    dropped slots with activation +0.0 -- and three attributes from the batch-level selection, all
    device tensors: `lengths` (int32 [T], the kept prefix of every row), `theta` (f32 scalar, this batch's threshold) and
    `n_saturated` (int32 scalar, the rows that kept all C slots)."""

    def __new__(cls, *fields, lengths: Tensor, theta: Tensor, n_saturated: Tensor):
        self = super().__new__(cls, *fields)
        self.lengths, self.theta, self.n_saturated = lengths, theta, n_saturated
        return self


class JumpForwardOutput(ForwardOutput):
    """The ForwardOutput of a "jump" Sae: the same six fields -- latent_acts / latent_indices are the [T, C] lists in the
    partitioned order (kept, near, rest), the dropped slots with activation +0.0 -- and four attributes from the JumpReLU
    selection, all device tensors: `lengths` (int32 [T], the kept entries of every row), `reach`
    (int32 [T], kept + near: what the decode reads), `l0` (f32 scalar, the mean number kept per token, differentiable
    with respect to log_threshold) and `n_saturated` (int32 scalar, the rows whose last list entry reaches the band of
    the lowest threshold)."""

    def __new__(cls, *fields, lengths: Tensor, reach: Tensor, l0: Tensor, n_saturated: Tensor):
        self = super().__new__(cls, *fields)
        self.lengths, self.reach, self.l0, self.n_saturated = lengths, reach, l0, n_saturated
        return self


class NestedForwardOutput(ForwardOutput):
    """The ForwardOutput of a Matryoshka Sae (SaeConfig.matryoshka): the same six fields -- fvu is the
    full dictionary's -- and, as attributes, `nested_fvu` ([G]: the FVU of every prefix), `nested_loss` (the weighted sum the
    trainer descends on) and `bounds` (the prefix sizes, a tuple).  For a "batchtopk" Sae it also carries `lengths`, `theta`
    and `n_saturated` as a BatchForwardOutput does; they are None otherwise."""

    def __new__(cls, *fields, nested_fvu: Tensor, nested_loss: Tensor, bounds: tuple, lengths: Optional[Tensor] = None,
                theta: Optional[Tensor] = None, n_saturated: Optional[Tensor] = None):
        self = super().__new__(cls, *fields)
        self.nested_fvu, self.nested_loss, self.bounds = nested_fvu, nested_loss, bounds
        self.lengths, self.theta, self.n_saturated = lengths, theta, n_saturated
        return self


class NestedErrorOutput(NamedTuple):
    """Per-token squared error of every dictionary prefix (Sae.nested_error; include/msae.h, "nested decode").  The tensor
    fields are f32; `fvu` is float64."""
    bounds: tuple
    """The prefix sizes: entry g of the G axis reconstructs from the listed features below bounds[g]."""
    err2: Tensor
    """|r_g - x|^2, [..., G]."""
    xnorm2: Tensor
    """|x|^2, [...]."""
    total_variance: Tensor
    """(x - x.mean(0)).pow(2).sum() over this call's tokens, a float64 scalar."""
    d_in: int

    @property
    def fvu(self) -> Tensor:
        """Fraction of variance unexplained of this call, [G]."""
        return self.err2.to(torch.float64).reshape(-1, self.err2.shape[-1]).sum(0) / self.total_variance


class ReconOutput(NamedTuple):
    """Per-token moments of the reconstruction at several sparsities (Sae.recon_error; include/msae.h, "reconstruction
    error against sparsity").  The tensor fields are the kernel's f32 outputs; the properties are float64."""
    ks: tuple
    """The checkpoints: entry c of the C axis reconstructs from the first ks[c] entries of the top-k list."""
    err2: Tensor
    """|r - x|^2, [..., C]."""
    dot: Tensor
    """x . r, [..., C]."""
    rnorm2: Tensor
    """|r|^2, [..., C]."""
    xnorm2: Tensor
    """|x|^2, [...]."""
    total_variance: Tensor
    """(x - x.mean(0)).pow(2).sum() over this call's tokens (sae.py:202), a float64 scalar."""
    d_in: int

    @property
    def mse(self) -> Tensor:
        """Mean squared error per element, [..., C]."""
        return self.err2.to(torch.float64) / self.d_in

    @property
    def cosine(self) -> Tensor:
        """x . r / (|x| |r|), [..., C] (nan where either norm is zero)."""
        return self.dot.to(torch.float64) / (self.xnorm2.to(torch.float64)[..., None] * self.rnorm2.to(torch.float64)).sqrt()

    @property
    def fvu(self) -> Tensor:
        """Fraction of variance unexplained of this call, [C]: e.pow(2).sum() / total_variance (sae.py:201-202, 228)."""
        err = self.err2.to(torch.float64).reshape(-1, self.err2.shape[-1]).sum(0)
        return err / self.total_variance


class RefitOutput(NamedTuple):
    """The least-squares refit of a batch on the support its encoder chose (Sae.refit; include/msae.h, "support refit").
    The tensor fields are the kernel's outputs; the properties are float64."""
    top_acts: Tensor
    """The refit coefficients, [..., s] f32: `sae.decode(out.top_acts, out.top_indices)` is the refit reconstruction.  0 for
    a slot outside the support (a zero activation, a dependent row)."""
    top_indices: Tensor
    """The first s columns of the encoder's indices, [..., s]."""
    gain: Tensor
    """What slot j takes off the optimal error when it joins the slots before it, [..., s]."""
    err_fit: Tensor
    """|x - refit reconstruction|^2, [...]."""
    err_enc: Tensor
    """|x - the encoder's reconstruction from the same s slots|^2, [...]."""
    xx: Tensor
    """|x - b_dec|^2, [...]: the error at kappa = 0."""
    n_dependent: Tensor
    """Live slots dropped as linearly dependent, [...] int32."""
    total_variance: Tensor
    """(x - x.mean(0)).pow(2).sum() over this call's tokens, a float64 scalar (as ReconOutput's)."""

    @property
    def fvu_fit(self) -> Tensor:
        """Fraction of variance unexplained at the optimal coefficients, a float64 scalar."""
        return self.err_fit.to(torch.float64).sum() / self.total_variance

    @property
    def fvu_enc(self) -> Tensor:
        """Fraction of variance unexplained at the encoder's coefficients, a float64 scalar."""
        return self.err_enc.to(torch.float64).sum() / self.total_variance

    @property
    def gap(self) -> Tensor:
        """The amortisation gap: (err_enc - err_fit) summed over the call / its total variance, a float64 scalar."""
        return (self.err_enc.to(torch.float64) - self.err_fit.to(torch.float64)).sum() / self.total_variance

    def optimal_curve(self, ks) -> Tensor:
        """The optimal squared error of the top-kappa support at each kappa in `ks` (integers in [0, s]), [..., len(ks)]
        float64: xx - gain[..., :kappa].sum(-1).  The lower envelope of `Sae.recon_error(x, ks).err2`."""
        s = self.gain.shape[-1]
        ks = [int(c) for c in ks]
        if not ks or any(c < 0 or c > s for c in ks):
            raise ValueError(f"RefitOutput.optimal_curve: ks must be one or more integers in [0, {s}], got {ks}")
        g = self.gain.to(torch.float64)
        pre = torch.cat([torch.zeros_like(g[..., :1]), g.cumsum(-1)], -1)
        return self.xx.to(torch.float64)[..., None] - torch.stack([pre[..., c] for c in ks], -1)   # (selects: nothing copied)


class _SqErr(torch.autograd.Function):
    """sum((pred - target)^2) -> (scalar, pred - target) with ONE elementwise kernel and one reduction forward and one
    elementwise kernel backward, where the reference's `e = pred - x; e.pow(2).sum()` (sae.py:201,227) costs three
    T x d sweeps forward and three backward.  `target` is a constant (the LLM's activations)."""

    @staticmethod
    def forward(ctx, pred, target):
        e = pred - target
        ctx.save_for_backward(e)
        ctx.mark_non_differentiable(e)
        return torch.linalg.vector_norm(e).square(), e

    @staticmethod
    def backward(ctx, g, _ge):
        e, = ctx.saved_tensors
        return e * (2.0 * g), None


def _total_variance(x: Tensor) -> Tensor:
    """(x - x.mean(0)).pow(2).sum() (sae.py:202) as one column-variance kernel + a d-element sum."""
    return torch.var(x, dim=0, correction=0).sum() * x.shape[0]


def _natural_key(s: str):
    return [int(p) if p.isdigit() else p for p in re.split(r"(\d+)", s)]


class Sae(nn.Module):
    _warned_detached = False     # the one-time notice of Sae.encode (see its docstring)
    auxk_path = "dense"          # how `forward` builds the AuxK selection when it is not told: "dense" or "subset"

    def __init__(self, d_in: int, cfg: SaeConfig, device: Union[str, torch.device] = "cpu",
                 dtype: Union[torch.dtype, None] = None, *, decoder: bool = True, d_out: Optional[int] = None):
        super().__init__()
        self.cfg = cfg
        self.d_in = d_in
        self.num_latents = cfg.num_latents or d_in * cfg.expansion_factor
        # a transcoder (cfg.transcode) predicts a tensor of its own width: W_dec is [N, d_out] and
        # b_dec [d_out] lives in the output space
        self.d_out = d_in if d_out is None else int(d_out)
        if not cfg.transcode and self.d_out != d_in:
            raise ValueError(f"d_out = {self.d_out} != d_in = {d_in} needs a transcoder (SaeConfig(transcode=True)): an "
                             "auto-encoder reconstructs its own input")
        if self.d_out < 1:
            raise ValueError(f"d_out must be positive, got {self.d_out}")

        self.encoder = nn.Linear(d_in, self.num_latents, device=device, dtype=dtype)
        self.encoder.bias.data.zero_()
        if cfg.transcode:
            # zeros: a clone of the encoder has the wrong width, and zero rows have no direction -- never normalised
            self.W_dec = nn.Parameter(torch.zeros(self.num_latents, self.d_out, dtype=self.encoder.weight.dtype,
                                                  device=device)) if decoder else None
        else:
            self.W_dec = nn.Parameter(self.encoder.weight.data.clone()) if decoder else None
            if decoder and self.cfg.normalize_decoder:
                self.set_decoder_norm_to_unit_norm()
        self.b_dec = nn.Parameter(torch.zeros(self.d_out, dtype=dtype, device=device))
        if cfg.skip_connection:
            self.W_skip = nn.Parameter(torch.zeros(self.d_out, d_in, dtype=torch.float32, device=device))
        if cfg.activation == "batchtopk":
            # the inference threshold BatchTopK learns in training (msae.train.SaeTrainStep folds every batch's theta into it);
            # -1 = not learned yet.  Saved and loaded with the model; a TopK Sae has no such key.
            self.register_buffer("threshold", torch.tensor(-1.0, dtype=torch.float32, device=device))
            self._threshold_checked = None     # the buffer's _version at which a host read last found it learned
        if cfg.activation == "jump":
            # theta = exp(log_threshold), a torch op: the kernels get one table of bits and never exponentiate
            self.log_threshold = nn.Parameter(torch.full((self.num_latents,), math.log(cfg.jump_init), dtype=torch.float32,
                                                         device=device))
        if cfg.matryoshka:
            # only here is d_in known, and with it the width of the dictionary the prefixes must end at
            if cfg.matryoshka[-1] != self.num_latents:
                raise ValueError(f"the last matryoshka prefix size must be the number of latents {self.num_latents}, got "
                                 f"{cfg.matryoshka[-1]}")
            # the loss weights live on the device from the start (not saved: cfg.json holds them)
            self.register_buffer("_nested_w", torch.tensor(cfg.nested_weights, dtype=torch.float32, device=device),
                                 persistent=False)
        self._prepared: Optional[Tensor] = None
        self._prepared_key = None

    # ---- checkpoint I/O (sae.py:69-162) -----------------------------------------------------------
    @staticmethod
    def load_many(name: str, local: bool = False, layers: Union[list, None] = None,
                  device: Union[str, torch.device] = "cpu", *, decoder: bool = True,
                  pattern: Union[str, None] = None) -> dict:
        pattern = pattern + "/*" if pattern is not None else None
        if local:
            repo_path = Path(name)
        else:
            from huggingface_hub import snapshot_download

            repo_path = Path(snapshot_download(name, allow_patterns=pattern))
        if layers is not None:
            return {layer: Sae.load_from_disk(repo_path / layer, device=device, decoder=decoder)
                    for layer in sorted(layers, key=_natural_key)}
        dirs = [f for f in repo_path.iterdir()
                if f.is_dir() and (pattern is None or fnmatch(f.name, pattern))]
        return {f.name: Sae.load_from_disk(f, device=device, decoder=decoder)
                for f in sorted(dirs, key=lambda f: _natural_key(f.name))}

    @staticmethod
    def load_from_hub(name: str, hookpoint: Union[str, None] = None,
                      device: Union[str, torch.device] = "cpu", *, decoder: bool = True) -> "Sae":
        from huggingface_hub import snapshot_download

        repo_path = Path(snapshot_download(
            name, allow_patterns=f"{hookpoint}/*" if hookpoint is not None else None))
        if hookpoint is not None:
            repo_path = repo_path / hookpoint
        elif not repo_path.joinpath("cfg.json").exists():
            raise FileNotFoundError("No config file found; try specifying a layer.")
        return Sae.load_from_disk(repo_path, device=device, decoder=decoder)

    @staticmethod
    def load_from_disk(path: Union[Path, str], device: Union[str, torch.device] = "cpu", *,
                       decoder: bool = True) -> "Sae":
        from safetensors.torch import load_model

        path = Path(path)
        with open(path / "cfg.json", "r") as f:
            cfg_dict = json.load(f)
        d_in = cfg_dict.pop("d_in")
        d_out = cfg_dict.pop("d_out", None)            # written for a transcoder only
        cfg = SaeConfig.from_dict(cfg_dict)
        sae = Sae(d_in, cfg, device=device, decoder=decoder, d_out=d_out)
        load_model(model=sae, filename=str(path / "sae.safetensors"), device=str(device),
                   strict=decoder)
        sae.invalidate_prepared()
        return sae

    def save_to_disk(self, path: Union[Path, str]):
        from safetensors.torch import save_model

        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        save_model(self, str(path / "sae.safetensors"))
        with open(path / "cfg.json", "w") as f:
            json.dump({**self.cfg.to_dict(), "d_in": self.d_in, **({"d_out": self.d_out} if self.cfg.transcode else {})}, f)

    @property
    def _b_pre(self) -> Optional[Tensor]:
        """What the encoder subtracts from its input: b_dec, or nothing for a transcoder (its b_dec is an output bias)."""
        return None if self.cfg.transcode else self.b_dec

    def _no_transcoder(self, what: str) -> None:
        """The paths that compare or combine a reconstruction with the encoder's own input are not built for a transcoder."""
        if self.cfg.transcode:
            raise NotImplementedError(f"{what} is not built for a transcoder (SaeConfig.transcode): it reconstructs the "
                                      "encoder's own input, and a transcoder predicts another tensor -- Sae.transcode(x) and "
                                      "msae.features.hooks.transcoder_hook are the transcoder's inference paths")

    @property
    def device(self):
        return self.encoder.weight.device

    @property
    def dtype(self):
        return self.encoder.weight.dtype

    # ---- hot path -----------------------------------------------------------------------------------
    def pre_acts(self, x: Tensor, features=None) -> Tensor:
        """relu((x - b_dec) W_enc^T + b_enc) as a dense [..., N] f32 tensor (sae.py:172-177).
        Kept for callers that edit or reduce the dense latents (steering.py:111-114,
        tools/probe_activations.py:116); the caching / encode paths use the fused op instead.

        `features` (a list or 1-d int tensor of M feature indices, any order, repeats allowed): only those columns,
        [..., M] f32 -- bit for bit `pre_acts(x)[..., features]`, sub-threshold values included, without building the
        [..., N] latents (activation histograms and dashboards of a filter list).  A host list with an index outside
        [0, N) raises ValueError; a tensor's entries are clamped.  Inference only: differentiate the dense `pre_acts`."""
        if features is None:
            return ops.pre_acts(x, self.encoder.weight, self.encoder.bias, self._b_pre)
        feats = self._feature_rows(features, "pre_acts")          # validates before any device work
        if torch.is_grad_enabled() and any(t.requires_grad for t in (x, self.encoder.weight, self.encoder.bias, self.b_dec)):
            raise NotImplementedError("Sae.pre_acts(x, features=...) has no autograd: call it under torch.no_grad(), or "
                                      "differentiate the dense pre_acts(x) and index its result")
        return ops.pre_acts_features(x, self.encoder.weight, self.encoder.bias, self._b_pre, feats)

    def select_topk(self, latents: Tensor) -> EncoderOutput:
        """Top-k latents (sae.py:179-181).  Order is canonical (value desc, index asc), a valid
        instance of the reference's `sorted=False`."""
        return EncoderOutput(*ops.topk(latents, self.cfg.k))

    def invalidate_prepared(self) -> None:
        """Drop the cached coarse-pass operands (bf16 / int8 copies of encoder.weight).  They are
        rebuilt when `encoder.weight`'s autograd version changes; an edit through `.data`, `copy_`
        into `.data` or a raw-pointer kernel does NOT bump the version -- call this after one.  (Stale
        operands cannot corrupt results silently in general: every re-scored pair checks the error
        model and sends the token to the exact path -- but that is the slow path.)"""
        self._prepared = None
        self._prepared_key = None
        if self.encoder.weight.is_cuda:
            ops.invalidate_train_operands(self.encoder.weight)     # the training loop's per-parameter buffer as well
            ops.invalidate_certified(self.encoder.weight)          # ... and the certified pass's two-plane operands

    def _prepared_weights(self) -> Optional[Tensor]:
        w = self.encoder.weight
        # (+ whether the fp8 pass is in force: its operands replace the int8 ones in the buffer; + the dither mode: the
        # operands of a large batch's subtractive dither are rounded against the seed of the PREPARE, so a buffer prepared
        # with the dither off cannot serve a dithering encode except through the exact path -- include/msae.h, `dither`)
        key = (w.data_ptr(), w._version, tuple(w.shape), w.device,
               ops.coarse_in_force() == "fp8", ops.dither_in_force())
        if self._prepared is None or self._prepared_key != key:
            self._prepared = ops.prepare_encoder(w)
            self._prepared_key = key
        return self._prepared

    def encode(self, x: Tensor, *, set_feature: int = -1, set_value: float = 0.0,
               zero_feature: int = -1, return_status: bool = False, resolve: bool = True,
               differentiable: Optional[bool] = None, exact: bool = False, certified: bool = False, edits=None,
               edit_group: Optional[Tensor] = None, threshold=None, cap: Optional[int] = None, return_lengths: bool = False):
        """Fused encode + TopK (sae.py:183-185).  `set_feature/set_value` and `zero_feature` apply
        the steering / attribution hooks' edits of the dense latents (steering.py:113-114,
        patching/utils.py:43-48) inside the kernel, before TopK.  `edits` (a msae.features.FeatureEdits) applies a SET of
        such edits -- the reference's indexing takes a list or tensor of features: the unedited encode over-fetches
        k + E entries per token and ops.edit_topk re-ranks each list with the edits applied; exact, bit-identical to the
        scalar arguments for E = 1.  It is mutually exclusive with the scalar arguments (ValueError).
        A msae.features.RowEdits holds one table per GROUP and `edit_group` names every token's group: an
        int32 / int64 device tensor of shape x.shape[:-1], or for a 3-d x of shape x.shape[:1] (per batch row, expanded on the
        device), or None: row b of a 3-d x with x.shape[0] == G uses group b.  A token whose id lies outside [0, G) (-1 by
        convention) or whose group is empty comes out as the plain encode's.  `edit_group` with anything but a RowEdits is a
        ValueError.

        The kernel verifies every token and recomputes the ones it cannot verify (degenerate
        activations: all-zero rows, fewer than k positive latents, tokens the error model of the
        candidate pass does not describe ...) exactly inside the call, on the device; nothing is read
        back, so the method is stream-ordered like every other op.  `status` (return_status=True):
        0 verified, 1 recomputed exactly.  `resolve` is accepted for compatibility and ignored.
        Guarantees (include/msae.h): the default int8 pass rounds its operands stochastically with per-call seeds, so a
        member of the true top-k is missed with probability <= k exp(-z^2 / 2) (7e-10 at z = 7, k = 32) for EVERY input;
        `certified=True` runs the two-plane pass with a deterministic error band (no probability left, ~3x the time on
        large batches); `exact=True` computes EVERY token by the exact path (msae_options::exact).  Both are inference switches.

        Autograd follows the reference (sae.py:183-185 builds a graph whenever autograd would): the call is one differentiable
        node (sparse backward through the selected latents) when gradients are enabled and `x` requires grad (the attribution
        hooks: the LLM's hidden states do), or the module is in TRAINING mode and a parameter requires grad (a loaded module is,
        as in the reference, until `.eval()` / `.requires_grad_(False)`), or `differentiable=True` is passed.  The detached fast
        path is what runs under `torch.no_grad()` (the cache and steering hooks) and in `eval()` mode.

        Threshold encode: with `threshold=` -- a float, a one-element tensor, or a per-feature table
        [N] such as `ActHist.threshold_at_rate(...)` -- the call is "top-`cap`, then drop what lies below its (feature's)
        threshold": an EncoderOutput of width `cap` (default cfg.k) whose rows hold the kept entries first, in list order, and
        +0.0 behind them (`return_lengths=True` adds the int32 row lengths as a last result).  A "batchtopk" Sae ALWAYS
        encodes this way: `threshold` defaults to its learned buffer (RuntimeError while that is still -1; checking costs
        one host read per change of the buffer, none with an explicit threshold or after `set_threshold`) and `cap` to
        cfg.cap.  No edits here (ValueError); autograd through a scalar threshold is the mask's, through a table
        NotImplementedError.  A "jump" Sae ALWAYS encodes this way with its own table
        exp(log_threshold) and cap = cfg.cap: under no_grad the same filter, with gradients ops.jump_select (the rows then come
        in its partitioned order and gradients reach log_threshold); a foreign table stays NotImplementedError there."""
        if threshold is not None or self.cfg.activation in ("batchtopk", "jump"):
            if edits is not None or edit_group is not None or set_feature >= 0 or zero_feature >= 0:
                raise ValueError("Sae.encode: a threshold encode takes no edits, set_feature or zero_feature (edit a per-token "
                                 "TopK encode instead)")
            return self._encode_threshold(x, threshold, cap, return_lengths, return_status, differentiable, exact, certified)
        if cap is not None or return_lengths:
            raise ValueError("Sae.encode: cap= and return_lengths= belong to a threshold encode (threshold=, or a 'batchtopk' Sae)")
        if edits is not None:
            if set_feature >= 0 or zero_feature >= 0:
                raise ValueError("Sae.encode: pass either edits= or the scalar set_feature / zero_feature arguments, not both")
            edits.check(self.num_latents, self.cfg.k, self.encoder.weight.device)
        rows = edits is not None and hasattr(edits, "offsets")        # a RowEdits: one table per token
        if edit_group is not None and not rows:
            raise ValueError("Sae.encode: edit_group names the groups of a msae.features.RowEdits; it does not go with a "
                             "FeatureEdits or with the scalar set_feature / zero_feature arguments")
        if rows:
            edit_group = self._token_groups(x, edits, edit_group)
        if differentiable is None:
            params = self.encoder.weight.requires_grad or self.encoder.bias.requires_grad or self.b_dec.requires_grad
            differentiable = x.requires_grad or (self.training and params and not (exact or certified or return_status))
        want_grad = torch.is_grad_enabled() and differentiable
        if want_grad and (exact or certified):
            raise RuntimeError("Sae.encode(exact=True / certified=True) is an inference switch: differentiate pre_acts -> "
                               "select_topk (the exact path with autograd) instead")
        if want_grad and return_status:
            raise RuntimeError("Sae.encode(return_status=True) returns non-differentiable outputs: call it under "
                               "torch.no_grad(), or without return_status where gradients must flow")
        if want_grad:
            # autograd must flow (attribution patching: patching/utils.py:33-58, attribution.py:165):
            # same kernel, as one autograd node with the sparse backward
            (acts, idx), = ops.sparse_encode(x, self.encoder.weight, self.encoder.bias, self._b_pre, self.cfg.k,
                                             prepared=self._prepared_weights(), set_feature=set_feature,
                                             set_value=set_value, zero_feature=zero_feature, edits=edits,
                                             edit_group=edit_group)
            return EncoderOutput(acts, idx)
        with torch.no_grad():      # (a custom op without an autograd formula would hang a raising node on the outputs)
            if rows:               # the same two steps with the table of every token's own group
                acts, idx, status = ops.encode_topk(x, self.encoder.weight, self.encoder.bias, self._b_pre,
                                                    self._prepared_weights(), self.cfg.k + edits.E_max, exact=exact,
                                                    certified=certified)
                if edits.value_dependent:  # scale / add / floor / cap: the edited features' exact latents, one pass
                    acts, idx = ops.edit_topk_rows(acts, idx, edit_group, edits, self.num_latents, self.cfg.k,
                                                   cur=self._edit_cur(x, edits.union), col=edits.col)
                else:
                    acts, idx = ops.edit_topk_rows(acts, idx, edit_group, edits, self.num_latents, self.cfg.k)
            elif edits is not None:  # over-fetch, then edit: `exact` / `certified` only change the first call
                acts, idx, status = ops.encode_topk(x, self.encoder.weight, self.encoder.bias, self._b_pre,
                                                    self._prepared_weights(), self.cfg.k + edits.E, exact=exact,
                                                    certified=certified)
                acts, idx = ops.edit_topk(acts, idx, edits.feat, edits.val, edits.kind, self.num_latents, self.cfg.k,
                                          cur=self._edit_cur(x, edits.feat) if edits.value_dependent else None)
            else:
                acts, idx, status = ops.encode_topk(x, self.encoder.weight, self.encoder.bias, self._b_pre,
                                                    self._prepared_weights(), self.cfg.k, set_feature,
                                                    float(set_value), zero_feature, exact=exact, certified=certified)
        out = EncoderOutput(acts, idx)
        return (out, status) if return_status else out

    # ---- threshold encode ------------------------------------------------------
    @torch.no_grad()
    def set_threshold(self, value) -> None:
        """Set the inference threshold of a "batchtopk" Sae from a host number (finite, >= 0): no device read.  On a "jump"
        Sae: a host number or a table [N] (finite, > 0 -- checked on the host for a number, and for a table that lives there;
        a device table is taken as it is, no read) is written into log_threshold as log(value): a trained BatchTopK scalar or
        an ActHist.threshold_at_rate table seeds the learned thresholds."""
        if self.cfg.activation == "jump":
            if isinstance(value, Tensor):
                if value.dim() != 1 or value.shape[0] != self.num_latents:
                    raise ValueError(f"Sae.set_threshold: a table must be [{self.num_latents}], got {tuple(value.shape)}")
                table = value.detach().to(torch.float32)
                if not table.is_cuda and not bool((torch.isfinite(table) & (table > 0)).all()):
                    raise ValueError("Sae.set_threshold: every threshold must be finite and positive")
                self.log_threshold.copy_(table.to(self.log_threshold.device).log())
                return
            value = float(value)
            if not (value > 0.0 and value != float("inf")):
                raise ValueError(f"Sae.set_threshold: the threshold must be finite and positive, got {value}")
            self.log_threshold.fill_(math.log(value))
            return
        if self.cfg.activation != "batchtopk":
            raise ValueError("Sae.set_threshold: only a 'batchtopk' Sae has a threshold buffer")
        value = float(value)
        if not (value >= 0.0 and value != float("inf")):
            raise ValueError(f"Sae.set_threshold: the threshold must be finite and not negative, got {value}")
        self.threshold.fill_(value)
        self._threshold_checked = self.threshold._version

    def _learned_threshold(self) -> Tensor:
        """The threshold buffer, once a host read (one per change of the buffer) has found it learned."""
        if self._threshold_checked != self.threshold._version:
            if float(self.threshold) < 0:
                raise RuntimeError("Sae.encode: this 'batchtopk' Sae has not learned its threshold yet (the buffer holds -1): "
                                   "train it (msae.train.SaeTrainStep), call set_threshold(), or pass threshold=")
            self._threshold_checked = self.threshold._version
        return self.threshold

    def _encode_threshold(self, x: Tensor, threshold, cap: Optional[int], return_lengths: bool, return_status: bool,
                          differentiable: Optional[bool], exact: bool, certified: bool):
        N = self.num_latents
        dev = self.encoder.weight.device
        if cap is None:
            cap = self.cfg.cap
        if not 1 <= int(cap) <= min(N, ops.LIST_FILTER_MAX_C):
            raise ValueError(f"Sae.encode: cap must be in [1, {min(N, ops.LIST_FILTER_MAX_C)}], got {cap}")
        cap = int(cap)
        table = None
        own = threshold is None and self.cfg.activation == "jump"      # the Sae's learned table: differentiable
        if own:
            table = self.log_threshold.exp()
            theta = None
        elif threshold is None:
            theta = self._learned_threshold()
        elif isinstance(threshold, Tensor):
            if threshold.numel() == 1:
                theta = threshold.detach().to(dev, torch.float32).reshape(())
            elif threshold.dim() == 1 and threshold.shape[0] == N:
                table = threshold.detach().to(dev, torch.float32).contiguous()
                theta = table.min()                      # the floor of the saturation count; stays on the device
            else:
                raise ValueError(f"Sae.encode: threshold must be a number, a one-element tensor or a table [{N}], got "
                                 f"{tuple(threshold.shape)}")
        else:
            theta = torch.full((), float(threshold), dtype=torch.float32, device=dev)
        if differentiable is None:
            params = self.encoder.weight.requires_grad or self.encoder.bias.requires_grad or self.b_dec.requires_grad
            differentiable = x.requires_grad or (self.training and params and not (exact or certified or return_status))
        want_grad = torch.is_grad_enabled() and differentiable
        if want_grad and table is not None and not own:
            raise NotImplementedError("Sae.encode: autograd through a per-feature threshold table is not built (the kept "
                                      "entries move inside their row): call it under torch.no_grad(), or use a scalar threshold")
        if want_grad and (exact or certified or return_status):
            raise RuntimeError("Sae.encode(exact / certified / return_status) are inference switches: call them under "
                               "torch.no_grad()")
        status = None
        if want_grad and own:
            if cap > ops.JUMP_MAX_C:
                raise ValueError(f"Sae.encode: a differentiable 'jump' encode takes cap <= {ops.JUMP_MAX_C}, got {cap}")
            (acts, idx), = ops.sparse_encode(x, self.encoder.weight, self.encoder.bias, self._b_pre, cap,
                                             prepared=self._prepared_weights())
            acts, idx, lengths, _, _, _ = ops.jump_select(acts, idx, table, self.cfg.jump_bandwidth)
        elif want_grad:
            (acts, idx), = ops.sparse_encode(x, self.encoder.weight, self.encoder.bias, self._b_pre, cap,
                                             prepared=self._prepared_weights())
            with torch.no_grad():
                kept, _, lengths, _ = ops.list_filter(acts, idx, theta)
            # a canonical row is value-descending: the kept entries are its prefix, the indices stay, the gradient is the mask's
            acts = torch.where(kept > 0, acts, torch.zeros((), dtype=acts.dtype, device=acts.device))
        else:
            with torch.no_grad():
                acts, idx, status = ops.encode_topk(x, self.encoder.weight, self.encoder.bias, self._b_pre,
                                                    self._prepared_weights(), cap, exact=exact, certified=certified)
                if own:
                    table = table.detach()
                    theta = table.min()
                acts, idx, lengths, _ = ops.list_filter(acts, idx, theta, table)
        out = (EncoderOutput(acts, idx),) + ((status,) if return_status else ()) + ((lengths,) if return_lengths else ())
        return out[0] if len(out) == 1 else out

    def _edit_cur(self, x: Tensor, feats: Tensor) -> Tensor:
        """The exact latents of the features a value-dependent edit reads: the listed columns of
        `pre_acts`, bit for bit, [..., len(feats)] f32."""
        return ops.pre_acts_features(x, self.encoder.weight, self.encoder.bias, self._b_pre, feats)

    @staticmethod
    def _token_groups(x: Tensor, edits, edit_group: Optional[Tensor]) -> Tensor:
        """`edit_group` of encode -> one group id per token, shape x.shape[:-1] (device work only: nothing is read back)."""
        lead = tuple(x.shape[:-1])
        if edit_group is None:
            if x.dim() != 3 or x.shape[0] != edits.G:
                raise ValueError(f"Sae.encode: edit_group=None means row b uses group b: x must be [G, S, d] with G = "
                                 f"{edits.G}, got {tuple(x.shape)}")
            return torch.arange(edits.G, dtype=torch.int32, device=x.device)[:, None].expand(*lead)
        if not isinstance(edit_group, Tensor) or edit_group.dtype not in (torch.int32, torch.int64):
            raise ValueError("Sae.encode: edit_group must be an int32 or int64 tensor")
        if tuple(edit_group.shape) == lead:
            return edit_group
        if x.dim() == 3 and tuple(edit_group.shape) == lead[:1]:
            return edit_group[:, None].expand(*lead)
        raise ValueError(f"Sae.encode: edit_group must have shape {lead} (per token)" +
                         (f" or {lead[:1]} (per batch row)" if x.dim() == 3 else "") + f", got {tuple(edit_group.shape)}")

    def intervene(self, x: Tensor, edits, edit_group: Optional[Tensor] = None, *, exact: bool = False,
                  certified: bool = False) -> Tensor:
        """Error-preserving intervention: x + (decode(encode(x, edits)) - decode(encode(x))) in x's
        shape and dtype (f32 / bf16 / f16).  The hidden state keeps the SAE's reconstruction error and moves by the decoded
        EDIT alone; a token no edit touches keeps its own bits.  `edits`: a msae.features.FeatureEdits or RowEdits,
        `edit_group` as in `encode`.  One over-fetching encode (k + E, or k + E_max), the list edit, and ops.delta_decode, which
        gathers only the entries the two lists differ in -- the over-fetch's first k columns ARE the plain list.  The bits:
        include/msae.h, "error-preserving interventions".  Inference only: no host synchronisation, allocations through torch
        alone (capturable in a HIP graph); with gradients enabled on x it raises RuntimeError -- the hooks' autograd path is
        `msae.features.hooks.sae_reconstruct(preserve_error=True)`."""
        self._no_transcoder("Sae.intervene")
        self._topk_only("intervene")
        if edits is None or not (hasattr(edits, "check") and (hasattr(edits, "offsets") or hasattr(edits, "E"))):
            raise ValueError("Sae.intervene: edits must be a msae.features.FeatureEdits or RowEdits")
        if self.W_dec is None:
            raise ValueError("Sae.intervene: this Sae has no decoder")
        if x.dim() < 1 or x.shape[-1] != self.d_in:
            raise ValueError(f"Sae.intervene: x must be [..., {self.d_in}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"Sae.intervene: x must be float32, bfloat16 or float16, got {x.dtype}")
        edits.check(self.num_latents, self.cfg.k, self.encoder.weight.device)
        rows = hasattr(edits, "offsets")
        if edit_group is not None and not rows:
            raise ValueError("Sae.intervene: edit_group names the groups of a msae.features.RowEdits; it does not go with a "
                             "FeatureEdits")
        if rows:
            edit_group = self._token_groups(x, edits, edit_group)
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("Sae.intervene is an inference path: call it under torch.no_grad() or on a detached input "
                               "(sae_reconstruct(preserve_error=True) is the differentiable form)")
        k = self.cfg.k
        with torch.no_grad():
            flat = x.reshape(-1, self.d_in)
            acts, idx, _ = ops.encode_topk(flat, self.encoder.weight, self.encoder.bias, self._b_pre, self._prepared_weights(),
                                           k + (edits.E_max if rows else edits.E), exact=exact, certified=certified)
            if rows and edits.value_dependent:
                q_acts, q_idx = ops.edit_topk_rows(acts, idx, edit_group.reshape(-1), edits, self.num_latents, k,
                                                   cur=self._edit_cur(flat, edits.union), col=edits.col)
            elif rows:
                q_acts, q_idx = ops.edit_topk_rows(acts, idx, edit_group.reshape(-1), edits, self.num_latents, k)
            else:
                q_acts, q_idx = ops.edit_topk(acts, idx, edits.feat, edits.val, edits.kind, self.num_latents, k,
                                              cur=self._edit_cur(flat, edits.feat) if edits.value_dependent else None)
            out = ops.delta_decode(flat, acts[:, :k], idx[:, :k], q_acts, q_idx, self.W_dec)
        return out.view(x.shape)

    def transcode(self, x: Tensor, *, edits=None, edit_group: Optional[Tensor] = None, exact: bool = False) -> Tensor:
        """A transcoder's prediction of the module output from the module input: x [..., d_in] in
        f32 / bf16 / f16 -> f32 [..., d_out] = decode(encode(x)) + b_dec (+ x W_skip^T with cfg.skip_connection, accumulated
        in place into the decode's output).  `edits` / `edit_group` / `exact` as in `encode`: the edits work on the list as
        they do there.  A "batchtopk" or "jump" transcoder encodes with its threshold(s) and decodes the kept entries.
        Inference only: no host synchronisation, allocations through torch alone; with gradients enabled on x it raises
        RuntimeError (`forward(x, y=)` is the differentiable form)."""
        if not self.cfg.transcode:
            raise ValueError("Sae.transcode: this Sae is an auto-encoder (SaeConfig.transcode is off): decode(encode(x)) "
                             "reconstructs x itself")
        if self.W_dec is None:
            raise ValueError("Sae.transcode: this Sae has no decoder")
        if x.dim() < 1 or x.shape[-1] != self.d_in:
            raise ValueError(f"Sae.transcode: x must be [..., {self.d_in}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"Sae.transcode: x must be float32, bfloat16 or float16, got {x.dtype}")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("Sae.transcode is an inference path: call it under torch.no_grad() or on a detached input "
                               "(Sae.forward(x, y=) is the differentiable form)")
        with torch.no_grad():
            if self.cfg.activation in ("batchtopk", "jump"):
                top, lengths = self.encode(x, edits=edits, edit_group=edit_group, exact=exact, return_lengths=True)
            else:
                top, lengths = self.encode(x, edits=edits, edit_group=edit_group, exact=exact), None
            out = self.decode(top.top_acts, top.top_indices, lengths)
            if self.cfg.skip_connection:
                out = ops.skip_add(out.contiguous(), x, self.W_skip)
        return out

    def default_recon_ks(self) -> tuple:
        """Powers of two up to cfg.k, plus cfg.k itself."""
        k = self.cfg.k
        return tuple(sorted({1 << i for i in range(k.bit_length()) if (1 << i) <= k} | {k}))

    def recon_error(self, x: Tensor, ks=None, *, top=None, exact: bool = False, chunk: Optional[int] = None) -> ReconOutput:
        """The SAE's reconstruction error on x [..., d_in] (f32 / bf16 / f16) at several sparsities, without materialising a
        reconstruction: one pass over each token's k decoder rows that stops at the checkpoints `ks`
        (default: `default_recon_ks()`; strictly ascending in [0, k], at most 16, 0 = b_dec alone).  The canonical top-k list
        is value-descending, so its first kappa entries are the top-kappa list and checkpoint kappa is, bit for bit, the
        error of `decode` over an Sae with cfg.k = kappa.  `top`: the list of x (an EncoderOutput or (top_acts, top_indices))
        when the caller holds it already; None: `self.encode(x, exact=exact)`.  `chunk`: tokens per kernel call (None: one
        call); the per-token outputs do not depend on it.  Inference only; nothing is read back."""
        self._no_transcoder("Sae.recon_error")
        self._topk_only("recon_error")
        if self.W_dec is None:
            raise ValueError("Sae.recon_error: this Sae has no decoder")
        if x.dim() < 1 or x.shape[-1] != self.d_in:
            raise ValueError(f"Sae.recon_error: x must be [..., {self.d_in}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"Sae.recon_error: x must be float32, bfloat16 or float16, got {x.dtype}")
        if chunk is not None and chunk < 1:
            raise ValueError(f"Sae.recon_error: chunk must be positive, got {chunk}")
        if top is not None and len(top) != 2:
            raise ValueError("Sae.recon_error: top must be an EncoderOutput or a (top_acts, top_indices) pair")
        k = self.cfg.k if top is None else top[0].shape[-1]
        ks = ops.recon_ks(self.default_recon_ks() if ks is None else ks, k, "Sae.recon_error")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("Sae.recon_error is an inference path: call it under torch.no_grad() or on a detached input")
        with torch.no_grad():
            flat = x.reshape(-1, self.d_in)
            T = flat.shape[0]
            if top is None:
                top = self.encode(flat, exact=exact)
            acts, idx = top[0].reshape(T, k), top[1].reshape(T, k)
            step = T if chunk is None else chunk
            parts = [ops.recon_curve(flat[a:a + step], acts[a:a + step], idx[a:a + step], self.W_dec, self.b_dec, ks)
                     for a in range(0, T, max(step, 1))]
            if len(parts) == 1:
                mom, xx = parts[0]
            elif parts:
                mom, xx = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
            else:
                mom, xx = flat.new_empty((0, len(ks), 3), dtype=torch.float32), flat.new_empty((0,), dtype=torch.float32)
            tv = self._total_variance(flat)                # this call's own
        lead = tuple(x.shape[:-1])
        C = len(ks)
        return ReconOutput(tuple(ks), mom[..., 0].reshape(*lead, C), mom[..., 1].reshape(*lead, C),
                           mom[..., 2].reshape(*lead, C), xx.reshape(lead), tv, self.d_in)

    def _total_variance(self, flat: Tensor) -> Tensor:
        """(flat - flat.mean(0)).pow(2).sum(), two passes in float64, a block of rows at a time."""
        T = flat.shape[0]
        tv = flat.new_zeros((), dtype=torch.float64)
        if T:
            rows = max(1, (32 << 20) // self.d_in)
            mean = sum(flat[a:a + rows].sum(0, dtype=torch.float64) for a in range(0, T, rows)) / T
            for a in range(0, T, rows):
                tv += (flat[a:a + rows].to(torch.float64) - mean).square().sum()
        return tv

    def refit(self, x: Tensor, *, s: Optional[int] = None, top=None, exact: bool = False,
              chunk: Optional[int] = None) -> RefitOutput:
        """Why the reconstruction of x [..., d_in] (f32 / bf16 / f16) falls short: keep the support the
        encoder chose and refit its coefficients by least squares against the fixed decoder.  `err_enc - err_fit` is lost
        to the encoder's magnitudes (the amortisation gap, `gap`); `err_fit` is what the dictionary cannot express on that
        support.  `s`: refit the first s slots of the list (None: all of them; at most 64 -- a longer list needs an
        explicit s).  `top`: the list of x (an EncoderOutput or (top_acts, top_indices)) when the caller holds it already;
        None: `self.encode(x, exact=exact)`.  `chunk`: tokens per kernel call (None: one call); the per-token outputs do
        not depend on it.  Inference only; nothing is read back."""
        self._no_transcoder("Sae.refit")
        self._topk_only("refit")
        if self.W_dec is None:
            raise ValueError("Sae.refit: this Sae has no decoder")
        if x.dim() < 1 or x.shape[-1] != self.d_in:
            raise ValueError(f"Sae.refit: x must be [..., {self.d_in}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"Sae.refit: x must be float32, bfloat16 or float16, got {x.dtype}")
        if chunk is not None and chunk < 1:
            raise ValueError(f"Sae.refit: chunk must be positive, got {chunk}")
        if top is not None and len(top) != 2:
            raise ValueError("Sae.refit: top must be an EncoderOutput or a (top_acts, top_indices) pair")
        k = self.cfg.k if top is None else top[0].shape[-1]
        if s is None:
            if k > ops.REFIT_MAX_S:
                raise ValueError(f"Sae.refit: the list holds {k} slots and at most {ops.REFIT_MAX_S} are refit at once: pass "
                                 f"s={ops.REFIT_MAX_S} to refit its first {ops.REFIT_MAX_S}")
            s = k
        if isinstance(s, bool) or not isinstance(s, int) or not 1 <= s <= min(k, ops.REFIT_MAX_S):
            raise ValueError(f"Sae.refit: s must be an integer in [1, {min(k, ops.REFIT_MAX_S)}], got {s!r}")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("Sae.refit is an inference path: call it under torch.no_grad() or on a detached input")
        with torch.no_grad():
            flat = x.reshape(-1, self.d_in)
            T = flat.shape[0]
            if top is None:
                top = self.encode(flat, exact=exact)
            acts, idx = top[0].reshape(T, k), top[1].reshape(T, k)
            step = T if chunk is None else chunk
            parts = [ops.support_refit(flat[a:a + step], acts[a:a + step], idx[a:a + step], self.W_dec, self.b_dec, s)
                     for a in range(0, T, max(step, 1))]
            if len(parts) == 1:
                raw = parts[0]
            elif parts:
                raw = ops.RefitRaw(*(torch.cat(f) for f in zip(*parts)))
            else:
                e = lambda *shape, dt=torch.float32: flat.new_empty(shape, dtype=dt)
                raw = ops.RefitRaw(e(0, s), e(0, s), e(0), e(0), e(0), e(0, dt=torch.int32))
            tv = self._total_variance(flat)
        lead = tuple(x.shape[:-1])
        return RefitOutput(raw.coef.reshape(*lead, s), idx[:, :s].reshape(*lead, s), raw.gain.reshape(*lead, s),
                           raw.err_fit.reshape(lead), raw.err_enc.reshape(lead), raw.yy.reshape(lead),
                           raw.n_dependent.reshape(lead), tv)

    def nested_error(self, x: Tensor, bounds=None, *, top=None, exact: bool = False) -> NestedErrorOutput:
        """How well the first m features alone explain x, GIVEN the selection over all N features: the per-token squared
        error |r_g - x|^2 of the reconstruction r_g from the listed features below bounds[g], for every prefix size at once
        (include/msae.h, "nested decode"; one pass over each token's decoder rows, no residual planes).  x [..., d_in] in
        f32 / bf16 / f16.  `bounds`: prefix sizes, strictly ascending, at most 8, the last one num_latents; None:
        cfg.matryoshka (ValueError when the Sae has none).  `top`: the list of x when the caller holds it -- an EncoderOutput,
        (top_acts, top_indices) or (top_acts, top_indices, lengths); None: `self.encode(x, exact=exact)`.  Available on any
        Sae; inference only, nothing is read back.  Not the same question as `truncate(m)`, which RE-SELECTS the top-k
        among the first m features."""
        self._no_transcoder("Sae.nested_error")
        if bounds is None:
            bounds = self.cfg.matryoshka
            if not bounds:
                raise ValueError("Sae.nested_error: give bounds= (this Sae's cfg.matryoshka is empty)")
        bounds = ops.nested_bounds(bounds, self.num_latents, "Sae.nested_error")
        if self.W_dec is None:
            raise ValueError("Sae.nested_error: this Sae has no decoder")
        if x.dim() < 1 or x.shape[-1] != self.d_in:
            raise ValueError(f"Sae.nested_error: x must be [..., {self.d_in}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"Sae.nested_error: x must be float32, bfloat16 or float16, got {x.dtype}")
        if top is not None and len(top) not in (2, 3):
            raise ValueError("Sae.nested_error: top must be (top_acts, top_indices) or (top_acts, top_indices, lengths)")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("Sae.nested_error is an inference path: call it under torch.no_grad() or on a detached input")
        with torch.no_grad():
            flat = x.reshape(-1, self.d_in)
            T = flat.shape[0]
            if top is None:
                if self.cfg.activation in ("batchtopk", "jump"):
                    enc, lengths = self.encode(flat, exact=exact, return_lengths=True)
                    top = (enc.top_acts, enc.top_indices, lengths)
                else:
                    top = self.encode(flat, exact=exact)
            k = top[0].shape[-1]
            lengths = top[2].reshape(T) if len(top) == 3 and top[2] is not None else None
            _, sq, _ = ops.nested_decode(flat, top[0].reshape(T, k), top[1].reshape(T, k), self.W_dec, self.b_dec, bounds,
                                         lengths)
            xf = flat.to(torch.float32)
            xx = (xf * xf).sum(-1)
            tv = flat.new_zeros((), dtype=torch.float64)
            if T:
                rows = max(1, (32 << 20) // self.d_in)
                mean = sum(flat[a:a + rows].sum(0, dtype=torch.float64) for a in range(0, T, rows)) / T
                for a in range(0, T, rows):
                    tv += (flat[a:a + rows].to(torch.float64) - mean).square().sum()
        lead = tuple(x.shape[:-1])
        return NestedErrorOutput(bounds, sq.reshape(*lead, len(bounds)), xx.reshape(lead), tv, self.d_in)

    def truncate(self, m: int, copy: bool = False) -> "Sae":
        """An Sae over the first m features: how a trained Matryoshka prefix is used on its own (steering, probes, neighbours
        on a 16k dictionary cut from a 131k one).  By default its parameters are row-slice VIEWS that share storage with this
        Sae's (copy=True: its own copies); its prepared encoder operands are its own.  cfg.num_latents becomes m,
        cfg.matryoshka is cut to the sizes <= m (with m itself as the last size; the weights are cut along where m is one of
        the sizes and reset to uniform otherwise), and a "batchtopk" threshold buffer is carried over.  m need not be a
        multiple of 8192: the encoder takes whatever path it takes for such a width.

        `truncate(m)` RE-SELECTS the top-k among the first m features; `nested_error` keeps the selection over all N features
        and restricts it to those below m.  The two agree only where the full selection already lies inside the prefix."""
        import dataclasses

        self._no_transcoder("Sae.truncate")
        m = int(m)
        if not self.cfg.cap <= m <= self.num_latents:
            raise ValueError(f"Sae.truncate: m must lie in [{self.cfg.cap}, {self.num_latents}], got {m}")
        sizes = [s for s in self.cfg.matryoshka if s <= m]
        weights = list(self.cfg.matryoshka_weights[:len(sizes)]) if self.cfg.matryoshka_weights else []
        if self.cfg.matryoshka and (not sizes or sizes[-1] != m):
            sizes, weights = sizes + [m], []
        if weights and not sum(weights) > 0:
            weights = []
        cfg = dataclasses.replace(self.cfg, num_latents=m, matryoshka=sizes, matryoshka_weights=weights)
        new = Sae(self.d_in, cfg, device="meta", decoder=self.W_dec is not None)     # the shell: no storage of its own

        def part(t: Tensor) -> Tensor:
            t = t.detach()[:m]
            return t.clone() if copy else t

        new.encoder.weight = nn.Parameter(part(self.encoder.weight), requires_grad=self.encoder.weight.requires_grad)
        new.encoder.bias = nn.Parameter(part(self.encoder.bias), requires_grad=self.encoder.bias.requires_grad)
        if self.W_dec is not None:
            new.W_dec = nn.Parameter(part(self.W_dec), requires_grad=self.W_dec.requires_grad)
        b = self.b_dec.detach()
        new.b_dec = nn.Parameter(b.clone() if copy else b, requires_grad=self.b_dec.requires_grad)
        if cfg.activation == "batchtopk":
            new.threshold = self.threshold.detach().clone()
        if cfg.activation == "jump":
            new.log_threshold = nn.Parameter(part(self.log_threshold), requires_grad=self.log_threshold.requires_grad)
        if cfg.matryoshka:
            new._nested_w = torch.tensor(cfg.nested_weights, dtype=torch.float32, device=self.device)
        new.train(self.training)
        return new

    def _topk_only(self, what: str) -> None:
        """The paths that read a per-token top-k list are not built for a "batchtopk" Sae."""
        if self.cfg.activation == "batchtopk":
            raise NotImplementedError(f"Sae.{what} is not built for activation='batchtopk': it works on per-token top-k lists "
                                      "(encode with threshold= and decode with lengths= are the BatchTopK inference path)")
        if self.cfg.activation == "jump":
            raise NotImplementedError(f"Sae.{what} is not built for activation='jump': it works on per-token top-k lists "
                                      "(encode and decode with lengths= are the JumpReLU inference path)")

    def decode(self, top_acts: Tensor, top_indices: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
        """`lengths` (int32, one per row: what a threshold encode or ops.batch_select returned): only the kept prefix of every
        row is read (ops.decode(lengths=)); the same bits as without it on such a list, at the cost of sum(lengths)."""
        assert self.W_dec is not None, "Decoder weight was not initialized."
        if lengths is not None:
            return ops.decode(top_indices, top_acts.to(self.dtype), self.W_dec, self.b_dec, lengths)
        # the module-level seam, as the reference (sae.py:190): `decoder_impl(top_indices, top_acts, W_dec.mT) + b_dec`.  The
        # default implementation is called with the bias inside the kernel (same bits: the kernel adds b_dec behind the
        # chain; one pass over the [A, d] output instead of two); a rebound decoder_impl gets the reference's call.
        impl = _seam.decoder_impl
        if impl is _seam.hip_decode:
            return ops.decode(top_indices, top_acts.to(self.dtype), self.W_dec, self.b_dec)
        return impl(top_indices, top_acts.to(self.dtype), self.W_dec.mT) + self.b_dec

    # ---- probe (tools/probe_activations.py:109-126) ----------------------------------------------------
    def _probe_inputs(self, x: Tensor, segments, what: str):
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError(f"Sae.{what} is an inference path: call it under torch.no_grad() or on a detached input "
                               "(differentiate pre_acts for gradients)")
        kind, seg = _probe.parse_segments(segments, x.shape)
        flat = x.reshape(-1, x.shape[-1])
        dev = self.encoder.weight.device
        if kind == "device":
            return flat, seg, None
        chunks = _probe.plan_chunks(seg, self.num_latents, self._cu_count(dev))
        # one pinned buffer, copied without a host synchronisation: the segments, then the chunk plan
        host = torch.tensor(seg + chunks, dtype=torch.int32)
        both = host.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else host
        return flat, both[:len(seg)], both[len(seg):]

    @staticmethod
    def _cu_count(dev: torch.device) -> int:
        return torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == "cuda" else 256

    def pooled_acts(self, x: Tensor, segments=None, reduce: str = "mean") -> Tensor:
        """[S, N] f32: the mean (or max) of `pre_acts(x)` over the tokens of each segment, without the dense [T, N] latents.
        x: [T, d] or [B, L, d] in f32 / bf16 / f16.  segments: None (one per row of a [B, L, d] input, one over everything
        for [T, d]), a host sequence of (start, end) pairs over the flattened tokens (validated: sorted, disjoint,
        non-empty, inside [0, T)), or an int32 [S, 2] CUDA tensor (used as is: no host read; clamped to [0, T), an empty
        segment pools to 0).  Bits: include/msae.h, "probe" -- mean = (float)(ascending-token f64 sum / length)."""
        if reduce not in _probe.REDUCE:
            raise ValueError(f"reduce must be one of {sorted(_probe.REDUCE)}, got {reduce!r}")
        flat, seg, chunks = self._probe_inputs(x, segments, "pooled_acts")
        with torch.no_grad():
            return ops.pooled_acts(flat, self.encoder.weight, self.encoder.bias, self._b_pre, seg, chunks,
                                   _probe.REDUCE[reduce])

    def probe(self, x: Tensor, k: int, segments=None, reduce: str = "mean", maps: bool = True) -> ProbeOutput:
        """Which features each segment of `x` activates, and where (tools/probe_activations.py:109-126: pre_acts ->
        mean over the tokens -> topk -> the chosen features' activations per token), in one pooled GEMM, a top-k of the
        [S, N] pooled rows and a small recompute of the T x k map values.  Returns ProbeOutput(values [S, k] f32,
        indices [S, k] int64, maps [T, k] f32 or None); `segments` / `reduce` as in `pooled_acts`.  k <= min(N, 16384);
        with maps, k <= 256.  Every value equals what pre_acts -> mean / max -> topk -> gather computes (include/msae.h)."""
        if not 0 < k <= min(self.num_latents, 16384):
            raise ValueError(f"k must be in [1, {min(self.num_latents, 16384)}], got {k}")
        if maps and k > _probe.MAX_MAPS_K:
            raise ValueError(f"maps=True supports k <= {_probe.MAX_MAPS_K}, got {k}: probe with maps=False, or fewer features")
        if reduce not in _probe.REDUCE:
            raise ValueError(f"reduce must be one of {sorted(_probe.REDUCE)}, got {reduce!r}")
        flat, seg, chunks = self._probe_inputs(x, segments, "probe")
        with torch.no_grad():
            pooled = ops.pooled_acts(flat, self.encoder.weight, self.encoder.bias, self._b_pre, seg, chunks,
                                     _probe.REDUCE[reduce])
            values, indices = ops.topk(pooled, k)
            m = ops.probe_maps(flat, self.encoder.weight, self.encoder.bias, self._b_pre, seg, indices) if maps else None
        return ProbeOutput(values, indices, m)

    # ---- neighbours and top logits (features/stats.py:12-47,76-120) -----------------------------------------
    def _feature_rows(self, features, what: str) -> Optional[Tensor]:
        """`features` (None, a list or a tensor of indices) -> int32 device tensor [M] or None (all), no host sync."""
        if features is None:
            return None
        dev = self.encoder.weight.device
        if isinstance(features, Tensor):
            if features.dtype not in (torch.int32, torch.int64) or features.dim() != 1:
                raise ValueError(f"Sae.{what}: features must be a 1-d int tensor, got {features.dtype} {tuple(features.shape)}")
            return features.to(dev, torch.int32).clamp(0, self.num_latents - 1)
        host = torch.tensor([int(f) for f in features], dtype=torch.int32)
        if host.numel() and not (0 <= int(host.min()) and int(host.max()) < self.num_latents):
            raise ValueError(f"Sae.{what}: feature indices must lie in [0, {self.num_latents})")
        return host.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else host

    def neighbors(self, features=None, k: int = 10, matrix: str = "decoder", exclude_self: bool = True):
        """The k nearest features of each selected feature by cosine similarity of the decoder (or encoder) rows
        (features/stats.py:76-120) -> (values f32 [M, k], indices int64 [M, k]), value descending, ties by ascending
        index.  features: a list or 1-d int tensor of indices, or None for all N; matrix: "decoder" (W_dec) or "encoder"
        (encoder.weight), both [N, d]; exclude_self skips the feature's own index (rank 0 is NOT dropped: with duplicated
        rows the feature itself need not rank first).  One fused GEMM + top-k: the [M, N] cosines are never stored.
        cos = dot * inv[m] * inv[n] with inv = ops.row_inv_norms (include/msae.h, "neighbours").  A transcoder's decoder rows
        live in the OUTPUT space ([N, d_out]) and its encoder rows in the input space: the two matrices answer different
        questions there."""
        if matrix not in ("decoder", "encoder"):
            raise ValueError(f"matrix must be 'decoder' or 'encoder', got {matrix!r}")
        W = self.W_dec if matrix == "decoder" else self.encoder.weight
        if W is None:
            raise ValueError("this Sae has no decoder: use matrix='encoder'")
        lim = min(ops.ROWS_TOPK_MAX_K, self.num_latents - (1 if exclude_self else 0))
        if not 1 <= k <= lim:
            raise ValueError(f"k must be in [1, {lim}], got {k}")
        rows = self._feature_rows(features, "neighbors")
        with torch.no_grad():
            W = W.detach()
            inv = ops.row_inv_norms(W)
            if rows is None:                       # every feature: the scales are one array, the exclusion is the row number
                own = torch.arange(self.num_latents, dtype=torch.int32, device=W.device) if exclude_self else None
                return ops.rows_topk(W, W, k, q_scale=inv, k_scale=inv, exclude=own)
            return ops.rows_topk(W, W, k, q_rows=rows, q_scale=torch.index_select(inv, 0, rows.long()), k_scale=inv,
                                 exclude=rows if exclude_self else None)

    def top_logits(self, W_U: Tensor, features=None, k: int = 10):
        """Direct logit attribution (features/stats.py:12-47): the k tokens each selected feature's decoder row pushes
        hardest -> (values f32 [M, k], token ids int64 [M, k]).  W_U: the unembedding [V, d] in f32, bf16 or f16 (up-cast
        to f32 once); no scales, no exclusion.  A transcoder's decoder rows live in the OUTPUT space (d_out wide)."""
        if self.W_dec is None:
            raise ValueError("this Sae has no decoder")
        if W_U.dim() != 2 or W_U.shape[1] != self.d_out:
            raise ValueError(f"W_U must be [V, {self.d_out}], got {tuple(W_U.shape)}")
        lim = min(ops.ROWS_TOPK_MAX_K, W_U.shape[0])
        if not 1 <= k <= lim:
            raise ValueError(f"k must be in [1, {lim}], got {k}")
        rows = self._feature_rows(features, "top_logits")
        with torch.no_grad():
            return ops.rows_topk(self.W_dec.detach(), W_U.detach(), k, q_rows=rows)

    @staticmethod
    def _dead_list(dead_mask: Tensor) -> Tensor:
        """The dead features as an ascending int32 device list.  Its length is the forward's ONE host read (torch.nonzero
        sizes its result on the host): it takes the place of `int(dead_mask.sum())`."""
        return torch.nonzero(dead_mask).flatten().to(torch.int32)

    def forward(self, x: Tensor, dead_mask: Union[Tensor, None] = None, *, y: Optional[Tensor] = None,
                auxk_path: Optional[str] = None) -> ForwardOutput:
        """Training forward (sae.py:193-247): reconstruction, FVU, AuxK and Multi-TopK terms, fully
        differentiable.  The encoder is one autograd node with a sparse backward (ops._SparseEncode):
        gradients reach encoder.weight / encoder.bias / b_dec / x only through the selected latents,
        exactly as in the reference's dense graph, without its second [T,N]x[T,d] GEMM.

        auxk_path ("dense" / "subset"; None: the attribute `self.auxk_path`, "dense" unless set): how the AuxK selection
        of a non-empty dead_mask is built.  "dense" materialises the [T, N] latents (pre_acts, where(dead_mask, ., -inf),
        top-k three times).  "subset" (with max(k, 4k) <= 256; otherwise the dense branch runs) keeps the main and
        Multi-TopK selections on the fused encoder and takes the AuxK one from an exact GEMM over the dead features only
        (ops.topk_within) -- the same selections bit for bit, no [T, N] tensor.

        y: the TARGET of a transcoder (cfg.transcode), [..., d_out] over the same tokens as x: required
        there, a ValueError on a plain Sae.  The encoder reads x without subtracting b_dec, the output is decode + b_dec
        (+ x W_skip^T with cfg.skip_connection, on the main and the Multi-TopK reconstruction; not on AuxK's e_hat, which
        models the residual), and every loss term is today's expression with y in the target's place (k_aux = d_out // 2)."""
        if self.cfg.transcode:
            if y is None:
                raise ValueError("Sae.forward: a transcoder (SaeConfig.transcode) needs its target: forward(x, y=...)")
            if y.shape[:-1] != x.shape[:-1] or y.shape[-1] != self.d_out or x.shape[-1] != self.d_in:
                raise ValueError(f"Sae.forward: x must be [..., {self.d_in}] and y [..., {self.d_out}] over the same tokens, got "
                                 f"{tuple(x.shape)} and {tuple(y.shape)}")
        elif y is not None:
            raise ValueError("Sae.forward: y= is the target of a transcoder (SaeConfig.transcode); an auto-encoder's target is x")
        tgt = y if self.cfg.transcode else x
        skip = self.cfg.skip_connection
        if auxk_path is None:
            auxk_path = self.auxk_path
        if auxk_path not in ops.AUXK_PATHS:
            raise ValueError(f"auxk_path must be one of {ops.AUXK_PATHS}, got {auxk_path!r}")
        k_aux, scale, dead_list = 0, 0.0, None
        if dead_mask is not None:
            if auxk_path == "subset":
                dead_list = self._dead_list(dead_mask)
                num_dead = dead_list.numel()
            else:
                num_dead = int(dead_mask.sum())
            if num_dead > 0:
                k_aux = tgt.shape[-1] // 2                    # heuristic from the paper (sae.py:209)
                scale = min(num_dead / k_aux, 1.0)
                k_aux = min(k_aux, num_dead)
        k_multi = 4 * self.cfg.k if self.cfg.multi_topk else 0
        batch = self.cfg.activation == "batchtopk"
        jump = self.cfg.activation == "jump"
        k_main = self.cfg.cap                     # cfg.k, or the list width C of the batch-level selection
        if auxk_path == "subset":
            sel = ops.sparse_encode(x, self.encoder.weight, self.encoder.bias, self._b_pre, k_main,
                                    dead_mask, k_aux, k_multi, auxk_path="subset", dead_list=dead_list)
        else:
            sel = ops.sparse_encode(x, self.encoder.weight, self.encoder.bias, self._b_pre, k_main,
                                    dead_mask, k_aux, k_multi)
        top_acts, top_indices = sel[0]
        nested = bool(self.cfg.matryoshka)
        lengths = theta = n_saturated = None
        if batch:
            # BatchTopK: the T*k largest entries of the batch's top-C lists, and a decode that reads
            # the kept prefix of every row only; theta, the lengths and the saturation count stay on the device
            top_acts, lengths, theta, n_saturated = ops.batch_select(top_acts, top_indices, self.cfg.k)
        if jump:
            # JumpReLU: every row partitioned into kept / near / rest; the decode reads kept + near, so
            # its backward hands the near slots the gradient the straight-through estimator of their threshold needs
            top_acts, top_indices, lengths, reach, l0_sum, n_saturated = ops.jump_select(
                top_acts, top_indices, self.log_threshold.exp(), self.cfg.jump_bandwidth)
        if nested:
            # Matryoshka: the full reconstruction and every prefix's squared error from one pass over
            # the decoder rows, one autograd node
            bounds = tuple(self.cfg.matryoshka)
            sae_out, sq_sum = ops.nested_reconstruct(x, top_acts.to(self.dtype), top_indices, self.W_dec, self.b_dec, bounds,
                                                     lengths)
            sae_out = sae_out.view(x.shape)
        elif batch:
            sae_out = self.decode(top_acts, top_indices, lengths)
        elif jump:
            sae_out = self.decode(top_acts, top_indices, reach)
        else:
            sae_out = self.decode(top_acts, top_indices)
        if skip:
            sae_out = ops.skip_add(sae_out.contiguous(), x, self.W_skip)      # in place, into the decode's output
        # the loss terms in as few T x d sweeps as autograd allows (each elementwise torch op on [T, d] is a 45-us kernel at
        # C2; the reference's expression is ~10 of them forward + backward): squared error and its gradient through _SqErr,
        # the total variance as one column-variance kernel.  An input that itself requires grad keeps the plain expressions.
        # (a transcoder's target is y: tgt below; an auto-encoder's is x itself)
        lean = tgt.is_cuda and tgt.dim() == 2 and not tgt.requires_grad and tgt.dtype == torch.float32
        if nested:
            sq_err, e = sq_sum[-1], None if lean else sae_out - tgt
            total_variance = _total_variance(tgt) if lean else (tgt - tgt.mean(0)).pow(2).sum()
        elif lean:
            sq_err, e = _SqErr.apply(sae_out, tgt)
            total_variance = _total_variance(tgt)
        else:
            e = sae_out - tgt
            sq_err = e.pow(2).sum()
            total_variance = (tgt - tgt.mean(0)).pow(2).sum()

        if k_aux > 0:
            auxk_acts, auxk_indices = sel[1]
            e_hat = self.decode(auxk_acts, auxk_indices)
            # (e is the residual the dead latents should explain: a constant target, as in the reference's graph it carries
            # gradient to the main path too -- keep that: use the differentiable residual when it matters)
            e_t = e if not lean else (sae_out - tgt)
            auxk_loss = scale * (e_hat - e_t).pow(2).sum() / total_variance
        else:
            auxk_loss = sae_out.new_zeros(())           # (built on the device: no host-to-device copy)

        fvu = sq_err / total_variance
        if k_multi > 0:
            top_acts, top_indices = sel[-1]
            sae_out = self.decode(top_acts, top_indices)
            if skip:
                sae_out = ops.skip_add(sae_out.contiguous(), x, self.W_skip)
            multi_topk_fvu = (_SqErr.apply(sae_out, tgt)[0] if lean else (sae_out - tgt).pow(2).sum()) / total_variance
        else:
            multi_topk_fvu = sae_out.new_zeros(())
        if nested:
            nested_fvu = sq_sum / total_variance
            return NestedForwardOutput(sae_out, top_acts, top_indices, fvu, auxk_loss, multi_topk_fvu, nested_fvu=nested_fvu,
                                       nested_loss=(nested_fvu * self._nested_w).sum(), bounds=bounds, lengths=lengths,
                                       theta=theta, n_saturated=n_saturated)
        if jump:
            return JumpForwardOutput(sae_out, top_acts, top_indices, fvu, auxk_loss, multi_topk_fvu, lengths=lengths,
                                     reach=reach, l0=l0_sum / max(lengths.numel(), 1), n_saturated=n_saturated)
        if batch:
            return BatchForwardOutput(sae_out, top_acts, top_indices, fvu, auxk_loss, multi_topk_fvu, lengths=lengths,
                                      theta=theta, n_saturated=n_saturated)
        return ForwardOutput(sae_out, top_acts, top_indices, fvu, auxk_loss, multi_topk_fvu)

    # ---- decoder-norm utilities (sae.py:249-271) ------------------------------------------------------
    @torch.no_grad()
    def set_decoder_norm_to_unit_norm(self):
        assert self.W_dec is not None, "Decoder weight was not initialized."
        eps = torch.finfo(self.W_dec.dtype).eps
        W = self.W_dec.data
        if W.is_cuda and W.dtype == torch.float32 and W.is_contiguous():
            ops.unit_norm_rows_(W, eps)       # one read + one write of the 2 GiB matrix
        else:                                 # module still on the host (construction, checkpoint tools)
            W /= torch.norm(W, dim=1, keepdim=True) + eps

    @torch.no_grad()
    def remove_gradient_parallel_to_decoder_directions(self):
        assert self.W_dec is not None, "Decoder weight was not initialized."
        assert self.W_dec.grad is not None
        along = (self.W_dec.grad * self.W_dec.data).sum(dim=1, keepdim=True)
        self.W_dec.grad -= along * self.W_dec.data
