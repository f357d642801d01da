"""Reconstruction error of an SAE over a dataset, against sparsity and position, built while the cache runs.

`Sae.recon_error` measures one batch; `ReconStats` accumulates the same moments over everything the cache loop pushes
through `encode`, next to `FeatureStats` and `CoactStats`.  One `ops.recon_curve` call per batch (msae_recon_curve_f32,
include/msae.h) gives, per token and per checkpoint kappa of `ks`, the moments (|r - x|^2, x . r, |r|^2) of the
reconstruction r from the token's first kappa list entries, and |x|^2; the rest is plain torch on `[B, S, C, 3]`.

Positions are split into GROUPS by `position_edges`, the first position of every group: (0,) is one group, (0, 576) is
the base image against the rest.  The last group is open-ended.  Per group the state is

    n                    tokens seen (a Python int, from the shapes alone)
    sums [C + 1, 3]      float64 sums of the three moments; kappa = 0 is always carried, whether `ks` asks for it or not
    xx_sum               float64 sum of |x|^2
    cos_sum [C + 1]      float64 sum of the per-token cosine x . r / (|x| |r|) (0 for a token with |x| |r| = 0)
    x_sum [d]            float64 sum of x

TOTAL VARIANCE without a second pass.  FVU divides by sum |x - mean|^2, and the mean is known only at the end.  The naive
one-pass form sum |x|^2 - n |mean|^2 cancels catastrophically on a residual stream with large constant dimensions.  With
a FIXED centre c,

    sum |x - mean|^2 = sum |x - c|^2 - n |mean - c|^2,

and the first term with c = b_dec is exactly the kappa = 0 checkpoint's error sum (r_0 = b_dec); the second comes from
x_sum.  b_dec is where training put the centre of the data, so |mean - b_dec| is small against the spread and the
subtraction is benign.

Unlike the integer counters of `FeatureStats` and `CoactStats`, these are FLOAT64 SUMS.  The per-token moments are
bit-identical however the rows are cut into calls or ranks; the accumulated sums agree only to float64 rounding (a
relative 2 n 2^-53 of the sum of the terms' magnitudes), and `merge` is associative to that bound, not bit for bit.

REFIT (`refit=True`).  One `ops.support_refit` call per batch (msae_support_refit_f32) beside the
curve: the least-squares optimum on the support the encoder chose, at every checkpoint of `ks` up to 64 (`refit_ks`) from
one factorisation.  Per group `refit_sums [R]` is the float64 sum of that optimal error, next to the encoder's own in
`sums[..., 0]`: their difference over the total variance is the amortisation gap (`gap`), the optimum over it is what the
dictionary cannot express on that support (`fvu_fit`).  Without the flag nothing of this exists, in memory or in the file.

The statistics cover exactly the positions handed to `update` -- in the cache loop every position the cache records,
padding included, as everything else in the loop does."""
from __future__ import annotations

import json
from typing import Optional, Sequence

import torch
from safetensors.torch import save_file
from torch import Tensor

from .. import ops
from ._pooled import open_stats_file

FORMAT = "msae.recon_stats.v1"
MAX_GROUPS = 8


def _edges(position_edges) -> tuple:
    try:
        e = tuple(int(p) for p in position_edges)
    except (TypeError, ValueError):
        raise ValueError(f"position_edges must be a sequence of integers, got {position_edges!r}") from None
    if not 1 <= len(e) <= MAX_GROUPS:
        raise ValueError(f"position_edges must name 1 to {MAX_GROUPS} groups, got {len(e)}")
    if e[0] != 0 or any(a >= b for a, b in zip(e, e[1:])):
        raise ValueError(f"position_edges must start at 0 and ascend strictly, got {e}")
    return e


class ReconStats:
    """Dataset-level reconstruction statistics of one SAE; see the module docstring.  `ks`: the checkpoints reported
    (strictly ascending, each at most the k of the lists passed to `update`); `b_dec`: the fixed centre, taken from the SAE
    of the first `update` when None.  `update` works on any device (the fused kernel on a HIP device); `merge`, the results,
    `save` and reading a loaded file need no GPU."""

    def __init__(self, d: int, ks: Sequence[int], position_edges: Sequence[int] = (0,), b_dec: Optional[Tensor] = None,
                 device=None, refit: bool = False):
        if d < 1:
            raise ValueError(f"d must be positive, got {d}")
        self.d = int(d)
        self.ks = tuple(ops.recon_ks(ks, ops.RECON_MAX_K, "ReconStats"))
        self._all_ks = self.ks if self.ks[0] == 0 else (0,) + self.ks           # kappa = 0 carried internally
        if len(self._all_ks) > ops.RECON_MAX_CHECKPOINTS:
            raise ValueError(f"ReconStats: at most {ops.RECON_MAX_CHECKPOINTS - 1} checkpoints besides 0, got {len(self.ks)}")
        self._slot = [self._all_ks.index(c) for c in self.ks]
        self.position_edges = _edges(position_edges)
        dev = torch.device("cpu") if device is None else torch.device(device)
        G, C1 = len(self.position_edges), len(self._all_ks)
        self.n = [0] * G
        self.sums = torch.zeros(G, C1, 3, dtype=torch.float64, device=dev)
        self.xx_sum = torch.zeros(G, dtype=torch.float64, device=dev)
        self.cos_sum = torch.zeros(G, C1, dtype=torch.float64, device=dev)
        self.x_sum = torch.zeros(G, self.d, dtype=torch.float64, device=dev)
        self.refit = bool(refit)
        self.refit_ks = tuple(c for c in self.ks if c <= ops.REFIT_MAX_S) if self.refit else ()
        self._refit_slot = [self._all_ks.index(c) for c in self.refit_ks]
        self.refit_sums = torch.zeros(G, len(self.refit_ks), dtype=torch.float64, device=dev) if self.refit else None
        self.b_dec: Optional[Tensor] = None
        if b_dec is not None:
            self._set_centre(b_dec)

    @property
    def device(self) -> torch.device:
        return self.sums.device

    @property
    def num_groups(self) -> int:
        return len(self.position_edges)

    def _set_centre(self, b_dec: Tensor) -> None:
        if b_dec.dim() != 1 or b_dec.shape[0] != self.d:
            raise ValueError(f"b_dec must be [{self.d}], got {tuple(b_dec.shape)}")
        self.b_dec = b_dec.detach().to(device=self.device, dtype=torch.float32).clone()

    def _ranges(self, S: int):
        ends = self.position_edges[1:] + (S,)
        return [(min(a, S), min(b, S)) for a, b in zip(self.position_edges, ends)]

    def update(self, hidden: Tensor, top_acts: Tensor, top_indices: Tensor, sae) -> None:
        """Add one batch: hidden [B, S, d] (f32 / bf16 / f16), its top-k list [B, S, k] and the SAE whose W_dec / b_dec
        decode it (the same SAE in every call: its b_dec is the centre).  One ops.recon_curve call, then float64 torch sums
        per group -- no atomics, no index_add_, nothing read back."""
        if hidden.dim() != 3 or hidden.shape[-1] != self.d:
            raise ValueError(f"hidden must be [B, S, {self.d}], got {tuple(hidden.shape)}")
        if top_acts.dim() != 3 or top_acts.shape != top_indices.shape or top_acts.shape[:2] != hidden.shape[:2]:
            raise ValueError(f"top_acts / top_indices must be [B, S, k] over hidden's rows, got {tuple(top_acts.shape)} and "
                             f"{tuple(top_indices.shape)}")
        if self.ks[-1] > top_acts.shape[-1]:
            raise ValueError(f"the checkpoints reach {self.ks[-1]}, the lists hold {top_acts.shape[-1]} entries")
        if getattr(getattr(sae, "cfg", None), "transcode", False):
            raise NotImplementedError("ReconStats.update " "is not built for a transcoder (SaeConfig.transcode): the curve compares the reconstruction with the "
                                      "encoder's own input, and a transcoder predicts another tensor (recon_error(x, y=) is a "
                                      "follow-up; Sae.transcode and msae.features.hooks.transcoder_hook are its inference paths)")
        if getattr(sae, "W_dec", None) is None:
            raise ValueError("ReconStats.update: this Sae has no decoder")
        if hidden.device != self.device:
            raise ValueError(f"hidden is on {hidden.device}, the statistics on {self.device}")
        if self.b_dec is None:
            self._set_centre(sae.b_dec)
        B, S, _ = hidden.shape
        if B * S == 0:
            return
        with torch.no_grad():
            mom, xx = ops.recon_curve(hidden.detach(), top_acts.detach(), top_indices, sae.W_dec, sae.b_dec, self._all_ks)
            den = (xx.to(torch.float64)[..., None] * mom[..., 2].to(torch.float64)).sqrt()
            cos = torch.where(den > 0, mom[..., 1].to(torch.float64) / den, torch.zeros_like(den))
            for g, (a, b) in enumerate(self._ranges(S)):
                if b <= a:
                    continue
                self.sums[g] += mom[:, a:b].sum((0, 1), dtype=torch.float64)
                self.xx_sum[g] += xx[:, a:b].sum(dtype=torch.float64)
                self.cos_sum[g] += cos[:, a:b].sum((0, 1))
                self.x_sum[g] += hidden[:, a:b].sum((0, 1), dtype=torch.float64)
                self.n[g] += B * (b - a)
            if self.refit_ks:
                raw = ops.support_refit(hidden.detach(), top_acts.detach(), top_indices, sae.W_dec, sae.b_dec,
                                        s=max(1, self.refit_ks[-1]))
                g64 = raw.gain.to(torch.float64)
                pre = torch.cat([torch.zeros_like(g64[..., :1]), g64.cumsum(-1)], -1)
                at = torch.stack([pre[..., c] for c in self.refit_ks], -1)                      # (selects: an index list would be copied
                opt = raw.yy.to(torch.float64)[..., None] - at                                  # to the device) [B, S, R]
                for g, (a, b) in enumerate(self._ranges(S)):
                    if b > a:
                        self.refit_sums[g] += opt[:, a:b].sum((0, 1))

    def _kind(self):
        return (self.d, self.ks, self.position_edges) + ((("refit",) + self.refit_ks,) if self.refit else ())

    def merge(self, other: "ReconStats") -> "ReconStats":
        """self += other (another rank's sums over the same checkpoints, groups, width and centre), on self's device."""
        if self._kind() != other._kind():
            raise ValueError(f"cannot merge reconstruction statistics of different kinds: {self._kind()} vs {other._kind()}")
        if self.b_dec is not None and other.b_dec is not None and \
                not torch.equal(self.b_dec.cpu().view(torch.int32), other.b_dec.cpu().view(torch.int32)):
            raise ValueError("cannot merge reconstruction statistics of different centres (b_dec differs)")
        if self.b_dec is None and other.b_dec is not None:
            self._set_centre(other.b_dec)
        dev = self.device
        self.sums += other.sums.to(dev)
        self.xx_sum += other.xx_sum.to(dev)
        self.cos_sum += other.cos_sum.to(dev)
        self.x_sum += other.x_sum.to(dev)
        if self.refit:
            self.refit_sums += other.refit_sums.to(dev)
        self.n = [a + b for a, b in zip(self.n, other.n)]
        return self

    # ---- results: float64 [C] on the CPU, of group `group` or (None) of all groups together ---------------------------
    def _state(self, group: Optional[int]):
        if group is None:
            return (sum(self.n), self.sums.sum(0).cpu(), self.xx_sum.sum(0).cpu(), self.cos_sum.sum(0).cpu(),
                    self.x_sum.sum(0).cpu())
        if not 0 <= group < self.num_groups:
            raise IndexError(f"group must lie in [0, {self.num_groups}), got {group}")
        return (self.n[group], self.sums[group].cpu(), self.xx_sum[group].cpu(), self.cos_sum[group].cpu(),
                self.x_sum[group].cpu())

    def total_variance(self, group: Optional[int] = None) -> Tensor:
        """sum |x - mean|^2 = sum |x - b_dec|^2 - n |mean - b_dec|^2 (float64 scalar); see the module docstring."""
        n, sums, _, _, x_sum = self._state(group)
        if n == 0 or self.b_dec is None:
            return torch.tensor(float("nan"), dtype=torch.float64)
        shift = x_sum / n - self.b_dec.cpu().to(torch.float64)
        return sums[0, 0] - n * (shift * shift).sum()

    def _err2(self, group):
        return self._state(group)[1][self._slot, 0]

    def fvu(self, group: Optional[int] = None) -> Tensor:
        """Fraction of variance unexplained per checkpoint: sum |r - x|^2 / sum |x - mean|^2."""
        return self._err2(group) / self.total_variance(group)

    def explained_variance(self, group: Optional[int] = None) -> Tensor:
        return 1.0 - self.fvu(group)

    def mse(self, group: Optional[int] = None) -> Tensor:
        """Mean squared error per element: sum |r - x|^2 / (n d)."""
        n = self._state(group)[0]
        return self._err2(group) / (n * self.d) if n else torch.full((len(self.ks),), float("nan"), dtype=torch.float64)

    def nmse(self, group: Optional[int] = None) -> Tensor:
        """sum |r - x|^2 / sum |x|^2."""
        return self._err2(group) / self._state(group)[2]

    def cosine(self, group: Optional[int] = None) -> Tensor:
        """Mean per-token cosine between x and its reconstruction."""
        n, _, _, cos_sum, _ = self._state(group)
        return cos_sum[self._slot] / n if n else torch.full((len(self.ks),), float("nan"), dtype=torch.float64)

    # ---- refit: float64 [R] over `refit_ks` ------------------------------------------------------------------------------
    def _refit(self, group: Optional[int]):
        if not self.refit:
            raise ValueError("these statistics were accumulated without refit=True")
        if group is not None and not 0 <= group < self.num_groups:
            raise IndexError(f"group must lie in [0, {self.num_groups}), got {group}")
        opt = (self.refit_sums.sum(0) if group is None else self.refit_sums[group]).cpu()
        return opt, self._state(group)[1][self._refit_slot, 0]

    def fvu_fit(self, group: Optional[int] = None) -> Tensor:
        """Fraction of variance unexplained at the least-squares coefficients on the encoder's support, per refit_ks."""
        return self._refit(group)[0] / self.total_variance(group)

    def gap(self, group: Optional[int] = None) -> Tensor:
        """The amortisation gap per refit_ks: (the encoder's error - the optimum on its support) / total variance."""
        opt, enc = self._refit(group)
        return (enc - opt) / self.total_variance(group)

    def summary(self, group: Optional[int] = None) -> str:
        """One line per checkpoint: kappa, fvu, cosine and, with refit, the optimum's fvu and the gap."""
        fvu, cos = self.fvu(group), self.cosine(group)
        head = f"{'kappa':>6} {'fvu':>10} {'cosine':>10}" + (f" {'fvu_fit':>10} {'gap':>10}" if self.refit else "")
        fit, gap = (self.fvu_fit(group), self.gap(group)) if self.refit else (None, None)
        lines = [head]
        for c, kappa in enumerate(self.ks):
            line = f"{kappa:>6} {float(fvu[c]):>10.6f} {float(cos[c]):>10.6f}"
            if self.refit:
                r = self.refit_ks.index(kappa) if kappa in self.refit_ks else None
                line += f" {float(fit[r]):>10.6f} {float(gap[r]):>10.6f}" if r is not None else f" {'-':>10} {'-':>10}"
            lines.append(line)
        return "\n".join(lines)

    # ---- file --------------------------------------------------------------------------------------------------------
    def metadata(self) -> dict:
        meta = {"format": FORMAT, "d": str(self.d), "ks": json.dumps(list(self.ks)),
                "position_edges": json.dumps(list(self.position_edges)), "n": json.dumps(self.n)}
        if self.refit:                                   # (without the flag the file is what it was, byte for byte)
            meta["refit_ks"] = json.dumps(list(self.refit_ks))
        return meta

    def save(self, path: str) -> None:
        tensors = {"sums": self.sums, "xx_sum": self.xx_sum, "cos_sum": self.cos_sum, "x_sum": self.x_sum}
        if self.b_dec is not None:
            tensors["b_dec"] = self.b_dec
        if self.refit:
            tensors["refit_sums"] = self.refit_sums
        save_file({k: v.detach().contiguous().cpu() for k, v in tensors.items()}, path, metadata=self.metadata())

    @classmethod
    def load(cls, path: str, device=None) -> "ReconStats":
        meta, tensors = open_stats_file(path, FORMAT, "a reconstruction statistics")
        st = cls(int(meta["d"]), json.loads(meta["ks"]), json.loads(meta["position_edges"]), b_dec=tensors.get("b_dec"),
                 device=device, refit="refit_ks" in meta)
        for name in ("sums", "xx_sum", "cos_sum", "x_sum") + (("refit_sums",) if st.refit else ()):
            getattr(st, name).copy_(tensors[name])
        st.n = [int(v) for v in json.loads(meta["n"])]
        return st
