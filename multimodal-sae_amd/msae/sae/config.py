"""SaeConfig / TrainConfig -- field-for-field mirror of the reference dataclasses
(sae_auto_interp/sae/config.py:7-78) without the simple_parsing dependency.  `to_dict()` gives the
same keys the reference writes into cfg.json (sae.py:150-162)."""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field
from typing import List, Union


class _Serializable:
    def to_dict(self) -> dict:
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d: dict, drop_extra_fields: bool = True):
        names = {f.name for f in dataclasses.fields(cls)}
        extra = set(d) - names
        if extra and not drop_extra_fields:
            raise TypeError(f"unexpected fields {sorted(extra)}")
        return cls(**{k: v for k, v in d.items() if k in names})


@dataclass
class SaeConfig(_Serializable):
    """Configuration of a TopK sparse autoencoder (config.py:7-29)."""

    expansion_factor: int = 32
    """Multiple of the input dimension to use as the SAE dimension."""
    normalize_decoder: bool = True
    """Normalize the decoder weights to have unit norm."""
    num_latents: int = 0
    """Number of latents to use. If 0, use `expansion_factor`."""
    k: int = 32
    """Number of nonzero features."""
    multi_topk: bool = False
    """Use Multi-TopK loss."""
    signed: bool = False
    """Kept so older checkpoints' cfg.json load."""
    activation: str = "topk"
    """"topk": k latents per token.  "batchtopk": the T*k largest of the batch in training, a learned threshold in inference
    (DESIGN.md section 7n).  "jump": JumpReLU, a learned threshold per feature (DESIGN.md section 7s)."""
    batch_cap: int = 0
    """"batchtopk" and "jump": the most latents one token may keep (the width C of the lists the selection works on).
    0: min(4k, 256).  "jump": at most 256."""
    jump_bandwidth: float = 1e-3
    """"jump" only: the bandwidth eps of the rectangle kernel of the straight-through estimators."""
    jump_init: float = 1e-3
    """"jump" only: the threshold every feature starts from."""
    matryoshka: List[int] = field(default_factory=list)
    """Matryoshka prefix sizes m_0 < m_1 < ... < m_{G-1} = num_latents (at most 8): the first m_g latents must reconstruct
    the input on their own, under one selection over all latents (DESIGN.md section 7o).  Empty: a plain SAE."""
    matryoshka_weights: List[float] = field(default_factory=list)
    """One loss weight per prefix (finite, not negative, a positive sum).  Empty: 1 / G each."""
    transcode: bool = False
    """A transcoder (DESIGN.md section 7u): the dictionary reads one tensor and predicts ANOTHER (a module's input -> its
    output).  b_dec lives in the output space and is not subtracted in front of the encoder; W_dec starts at zero and is
    never normalised."""
    skip_connection: bool = False
    """A transcoder only: a dense linear map W_skip [d_out, d_in] (zero-initialised) beside the sparse path."""

    ACTIVATIONS = ("topk", "batchtopk", "jump")
    JUMP_MAX_CAP = 256
    MATRYOSHKA_MAX_GROUPS = 8

    def __post_init__(self):
        if self.activation not in self.ACTIVATIONS:
            raise ValueError(f"activation must be one of {self.ACTIVATIONS}, got {self.activation!r}")
        if self.batch_cap < 0:
            raise ValueError(f"batch_cap must not be negative, got {self.batch_cap}")
        for name in ("transcode", "skip_connection"):
            if not isinstance(getattr(self, name), bool):
                raise ValueError(f"{name} must be a bool, got {getattr(self, name)!r}")
        if self.skip_connection and not self.transcode:
            raise ValueError("skip_connection is the dense path of a transcoder: it needs transcode=True")
        if self.transcode and self.matryoshka:
            raise ValueError("matryoshka with transcode is not built (a follow-up: the nested decode node takes ONE tensor as "
                             "input and as target; a Matryoshka transcoder needs the two apart)")
        if self.activation == "batchtopk":
            if self.multi_topk:
                raise ValueError("multi_topk is a per-token TopK loss term: it does not go with activation='batchtopk'")
            if not self.k <= self.cap <= 4096:
                raise ValueError(f"batch_cap must lie in [k = {self.k}, 4096], got {self.cap}")
        if self.activation == "jump":
            if self.multi_topk:
                raise ValueError("multi_topk is a per-token TopK loss term: it does not go with activation='jump'")
            if self.matryoshka:
                raise ValueError("matryoshka with activation='jump' is not built (a follow-up: the nested decode of a "
                                 "three-way partitioned list)")
            if not self.k <= self.cap <= self.JUMP_MAX_CAP:
                raise ValueError(f"batch_cap must lie in [k = {self.k}, {self.JUMP_MAX_CAP}] for activation='jump', got {self.cap}")
            for name in ("jump_bandwidth", "jump_init"):
                v = getattr(self, name)
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v > 0 and math.isfinite(v)):
                    raise ValueError(f"{name} must be a positive finite number, got {v!r}")
        self.matryoshka = list(self.matryoshka or [])
        self.matryoshka_weights = list(self.matryoshka_weights or [])
        if self.matryoshka_weights and not self.matryoshka:
            raise ValueError("matryoshka_weights needs the prefix sizes in matryoshka")
        if self.matryoshka:
            sizes = self.matryoshka
            if any(isinstance(m, bool) or not isinstance(m, int) for m in sizes):
                raise ValueError(f"matryoshka must hold integers, got {sizes!r}")
            if len(sizes) > self.MATRYOSHKA_MAX_GROUPS:
                raise ValueError(f"matryoshka takes at most {self.MATRYOSHKA_MAX_GROUPS} prefix sizes, got {len(sizes)}")
            if sizes[0] < 1 or any(a >= b for a, b in zip(sizes, sizes[1:])):
                raise ValueError(f"matryoshka prefix sizes must be at least 1 and strictly ascending, got {sizes}")
            if self.num_latents and sizes[-1] != self.num_latents:
                raise ValueError(f"the last matryoshka prefix size must be num_latents = {self.num_latents}, got {sizes[-1]}")
            if self.multi_topk:
                raise ValueError("multi_topk is a loss term of the full dictionary alone: it does not go with matryoshka")
            w = self.matryoshka_weights
            if w:
                if len(w) != len(sizes):
                    raise ValueError(f"matryoshka_weights must hold one weight per prefix size ({len(sizes)}), got {len(w)}")
                try:
                    w = [float(v) for v in w]
                except (TypeError, ValueError):
                    raise ValueError(f"matryoshka_weights must hold numbers, got {self.matryoshka_weights!r}") from None
                if any(not math.isfinite(v) or v < 0 for v in w) or not sum(w) > 0:
                    raise ValueError(f"matryoshka_weights must be finite, not negative and have a positive sum, got {w}")
                self.matryoshka_weights = w

    @property
    def cap(self) -> int:
        """The list width of the main selection: k for "topk", batch_cap (0: min(4k, 256)) for "batchtopk" and "jump"."""
        if self.activation == "topk":
            return self.k
        return self.batch_cap or min(4 * self.k, 256)

    @property
    def nested_weights(self) -> List[float]:
        """The loss weight of every prefix: matryoshka_weights, or 1 / G each."""
        G = len(self.matryoshka)
        return list(self.matryoshka_weights) or [1.0 / G] * G

    def to_dict(self) -> dict:
        """The BatchTopK, Matryoshka and transcoder fields are written only where they differ from the defaults, the JumpReLU
        ones only for "jump": a TopK cfg.json is the reference's."""
        d = super().to_dict()
        if d["activation"] != "jump":
            del d["jump_bandwidth"], d["jump_init"]
        if d["activation"] == "topk":
            del d["activation"]
        if d["batch_cap"] == 0:
            del d["batch_cap"]
        for name in ("matryoshka", "matryoshka_weights", "transcode", "skip_connection"):
            if not d[name]:
                del d[name]
        return d


@dataclass
class TrainConfig(_Serializable):
    """Training hyper-parameters (config.py:32-78); consumed by the trainer row."""

    sae: SaeConfig = field(default_factory=SaeConfig)
    batch_size: int = 8
    grad_acc_steps: int = 1
    micro_acc_steps: int = 1
    lr: Union[float, None] = None
    lr_warmup_steps: int = 1000
    auxk_alpha: float = 0.0
    dead_feature_threshold: int = 10_000_000
    hookpoints: List[str] = field(default_factory=list)
    layers: List[int] = field(default_factory=list)
    layer_stride: int = 1
    distribute_modules: bool = False
    save_every: int = 1000
    log_to_wandb: bool = True
    run_name: Union[str, None] = None
    wandb_log_frequency: int = 1

    def to_dict(self) -> dict:
        return {**super().to_dict(), "sae": self.sae.to_dict()}
