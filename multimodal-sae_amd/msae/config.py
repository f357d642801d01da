"""CLI configuration of the caching entry points -- same fields, defaults, positional arguments and
`--flag` names as the reference's `CacheConfig` (sae_auto_interp/config.py:76-117), parsed with
argparse instead of simple_parsing (not installed on the target image)."""
from __future__ import annotations

import argparse
import dataclasses
import sys
from dataclasses import dataclass
from typing import Optional, Sequence, Union


@dataclass
class CacheConfig:
    model: str = "EleutherAI/pythia-160m"
    """Name of the model to use (positional)."""
    dataset: str = "togethercomputer/RedPajama-Data-1T-Sample"
    """Path to the dataset (positional)."""
    sae_path: Union[str, None] = None
    """Path to your trained sae, can be either local or on the hub"""
    batch_size: int = 32
    """Number of sequences to process in a batch"""
    load_in_8bit: bool = False
    """Load the model in 8-bit mode."""
    split: str = "train"
    """Dataset split to use."""
    n_splits: int = 2
    """Number of splits to divide .safetensors into"""
    ctx_len: int = 2048
    """Context length of the autoencoder. Each batch is shape (batch_size, ctx_len)"""
    hf_token: Union[str, None] = None
    """Huggingface API token for downloading models."""
    save_dir: str = "./features_cache"
    """Save dir for your feature"""
    verbosity: str = "INFO"
    """Verbosity level"""
    filters_path: Optional[str] = None
    """The json file for filtering the features and sae should be in a json file"""
    feature_stats: bool = False
    """Also write per-feature statistics and top-example tables (feature_stats.safetensors per module)"""
    stats_top: int = 64
    """Top examples kept per feature in the statistics (55..256)"""
    example_ctx_len: int = 64
    """Window length of the text statistics' max-pooled examples"""
    stats_sample: int = 0
    """Uniformly sampled examples kept per feature in the statistics (0: none, up to 256)"""
    stats_seed: int = 22
    """Seed of the statistics' example sample"""
    coact: bool = False
    """Also count which features fire together with the filtered features (coact.safetensors per module)"""
    coact_pool: Optional[str] = None
    """Segments of the co-activation counters: token, window or image (default: image on cache_image, token on cache)"""
    coact_features: Optional[str] = None
    """Filter-format json {module: [ids]} of the co-activation query features (default: --filters_path)"""
    recon_stats: bool = False
    """Also measure every SAE's reconstruction error against sparsity and position (recon_stats.safetensors per module)"""
    recon_ks: Optional[str] = None
    """Comma-separated checkpoints of --recon_stats, e.g. 0,1,2,4,8,16,32 (default: powers of two up to k, and k)"""
    recon_refit: bool = False
    """With --recon_stats: also refit every token's coefficients on its support by least squares (the amortisation gap)"""
    act_hist: bool = False
    """Also count how strongly every feature fires (act_hist.safetensors per module: a histogram per feature)"""
    act_hist_pool: Optional[str] = None
    """Segments of the activation histograms: token, window or image (default: image on cache_image, token on cache)"""
    act_hist_bins: Optional[str] = None
    """Bins of the activation histograms as s,e_lo,octaves: 2^s bins per octave from 2^e_lo up (default: 3,-16,32)"""
    pos_profile: bool = False
    """Also count where in a row every feature fires (pos_profile.safetensors per module: counts and strength per position bin)"""
    pos_profile_bins: Optional[str] = None
    """Position bins: grid:SIDE:CELL, log2 or linear:P (default: the image grid in cells of 4 on cache_image, log2 on cache)"""
    token_profile: bool = False
    """Also count on which tokens the filtered features fire (token_profile.safetensors per module; text cache only)"""
    token_profile_offsets: Optional[str] = None
    """Comma-separated token offsets of --token_profile, e.g. -1,0,1: the token at the firing position plus each (default: 0)"""
    token_profile_mass: bool = False
    """Also sum the activation strength per (feature, token), for the mean strength on a token"""

    def to_dict(self):
        return dataclasses.asdict(self)


@dataclass
class AttributionConfig:
    """sae_auto_interp/config.py:121-138."""
    model: str = "EleutherAI/pythia-160m"
    """Name of the model to use (positional)."""
    data_path: str = "./data/digit.json"
    """Path to the dataset. Should be a formated json file"""
    sae_path: Union[str, None] = None
    """Path to your trained sae, can be either local or on the hub"""
    selected_sae: str = "layers.24"
    """Name of the selected sae"""
    save_dir: str = "./attribution_cache"
    """Save dir for your feature attribution result"""
    method: str = "exact"
    """"exact": the reference's per-feature loop; "batched": all features from one forward + backward"""
    preserve_error: bool = False
    """(new) ablate in the model itself: the hooked layer keeps the SAE's reconstruction error (method "exact" only)"""

    def to_dict(self):
        return dataclasses.asdict(self)


def parse_attribution_config(argv: Optional[Sequence[str]] = None) -> AttributionConfig:
    p = argparse.ArgumentParser(description="Attribution patching (MI355X HIP path)")
    for f in dataclasses.fields(AttributionConfig):
        if f.name == "model":
            p.add_argument("model", nargs="?", default=f.default, type=str)
        elif f.type in (bool, "bool"):
            p.add_argument(f"--{f.name}", f"--{f.name.replace('_', '-')}", dest=f.name, action="store_true", default=f.default)
        else:
            p.add_argument(f"--{f.name}", type=str, default=f.default)
    return AttributionConfig(**vars(p.parse_args(argv)))


_POSITIONAL = ("model", "dataset")


def parse_cache_config(argv: Optional[Sequence[str]] = None) -> CacheConfig:
    p = argparse.ArgumentParser(description="Cache SAE feature activations (MI355X HIP path)")
    for f in dataclasses.fields(CacheConfig):
        if f.name in _POSITIONAL:
            p.add_argument(f.name, nargs="?", default=f.default, type=str)
        elif f.type in (bool, "bool"):
            p.add_argument(f"--{f.name}", action=argparse.BooleanOptionalAction, default=f.default)
        else:
            typ = int if f.type in (int, "int") else str
            p.add_argument(f"--{f.name}", type=typ, default=f.default)
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):       # `--token_profile_offsets -1,0,1`: argparse would read the value as a flag
        if argv[i] == "--token_profile_offsets" and argv[i + 1][:1] == "-" and argv[i + 1][1:2].isdigit():
            argv[i:i + 2] = [f"{argv[i]}={argv[i + 1]}"]
            break
    cfg = CacheConfig(**vars(p.parse_args(argv)))
    if cfg.coact_pool is not None and cfg.coact_pool not in COACT_POOLS:
        p.error(f"--coact_pool must be one of {', '.join(COACT_POOLS)}, got {cfg.coact_pool!r}")
    if cfg.coact and not (cfg.coact_features or cfg.filters_path):
        p.error("--coact needs query features: give --coact_features or --filters_path")
    if cfg.recon_ks is not None:
        try:
            recon_ks_list(cfg.recon_ks)
        except ValueError as e:
            p.error(str(e))
    if cfg.recon_refit and not cfg.recon_stats:
        p.error("--recon_refit adds to --recon_stats: give both")
    if cfg.act_hist_pool is not None and cfg.act_hist_pool not in COACT_POOLS:
        p.error(f"--act_hist_pool must be one of {', '.join(COACT_POOLS)}, got {cfg.act_hist_pool!r}")
    if cfg.act_hist_bins is not None:
        try:
            act_hist_bins(cfg.act_hist_bins)
        except ValueError as e:
            p.error(str(e))
    if cfg.pos_profile_bins is not None:
        try:
            pos_profile_spec(cfg.pos_profile_bins)
        except ValueError as e:
            p.error(str(e))
    if cfg.token_profile and not cfg.filters_path:
        p.error("--token_profile needs query features: give --filters_path")
    if cfg.token_profile_offsets is not None:
        try:
            token_profile_offsets(cfg.token_profile_offsets)
        except ValueError as e:
            p.error(str(e))
    return cfg


def token_profile_offsets(text: str) -> tuple:
    """'-1,0,1' -> (-1, 0, 1): one to four distinct integers in [-64, 64], within what the token profiles take
    (include/msae.h)."""
    try:
        offs = tuple(int(t) for t in text.split(","))
    except ValueError:
        raise ValueError(f"--token_profile_offsets must be comma-separated integers, got {text!r}") from None
    if not 1 <= len(offs) <= 4 or len(set(offs)) != len(offs) or min(offs) < -64 or max(offs) > 64:
        raise ValueError(f"--token_profile_offsets must be 1 to 4 distinct integers in [-64, 64], got {text!r}")
    return offs


def token_profile_kwargs(cfg: CacheConfig, vocab_size: int) -> Optional[dict]:
    """The `tokens=` argument of the text feature cache for a parsed command line (None without --token_profile): the
    launcher's vocabulary size, the offsets of --token_profile_offsets and --token_profile_mass.  The queries are the
    filter lists."""
    if not cfg.token_profile:
        return None
    offs = (0,) if cfg.token_profile_offsets is None else token_profile_offsets(cfg.token_profile_offsets)
    return dict(vocab_size=int(vocab_size), offsets=offs, mass=bool(cfg.token_profile_mass))


TOKEN_PROFILE_IMAGE_ERROR = ("--token_profile is for the text cache: image rows carry no token per position (the hidden "
                             "sequence the SAE sees holds the expanded image features and is not aligned with input_ids)")


def recon_ks_list(text: str) -> list:
    """'0,1,2,4' -> [0, 1, 2, 4]: non-negative, strictly ascending, at most 16."""
    try:
        ks = [int(t) for t in text.split(",")]
    except ValueError:
        raise ValueError(f"--recon_ks must be comma-separated integers, got {text!r}") from None
    if not 1 <= len(ks) <= 16 or ks[0] < 0 or any(a >= b for a, b in zip(ks, ks[1:])):
        raise ValueError(f"--recon_ks must be 1 to 16 strictly ascending non-negative integers, got {text!r}")
    return ks


def recon_kwargs(cfg: CacheConfig, position_edges=(0,)) -> Optional[dict]:
    """The `recon=` argument of the feature caches for a parsed command line (None without --recon_stats): the checkpoints
    of --recon_ks (None: every SAE's own default) and the launcher's position groups."""
    if not cfg.recon_stats:
        return None
    kw = dict(ks=None if cfg.recon_ks is None else recon_ks_list(cfg.recon_ks), position_edges=tuple(position_edges))
    if cfg.recon_refit:                                  # (absent without the flag: the off path is what it was)
        kw["refit"] = True
    return kw


COACT_POOLS = ("token", "window", "image")


def coact_kwargs(cfg: CacheConfig, default_pool: str, pool_len: int = 576, device="cpu") -> Optional[dict]:
    """The `coact=` argument of the feature caches for a parsed command line (None without --coact): the pool (the
    launcher's default unless --coact_pool), the window of the text statistics, `pool_len` of the image ones, and the
    query lists of --coact_features (without it the caches take the filter lists)."""
    if not cfg.coact:
        return None
    kw = dict(pool=cfg.coact_pool or default_pool, window=cfg.example_ctx_len, pool_len=pool_len)
    if cfg.coact_features:
        from .utils import load_filter

        kw["queries"] = load_filter(cfg.coact_features, device=device)
    return kw


def act_hist_bins(text: str) -> dict:
    """'s,e_lo,octaves' -> dict(sub_bits=s, e_lo=e_lo, octaves=octaves), within what the histograms take (include/msae.h):
    s in [0, 4], the octaves inside [-126, 128], at most 512 bins."""
    try:
        s, e_lo, octaves = (int(t) for t in text.split(","))
    except ValueError:
        raise ValueError(f"--act_hist_bins must be three comma-separated integers s,e_lo,octaves, got {text!r}") from None
    if not (0 <= s <= 4 and octaves >= 1 and e_lo >= -126 and e_lo + octaves <= 128 and octaves << s <= 512):
        raise ValueError(f"--act_hist_bins: s in [0, 4], octaves inside [-126, 128] and at most 512 bins, got {text!r}")
    return dict(sub_bits=s, e_lo=e_lo, octaves=octaves)


def act_hist_kwargs(cfg: CacheConfig, default_pool: str, pool_len: int = 576) -> Optional[dict]:
    """The `hist=` argument of the feature caches for a parsed command line (None without --act_hist): the pool (the
    launcher's default unless --act_hist_pool), the window of the text statistics, `pool_len` of the image ones, and the
    bins of --act_hist_bins."""
    if not cfg.act_hist:
        return None
    kw = dict(pool=cfg.act_hist_pool or default_pool, window=cfg.example_ctx_len, pool_len=pool_len)
    if cfg.act_hist_bins is not None:
        kw.update(act_hist_bins(cfg.act_hist_bins))
    return kw


def pos_profile_spec(text: str) -> tuple:
    """'grid:SIDE:CELL' -> ("grid", SIDE, CELL), 'log2' -> ("log2",), 'linear:P' -> ("linear", P), within what the position
    profiles take (include/msae.h): SIDE a positive multiple of CELL with SIDE^2 <= 65536, P in [1, 1024]."""
    parts = text.split(":")
    try:
        nums = [int(t) for t in parts[1:]]
    except ValueError:
        nums = None
    if nums is not None and parts[0] == "grid" and len(nums) == 2:
        side, cell = nums
        if not (cell >= 1 and 1 <= side <= 256 and side % cell == 0 and (side // cell) ** 2 < 1024):
            raise ValueError(f"--pos_profile_bins grid:SIDE:CELL needs SIDE in [1, 256], a multiple of CELL, and fewer than "
                             f"1024 cells, got {text!r}")
        return ("grid", side, cell)
    if nums == [] and parts[0] == "log2":
        return ("log2",)
    if nums is not None and parts[0] == "linear" and len(nums) == 1:
        if not 1 <= nums[0] <= 1024:
            raise ValueError(f"--pos_profile_bins linear:P needs P in [1, 1024], got {text!r}")
        return ("linear", nums[0])
    raise ValueError(f"--pos_profile_bins must be grid:SIDE:CELL, log2 or linear:P, got {text!r}")


def pos_profile_grid_default(pool_len: int, cell: int = 4) -> str:
    """The image launcher's default bins, 'grid:isqrt(pool_len):4': the base image's grid in cells of 4 x 4, one more bin for
    the rest of the row.  A `pool_len` that is no such grid is a ValueError that names the flag to give instead."""
    import math

    side = math.isqrt(pool_len)
    if side < 1 or side * side != pool_len or side % cell:
        raise ValueError(f"--pos_profile: {pool_len} image positions are not a square grid with a side divisible by {cell}; "
                         f"give --pos_profile_bins (grid:SIDE:CELL, log2 or linear:P)")
    return f"grid:{side}:{cell}"


def cache_config_error(message: str):
    """End like the parser does on a bad flag (usage, the message, exit status 2): for what a launcher can only check once
    the model is loaded."""
    argparse.ArgumentParser(description="Cache SAE feature activations (MI355X HIP path)").error(message)


def pos_profile_kwargs(cfg: CacheConfig, default_bins: str, length: int) -> Optional[dict]:
    """The `pos=` argument of the feature caches for a parsed command line (None without --pos_profile): the bins of
    --pos_profile_bins (the launcher's `default_bins` without it); log2 and linear bins span `length` positions, a grid gets
    one more bin for everything behind it."""
    if not cfg.pos_profile:
        return None
    from .features.pos import PosProfile

    spec = pos_profile_spec(cfg.pos_profile_bins or default_bins)
    if spec[0] == "grid":
        table, tail_bin, n_bins, _ = PosProfile.grid_bins(spec[1], spec[2], rest=True)
    elif spec[0] == "log2":
        table, tail_bin, n_bins, _ = PosProfile.log2_bins(length)
    else:
        table, tail_bin, n_bins, _ = PosProfile.linear_bins(length, spec[1])
    return dict(bins=table, tail_bin=tail_bin, n_bins=n_bins)
