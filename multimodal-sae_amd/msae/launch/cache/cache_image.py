"""python -m msae.launch.cache.cache_image <model> <dataset> --sae_path ... --n_splits ... (README
command of the reference, launch/cache/cache_image.py:24-104): image feature caching."""
from __future__ import annotations

import torch
import torch.distributed as dist

from ...config import (TOKEN_PROFILE_IMAGE_ERROR, CacheConfig, act_hist_kwargs, cache_config_error, coact_kwargs,
                       parse_cache_config, pos_profile_grid_default, pos_profile_kwargs, recon_kwargs)
from ...features import FeatureImageCache
from ...utils import ddp_setup, load_filter, load_saes, maybe_load_llava_model, shard_offsets


COACT_DEFAULT_POOL = "image"
ACT_HIST_DEFAULT_POOL = "image"


def check_config(cfg: CacheConfig) -> None:
    """What this launcher refuses, before anything is loaded: the token profiles belong to the text cache."""
    if cfg.token_profile:
        cache_config_error(TOKEN_PROFILE_IMAGE_ERROR)


def main(cfg: CacheConfig):
    from datasets import load_dataset
    from transformers import AutoTokenizer

    check_config(cfg)
    ddp, rank, world = ddp_setup(timeout_s=18000)
    dtype = torch.bfloat16 if torch.cuda.is_bf16_supported() else "auto"
    model, processor = maybe_load_llava_model(cfg.model, rank, dtype, cfg.hf_token)
    tokenizer = AutoTokenizer.from_pretrained(cfg.model, token=cfg.hf_token)
    dataset = load_dataset(cfg.dataset, split=cfg.split)
    filters = load_filter(cfg.filters_path, device=model.device) if cfg.filters_path else None
    shard_size = 0
    if ddp:
        dist.barrier()
        dataset = dataset.shard(world, rank, contiguous=True)
        shard_size = sum(shard_offsets(len(dataset), model.device)[:rank])
    saes = load_saes(cfg.sae_path, filters=filters, device=model.device)
    stats = None
    pool_len = getattr(processor, "num_image_tokens", None) or 576
    if cfg.feature_stats:   # the image constructor pools the processor's first num_image_tokens positions
        stats = dict(pool="image", pool_len=pool_len, n_top=cfg.stats_top,
                     n_sample=cfg.stats_sample, sample_seed=cfg.stats_seed)
    pos = None
    if cfg.pos_profile:     # the base image's grid in cells of 4 x 4 and the rest of the row; log2 / linear bins over ctx_len
        try:
            pos = pos_profile_kwargs(cfg, cfg.pos_profile_bins or pos_profile_grid_default(pool_len), cfg.ctx_len)
        except ValueError as e:
            cache_config_error(str(e))
    cache = FeatureImageCache(model, tokenizer, saes, batch_size=cfg.batch_size, shard_size=shard_size,
                              processor=processor, filters=filters, stats=stats,
                              coact=coact_kwargs(cfg, COACT_DEFAULT_POOL, pool_len=pool_len, device=model.device),
                              recon=recon_kwargs(cfg, (0, pool_len)),    # the base image against the rest
                              hist=act_hist_kwargs(cfg, ACT_HIST_DEFAULT_POOL, pool_len=pool_len),
                              pos=pos)
    if ddp:
        dist.barrier()
    cache.run(cfg.ctx_len, dataset)
    cache.save_splits(n_splits=cfg.n_splits, save_dir=cfg.save_dir, rank=rank)
    if ddp:
        dist.barrier()
    if rank == 0:
        cache.concate_safetensors(n_splits=cfg.n_splits, save_dir=cfg.save_dir)
    if ddp:
        dist.barrier()


if __name__ == "__main__":
    main(parse_cache_config())
