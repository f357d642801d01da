"""Activation masks over the base image (reference features/features.py:130-136, tools/probe_activations.py:135-160).

A feature's per-token activations on the first 576 image positions (LLaVA-NeXT's 24 x 24 base-image grid) become a mask:
224 where the activation is below 1e-5, 0 where the feature fires; bilinearly resized to 336 x 336 and used to composite a
black background over the 336 x 336 resized image, so the regions that activate the feature stay visible."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
from PIL import Image

BASE_IMAGE_TOKENS = 576
PATCH_GRID = 24
IMAGE_SIZE = (336, 336)


def upsample_mask(acts, image_size: Tuple[int, int] = IMAGE_SIZE, value: int = 224, mode=Image.BILINEAR) -> Image.Image:
    """[h, w] activations (array or tensor) -> "L" mask image: `value` where the activation is < 1e-5, resized."""
    a = acts.detach().cpu().numpy() if hasattr(acts, "detach") else np.asarray(acts)
    mask = (a < 1e-5).astype(np.int64) * value
    return Image.fromarray(mask.astype(np.uint8), mode="L").resize(image_size, mode)


def base_grid(acts, tokens: int = BASE_IMAGE_TOKENS, grid: int = PATCH_GRID) -> np.ndarray:
    """The first `tokens` positions of a [L] activation row as a [grid, grid] array; a shorter row is padded with zeros."""
    a = acts.detach().cpu().numpy() if hasattr(acts, "detach") else np.asarray(acts)
    a = np.asarray(a, dtype=np.float32).ravel()[:tokens]
    if a.size < tokens:
        a = np.concatenate([a, np.zeros(tokens - a.size, dtype=np.float32)])
    return a.reshape(grid, grid)


def activation_image(image: Image.Image, acts, image_size: Tuple[int, int] = IMAGE_SIZE) -> Image.Image:
    """One feature's mask composited onto the resized image (reference: Image.composite(background, image, mask))."""
    mask = upsample_mask(base_grid(acts), image_size)
    background = Image.new("L", image_size, 0).convert("RGB")
    return Image.composite(background, image.convert("RGB").resize(image_size), mask).convert("RGB")


def activation_images(image: Image.Image, maps_rows: Sequence) -> list:
    """activation_image for each feature's [L] activation row."""
    return [activation_image(image, row) for row in maps_rows]
