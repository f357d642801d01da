"""Host side of `Sae.probe` / `Sae.pooled_acts`: the segment forms the methods accept and the chunk plan of the pooled
kernel (csrc/probe.hip).  Pure Python; nothing here touches a device.

A segment is a token range [start, end) over the flattened [T, d] hidden states.  The pooled kernel gives each workgroup one
128-feature strip and one CHUNK -- a run of adjacent segments it walks as packed 128-token tiles -- and never splits a segment,
so a segment's pooled value is the same however the segments are chunked (include/msae.h, "probe")."""
from __future__ import annotations

import math
import operator
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

TILE = 128                 # tokens (and features) per tile of the f32 MFMA kernel
WORKGROUPS_PER_CU = 2      # __launch_bounds__(256, 2) of pooled_f32_kernel
REDUCE = {"mean": 0, "max": 1}
MAX_MAPS_K = 256           # MSAE_PROBE_MAX_K


class ProbeOutput(NamedTuple):
    values: Tensor
    """[S, k] f32: the k largest pooled activations of each segment, descending (ties by ascending index)."""
    indices: Tensor
    """[S, k] int64: their feature indices."""
    maps: Optional[Tensor]
    """[T, k] f32: maps[t, j] = pre_acts(x)[t, indices[segment of t, j]]; 0 outside every segment.  None unless maps=True."""


Segments = Union[None, Tensor, Sequence[Tuple[int, int]]]


def default_segments(shape: Sequence[int]) -> List[Tuple[int, int]]:
    """None -> one segment per leading row of a [B, L, d] input, one over everything for [T, d]."""
    if len(shape) == 3:
        B, L = shape[0], shape[1]
        return [(b * L, (b + 1) * L) for b in range(B)]
    if len(shape) == 2:
        return [(0, shape[0])]
    raise ValueError(f"x must be [T, d] or [B, L, d], got shape {tuple(shape)}")


def validate_segments(segments: Sequence, T: int) -> List[Tuple[int, int]]:
    """A host sequence of (start, end) pairs -> list of int pairs; ValueError unless they are ints, sorted, non-overlapping,
    non-empty and inside [0, T)."""
    out: List[Tuple[int, int]] = []
    try:
        items = list(segments)
    except TypeError:
        raise ValueError(f"segments must be a sequence of (start, end) pairs, got {type(segments).__name__}") from None
    if not items:
        raise ValueError("segments is empty: give at least one (start, end) pair")
    prev_end = 0
    for i, item in enumerate(items):
        try:
            start, end = item
        except (TypeError, ValueError):
            raise ValueError(f"segment {i}: expected a (start, end) pair, got {item!r}") from None
        if isinstance(start, bool) or isinstance(end, bool):
            raise ValueError(f"segment {i}: bounds must be ints, got {item!r}")
        try:
            start, end = operator.index(start), operator.index(end)
        except TypeError:
            raise ValueError(f"segment {i}: bounds must be ints, got {item!r}") from None
        if not 0 <= start < end <= T:
            raise ValueError(f"segment {i}: [{start}, {end}) is empty or outside the {T} tokens")
        if start < prev_end:
            raise ValueError(f"segment {i}: [{start}, {end}) overlaps or precedes the previous segment (ends at {prev_end})")
        out.append((start, end))
        prev_end = end
    return out


def parse_segments(segments: Segments, shape: Sequence[int]):
    """-> ("host", [(start, end), ...]) validated, or ("device", int32 [S, 2] CUDA tensor) passed through unread."""
    if len(shape) not in (2, 3):
        raise ValueError(f"x must be [T, d] or [B, L, d], got shape {tuple(shape)}")
    T = math.prod(shape[:-1])
    if segments is None:
        return "host", default_segments(shape)
    if isinstance(segments, Tensor) and segments.is_cuda:
        if segments.dtype != torch.int32 or segments.dim() != 2 or segments.shape[1] != 2:
            raise ValueError("device segments must be an int32 [S, 2] tensor of (start, end) rows, got "
                             f"{segments.dtype} {tuple(segments.shape)}")
        return "device", segments
    if isinstance(segments, Tensor):
        segments = segments.tolist()
    return "host", validate_segments(segments, T)


def plan_chunks(segments: Sequence[Tuple[int, int]], N: int, n_cu: int = 256) -> List[Tuple[int, int]]:
    """Group validated segments into chunks [first, last) of adjacent segments for the pooled kernel.

    The launch is (N / 128 strips) x (chunks) workgroups.  Enough chunks are made that the grid fills the machine twice
    (2 x n_cu x WORKGROUPS_PER_CU workgroups) where the strips alone do not; the tokens are spread over them evenly: a chunk
    closes before a segment that would take it past the budget (total / chunks, rounded up to whole tiles) and at every gap
    between segments (so no token outside a segment is computed).  A segment longer than the budget is a chunk of its own --
    segments are never split, which keeps every pooled value one ascending-token chain."""
    if not segments:
        return []
    strips = -(-N // TILE)
    want = max(1, -(-2 * n_cu * WORKGROUPS_PER_CU // strips))
    total = sum(e - s for s, e in segments)
    budget = -(-total // want)
    budget = -(-budget // TILE) * TILE
    chunks: List[Tuple[int, int]] = []
    first, tokens, prev_end = 0, 0, None
    for i, (s, e) in enumerate(segments):
        if i > first and (s != prev_end or tokens + (e - s) > budget):
            chunks.append((first, i))
            first, tokens = i, 0
        tokens += e - s
        prev_end = e
    chunks.append((first, len(segments)))
    return chunks
