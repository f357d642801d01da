"""What the accumulators of the cache loop share on the host (`FeatureStats`, `CoactStats`, `ActHist`, `ReconStats`): the pool
modes and their argument checks, the segment arithmetic, the checks and the whole-row chunking of an `update`, the call into
a pooled `msae_*_update` entry, and the statistics files.  csrc/pool_segments.h is the device side of the same pooling."""
from __future__ import annotations

import json
import struct
from typing import Dict, Iterator, Sequence, Tuple

import torch
from safetensors import safe_open
from torch import Tensor

from .. import _hip, ops

POOL_MODES = {"image": 0, "window": 1, "token": 2}
MAX_LATENTS, MAX_K, MAX_CALL_TOKENS, MAX_POOL_LEN, MAX_WINDOW = 262144, 256, 65536, 2880, 4096


# ---- constructor arguments -------------------------------------------------------------------------------------------------
def check_pool(pool: str, allowed: Sequence[str] = tuple(POOL_MODES)) -> None:
    if pool not in allowed:
        raise ValueError(f"pool must be one of {sorted(allowed)}, got {pool!r}")


def check_pool_args(num_latents: int, pool: str, pool_len: int, window: int) -> None:
    if not 0 < num_latents <= MAX_LATENTS:
        raise ValueError(f"num_latents must lie in [1, {MAX_LATENTS}], got {num_latents}")
    if pool == "image" and not 0 < pool_len <= MAX_POOL_LEN:
        raise ValueError(f"pool_len must lie in [1, {MAX_POOL_LEN}], got {pool_len}")
    if pool == "window" and not 0 < window <= MAX_WINDOW:
        raise ValueError(f"window must lie in [1, {MAX_WINDOW}], got {window}")


def pool_kind(pool: str, pool_len: int, window: int) -> tuple:
    """The pool part of an accumulator's kind: only the parameter its pool uses counts."""
    return (pool, pool_len if pool == "image" else None, window if pool == "window" else None)


# ---- one update ------------------------------------------------------------------------------------------------------------
def segments_of(pool: str, B: int, S: int, window: int) -> int:
    if pool == "token":
        return B * S
    if pool == "window":
        return B * (S // window)
    return B


def topk_shape(top_acts: Tensor, top_indices: Tensor) -> Tuple[int, int, int]:
    if top_acts.dim() != 3 or top_acts.shape != top_indices.shape:
        raise ValueError(f"top_acts / top_indices must be [B, S, k] of one shape, got {tuple(top_acts.shape)} and "
                         f"{tuple(top_indices.shape)}")
    return tuple(top_acts.shape)


def check_call_limits(S: int, k: int) -> None:
    if not 0 < k <= MAX_K:
        raise ValueError(f"k must lie in [1, {MAX_K}], got {k}")
    if S > MAX_CALL_TOKENS:
        raise ValueError(f"rows of {S} positions exceed {MAX_CALL_TOKENS}")


def total_segments(seen: int, more: int) -> int:
    total = seen + more
    if total >= 1 << 31:
        raise OverflowError(f"{total} segments: the int32 counters hold fewer than 2^31")
    return total


def row_chunks(B: int, S: int) -> Iterator[slice]:
    """Whole rows, at most MAX_CALL_TOKENS positions a call: a row never spans two calls, so any such cut is exact."""
    rows = max(1, MAX_CALL_TOKENS // S)
    for b0 in range(0, B, rows):
        yield slice(b0, b0 + rows)


def topk_inputs(top_acts: Tensor, top_indices: Tensor, *state: Tensor):
    """What a custom op around a pooled `msae_*_update` entry starts with: (the device of the batch and of the `state` it
    updates, the library, vals f32 / idx int32, contiguous, (B * S, k))."""
    dev = _hip.require_device(top_acts, top_indices, *state)
    lib = _hip.load()
    assert top_acts.dim() == 3 and top_acts.shape == top_indices.shape
    B, S, k = top_acts.shape
    return dev, lib, ops._f32c(top_acts), ops._idx32(top_indices), (B * S, k)


def pooled_update(lib, entry: str, vals: Tensor, idx: Tensor, thresh: float, N: int, mode: int, pool_len: int, window: int,
                  args: Sequence, ws: Tensor) -> None:
    """`lib.<entry>(vals, idx, B, S, k, thresh, N, mode, pool_len, window, *args, ws, ws_bytes, stream)`, checked.  The op
    fetches `ws` itself: `ops._workspace`, looked up when it is called."""
    B, S, k = vals.shape
    _hip.check(getattr(lib, entry)(_hip.ptr(vals), _hip.ptr(idx), B, S, k, thresh, N, mode, pool_len, window, *args,
                                   _hip.ptr(ws), ws.numel(), _hip.stream_of(vals)), entry)


# ---- files -----------------------------------------------------------------------------------------------------------------
def open_stats_file(path: str, fmt: str, what: str) -> Tuple[Dict[str, str], Dict[str, Tensor]]:
    """(metadata, tensors) of a statistics file whose metadata names the format `fmt`; `what`: "a ... statistics"."""
    with safe_open(path, framework="pt") as fh:
        meta = fh.metadata() or {}
        if meta.get("format") != fmt:
            raise ValueError(f"{path}: not {what} file")
        return meta, {k: fh.get_tensor(k) for k in fh.keys()}


_ST_DTYPES = {torch.int64: "I64", torch.int32: "I32"}


def _write_safetensors(tensors: Dict[str, Tensor], path: str, metadata: Dict[str, str]) -> None:
    """A safetensors file with a canonical header (metadata keys sorted; tensors by item size, then name; padded to eight
    bytes): equal state gives equal bytes, which `safetensors.torch.save_file` does not promise for several metadata
    keys.  Any safetensors reader opens it."""
    header, off, blobs = {"__metadata__": {k: metadata[k] for k in sorted(metadata)}}, 0, []
    for name in sorted(tensors, key=lambda n: (-tensors[n].element_size(), n)):
        t = tensors[name]
        blob = t.numpy().tobytes()
        header[name] = {"dtype": _ST_DTYPES[t.dtype], "shape": list(t.shape), "data_offsets": [off, off + len(blob)]}
        off += len(blob)
        blobs.append(blob)
    head = json.dumps(header, separators=(",", ":")).encode()
    head += b" " * (-len(head) % 8)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<Q", len(head)))
        fh.write(head)
        for blob in blobs:
            fh.write(blob)
