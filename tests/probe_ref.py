"""Numpy restatement of the probe's numerics contract (include/msae.h, "probe"), from the dense
pre-activations v[T, N] (= oracle.pre_acts / Sae.pre_acts, bit for bit):

  mean   (float)(S_f / n): S_f the f64 sum of v[t, f] over the segment, added one by one in ascending t from +0.0
         (np.add.accumulate is that sequential chain; np.sum would add pairwise)
  max    max_t v[t, f]; 0 for an all-zero column
  rank   canonical top-k of each pooled row: value descending, index ascending
  maps   maps[t, j] = v[t, idx[s, j]] for t in segment s; 0 outside every segment

Segments are clamped to [0, T) as the kernel clamps device-side segments; an empty one pools to 0."""
from __future__ import annotations

import numpy as np


def clamp(seg, T):
    b, e = int(seg[0]), int(seg[1])
    b = min(max(b, 0), T)
    e = min(max(e, b), T)
    return b, e


def pooled(v: np.ndarray, segments, reduce: str = "mean") -> np.ndarray:
    T, N = v.shape
    out = np.zeros((len(segments), N), dtype=np.float32)
    for s, seg in enumerate(segments):
        b, e = clamp(seg, T)
        if e <= b:
            continue
        if reduce == "mean":
            acc = np.add.accumulate(v[b:e].astype(np.float64), axis=0)[-1] + 0.0
            out[s] = (acc / np.float64(e - b)).astype(np.float32)
        else:
            out[s] = np.maximum(v[b:e].max(axis=0), np.float32(0.0))
    return out


def topk(rows: np.ndarray, k: int):
    """Canonical top-k (value desc, index asc) of each row; -0.0 ranks with +0.0."""
    vals = np.empty((rows.shape[0], k), dtype=np.float32)
    idx = np.empty((rows.shape[0], k), dtype=np.int64)
    for r, row in enumerate(rows):
        key = np.where(row == 0, np.float32(0.0), row).astype(np.float64)
        order = np.lexsort((np.arange(row.size), -key))[:k]
        idx[r], vals[r] = order, row[order]
    return vals, idx


def maps(v: np.ndarray, segments, idx: np.ndarray) -> np.ndarray:
    T = v.shape[0]
    out = np.zeros((T, idx.shape[1]), dtype=np.float32)
    for s, seg in enumerate(segments):
        b, e = clamp(seg, T)
        if e > b:
            out[b:e] = v[b:e][:, idx[s]]
    return out
