"""numpy restatement of the position profiles (include/msae.h, msae_pos_profile_*), sharing no code with
the package: the bin of a position by a table lookup, the keep and count rules by explicit loops over rows, positions and
slots (`np.add.at` for the wide cases: `wide=True`), q(v) with Python integers and fractions, the masses as Python integers
reduced mod 2^64, and the summary's rate comparison with Python big integers.

`mutant=` switches ONE deliberate mistake on, for the tests that show that the cases can tell the restatement from a wrong
one: "lookup" (the table is read one position late), "ge" (v >= 0 counts instead of v > 0), "count_peak" (the peak is the
bin with the most fires, not the highest rate)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

Q_ONE = 1 << 20
Q_MAX = 1 << 60
MASK = (1 << 64) - 1


def q_of(v) -> int:
    """q(v) for one float32 v > 0: v * 2^20 as an exact fraction, rounded half to even; 2^60 from 2^40 on, +inf included."""
    v = float(np.float32(v))
    if v == float("inf") or v >= 2.0 ** 40:
        return Q_MAX
    return int(round(Fraction(v) * Q_ONE))           # round() of a Fraction rounds half to even


def q_many(v) -> np.ndarray:
    """q of every element of `v` (float32, > 0), uint64: the f64 product v * 2^20 is exact (a power of two), and np.rint rounds
    half to even.  test_pos_profile_host.py holds it to `q_of`."""
    x = np.asarray(v, np.float32).astype(np.float64) * float(Q_ONE)
    big = x >= float(Q_MAX)
    return np.where(big, np.uint64(Q_MAX), np.rint(np.where(big, 0.0, x)).astype(np.uint64))


def bin_of(s: int, table, tail_bin: int, mutant=None) -> int:
    if mutant == "lookup":
        s += 1
    return int(table[s]) if s < len(table) else int(tail_bin)


def new_state(N: int, P: int) -> dict:
    return dict(count=np.zeros((N, P), np.int32), mass=np.zeros((N, P), np.uint64), bin_positions=np.zeros(P, np.int64),
                n_rows=0, n_positions=0)


def update(state: dict, vals, idx, N: int, table, tail_bin: int, thresh=1e-5, wide=False, mutant=None) -> dict:
    """One `[B, S, k]` batch into a copy of `state`."""
    vals, idx = np.asarray(vals, np.float32), np.asarray(idx, np.int64)
    table = np.asarray(table, np.int64)
    B, S, k = vals.shape
    st = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in state.items()}
    count, P = st["count"], st["count"].shape[1]
    bins = np.array([bin_of(s, table, tail_bin, mutant) for s in range(S)], np.int64)
    for s in range(S):
        if bins[s] >= 0:
            st["bin_positions"][bins[s]] += B
    st["n_rows"] += B
    st["n_positions"] += B * S
    if wide:
        with np.errstate(invalid="ignore"):
            on = (np.abs(vals) > np.float32(thresh)) & (idx >= 0) & (idx < N) & ((vals >= 0) if mutant == "ge" else (vals > 0))
        on &= (bins >= 0)[None, :, None]
        b = np.broadcast_to(bins[None, :, None], vals.shape)[on]
        np.add.at(count, (idx[on], b), 1)
        np.add.at(st["mass"], (idx[on], b), q_many(vals[on]))          # uint64 adds wrap: mod 2^64
        return st
    mass = {}
    for r in range(B):
        for s in range(S):
            if bins[s] < 0:
                continue
            for j in range(k):
                v, f = vals[r, s, j], int(idx[r, s, j])
                if not (abs(v) > np.float32(thresh)) or not (0 <= f < N):      # a NaN fails the comparison
                    continue
                if not ((v >= 0) if mutant == "ge" else (v > 0)):
                    continue
                count[f, bins[s]] += 1
                mass[f, bins[s]] = mass.get((f, bins[s]), 0) + q_of(v)
    for (f, b), m in mass.items():
        st["mass"][f, b] = np.uint64((int(st["mass"][f, b]) + m) & MASK)
    return st


def run(calls, N: int, table, tail_bin: int, P: int, thresh=1e-5, wide=False, mutant=None) -> dict:
    """calls: [(vals [B, S, k], idx)] -> the state after all of them."""
    st = new_state(N, P)
    for vals, idx in calls:
        st = update(st, vals, idx, N, table, tail_bin, thresh, wide, mutant)
    return st


def summary(count, bin_positions, mutant=None):
    """(fired int64 [N], peak int32 [N, 2]): the row total, and (bin, count in it) of the highest rate count / positions among
    the bins with positions -- compared as Python integers by cross-multiplication, ties to the lowest bin, (-1, 0) when
    nothing fired in such a bin."""
    count = np.asarray(count)
    N, P = count.shape
    fired, peak = np.zeros(N, np.int64), np.zeros((N, 2), np.int32)
    bp = [int(x) for x in bin_positions]
    for f in range(N):
        row = [int(c) for c in count[f]]
        fired[f] = sum(row)
        best = (-1, 0, 1)
        for b in range(P):
            if bp[b] <= 0:
                continue
            if mutant == "count_peak":
                better = row[b] > best[1]
            else:
                better = row[b] * best[2] > best[1] * bp[b]
            if better:
                best = (b, row[b], bp[b])
        peak[f] = best[:2]
    return fired, peak
