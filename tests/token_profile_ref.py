"""numpy restatement of the token profiles (include/msae.h, msae_token_profile_*), sharing no code with
the package: the keep and count rules, the offsets and the vocabulary check by explicit loops over rows, positions, slots and
offsets; q(v) with Python fractions; the masses as Python integers reduced mod 2^64; the three metrics of the top-token lists
with Python floats (IEEE doubles; int -> float is correctly rounded) rounded once to float32, ordered by (score descending,
token ascending)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

Q_ONE = 1 << 20
Q_MAX = 1 << 60
MASK = (1 << 64) - 1


def q_of(v) -> int:
    """q(v) for one float32 v > 0: v * 2^20 as an exact fraction, rounded half to even; 2^60 from 2^40 on, +inf included."""
    v = float(np.float32(v))
    if v == float("inf") or Fraction(v) >= Fraction(2) ** 40:
        return Q_MAX
    x = Fraction(v) * Q_ONE
    fl = x.numerator // x.denominator
    rem = x - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl


def new_state(O: int, F: int, V: int) -> dict:
    return dict(counts=np.zeros((O, F, V), np.int32), mass=np.zeros((O, F, V), np.uint64), tok_count=np.zeros((O, V), np.int64),
                n_rows=0, n_positions=0)


def update(state: dict, vals, idx, ids, N: int, queries, offsets, thresh=1e-5) -> dict:
    """One `[B, S, k]` batch with its `[B, S]` token ids into a copy of `state`."""
    vals, idx, ids = np.asarray(vals, np.float32), np.asarray(idx, np.int64), np.asarray(ids, np.int64)
    B, S, k = vals.shape
    assert ids.shape == (B, S)
    st = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in state.items()}
    counts, tok = st["counts"], st["tok_count"]
    V = counts.shape[2]
    slot = {int(q): i for i, q in enumerate(queries)}
    mass = {}
    for b in range(B):
        for s in range(S):
            for a, o in enumerate(offsets):
                if 0 <= s + o < S and 0 <= int(ids[b, s + o]) < V:
                    tok[a, int(ids[b, s + o])] += 1
            for j in range(k):
                v, f = vals[b, s, j], int(idx[b, s, j])
                if not (abs(v) > np.float32(thresh)) or not (0 <= f < N):      # a NaN fails the comparison
                    continue
                if not v > 0 or f not in slot:
                    continue
                for a, o in enumerate(offsets):
                    if not 0 <= s + o < S:
                        continue
                    t = int(ids[b, s + o])
                    if not 0 <= t < V:
                        continue
                    counts[a, slot[f], t] += 1
                    mass[a, slot[f], t] = mass.get((a, slot[f], t), 0) + q_of(v)
    for cell, m in mass.items():
        st["mass"][cell] = np.uint64((int(st["mass"][cell]) + m) & MASK)
    st["n_rows"] += B
    st["n_positions"] += B * S
    return st


def run(calls, N: int, queries, V: int, offsets, thresh=1e-5) -> dict:
    """calls: [(vals [B, S, k], idx, ids [B, S])] -> the state after all of them."""
    st = new_state(len(offsets), len(queries), V)
    for vals, idx, ids in calls:
        st = update(st, vals, idx, ids, N, queries, offsets, thresh)
    return st


def score(metric: str, c: int, tc: int, mass: int) -> np.float32:
    """One fixed operation sequence per metric; `mass` is the unsigned sum."""
    if metric == "count":
        return np.float32(c)
    if metric == "precision":
        return np.float32(np.float64(c) / np.float64(tc)) if tc != 0 else np.float32(np.inf)
    return np.float32(float(mass) / float(c) * 2.0 ** -20)


def top_tokens(counts, mass, tok_count, m: int, metric: str, min_count: int):
    """(values [F, m] f32, tokens [F, m] int32, totals [F] int64) of one offset plane: counts [F, V], mass [F, V] uint64 (or
    None), tok_count [V]."""
    counts = np.asarray(counts)
    F, V = counts.shape
    val, tok = np.zeros((F, m), np.float32), np.full((F, m), -1, np.int32)
    tot = np.zeros(F, np.int64)
    for i in range(F):
        cands = []
        for t in range(V):
            c = int(counts[i, t])
            tot[i] += c
            if c >= min_count:
                sc = score(metric, c, int(tok_count[t]), 0 if mass is None else int(np.asarray(mass)[i, t].astype(np.uint64)))
                cands.append((-float(sc), t, sc))
        cands.sort(key=lambda x: (x[0], x[1]))
        for r, (_, t, sc) in enumerate(cands[:m]):
            val[i, r], tok[i, r] = sc, t
    return val, tok, tot
