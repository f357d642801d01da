"""numpy restatement of the per-feature uniform example sample (include/msae.h, msae_feature_stats_update_sampled /
msae_feature_sample_merge): the priority hash, the bottom-n-by-priority table and its merge, written from the rules and
not from the kernels.  Candidates come from feature_stats_ref.candidates."""
from __future__ import annotations

import numpy as np

GOLDEN_GAMMA = np.uint64(0x9E3779B97F4A7C15)

# prio(seed, f, id) pinned in include/msae.h
PINNED = (((22, 0, 0), 0xbe5264ad2aa020f4), ((1, 5, 7), 0xb2e6c178b81a5c56), ((22, 7, 2 ** 33), 0x27044a0765e2616f),
          ((22, 131071, 12345), 0x45984866898b23bf), ((2 ** 64 - 1, 262143, 2 ** 40 + 3), 0xaf8ee0a530541d25))


def mix64(z):
    """The splitmix64 finaliser, mod 2^64, elementwise."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def prio(seed, f, ids):
    """prio(seed, f, id) = mix64(mix64(seed + 0x9E3779B97F4A7C15 * (f + 1)) ^ (uint64)id), elementwise (broadcast) over seed, f and ids."""
    f = np.asarray(f, np.int64).astype(np.uint64)
    ids = np.asarray(ids, np.int64).astype(np.uint64)          # two's complement, as the C cast
    seed = np.asarray(seed % 2 ** 64 if isinstance(seed, int) else seed, np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(seed + GOLDEN_GAMMA * (f + np.uint64(1)))
    return mix64(h ^ ids)


def sample_tables(cf, cv, ci, N, n, seed):
    """(seg_count [N] int64, smp_val [N, n] f32, smp_id [N, n] int64) from all candidates (feature, pooled, id): per feature
    the n candidates of smallest priority, priority ascending then id ascending; free slots (0, -1)."""
    cf, cv, ci = np.asarray(cf, np.int64), np.asarray(cv, np.float32), np.asarray(ci, np.int64)
    seg = np.bincount(cf, minlength=N).astype(np.int64)
    sv = np.zeros((N, n), np.float32)
    si = np.full((N, n), -1, np.int64)
    if len(cf):
        p = prio(seed, cf, ci)
        order = np.lexsort((ci, p, cf))
        cf, cv, ci = cf[order], cv[order], ci[order]
        first = np.ones(len(cf), bool)
        first[1:] = cf[1:] != cf[:-1]
        rank = np.arange(len(cf)) - np.flatnonzero(first)[np.cumsum(first) - 1]
        m = rank < n
        sv[cf[m], rank[m]] = cv[m]
        si[cf[m], rank[m]] = ci[m]
    return seg, sv, si


def merge_samples(a, b, n, seed):
    """dst += src restated: counts add, tables merge in the same (priority, id) order."""
    (ca, va, ia), (cb, vb, ib) = a, b
    N = len(ca)
    fa = np.repeat(np.arange(N), n)
    ids = np.concatenate([ia.reshape(-1), ib.reshape(-1)])
    m = ids >= 0
    _, sv, si = sample_tables(np.concatenate([fa, fa])[m], np.concatenate([va.reshape(-1), vb.reshape(-1)])[m], ids[m],
                              N, n, seed)
    return ca + cb, sv, si
