"""numpy restatement of the exact encode over a feature subset (include/msae.h, "exact encode over a feature subset") on the
C oracle: the listed rows of W_enc and entries of b_enc go through oracle.pre_acts -- the same ascending-k fmaf chain per
(token, feature), whatever the other rows -- and oracle.topk ranks the resulting rows by value, then position."""
import numpy as np

from oracle import oracle


def clamp_features(features, N: int) -> np.ndarray:
    """An entry outside [0, N) is clamped into it (the kernel never faults on one)."""
    return np.clip(np.asarray(features, dtype=np.int64), 0, N - 1).astype(np.int32)


def pre_acts_features(x, W_enc, b_enc, b_dec, features, relu: bool = True) -> np.ndarray:
    """-> [T, M] f32: column m is feature features[m] (clamped) of oracle.pre_acts(x, W_enc, b_enc, b_dec)."""
    W_enc = np.asarray(W_enc, dtype=np.float32)
    f = clamp_features(features, W_enc.shape[0])
    if f.size == 0:
        return np.empty((np.asarray(x).shape[0], 0), dtype=np.float32)
    return oracle.pre_acts(x, W_enc[f], None if b_enc is None else np.asarray(b_enc, dtype=np.float32)[f], b_dec, relu=relu)


def topk_within(x, W_enc, b_enc, b_dec, features, k: int):
    """-> (vals [T, k] f32, idx [T, k] int64 global feature ids): value descending, ties by ascending position in the list."""
    f = clamp_features(features, np.asarray(W_enc).shape[0])
    vals, pos = oracle.topk(pre_acts_features(x, W_enc, b_enc, b_dec, f), k)
    return vals, f[pos].astype(np.int64)


def topk_map(latents, col_map, k: int):
    """msae_topk_map_i64_f32: oracle.topk of the rows, positions sent through col_map."""
    vals, pos = oracle.topk(latents, k)
    return vals, np.asarray(col_map, dtype=np.int64)[pos]
