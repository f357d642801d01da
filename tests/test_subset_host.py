"""Host-side checks of the exact encode over a feature subset: the numpy restatement the GPU tests
compare against (tests/subset_ref.py) is itself pinned to the dense oracle, the chunk rule of ops.topk_within is checked as
arithmetic, and the argument errors of the public interface are raised before any device is touched."""
import numpy as np
import pytest
import torch

import subset_ref
from oracle import oracle


def _problem(T=9, d=70, N=512, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, d)).astype(np.float32)
    W = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    bd = (0.1 * rng.standard_normal(d)).astype(np.float32)
    return x, W, b, bd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _canonical_topk(lat, k):
    """Value descending, index ascending, in float64 with -0 folded onto +0 (a stable sort of -value)."""
    key = lat.astype(np.float64)
    key = np.where(key == 0, 0.0, key)
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(lat, order, 1), order.astype(np.int64)


def test_restated_columns_equal_the_dense_oracle_bit_for_bit():
    x, W, b, bd = _problem()
    f = np.array([500, 3, 3, 77, 0, 511, 200, 3, 499, 77], dtype=np.int32)       # unsorted, with repeats
    dense = oracle.pre_acts(x, W, b, bd)
    got = subset_ref.pre_acts_features(x, W, b, bd, f)
    assert got.shape == (9, f.size)
    assert np.array_equal(_bits(got), _bits(dense[:, f]))
    raw = oracle.pre_acts(x, W, b, bd, relu=False)
    assert np.array_equal(_bits(subset_ref.pre_acts_features(x, W, b, bd, f, relu=False)), _bits(raw[:, f]))
    assert (raw[:, f] < 0).any()                                                  # the ReLU rule was exercised
    # out-of-range entries are clamped first
    g = np.array([-1, 517, 5], dtype=np.int32)
    assert np.array_equal(_bits(subset_ref.pre_acts_features(x, W, b, bd, g)), _bits(dense[:, [0, 511, 5]]))
    assert subset_ref.pre_acts_features(x, W, b, bd, []).shape == (9, 0)


@pytest.mark.parametrize("n_dead", [1, 12, 40], ids=["one", "exactly_k_aux", "more_than_k_aux"])
def test_restated_topk_within_equals_the_masked_dense_topk(n_dead):
    k_aux = min(12, n_dead)
    x, W, b, bd = _problem(seed=1)
    N = W.shape[0]
    dead = np.sort(np.random.default_rng(2).permutation(N)[:n_dead]).astype(np.int32)
    b = b.copy()
    b[dead] = -np.abs(b[dead]) - 1e-3                 # dead-like: many latents at 0 ...
    x[4] = bd                                         # ... and one row whose dead latents are ALL 0 (x - b_dec = 0, b_enc < 0)
    dense = oracle.pre_acts(x, W, b, bd)
    assert float(np.abs(dense[4, dead]).max()) == 0.0
    masked = np.where(np.isin(np.arange(N), dead)[None], dense, -np.inf).astype(np.float32)
    rv, ri = _canonical_topk(masked, k_aux)
    gv, gi = subset_ref.topk_within(x, W, b, bd, dead, k_aux)
    assert gi.dtype == np.int64 and np.array_equal(gi, ri)
    assert np.array_equal(_bits(gv), _bits(rv))
    assert np.array_equal(gi[4], dead[:k_aux])        # ties at 0 fall to the lowest feature ids
    assert np.isin(gi, dead).all()


def test_rows_per_chunk_rule():
    from msae.ops import rows_per_chunk

    assert rows_per_chunk(100, 10) == 100                              # T below 128: one chunk of T rows
    assert rows_per_chunk(127, 65536, 1 << 20) == 127
    assert rows_per_chunk(1000, 4096, 1 << 20) == 128                  # one 128-row chunk is 2 MiB > the cap: still 128
    assert rows_per_chunk(1000, 1000, 256 * 1000 * 4) == 256           # exact multiple
    assert rows_per_chunk(1000, 1000, 256 * 1000 * 4 - 1) == 128
    assert rows_per_chunk(1000, 997, 256 * 1000 * 4) == 256            # ld = 1000: M rounded up to 4
    assert rows_per_chunk(200, 1000, 256 * 1000 * 4) == 200            # at most T
    # the default cap (256 MiB): M = 6554 -> ld = 6556, 268435456 // 26224 = 10236 -> 79 * 128
    assert rows_per_chunk(100000, 6554) == 10112
    assert rows_per_chunk(8192, 6554) == 8192
    assert rows_per_chunk(8192, 65536) == 1024                         # 256 MiB / 256 KiB per row, exactly
    for T, M, cap in [(100000, 6554, 256 << 20), (8192, 65536, 256 << 20), (5000, 333, 1 << 22)]:
        r = rows_per_chunk(T, M, cap)
        ld = (M + 3) // 4 * 4
        assert r % 128 == 0 and r * ld * 4 <= cap < (r + 128) * ld * 4


def _cpu_sae():
    from msae import Sae, SaeConfig

    return Sae(64, SaeConfig(num_latents=256, k=4), device="cpu")


def test_pre_acts_features_validates_before_touching_a_device():
    sae = _cpu_sae()
    x = torch.zeros(3, 64)
    with torch.no_grad():
        for bad in ([0, 256], [-1], [5, 1000, 2]):
            with pytest.raises(ValueError, match="feature indices"):
                sae.pre_acts(x, features=bad)
        with pytest.raises(ValueError, match="1-d int tensor"):
            sae.pre_acts(x, features=torch.zeros(2, 2, dtype=torch.int64))
        with pytest.raises(ValueError, match="1-d int tensor"):
            sae.pre_acts(x, features=torch.zeros(2))
    # gradients: parameters of a fresh Sae require grad
    with pytest.raises(NotImplementedError, match="pre_acts"):
        sae.pre_acts(x, features=[1, 2])
    sae.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="pre_acts"):
        sae.pre_acts(x.clone().requires_grad_(True), features=[1, 2])
    with pytest.raises(ValueError, match="feature indices"):           # validation comes first
        sae.pre_acts(x.clone().requires_grad_(True), features=[256])


def test_auxk_path_values():
    from msae import ops
    from msae.train import SaeTrainStep

    sae = _cpu_sae()
    assert sae.auxk_path == "dense" and ops.AUXK_PATHS == ("dense", "subset")
    x = torch.zeros(3, 64)
    with pytest.raises(ValueError, match="auxk_path"):
        sae(x, None, auxk_path="sparse")
    sae.auxk_path = "fused"
    with pytest.raises(ValueError, match="auxk_path"):
        sae(x)
    sae.auxk_path = "dense"
    with pytest.raises(ValueError, match="auxk_path"):
        ops.sparse_encode(x, sae.encoder.weight, sae.encoder.bias, sae.b_dec, 4, auxk_path="other")
    with pytest.raises(ValueError, match="auxk_path"):
        SaeTrainStep(sae, auxk_path="other")
    assert SaeTrainStep(sae).auxk_path == "dense"
    assert SaeTrainStep(sae, auxk_path="subset").auxk_path == "subset"


def test_topk_within_rejects_k_outside_its_range():
    from msae import ops

    args = (torch.zeros(2, 8), torch.zeros(16, 8), None, None, torch.zeros(4, dtype=torch.int32))
    for k in (0, 5, -1):
        with pytest.raises(ValueError, match="topk_within"):
            ops.topk_within(*args, k)
    with pytest.raises(ValueError, match="topk_within"):               # the LDS-resident selection's limit
        ops.topk_within(torch.zeros(2, 8), torch.zeros(16, 8), None, None, torch.zeros(20000, dtype=torch.int32), 16385)
    with pytest.raises(RuntimeError, match="MI355X"):                  # a valid k: refused for the CPU tensors instead
        ops.topk_within(*args, 4)


def test_prototypes_carry_the_new_symbols():
    from msae import _hip

    assert _hip.ABI_VERSION == 4
    assert len(_hip.PROTOTYPES["msae_pre_acts_features_f32"][1]) == 14
    assert len(_hip.PROTOTYPES["msae_topk_map_i64_f32"][1]) == 9
    lib = _hip.load()
    assert hasattr(lib, "msae_pre_acts_features_f32") and hasattr(lib, "msae_topk_map_i64_f32")
    # pure host-side argument checks (no launch): an empty list or batch is a no-op, a short pitch is refused
    assert lib.msae_pre_acts_features_f32(None, 0, None, None, None, None, 0, 5, 8, 16, 1, None, 0, None) == 0
    assert lib.msae_pre_acts_features_f32(None, 0, None, None, None, None, 3, 0, 8, 16, 1, None, 4, None) == 0
    assert lib.msae_pre_acts_features_f32(None, 0, None, None, None, None, 5, 5, 8, 16, 1, None, 4, None) != 0
