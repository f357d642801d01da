"""CPU: which batches the fused encoder plans on its small-T path (csrc/encode_small.h), read off the workspace helper -- the
witness of tests/encode_routes.py, no GPU needed.

The plan must be small exactly for the shapes run_small (csrc/encode_fused.hip) has kernels for: a shape that is planned small
without a kernel makes the encode return MSAE_ENOTIMPL after its first launch (d_in = 3072, 5120, 6144, 7168, and d_in = 8192
with 3 or 4 tokens, did: Sae.encode raised at the steering decode step).  tests/test_gpu_encode_shape_lattice.py runs the same
table on the GPU.
"""
import itertools

import pytest

from encode_routes import plan_is_small, small_expected

TS = tuple(range(1, 18))
DS = tuple(range(1024, 9216 + 1, 1024))
KS = (1, 64, 65)
NS = (8192, 24576, 262144, 270336)


@pytest.fixture(scope="module")
def lib():
    from msae import _hip

    return _hip.load()


@pytest.mark.parametrize("d", DS)
def test_small_path_is_planned_exactly_where_it_has_kernels(lib, monkeypatch, d):
    for name in ("MSAE_COARSE", "MSAE_FM", "MSAE_LPR"):       # (the int8 pass and the default re-score routes)
        monkeypatch.delenv(name, raising=False)
    wrong, zero = [], []
    for T, k, N in itertools.product(TS, KS, NS):
        small, a, b = plan_is_small(lib, monkeypatch, T, d, N, k)
        if a == 0 or b == 0:
            zero.append((T, d, N, k, a, b))
        if small != small_expected(T, d, N, k):
            wrong.append((T, d, N, k, "small" if small else "not small"))
        assert a >= b, (T, d, N, k, a, b)                     # (the small-path plan only ADDS regions)
    assert not zero, f"the helper returns 0 at {len(zero)} shapes, first {zero[:4]}"
    assert not wrong, f"{len(wrong)} shapes (T, d, N, k) off the route table, first {wrong[:6]}"


def test_the_witness_sees_both_routes(lib, monkeypatch):
    """The witness is not vacuous: it says small at the steering decode step and not small at 17 tokens."""
    assert plan_is_small(lib, monkeypatch, 1, 1024, 8192, 32)[0]
    assert not plan_is_small(lib, monkeypatch, 17, 1024, 8192, 32)[0]
