"""The int8 candidate GEMM's accumulator layout (csrc/gemm_mfma.h, GemmCfg bit 7 / tuning.h MSAE_GEMM_MF): the outlier k-tile
at every fill the 16x16x64 re-layout distinguishes, through the tile-major MFMA pass and its partial last row tile.

  n_out 0            no outlier k-tile work (accumulators only take -E)
  n_out 1, 31, 32    the compact outlier image (32 B per row: lanes 32-63 of a 16x16x64 fragment feed zeros)
  n_out 33 .. 128    the full outlier k-tile, ceil(n_out / 64) k-steps of 64 B (one or two)

Every record is audited by tests/test_gpu_candidate_audit.py's P1-P6 against the f64 pre-activations of every pair, P5 included:
the recorded coarse value is the restated integer product, so a lost, doubled or misplaced accumulator shows at once.
"""
from __future__ import annotations

import gc

import pytest
import torch

import hostile
from test_gpu_candidate_audit import N8, audit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_after():
    yield
    from msae import ops

    ops.set_coarse_mode("default")
    ops.set_dither("default")
    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n_out", [0, 1, 31, 32, 33, 64, 65, 128])
def test_outlier_fill(dev, n_out):
    """T = 300: one full and one partial (44-row) tile of 256 tokens; n_out dims carry per-token multipliers 2 .. 252."""
    T, d = 300, 4096
    W, b, _ = hostile.weights("gauss", N8, d, dev, seed=40 + n_out)
    bd = torch.zeros(d, device=dev)
    g = torch.Generator(device=dev).manual_seed(50 + n_out)
    x = (torch.rand(T, d, generator=g, device=dev) * 2 - 1) * torch.exp(torch.randn(T, 1, generator=g, device=dev))
    if n_out:
        odim = torch.randperm(d, generator=g, device=dev)[:n_out]
        inmax = x[:, [i for i in range(d) if i not in set(odim.tolist())]].abs().max(dim=1).values
        ms = torch.randint(2, 253, (T,), generator=g, device=dev).float()
        sign = torch.where(torch.rand(T, n_out, generator=g, device=dev) < 0.5, -1.0, 1.0)
        mag = ms[:, None] - 1 + torch.rand(T, n_out, generator=g, device=dev) * 0.9
        mag[:, 0] = ms - 0.05
        x[:, odim] = sign * mag * inmax[:, None]
    R = audit(dev, x, W, b, bd, 32, 256, mode="sd", label=f"n_out {n_out}")
    assert int(R["restate"]["out"].sum()) == n_out
    assert R["stats"]["pairs"] > 0
