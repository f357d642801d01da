"""Shared by tests/test_encode_routes_host.py, tests/test_gpu_encode_shape_lattice.py and tests/small_dot4_runner.py: the route
table of the fused encoder's small-T path, its host-side witness, and the seeded generators of the lattice tests.

The witness.  msae_encode_topk_ws_bytes is host code that rebuilds the plan at every call, and the small-T plan carves regions
no other plan has (the two activation planes, the survivor keys, the workgroups' bounds ...).  MSAE_NO_SMALL_PATH=1 -- read at
every call -- takes the small path out of the plan and changes nothing else, so

    ws_bytes(T, d, N, k) != ws_bytes(T, d, N, k) under MSAE_NO_SMALL_PATH=1   <=>   the plan is the small path.
"""
import numpy as np
import torch

SMALL_T_MAX, SMALL_K_MAX, SMALL_N_MAX = 16, 64, 262144


def small_expected(T, d, N, k):
    """The route table (csrc/encode_small.h, small_kernel_for): the small path has kernels for d_in = 1024, 2048, 4096 at every
    T <= 16 and for d_in = 8192 at T <= 2; every other batch of <= 256 tokens at d_in % 1024 == 0 takes the weight-stream
    kernel (csrc/gemm_skinny.h)."""
    return T <= SMALL_T_MAX and k <= SMALL_K_MAX and N <= SMALL_N_MAX and (d in (1024, 2048, 4096) or (d == 8192 and T <= 2))


def plan_is_small(lib, monkeypatch, T, d, N, k):
    """-> (the plan is the small path, bytes with the small path allowed, bytes with it switched off).  Leaves the switch unset."""
    monkeypatch.delenv("MSAE_NO_SMALL_PATH", raising=False)
    with_small = lib.msae_encode_topk_ws_bytes(T, d, N, k, None)
    monkeypatch.setenv("MSAE_NO_SMALL_PATH", "1")
    without = lib.msae_encode_topk_ws_bytes(T, d, N, k, None)
    monkeypatch.delenv("MSAE_NO_SMALL_PATH", raising=False)
    return with_small != without, with_small, without


# ---- seeded inputs (the generators of tests/test_gpu_parity.py: unit-scale rows, two massive-activation dims) ----------------
def rand_sae(dev, d, N, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    W_enc = torch.randn(N, d, generator=g, device=dev) / d ** 0.5
    b_enc = torch.randn(N, generator=g, device=dev) * 0.05
    b_dec = torch.randn(d, generator=g, device=dev) * 0.1
    return W_enc, b_enc, b_dec


def rand_x(dev, T, d, seed, dtype=torch.bfloat16):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(T, d, generator=g, device=dev)
    x[:, 13 % d] *= 20.0
    x[:, 990 % d] *= 20.0
    return x.to(dtype)


def np32(t):
    return np.ascontiguousarray(t.detach().float().cpu().numpy())


def same_bits(a, b):
    """Per-row equality of two [T, k] arrays of one dtype by BIT pattern (NaN == NaN), -0.0 == +0.0 accepted for floats (the
    oracle skips zero activations, the kernels select them)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        eq = (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))
    else:
        eq = a == b
    return eq.all(-1)
