"""GPU: ops.rows_topk / ops.row_inv_norms / Sae.neighbors / Sae.top_logits (csrc/neighbors.hip) against the numpy
restatement of their numerics contract (tests/neighbors_ref.py: oracle dots, two f32 multiplies, canonical ranking), bit for
bit, and against the reference's own results (tests/golden/g15_neighbors.npz) within the derived bound."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbors_ref as nref
import probe_ref
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_after():
    yield
    from msae import ops

    ops.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


def _np(t):
    return t.detach().cpu().numpy()


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero((a.view(np.uint32) if a.dtype == np.float32 else a).ravel()
                         != (b.view(np.uint32) if b.dtype == np.float32 else b).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {np.unravel_index(bad[0], a.shape)}"


def _weights(N, d, seed):
    """Clustered rows with free norms: neighbours are meaningful and near-ties occur."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((32, d)).astype(np.float32)
    W = centers[rng.integers(0, 32, N)] * np.float32(0.7) + rng.standard_normal((N, d)).astype(np.float32)
    return np.ascontiguousarray(W * rng.uniform(0.5, 2.0, (N, 1)).astype(np.float32), dtype=np.float32)


_DENSE = {}


def _dense(d, N):
    """(W, oracle dots W W^T [N, N], inv) of the grid's (d, N), computed once and left unchanged."""
    if (d, N) not in _DENSE:
        W = _weights(N, d, seed=1000 + d + N)
        _DENSE[(d, N)] = (W, nref.dots(W, W), nref.inv_norms(W))
    return _DENSE[(d, N)]


def _strips(N):
    return -(-N // 128)


# ---- grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 130, "all"])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("d,N", [(64, 1000), (100, 1000), (768, 1000), (64, 4096), (100, 4096), (768, 4096)])
def test_grid(dev, d, N, k, M):
    from msae import ops

    W, dot, inv = _dense(d, N)
    rng = np.random.default_rng(d * 7 + N + k)
    if M == "all":
        rows = None
    else:
        rows = rng.integers(0, N, M)                          # unsorted, with repeats at M = 130
        if M == 130:
            rows[5] = rows[77]
    qi = np.arange(N) if rows is None else rows
    Wt, invt = torch.from_numpy(W).to(dev), torch.from_numpy(inv).to(dev)
    rt = None if rows is None else torch.from_numpy(rows.astype(np.int32)).to(dev)
    ex = torch.from_numpy(qi.astype(np.int32)).to(dev)
    # scales and exclusion on
    v, i = ops.rows_topk(Wt, Wt, k, q_rows=rt, q_scale=torch.from_numpy(inv[qi]).to(dev), k_scale=invt, exclude=ex)
    rv, ri = nref.rank(nref.values(dot[qi], inv[qi], inv), k, qi)
    _eq(_np(i), ri, "indices (scales, exclusion)")
    _eq(_np(v), rv, "values (scales, exclusion)")
    # both off; the query matrix as a view 4 bytes off alignment -> the tile's generic staging path
    flat = torch.empty(N * d + 1, dtype=torch.float32, device=dev)
    Qoff = flat[1:].view(N, d)
    Qoff.copy_(Wt)
    assert Qoff.data_ptr() % 16 == 4
    v, i = ops.rows_topk(Qoff, Wt, k, q_rows=rt)
    rv, ri = nref.rank(dot[qi], k)
    _eq(_np(i), ri, "indices (plain, offset Q)")
    _eq(_np(v), rv, "values (plain, offset Q)")


def test_q_rows_out_of_range_are_clamped(dev):
    from msae import ops

    W, dot, inv = _dense(64, 1000)
    rows = np.array([-5, 0, 999, 1000, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)
    Wt = torch.from_numpy(W).to(dev)
    v, i = ops.rows_topk(Wt, Wt, 10, q_rows=torch.from_numpy(rows.astype(np.int32)).to(dev))
    rv, ri = nref.rank(dot[np.clip(rows, 0, 999)], 10)
    _eq(_np(i), ri, "indices")
    _eq(_np(v), rv, "values")


# ---- chunk invariance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 64])
def test_chunk_invariance(dev, k):
    from msae import ops

    d, N = 64, 4096
    W, dot, inv = _dense(d, N)
    rows = np.random.default_rng(3).integers(0, N, 130)
    Wt, invt = torch.from_numpy(W).to(dev), torch.from_numpy(inv).to(dev)
    rt = torch.from_numpy(rows.astype(np.int32)).to(dev)
    qs = torch.from_numpy(inv[rows]).to(dev)
    outs = [ops.rows_topk(Wt, Wt, k, q_rows=rt, q_scale=qs, k_scale=invt, exclude=rt, chunks=c)
            for c in (1, 3, _strips(N), 0)]
    rv, ri = nref.rank(nref.values(dot[rows], inv[rows], inv), k, rows)
    for (v, i), c in zip(outs, (1, 3, _strips(N), 0)):
        _eq(_np(i), ri, f"indices, chunks={c}")
        _eq(_np(v), rv, f"values, chunks={c}")
    # one query alone == the same query inside the batch
    for c in (1, 3):
        v1, i1 = ops.rows_topk(Wt, Wt, k, q_rows=rt[17:18], q_scale=qs[17:18], k_scale=invt, exclude=rt[17:18], chunks=c)
        _eq(_np(i1), ri[17:18], f"alone, chunks={c}")
        _eq(_np(v1), rv[17:18], f"alone values, chunks={c}")


# ---- planted ties -------------------------------------------------------------------------------------------------------
def test_planted_ties(dev):
    """Duplicated decoder rows: equal cosines across a strip boundary (127 / 128), a chunk boundary (3 chunks of 1000 keys'
    8 strips: strips 2 | 3 -> n = 383 / 384) and the last partial strip (n = 990); ties rank by ascending index."""
    from msae import Sae, SaeConfig

    d, N, k = 64, 1000, 10
    W = _weights(N, d, seed=77).copy()
    for a, b in ((127, 128), (383, 384), (20, 990), (127, 600)):
        W[b] = W[a]
    W[385] = W[383] * np.float32(2.0)                          # same direction, other norm: a tie up to the scales' rounding
    sae = Sae(d, SaeConfig(num_latents=N, k=8), device=dev)
    with torch.no_grad():
        sae.W_dec.copy_(torch.from_numpy(W))
    feats = [127, 128, 600, 383, 384, 20, 990, 5, 385]
    for excl in (True, False):                                 # a query whose twin is excluded (it is not: only ITSELF is) ...
        rv, ri = nref.neighbors(W, feats, k, exclude_self=excl)
        v, i = sae.neighbors(feats, k=k, exclude_self=excl)
        _eq(_np(i), ri, f"indices exclude_self={excl}")
        _eq(_np(v), rv, f"values exclude_self={excl}")
    # ... and through the op: query 127 with its twin 128 excluded, query 383 with nothing excluded
    from msae import ops

    inv = nref.inv_norms(W)
    Wt, invt = torch.from_numpy(W).to(dev), torch.from_numpy(inv).to(dev)
    rows = np.array([127, 383, 20])
    ex = np.array([128, -1, 990])
    for c in (1, 3, 8):
        v, i = ops.rows_topk(Wt, Wt, k, q_rows=torch.from_numpy(rows.astype(np.int32)).to(dev),
                             q_scale=torch.from_numpy(inv[rows]).to(dev), k_scale=invt,
                             exclude=torch.from_numpy(ex.astype(np.int32)).to(dev), chunks=c)
        rv, ri = nref.rows_topk(W, W, k, rows, inv[rows], inv, ex)
        _eq(_np(i), ri, f"twin excluded, chunks={c}")
        _eq(_np(v), rv, f"twin excluded values, chunks={c}")
        assert 128 not in _np(i)[0] and _np(i)[0][0] == 127 and list(_np(i)[1][:2]) == [383, 384]


# ---- hostile order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rising", [True, False])
def test_hostile_order(dev, rising):
    """Keys whose cosine to the query rises with n (every column beats the list: the insert runs hot) or falls with n."""
    from msae import ops

    d, N, k = 64, 4096, 64
    rng = np.random.default_rng(9)
    q = rng.standard_normal(d).astype(np.float32)
    u = rng.standard_normal(d).astype(np.float32)
    u -= q * np.float32(u @ q / (q @ q))
    t = np.linspace(-1.0, 1.0, N, dtype=np.float32)
    if not rising:
        t = t[::-1]
    K = (t[:, None] * q[None, :] + np.sqrt(1 - t * t)[:, None] * u[None, :] * np.float32(np.linalg.norm(q) / np.linalg.norm(u)))
    K = np.ascontiguousarray(K, dtype=np.float32)
    Q = np.stack([q, -q, q * np.float32(3.0)]).astype(np.float32)
    inv_k, inv_q = nref.inv_norms(K), nref.inv_norms(Q)
    dot = nref.dots(Q, K)
    cosv = nref.values(dot, inv_q, inv_k)
    assert np.mean(np.diff(cosv[0]) > 0) > 0.95 if rising else np.mean(np.diff(cosv[0]) < 0) > 0.95
    rv, ri = nref.rank(cosv, k)
    for c in (1, 4, 0):
        v, i = ops.rows_topk(torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev), k,
                             q_scale=torch.from_numpy(inv_q).to(dev), k_scale=torch.from_numpy(inv_k).to(dev), chunks=c)
        _eq(_np(i), ri, f"indices chunks={c}")
        _eq(_np(v), rv, f"values chunks={c}")


# ---- inverse norms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 100, 4096])
def test_inv_norms(dev, d):
    from msae import ops

    N = 777
    W = _weights(N, d, seed=d)
    W[13] = 0.0                                                # a zero row: the 1e-12 clamp
    W[14] *= np.float32(1e-20)
    Wt = torch.from_numpy(W).to(dev)
    a, b = _np(ops.row_inv_norms(Wt)), _np(ops.row_inv_norms(Wt))
    _eq(a, b, "two runs")
    ref64 = 1.0 / np.maximum(np.sqrt((W.astype(np.float64) ** 2).sum(axis=1)), 1e-12)
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(a.astype(np.float64) - ref64) <= ulp), float(np.max(np.abs(a - ref64) / ulp))
    assert a[13] == np.float32(1e12)


# ---- production width ---------------------------------------------------------------------------------------------------
def test_production_width(dev):
    """N = 131072, d = 4096, 130 selected features, k = 10 against a restatement built from torch.ops.msae.pre_acts on Q and
    on -Q with zero biases: relu(p) - relu(n) is the signed chain exactly, and that op is pinned to the oracle elsewhere."""
    from msae import ops

    d, N, M, k = 4096, 131072, 130, 10
    g = torch.Generator(device=dev).manual_seed(5)
    W = torch.randn(N, d, device=dev, generator=g)
    W.mul_(torch.rand(N, 1, device=dev, generator=g) + 0.5)
    rows = torch.randint(0, N, (M,), device=dev, generator=g, dtype=torch.int64)
    twin = (int(rows[3]) + 1) % N
    W[twin] = W[int(rows[3])]                                  # a planted twin at full width
    inv = ops.row_inv_norms(W)
    r32 = rows.to(torch.int32)
    v, i = ops.rows_topk(W, W, k, q_rows=r32, q_scale=inv[rows], k_scale=inv, exclude=r32)
    Q = W[rows].contiguous()
    zb, zd = torch.zeros(N, device=dev), torch.zeros(d, device=dev)
    dot = torch.ops.msae.pre_acts(Q, W, zb, zd) - torch.ops.msae.pre_acts(-Q, W, zb, zd)
    dense = _np((dot * inv[rows][:, None]) * inv[None, :])     # two separately rounded f32 multiplies
    del dot
    rv, ri = nref.rank(dense, k, _np(rows))
    _eq(_np(i), ri, "indices")
    _eq(_np(v), rv, "values")


# ---- the reference's own results ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g15():
    return dict(np.load(GOLDEN / "g15_neighbors.npz"))


def _g15_sae(dev, g):
    from msae import Sae, SaeConfig

    N, d = g["W_dec"].shape
    sae = Sae(d, SaeConfig(num_latents=N, k=8), device=dev)
    with torch.no_grad():
        sae.W_dec.copy_(torch.from_numpy(g["W_dec"]))
    return sae.eval().requires_grad_(False)


def test_g15_neighbors_and_get_neighbors(dev, g15):
    from msae.features import cos, get_neighbors

    g = g15
    sae, k, feats = _g15_sae(dev, g), int(g["k"]), g["features"].tolist()
    bound = nref.cos_bound(g["W_dec"].shape[1])
    v, i = sae.neighbors(feats, k=k, exclude_self=False)
    ok, compared, mism, left = nref.compare_with_reference(_np(v), _np(i), g["nb_values"], g["nb_indices"][:, :k], bound)
    print(f"neighbors vs reference: compared {compared}, mismatches {mism}, left out {left}")
    assert ok and mism == 0 and left < 0.01 * v.numel()
    nd, plf = get_neighbors({"model.layers.0": sae, "unused": sae}, {"model.layers.0": feats}, k=k)
    assert list(nd) == ["model.layers.0"] and sorted(nd["model.layers.0"]) == list(range(len(feats)))
    gi = np.array([nd["model.layers.0"][m]["indices"] for m in range(len(feats))])
    gv = np.array([nd["model.layers.0"][m]["values"] for m in range(len(feats))], dtype=np.float32)
    assert gi.shape == g["gn_indices"].shape
    ok, compared, mism, left = nref.compare_with_reference(gv, gi, g["nb_values"][:, 1:], g["gn_indices"], bound)
    assert ok and mism == 0 and left < 0.01 * gi.size
    assert np.max(np.abs(gv.astype(np.float64) - g["gn_values"])) <= bound
    if np.array_equal(_np(i), g["nb_indices"][:, :k]):
        assert plf["model.layers.0"] == g["gn_layer_features"].tolist()
    c = _np(cos(sae.W_dec, feats[:16]))
    assert c.shape == g["cos_head"].shape and np.max(np.abs(c.astype(np.float64) - g["cos_head"])) <= bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_g15_logits(dev, g15, dtype):
    """V = 300 (V % 128 != 0).  With a bf16 W_U the reference values are recomputed from the rounded matrix in f64."""
    from msae.features import logits

    g = g15
    sae, k, feats = _g15_sae(dev, g), int(g["k"]), g["features"].tolist()
    W_U = torch.from_numpy(g["W_U"]).to(dev, dtype)
    d = g["W_dec"].shape[1]
    Wu32 = _np(W_U.float())
    qn = np.linalg.norm(g["W_dec"][g["features"]].astype(np.float64), axis=1)[:, None]
    bound = nref.cos_bound(d) * qn * np.linalg.norm(Wu32.astype(np.float64), axis=1).max()
    v, i = sae.top_logits(W_U, feats, k=k)
    if dtype == torch.float32:
        ref_vals, ref_idx = g["lg_values"], g["lg_indices"]
    else:
        full = g["W_dec"][g["features"]].astype(np.float64) @ Wu32.astype(np.float64).T
        rvv, rii = probe_ref.topk(full.astype(np.float32), k + 1)
        ref_vals, ref_idx = np.take_along_axis(full, rii, axis=1), rii[:, :k]
    ok, compared, mism, left = nref.compare_with_reference(_np(v), _np(i), ref_vals, ref_idx, bound)
    print(f"logits {dtype}: compared {compared}, mismatches {mism}, left out {left}")
    assert ok and mism == 0 and left < 0.01 * v.numel()

    class Tok:
        def batch_decode(self, ids):
            return [f"t{int(t)}" for t in ids]

    class Rec:
        def __init__(self, f):
            self.feature = type("F", (), {"feature_index": f})()
            self.top_logits = None

    recs = [Rec(f) for f in feats[:5]]
    out = logits(recs, W_U, sae, k=k, tokenizer=Tok())
    assert [r.top_logits for r in recs] == out == [[f"t{t}" for t in row] for row in _np(i)[:5].tolist()]
    out2 = logits([Rec(f) for f in feats[:5]], W_U, sae.W_dec, k=k, tokenizer=Tok())
    assert out2 == out


# ---- memory, host syncs, launcher ---------------------------------------------------------------------------------------
def test_memory_all_features(dev):
    """All 32768 features at d = 768: the dense cosines would be 4 GiB; the call may take its outputs, the workspace the
    library reports and two N-float arrays (the inverse norms; the exclusion list takes the second one's place)."""
    from msae import Sae, SaeConfig, _hip

    N, d, k = 32768, 768, 10
    from msae import ops

    sae = Sae(d, SaeConfig(num_latents=N, k=8), device=dev).eval().requires_grad_(False)
    ops.release_workspaces()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # the bytes ASKED of the allocator (requested_bytes): allocated_bytes counts a reused cached block at the block's own
    # size, which depends on what earlier tests left in the allocator's segments
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_stats(dev)["requested_bytes.all.current"]
    v, i = sae.neighbors(None, k=k)
    torch.cuda.synchronize()
    peak = torch.cuda.memory_stats(dev)["requested_bytes.all.peak"] - base
    ws = _hip.load().msae_rows_topk_ws_bytes(N, N, k, 0)
    budget = v.numel() * 4 + i.numel() * 8 + ws + 2 * N * 4
    print(f"peak increase {peak} B, budget {budget} B (workspace {ws} B)")
    assert 0 < ws < 64 << 20 and peak <= budget
    assert i.dtype == torch.int64 and not bool((i == torch.arange(N, device=dev)[:, None]).any())


def test_no_host_sync(dev, g15):
    sae = _g15_sae(dev, g15)
    W_U = torch.from_numpy(g15["W_U"]).to(dev)
    feats = g15["features"].tolist()
    sae.neighbors(feats, k=10)                                 # (library load, kernel attributes)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = sae.neighbors(feats, k=10)
        b = sae.top_logits(W_U, feats, k=10)
        c = sae.neighbors(None, k=10)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert a[0].shape == (200, 10) and b[1].shape == (200, 10) and c[0].shape == (1000, 10)


def test_launcher(dev, g15, tmp_path):
    import json

    from safetensors import safe_open

    sae = _g15_sae(dev, g15)
    sae.save_to_disk(tmp_path / "ckpt")
    feats = g15["features"][:37].tolist()
    (tmp_path / "filter.json").write_text(json.dumps({"model.layers.0": feats}))
    env = dict(os.environ, PYTHONPATH=str(REPO / "multimodal-sae_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "nb.safetensors"
    subprocess.run([sys.executable, "-m", "msae.launch.features.neighbors", "--sae_path", str(tmp_path / "ckpt"),
                    "--features", str(tmp_path / "filter.json"), "--k", "7", "--out", str(out)],
                   check=True, env=env, timeout=300)
    v, i = sae.neighbors(feats, k=7)
    with safe_open(str(out), framework="pt") as f:
        assert f.metadata() == {"k": "7", "matrix": "decoder", "exclude_self": "True"}
        idx, val, ft = f.get_tensor("indices"), f.get_tensor("values"), f.get_tensor("features")
    assert idx.dtype == torch.int32 and ft.dtype == torch.int32 and ft.tolist() == feats
    _eq(idx.numpy().astype(np.int64), _np(i), "launcher indices")
    _eq(val.numpy(), _np(v), "launcher values")
