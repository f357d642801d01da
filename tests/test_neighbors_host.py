"""Host side of the neighbours / top-logits feature: the numpy restatement (tests/neighbors_ref.py) on hand-computed cases
and against the reference's own results (tests/golden/g15_neighbors.npz), the wrappers' argument errors, and the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import neighbors_ref as nref
from conftest import GOLDEN


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(GOLDEN / "g15_neighbors.npz"))


# 4 queries x 6 keys in d = 2, every product exact in f32
Q4 = np.array([[1, 0], [0, 2], [-1, 0], [0, 0]], dtype=np.float32)
K6 = np.array([[2, 0], [1, 0], [0, 1], [-3, 0], [4, 0], [0, 0]], dtype=np.float32)


def test_restatement_dots_and_ties():
    dot = nref.dots(Q4, K6)
    assert dot.tolist() == [[2, 1, 0, -3, 4, 0], [0, 0, 2, 0, 0, 0], [-2, -1, 0, 3, -4, 0], [0, 0, 0, 0, 0, 0]]
    v, i = nref.rank(dot, 3)
    assert i.tolist() == [[4, 0, 1], [2, 0, 1], [3, 2, 5], [0, 1, 2]]          # ties -> index ascending (+0 and -0 tie too)
    assert v.tolist() == [[4, 2, 1], [2, 0, 0], [3, 0, 0], [0, 0, 0]]
    assert not np.signbit(v).any()                                             # -0 is returned as +0


def test_restatement_exclusion_and_negative_cosines():
    inv_q, inv_k = nref.inv_norms(Q4), nref.inv_norms(K6)
    assert inv_q.tolist() == [1.0, 0.5, 1.0, np.float32(1e12)]                 # a zero row: the 1e-12 clamp
    assert inv_k[5] == np.float32(1e12) and inv_k[3] == np.float32(1.0 / 3.0)
    cosv = nref.values(nref.dots(Q4, K6), inv_q, inv_k)
    assert cosv[0].tolist() == [1, 1, 0, -1, 1, 0] and cosv[2].tolist() == [-1, -1, 0, 1, -1, 0]
    v, i = nref.rank(cosv, 5, exclude=[0, 2, -1, 7])
    assert i[0].tolist() == [1, 4, 2, 5, 3] and v[0].tolist() == [1, 1, 0, 0, -1]   # key 0 skipped; the negative one last
    assert i[1].tolist() == [0, 1, 3, 4, 5]                                    # its only nonzero column is the excluded one
    assert i[2].tolist() == [3, 2, 5, 0, 1] and v[2].tolist() == [1, 0, 0, -1, -1]
    assert i[3].tolist() == [0, 1, 2, 3, 4]                                    # exclusion outside [0, N): nothing skipped
    with pytest.raises(AssertionError):
        nref.rank(cosv, 6, exclude=[0, 0, 0, 0])                               # k > N - 1


def test_restatement_q_rows_and_self():
    W = np.array([[1, 0], [1, 1], [0, 1], [-1, 0]], dtype=np.float32)
    v, i = nref.neighbors(W, [2, 2, 0], 2)
    assert i.tolist() == [[1, 0], [1, 0], [1, 2]]
    v2, i2 = nref.neighbors(W, [2], 2, exclude_self=False)
    assert i2.tolist() == [[2, 1]] and v2[0, 0] == 1.0
    assert np.array_equal(nref.dots(W, W, [-3, 9]), nref.dots(W, W, [0, 3]))   # clamped like the kernel's


def test_restatement_matches_reference_fixture(g15):
    g = g15
    k, feats, d = int(g["k"]), g["features"], g["W_dec"].shape[1]
    bound = nref.cos_bound(d)
    v, i = nref.neighbors(g["W_dec"], feats, k, exclude_self=False)
    ok, compared, mism, left = nref.compare_with_reference(v, i, g["nb_values"], g["nb_indices"][:, :k], bound)
    assert ok and mism == 0 and left < 0.01 * v.size, (ok, compared, mism, left)
    cosv = nref.values(nref.dots(g["W_dec"], g["W_dec"], feats[:16]), nref.inv_norms(g["W_dec"])[feats[:16]],
                       nref.inv_norms(g["W_dec"]))
    assert np.max(np.abs(cosv.astype(np.float64) - g["cos_head"])) <= bound
    # logits: the bound scales with |q| |key|
    lv, li = nref.rows_topk(g["W_dec"], g["W_U"], k, q_rows=feats)
    qn = np.linalg.norm(g["W_dec"][feats].astype(np.float64), axis=1)[:, None]
    lb = bound * qn * np.linalg.norm(g["W_U"].astype(np.float64), axis=1).max()
    ok, compared, mism, left = nref.compare_with_reference(lv, li, g["lg_values"], g["lg_indices"], lb)
    assert ok and mism == 0 and left < 0.01 * lv.size, (ok, compared, mism, left)


def test_get_neighbors_dict_shape(g15):
    """get_neighbors over a stand-in Sae whose neighbors() is the restatement: the reference's dict layout."""
    from msae.features import get_neighbors

    g = g15
    k, feats = int(g["k"]), g["features"].tolist()

    class FakeSae:
        def neighbors(self, features, k=10, matrix="decoder", exclude_self=True):
            assert matrix == "decoder" and exclude_self is False
            v, i = nref.neighbors(g["W_dec"], features, k, exclude_self=False)
            return torch.from_numpy(v), torch.from_numpy(i)

    nd, plf = get_neighbors({"a": FakeSae(), "b": FakeSae(), "c": FakeSae()}, {"a": feats, "b": [], "d": [1]}, k=k)
    assert list(nd) == ["a"] and list(plf) == ["a"] and sorted(nd["a"]) == list(range(len(feats)))
    ent = nd["a"][0]
    assert sorted(ent) == ["indices", "values"] and len(ent["indices"]) == len(ent["values"]) == k - 1
    assert all(isinstance(x, int) for x in ent["indices"]) and all(isinstance(x, float) for x in ent["values"])
    gi = np.array([nd["a"][m]["indices"] for m in range(len(feats))])
    gv = np.array([nd["a"][m]["values"] for m in range(len(feats))])
    ok, compared, mism, left = nref.compare_with_reference(gv, gi, g["nb_values"][:, 1:], g["gn_indices"],
                                                           nref.cos_bound(g["W_dec"].shape[1]))
    assert ok and mism == 0 and left < 0.01 * gi.size
    assert plf["a"] == sorted(set(plf["a"])) and set(gi.ravel()) <= set(plf["a"])


def test_wrapper_argument_errors():
    from msae import Sae, SaeConfig, ops
    from msae.features import cos

    sae = Sae(16, SaeConfig(num_latents=64, k=4))
    for k in (0, 65, -1):
        with pytest.raises(ValueError):
            sae.neighbors([1, 2], k=k)
        with pytest.raises(ValueError):
            sae.top_logits(torch.zeros(100, 16), [1], k=k)
    with pytest.raises(ValueError):
        sae.neighbors(k=64)                                # 64 latents, one excluded: k <= 63
    with pytest.raises(ValueError):
        sae.top_logits(torch.zeros(5, 16), [1], k=6)       # k > V
    with pytest.raises(ValueError):
        sae.neighbors([1], matrix="unembedding")
    with pytest.raises(ValueError):
        sae.neighbors([64])
    with pytest.raises(ValueError):
        sae.top_logits(torch.zeros(100, 8))
    with pytest.raises(ValueError):
        Sae(16, SaeConfig(num_latents=64, k=4), decoder=False).neighbors([1])
    # no CPU path
    for call in (lambda: sae.neighbors([1, 2], k=3), lambda: sae.top_logits(torch.zeros(100, 16), [1], k=3),
                 lambda: ops.row_inv_norms(torch.zeros(4, 4)), lambda: ops.rows_topk(torch.zeros(4, 4), torch.zeros(9, 4), 2),
                 lambda: cos(torch.zeros(4, 4), [0])):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
    # inference only
    w = torch.zeros(4, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference"):
        ops.row_inv_norms(w)
    with pytest.raises(RuntimeError, match="inference"):
        ops.rows_topk(w, torch.zeros(9, 4), 2)
    assert hasattr(torch.ops.msae, "rows_topk") and hasattr(torch.ops.msae, "row_inv_norms")


def test_symbols_and_workspace_size():
    from msae import _hip

    lib = ctypes.CDLL(str(_hip.LIB_PATH))
    for name in ("msae_row_inv_norms_f32", "msae_rows_topk_ws_bytes", "msae_rows_topk_f32", "msae_rows_topk_i64_f32"):
        assert hasattr(lib, name), name
        assert name in _hip.PROTOTYPES
    ws = _hip.load().msae_rows_topk_ws_bytes
    for M, N, k, chunks in ((130, 4096, 10, 3), (130, 4096, 64, 32), (1000, 1000, 1, 8), (1, 131072, 10, 64),
                            (4096, 4096, 64, 2)):
        assert ws(M, N, k, chunks) >= chunks * 2 * M * k * 4, (M, N, k, chunks)
    assert ws(130, 1000, 10, 99) >= 8 * 2 * 130 * 10 * 4          # forced chunks are capped at the 8 strips
    assert ws(130, 4096, 10, 0) >= 2 * 130 * 10 * 4
    assert ws(0, 4096, 10, 0) > 0
    for bad in ((130, 4096, 0, 1), (130, 4096, 65, 1), (130, 0, 10, 1), (-1, 4096, 10, 1), (130, 131072, 64, 129)):
        assert ws(*bad) == 0, bad
    assert _hip.load().msae_abi_version() == _hip.ABI_VERSION
    # argument errors of the entry point itself (no launch happens)
    f = _hip.load().msae_rows_topk_f32
    one = ctypes.c_void_p(16)
    assert f(one, 10, None, 4, one, 10, 8, None, None, None, 11, 0, one, one, None, 0, None) == -1     # k > N
    assert f(one, 10, None, 4, one, 10, 8, None, None, one, 10, 0, one, one, None, 0, None) == -1      # k > N - 1 with exclude
    assert f(one, 10, None, 11, one, 10, 8, None, None, None, 2, 0, one, one, None, 0, None) == -1     # M > Qn without q_rows
    assert f(one, 10, None, 0, one, 10, 8, None, None, None, 2, 0, one, one, None, 0, None) == 0       # M = 0: nothing to do
