"""Host side of the set-valued latent edits: the two numpy restatements (tests/edits_ref.py: dense definition and the
list rule the HIP kernel implements) on hand-computed and random cases and against the reference's own hooks run with
feature lists (tests/golden/g16_multi_edit.npz), FeatureEdits' validation, the wrappers' argument errors, the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import edits_ref as eref
import synth
from conftest import GOLDEN
from oracle import oracle

# 2 tokens x 8 features; token 1 has two positive latents only, so its tail is zero fill by ascending index
L28 = np.array([[5, 0, 3, 0, 4, 1, 0, 2],
                [0, 0, 7, 0, 0, 6, 0, 0]], dtype=np.float32)


def _both(L, k, set_edits=None, zero=None, extra=0):
    """dense definition and list rule on explicit latents; asserts that they agree bit for bit."""
    feats, vals, kinds = eref.merge(set_edits, zero)
    dv, di = eref.dense_topk(L, k, feats, vals, kinds)
    lv, li = oracle.topk(L, k + len(feats) + extra)
    ev, ei = eref.list_edit(lv, li, k, feats, vals, kinds)
    assert np.array_equal(di, ei) and np.array_equal(eref.bits(dv), eref.bits(ev)), (di, ei, dv, ev)
    return dv, di


def test_hand_cases_cover_the_contract():
    # 1. SET and ZERO: feature 0 (rank 1 of token 0) zeroed, feature 6 set to 4.5
    v, i = _both(L28, 3, {6: 4.5}, [0])
    assert i.tolist() == [[6, 4, 2], [2, 5, 6]] and v.tolist() == [[4.5, 4, 3], [7, 6, 4.5]]
    # ZERO wins where a feature is in both lists
    v, i = _both(L28, 3, {0: 9.0, 6: 4.5}, [0])
    assert i.tolist() == [[6, 4, 2], [2, 5, 6]]
    # 3. a SET value equal to a selected value: index order decides (feature 1 before feature 4 at value 4)
    v, i = _both(L28, 3, {1: 4.0})
    assert i.tolist() == [[0, 1, 4], [2, 5, 1]] and v[0].tolist() == [5, 4, 4]
    #    SET to 0 ties with the zero fill by index; SET to -1 never appears (k + E <= N)
    v, i = _both(L28, 4, {2: 0.0, 5: -1.0})
    assert i.tolist() == [[0, 4, 7, 1], [0, 1, 2, 3]] and v.tolist() == [[5, 4, 2, 0], [0, 0, 0, 0]]
    #    a SET below the k-th value does not appear; one on a selected feature replaces its value
    v, i = _both(L28, 3, {6: 2.5, 4: 9.0})
    assert i[0].tolist() == [4, 0, 2] and v[0].tolist() == [9, 5, 3]
    # all of token 1's positives zeroed (E >= its support): the row becomes pure fill
    v, i = _both(L28, 2, None, [2, 5])
    assert i.tolist() == [[0, 4], [0, 1]] and v[1].tolist() == [0, 0]
    # fewer than k positives: ZERO on the fill (features 0, 1) and SET among it (feature 3)
    v, i = _both(L28, 4, {3: 0.5}, [0, 1])
    assert i[1].tolist() == [2, 5, 3, 0] and v[1].tolist() == [7, 6, 0.5, 0]
    # an all-zero row
    Z = np.zeros((1, 8), dtype=np.float32)
    v, i = _both(Z, 3, {1: 0.0, 5: 2.0}, [0])
    assert i.tolist() == [[5, 0, 1]] and v.tolist() == [[2, 0, 0]]
    # 5. independent of kk beyond k + E
    for extra in (0, 1, 3):
        _both(L28, 2, {6: 4.5, 1: 1.5}, [0], extra=extra)
    # -0 as a set value comes back as +0 from the list rule (the library decodes values from rank keys)
    feats, vals, kinds = eref.merge({3: -0.0})
    lv, li = oracle.topk(L28, 5)
    ev, ei = eref.list_edit(lv, li, 4, feats, vals, kinds)
    assert not np.signbit(ev).any()


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(77)
    for case in range(60):
        T, N = int(rng.integers(1, 6)), int(rng.integers(12, 80))
        k = int(rng.integers(1, 6))
        E = int(rng.integers(1, N - k + 1))
        L = rng.standard_normal((T, N)).astype(np.float32)
        L[L < rng.uniform(-0.5, 1.5)] = 0.0                               # relu-like, sparse to nearly empty rows
        if case % 5 == 0:
            L[0] = 0.0
        L = np.round(L * 4) / 4                                           # ties
        feats = rng.permutation(N)[:E]
        n_set = int(rng.integers(0, E + 1))
        pool = np.concatenate([np.unique(L), np.array([0.0, -1.0, 0.125], dtype=np.float32)])
        set_edits = {int(f): float(rng.choice(pool)) for f in feats[:n_set]}
        zero = [int(f) for f in feats[n_set:]] + [int(f) for f in feats[:n_set][:2]]     # two features in both lists
        _both(L.astype(np.float32), k, set_edits, zero, extra=min(int(rng.integers(0, 4)), N - k - E))   # kk <= N


def test_one_edit_equals_the_oracle_s_scalar_arguments():
    d, N, k, T = 32, 200, 6, 9
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, N, 5)
    x = synth.activations(T, d, 3, n_outlier=1)
    top_v, top_i = oracle.encode_topk(x, W_enc, b_enc, b_dec, k + 3)
    for f in (int(top_i[0, 0]), int(top_i[0, k]), int(top_i[0, k + 2]), 0, N - 1):
        for kw, ed in (({"set_feature": f, "set_value": 0.75}, ({f: 0.75}, None)),
                       ({"zero_feature": f}, (None, [f])),
                       ({"set_feature": f, "set_value": 0.0}, ({f: 0.0}, None))):
            rv, ri = oracle.encode_topk(x, W_enc, b_enc, b_dec, k, **kw)
            for got in (eref.dense_encode(x, W_enc, b_enc, b_dec, k, *ed), eref.list_encode(x, W_enc, b_enc, b_dec, k, *ed)):
                assert np.array_equal(got[1], ri) and np.array_equal(eref.bits(got[0]), eref.bits(rv)), (f, kw)


def test_restatement_matches_the_reference_hooks_with_feature_lists():
    """g16 = the reference's own steering / attribution hooks called with LISTS; tolerance: test_oracle_golden's for g5."""
    g = np.load(GOLDEN / "g16_multi_edit.npz")
    d, N, k = int(g["d"]), int(g["N"]), int(g["k"])
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, N, int(g["wseed"]))
    feats, clamp = g["steer_features"].tolist(), float(g["steer_clamp"])
    for S in (5, 1):
        x = g[f"steer_S{S}_x"][0].astype(np.float32)
        if S != 1:
            v, i = eref.list_encode(x, W_enc, b_enc, b_dec, k, {f: clamp for f in feats})
            assert set(feats) <= set(i[0].tolist())
        else:
            v, i = oracle.encode_topk(x, W_enc, b_enc, b_dec, k)
        out = oracle.decode(i, v, W_dec, b_dec).astype(np.float16)
        ref = g[f"steer_S{S}_out"][0]
        assert np.abs(out.astype(np.float32) - ref.astype(np.float32)).max() <= 2e-3 * np.abs(ref).max()
    x = g["attr_x"].reshape(-1, d).astype(np.float32)
    for tag in ("few", "many"):
        off = g[f"attr_{tag}_features"].tolist()
        for v, i in (eref.list_encode(x, W_enc, b_enc, b_dec, k, None, off), eref.dense_encode(x, W_enc, b_enc, b_dec, k, None, off)):
            out = oracle.decode(i, v, W_dec, b_dec).astype(np.float16).reshape(g["attr_x"].shape)
            ref = g[f"attr_{tag}_out"]
            assert np.abs(out.astype(np.float32) - ref.astype(np.float32)).max() <= 2e-3 * np.abs(ref).max()
    assert len(g["attr_many_features"]) >= k


def test_feature_edits_validation():
    from msae.features import FeatureEdits

    e = FeatureEdits(100, set={7: 1.5, 3: 2.0, 50: 4.0}, zero=[9, 3, 9], device="cpu")
    assert e.E == 4 and e.features == (3, 7, 9, 50) and len(e) == 4
    assert e.feat.tolist() == [3, 7, 9, 50] and e.feat.dtype == torch.int32
    assert e.kind.tolist() == [1, 0, 1, 0]                                  # the same feature in both lists -> ZERO
    assert e.val.dtype == torch.float32 and e.val[1].item() == 1.5 and e.val[3].item() == 4.0
    assert e.mask.dtype == torch.bool and e.mask.nonzero().flatten().tolist() == [3, 7, 9, 50]
    rf, rv, rk = eref.merge({7: 1.5, 3: 2.0, 50: 4.0}, [9, 3, 9])
    assert rf.tolist() == e.feat.tolist() and rk.tolist() == e.kind.tolist()
    pair = FeatureEdits(100, set=(torch.tensor([5, 2]), torch.tensor([1.0, 3.0])), zero=torch.tensor([8]), device="cpu")
    assert pair.features == (2, 5, 8) and pair.val.tolist()[:2] == [3.0, 1.0]
    assert FeatureEdits(100, zero=4, device="cpu").features == (4,)
    assert FeatureEdits(100, zero=np.array([4, 2]), device="cpu").features == (2, 4)
    for bad in (dict(set={100: 1.0}), dict(set={-1: 1.0}), dict(zero=[100]), dict(zero=[-2]),     # out of range
                dict(set=([3, 3], [1.0, 2.0])),                                                  # duplicate in set
                dict(), dict(set={}, zero=[]),                                                   # empty
                dict(set=([1, 2], [1.0])), dict(set={1: float("nan")}), dict(set={1: float("inf")}),
                dict(zero=[1.5]), dict(set=5)):
        with pytest.raises(ValueError):
            FeatureEdits(100, device="cpu", **bad)
    with pytest.raises(ValueError):
        FeatureEdits(5000, zero=range(4096), device="cpu")                   # k + E <= 4096 leaves at most 4095
    e.check(100, 8)
    with pytest.raises(ValueError):
        e.check(101, 8)
    with pytest.raises(ValueError):
        e.check(100, 97)                                                    # k + E > N


def test_wrapper_argument_errors():
    from msae import Sae, SaeConfig, ops
    from msae.features import FeatureEdits, clamp_features_max
    from msae.features.patching import Attribution

    sae = Sae(16, SaeConfig(num_latents=64, k=4))
    e = FeatureEdits(64, set={3: 1.0}, zero=[5], device="cpu")
    x = torch.zeros(2, 16)
    for kw in (dict(set_feature=3), dict(zero_feature=2), dict(set_feature=3, set_value=1.0, zero_feature=2)):
        with pytest.raises(ValueError, match="either"):
            sae.encode(x, edits=e, **kw)
    with pytest.raises(ValueError):
        sae.encode(x, edits=FeatureEdits(65, zero=[1], device="cpu"))       # built for another width
    with pytest.raises(ValueError):
        sae.encode(x, edits=FeatureEdits(64, zero=range(61), device="cpu"))  # k + E > N
    with pytest.raises(RuntimeError, match="MI355X"):                       # no CPU path
        sae.encode(x, edits=e)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.edit_topk(torch.zeros(2, 6), torch.zeros(2, 6, dtype=torch.int64), e.feat, e.val, e.kind, 64, 4)
    for kk, k, N in ((5, 4, 64), (70, 63, 64)):                             # kk < k + E, k + E > N
        with pytest.raises(ValueError):
            ops.edit_topk(torch.zeros(2, kk), torch.zeros(2, kk, dtype=torch.int64), e.feat, e.val, e.kind, N, k)
    with pytest.raises(ValueError):                                         # k + E > 4096
        ops.edit_topk(torch.zeros(1, 5000), torch.zeros(1, 5000, dtype=torch.int64), e.feat, e.val, e.kind, 8192, 4095)
    assert hasattr(torch.ops.msae, "edit_topk")
    # the hooks build their FeatureEdits on the Sae's device; a sharded engine takes one feature only
    layer = torch.nn.Identity()
    for h in clamp_features_max(sae, [3, 5], layer, k=2.0) + clamp_features_max(sae, {3: 1.0, 5: 2.0}, layer) \
            + clamp_features_max(sae, 3, layer):
        h.remove()
    with pytest.raises(ValueError):
        clamp_features_max(sae, [3, 64], layer)

    class Engine:                                                           # not an Sae: the engine interface
        pass

    with pytest.raises(NotImplementedError, match="Sae"):
        clamp_features_max(Engine(), [3, 5], layer)
    from msae.parallel import EmulatedShardGroup, ShardedSae

    for cls in (ShardedSae, EmulatedShardGroup):
        with pytest.raises(NotImplementedError, match="Sae"):
            cls.encode(object.__new__(cls), x, edits=e)
    attr = Attribution.__new__(Attribution)
    with pytest.raises(ValueError, match="batched"):
        attr.get_attribution([[1, 2], 3], method="batched")


def test_fake_impl_shapes():
    from msae import ops  # noqa: F401  (registers the op)
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        v, i = torch.ops.msae.edit_topk(torch.empty(3, 5, 40), torch.empty(3, 5, 40, dtype=torch.int64),
                                        torch.empty(8, dtype=torch.int32), torch.empty(8), torch.empty(8, dtype=torch.int32),
                                        1000, 32)
        assert v.shape == (3, 5, 32) and v.dtype == torch.float32 and i.shape == (3, 5, 32) and i.dtype == torch.int64


def test_symbols_and_argument_errors_of_the_entry_points():
    from msae import _hip

    lib = ctypes.CDLL(str(_hip.LIB_PATH))
    for name in ("msae_edit_topk_f32", "msae_edit_topk_i64_f32"):
        assert hasattr(lib, name), name
        assert name in _hip.PROTOTYPES
    assert _hip.load().msae_abi_version() == 4 == _hip.ABI_VERSION
    one = ctypes.c_void_p(16)
    for f in (_hip.load().msae_edit_topk_f32, _hip.load().msae_edit_topk_i64_f32):
        #          vals_in idx_in T  kk  feat val kind E  N     k   vals idx stream          (no launch happens)
        assert f(one, one, 4, 10, one, one, one, 3, 1000, 8, one, one, None) == -1           # kk < k + E
        assert f(one, one, 4, 64, one, one, one, 30, 40, 32, one, one, None) == -1           # k + E > N
        assert f(one, one, 4, 5000, one, one, one, 97, 8192, 4000, one, one, None) == -1     # k + E > 4096
        assert f(one, one, 4, 64, one, one, one, 0, 1000, 8, one, one, None) == -1           # E < 1
        assert f(one, one, 4, 64, one, one, one, 3, 1000, 0, one, one, None) == -1           # k < 1
        assert f(one, one, -1, 64, one, one, one, 3, 1000, 8, one, one, None) == -1          # T < 0
        for hole in range(7):                                                               # a null pointer
            p = [one] * 7
            p[hole] = None
            assert f(p[0], p[1], 4, 64, p[2], p[3], p[4], 3, 1000, 8, p[5], p[6], None) == -1
        assert f(one, one, 0, 64, one, one, one, 3, 1000, 8, one, one, None) == 0            # T = 0: nothing to do
