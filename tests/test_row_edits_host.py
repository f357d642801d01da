"""Host side of the per-token latent edits: the two numpy restatements of tests/row_edits_ref.py
against each other, RowEdits' validation, the argument errors of Sae.encode and of the C entry points that need no
device, the C ABI, and SteeringController(batch_features=) on tests/fakes.py's model with an oracle-backed splice."""
import ctypes

import numpy as np
import pytest
import torch

import edits_ref as eref
import fakes
import row_edits_ref as rref
import synth
from conftest import GOLDEN, REPO
from oracle import oracle

D, N, T = 64, 1000, 12
SIZES = (0, 1, 3, 50)
GROUP_OF = np.array([3, 3, 1, 2, -1, 0, 3, 1, 2, -1, 0, 2], dtype=np.int32)     # token 1 (all-zero row) -> the long table


def _weights(d, n, seed):
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, n, seed)
    b_enc = (-np.abs(b_enc) - np.float32(0.5)).astype(np.float32)          # b_enc <= 0: x = b_dec is an all-zero row
    return W_enc, b_enc, W_dec, b_dec


def _case(k):
    W_enc, b_enc, _, b_dec = _weights(D, N, 67)
    x = synth.activations(T, D, 9, n_outlier=1)
    x[1] = b_dec
    L = oracle.pre_acts(x, W_enc, b_enc, b_dec)
    assert (L[1] == 0).all()
    order = np.stack([np.lexsort((np.arange(N), -L[t].astype(np.float64))) for t in range(T)])
    # each group's plan is planted relative to the ranking of its first token: 2 (group 1), 3 (group 2), 0 (group 3)
    specs = [None, rref.plan(L, order, k, 1, 2, N), rref.plan(L, order, k, 3, 3, N, start=1), rref.plan(L, order, k, 50, 0, N)]
    return L, order, specs


@pytest.mark.parametrize("k", [4, 32])
def test_restatements_agree_with_planted_positions(k):
    L, order, specs = _case(k)
    groups = rref.merge_groups(specs)
    assert [0 if g is None else len(g[0]) for g in groups] == list(SIZES)
    dv, di = rref.dense_topk_rows(L, k, groups, GROUP_OF)
    for extra in (0, 3):                                                    # independent of kk beyond k + E_max
        lv, li = oracle.topk(L, k + max(SIZES) + extra)
        ev, ei, edited = rref.list_edit_rows(lv, li, k, groups, GROUP_OF)
        assert np.array_equal(di, ei) and np.array_equal(eref.bits(dv), eref.bits(ev))
    pv, pi = oracle.topk(L, k)
    for t in np.nonzero((GROUP_OF < 0) | (GROUP_OF == 0))[0]:               # group -1 and the empty group: the plain rows
        assert np.array_equal(di[t], pi[t]) and np.array_equal(eref.bits(dv[t]), eref.bits(pv[t])) and not edited[t].any()
    # `edited` marks exactly the slots whose feature is in the token's table
    for t, g in enumerate(GROUP_OF):
        tab = rref.table_of(groups, g)
        want = np.zeros(k, dtype=bool) if tab is None else np.isin(di[t], tab[0])
        assert np.array_equal(edited[t].astype(bool), want)
    # the planted positions
    assert int(order[2][0]) not in di[2].tolist()                           # group 1: a ZERO inside token 2's top-k
    assert int(order[2][0]) not in di[7].tolist() and GROUP_OF[7] == 1      # ... nor in the group's other token
    o3, row3 = order[3], di[3].tolist()                                     # group 2 (start=1): SET equal, SET below, SET -1
    assert int(o3[k]) in row3 and specs[2]["set"][int(o3[k])] == float(L[3, o3[min(1, k - 1)]])
    assert int(o3[k + 3 + 5]) not in row3 and int(o3[k + 1]) not in row3
    o0, row0 = order[0], di[0].tolist()                                     # group 3: every position of the plan
    assert int(o0[0]) not in row0 and int(o0[k + 1]) not in row0 and int(o0[k + 50 + 5]) not in row0
    if k == 32:                                                             # (at k = 4 the table's random SETs crowd it out)
        assert int(o0[k]) in row0
    assert (dv >= 0).all()
    # the all-zero row (token 1, the long table): positive SETs first, then zeros by ascending index, the SET to 0 on
    # feature 1 and the ZEROs on 2 and 3 keeping their places in the fill
    r1 = di[1].tolist()
    assert dv[1, 0] > 0 and r1[0] in specs[3]["set"]
    tail = [f for f, val in zip(r1, dv[1]) if val == 0]
    assert tail == sorted(tail) and (len(tail) < 3 or tail[:3] == [1, 2, 3])


def test_row_edits_validation():
    from msae.features import FeatureEdits, RowEdits

    fe = FeatureEdits(100, set={7: 1.5}, zero=[9, 3], device="cpu")
    r = RowEdits(100, [fe, None, dict(set={5: 2.0, 2: 1.0}, zero=[8]), dict(zero=[4])], device="cpu")
    assert (r.G, r.E_max, r.E_total) == (4, 3, 7) and len(r) == 4
    assert r.offsets.tolist() == [0, 3, 3, 6, 7] and r.offsets.dtype == torch.int32      # the None group keeps its index
    assert r.feat.tolist() == [3, 7, 9, 2, 5, 8, 4] and r.feat.dtype == torch.int32
    assert r.kind.tolist() == [1, 0, 1, 0, 0, 1, 1] and r.val.dtype == torch.float32
    assert r.val[1].item() == 1.5 and r.val[3].item() == 1.0 and r.val[4].item() == 2.0
    assert r.tables[1] == ((), (), ()) and r.tables[2][0] == (2, 5, 8)
    for bad in ([dict(set=([3, 3], [1.0, 2.0]))],                           # a duplicate SET feature inside a group
                [dict(zero=[1]), dict(set={100: 1.0})], [dict(zero=[-1])],  # a feature out of range
                [None, None], [],                                           # every group empty / no group
                [dict(zero=[1]), 5], [dict(zero=[1], other=[2])], [dict()],
                dict(zero=[1]), fe,                                         # not a sequence of groups
                [FeatureEdits(101, zero=[1], device="cpu")]):               # built for another width
        with pytest.raises(ValueError):
            RowEdits(100, bad, device="cpu")
    assert RowEdits(100, [dict(set={3: 1.0}), dict(set={3: 2.0})], device="cpu").E_max == 1   # the same feature in two groups
    r.check(100, 8)
    with pytest.raises(ValueError):
        r.check(101, 8)
    with pytest.raises(ValueError):
        r.check(100, 98)                                                    # k + E_max > N
    big = RowEdits(8192, [dict(zero=range(100)), dict(zero=[1])], device="cpu")
    big.check(8192, 3996)
    with pytest.raises(ValueError):
        big.check(8192, 3997)                                               # k + E_max > 4096


def test_encode_argument_errors_without_a_device():
    from msae import Sae, SaeConfig, ops
    from msae.features import FeatureEdits, RowEdits, clamp_features_rows
    from msae.parallel import EmulatedShardGroup, ShardedSae

    sae = Sae(16, SaeConfig(num_latents=64, k=4))
    fe = FeatureEdits(64, zero=[5], device="cpu")
    r = RowEdits(64, [dict(set={3: 1.0}), None, dict(zero=[5, 6])], device="cpu")
    x2, x3 = torch.zeros(6, 16), torch.zeros(3, 2, 16)
    grp = torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="edit_group"):
        sae.encode(x2, edits=fe, edit_group=grp)                            # edit_group with a FeatureEdits
    with pytest.raises(ValueError, match="edit_group"):
        sae.encode(x2, set_feature=3, edit_group=grp)                       # ... with the scalar arguments
    with pytest.raises(ValueError, match="edit_group"):
        sae.encode(x2, edit_group=grp)
    with pytest.raises(ValueError, match="either"):
        sae.encode(x2, edits=r, edit_group=grp, zero_feature=2)
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros(6, 1, dtype=torch.int32), torch.zeros(6), [0] * 6):
        with pytest.raises(ValueError, match="edit_group"):
            sae.encode(x2, edits=r, edit_group=bad)                         # a wrong shape / dtype / type
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="edit_group"):
            sae.encode(x3, edits=r, edit_group=bad)
    with pytest.raises(ValueError, match="group b"):
        sae.encode(x2, edits=r)                                             # edit_group=None needs a 3-d x ...
    with pytest.raises(ValueError, match="group b"):
        sae.encode(torch.zeros(2, 3, 16), edits=r)                          # ... with x.shape[0] == G
    with pytest.raises(ValueError):
        sae.encode(x3, edits=RowEdits(65, [dict(zero=[1])] * 3, device="cpu"))
    with pytest.raises(ValueError):
        sae.encode(x3, edits=RowEdits(64, [dict(zero=range(61))] * 3, device="cpu"))   # k + E_max > N
    for ok in (dict(edit_group=None), dict(edit_group=torch.zeros(3, dtype=torch.int64)),
               dict(edit_group=torch.zeros(3, 2, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="MI355X"):                   # the arguments pass; there is no CPU path
            sae.encode(x3, edits=r, **ok)
    v, i = torch.zeros(6, 8), torch.zeros(6, 8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.edit_topk_rows(v, i, grp, r, 64, 4)
    for args in ((v[:, :5], i[:, :5], grp, r, 64, 4), (v, i, grp, r, 5, 4), (v, i, grp[:5], r, 64, 4),
                 (v, i, grp.float(), r, 64, 4), (v, i.float(), grp, r, 64, 4), (v, i, grp, r, 64, 0)):
        with pytest.raises(ValueError):
            ops.edit_topk_rows(*args)
    assert hasattr(torch.ops.msae, "edit_topk_rows")
    for cls in (ShardedSae, EmulatedShardGroup):
        with pytest.raises(NotImplementedError, match="Sae"):
            cls.encode(object.__new__(cls), x2, edits=r)
    layer = torch.nn.Identity()
    for h in clamp_features_rows(sae, [3, [4, 5], {6: 1.0}, None], layer, k=2.0):
        assert h.edits.G == 4 and h.edits.offsets.tolist() == [0, 1, 3, 4, 4]
        h.remove()
    with pytest.raises(ValueError):
        clamp_features_rows(sae, [3, 64], layer)
    with pytest.raises(ValueError):
        clamp_features_rows(sae, [None, None], layer)
    with pytest.raises(NotImplementedError, match="Sae"):
        clamp_features_rows(object(), [3, 5], layer)


def test_fake_impl_shapes():
    from msae import ops  # noqa: F401  (registers the op)
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        e = lambda n, dt=torch.int32: torch.empty(n, dtype=dt)
        for want, m in ((True, 32), (False, 0)):
            v, i, ed = torch.ops.msae.edit_topk_rows(torch.empty(3, 5, 40), torch.empty(3, 5, 40, dtype=torch.int64), e((3, 5)),
                                                     e(4), e(8), e(8, torch.float32), e(8), 5, 1000, 32, want)
            assert v.shape == (3, 5, 32) and v.dtype == torch.float32 and i.shape == (3, 5, 32) and i.dtype == torch.int64
            assert ed.shape == (3, 5, m) and ed.dtype == torch.uint8


def test_symbols_and_argument_errors_of_the_entry_points():
    from msae import _hip

    header = (REPO / "include" / "msae.h").read_text()
    lib = ctypes.CDLL(str(_hip.LIB_PATH))
    for name in ("msae_edit_topk_rows_f32", "msae_edit_topk_rows_i64_f32"):
        assert hasattr(lib, name) and name in _hip.PROTOTYPES and f"int {name}(" in header, name
    assert _hip.load().msae_abi_version() == 4 == _hip.ABI_VERSION
    one = ctypes.c_void_p(16)
    for f in (_hip.load().msae_edit_topk_rows_f32, _hip.load().msae_edit_topk_rows_i64_f32):
        def call(T=4, kk=64, G=2, E_total=5, E_max=3, n=1000, k=8, ptrs=None, edited=one):
            p = ptrs or [one] * 9
            return f(p[0], p[1], T, kk, p[2], p[3], G, p[4], p[5], p[6], E_total, E_max, n, k, p[7], p[8], edited, None)

        assert call(T=-1) == -1 and call(G=0) == -1 and call(k=0) == -1
        assert call(E_max=0) == -1 and call(E_total=-1) == -1
        assert call(E_max=30, n=40, k=32) == -1                             # k + E_max > N
        assert call(kk=5000, E_max=97, n=8192, k=4000) == -1                # k + E_max > 4096
        assert call(kk=10) == -1                                            # kk < k + E_max
        for hole in range(9):                                               # a null pointer
            p = [one] * 9
            p[hole] = None
            assert call(ptrs=p) == -1
        assert call(T=0) == 0 and call(T=0, edited=None) == 0               # T = 0: nothing to do; `edited` may be null
        assert call(T=0, E_total=0) == 0 and call(T=-1, edited=None) == -1


def _oracle_splice(weights):
    """sae_reconstruct on the oracle: the dense definition per token, then oracle.decode (no device)."""
    from msae.features import RowEdits

    W_enc, b_enc, W_dec, b_dec = weights
    calls = []

    def reconstruct(sae, hidden, *, set_feature=-1, set_value=0.0, zero_feature=-1, out_dtype=None, differentiable=None,
                    edits=None, edit_group=None):
        k = sae.cfg.k
        x = hidden.reshape(-1, hidden.shape[-1]).float().numpy()
        L = oracle.pre_acts(x, W_enc, b_enc, b_dec)
        if isinstance(edits, RowEdits):
            assert edit_group is None and hidden.dim() == 3 and hidden.shape[0] == edits.G
            groups = [None if not t[0] else tuple(np.asarray(a, dtype=dt) for a, dt in zip(t, (np.int32, np.float32, np.int32)))
                      for t in edits.tables]
            L = rref.apply_dense_rows(L, groups, np.repeat(np.arange(edits.G), hidden.shape[1]))
            calls.append(edits.G)
        elif set_feature >= 0:
            L[:, set_feature] = np.float32(set_value)
        assert edits is None or isinstance(edits, RowEdits)
        v, i = oracle.topk(L, k)
        out = oracle.decode(i, v, W_dec, b_dec)
        return torch.from_numpy(out).to(out_dtype or hidden.dtype).view(hidden.shape)

    return reconstruct, calls


def test_controller_batches_the_feature_list(monkeypatch):
    from msae import Sae, SaeConfig
    from msae.features import hooks
    from msae.features.steering import SteeringController

    g = np.load(GOLDEN / "g10_steering.npz")
    d, n, k = int(g["d"]), int(g["N"]), int(g["k"])
    model = fakes.TinyLlava(vocab=int(g["vocab"]), d=d)
    weights = synth.sae_weights(d, n, int(g["wseed"]))
    sae = Sae(d, SaeConfig(num_latents=n, k=k))
    reconstruct, calls = _oracle_splice(weights)
    monkeypatch.setattr(hooks, "sae_reconstruct", reconstruct)
    feats = [3, 17, 5, 40, 8, 21]
    kw = dict(sae=sae, module_name=str(g["module"]), feature_idx=feats, model=model, processor=fakes.FakeProcessor(int(g["vocab"])),
              prompt="hello", k=float(g["clamp"]))
    one = SteeringController(**kw).run()
    assert not calls
    four = SteeringController(batch_features=4, **kw).run()
    assert list(four) == list(one) and len(four) == len(feats)
    for key in one:
        assert four[key].keys() == one[key].keys()
        assert four[key]["original_resps"] == one[key]["original_resps"] and four[key]["idx"] == one[key]["idx"]
        assert isinstance(four[key]["clamped_resps"], str) and four[key]["clamped_resps"]
    assert calls == [4, 2]                                                  # one prefill per chunk; the last chunk is short
    assert SteeringController(**kw).batch_features == 1
    with pytest.raises(ValueError):
        SteeringController(batch_features=0, **kw)
    with pytest.raises(NotImplementedError, match="Sae"):
        SteeringController(batch_features=2, **{**kw, "sae": object()})


def test_launcher_flag():
    from msae.launch.features import steering as launch

    assert launch.parse_argument(["-t", "x"]).batch_features == 1
    assert launch.parse_argument(["-t", "x", "--batch-features", "16"]).batch_features == 16
    for bad in (["--batch-features", "4", "--shard-sae"], ["--batch-features", "0"]):
        with pytest.raises(SystemExit):
            launch.parse_argument(["-t", "x"] + bad)
