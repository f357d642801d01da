"""Host side of the value-dependent latent edits (scale / add / floor / cap): FeatureEdits' and
RowEdits' new arguments and every ValueError, the plain-torch host paths of ops.edit_topk / ops.edit_topk_rows against the
numpy restatement tests/value_edits_ref.py BIT FOR BIT, the planted cases against four wrong variants, the fake
implementations, the hooks' `mode` and the C entry points' argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import edits_ref as eref
import synth
import value_edits_ref as vref
from oracle import oracle

D, N = 64, 512


def _case(T=12, seed=5):
    W_enc, b_enc, _, b_dec = synth.sae_weights(D, N, seed)
    b_enc = (-np.abs(b_enc) - np.float32(0.05)).astype(np.float32)
    x = synth.activations(T, D, seed + 1)
    x[1] = b_dec                                                            # an all-zero row
    L = oracle.pre_acts(x, W_enc, b_enc, b_dec)
    pre = ((x - b_dec) @ W_enc.T + b_enc).astype(np.float32)
    order = np.stack([np.lexsort((np.arange(N), -L[t].astype(np.float64))) for t in range(T)])
    assert (L[1] == 0).all()
    return L, pre, order


def _kw_for_small_N(L, order, k, E, seed=0):
    """value_edits_ref.plan at N = 512: the GPU inputs' degenerate rows are not here, four low features stand in."""
    return vref.plan(L, order, k, E, seed, special=(40, 17, 90, 50))


def _list(L, kk):
    v, i = oracle.topk(L, kk)
    return torch.from_numpy(v), torch.from_numpy(i.astype(np.int64))


def _assert_bits(got, ref, what=""):
    gv, gi = got[0].numpy(), got[1].numpy()
    assert np.array_equal(gi, ref[1]), f"indices differ {what}"
    assert np.array_equal(vref.bits(gv), vref.bits(ref[0])), f"values differ {what}"
    if len(got) > 2:
        assert np.array_equal(vref.bits(got[2].numpy()), vref.bits(ref[2])), f"gain differs {what}"


# ---- the objects ----------------------------------------------------------------------------------------------------------
def test_constructor_rules_and_errors():
    from msae.features import FeatureEdits
    from msae.features.edits import EDIT_ADD, EDIT_CAP, EDIT_FLOOR, EDIT_SCALE, EDIT_SET, EDIT_ZERO

    e = FeatureEdits(64, set={3: 1.0}, zero=[5, 9], scale={9: 4.0, 7: 2.0}, add=([1, 2], [0.5, -0.5]), floor={40: 1.5},
                     cap=(torch.tensor([50]), torch.tensor([0.25])), device="cpu")
    assert e.features == (1, 2, 3, 5, 7, 9, 40, 50) and e.E == 8 and e.value_dependent
    assert e.kinds == (EDIT_ADD, EDIT_ADD, EDIT_SET, EDIT_ZERO, EDIT_SCALE, EDIT_ZERO, EDIT_FLOOR, EDIT_CAP)   # ZERO wins over scale
    assert e.values == (0.5, -0.5, 1.0, 0.0, 2.0, 0.0, 1.5, 0.25)
    assert e.kind.tolist() == list(e.kinds) and e.val.tolist() == list(e.values) and e.feat.tolist() == list(e.features)
    assert (EDIT_SET, EDIT_ZERO, EDIT_SCALE, EDIT_ADD, EDIT_FLOOR, EDIT_CAP) == (0, 1, 2, 3, 4, 5)
    assert "value-dependent" in repr(e)
    assert not FeatureEdits(64, set={3: 1.0}, zero=[5], device="cpu").value_dependent
    assert not FeatureEdits(64, zero=[5], scale={5: 2.0}, device="cpu").value_dependent       # the scale was zeroed
    for a, b in (("set", "scale"), ("scale", "add"), ("add", "floor"), ("floor", "cap"), ("set", "cap")):
        with pytest.raises(ValueError, match="both"):
            FeatureEdits(64, device="cpu", **{a: {3: 1.0}, b: {3: 2.0}})
    for name in ("scale", "add", "floor", "cap"):
        with pytest.raises(ValueError, match="twice"):
            FeatureEdits(64, device="cpu", **{name: ([3, 3], [1.0, 2.0])})
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="finite"):
                FeatureEdits(64, device="cpu", **{name: {3: bad}})
        with pytest.raises(ValueError):
            FeatureEdits(64, device="cpu", **{name: {64: 1.0}})             # outside [0, N)
        with pytest.raises(ValueError):
            FeatureEdits(64, device="cpu", **{name: {-1: 1.0}})
        with pytest.raises(ValueError):
            FeatureEdits(64, device="cpu", **{name: ([1, 2], [1.0])})       # lengths differ
        with pytest.raises(ValueError):
            FeatureEdits(64, device="cpu", **{name: {1.5: 1.0}})            # a float feature
        with pytest.raises(ValueError):
            FeatureEdits(64, device="cpu", **{name: 3})                     # neither a mapping nor a pair
        with pytest.raises(ValueError):
            FeatureEdits(64, device="cpu", **{name: {}})                    # nothing to edit
    with pytest.raises(ValueError):
        FeatureEdits(8192, scale={f: 2.0 for f in range(4096)}, device="cpu")


def test_existing_objects_are_unchanged():
    """A table without the new arguments has the arrays it had: same feat / val / kind, same merge as edits_ref."""
    from msae.features import FeatureEdits, RowEdits

    set_edits, zero = {9: 1.5, 3: -2.0, 40: 0.0, 7: 8.0}, [7, 1, 1, 60]
    e = FeatureEdits(64, set_edits, zero, "cpu")                            # positional, as before
    feats, vals, kinds = eref.merge(set_edits, zero)
    assert np.array_equal(e.feat.numpy(), feats) and np.array_equal(eref.bits(e.val.numpy()), eref.bits(vals))
    assert np.array_equal(e.kind.numpy(), kinds) and e.kind.dtype == torch.int32 and e.feat.dtype == torch.int32
    assert repr(e) == "FeatureEdits(num_latents=64, E=6: 3 set, 3 zero)" and not e.value_dependent
    r = RowEdits(64, [dict(set=set_edits, zero=zero), None, e, dict(zero=[2])], device="cpu")
    assert r.offsets.tolist() == [0, 6, 6, 12, 13] and r.feat.tolist() == list(feats) * 2 + [2]
    assert r.kind.tolist() == list(kinds) * 2 + [1] and np.array_equal(eref.bits(r.val.numpy()[:6]), eref.bits(vals))
    assert not r.value_dependent and r.union.numel() == 0 and r.col.tolist() == [0] * 13


def test_row_edits_union_and_col():
    from msae.features import FeatureEdits, RowEdits

    r = RowEdits(64, [dict(scale={9: 2.0}, set={3: 1.0}), None, dict(add={9: 0.5, 4: 1.0}, zero=[3]),
                      FeatureEdits(64, cap={50: 0.1}, floor={4: 0.2}, zero=[50], device="cpu"), dict(zero=[7])], device="cpu")
    assert r.G == 5 and r.E_max == 3 and r.E_total == 8 and r.value_dependent
    assert r.feat.tolist() == [3, 9, 3, 4, 9, 4, 50, 7] and r.offsets.tolist() == [0, 2, 2, 5, 7, 8]
    feat, kind = r.feat.tolist(), r.kind.tolist()
    assert r.union.dtype == torch.int32 and r.col.dtype == torch.int32 and r.col.numel() == r.E_total
    assert r.union.tolist() == [4, 9]                                       # 50 was zeroed in its group: not value-dependent
    for f, kd, c in zip(feat, kind, r.col.tolist()):
        assert (r.union[c].item() == f) if kd >= 2 else c == 0
    with pytest.raises(ValueError):
        RowEdits(64, [dict(scale={1: 2.0}, add={1: 1.0})], device="cpu")
    with pytest.raises(ValueError):
        RowEdits(64, [dict(scales={1: 2.0})], device="cpu")                 # an unknown key


# ---- the ops' host paths --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,E", [(4, 1), (4, 3), (8, 13), (32, 50)])
def test_host_path_equals_the_restatement(k, E):
    from msae import ops
    from msae.features import FeatureEdits

    L, _, order = _case()
    kw = _kw_for_small_N(L, order, k, E)
    e = FeatureEdits(N, device="cpu", **kw)
    feats, vals, kinds = vref.merge(**kw)
    assert e.E == len(feats) and np.array_equal(e.kind.numpy(), kinds)
    ref = vref.dense_topk(L, k, feats, vals, kinds)
    cur = torch.from_numpy(np.ascontiguousarray(L[:, feats]))
    for extra in (0, 5):                                                    # independent of kk beyond k + E
        lv, li = _list(L, k + e.E + extra)
        _assert_bits(ops.edit_topk(lv, li, e.feat, e.val, e.kind, N, k, cur=cur, want_gain=True), ref, f"extra={extra}")
    got = ops.edit_topk(lv, li.to(torch.int32), e.feat, e.val, e.kind, N, k, cur=cur)
    assert len(got) == 2 and got[1].dtype == torch.int32
    _assert_bits(got, ref)
    # permuted columns, wider than E, NaN where nothing may be read
    perm = torch.randperm(e.E, generator=torch.Generator().manual_seed(3))
    wide = torch.full((L.shape[0], e.E + 3), float("nan"))
    wide[:, perm] = cur
    dep = torch.from_numpy(kinds >= 2)
    wide[:, perm[~dep]] = float("nan")                                      # SET / ZERO entries read no latent
    _assert_bits(ops.edit_topk(lv, li, e.feat, e.val, e.kind, N, k, cur=wide, col=perm.to(torch.int32), want_gain=True), ref)
    # [B, S] leading dims
    T = L.shape[0]
    got = ops.edit_topk(lv.reshape(2, T // 2, -1), li.reshape(2, T // 2, -1), e.feat, e.val, e.kind, N, k,
                        cur=cur.reshape(2, T // 2, -1), want_gain=True)
    assert got[0].shape == (2, T // 2, k) and got[2].shape == (2, T // 2, k)
    _assert_bits([g.reshape(T, k) for g in got], ref)


def test_set_zero_table_through_the_valued_path_is_the_list_rule():
    """A SET / ZERO-only table through the valued path: the bits ops.edit_topk is held to (edits_ref.list_edit); `cur` is
    not read (all NaN)."""
    from msae import ops
    from msae.features import FeatureEdits

    L, _, order = _case()
    k = 8
    set_edits = {int(order[0][0]): 0.5, int(order[0][k]): float(L[0, order[0][1]]), 3: 0.0, int(order[0][k + 20]): -1.0}
    zero = [int(order[0][2]), 0]
    e = FeatureEdits(N, set=set_edits, zero=zero, device="cpu")
    lv, li = _list(L, k + e.E)
    ref_v, ref_i = eref.list_edit(lv.numpy(), li.numpy(), k, *eref.merge(set_edits, zero))
    got = ops.edit_topk(lv, li, e.feat, e.val, e.kind, N, k, cur=torch.full((L.shape[0], e.E), float("nan")), want_gain=True)
    assert np.array_equal(got[1].numpy(), ref_i) and np.array_equal(eref.bits(got[0].numpy()), eref.bits(ref_v))
    edited = np.isin(ref_i, np.array(e.features))
    assert np.array_equal(got[2].numpy(), np.where(edited, 0.0, 1.0).astype(np.float32))


def test_identity_edits_return_the_unedited_topk():
    from msae import ops
    from msae.features import FeatureEdits

    L, _, order = _case()
    k = 8
    o0 = order[0]
    for name, v in (("scale", 1.0), ("add", 0.0), ("floor", 0.0), ("cap", 3e38)):
        feats = sorted({int(o0[0]), int(o0[k - 1]), int(o0[k]), int(o0[k + 9]), 0, 1, int(o0[-1])})
        e = FeatureEdits(N, device="cpu", **{name: {f: v for f in feats}})
        lv, li = _list(L, k + e.E)
        got = ops.edit_topk(lv, li, e.feat, e.val, e.kind, N, k, cur=torch.from_numpy(np.ascontiguousarray(L[:, feats])),
                            want_gain=True)
        assert torch.equal(got[1], li[:, :k]) and torch.equal(got[0].view(torch.int32), lv[:, :k].view(torch.int32)), name
        want = torch.where(torch.from_numpy(np.isin(li[:, :k].numpy(), feats)) & (lv[:, :k] <= 0), 0.0, 1.0)
        assert torch.equal(got[2], want), name                              # gain 1 where it fires, 0 on an edited zero


def test_rows_host_path_equals_the_one_table_call():
    from msae import ops
    from msae.features import FeatureEdits, RowEdits

    L, _, order = _case()
    k, T = 8, L.shape[0]
    kws = [_kw_for_small_N(L, order, k, 9), None, _kw_for_small_N(L, order, k, 3, seed=1), dict(set={5: 1.0}, zero=[int(order[0][0])]),
           _kw_for_small_N(L, order, k, 1)]
    r = RowEdits(N, kws, device="cpu")
    group_of = torch.tensor([0, 1, 2, 3, 4, -1, 5, 0, 2, 2**40, 4, 3])      # ids outside [0, G): unedited
    lv, li = _list(L, k + r.E_max + 2)
    cur = torch.from_numpy(np.ascontiguousarray(L[:, r.union.numpy()]))
    v, i, ed, g = ops.edit_topk_rows(lv, li, group_of, r, N, k, want_mask=True, cur=cur, col=r.col, want_gain=True)
    tables = [None if kw is None else vref.merge(**kw) for kw in kws]
    ref = vref.dense_topk_rows(L, k, group_of.clamp(-1, r.G).numpy(), tables)
    _assert_bits((v, i, g), ref)
    for t in range(T):
        gid = int(group_of[t])
        if 0 <= gid < r.G and kws[gid] is not None:
            e = FeatureEdits(N, device="cpu", **kws[gid])
            one = ops.edit_topk(lv[t:t + 1], li[t:t + 1], e.feat, e.val, e.kind, N, k,
                                cur=torch.from_numpy(np.ascontiguousarray(L[t:t + 1, e.features])), want_gain=True)
            assert torch.equal(one[1], i[t:t + 1]) and torch.equal(one[0].view(torch.int32), v[t:t + 1].view(torch.int32))
            assert torch.equal(one[2], g[t:t + 1])
            assert torch.equal(ed[t].bool(), torch.from_numpy(np.isin(i[t].numpy(), e.features)))
        else:
            assert torch.equal(i[t], li[t, :k]) and torch.equal(v[t], lv[t, :k]) and (g[t] == 1).all() and (ed[t] == 0).all()
    got = ops.edit_topk_rows(lv, li, group_of, r, N, k, cur=cur, col=r.col)
    assert len(got) == 2 and torch.equal(got[1], i)
    # col=None: entry e of the concatenated table reads column e
    cols = torch.from_numpy(np.ascontiguousarray(L[:, r.feat.numpy()]))
    got = ops.edit_topk_rows(lv, li, group_of, r, N, k, cur=cols, want_gain=True)
    _assert_bits(got, ref)


def test_planted_cases_reject_the_wrong_variants():
    L, pre, order = _case()
    k, E = 8, 13
    kw = _kw_for_small_N(L, order, k, E)
    feats, vals, kinds = vref.merge(**kw)
    assert set(kinds.tolist()) >= {0, 1, 2, 3, 4, 5}
    ref = vref.dense_topk(L, k, feats, vals, kinds)
    o0, row = order[0], ref[1][0].tolist()
    far = int(o0[k + E + 5])
    assert row[0] == far and kw["scale"][far] > 1                           # entered from beyond the list, at the top
    inactive = [f for f in kw["scale"] if L[0, f] == 0 and kw["scale"][f] < 0]
    assert inactive and inactive[0] not in row and pre[0, inactive[0]] < 0
    entered = [f for f in kw["add"] if L[0, f] == 0 and kw["add"][f] > 0]
    assert entered and ref[0][0, row.index(entered[0])] == np.float32(kw["add"][entered[0]]) and ref[2][0, row.index(entered[0])] == 0
    assert int(o0[0]) not in row                                            # ADD drove it below 0
    assert int(o0[k]) in row                                                # ... and a feature beyond rank k took its place
    unchanged = int(o0[2])
    assert ref[0][0, row.index(unchanged)] == L[0, unchanged] and ref[2][0, row.index(unchanged)] == 1
    tie, with_ = int(o0[k + 1]), int(o0[3])                                 # FLOOR exactly at a selected value: index order
    a, b = row.index(tie), row.index(with_)
    assert ref[0][0, a] == ref[0][0, b] and abs(a - b) == 1 and (a < b) == (tie < with_)
    wrong = vref.wrong_variants(k, pre)
    assert len(wrong) == 4
    for name, edit in wrong.items():
        got = vref.dense_topk(L, k, feats, vals, kinds, edit=edit)
        same = all(np.array_equal(vref.bits(a), vref.bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
                   for a, b in zip(got, ref))
        assert not same, f"the planted cases do not tell '{name}' from the definition"


# ---- wrappers, fakes, hooks, entry points ------------------------------------------------------------------------------------
def test_wrapper_argument_errors():
    from msae import Sae, SaeConfig, ops
    from msae.features import FeatureEdits, RowEdits

    e = FeatureEdits(64, scale={3: 2.0}, zero=[5], device="cpu")
    v, i = torch.zeros(2, 6), torch.zeros(2, 6, dtype=torch.int64)
    cur = torch.zeros(2, 2)
    for kw in (dict(want_gain=True), dict(col=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(ValueError, match="cur"):                        # the valued arguments need cur
            ops.edit_topk(v, i, e.feat, e.val, e.kind, 64, 4, **kw)
    for bad in (cur.double(), torch.zeros(3, 2), torch.zeros(2, 0), torch.zeros(2), [[0.0, 0.0]] * 2):
        with pytest.raises(ValueError, match="cur"):
            ops.edit_topk(v, i, e.feat, e.val, e.kind, 64, 4, cur=bad)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2), [0, 1]):
        with pytest.raises(ValueError, match="col"):
            ops.edit_topk(v, i, e.feat, e.val, e.kind, 64, 4, cur=cur, col=bad)
    with pytest.raises(ValueError):
        ops.edit_topk(v[:, :5], i[:, :5], e.feat, e.val, e.kind, 64, 4, cur=cur)          # kk < k + E
    with pytest.raises(ValueError):
        ops.edit_topk(v, i.float(), e.feat, e.val, e.kind, 64, 4, cur=cur)
    r = RowEdits(64, [dict(scale={3: 2.0}), dict(add={3: 1.0, 9: 1.0})], device="cpu")
    grp = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="cur"):
        ops.edit_topk_rows(v, i, grp, r, 64, 4, want_gain=True)
    with pytest.raises(ValueError, match="cur"):
        ops.edit_topk_rows(v, i, grp, r, 64, 4, cur=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="col"):
        ops.edit_topk_rows(v, i, grp, r, 64, 4, cur=cur, col=torch.zeros(2, dtype=torch.int32))    # E_total = 3
    sae = Sae(16, SaeConfig(num_latents=64, k=4))
    with pytest.raises(RuntimeError, match="MI355X"):                       # the encode itself has no CPU path
        sae.encode(torch.zeros(2, 16), edits=e)
    with pytest.raises(RuntimeError, match="MI355X"):
        sae.intervene(torch.zeros(2, 16), e)
    with pytest.raises(ValueError):                                         # a threshold encode takes no edits
        sae.encode(torch.zeros(2, 16), edits=e, threshold=0.5)
    assert hasattr(torch.ops.msae, "edit_topk_valued") and hasattr(torch.ops.msae, "edit_topk_rows_valued")


def test_fake_impl_shapes():
    from msae import ops  # noqa: F401  (registers the ops)
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        e32 = lambda *s: torch.empty(*s, dtype=torch.int32)
        for want_gain in (True, False):
            v, i, g = torch.ops.msae.edit_topk_valued(torch.empty(3, 5, 40), torch.empty(3, 5, 40, dtype=torch.int64), e32(8),
                                                      torch.empty(8), e32(8), torch.empty(3, 5, 8), None, 1000, 32, want_gain)
            assert v.shape == (3, 5, 32) and v.dtype == torch.float32 and i.shape == (3, 5, 32) and i.dtype == torch.int64
            assert g.shape == (3, 5, 32 if want_gain else 0) and g.dtype == torch.float32
            v, i, ed, g = torch.ops.msae.edit_topk_rows_valued(torch.empty(3, 5, 40), e32(3, 5, 40), e32(3, 5), e32(3), e32(9),
                                                               torch.empty(9), e32(9), torch.empty(3, 5, 4), e32(9), 6, 1000, 32,
                                                               not want_gain, want_gain)
            assert v.shape == (3, 5, 32) and i.dtype == torch.int32 and ed.dtype == torch.uint8
            assert ed.shape == (3, 5, 0 if want_gain else 32) and g.shape == (3, 5, 32 if want_gain else 0)


def test_hook_modes_on_the_host():
    from msae import Sae, SaeConfig
    from msae.features import RowEdits, clamp_features_max, clamp_features_rows
    from msae.features.steering import SteeringController
    from msae.features.edits import EDIT_CAP, EDIT_SCALE, EDIT_SET
    from msae.features.hooks import _steering_edits
    from msae.launch.features.steering import parse_argument

    sae = Sae(16, SaeConfig(num_latents=64, k=4))
    layer = torch.nn.Identity()
    assert _steering_edits(sae, 3, 2.0) == (3, None)                        # "set" on an int: the in-kernel scalar route
    for mode, kind in (("scale", 2), ("add", 3), ("floor", 4), ("cap", 5)):
        for feature, feats in ((3, (3,)), ([3, 9], (3, 9)), ({9: 1.0, 3: 0.5}, (3, 9)), (torch.tensor([9, 3]), (3, 9))):
            sf, ed = _steering_edits(sae, feature, 2.0, mode)
            assert sf == -1 and ed.features == feats and ed.kinds == (kind,) * len(feats) and ed.value_dependent
        for h in clamp_features_max(sae, 3, layer, k=2.0, mode=mode) + \
                clamp_features_max(sae, [3, 5], layer, k=2.0, mode=mode, preserve_error=True):
            h.remove()
    with pytest.raises(ValueError, match="mode"):
        clamp_features_max(sae, 3, layer, mode="multiply")
    with pytest.raises(ValueError, match="mode"):
        clamp_features_rows(sae, [3, 4], layer, mode=["scale"])             # one mode per row
    with pytest.raises(ValueError, match="mode"):
        clamp_features_rows(sae, [3, 4], layer, mode=["scale", "x"])
    hs = clamp_features_rows(sae, [3, None, {4: 0.5, 9: 1.0}, [5, 6]], layer, k=2.0, mode=["scale", "add", "cap", "set"])
    ed = hs[0].edits
    assert isinstance(ed, RowEdits) and ed.kind.tolist() == [EDIT_SCALE, EDIT_CAP, EDIT_CAP, EDIT_SET, EDIT_SET]
    assert ed.offsets.tolist() == [0, 1, 1, 3, 5] and ed.union.tolist() == [3, 4, 9] and ed.value_dependent
    hs[0].remove()

    class Engine:                                                           # not an Sae: a feature-sharded engine's interface
        pass

    for feature in (3, [3, 5]):
        with pytest.raises(NotImplementedError, match="single-GPU msae.Sae"):
            clamp_features_max(Engine(), feature, layer, mode="scale")
    for h in clamp_features_max(Engine(), 3, layer, mode="set"):            # the scalar route is open to an engine, as before
        h.remove()
    ctl = SteeringController.__new__(SteeringController)
    with pytest.raises(NotImplementedError, match="single-GPU msae.Sae"):
        SteeringController.__init__(ctl, Engine(), "m", [1], None, None, "p", mode="scale")
    with pytest.raises(ValueError, match="mode"):
        SteeringController.__init__(ctl, sae, "m", [1], None, None, "p", mode="x")
    assert parse_argument(["-t", "q"]).steer_mode == "set"
    assert parse_argument(["-t", "q", "--steer-mode", "scale"]).steer_mode == "scale"
    with pytest.raises(SystemExit):
        parse_argument(["-t", "q", "--steer-mode", "scale", "--shard-sae"])


def test_symbols_and_argument_errors_of_the_entry_points():
    from msae import _hip

    lib = ctypes.CDLL(str(_hip.LIB_PATH))
    names = ("msae_edit_topk_valued_f32", "msae_edit_topk_valued_i64_f32", "msae_edit_topk_rows_valued_f32",
             "msae_edit_topk_rows_valued_i64_f32")
    for name in names:
        assert hasattr(lib, name), name
        assert name in _hip.PROTOTYPES
    L = _hip.load()
    assert L.msae_abi_version() == 4 == _hip.ABI_VERSION
    p = ctypes.c_void_p(16)                                                 # never dereferenced: every call below is refused
    for fn in (L.msae_edit_topk_valued_f32, L.msae_edit_topk_valued_i64_f32):
        ok = dict(T=4, kk=40, E=3, N=1000, k=8, cur=p, ld=4)
        for bad in (dict(cur=None), dict(ld=0), dict(kk=10), dict(E=0), dict(k=0), dict(N=10), dict(T=-1), dict(k=4094, kk=5000)):
            a = {**ok, **bad}
            assert fn(p, p, a["T"], a["kk"], p, p, p, a["E"], a["N"], a["k"], a["cur"], a["ld"], None, p, p, None, None) == -1, bad
        assert fn(p, p, 0, 40, p, p, p, 3, 1000, 8, p, 4, None, p, p, None, None) == 0      # T == 0 does nothing
    for fn in (L.msae_edit_topk_rows_valued_f32, L.msae_edit_topk_rows_valued_i64_f32):
        ok = dict(T=4, kk=40, G=2, Et=5, Em=3, N=1000, k=8, cur=p, ld=4)
        for bad in (dict(cur=None), dict(ld=0), dict(kk=10), dict(Em=0), dict(G=0), dict(k=0), dict(N=10), dict(T=-1), dict(Et=-1)):
            a = {**ok, **bad}
            assert fn(p, p, a["T"], a["kk"], p, p, a["G"], p, p, p, a["Et"], a["Em"], a["N"], a["k"], a["cur"], a["ld"], None,
                      p, p, None, None, None) == -1, bad
        assert fn(p, p, 0, 40, p, p, 2, p, p, p, 5, 3, 1000, 8, p, 4, None, p, p, None, None, None) == 0
