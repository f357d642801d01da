"""Value-dependent latent edits on the HIP path (FeatureEdits(scale=, add=, floor=, cap=); ops.edit_topk(cur=),
ops.edit_topk_rows(cur=), Sae.encode / Sae.intervene, the autograd node, the hooks' `mode`) against the numpy restatement
tests/value_edits_ref.py -- dense latents from oracle.pre_acts, one float32 operation per edited column, lexsort -- BIT FOR
BIT unless a test says otherwise.  The op-level tests run on synthetic lists (N = 512, no encoder) and walk the three kernel
layouts; the Sae-level tests use test_gpu_edits' shapes (d = 256, N = 8192), inputs and degenerate rows, and run under
torch.cuda.set_sync_debug_mode("error")."""
import contextlib

import numpy as np
import pytest
import torch

import intervene_ref as iref
import test_gpu_edits as tge
import test_intervene_host as tih
import value_edits_ref as vref
from test_gpu_edits import dev, tiny  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

D, N = tge.D, tge.N
DTYPES = tge.DTYPES
N_OP = 512


@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _assert_bits(got, ref, what=""):
    gi, gv = got[1].cpu().numpy(), got[0].cpu().numpy()
    assert np.array_equal(gi.reshape(ref[1].shape), ref[1]), f"indices differ {what}"
    assert np.array_equal(vref.bits(gv).reshape(ref[0].shape), vref.bits(ref[0])), f"values differ {what}"
    if len(got) > 2:
        assert np.array_equal(vref.bits(got[2].cpu().numpy()).reshape(ref[2].shape), vref.bits(ref[2])), f"gain differs {what}"


# ---- the ops on synthetic lists --------------------------------------------------------------------------------------------
_SYN = {}


def _synthetic(T):
    """Dense latents [T, 512]: multiples of 1/8 in [0, 4) (ties), 40 % zeros, row 1 (T >= 5) all zero, row 2 three positives."""
    if T not in _SYN:
        rng = np.random.default_rng(900 + T)
        L = (rng.integers(1, 32, size=(T, N_OP)) / 8.0).astype(np.float32)
        L[rng.random((T, N_OP)) < 0.4] = 0
        if T >= 5:
            L[1] = 0
            L[2] = 0
            L[2, [7, 300, 511]] = (0.5, 2.0, 0.5)
        _SYN[T] = L
    return _SYN[T]


def _table(rng, L, E):
    """A random table of E distinct features over all six kinds -> value_edits_ref.merge's keyword arguments."""
    feats = rng.permutation(N_OP)[:E]
    names = ("scale", "add", "floor", "cap", "set", "zero")
    kw = {}
    for j, f in enumerate(feats.tolist()):
        name = names[(j + int(rng.integers(6))) % 6] if j >= 6 else names[j]
        par = {"scale": rng.choice([-1.0, 0.0, 0.5, 2.0, 3.0]), "add": rng.choice([-4.0, -0.5, 0.25, 1.0]),
               "floor": rng.choice([0.0, 0.5, 2.0, 3.875]), "cap": rng.choice([0.0, 0.125, 1.0, 5.0]),
               "set": rng.choice([-1.0, 0.0, 1.5, float(L.max())]), "zero": 0.0}[name]
        if name == "zero":
            kw.setdefault("zero", []).append(f)
        else:
            kw.setdefault(name, {})[f] = float(par)
    return kw


def _poisoned_list(L, k, e_max, extra, wide, dev):
    """The canonical top-(k + e_max) list with `extra` poisoned columns behind it (NaN values, hostile indices)."""
    lv, li = vref.canonical_topk(L, k + e_max)
    T = L.shape[0]
    lv = np.concatenate([lv, np.full((T, extra), np.nan, np.float32)], 1)
    li = np.concatenate([li.astype(np.int64), np.full((T, extra), 2**31 - 1, np.int64)], 1)
    li[:, k + e_max::2] = -7
    return torch.from_numpy(lv).to(dev), torch.from_numpy(li).to(dev, torch.int64 if wide else torch.int32)


# (k, E_max): next_pow2(k + 2 E_max) = 8 (one register per lane), 128, 256, 512 (the workgroup layout of the rows form)
LAYOUTS = [(4, 1), (32, 40), (32, 100), (32, 150)]


@pytest.mark.parametrize("k,E", LAYOUTS)
@pytest.mark.parametrize("T", [1, 5, 300])
def test_op_one_table_equals_the_restatement(dev, T, k, E):
    from msae import ops
    from msae.features import FeatureEdits

    L = _synthetic(T)
    rng = np.random.default_rng(10 * E + T)
    kw = _table(rng, L, E)
    feats, vals, kinds = vref.merge(**kw)
    ed = FeatureEdits(N_OP, device=dev, **kw)
    ref = vref.dense_topk(L, k, feats, vals, kinds)
    cur = torch.from_numpy(np.ascontiguousarray(L[:, feats])).to(dev)
    perm = torch.from_numpy(rng.permutation(E))
    wide_cur = torch.full((T, E + 5), float("nan"))
    wide_cur[:, perm] = torch.from_numpy(np.ascontiguousarray(L[:, feats]))
    wide_cur[:, perm[torch.from_numpy(kinds < 2)]] = float("nan")         # SET / ZERO entries read no latent
    wide_cur, perm = wide_cur.to(dev), perm.to(dev, torch.int32)
    for wide in (False, True):
        lv, li = _poisoned_list(L, k, E, 3, wide, dev)
        got = ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N_OP, k, cur=cur, want_gain=True)
        assert got[1].dtype == li.dtype
        _assert_bits(got, ref, f"col=None wide={wide}")
        _assert_bits(ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N_OP, k, cur=wide_cur, col=perm, want_gain=True), ref,
                     f"permuted wide={wide}")
        _assert_bits(ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N_OP, k, cur=wide_cur[:, :E + 2], col=perm), ref,
                     "a column-sliced view, no gain")
    # a SET / ZERO-only table through the valued kernel: the unvalued kernel's bits, `cur` (all NaN) is not read
    kw0 = {name: spec for name, spec in kw.items() if name in ("set", "zero")}
    if not kw0:
        return
    e0 = FeatureEdits(N_OP, device=dev, **kw0)
    lv, li = _poisoned_list(L, k, e0.E, 2, True, dev)
    a = ops.edit_topk(lv, li, e0.feat, e0.val, e0.kind, N_OP, k)
    b = ops.edit_topk(lv, li, e0.feat, e0.val, e0.kind, N_OP, k, cur=torch.full((T, 1), float("nan"), device=dev), want_gain=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(b[2], (~torch.isin(b[1], e0.feat.long())).float())


@pytest.mark.parametrize("k,E", LAYOUTS)
@pytest.mark.parametrize("T", [1, 5, 300])
def test_op_rows_equals_the_restatement_and_the_one_table_call(dev, T, k, E):
    """Groups: a table of E_max entries, an empty group, tables of 8 and 9 entries (the scan / search switch) where E_max
    allows, one entry; group ids outside [0, G) copy.  Every group's rows equal the one-table call with that table."""
    from msae import ops
    from msae.features import FeatureEdits, RowEdits

    L = _synthetic(T)
    rng = np.random.default_rng(20 * E + T)
    kws = [_table(rng, L, E), None] + ([_table(rng, L, 8), _table(rng, L, 9)] if E >= 9 else []) + [_table(rng, L, 1)]
    r = RowEdits(N_OP, kws, device=dev)
    assert r.E_max == E
    G = r.G
    ids = np.array(list(range(G)) + [-1, G, 2**31 + 3, -2**40], dtype=np.int64)
    group_of = ids[(np.arange(T) * 5 + (np.arange(T) // 7)) % len(ids)] if T > 1 else ids[:1]
    tables = [None if kw is None else vref.merge(**kw) for kw in kws]
    ref = vref.dense_topk_rows(L, k, np.clip(group_of, -1, G), tables)
    union = r.union.cpu().numpy()
    cur_np = np.full((T, len(union) + 3), np.nan, np.float32)
    cur_np[:, :len(union)] = L[:, union]
    for t in range(T):                                                     # a token's row holds its own table's columns only
        gid = int(np.clip(group_of[t], -1, G))
        mine = tables[gid][0][tables[gid][2] >= 2] if 0 <= gid < G and tables[gid] is not None else []
        cur_np[t, :len(union)][~np.isin(union, mine)] = np.nan
    cur = torch.from_numpy(cur_np).to(dev)
    for wide in (False, True):
        lv, li = _poisoned_list(L, k, E, 3, wide, dev)
        go = torch.from_numpy(group_of).to(dev)
        v, i, ed, g = ops.edit_topk_rows(lv, li, go, r, N_OP, k, want_mask=True, cur=cur, col=r.col, want_gain=True)
        _assert_bits((v, i, g), ref, f"wide={wide}")
        go32 = torch.from_numpy(np.clip(group_of, -1, G).astype(np.int32)).to(dev)
        v2, i2 = ops.edit_topk_rows(lv, li, go32, r, N_OP, k, cur=cur, col=r.col)
        assert torch.equal(i2, i) and torch.equal(v2.view(torch.int32), v.view(torch.int32))
        for gid, kw in enumerate(kws):
            rows = np.nonzero(group_of == gid)[0]
            if not len(rows):
                continue
            sel = torch.from_numpy(rows).to(dev)
            if kw is None:
                assert torch.equal(i[sel], li[sel, :k]) and torch.equal(v[sel].view(torch.int32), lv[sel, :k].view(torch.int32))
                assert (g[sel] == 1).all() and (ed[sel] == 0).all()
                continue
            e = FeatureEdits(N_OP, device=dev, **kw)
            one = ops.edit_topk(lv[sel], li[sel], e.feat, e.val, e.kind, N_OP, k,
                                cur=torch.from_numpy(np.ascontiguousarray(L[rows][:, tables[gid][0]])).to(dev), want_gain=True)
            assert torch.equal(one[1], i[sel]) and torch.equal(one[0].view(torch.int32), v[sel].view(torch.int32)), gid
            assert torch.equal(one[2], g[sel]), gid
            assert torch.equal(ed[sel].bool(), torch.isin(i[sel].long(), e.feat.long())), gid
        out = np.nonzero((group_of < 0) | (group_of >= G))[0]
        if len(out):
            sel = torch.from_numpy(out).to(dev)
            assert torch.equal(i[sel], li[sel, :k]) and (g[sel] == 1).all() and (ed[sel] == 0).all()
    # col=None: entry e of the concatenated table reads column e
    lv, li = _poisoned_list(L, k, E, 0, True, dev)
    cols = torch.from_numpy(np.ascontiguousarray(L[:, r.feat.cpu().numpy()])).to(dev)
    _assert_bits(ops.edit_topk_rows(lv, li, torch.from_numpy(group_of).to(dev), r, N_OP, k, cur=cols, want_gain=True), ref)


# ---- Sae.encode ------------------------------------------------------------------------------------------------------------
def _edits(dev, kw):
    from msae.features import FeatureEdits

    return FeatureEdits(N, device=dev, **kw)


def _encode_checked(sae, x, **kw):
    """The call once to warm (workspaces, prepared operands), then again with host synchronisation an error."""
    with torch.no_grad():
        sae.encode(x, **kw)
        with no_sync():
            return sae.encode(x, **kw)


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("E", [1, 3, 50])
@pytest.mark.parametrize("k", [4, 32])
@pytest.mark.parametrize("T", [1, 5, 40, 300])
def test_encode_equals_the_dense_definition(dev, T, k, E, dtype):
    sae = tge._sae(dev, k)
    xt, L, order = tge._inputs(T, dtype)
    kw = vref.plan(L, order, k, E)
    ed = _edits(dev, kw)
    assert ed.E == E and ed.value_dependent
    ref = vref.dense_topk(L, k, *vref.merge(**kw))
    top = _encode_checked(sae, xt.to(dev), edits=ed)
    assert top.top_indices.dtype == torch.int64 and top.top_acts.shape == (T, k)
    _assert_bits((top.top_acts, top.top_indices), ref, f"T={T} k={k} E={E} {dtype}")
    far = int(order[0][k + E + 5])                                          # from beyond the over-fetched list to the top:
    assert ref[1][0, 0] == far and kw["scale"][far] > 1                     # an edit kernel without `cur` cannot place it


def test_planted_cases(dev):
    """Every planted case of value_edits_ref.plan in one table (E = 24), at token 0, and the degenerate rows."""
    for k in (4, 32):
        E = 24
        sae = tge._sae(dev, k)
        xt, L, order = tge._inputs(40, "bf16")
        kw = vref.plan(L, order, k, E, seed=5)
        ref = vref.dense_topk(L, k, *vref.merge(**kw))
        top = _encode_checked(sae, xt.to(dev), edits=_edits(dev, kw))
        _assert_bits((top.top_acts, top.top_indices), ref, f"k={k}")
        with torch.no_grad():
            exact = sae.encode(xt.to(dev), edits=_edits(dev, kw), exact=True)
            cert = sae.encode(xt.to(dev).reshape(2, 20, D), edits=_edits(dev, kw), certified=True)
        _assert_bits((exact.top_acts, exact.top_indices), ref, "exact")
        assert cert.top_acts.shape == (2, 20, k)
        _assert_bits((cert.top_acts, cert.top_indices), ref, "certified, [B, S, d]")
        o0, row, val = order[0], ref[1][0].tolist(), ref[0][0]
        v = lambda r: L[0, o0[r]]
        assert row[0] == int(o0[k + E + 5])                                 # scaled in from beyond rank k + E
        stays_out = [f for f, a in kw["scale"].items() if L[0, f] == 0 and a < 0]
        assert stays_out and stays_out[0] not in row                        # inactive under SCALE
        enters = [f for f, dlt in kw["add"].items() if L[0, f] == 0 and dlt > 0][0]
        assert val[row.index(enters)] == np.float32(kw["add"][enters])      # inactive under ADD: delta itself
        assert int(o0[0]) not in row and kw["add"][int(o0[0])] < 0          # driven below 0: dropped
        capped = int(o0[min(1, k - 1)])
        assert kw["cap"][capped] < v(k - 1) and (capped not in row or val[row.index(capped)] == np.float32(kw["cap"][capped]))
        kept = int(o0[min(2, k - 1)])
        assert kw["floor"][kept] < L[0, kept] and (kept not in row or val[row.index(kept)] == L[0, kept])   # FLOOR below: same bits
        assert k == 4 or kept in row
        tie, with_ = int(o0[k + 1]), int(o0[min(3, k - 1)])
        if tie in row and with_ in row:                                     # FLOOR exactly at a selected value: by index
            a, b = row.index(tie), row.index(with_)
            assert val[a] == val[b] and (a < b) == (tie < with_)
        if k == 32:
            assert tie in row and with_ in row
        assert (ref[0] >= 0).all()


def test_row_edits_every_group_equals_the_one_table_call(dev):
    from msae.features import RowEdits

    k, T = 32, 300
    sae = tge._sae(dev, k)
    xt, L, order = tge._inputs(T, "bf16")
    kws = [vref.plan(L, order, k, 9, seed=1), None, vref.plan(L, order, k, 3, seed=2), dict(set={5: 1.0}, zero=[int(order[0][0])]),
           vref.plan(L, order, k, 50, seed=3)]
    r = RowEdits(N, kws, device=dev)
    assert r.value_dependent and r.E_max == 50
    group_of = np.array([0, 1, 2, 3, 4, -1, 5, 4])[np.arange(T) % 8]
    group_of[:5] = 4                                                        # token 0 and the degenerate rows: the long table
    go = torch.from_numpy(group_of).to(dev)
    x = xt.to(dev)
    top = _encode_checked(sae, x, edits=r, edit_group=go)
    tables = [None if kw is None else vref.merge(**kw) for kw in kws]
    _assert_bits((top.top_acts, top.top_indices), vref.dense_topk_rows(L, k, group_of, tables)[:2])
    with torch.no_grad():
        plain = sae.encode(x)
        for gid, kw in enumerate(kws):
            sel = go == gid
            one = plain if kw is None else sae.encode(x, edits=_edits(dev, kw))
            assert torch.equal(top.top_indices[sel], one.top_indices[sel]), gid
            assert torch.equal(top.top_acts[sel].view(torch.int32), one.top_acts[sel].view(torch.int32)), gid
        sel = (go < 0) | (go >= r.G)
        assert torch.equal(top.top_indices[sel], plain.top_indices[sel])
        # "row b uses group b" on [G, S, d]
        b = sae.encode(x[:5 * 40].reshape(5, 40, D), edits=r)
    _assert_bits((b.top_acts, b.top_indices), vref.dense_topk_rows(L[:200], k, np.repeat(np.arange(5), 40), tables)[:2])


# ---- Sae.intervene ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_intervene_is_delta_decode_on_the_two_lists(dev, dtype):
    from msae import ops
    from msae.features import RowEdits

    k, T, E = 32, 40, 24
    sae = tge._sae(dev, k)
    W_dec = tge._w()[2]
    xt, L, order = tge._inputs(T, dtype)
    x = xt.to(dev)
    kw = vref.plan(L, order, k, E)
    ed = _edits(dev, kw)
    Q = vref.dense_topk(L, k, *vref.merge(**kw))[:2]
    P = vref.canonical_topk(L, k)
    with torch.no_grad():
        sae.intervene(x, ed)
        with no_sync():
            out = sae.intervene(x, ed)
        p, q = sae.encode(x), sae.encode(x, edits=ed)
        want = ops.delta_decode(x, p.top_acts, p.top_indices, q.top_acts, q.top_indices, sae.W_dec)
    bits = tih.TORCH_BITS[dtype]
    assert out.dtype == x.dtype and torch.equal(out.view(bits), want.view(bits))
    xb = tih.x_bits(xt, dtype)
    xf = iref.to_f32(xb, dtype)
    got = tih.x_bits(out, dtype)
    err = np.abs(iref.values_f64(got, dtype) - iref.composed_f64(xf, *P, *Q, W_dec))
    assert (err <= iref.bound(xf, dtype, *P, *Q, W_dec)).all()
    assert not np.array_equal(got[0], xb[0])                                # token 0 moved
    # per-token tables: the tokens no table touches keep the input's bits
    r = RowEdits(N, [kw, None, vref.plan(L, order, k, 3, seed=2)], device=dev)
    group_of = np.array([0, 1, 2, -1, 3])[np.arange(T) % 5]
    with torch.no_grad():
        out = sae.intervene(x, r, torch.from_numpy(group_of).to(dev))
        q = sae.encode(x, edits=r, edit_group=torch.from_numpy(group_of).to(dev))
        want = ops.delta_decode(x, p.top_acts, p.top_indices, q.top_acts, q.top_indices, sae.W_dec)
    assert torch.equal(out.view(bits), want.view(bits))
    keep = torch.from_numpy(~np.isin(group_of, [0, 2])).to(dev)
    assert keep.any() and torch.equal(out[keep].view(bits), x[keep].view(bits))
    assert not torch.equal(out[~keep].view(bits), x[~keep].view(bits))


# ---- autograd --------------------------------------------------------------------------------------------------------------
def _legacy_edit(lat, ed):
    """pre_acts -> torch `*`, `+`, clamp on the edited columns (SET / ZERO: constants, no gradient)."""
    feats = torch.tensor(ed.features, device=lat.device)
    cols = []
    for f, v, kd in zip(ed.features, ed.values, ed.kinds):
        c = lat[:, f]
        cols.append({0: torch.full_like(c, v), 1: torch.zeros_like(c), 2: c * v, 3: c + v, 4: torch.clamp(c, min=v),
                     5: torch.clamp(c, max=v)}[kd])
    return lat.index_copy(1, feats, torch.stack(cols, 1))


def _grads(sae, x0, route, ed, group=None, eds=None):
    params = (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)
    x = x0.clone().requires_grad_()
    if route == "fused":
        top = sae.encode(x, edits=ed, edit_group=group)
        assert top.top_acts.requires_grad
    else:
        lat = sae.pre_acts(x)
        if eds is None:
            lat = _legacy_edit(lat, ed) if ed is not None else lat
        else:                                                              # per-token tables: each group's rows with its table
            parts = [(_legacy_edit(lat, e) if e is not None else lat) for e in eds]
            sel = torch.stack([group == g for g in range(len(eds))], 0)
            new = lat
            for g, part in enumerate(parts):
                new = torch.where(sel[g][:, None], part, new)
            lat = new
        top = sae.select_topk(lat)
    out = sae.decode(top.top_acts, top.top_indices)
    (out * torch.linspace(-1, 1, D, device=x.device)).sum().backward()
    grads = [x.grad.clone()] + [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    return grads, top.top_indices.detach()


def _assert_grads_close(a, b):
    for ga, gb, nm in zip(a, b, ("x", "W_enc", "b_enc", "W_dec", "b_dec")):
        assert gb.abs().max() > 0, nm
        assert (ga - gb).abs().max().item() <= 2e-3 * gb.abs().max().item() + 1e-8, nm


def test_autograd_matches_the_legacy_seam(dev):
    from msae.features import RowEdits

    k, E, T = 32, 24, 40
    sae = tge._make_sae(dev, D, N, k, tge._w())
    xt, L, order = tge._inputs(T, "f32")
    x0 = xt.to(dev)
    kw = vref.plan(L, order, k, E)
    kw["set"] = {f: v + float(L.max()) for f, v in kw["set"].items()}      # selected everywhere: SET slots meet the zero gain
    ed = _edits(dev, kw)
    fused, fi = _grads(sae, x0, "fused", ed)
    legacy, li = _grads(sae, x0, "legacy", ed)
    assert torch.equal(fi.sort(-1).values, li.sort(-1).values)
    _assert_grads_close(fused, legacy)
    const = torch.tensor([f for f, kd in zip(ed.features, ed.kinds) if kd < 2], device=dev)
    assert torch.isin(fi, const).any()                                      # SET / ZERO slots were selected ...
    assert (fused[1][const] == 0).all() and (fused[2][const] == 0).all()    # ... and their encoder rows get exactly 0
    dep = torch.tensor([f for f, kd in zip(ed.features, ed.kinds) if kd >= 2], device=dev)
    assert (fused[1][dep] != 0).any()                                       # a value-dependent edit carries gradient
    # per-token tables through the same node
    kws = [kw, None, vref.plan(L, order, k, 3, seed=2)]
    r = RowEdits(N, kws, device=dev)
    group = torch.from_numpy(np.array([0, 1, 2, -1])[np.arange(T) % 4]).to(dev)
    fused, fi = _grads(sae, x0, "fused", r, group)
    legacy, li = _grads(sae, x0, "legacy", None, group, [None if w is None else _edits(dev, w) for w in kws])
    assert torch.equal(fi.sort(-1).values, li.sort(-1).values)
    _assert_grads_close(fused, legacy)


def test_a_scaled_row_gets_alpha_times_the_gradient(dev):
    """One token, its top feature scaled by 2: the selection is the same set, the loss is linear in the latents, so the
    feature's encoder row and bias get exactly twice the unedited run's gradient, every other row the same one."""
    k = 32
    sae = tge._make_sae(dev, D, N, k, tge._w())
    xt, L, order = tge._inputs(1, "f32")
    f = int(order[0][0])
    assert L[0, f] > 0
    x0 = xt.to(dev)
    plain, pi = _grads(sae, x0, "legacy", None)
    scaled, si = _grads(sae, x0, "fused", _edits(dev, {"scale": {f: 2.0}}))
    assert torch.equal(pi.sort(-1).values, si.sort(-1).values)
    for j in (1, 2):                                                        # W_enc, b_enc
        want = plain[j].clone()
        want[f] = 2.0 * want[f]
        assert plain[j][f].abs().max() > 0
        assert (scaled[j] - want).abs().max().item() <= 2e-3 * want.abs().max().item() + 1e-8


# ---- hooks -----------------------------------------------------------------------------------------------------------------
def _legacy_steer(sae, h, ed):
    """The reference's steering hook body (steering.py:111-118) with the value-dependent edit in torch on the dense seam."""
    latents = sae.pre_acts(h)
    if latents.shape[1] != 1 and ed is not None:
        for f, v, kd in zip(ed.features, ed.values, ed.kinds):
            c = latents[:, :, f]
            latents[:, :, f] = {0: torch.full_like(c, v), 1: torch.zeros_like(c), 2: c * v, 3: c + v, 4: torch.clamp(c, min=v),
                                5: torch.clamp(c, max=v)}[kd]
    top_acts, top_indices = sae.select_topk(latents)
    return sae.decode(top_acts[0], top_indices[0]).unsqueeze(0).to(torch.float16)


def test_hooks_on_the_fake_model_equal_the_legacy_seam(dev, tiny):
    from msae.features import FeatureEdits, clamp_features_max, clamp_features_rows

    g, model, sae, inputs = tiny
    layer = model.language_model.get_submodule(str(g["module"]))
    active = g["clean_top_idx"]
    feats = sorted(set(active[1][:3].tolist() + [int(active[4][0]), 5, 1000]))
    n = sae.num_latents
    seen = {}
    probe = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o[0].detach().clone()))
    ids = inputs["input_ids"][:1]
    top = int(active[1][0])
    with torch.no_grad():
        model(input_ids=ids)
        peak = float(sae.pre_acts(seen["h"]).max())                        # a floor above it enters every token's top-k
    cases = [(dict(feature=top, k=4.0, mode="scale"), dict(scale={top: 4.0})),
             (dict(feature=feats, k=4.0, mode="scale"), dict(scale={f: 4.0 for f in feats})),
             (dict(feature={f: 0.5 + j for j, f in enumerate(feats)}, mode="add"), dict(add={f: 0.5 + j for j, f in enumerate(feats)})),
             (dict(feature=feats, k=0.75, mode="floor"), dict(floor={f: 0.75 for f in feats})),
             (dict(feature=feats, k=2.0 * peak, mode="floor"), dict(floor={f: 2.0 * peak for f in feats})),
             (dict(feature=feats, k=0.05, mode="cap"), dict(cap={f: 0.05 for f in feats}))]
    six = list(dict.fromkeys(active[1][:3].tolist() + [int(active[4][0]), 5, 1000, 6, 1001]))[:6]
    mixed = dict(scale={six[0]: 3.0}, add={six[1]: -0.25}, cap={six[2]: 0.1}, floor={six[4]: 1.0}, set={six[5]: 2.0}, zero=[six[3]])
    cases.append((dict(feature=FeatureEdits(n, device=dev, **mixed)), mixed))
    try:
        for call, kw in cases:
            handles = clamp_features_max(sae, call.pop("feature"), layer, **call)
            after = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o[0].detach().clone()))
            with torch.no_grad():
                model(input_ids=ids)
                want = _legacy_steer(sae, seen["h"], FeatureEdits(n, device="cpu", **kw))
                plain = _legacy_steer(sae, seen["h"], None)
            for h in handles + [after]:
                h.remove()
            assert seen["out"].dtype == torch.float16 and torch.equal(seen["out"].view(torch.int16), want.view(torch.int16)), call
            if call.get("mode") in ("scale", "add") or call.get("k", 0) > peak:
                assert not torch.equal(want, plain), call                  # (a low floor or a cap may leave this prompt alone)
        # another mode per batch row, a row of None
        features = [int(active[1][0]), None, feats, {int(active[4][0]): 1.5, 7: 3.0}]
        modes = ["scale", "add", "cap", "floor"]
        kws = [{"scale": {features[0]: 0.5}}, None, {"cap": {f: 0.5 for f in feats}}, {"floor": features[3]}]
        handles = clamp_features_rows(sae, features, layer, k=0.5, mode=modes)
        after = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o[0].detach().clone()))
        with torch.no_grad():
            model(input_ids=ids.repeat(len(features), 1))
            want = torch.cat([_legacy_steer(sae, seen["h"][b:b + 1], None if kw is None else FeatureEdits(n, device="cpu", **kw))
                              for b, kw in enumerate(kws)])
        for h in handles + [after]:
            h.remove()
        assert torch.equal(seen["out"].view(torch.int16), want.view(torch.int16))
        assert not torch.equal(seen["out"][0], seen["out"][1])
    finally:
        probe.remove()


def test_argument_errors_on_the_device(dev):
    from msae import _hip, ops
    from msae.features import FeatureEdits, clamp_features_max
    from msae.parallel import EmulatedShardGroup

    lib = _hip.load()
    v = torch.zeros(4, 64, device=dev)
    i32 = torch.zeros(4, 64, dtype=torch.int32, device=dev)
    e = torch.zeros(97, dtype=torch.int32, device=dev)
    ev = torch.zeros(97, device=dev)
    cur = torch.zeros(4, 100, device=dev)
    o = torch.zeros(4, 4000, device=dev)
    oi = torch.zeros(4, 4000, dtype=torch.int32, device=dev)
    p = _hip.ptr

    def call(kk, E, n, k, c=cur, ld=100):
        return lib.msae_edit_topk_valued_f32(p(v), p(i32), 4, kk, p(e), p(ev), p(e), E, n, k, p(c) if c is not None else None, ld,
                                             None, p(o), p(oi), None, None)

    assert call(10, 3, 1000, 8) == -1          # kk < k + E
    assert call(64, 30, 40, 32) == -1          # k + E > N
    assert call(5000, 97, 8192, 4000) == -1    # k + E > 4096
    assert call(64, 3, 1000, 8, c=None) == -1  # no cur
    assert call(64, 3, 1000, 8, ld=0) == -1    # ld_cur < 1
    torch.cuda.synchronize()
    sae = tge._sae(dev, 32)
    ed = FeatureEdits(N, scale={1: 2.0, 2: 3.0}, device=dev)
    x = torch.zeros(4, D, device=dev)
    with pytest.raises(NotImplementedError, match="Sae"):
        EmulatedShardGroup(sae, 2).encode(x, edits=ed)
    with pytest.raises(NotImplementedError, match="single-GPU msae.Sae"):
        clamp_features_max(EmulatedShardGroup(sae, 2), 3, torch.nn.Identity(), mode="scale")
    with pytest.raises(ValueError):
        sae.encode(x, edits=ed, set_feature=3)
    with pytest.raises(ValueError):
        sae.encode(x, edits=FeatureEdits(N, scale={1: 2.0}, device="cpu"))   # lives on another device
    with pytest.raises(ValueError):
        sae.encode(x, edits=ed, threshold=0.5)
    lv, li = torch.zeros(4, 40, device=dev), torch.zeros(4, 40, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="cur"):
        ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N, 32, cur=torch.zeros(4, 2))              # cur on the host
    with pytest.raises(ValueError, match="cur"):
        ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N, 32, cur=torch.zeros(5, 2, device=dev))
    with pytest.raises(ValueError, match="col"):
        ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N, 32, cur=torch.zeros(4, 2, device=dev),
                      col=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N, 32, cur=torch.zeros(4, 2, device=dev, requires_grad=True))
    # a hostile column is clamped, not followed: the call completes and stays inside `cur`
    got = ops.edit_topk(lv, li, ed.feat, ed.val, ed.kind, N, 32, cur=torch.ones(4, 2, device=dev),
                        col=torch.tensor([-5, 2**31 - 1], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert got[0].shape == (4, 32)
