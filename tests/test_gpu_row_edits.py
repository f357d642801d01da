"""Per-token latent edits on the HIP path (Sae.encode(edits=RowEdits, edit_group=...), ops.edit_topk_rows, clamp_features_rows,
the batched controller and attribution) against the numpy restatement tests/row_edits_ref.py -- each token's table applied
to its dense row, oracle.topk -- BIT FOR BIT unless a test says otherwise.  Shapes, weights, inputs and the planted edit
positions are tests/test_gpu_edits.py's (D = 256, N = 8192: the smallest width with the fused pass; rows 1-3 degenerate)."""
import numpy as np
import pytest
import torch

import edits_ref as eref
import fakes
import row_edits_ref as rref
import synth
import test_gpu_edits as tge
from oracle import oracle

pytestmark = pytest.mark.gpu

D, N = tge.D, tge.N
# group sizes: at k = 32 the long config needs 64, 64, 64, 256 and 512 keys, and E_max = 150 sends the WHOLE call through the
# workgroup layout; the short config stays in the register layout (E_max = 3)
CONFIGS = {"long": (0, 1, 3, 50, 150), "short": (1, 1, 3)}


tiny = tge.tiny                # (the fake model + g8's Sae and inputs; built on this module's `dev`)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


def _group_of(T, G):
    """Round-robin over the groups; every fifth token unedited (-1)."""
    out, g = np.empty(T, dtype=np.int32), 0
    for t in range(T):
        if t % 5 == 4:
            out[t] = -1
        else:
            out[t], g = g % G, g + 1
    return out


def _specs(L, order, k, sizes):
    specs = []
    for g, E in enumerate(sizes):
        if E == 0:
            specs.append(None)
            continue
        s, z = tge._plan(L, order, k, E, seed=g)
        specs.append({"set": s or None, "zero": z or None})
    return specs


def _row_edits(dev, specs, n=N):
    from msae.features import RowEdits

    return RowEdits(n, specs, device=dev)


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("k", [4, 32])
@pytest.mark.parametrize("T", [1, 5, 40, 300])
def test_encode_with_row_edits_equals_the_dense_definition(dev, T, k, dtype):
    sae = tge._sae(dev, k)
    xt, L, order = tge._inputs(T, dtype)
    x = xt.to(dev)
    with torch.no_grad():
        plain = sae.encode(x)
    for name, sizes in CONFIGS.items():
        specs = _specs(L, order, k, sizes)
        groups = rref.merge_groups(specs)
        assert [0 if g is None else len(g[0]) for g in groups] == list(sizes)
        group_of = _group_of(T, len(sizes))
        ed = _row_edits(dev, specs)
        assert (ed.G, ed.E_max, ed.E_total) == (len(sizes), max(sizes), sum(sizes))
        ref_v, ref_i = rref.dense_topk_rows(L, k, groups, group_of)
        with torch.no_grad():
            top, status = sae.encode(x, edits=ed, edit_group=torch.from_numpy(group_of).to(dev), return_status=True)
        assert top.top_indices.dtype == torch.int64 and top.top_acts.shape == (T, k) and status.shape == (T,)
        tge._assert_bits(top.top_acts, top.top_indices, ref_v, ref_i, f"{name} T={T} k={k} {dtype}")
        plain_rows = torch.from_numpy(np.array([rref.table_of(groups, g) is None for g in group_of])).to(dev)
        assert torch.equal(top.top_indices[plain_rows], plain.top_indices[plain_rows])
        assert torch.equal(top.top_acts[plain_rows].view(torch.int32), plain.top_acts[plain_rows].view(torch.int32))


@pytest.mark.parametrize("T", [5, 300])
def test_each_group_equals_the_sibling_with_that_table(dev, T):
    from msae.features import FeatureEdits

    k = 32
    sae = tge._sae(dev, k)
    xt, L, order = tge._inputs(T, "bf16")
    x = xt.to(dev)
    for sizes in CONFIGS.values():
        specs = _specs(L, order, k, sizes)
        group_of = torch.from_numpy(_group_of(T, len(sizes))).to(dev)
        with torch.no_grad():
            top = sae.encode(x, edits=_row_edits(dev, specs), edit_group=group_of)
            for g, spec in enumerate(specs):
                rows = group_of == g
                if spec is None or not bool(rows.any()):
                    continue
                one = sae.encode(x, edits=FeatureEdits(N, device=dev, **spec))
                assert torch.equal(top.top_indices[rows], one.top_indices[rows]), g
                assert torch.equal(top.top_acts[rows].view(torch.int32), one.top_acts[rows].view(torch.int32)), g
    o0 = order[0]
    all0 = torch.zeros(T, dtype=torch.int64, device=dev)
    with torch.no_grad():                                                  # one group of one edit: the scalar arguments
        for f in (int(o0[0]), int(o0[k]), 0, 4000):
            for kw, spec in ((dict(zero_feature=f), dict(zero=[f])),
                             (dict(set_feature=f, set_value=float(L[0, o0[1]])), dict(set={f: float(L[0, o0[1]])})),
                             (dict(set_feature=f, set_value=-1.0), dict(set={f: -1.0}))):
                a = sae.encode(x, **kw)
                b = sae.encode(x, edits=_row_edits(dev, [spec]), edit_group=all0)
                assert torch.equal(a.top_indices, b.top_indices), (f, kw)
                assert torch.equal(a.top_acts.view(torch.int32), b.top_acts.view(torch.int32)), (f, kw)


def test_op_level_consistency(dev):
    """ops.edit_topk_rows: independent of kk beyond k + E_max; the int32 and int64 forms agree; `edited` marks exactly the
    slots whose index is in the token's table; ids outside [0, G) are defined input (unedited), not a fault."""
    from msae import ops

    k, T = 32, 40
    sae = tge._sae(dev, k)
    xt, L, order = tge._inputs(T, "bf16")
    w = (sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights())
    for sizes in CONFIGS.values():
        specs = _specs(L, order, k, sizes)
        groups = rref.merge_groups(specs)
        G, E_max = len(sizes), max(sizes)
        ed = _row_edits(dev, specs)
        group_of = _group_of(T, G)
        group_of[[4, 9, 14]] = (G, G + 7, -5)                              # (the round-robin's own -1 rows, made hostile)
        go = torch.from_numpy(group_of).to(dev)
        with torch.no_grad():
            v0, i0, _ = ops.encode_topk(xt.to(dev), *w[:3], w[3], k + E_max)
            v7, i7, _ = ops.encode_topk(xt.to(dev), *w[:3], w[3], k + E_max + 7)
            a = ops.edit_topk_rows(v0, i0, go, ed, N, k, want_mask=True)
            b = ops.edit_topk_rows(v7, i7, go.long(), ed, N, k, want_mask=True)
            c = ops.edit_topk_rows(v7, i7.to(torch.int32), go, ed, N, k, want_mask=True)
            two = ops.edit_topk_rows(v7, i7, go, ed, N, k)
        assert len(two) == 2 and a[1].dtype == torch.int64 and c[1].dtype == torch.int32 and a[2].dtype == torch.uint8
        ref_v, ref_i, ref_e = rref.list_edit_rows(v0.cpu().numpy(), i0.cpu().numpy(), k, groups, group_of)
        for got in (a, b, c, two):
            tge._assert_bits(got[0], got[1], ref_v, ref_i)
        for got in (a, b, c):
            assert np.array_equal(got[2].cpu().numpy(), ref_e)
        tge._assert_bits(a[0], a[1], *rref.dense_topk_rows(L, k, groups, group_of))
        assert ref_e.any() and not ref_e[[4, 9, 14]].any()
        tge._assert_bits(a[0][[4, 9, 14]], a[1][[4, 9, 14]], v0[[4, 9, 14], :k].cpu().numpy(), i0[[4, 9, 14], :k].cpu().numpy())


def test_shape_off_the_fast_path_and_a_long_table(dev):
    """d = 64, N = 1000 (no fused pass), k = 32: a group of 300 edits (k' = 332 > 256: the exact route, 1024 keys) beside a
    group of 1."""
    d, n, k, T = 64, 1000, 32, 7
    w = tge._weights(d, n, 67)
    sae = tge._make_sae(dev, d, n, k, w)
    x = synth.activations(T, d, 9, n_outlier=1)
    x[1] = w[3]
    L = oracle.pre_acts(x, w[0], w[1], w[3])
    order = np.stack([np.lexsort((np.arange(n), -L[t].astype(np.float64))) for t in range(T)])
    specs = [rref.plan(L, order, k, 300, 0, n), rref.plan(L, order, k, 1, 2, n)]
    groups = rref.merge_groups(specs)
    assert [len(g[0]) for g in groups] == [300, 1]
    group_of = np.array([0, 0, 1, 0, -1, 1, 0], dtype=np.int32)
    ref_v, ref_i = rref.dense_topk_rows(L, k, groups, group_of)
    with torch.no_grad():
        top = sae.encode(torch.from_numpy(x).to(dev), edits=_row_edits(dev, specs, n), edit_group=torch.from_numpy(group_of).to(dev))
    tge._assert_bits(top.top_acts, top.top_indices, ref_v, ref_i)


def test_batched_input_shapes(dev):
    k, B, S = 32, 4, 10
    sae = tge._sae(dev, k)
    xt, L, order = tge._inputs(40, "bf16")
    specs = [_specs(L, order, k, (3,))[0], None, _specs(L, order, k, (0, 1))[1], _specs(L, order, k, (0, 0, 50))[2]]
    groups = rref.merge_groups(specs)
    ref_v, ref_i = rref.dense_topk_rows(L, k, groups, np.repeat(np.arange(B), S))
    ed = _row_edits(dev, specs)
    x = xt.to(dev).reshape(B, S, D)
    with torch.no_grad():
        a = sae.encode(x, edits=ed)                                        # row b -> group b
        b = sae.encode(x, edits=ed, edit_group=torch.arange(B, device=dev))
        c = sae.encode(x, edits=ed, edit_group=torch.arange(B, device=dev, dtype=torch.int32)[:, None].expand(B, S))
        perm = torch.tensor([2, -1, 0, 3], device=dev)
        p = sae.encode(x, edits=ed, edit_group=perm)
    for got in (a, b, c):
        assert got.top_acts.shape == (B, S, k) and got.top_indices.shape == (B, S, k)
        tge._assert_bits(got.top_acts, got.top_indices, ref_v, ref_i)
    tge._assert_bits(p.top_acts, p.top_indices, *rref.dense_topk_rows(L, k, groups, np.repeat([2, -1, 0, 3], S)))


def test_status_exact_certified_and_no_host_sync(dev):
    from msae import ops

    k, T = 32, 300
    sae = tge._sae(dev, k)
    xt, L, order = tge._inputs(T, "bf16")
    x = xt.to(dev)
    specs = _specs(L, order, k, (8, 0, 1))
    groups = rref.merge_groups(specs)
    group_of = _group_of(T, 3)
    go = torch.from_numpy(group_of).to(dev)
    ed = _row_edits(dev, specs)
    ref_v, ref_i = rref.dense_topk_rows(L, k, groups, group_of)
    with torch.no_grad():
        _, _, st_plain = ops.encode_topk(x, sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights(), k + 8)
        sae.encode(x, edits=ed, edit_group=go)                             # warm: workspaces, prepared operands
        sae.encode(x.reshape(3, 100, D), edits=ed)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            top, st = sae.encode(x, edits=ed, edit_group=go, return_status=True)
            rows = sae.encode(x.reshape(3, 100, D), edits=ed)              # the device-side expansion of "row b -> group b"
        finally:
            torch.cuda.set_sync_debug_mode("default")
        tge._assert_bits(top.top_acts, top.top_indices, ref_v, ref_i)
        tge._assert_bits(rows.top_acts, rows.top_indices, *rref.dense_topk_rows(L, k, groups, np.repeat(np.arange(3), 100)))
        assert st.dtype == torch.int32 and set(st.cpu().tolist()) <= {0, 1}
        assert torch.equal(st[1:4], st_plain[1:4])
        top_e, st_e = sae.encode(x, edits=ed, edit_group=go, exact=True, return_status=True)
        assert (st_e == 1).all()
        tge._assert_bits(top_e.top_acts, top_e.top_indices, ref_v, ref_i, "exact")
        top_c, _ = sae.encode(x, edits=ed, edit_group=go, certified=True, return_status=True)
        tge._assert_bits(top_c.top_acts, top_c.top_indices, ref_v, ref_i, "certified")


def test_autograd_matches_the_legacy_seam(dev):
    """encode(edits=RowEdits) -> decode -> weighted sum against the legacy seam (pre_acts -> per-token torch edit ->
    select_topk -> decode): equal selections, gradients within test_gpu_edits' bar (2e-3 of the largest entry + 1e-8).
    Feature `hot` is clamped high in group 0 and left alone in group 1: it carries no gradient through group 0's tokens
    and a non-zero one through group 1's -- the case a feature-wide mask gets wrong."""
    k, T = 32, 40
    sae = tge._make_sae(dev, D, N, k, tge._w())
    xt, L, order = tge._inputs(T, "f32")
    hot = int(order[7][0])                                                 # token 7 (group 1) selects it on its own
    s0, z0 = tge._plan(L, order, k, 12)
    s0 = {f: (v if v <= 0 else v + float(L.max())) for f, v in s0.items() if f != hot}
    z0 = [f for f in z0 if f != hot]
    s0[hot] = 2.0 * float(L.max())
    s1, z1 = tge._plan(L, order, k, 3, seed=1)
    assert hot not in s1 and hot not in z1
    specs = [{"set": s0, "zero": z0 or None}, {"set": s1 or None, "zero": z1 or None}]
    groups = rref.merge_groups(specs)
    group_of = np.array([t % 2 if t % 5 != 4 else -1 for t in range(T)], dtype=np.int32)
    assert group_of[0] == 0 and group_of[7] == 1
    go = torch.from_numpy(group_of).to(dev)
    ed = _row_edits(dev, specs)
    # the legacy seam's per-token edit as two dense tensors: a keep mask and the set values
    keep, setv = np.ones((T, N), dtype=np.float32), np.zeros((T, N), dtype=np.float32)
    for t, g in enumerate(group_of):
        tab = rref.table_of(groups, g)
        if tab is not None:
            keep[t, tab[0]] = 0
            setv[t, tab[0]] = np.where(tab[2] == eref.ZERO, np.float32(0), tab[1])
    keep, setv = torch.from_numpy(keep).to(dev), torch.from_numpy(setv).to(dev)
    params = (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)
    grads = {}
    for route in ("fused", "legacy"):
        x = xt.to(dev).clone().requires_grad_()
        if route == "fused":
            top = sae.encode(x, edits=ed, edit_group=go)
            assert top.top_acts.requires_grad
        else:
            top = sae.select_topk(sae.pre_acts(x) * keep + setv)
        out = sae.decode(top.top_acts, top.top_indices)
        (out * torch.linspace(-1, 1, D, device=dev)).sum().backward()
        grads[route] = [x.grad.clone()] + [p.grad.clone() for p in params]
        grads[route + "_idx"] = top.top_indices.detach()
        for p in params:
            p.grad = None
    assert torch.equal(grads["fused_idx"], grads["legacy_idx"])
    for a, b, nm in zip(grads["fused"], grads["legacy"], ("x", "W_enc", "b_enc", "W_dec", "b_dec")):
        assert b.abs().max() > 0, nm
        assert (a - b).abs().max().item() <= 2e-3 * b.abs().max().item() + 1e-8, nm
    # the feature with two roles, seen through the encoder-bias gradient of single-token losses
    assert (grads["fused_idx"][0] == hot).any() and (grads["fused_idx"][7] == hot).any()
    for t, zero in ((0, True), (7, False)):
        x = xt.to(dev).clone().requires_grad_()
        top = sae.encode(x, edits=ed, edit_group=go)
        sae.decode(top.top_acts, top.top_indices)[t].sum().backward()
        gb = sae.encoder.bias.grad[hot].item()
        assert (gb == 0) if zero else (gb != 0), (t, gb)
        for p in params:
            p.grad = None


# ---- hooks ---------------------------------------------------------------------------------------------------------------
def test_hook_reproduces_the_reference_runs_row_by_row(dev, golden_dir):
    """g18: the reference's own batch-1 hook run once per feature on one hidden state; row f of clamp_features_rows on the
    hidden state repeated F times must be within g5 / g16's GPU tolerance (2e-3 of the largest reference entry) of run f."""
    from msae.features import clamp_features_rows

    g = np.load(golden_dir / "g18_row_edits.npz")
    sae = tge._golden_sae(dev, g)
    feats, clamp = g["features"].tolist(), float(g["clamp"])
    F = len(feats)
    layer = torch.nn.Identity()
    for features in (feats, [[f] for f in feats], [{f: clamp} for f in feats]):
        handles = clamp_features_rows(sae, features, layer, k=clamp)
        with torch.no_grad():
            out = layer(torch.from_numpy(g["x"]).to(dev).repeat(F, 1, 1))
            step = layer(torch.from_numpy(g["x_S1"]).to(dev).repeat(F, 1, 1))
        for h in handles:
            h.remove()
        ref = g["out"].astype(np.float32)
        assert out.dtype == torch.float16 and out.shape == ref.shape
        for f in range(F):
            assert np.abs(out[f].float().cpu().numpy() - ref[f]).max() <= 2e-3 * np.abs(ref[f]).max(), f
        ref1 = g["out_S1"].astype(np.float32)[0]
        assert step.shape == (F, 1, ref1.shape[-1])
        for f in range(F):
            assert np.abs(step[f].float().cpu().numpy() - ref1).max() <= 2e-3 * np.abs(ref1).max(), f


def _table(element, kv):
    if element is None:
        return {}
    if isinstance(element, dict):
        return element
    return {int(f): float(kv) for f in (element if isinstance(element, list) else [element])}


def _legacy_rows_hook(sae, features, kv, seen=None):
    """The reference's hook body (test_gpu_edits._legacy_steer) applied to h[b : b + 1] with row b's table."""
    def hook(module, _i, outputs):
        h = outputs[0]
        if seen is not None:
            seen["h"] = h.detach().clone()
        out = torch.cat([tge._legacy_steer(sae, h[b:b + 1], _table(features[b], kv)) for b in range(h.shape[0])])
        return (out,) + tuple(outputs[1:])
    return hook


def test_hook_on_the_fake_model_equals_the_legacy_seam_per_row(dev, tiny):
    from msae.features import clamp_features_rows

    g, model, sae, inputs = tiny
    layer = model.language_model.get_submodule(str(g["module"]))
    active = g["clean_top_idx"]
    features = [int(active[1][0]), None, sorted(set(active[1][:3].tolist() + [5, 1000])), {int(active[4][0]): 1.5, 7: 3.0}]
    ids = inputs["input_ids"][:1].repeat(len(features), 1)
    seen = {}
    probe = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o[0].detach().clone()))
    handles = clamp_features_rows(sae, features, layer, k=7.0)
    after = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o[0].detach().clone()))
    try:
        with torch.no_grad():
            model(input_ids=ids)
            want = torch.cat([tge._legacy_steer(sae, seen["h"][b:b + 1], _table(f, 7.0)) for b, f in enumerate(features)])
            plain = tge._legacy_attr(sae, seen["h"][1:2], [])              # the unclamped splice
    finally:
        for h in handles + [probe, after]:
            h.remove()
    assert seen["out"].dtype == torch.float16 and torch.equal(seen["out"].view(torch.int16), want.view(torch.int16))
    assert torch.equal(seen["out"][1:2].view(torch.int16), plain.view(torch.int16))
    assert not torch.equal(seen["out"][0], seen["out"][1])


def test_the_batch_step_replays_from_a_hip_graph(dev):
    from msae.features import clamp_features_rows

    B = 4
    sae = tge._sae(dev, 32)
    layer_g, layer_e = torch.nn.Identity(), torch.nn.Identity()
    hg = clamp_features_rows(sae, [5, None, [7, 9], 11], layer_g, k=10, graph_step=True)
    he = clamp_features_rows(sae, [5, None, [7, 9], 11], layer_e, k=10, graph_step=False)
    gen = torch.Generator(device=dev).manual_seed(3)
    try:
        with torch.no_grad():
            graphs = []
            for step in range(3):
                h = torch.randn(B, 1, D, generator=gen, device=dev).to(torch.float16)
                a, b = layer_g(h), layer_e(h)
                assert a.dtype == torch.float16 and a.shape == h.shape and torch.equal(a, b), step
                graphs.append(hg[0].step_graph.graph)
            hp = torch.randn(B, 6, D, generator=gen, device=dev).to(torch.float16)
            assert torch.equal(layer_g(hp), layer_e(hp))
        sg = hg[0].step_graph
        assert sg is not None and sg.graph is not None and not sg.failed and he[0].step_graph is None
        assert all(x is graphs[0] for x in graphs)                         # captured once over the three steps
        assert tuple(sg.x.shape) == (B, D)
    finally:
        for hdl in hg + he:
            hdl.remove()


def test_controller_batches_the_features(dev, golden_dir):
    """SteeringController(batch_features=4) on 6 features: the texts equal those of the same batched model calls with the
    per-row legacy hook (so the hidden states entering the hook are the same tensors); the original is the unclamped run."""
    from msae.features.steering import SteeringController

    g = np.load(golden_dir / "g10_steering.npz")
    model = fakes.TinyLlava(vocab=int(g["vocab"]), d=int(g["d"])).to(dev)
    sae = tge._golden_sae(dev, g)
    module, kv = str(g["module"]), float(g["clamp"])
    feats = [int(f) for f in g["features"]] + [3, 17, 40]
    proc = fakes.FakeProcessor(int(g["vocab"]))
    ctl = SteeringController(sae=sae, module_name=module, feature_idx=feats, model=model, processor=proc, prompt="describe",
                             k=kv, batch_features=4)
    res = ctl.run()
    assert list(res) == [f"{module}_feature{f}" for f in feats]
    layer = model.language_model.get_submodule(module)
    want = []
    for chunk in (feats[:4], feats[4:]):
        inputs = {key: v.repeat(len(chunk), *([1] * (v.dim() - 1))) for key, v in ctl.inputs.items()}
        h = layer.register_forward_hook(_legacy_rows_hook(sae, chunk, kv))
        try:
            with torch.no_grad():
                out = model.generate(**inputs, max_new_tokens=512)
        finally:
            h.remove()
        want += proc.batch_decode(out[:, ctl.inputs["input_ids"].shape[-1]:], skip_special_tokens=True)
    for f, ref in zip(feats, want):
        assert res[f"{module}_feature{f}"]["clamped_resps"] == ref, f
        assert res[f"{module}_feature{f}"]["idx"] == f
        assert res[f"{module}_feature{f}"]["original_resps"] == str(g["original"])
    assert len(set(want)) > 1                                              # the rows really were steered differently


def test_attribution_with_several_features_per_pass(dev, tiny, capsys):
    """get_attribution(groups, "exact", features_per_pass=3) == the dense-seam loop on the SAME 3x-repeated batch (one uniform
    ablation per pass, the rows of that copy, the metric times 3), to test_gpu_edits' bar: 2^-10 of the largest score."""
    from msae.features import Attribution
    from msae.features.patching import get_logit_diff

    g, model, sae, inputs = tiny
    name = str(g["module"])
    answer = torch.from_numpy(g["answer_ids"]).to(dev)
    attr = Attribution.from_parts(model, {name: sae}, inputs, answer)
    active = g["clean_top_idx"]
    groups = [[int(active[4][0]), int(active[7][1])], int(active[9][0]), [int(active[4][1]), 5, int(active[9][2])]]
    G, B = 3, answer.shape[0]
    got = torch.stack(attr.get_attribution(groups, method="exact", features_per_pass=G)[name]).float()
    assert got.shape[0] == len(groups) and got.shape[1] == B
    layer = attr.name_to_module[name]
    rep = attr._repeated_inputs(G)
    assert rep["input_ids"].shape[0] == G * B and len(rep["image_sizes"]) == G * B

    def run(off):
        cache = {}

        def hook(module, _i, outputs):
            out = tge._legacy_attr(sae, outputs[0], off)
            cache[name] = out
            return (out,) + tuple(outputs[1:])

        h = layer.register_forward_hook(hook)
        try:
            logits = model(**rep)["logits"]
        finally:
            h.remove()
        return logits, cache

    with torch.no_grad():
        _, clean = run([])
    want = []
    for c, grp in enumerate(groups):
        logits, cor = run(grp if isinstance(grp, list) else [grp])
        cor[name].retain_grad()
        (G * get_logit_diff(logits, answer.repeat(G, 1))).backward()
        want.append(((clean[name] - cor[name]) * cor[name].grad).detach().sum(-1)[c * B:(c + 1) * B].cpu())
        attr._zero_param_grads()
    want = torch.stack(want).float()
    scale = want.abs().max().item()
    dev_batched = (got - want).abs().max().item()
    single = torch.stack(attr.get_attribution(groups, method="exact")[name]).float()
    with capsys.disabled():
        print(f"\n[row edits] attribution: |batched - dense loop on the repeated batch| = {dev_batched:.3e}, "
              f"|features_per_pass=3 - features_per_pass=1| = {(got - single).abs().max().item():.3e}, largest score {scale:.3e}")
    assert scale > 0 and dev_batched <= 2.0 ** -10 * scale
    # a chunk shorter than features_per_pass, and more entries than one pass holds
    more = torch.stack(attr.get_attribution(groups + [groups[1]], method="exact", features_per_pass=3)[name]).float()
    assert more.shape[0] == 4 and (more[:3] - got).abs().max().item() <= 2.0 ** -10 * scale
    assert (more[3] - got[1]).abs().max().item() <= 2.0 ** -10 * scale


def test_argument_errors_on_the_device(dev):
    from msae import _hip
    from msae.parallel import EmulatedShardGroup

    lib = _hip.load()
    v = torch.zeros(4, 64, device=dev)
    i32 = torch.zeros(4, 64, dtype=torch.int32, device=dev)
    e = torch.zeros(97, dtype=torch.int32, device=dev)
    ev = torch.zeros(97, device=dev)
    o = torch.zeros(4, 4000, device=dev)
    oi = torch.zeros(4, 4000, dtype=torch.int32, device=dev)
    m = torch.zeros(4, 4000, dtype=torch.uint8, device=dev)
    p = _hip.ptr

    def call(T=4, kk=64, G=2, E_total=5, E_max=3, n=1000, k=8, edited=m):
        return lib.msae_edit_topk_rows_f32(p(v), p(i32), T, kk, p(e), p(e), G, p(e), p(ev), p(e), E_total, E_max, n, k, p(o),
                                           p(oi), None if edited is None else p(edited), None)

    assert call(T=-1) == -1 and call(G=0) == -1 and call(k=0) == -1 and call(E_max=0) == -1 and call(E_total=-1) == -1
    assert call(kk=10) == -1                       # kk < k + E_max
    assert call(E_max=30, n=40, k=32) == -1        # k + E_max > N
    assert call(kk=5000, E_max=97, n=8192, k=4000) == -1
    assert call(T=0) == 0 and call(T=0, edited=None) == 0
    torch.cuda.synchronize()
    sae = tge._sae(dev, 32)
    with pytest.raises(NotImplementedError, match="Sae"):
        EmulatedShardGroup(sae, 2).encode(torch.zeros(4, D, device=dev), edits=_row_edits(dev, [dict(zero=[1, 2])]))
    with pytest.raises(ValueError):
        sae.encode(torch.zeros(4, D, device=dev), edits=_row_edits(dev, [dict(zero=[1])]),
                   edit_group=torch.zeros(4, dtype=torch.int32, device=dev), zero_feature=3)
