"""Set-valued latent edits on the HIP path (Sae.encode(edits=...), ops.edit_topk, the hooks) against the numpy
restatement tests/edits_ref.py -- dense latents from oracle.pre_acts, edits applied, oracle.topk -- BIT FOR BIT unless a
test says otherwise.  Shapes: d = 256, N = 8192 is the smallest width with the fused fast path; T = 1 and 5 run the
<= 16-token streams, 40 the weight-stream GEMM, 300 the large-batch GEMM with the feature-major re-score.  b_enc <= 0 and
the batch holds degenerate tokens (an all-zero row x = b_dec, rows with 1 and 3 positive latents) wherever T allows."""
import numpy as np
import pytest
import torch

import edits_ref as eref
import fakes
import synth
from oracle import oracle

pytestmark = pytest.mark.gpu

D, N = 256, 8192
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


def _weights(d, n, seed):
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, n, seed)
    b_enc = (-np.abs(b_enc) - np.float32(0.5)).astype(np.float32)          # b_enc <= 0: x = b_dec is an all-zero row
    b_dec = (np.round(b_dec * 256) / 256).astype(np.float32)               # exact in bf16 and f16
    return W_enc, b_enc, W_dec, b_dec


def _make_sae(dev, d, n, k, weights):
    from msae import Sae, SaeConfig

    sae = Sae(d, SaeConfig(num_latents=n, k=k), device=dev)
    with torch.no_grad():
        for p, a in zip((sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec), weights):
            p.copy_(torch.from_numpy(a))
    return sae.eval()


_W = {}
_CASE = {}


def _w():
    if "w" not in _W:
        _W["w"] = _weights(D, N, 61)
    return _W["w"]


def _sae(dev, k):
    if ("sae", k) not in _W:
        _W[("sae", k)] = _make_sae(dev, D, N, k, _w())
    return _W[("sae", k)]


def _inputs(T, dtype):
    """x [T, D] in `dtype` (as f32 numpy, exactly what the kernel up-casts), its dense latents and each token's canonical
    order.  Rows 1-3 (T >= 5) are degenerate: all-zero, one positive latent, three positive latents."""
    key = (T, dtype)
    if key not in _CASE:
        W_enc, b_enc, _, b_dec = _w()
        x = synth.activations(T, D, 70 + T)
        if T >= 5:
            unit = W_enc / np.linalg.norm(W_enc, axis=1, keepdims=True)
            x[1] = b_dec
            x[2] = b_dec + np.float32(0.6) * unit[4000]
            x[3] = b_dec + np.float32(0.6) * (unit[17] + unit[900] + unit[5000])
        xt = torch.from_numpy(x).to(DTYPES[dtype])
        xf = xt.float().numpy()
        L = oracle.pre_acts(xf, W_enc, b_enc, b_dec)
        order = np.stack([np.lexsort((np.arange(N), -L[t].astype(np.float64))) for t in range(T)])
        if T >= 5:
            assert (L[1] == 0).all() and (L[2] > 0).sum() == 1 and (L[3] > 0).sum() == 3
        _CASE[key] = (xt, L, order)
    return _CASE[key]


def _plan(L, order, k, E, seed=0):
    """(set dict, zero list) with E distinct features (the last SET also named in `zero` in the longer tables), planted relative to
    token 0's ranking (and the last token's): see the comments.  Truncated to E in priority order."""
    T = L.shape[0]
    o0, last = order[0], order[T - 1]
    v = lambda r: float(L[0, o0[r]])
    picks = [("zero", int(o0[0]), None),                                   # a feature inside the top-k
             ("set", int(o0[k]), v(min(1, k - 1))),                        # rank k + 1, SET exactly equal to a selected value
             ("set", int(o0[k + E + 5]), 0.5 * v(k - 1)),                  # outside the list, SET below token 0's k-th value
             ("set", int(o0[min(2, k - 1)]), 2.0 * v(0)),                  # SET on a feature already selected
             ("set", 0, 0.25), ("set", 1, 0.0),                            # SET on features 0 and 1 (among the zero fill)
             ("zero", 2, None), ("zero", 3, None),                         # ZERO below / among the fill entries
             ("set", int(o0[k + 1]), -1.0),                                # SET to -1: never selected
             ("set", int(o0[min(3, k - 1)]), 0.0),                         # SET to 0 on a selected feature
             ("zero", 4000, None), ("zero", 17, None)]                     # the degenerate rows' own positives
    picks += [("zero", int(f), None) for f in last[:k]]                    # ALL of the last token's top-k (needs E >= k)
    rng = np.random.default_rng(1000 * k + E + seed)
    picks += [("set" if j % 2 else "zero", int(f), float(rng.uniform(0.0, 2.0) * v(k - 1))) for j, f in
              enumerate(rng.permutation(N)[:E + 8])]
    set_edits, zero = {}, []
    for kind, f, val in picks:
        if len(set_edits) + len(zero) >= E:
            break
        if f in set_edits or f in zero:
            continue
        if kind == "set":
            set_edits[f] = val
        else:
            zero.append(f)
    if len(set_edits) >= 7:
        zero.append(list(set_edits)[-1])                                   # in both lists: ZERO wins, E unchanged
    return set_edits, zero


def _edits(dev, set_edits, zero, n=N):
    from msae.features import FeatureEdits

    return FeatureEdits(n, set=set_edits or None, zero=zero or None, device=dev)


def _assert_bits(got_v, got_i, ref_v, ref_i, what=""):
    gi, gv = got_i.cpu().numpy(), got_v.cpu().numpy()
    assert np.array_equal(gi.reshape(ref_i.shape), ref_i), f"indices differ {what}"
    assert np.array_equal(eref.bits(gv).reshape(ref_v.shape), eref.bits(ref_v)), f"values differ {what}"


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("E", [1, 3, 50])
@pytest.mark.parametrize("k", [4, 32])
@pytest.mark.parametrize("T", [1, 5, 40, 300])
def test_encode_with_edits_equals_the_dense_definition(dev, T, k, E, dtype):
    sae = _sae(dev, k)
    xt, L, order = _inputs(T, dtype)
    set_edits, zero = _plan(L, order, k, E)
    ed = _edits(dev, set_edits, zero)
    assert ed.E == E
    ref_v, ref_i = eref.dense_topk(L, k, *eref.merge(set_edits, zero))
    with torch.no_grad():
        top, status = sae.encode(xt.to(dev), edits=ed, return_status=True)
    assert top.top_indices.dtype == torch.int64 and top.top_acts.shape == (T, k) and status.shape == (T,)
    _assert_bits(top.top_acts, top.top_indices, ref_v, ref_i, f"T={T} k={k} E={E} {dtype}")
    assert (ref_v >= 0).all()                 # (the plan's SET to -1 is never selected)
    if E >= k + 12 and T > 1:                 # the plan zeroed the whole selection of the last token: nothing of it survives
        assert not (set(order[T - 1][:k].tolist()) - set(set_edits)) & set(ref_i[T - 1].tolist())


def test_planted_positions_in_one_table(dev):
    """Every planted position of the plan in ONE call (E = 24 at k = 4 and k = 32), checked against both restatements."""
    for k in (4, 32):
        sae = _sae(dev, k)
        xt, L, order = _inputs(40, "bf16")
        set_edits, zero = _plan(L, order, k, 24, seed=5)
        feats, vals, kinds = eref.merge(set_edits, zero)
        ref_v, ref_i = eref.dense_topk(L, k, feats, vals, kinds)
        lv, li = oracle.topk(L, k + 24)
        lst = eref.list_edit(lv, li, k, feats, vals, kinds)
        assert np.array_equal(lst[1], ref_i) and np.array_equal(eref.bits(lst[0]), eref.bits(ref_v))
        with torch.no_grad():
            top = sae.encode(xt.to(dev), edits=_edits(dev, set_edits, zero))
        _assert_bits(top.top_acts, top.top_indices, ref_v, ref_i)
        o0, row = order[0], ref_i[0].tolist()
        assert int(o0[0]) not in row                                       # zeroed
        low = int(o0[k + 24 + 5])
        assert set_edits[low] < ref_v[0, -1] and low not in row            # SET below the k-th value: must not appear
        if k == 32:
            assert int(o0[k]) in row and row.index(int(o0[k])) in (1, 2)   # equal to the 2nd value: index order decides
        assert int(o0[k + 1]) not in row                                   # SET to -1
        assert (ref_v >= 0).all()
        # the all-zero row: the positive SET values first, then zeros by ascending index -- the ZERO edits on features
        # 2 and 3 and the SET to 0 on feature 1 tie with the fill and keep their places in it
        r1 = ref_i[1].tolist()
        assert r1[0] in set_edits and ref_v[1, 0] > 0
        tail = [f for f, val in zip(r1, ref_v[1]) if val == 0]
        assert tail == sorted(tail) and (len(tail) < 3 or tail[:3] == [1, 2, 3])


def test_batched_input_shape(dev):
    k, E = 32, 3
    sae = _sae(dev, k)
    xt, L, order = _inputs(40, "bf16")
    set_edits, zero = _plan(L, order, k, E)
    ref_v, ref_i = eref.dense_topk(L, k, *eref.merge(set_edits, zero))
    with torch.no_grad():
        top = sae.encode(xt.to(dev).reshape(2, 20, D), edits=_edits(dev, set_edits, zero))
    assert top.top_acts.shape == (2, 20, k) and top.top_indices.shape == (2, 20, k)
    _assert_bits(top.top_acts, top.top_indices, ref_v, ref_i)


def test_shape_off_the_fast_path_and_a_long_table(dev):
    """d = 64, N = 1000 (no fused pass) with k = 32, E = 300: k' = 332 > 256 runs the exact route; 512 + 128 keys sorted."""
    d, n, k, E, T = 64, 1000, 32, 300, 7
    w = _weights(d, n, 67)
    sae = _make_sae(dev, d, n, k, w)
    x = synth.activations(T, d, 9, n_outlier=1)
    x[1] = w[3]
    L = oracle.pre_acts(x, w[0], w[1], w[3])
    assert (L[1] == 0).all()
    order = np.stack([np.lexsort((np.arange(n), -L[t].astype(np.float64))) for t in range(T)])
    rng = np.random.default_rng(3)
    feats = list(dict.fromkeys(order[0][:40].tolist() + order[2][20:60].tolist() + [0, 1, 2] + rng.permutation(n).tolist()))[:E]
    set_edits = {int(f): float(rng.choice([0.0, -1.0, float(L[0, order[0][5]]), float(rng.uniform(0, 3))])) for f in feats[::2]}
    zero = [int(f) for f in feats[1::2]]
    ref_v, ref_i = eref.dense_topk(L, k, *eref.merge(set_edits, zero))
    with torch.no_grad():
        top = sae.encode(torch.from_numpy(x).to(dev), edits=_edits(dev, set_edits, zero, n))
    _assert_bits(top.top_acts, top.top_indices, ref_v, ref_i)


@pytest.mark.parametrize("T", [5, 300])
def test_one_edit_equals_the_scalar_arguments(dev, T):
    k = 32
    sae = _sae(dev, k)
    xt, L, order = _inputs(T, "bf16")
    x = xt.to(dev)
    o0 = order[0]
    with torch.no_grad():
        for f in (int(o0[0]), int(o0[k]), int(o0[k + 3]), 0, 4000):
            for kw, (s, z) in ((dict(zero_feature=f), (None, [f])),
                               (dict(set_feature=f, set_value=float(L[0, o0[1]])), ({f: float(L[0, o0[1]])}, None)),
                               (dict(set_feature=f, set_value=0.0), ({f: 0.0}, None)),
                               (dict(set_feature=f, set_value=-1.0), ({f: -1.0}, None))):
                a = sae.encode(x, **kw)
                b = sae.encode(x, edits=_edits(dev, s, z))
                assert torch.equal(a.top_indices, b.top_indices), (f, kw)
                assert torch.equal(a.top_acts.view(torch.int32), b.top_acts.view(torch.int32)), (f, kw)


def test_edit_topk_op_consistency(dev):
    """ops.edit_topk: independent of kk beyond k + E; the int32 and int64 forms agree; equals the list restatement."""
    from msae import ops

    k, E, T = 32, 50, 40
    sae = _sae(dev, k)
    xt, L, order = _inputs(T, "bf16")
    set_edits, zero = _plan(L, order, k, E)
    ed = _edits(dev, set_edits, zero)
    feats, vals, kinds = eref.merge(set_edits, zero)
    with torch.no_grad():
        v0, i0, _ = ops.encode_topk(xt.to(dev), sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights(), k + E)
        v7, i7, _ = ops.encode_topk(xt.to(dev), sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights(), k + E + 7)
        a = ops.edit_topk(v0, i0, ed.feat, ed.val, ed.kind, N, k)
        b = ops.edit_topk(v7, i7, ed.feat, ed.val, ed.kind, N, k)
        c = ops.edit_topk(v7, i7.to(torch.int32), ed.feat, ed.val, ed.kind, N, k)
        t = torch.ops.msae.edit_topk(v7, i7, ed.feat, ed.val, ed.kind, N, k)
    assert a[1].dtype == torch.int64 and c[1].dtype == torch.int32
    ref_v, ref_i = eref.list_edit(v0.cpu().numpy(), i0.cpu().numpy(), k, feats, vals, kinds)
    for got in (a, b, c, t):
        _assert_bits(got[0], got[1], ref_v, ref_i)
    _assert_bits(a[0], a[1], *eref.dense_topk(L, k, feats, vals, kinds))


def test_status_exact_certified_and_no_host_sync(dev):
    from msae import ops

    k, E, T = 32, 8, 300
    sae = _sae(dev, k)
    xt, L, order = _inputs(T, "bf16")
    x = xt.to(dev)
    set_edits, zero = _plan(L, order, k, E)
    ed = _edits(dev, set_edits, zero)
    ref_v, ref_i = eref.dense_topk(L, k, *eref.merge(set_edits, zero))
    with torch.no_grad():
        _, _, st_plain = ops.encode_topk(x, sae.encoder.weight, sae.encoder.bias, sae.b_dec, sae._prepared_weights(), k + E)
        sae.encode(x, edits=ed)                                            # warm: workspaces, prepared operands, ed.mask is not needed
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            top, st = sae.encode(x, edits=ed, return_status=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        _assert_bits(top.top_acts, top.top_indices, ref_v, ref_i)
        # the status is the underlying over-fetching encode's (compared on the degenerate rows, whose route does not
        # depend on the call's dither seed)
        assert st.dtype == torch.int32 and set(st.cpu().tolist()) <= {0, 1}
        assert torch.equal(st[1:4], st_plain[1:4])
        top_e, st_e = sae.encode(x, edits=ed, exact=True, return_status=True)
        assert (st_e == 1).all()
        _assert_bits(top_e.top_acts, top_e.top_indices, ref_v, ref_i, "exact")
        top_c, st_c = sae.encode(x, edits=ed, certified=True, return_status=True)
        _assert_bits(top_c.top_acts, top_c.top_indices, ref_v, ref_i, "certified")


def test_autograd_matches_the_legacy_seam(dev):
    """encode(edits) -> decode -> sum: gradients w.r.t. x and the parameters equal the legacy seam's (pre_acts -> torch
    edit -> select_topk -> decode) within the splice-hook tests' tolerance (test_gpu_dropin: 2e-3 of the largest entry +
    1e-8); edited features' encoder rows get exactly zero gradient."""
    k, E, T = 32, 12, 40
    sae = _make_sae(dev, D, N, k, _w())
    xt, L, order = _inputs(T, "f32")
    set_edits, zero = _plan(L, order, k, E)
    # clamps high enough to be selected everywhere, so set latents with a positive value meet the mask
    set_edits = {f: (v if v <= 0 else v + float(L.max())) for f, v in set_edits.items()}
    ed = _edits(dev, set_edits, zero)
    feats = torch.tensor(ed.features, device=dev)
    params = (sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec)
    grads = {}
    for route in ("fused", "legacy"):
        x = xt.to(dev).clone().requires_grad_()
        if route == "fused":
            top = sae.encode(x, edits=ed)
            assert top.top_acts.requires_grad
        else:
            lat = sae.pre_acts(x)
            mask = torch.ones_like(lat)
            mask[:, feats] = 0
            lat = lat * mask                                               # (no gradient through an overwritten latent)
            sv = torch.zeros(N, device=dev)
            for f, v in set_edits.items():
                if f not in zero:
                    sv[f] = v
            lat = lat + sv
            top = sae.select_topk(lat)
        out = sae.decode(top.top_acts, top.top_indices)
        (out * torch.linspace(-1, 1, D, device=dev)).sum().backward()
        grads[route] = [x.grad.clone()] + [p.grad.clone() for p in params]
        idx = top.top_indices.detach()
        for p in params:
            p.grad = None
        grads[route + "_idx"] = idx
    assert torch.equal(grads["fused_idx"], grads["legacy_idx"])
    for a, b, nm in zip(grads["fused"], grads["legacy"], ("x", "W_enc", "b_enc", "W_dec", "b_dec")):
        assert b.abs().max() > 0, nm
        assert (a - b).abs().max().item() <= 2e-3 * b.abs().max().item() + 1e-8, nm
    assert (grads["fused"][1][feats] == 0).all() and (grads["fused"][2][feats] == 0).all()
    hit = torch.isin(grads["fused_idx"], feats).any()
    assert bool(hit)                                                       # edited features were selected, and masked


# ---- hooks ---------------------------------------------------------------------------------------------------------------
def _golden_sae(dev, g):
    d, n, k = int(g["d"]), int(g["N"]), int(g["k"])
    return _make_sae(dev, d, n, k, synth.sae_weights(d, n, int(g["wseed"])))


def test_hooks_reproduce_the_reference_run_with_lists(dev, golden_dir):
    """g16 (the reference's own hooks called with feature lists) through the HIP path, to g5's GPU tolerance."""
    from msae.features import attribution_sae_hook, clamp_features_max

    g = np.load(golden_dir / "g16_multi_edit.npz")
    sae = _golden_sae(dev, g)
    layer = torch.nn.Identity()
    feats, clamp = g["steer_features"].tolist(), float(g["steer_clamp"])
    for S in (5, 1):
        x = torch.from_numpy(g[f"steer_S{S}_x"]).to(dev)
        for feature, kv in ((feats, clamp), ({f: clamp for f in feats}, 1.0)):
            handles = clamp_features_max(sae, feature, layer, k=kv)
            with torch.no_grad():
                out = layer(x)
            for h in handles:
                h.remove()
            ref = g[f"steer_S{S}_out"]
            assert out.dtype == torch.float16 and out.shape == x.shape
            assert np.abs(out.float().cpu().numpy() - ref.astype(np.float32)).max() <= 2e-3 * np.abs(ref).max()
    x = torch.from_numpy(g["attr_x"]).to(dev)
    for tag in ("few", "many"):
        for off in (g[f"attr_{tag}_features"].tolist(), torch.from_numpy(g[f"attr_{tag}_features"]).to(dev)):
            cache = {}
            h = layer.register_forward_hook(attribution_sae_hook({"L": sae}, {layer: "L"}, cache, off))
            with torch.no_grad():
                out = layer(x)
            h.remove()
            ref = g[f"attr_{tag}_out"]
            assert np.abs(out.float().cpu().numpy() - ref.astype(np.float32)).max() <= 2e-3 * np.abs(ref).max()
            assert cache["L"] is out


def _legacy_steer(sae, h, table):
    """The reference's steering hook body on the legacy seam (steering.py:111-118), dense latents and torch indexing."""
    latents = sae.pre_acts(h)
    if latents.shape[1] != 1:
        for f, v in table.items():
            latents[:, :, f] = v
    top_acts, top_indices = sae.select_topk(latents)
    return sae.decode(top_acts[0], top_indices[0]).unsqueeze(0).to(torch.float16)


def _legacy_attr(sae, h, off):
    """patching/utils.py:41-51 on the legacy seam."""
    bs, seq_len, dim = h.shape
    latents = sae.pre_acts(h.flatten(0, 1))
    mask = torch.ones_like(latents)
    mask[:, off] = 0
    latents = latents * mask
    top_acts, top_indices = sae.select_topk(latents)
    return sae.decode(top_acts, top_indices).to(torch.float16).view(bs, seq_len, dim)


@pytest.fixture(scope="module")
def tiny(dev, golden_dir):
    g = np.load(golden_dir / "g8_attribution.npz")
    model = fakes.TinyLlava(vocab=int(g["vocab"]), d=int(g["d"])).to(dev)
    sae = _golden_sae(dev, g)
    inputs = {"input_ids": torch.from_numpy(g["input_ids"]).to(dev), "pixel_values": torch.from_numpy(g["pixel_values"]).to(dev),
              "image_sizes": [[8, 6], [8, 6]],
              "attention_mask": torch.ones(g["input_ids"].shape, dtype=torch.bool, device=dev)}
    return g, model, sae, inputs


def test_hooks_on_the_fake_model_equal_the_legacy_seam(dev, tiny):
    """clamp_features_max with a list and a mapping, attribution_sae_hook with a list, on tests/fakes.py's model: the fp16
    output of the hooked layer is bit-identical to the reference hook body restated on the legacy seam."""
    from msae.features import attribution_sae_hook, clamp_features_max

    g, model, sae, inputs = tiny
    name = str(g["module"])
    layer = model.language_model.get_submodule(name)
    seen = {}
    probe = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o[0].detach().clone()))
    probe_after = None
    active = g["clean_top_idx"]
    feats = sorted(set(active[1][:3].tolist() + [int(active[4][0]), 5, 1000]))
    ids = inputs["input_ids"][:1]
    try:
        for feature, kv, table in ((feats, 7.0, {f: 7.0 for f in feats}),
                                   ({f: 1.0 + 0.5 * j for j, f in enumerate(feats)}, 3.0, {f: 1.0 + 0.5 * j for j, f in enumerate(feats)})):
            handles = clamp_features_max(sae, feature, layer, k=kv)
            probe_after = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o[0].detach().clone()))
            with torch.no_grad():
                model(input_ids=ids)
                want = _legacy_steer(sae, seen["h"], table)
            for h in handles + [probe_after]:
                h.remove()
            assert seen["out"].dtype == torch.float16 and torch.equal(seen["out"].view(torch.int16), want.view(torch.int16))
        off = sorted(set(active[0][:4].tolist() + active[7][:2].tolist() + [3]))
        cache = {}
        h = layer.register_forward_hook(attribution_sae_hook({name: sae}, {layer: name}, cache, off))
        with torch.no_grad():
            model(**inputs)
            want = _legacy_attr(sae, seen["h"], off)
        h.remove()
        assert torch.equal(cache[name].view(torch.int16), want.view(torch.int16))
    finally:
        probe.remove()


def test_attribution_with_a_group_equals_the_dense_loop(dev, tiny):
    """get_attribution([[a, b], c], "exact") == the reference-shaped loop with the dense seam (a list in off_features)."""
    from msae.features import Attribution
    from msae.features.patching import get_logit_diff

    g, model, sae, inputs = tiny
    name = str(g["module"])
    answer = torch.from_numpy(g["answer_ids"]).to(dev)
    attr = Attribution.from_parts(model, {name: sae}, inputs, answer)
    active = g["clean_top_idx"]
    groups = [[int(active[4][0]), int(active[7][1])], int(active[9][0]), [int(active[4][1]), 5, int(active[9][2])]]
    got = torch.stack(attr.get_attribution(groups, method="exact")[name]).float()
    assert got.shape[0] == len(groups)
    layer = attr.name_to_module[name]

    def run(off):
        cache = {}

        def hook(module, _i, outputs):
            out = _legacy_attr(sae, outputs[0], off) if off is not None else _legacy_attr(sae, outputs[0], [])
            cache[name] = out
            return (out,) + tuple(outputs[1:])

        h = layer.register_forward_hook(hook)
        try:
            logits = model(**inputs)["logits"]
        finally:
            h.remove()
        return logits, cache

    with torch.no_grad():
        _, clean = run(None)
    want = []
    for grp in groups:
        logits, cor = run(grp if isinstance(grp, list) else [grp])
        cor[name].retain_grad()
        get_logit_diff(logits, answer).backward()
        want.append(((clean[name] - cor[name]) * cor[name].grad).detach().sum(-1).cpu())
        attr._zero_param_grads()
    want = torch.stack(want).float()
    scale = want.abs().max().item()
    # the forwards are bit-identical and the cached gradient is taken DOWNSTREAM of the splice, so the two loops run the
    # same arithmetic; the bar is two fp16 ulps (2^-10) of the largest score, for torch kernels that sum in another order
    assert scale > 0 and (got - want).abs().max().item() <= 2.0 ** -10 * scale
    with pytest.raises(ValueError, match="batched"):
        attr.get_attribution(groups, method="batched")


def test_argument_errors_on_the_device(dev):
    from msae import _hip, ops
    from msae.features import FeatureEdits
    from msae.parallel import EmulatedShardGroup

    lib = _hip.load()
    v = torch.zeros(4, 64, device=dev)
    i32 = torch.zeros(4, 64, dtype=torch.int32, device=dev)
    e = torch.zeros(97, dtype=torch.int32, device=dev)
    ev = torch.zeros(97, device=dev)
    o = torch.zeros(4, 4000, device=dev)
    oi = torch.zeros(4, 4000, dtype=torch.int32, device=dev)
    p = _hip.ptr

    def call(kk, E, n, k):
        return lib.msae_edit_topk_f32(p(v), p(i32), 4, kk, p(e), p(ev), p(e), E, n, k, p(o), p(oi), None)

    assert call(10, 3, 1000, 8) == -1          # kk < k + E
    assert call(64, 30, 40, 32) == -1          # k + E > N
    assert call(5000, 97, 8192, 4000) == -1    # k + E > 4096
    torch.cuda.synchronize()
    sae = _sae(dev, 32)
    with pytest.raises(NotImplementedError, match="Sae"):
        EmulatedShardGroup(sae, 2).encode(torch.zeros(4, D, device=dev), edits=FeatureEdits(N, zero=[1, 2], device=dev))
    with pytest.raises(ValueError):
        sae.encode(torch.zeros(4, D, device=dev), edits=FeatureEdits(N, zero=[1], device=dev), zero_feature=3)
