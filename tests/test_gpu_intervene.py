"""Error-preserving interventions on the HIP path (ops.delta_decode, Sae.intervene, the hooks' preserve_error) against the
numpy restatement tests/intervene_ref.py -- BIT FOR BIT unless a test says otherwise -- and against the float64 composition
x + sum_Q - sum_P within the bound derived there.  The device calls run under torch.cuda.set_sync_debug_mode("error")
(`no_sync`); results are read back outside it.  Plans, weights and inputs: tests/test_intervene_host.py."""
import contextlib

import numpy as np
import pytest
import torch

import fakes
import intervene_ref as iref
import test_gpu_edits as tge
import test_gpu_row_edits as tgr
import test_intervene_host as tih

pytestmark = pytest.mark.gpu

D, N = tge.D, tge.N
DTYPES = tge.DTYPES
tiny = tge.tiny


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _bits(t, dtype):
    return tih.x_bits(t.reshape(-1, t.shape[-1]), dtype)


# ---- the op on synthetic lists (no encode, N = 64) -----------------------------------------------------------------------
N_OP = 64
_W_OP = {}


def _w_op(d):
    if d not in _W_OP:
        _W_OP[d] = np.random.default_rng(100 + d).standard_normal((N_OP, d)).astype(np.float32)
    return _W_OP[d]


def _lists(T, k, rng, first):
    """(P_v, P_i, Q_v, Q_i, category [T]): token t is of category (first + t) % 5 --
    0 identical lists, 1 every entry survives (Q's values differ), 2 a few features with a new value, 3 +-0 entries with
    other indices plus one real difference, 4 Q shifted by an inserted entry (the shape an edit leaves).  Values are small
    multiples of 1/64 so that sums stay far from the f16 range; features repeat when k > N (a hostile list: same rule)."""
    cat = (first + np.arange(T)) % 5
    P_v = (rng.integers(1, 256, (T, k)) / 64.0).astype(np.float32)
    P_i = np.stack([np.resize(rng.permutation(N_OP), k) for _ in range(T)]).astype(np.int64)
    Q_v, Q_i = P_v.copy(), P_i.copy()
    for t in range(T):
        c = cat[t]
        if c == 1 or (c == 4 and k == 1):
            Q_v[t] = P_v[t] + np.float32(0.5)
        elif c == 2:
            j = rng.permutation(k)[:max(1, min(3, k // 2))]
            Q_v[t, j] = P_v[t, j] + np.float32(64.0)                       # (off P's grid: it cannot meet a repeated feature's value)
        elif c == 3:
            h = k // 2
            P_v[t, h:] = 0.0
            Q_v[t, h:] = -0.0 if t % 2 else 0.0
            Q_i[t, h:] = (P_i[t, h:] + 5) % N_OP
            Q_v[t, 0] = P_v[t, 0] + np.float32(64.0)
        elif c == 4:
            Q_v[t, 1:], Q_i[t, 1:] = P_v[t, :-1], P_i[t, :-1]
            Q_v[t, 0], Q_i[t, 0] = np.float32(9.0), (P_i[t, 0] + 1) % N_OP
    return P_v, P_i, Q_v, Q_i, cat


def _x(T, d, dtype, rng, cat, dev):
    x = torch.from_numpy((rng.integers(-512, 512, (T, d)) / 128.0).astype(np.float32)).to(DTYPES[dtype])
    for t in np.nonzero(cat == 0)[0]:          # untouched tokens: -0 and NaN payloads must pass through
        x[t, 0] = -0.0
        x[t, d - 1] = float("nan")
    return x.to(dev)


def _run_op(dev, T, k, d, dtype, wide, strided, first, seed):
    from msae import ops

    rng = np.random.default_rng(seed)
    P_v, P_i, Q_v, Q_i, cat = _lists(T, k, rng, first)
    W = _w_op(d)
    x = _x(T, d, dtype, rng, cat, dev)
    it = torch.int64 if wide else torch.int32
    if strided:                                # the plain list as the first k columns of a wider [T, kk] tensor
        kk = k + 3
        pv = torch.full((T, kk), 7.0, device=dev)
        pi = torch.full((T, kk), N_OP + 9, dtype=it, device=dev)       # (a kernel reading past k would see a bad index)
        pv[:, :k], pi[:, :k] = torch.from_numpy(P_v).to(dev), torch.from_numpy(P_i).to(dev, it)
        pv, pi = pv[:, :k], pi[:, :k]
        assert not pv.is_contiguous() or T == 1 or k == kk
    else:
        pv, pi = torch.from_numpy(P_v).to(dev), torch.from_numpy(P_i).to(dev, it)
    qv, qi = torch.from_numpy(Q_v).to(dev), torch.from_numpy(Q_i).to(dev, it)
    Wt = torch.from_numpy(W).to(dev)
    with no_sync():
        out = ops.delta_decode(x, pv, pi, qv, qi, Wt)
    ref, n, flagged = iref.intervene(_bits(x, dtype), dtype, P_v, P_i, Q_v, Q_i, W, N_OP)
    assert not flagged and out.dtype == x.dtype and out.shape == x.shape
    assert ((n == 0) == (cat == 0)).all()
    got = _bits(out, dtype)
    bad = np.nonzero((got != ref).any(1))[0]
    assert bad.size == 0, f"tokens {bad[:8].tolist()} (categories {cat[bad[:8]].tolist()}) differ: T={T} k={k} d={d} {dtype}"
    return x, (pv, pi, qv, qi, Wt), ref


_DS, _KS, _TS, _DTS = (4, 6, 260, 1028, 4096), (1, 4, 32, 256, 300), (1, 5, 300), ("f32", "bf16", "f16")
# every (d, k) pair; T, dtype, index width and the strided plain list rotate so that every value of each meets every d and k
OP_CASES = [(d, k, _TS[(a + b) % 3], _DTS[(a + 2 * b) % 3], (a + b) % 2 == 0, (a * 5 + b) % 3 != 0)
            for a, d in enumerate(_DS) for b, k in enumerate(_KS)]


@pytest.mark.parametrize("d,k,T,dtype,wide,strided", OP_CASES)
def test_op_equals_the_restatement(dev, d, k, T, dtype, wide, strided):
    _run_op(dev, T, k, d, dtype, wide, strided, first=d + k, seed=1000 * d + k)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_op_every_category_at_one_token_and_in_place(dev, dtype):
    from msae import ops

    for first in range(5):                     # T = 1 of every category, both index widths
        _run_op(dev, 1, 32, 260, dtype, first % 2 == 0, True, first=first, seed=first)
    x, (pv, pi, qv, qi, Wt), ref = _run_op(dev, 5, 4, 1028, dtype, True, True, first=0, seed=77)
    x_in = x.clone()
    with no_sync():
        same = ops.delta_decode(x_in, pv, pi, qv, qi, Wt, out=x_in)        # out aliases x
        other = torch.empty_like(x)
        ops.delta_decode(x, pv, pi, qv, qi, Wt, out=other)
    assert same is x_in and np.array_equal(_bits(x_in, dtype), ref) and np.array_equal(_bits(other, dtype), ref)


def test_op_envelope_k_4096(dev):
    """k = 4096: 128 KiB of LDS per workgroup, the loops over the lists at their longest."""
    _run_op(dev, 2, 4096, 8, "f32", True, False, first=3, seed=5)
    _run_op(dev, 2, 4096, 6, "bf16", False, True, first=0, seed=6)


def test_op_out_of_range_feature_is_skipped_and_flagged(dev):
    """(reads the flag back, so this one test runs without the sync guard)"""
    from msae import ops

    rng = np.random.default_rng(9)
    T, k, d = 5, 4, 260
    P_v, P_i, Q_v, Q_i, cat = _lists(T, k, rng, 0)
    Q_i[1, 2], Q_v[1, 2] = N_OP + 1000, np.float32(3.0)                    # survives, out of range: skipped
    Q_i[2, 0] = -7
    P_i[0, 1] = Q_i[0, 1] = 2 ** 40                                        # in both lists: cancels, still flagged
    W = _w_op(d)
    x = _x(T, d, "f32", rng, cat, dev)
    args = [torch.from_numpy(a).to(dev) for a in (P_v, P_i, Q_v, Q_i, W)]
    out = ops.delta_decode(x, *args)
    ref, n, flagged = iref.intervene(_bits(x, "f32"), "f32", P_v, P_i, Q_v, Q_i, W, N_OP)
    assert flagged and np.array_equal(_bits(out, "f32"), ref)
    ops.set_debug_bounds(True)
    try:
        with pytest.raises(IndexError):
            ops.delta_decode(x, *args)
        args[1][0, 1] = args[3][0, 1] = 3
        args[3][1, 2], args[3][2, 0] = 5, 6
        ops.delta_decode(x, *args)                                         # every feature in range: no error
    finally:
        ops.set_debug_bounds(False)


# ---- Sae.intervene against the restatement fed with the dense definition's lists ------------------------------------------
def _check(out, xt, dtype, P, Q, W_dec, what, n_want=None):
    xb = tih.x_bits(xt, dtype)
    ref, n, _ = iref.intervene(xb, dtype, *P, *Q, W_dec, N)
    got = _bits(out, dtype)
    assert out.dtype == DTYPES[dtype] and np.array_equal(got, ref), f"bits differ: {what}"
    xf = iref.to_f32(xb, dtype)
    err = np.abs(iref.values_f64(got, dtype) - iref.composed_f64(xf, *P, *Q, W_dec))
    assert (err <= iref.bound(xf, dtype, *P, *Q, W_dec)).all(), f"outside the bound of the float64 composition: {what}"
    return n


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("k", [4, 32])
@pytest.mark.parametrize("T", [1, 5, 40, 300])
def test_intervene_equals_the_restatement(dev, T, k, dtype):
    from msae.features import RowEdits

    sae = tge._sae(dev, k)
    W_dec = tge._w()[2]
    for E in (1, 3, 50):
        xt, P, Q, s, z = tih.feature_case(T, k, E, dtype)
        ed = tge._edits(dev, s, z)
        assert ed.E == E
        x = xt.to(dev)
        with torch.no_grad():
            sae.intervene(x, ed)                                           # warm: workspaces, prepared operands
            with no_sync():
                out = sae.intervene(x, ed)
        n = _check(out, xt, dtype, P, Q, W_dec, f"E={E} T={T} k={k} {dtype}")
        tih.check_planted(n)                   # every token differs: a kernel returning x cannot pass
    for config, sizes in tgr.CONFIGS.items():
        xt, P, Q, sp, group_of = tih.rows_case(T, k, config, dtype)
        ed = RowEdits(N, sp, device=dev)
        x, go = xt.to(dev), torch.from_numpy(group_of).to(dev)
        with torch.no_grad():
            sae.intervene(x, ed, go)
            with no_sync():
                out = sae.intervene(x, ed, go)
        n = _check(out, xt, dtype, P, Q, W_dec, f"{config} T={T} k={k} {dtype}")
        tih.check_planted(n, group_of, sizes)
        keep = torch.from_numpy(n == 0).to(dev)                            # group -1 and the empty group: x's own bits
        assert torch.equal(out[keep].view(tih.TORCH_BITS[dtype]), x[keep].view(tih.TORCH_BITS[dtype]))


def test_intervene_does_not_depend_on_the_chunk(dev):
    """A token's result does not depend on T or on its neighbours; [B, S, d] inputs with per-row groups."""
    from msae.features import RowEdits

    k, dtype = 32, "bf16"
    sae = tge._sae(dev, k)
    xt, P, Q, s, z = tih.feature_case(300, k, 50, dtype)
    ed = tge._edits(dev, s, z)
    x = xt.to(dev)
    with torch.no_grad(), no_sync():
        full = sae.intervene(x, ed)
        parts = [sae.intervene(x[a:b], ed) for a, b in ((0, 1), (1, 6), (6, 46), (46, 300))]
        rolled = sae.intervene(torch.roll(x, 7, 0), ed)
        cube = sae.intervene(x[:296].reshape(8, 37, D), ed)
    assert torch.equal(torch.cat(parts).view(torch.int16), full.view(torch.int16))
    assert torch.equal(torch.roll(rolled, -7, 0).view(torch.int16), full.view(torch.int16))
    assert cube.shape == (8, 37, D) and torch.equal(cube.reshape(-1, D).view(torch.int16), full[:296].view(torch.int16))
    xt, P, Q, sp, group_of = tih.rows_case(40, k, "short", dtype)          # "row b uses group b" on [G, S, d]
    ed = RowEdits(N, sp, device=dev)
    xg = xt.to(dev)[:39].reshape(3, 13, D)
    with torch.no_grad(), no_sync():
        by_row = sae.intervene(xg, ed)
        by_tok = sae.intervene(xg.reshape(-1, D), ed, torch.arange(3, device=dev, dtype=torch.int32).repeat_interleave(13))
    assert torch.equal(by_row.reshape(-1, D).view(torch.int16), by_tok.view(torch.int16))
    assert not torch.equal(by_row.view(torch.int16), xg.view(torch.int16))


def test_intervene_replays_from_a_hip_graph(dev):
    """One capture on one stream, one replay on new data."""
    k, dtype = 32, "bf16"
    sae = tge._sae(dev, k)
    xt, P, Q, s, z = tih.feature_case(40, k, 3, dtype)
    ed = tge._edits(dev, s, z)
    x = xt.to(dev)
    buf = torch.zeros_like(x)
    side = torch.cuda.Stream(device=dev)
    with torch.no_grad():
        want = sae.intervene(x, ed)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                sae.intervene(buf, ed)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = sae.intervene(buf, ed)
        buf.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)) and not torch.equal(out, x)


# ---- hooks on the fake model ---------------------------------------------------------------------------------------------
def _count_encodes(monkeypatch):
    from msae import ops

    calls, real = [], ops.encode_topk

    def counted(x, *a, **kw):
        calls.append(tuple(x.shape))
        return real(x, *a, **kw)

    monkeypatch.setattr(ops, "encode_topk", counted)
    return calls


def _ref_rows(sae, h, tables, dtype="f16"):
    """h [B, S, d] on the device, one {feature: value} table (or None) per row -> the restatement's bits [B * S, d], from the
    encoder's own lists of each row."""
    from msae.features import FeatureEdits

    out = []
    for b, table in enumerate(tables):
        with torch.no_grad():
            p = sae.encode(h[b])
            q = p if not table else sae.encode(h[b], edits=FeatureEdits(sae.num_latents, set=table, device=h.device))
        P = (p.top_acts.cpu().numpy(), p.top_indices.cpu().numpy())
        Q = (q.top_acts.cpu().numpy(), q.top_indices.cpu().numpy())
        ref, n, _ = iref.intervene(tih.x_bits(h[b], dtype), dtype, *P, *Q, sae.W_dec.detach().cpu().numpy(), sae.num_latents)
        assert (n > 0).all() if table else (n == 0).all()
        out.append(ref)
    return np.concatenate(out)


def test_steering_hooks_preserve_the_error(dev, tiny, monkeypatch):
    from msae.features import clamp_features_max, clamp_features_rows

    g, model, sae, inputs = tiny
    layer = model.language_model.get_submodule(str(g["module"]))
    active = g["clean_top_idx"]
    features = [int(active[1][0]), None, sorted(set(active[1][:3].tolist() + [5, 1000])), {int(active[4][0]): 15.0, 7: 13.0}]
    tables = [None if f is None else tgr._table(f, 17.0) for f in features]
    ids = inputs["input_ids"][:1].repeat(len(features), 1)
    seen = {}
    probe = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o[0].detach().clone()))
    handles = clamp_features_rows(sae, features, layer, k=17.0, preserve_error=True)
    after = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o[0].detach().clone()))
    calls = _count_encodes(monkeypatch)
    try:
        with torch.no_grad():
            model(input_ids=ids)
            h, out = seen["h"], seen["out"]
            assert len(calls) == 1 and handles[0].step_graph is None
            assert out.dtype == h.dtype == torch.float16
            assert torch.equal(out[1].view(torch.int16), h[1].view(torch.int16))          # the row of None: the model's own
            assert np.array_equal(_bits(out, "f16"), _ref_rows(sae, h, tables))             # steered rows: h + restatement
            assert not torch.equal(out[0], h[0])
            del calls[:]
            toks = model.generate(input_ids=ids, max_new_tokens=4)
            assert calls == [(len(features) * ids.shape[1], h.shape[-1])], calls            # the prefill; no S = 1 call
            assert seen["h"].shape[1] == 1 and torch.equal(seen["out"].view(torch.int16), seen["h"].view(torch.int16))
            assert toks.shape[0] == len(features)
    finally:
        for hd in handles + [after]:
            hd.remove()
    # clamp_features_max, one feature and a list
    try:
        for feature, table in ((features[0], tables[0]), (features[2], tables[2])):
            handles = clamp_features_max(sae, feature, layer, k=17.0, preserve_error=True)
            after = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o[0].detach().clone()))
            del calls[:]
            with torch.no_grad():
                model(input_ids=ids[:1])
                assert np.array_equal(_bits(seen["out"], "f16"), _ref_rows(sae, seen["h"], [table]))
                del calls[:]
                model.generate(input_ids=ids[:1], max_new_tokens=3)
            assert len(calls) == 1 and handles[0].step_graph is None
            for hd in handles + [after]:
                hd.remove()
    finally:
        probe.remove()


def test_attribution_hook_leaves_unedited_positions_alone(dev, tiny):
    from msae.features import RowEdits, attribution_sae_hook

    g, model, sae, inputs = tiny
    name = str(g["module"])
    layer = model.language_model.get_submodule(name)
    active = g["clean_top_idx"]
    B, S = inputs["input_ids"].shape
    ed = RowEdits(sae.num_latents, [dict(zero=[int(active[0][0]), int(active[1][0])]), None], device=dev)
    group = torch.full((B, S), -1, dtype=torch.int32, device=dev)
    group[0, :2] = 0                                                       # two edited positions; group 1 is empty
    group[1, 0] = 1
    seen, cache = {}, {}
    probe = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o[0].detach().clone()))
    hk = layer.register_forward_hook(attribution_sae_hook({name: sae}, {layer: name}, cache, ed, group, preserve_error=True))
    try:
        with torch.no_grad(), no_sync():
            model(**inputs)
    finally:
        probe.remove()
        hk.remove()
    h, out = seen["h"], cache[name]
    changed = (out.view(torch.int16) != h.view(torch.int16)).any(-1)
    assert out.dtype == h.dtype and changed[0, :2].all() and int(changed.sum()) == 2
    # no edit at all under no_grad: the hidden state itself, no SAE call
    cache = {}
    hk = layer.register_forward_hook(attribution_sae_hook({name: sae}, {layer: name}, cache, None, preserve_error=True))
    probe = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o[0]), prepend=True)
    try:
        with torch.no_grad():
            model(**inputs)
    finally:
        hk.remove()
        probe.remove()
    assert cache[name] is seen["h"]


def _steer_ref_hook(sae, chunk, kv):
    """The definition of the error-preserving steering hook, row by row through Sae.intervene with that row's own table."""
    from msae.features import FeatureEdits

    def hook(module, _i, outputs):
        h = outputs[0]
        if h.shape[1] == 1:
            return outputs
        rows = [sae.intervene(h[b:b + 1], FeatureEdits(sae.num_latents, set={int(f): float(kv)}, device=h.device))
                for b, f in enumerate(chunk)]
        return (torch.cat(rows),) + tuple(outputs[1:])
    return hook


def test_controller_with_preserve_error(dev, golden_dir):
    from msae.features.steering import SteeringController

    g = np.load(golden_dir / "g10_steering.npz")
    model = fakes.TinyLlava(vocab=int(g["vocab"]), d=int(g["d"])).to(dev)
    sae = tge._golden_sae(dev, g)
    module, kv = str(g["module"]), float(g["clamp"])
    feats = [int(f) for f in g["features"]] + [3, 17, 40]
    proc = fakes.FakeProcessor(int(g["vocab"]))
    kw = dict(sae=sae, module_name=module, feature_idx=feats, model=model, processor=proc, prompt="describe", k=kv)
    layer = model.language_model.get_submodule(module)
    for B in (1, 4):
        ctl = SteeringController(batch_features=B, preserve_error=True, **kw)
        res = ctl.run()
        assert list(res) == [f"{module}_feature{f}" for f in feats]
        want = []
        for lo in range(0, len(feats), B):
            chunk = feats[lo:lo + B]
            inputs = {key: v.repeat(len(chunk), *([1] * (v.dim() - 1))) for key, v in ctl.inputs.items()}
            h = layer.register_forward_hook(_steer_ref_hook(sae, chunk, kv))
            try:
                with torch.no_grad():
                    out = model.generate(**inputs, max_new_tokens=512)
            finally:
                h.remove()
            want += proc.batch_decode(out[:, ctl.inputs["input_ids"].shape[-1]:], skip_special_tokens=True)
        for f, ref in zip(feats, want):
            assert res[f"{module}_feature{f}"]["clamped_resps"] == ref, (B, f)
            assert res[f"{module}_feature{f}"]["original_resps"] == str(g["original"])
        assert len(set(want)) > 1                                          # the rows really were steered differently


def test_autograd_form_against_the_fused_path_and_the_reconstruct_hook(dev, tiny):
    """sae_reconstruct(preserve_error=True) under autograd: the forward is within the two derived bounds of the fused path; the
    gradients with respect to the latents equal the reconstruct path's (the error term is a constant of the forward)."""
    from msae.features import Attribution, FeatureEdits, sae_reconstruct

    g, model, sae, inputs = tiny
    name = str(g["module"])
    layer = model.language_model.get_submodule(name)
    active = g["clean_top_idx"]
    off = sorted({int(active[0][0]), int(active[3][1]), int(active[7][0]), 5})
    ed = FeatureEdits(sae.num_latents, zero=off, device=dev)
    seen = {}
    probe = layer.register_forward_hook(lambda m, i, o: seen.__setitem__("h", o[0].detach().clone()))
    with torch.no_grad():
        model(**inputs)
    probe.remove()
    W_dec, b_dec = sae.W_dec.detach().cpu().numpy(), sae.b_dec.detach().cpu().numpy()
    cot = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(seen["h"].shape)).astype(np.float32)).to(dev)
    for dtype in ("f16", "f32"):
        h = seen["h"].to(DTYPES[dtype])
        flat = h.reshape(-1, h.shape[-1])
        with torch.no_grad():
            fused = sae.intervene(h, ed)
            p, q = sae.encode(flat), sae.encode(flat, edits=ed)
        grads = {}
        real_decode = sae.decode
        for mode in ("preserve", "reconstruct"):
            def decode(top_acts, top_indices, mode=mode):
                if top_acts.requires_grad:
                    top_acts.retain_grad()
                    grads[mode] = top_acts
                return real_decode(top_acts, top_indices)

            sae.decode = decode
            try:
                hg = h.clone().requires_grad_()
                out = sae_reconstruct(sae, hg, edits=ed, preserve_error=True) if mode == "preserve" else \
                    sae_reconstruct(sae, hg, edits=ed, out_dtype=h.dtype)      # (the same cast in front of both graphs)
                (out.float() * cot).sum().backward()
            finally:
                sae.decode = real_decode
                for prm in sae.parameters():
                    prm.grad = None
            if mode == "preserve":
                got = out.detach()
        assert got.dtype == h.dtype and grads["preserve"].grad is not None
        assert torch.equal(grads["preserve"].grad, grads["reconstruct"].grad)
        assert torch.equal(grads["preserve"].detach().view(torch.int32), grads["reconstruct"].detach().view(torch.int32))
        P = (p.top_acts.cpu().numpy(), p.top_indices.cpu().numpy())
        Q = (q.top_acts.cpu().numpy(), q.top_indices.cpu().numpy())
        xf = iref.to_f32(_bits(h, dtype), dtype)
        limit = iref.bound(xf, dtype, *P, *Q, W_dec) + iref.bound_composed_f32(xf, dtype, *P, *Q, W_dec, b_dec)
        err = np.abs(iref.values_f64(_bits(got, dtype), dtype) - iref.values_f64(_bits(fused, dtype), dtype))
        assert (err <= limit).all() and (_bits(fused, dtype) != _bits(h, dtype)).any()
    # the Attribution driver with the switch on: the clean run is the model itself, scores come out finite and not all zero
    answer = torch.from_numpy(g["answer_ids"]).to(dev)
    attr = Attribution.from_parts(model, {name: sae}, inputs, answer, preserve_error=True)
    one = torch.stack(attr.get_attribution([off, int(active[9][0])], method="exact")[name]).float()
    two = torch.stack(attr.get_attribution([off, int(active[9][0])], method="exact", features_per_pass=2)[name]).float()
    assert one.shape == two.shape and torch.isfinite(one).all() and one.abs().max() > 0
    assert (one - two).abs().max().item() <= 2.0 ** -10 * one.abs().max().item()
    with pytest.raises(ValueError, match="exact"):
        attr.get_attribution([1], method="batched")
