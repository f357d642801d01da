"""Error-preserving interventions without a device: the numpy restatement tests/intervene_ref.py
against the float64 composition x + sum_Q - sum_P within its derived bound -- and the bound's power against nearly-right
variants --, the survival rule on small lists, and the host layer (symbols, argument errors before any device work, launcher
flags, hooks that build today's objects when preserve_error is off).

Inputs: the weights, activations and planted edit positions of tests/test_gpu_edits.py (D = 256, N = 8192; rows 1-3
degenerate), each table preceded by ONE CLAMP -- a SET far above every latent, on a feature the plan does not name -- so that
every edited token has a non-empty difference (a plan that only zeroes token 0's features leaves most tokens untouched: a
kernel returning x would pass).  tests/test_gpu_intervene.py uses the same plans."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import edits_ref as eref
import intervene_ref as iref
import row_edits_ref as rref
import test_gpu_edits as tge
import test_gpu_row_edits as tgr
from oracle import oracle

REPO = Path(__file__).resolve().parents[1]
D, N = tge.D, tge.N
BITS = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}
TORCH_BITS = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}


def x_bits(xt, dtype):
    """A torch tensor in its storage dtype -> its bits as numpy."""
    return xt.contiguous().view(TORCH_BITS[dtype]).cpu().numpy().view(BITS[dtype])


def plan(L, order, k, E, seed=0):
    """(set dict, zero list) with E distinct features: one clamp (2 max L + 1, on a feature outside every planted position),
    then test_gpu_edits._plan's E - 1."""
    set_edits, zero = tge._plan(L, order, k, E - 1, seed=seed) if E > 1 else ({}, [])
    clamp = next(int(f) for f in order[0][k + E + 20:] if int(f) not in set_edits and int(f) not in zero and int(f) > 3)
    return {clamp: float(2.0 * L.max() + 1.0), **set_edits}, zero


def specs(L, order, k, sizes):
    out = []
    for g, E in enumerate(sizes):
        if E == 0:
            out.append(None)
            continue
        s, z = plan(L, order, k, E, seed=g)
        out.append({"set": s or None, "zero": z or None})
    return out


_CASES = {}


def feature_case(T, k, E, dtype):
    """-> (xt, P, Q) with P / Q = (vals, idx) of the dense definition; set_edits / zero of the plan."""
    key = ("f", T, k, E, dtype)
    if key not in _CASES:
        xt, L, order = tge._inputs(T, dtype)
        s, z = plan(L, order, k, E)
        _CASES[key] = (xt, oracle.topk(L, k), eref.dense_topk(L, k, *eref.merge(s, z)), s, z)
    return _CASES[key]


def rows_case(T, k, config, dtype):
    """-> (xt, P, Q, specs, group_of) for a group config of tests/test_gpu_row_edits.py."""
    key = ("r", T, k, config, dtype)
    if key not in _CASES:
        xt, L, order = tge._inputs(T, dtype)
        sizes = tgr.CONFIGS[config]
        sp = specs(L, order, k, sizes)
        group_of = tgr._group_of(T, len(sizes))
        _CASES[key] = (xt, oracle.topk(L, k), rref.dense_topk_rows(L, k, rref.merge_groups(sp), group_of), sp, group_of)
    return _CASES[key]


def check_planted(n, group_of=None, sizes=None):
    """The conditions a test of the intervention needs: edited tokens differ, unedited ones do not."""
    if group_of is None:
        assert (n > 0).all()
        return
    edited = np.array([0 <= g < len(sizes) and sizes[g] > 0 for g in group_of])
    assert (n[edited] > 0).all() and (n[~edited] == 0).all()
    assert len(n) < 5 or (edited.any() and (~edited).any())                # (T = 1: the one token may sit in the empty group)


def _within(out_bits, dtype, xf, P, Q, W_dec):
    err = np.abs(iref.values_f64(out_bits, dtype) - iref.composed_f64(xf, *P, *Q, W_dec))
    return err, iref.bound(xf, dtype, *P, *Q, W_dec)


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("k", [4, 32])
def test_restatement_is_within_the_bound_of_the_composition(k, dtype):
    W_dec = tge._w()[2]
    for T, E in ((40, 1), (5, 3), (40, 50)):
        xt, P, Q, _, _ = feature_case(T, k, E, dtype)
        xb = x_bits(xt, dtype)
        out, n, flagged = iref.intervene(xb, dtype, *P, *Q, W_dec, N)
        check_planted(n)
        assert not flagged
        err, bnd = _within(out, dtype, iref.to_f32(xb, dtype), P, Q, W_dec)
        assert (err <= bnd).all(), (T, E, float((err / bnd).max()))
    for config in ("long", "short"):
        xt, P, Q, sp, group_of = rows_case(40, k, config, dtype)
        xb = x_bits(xt, dtype)
        out, n, _ = iref.intervene(xb, dtype, *P, *Q, W_dec, N)
        check_planted(n, group_of, tgr.CONFIGS[config])
        assert np.array_equal(out[n == 0], xb[n == 0])
        err, bnd = _within(out, dtype, iref.to_f32(xb, dtype), P, Q, W_dec)
        assert (err <= bnd).all(), (config, float((err / bnd).max()))


@pytest.mark.parametrize("dtype", ["bf16", "f32", "f16"])
@pytest.mark.parametrize("k", [4, 32])
def test_the_bound_rejects_nearly_right_variants(k, dtype):
    """One survivor dropped, the plain part's sign flipped, a same-feature-different-value pair cancelled, b_dec added once:
    each leaves the bound somewhere at these inputs."""
    _, _, W_dec, b_dec = tge._w()
    xt, P, Q, _, _ = feature_case(40, k, 50, dtype)
    xb = x_bits(xt, dtype)
    xf = iref.to_f32(xb, dtype)
    idx, coef, n, _, n_q = iref.diff_lists(*P, *Q, with_split=True)
    comp, bnd = iref.composed_f64(xf, *P, *Q, W_dec), iref.bound(xf, dtype, *P, *Q, W_dec)

    def out_of(idx_v, coef_v, extra=None):
        s = xf + oracle.decode(idx_v, coef_v, W_dec, None)
        if extra is not None:
            s = s + extra
        return iref.values_f64(iref.from_f32(s, dtype), dtype)

    assert (np.abs(out_of(idx, coef) - comp) <= bnd).all()
    dropped = coef.copy()
    dropped[:, 0] = 0                                                      # the first survivor of every token
    flipped, pairs, n_pairs = coef.copy(), coef.copy(), 0
    for t in range(coef.shape[0]):
        a, b = int(n_q[t]), int(n[t])
        flipped[t, a:b] *= -1
        q_feats = idx[t, :a].tolist()
        for j in range(a, b):
            if int(idx[t, j]) in q_feats:                                  # the feature survives from both lists
                pairs[t, j] = 0
                pairs[t, q_feats.index(int(idx[t, j]))] = 0
                n_pairs += 1
    assert n_pairs > 0 and (n > 1).any()
    for name, got in (("dropped", out_of(idx, dropped)), ("flipped", out_of(idx, flipped)), ("pairs", out_of(idx, pairs)),
                      ("b_dec", out_of(idx, coef, b_dec[None, :]))):
        assert (np.abs(got - comp) > bnd).any(), name


def test_survival_rule_cases():
    rng = np.random.default_rng(3)
    d, n_feat, k, T = 6, 64, 4, 3
    W = rng.standard_normal((n_feat, d)).astype(np.float32)
    x = rng.standard_normal((T, d)).astype(np.float32)
    x[0, 0], x[1, 1] = -0.0, np.float32(np.nan)
    xb = x.view(np.uint32).copy()
    xb[1, 2] = 0x7FC12345                                                  # a NaN payload
    v = np.abs(rng.standard_normal((T, k))).astype(np.float32) + 1
    i = np.stack([rng.permutation(n_feat)[:k] for _ in range(T)]).astype(np.int32)
    out, n, _ = iref.intervene(xb, "f32", v, i, v.copy(), i.copy(), W)
    assert (n == 0).all() and np.array_equal(out, xb)                      # identical lists: x's bits
    # +-0 entries never survive: zero fill with different indices
    vz, i2 = v.copy(), i.copy()
    vz[:, 2:] = 0
    vq = vz.copy()
    vq[:, 3] = -0.0
    i2[:, 2:] = (i[:, 2:] + 7) % n_feat
    out, n, _ = iref.intervene(xb, "f32", vz, i, vq, i2, W)
    assert (n == 0).all() and np.array_equal(out, xb)
    # disjoint lists: 2 k survivors, Q's in slot order with +value, then P's with -value
    iq = (i + 1 + np.arange(T)[:, None] * 0) % n_feat
    iq = np.stack([np.setdiff1d(np.arange(n_feat), i[t])[:k] for t in range(T)]).astype(np.int32)
    idx, coef, n, _ = iref.diff_lists(v, i, 2 * v, iq)
    assert (n == 2 * k).all()
    assert np.array_equal(idx, np.concatenate([iq, i], 1)) and np.array_equal(coef, np.concatenate([2 * v, -v], 1))
    # the same feature with another value survives twice
    v2 = v.copy()
    v2[:, 1] *= 3
    idx, coef, n, _ = iref.diff_lists(v, i, v2, i)
    assert (n == 2).all() and np.array_equal(idx[:, 0], i[:, 1]) and np.array_equal(idx[:, 1], i[:, 1])
    assert np.array_equal(coef[:, 0], v2[:, 1]) and np.array_equal(coef[:, 1], -v[:, 1])
    # an out-of-range survivor is skipped and flagged
    ibad = i.astype(np.int64)
    ibad[0, 0] = n_feat + 5
    idx, coef, n, flagged = iref.diff_lists(v, i, v, ibad, n_feat)
    assert flagged and n[0] == 1 and idx[0, 0] == i[0, 0] and coef[0, 0] == -v[0, 0] and (n[1:] == 0).all()
    # conversions: round to nearest even, ties included
    assert iref.from_f32(np.array([1.00390625, 1.01171875], dtype=np.float32), "bf16").tolist() == [0x3F80, 0x3F82]
    assert iref.from_f32(np.array([1.00048828125], dtype=np.float32), "f16").tolist() == [0x3C00]


# ---- host layer: these fail without the feature --------------------------------------------------------------------------
def _arg_count(header, name):
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, header, re.S)
    assert m, name
    return m.group(1).count(",") + 1


def test_symbols_prototypes_and_argument_errors_of_the_entry_points():
    from msae import _hip

    header = (REPO / "include" / "msae.h").read_text()
    lib = ctypes.CDLL(str(_hip.LIB_PATH))
    for name in ("msae_delta_decode_f32", "msae_delta_decode_i64_f32"):
        assert hasattr(lib, name) and name in _hip.PROTOTYPES
        res, args = _hip.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == _arg_count(header, name) == 16
    assert _hip.load().msae_abi_version() == 4 == _hip.ABI_VERSION
    one = ctypes.c_void_p(16)
    for f in (_hip.load().msae_delta_decode_f32, _hip.load().msae_delta_decode_i64_f32):
        def call(T=4, k=8, ld_p=8, ld_q=8, n=1000, d=16, dt=0, ptrs=None, status=one):
            p = ptrs or [one] * 7
            return f(p[0], dt, p[1], p[2], ld_p, p[3], p[4], ld_q, p[5], T, k, n, d, p[6], status, None)

        assert call(T=-1) == -1 and call(k=0) == -1 and call(k=4097, ld_p=5000, ld_q=5000) == -1
        assert call(ld_p=7) == -1 and call(ld_q=7) == -1 and call(dt=3) == -1 and call(dt=-1) == -1
        for hole in range(7):
            p = [one] * 7
            p[hole] = None
            assert call(ptrs=p) == -1
        assert call(T=0) == 0 and call(T=0, status=None) == 0 and call(T=0, k=4096, ld_p=4096, ld_q=5000) == 0


def test_op_argument_errors_before_any_device_work():
    from msae import ops

    x, W = torch.zeros(3, 16), torch.zeros(64, 16)
    v, i = torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.int64)
    good = dict(x=x, plain_acts=v, plain_idx=i, edit_acts=v, edit_idx=i, W_dec=W)
    for bad in (dict(W_dec=torch.zeros(64, 8)), dict(x=x.double()), dict(edit_acts=torch.zeros(3, 5)),
                dict(plain_idx=i.to(torch.int32)), dict(plain_idx=i.to(torch.int16), edit_idx=i.to(torch.int16)),
                dict(plain_acts=v.double()), dict(x=torch.zeros(4, 16)), dict(out=torch.zeros(3, 16, dtype=torch.float16)),
                dict(out=torch.zeros(16, 3).t()),
                dict(plain_acts=torch.zeros(3, 5000), plain_idx=torch.zeros(3, 5000, dtype=torch.int64),
                     edit_acts=torch.zeros(3, 5000), edit_idx=torch.zeros(3, 5000, dtype=torch.int64))):
        with pytest.raises(ValueError, match="delta_decode"):
            ops.delta_decode(**{**good, **bad})
    with pytest.raises(RuntimeError, match="MI355X"):                      # valid arguments reach the device check
        ops.delta_decode(**good)
    with pytest.raises(RuntimeError, match="inference"):
        ops.delta_decode(**{**good, "x": x.clone().requires_grad_()})
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        o = torch.ops.msae.delta_decode(torch.empty(2, 3, 16, dtype=torch.bfloat16), torch.empty(6, 40)[:, :4],
                                        torch.empty(6, 40, dtype=torch.int64)[:, :4], torch.empty(6, 4),
                                        torch.empty(6, 4, dtype=torch.int64), torch.empty(64, 16))
        assert o.shape == (2, 3, 16) and o.dtype == torch.bfloat16


def test_intervene_and_reconstruct_argument_errors_before_any_device_work():
    from msae import Sae, SaeConfig
    from msae.features import FeatureEdits, RowEdits, sae_reconstruct

    sae = Sae(16, SaeConfig(num_latents=64, k=4)).eval()
    fe = FeatureEdits(64, set={5: 2.0}, device="cpu")
    re_ = RowEdits(64, [dict(set={3: 1.0}), None, dict(zero=[5, 6])], device="cpu")
    x, x3 = torch.zeros(3, 16), torch.zeros(3, 2, 16)
    for args in ((x, None), (x, {5: 2.0}), (torch.zeros(3, 8), fe), (x.double(), fe), (x, FeatureEdits(65, zero=[1], device="cpu")),
                 (x, FeatureEdits(64, zero=range(61), device="cpu")), (torch.zeros(2, 2, 16), re_)):
        with pytest.raises(ValueError):
            sae.intervene(*args)
    with pytest.raises(ValueError, match="edit_group"):
        sae.intervene(x, fe, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="edit_group"):
        sae.intervene(x3, re_, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="inference"):
        sae.intervene(x.clone().requires_grad_(), fe)
    with pytest.raises(RuntimeError, match="MI355X"):                      # valid arguments reach the device check
        sae.intervene(x3, re_)
    with pytest.raises(ValueError, match="out_dtype"):
        sae_reconstruct(sae, x, edits=fe, preserve_error=True, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="not both"):
        sae_reconstruct(sae, x, edits=fe, set_feature=3, preserve_error=True)
    with pytest.raises(ValueError, match="edit_group"):
        sae_reconstruct(sae, x, edits=fe, edit_group=torch.zeros(3, dtype=torch.int32), preserve_error=True)
    with pytest.raises(NotImplementedError, match="Sae"):
        sae_reconstruct(object(), x, set_feature=3, preserve_error=True)
    with torch.no_grad():                                                  # no edit under no_grad: the hidden state itself
        assert sae_reconstruct(sae, x, preserve_error=True) is x


def test_hooks_build_todays_objects_when_the_switch_is_off(monkeypatch):
    from msae import Sae, SaeConfig
    from msae.features import RowEdits, attribution_sae_hook, clamp_features_max, clamp_features_rows, hooks
    from msae.features.steering import SteeringController

    monkeypatch.delenv("MSAE_HOOK_GRAPH", raising=False)
    sae = Sae(16, SaeConfig(num_latents=64, k=4)).eval()
    layer = torch.nn.Identity()
    calls = []

    def reconstruct(sae_, hidden, **kw):
        calls.append(kw)
        return hidden.to(kw.get("out_dtype") or hidden.dtype)

    monkeypatch.setattr(hooks, "sae_reconstruct", reconstruct)
    h3, h1 = torch.zeros(2, 5, 16), torch.zeros(2, 1, 16)
    off = clamp_features_max(sae, 5, layer, k=3.0)
    assert isinstance(off[0].step_graph, hooks._DecodeStepGraph) and not hasattr(off[0], "edits")
    layer(h3[:1])
    assert calls.pop() == dict(set_feature=5, set_value=3.0, out_dtype=torch.float16, edits=None)
    off[0].remove()
    on = clamp_features_max(sae, 5, layer, k=3.0, preserve_error=True)
    assert on[0].step_graph is None and on[0].edits.features == (5,) and on[0].edits.values == (3.0,)
    assert layer(h1[:1]) is not None and not calls                         # S = 1: untouched, no SAE call
    out = layer(h3[:1])
    kw = calls.pop()
    assert kw == dict(edits=on[0].edits, preserve_error=True) and out.dtype == h3.dtype
    on[0].remove()
    rows_off = clamp_features_rows(sae, [5, None], layer, k=3.0)
    assert isinstance(rows_off[0].step_graph, hooks._DecodeStepGraph) and isinstance(rows_off[0].edits, RowEdits)
    layer(h3)
    assert calls.pop() == dict(out_dtype=torch.float16, edits=rows_off[0].edits)
    layer(h1)
    assert calls.pop() == dict(out_dtype=torch.float16)
    rows_off[0].remove()
    rows_on = clamp_features_rows(sae, [5, None], layer, k=3.0, preserve_error=True)
    assert rows_on[0].step_graph is None
    assert layer(h1) is h1 and not calls
    layer(h3)
    assert calls.pop() == dict(edits=rows_on[0].edits, preserve_error=True)
    with pytest.raises(ValueError, match="batch"):
        layer(torch.zeros(3, 5, 16))
    rows_on[0].remove()
    for flag, want in ((False, dict(zero_feature=7, edits=None, edit_group=None, out_dtype=torch.float16, differentiable=True)),
                       (True, None)):
        cache = {}
        hk = layer.register_forward_hook(attribution_sae_hook({"L": sae}, {layer: "L"}, cache, 7, **({"preserve_error": True} if flag else {})))
        layer(h3)
        hk.remove()
        kw = calls.pop()
        if want is not None:
            assert kw == want
        else:
            assert kw["preserve_error"] is True and kw["edits"].features == (7,) and kw["edits"].kinds == (1,) and "out_dtype" not in kw
    with pytest.raises(NotImplementedError, match="Sae"):
        clamp_features_max(object(), 5, layer, preserve_error=True)
    with pytest.raises(NotImplementedError, match="Sae"):
        SteeringController.__init__(SteeringController.__new__(SteeringController), object(), "m", [1], None, None, "p",
                                    preserve_error=True)


def test_launcher_flags():
    from msae.config import parse_attribution_config
    from msae.launch.features import steering as launch

    assert launch.parse_argument(["-t", "x"]).preserve_error is False
    assert launch.parse_argument(["-t", "x", "--preserve-error"]).preserve_error is True
    assert launch.parse_argument(["-t", "x", "--preserve_error", "--batch-features", "4"]).preserve_error is True
    with pytest.raises(SystemExit):
        launch.parse_argument(["-t", "x", "--preserve-error", "--shard-sae"])
    assert parse_attribution_config(["m"]).preserve_error is False
    cfg = parse_attribution_config(["m", "--preserve-error", "--method", "exact"])
    assert cfg.preserve_error is True and cfg.method == "exact" and cfg.to_dict()["preserve_error"] is True
    assert parse_attribution_config(["m", "--preserve_error"]).preserve_error is True


def test_flags_through_the_compat_alias():
    import os
    import subprocess
    import sys

    pkg = REPO / "multimodal-sae_amd"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(pkg), str(pkg / "compat")]))
    code = ("from sae_auto_interp.launch.features import steering as s; from sae_auto_interp.config import parse_attribution_config as p;"
            "assert s.parse_argument(['-t', 'x', '--preserve-error']).preserve_error;"
            "assert p(['m', '--preserve-error']).preserve_error; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
