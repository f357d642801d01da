"""CPU: the batch-level selection without a GPU -- the plain-torch host paths of ops.batch_kth,
ops.list_filter, ops.batch_select and ops.decode(lengths=) against the sorting restatement (tests/batch_select_ref.py), the
properties the definition promises (token order does not matter, ties at theta are all kept), the errors of the public
interface, the checkpoint format of a "batchtopk" Sae (and that a TopK Sae's is untouched), the workspace helper, and the
trainer's dead-feature bookkeeping (a feature named only by dropped slots has not fired)."""
import json

import numpy as np
import pytest
import torch

import batch_select_ref as ref


def _lists(rng, T, C, N, scale=1.0, zeros=0.3):
    """canonical [T, C] lists of relu-like rows: some rows run out of positive values"""
    pre = rng.standard_normal((T, N)).astype(np.float32) * np.float32(scale)
    pre[rng.random((T, N)) < zeros] = 0.0
    pre = np.maximum(pre, 0)
    return ref.canonical_lists(pre, C)


@pytest.mark.parametrize("T,C,K", [(1, 1, 1), (37, 13, 100), (37, 13, 1), (37, 13, 10 ** 6), (5, 8, 40)])
def test_batch_kth_host_equals_the_restatement(T, C, K):
    from msae import ops

    rng = np.random.default_rng(T * 100 + C)
    vals, _ = _lists(rng, T, C, 64)
    th, n_pos = ops.batch_kth(torch.from_numpy(vals), K)
    rt, rn = ref.theta(vals, K)
    assert th.dtype == torch.float32 and th.shape == () and n_pos.dtype == torch.int32
    assert np.array_equal(np.float32(th.item()).view(np.uint32), rt.view(np.uint32)) and int(n_pos) == rn
    wide = np.concatenate([vals, np.full((T, 3), 99.0, np.float32)], 1)             # the [:, :C] view of a wider list
    th2, _ = ops.batch_kth(torch.from_numpy(wide)[:, :C], K)
    assert float(th2) == float(th)


def test_batch_kth_host_special_values():
    from msae import ops

    v = np.array([[np.nan, -0.0, -3.0, 0.0], [np.inf, 1e-45, 2.0, -np.inf]], np.float32)
    for K, want in ((1, np.inf), (2, 2.0), (3, 1e-45), (4, 1e-45), (100, 1e-45)):
        th, n_pos = ops.batch_kth(torch.from_numpy(v), K)
        assert np.float32(th.item()) == np.float32(want) == ref.theta(v, K)[0] and int(n_pos) == 3
    th, n_pos = ops.batch_kth(torch.from_numpy(np.array([[np.nan, -1.0, 0.0]], np.float32)), 2)
    assert float(th) == np.inf and int(n_pos) == 0                                   # P empty
    with pytest.raises(ValueError):
        ops.batch_kth(torch.from_numpy(v), 0)
    with pytest.raises(ValueError):
        ops.batch_kth(torch.from_numpy(v).double(), 1)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("table", [False, True])
def test_list_filter_host_equals_the_restatement(table, wide):
    from msae import ops

    rng = np.random.default_rng(3 + table)
    T, C, N = 23, 9, 50
    vals, idx = _lists(rng, T, C, N)
    vals[3, 2] = np.nan
    idx[5, 1] = N + 7                          # outside the table: dropped in table mode, never looked up
    idx[6, 0] = -1
    idx = idx if wide else idx.astype(np.int32)
    tf = (rng.random(N).astype(np.float32) * 1.5) if table else None
    th = np.float32(tf.min()) if table else np.float32(0.8)
    vo, io, ln, n_sat = ops.list_filter(torch.from_numpy(vals), torch.from_numpy(idx), None if table else float(th),
                                        None if tf is None else torch.from_numpy(tf))
    rv, ri, rl, rs = ref.list_filter(vals, idx, th, tf)
    assert np.array_equal(vo.numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(io.numpy(), ri)
    assert io.dtype == (torch.int64 if wide else torch.int32)
    assert np.array_equal(ln.numpy(), rl) and ln.dtype == torch.int32 and int(n_sat) == int(rs.sum())
    # the counter accumulates
    acc = torch.full((), 5, dtype=torch.int32)
    ops.list_filter(torch.from_numpy(vals), torch.from_numpy(idx), float(th), None if tf is None else torch.from_numpy(tf),
                    n_saturated=acc)
    assert int(acc) == 5 + int(rs.sum())
    # every row keeps its own set of indices
    assert np.array_equal(np.sort(io.numpy(), 1), np.sort(idx, 1))


def test_batch_select_host_permutation_invariance_and_ties():
    from msae import ops

    rng = np.random.default_rng(11)
    T, C, N, k = 40, 12, 80, 3
    vals, idx = _lists(rng, T, C, N)
    # plant a tie AT theta across several tokens: theta of this batch, written into three more rows' lists in order
    th0, _ = ref.theta(vals, T * k)
    for t in (1, 7, 20):
        row = np.sort(np.concatenate([vals[t, :-1], [th0]]))[::-1]
        vals[t] = row
    kept, ln, th, n_sat = ops.batch_select(torch.from_numpy(vals), torch.from_numpy(idx), k)
    rv, _, rl, rt, rs = ref.batch_select(vals, idx, k)
    assert float(th) == float(rt) and np.array_equal(kept.numpy().view(np.uint32), rv.view(np.uint32))
    assert np.array_equal(ln.numpy(), rl) and int(n_sat) == int(rs.sum())
    n_ties = int((vals == rt).sum())
    assert n_ties >= 3 and int((kept.numpy() == rt).sum()) == n_ties                 # ties at theta: all kept
    assert int(ln.sum()) >= min(T * k, int(ref.positive(vals).sum()))
    assert int(ln.sum()) == int((ref.positive(vals) & (vals >= rt)).sum())
    # a permutation of the tokens permutes the result and leaves theta alone
    perm = rng.permutation(T)
    kp, lp, tp, _ = ops.batch_select(torch.from_numpy(vals[perm]), torch.from_numpy(idx[perm]), k)
    assert float(tp) == float(th) and torch.equal(kp, kept[perm]) and torch.equal(lp, ln[perm])
    # the gradient is the keep mask's
    a = torch.from_numpy(vals).requires_grad_()
    out = ops.batch_select(a, torch.from_numpy(idx), k)
    assert not out[1].requires_grad and not out[2].requires_grad
    (out[0] * 2).sum().backward()
    assert torch.equal(a.grad, 2.0 * (kept > 0))
    with pytest.raises(ValueError):
        ops.batch_select(torch.from_numpy(vals), torch.from_numpy(idx), C + 1)


def test_decode_with_lengths_host_path_and_gradients():
    from msae import ops

    rng = np.random.default_rng(5)
    T, C, N, d = 9, 6, 30, 10
    vals, idx = _lists(rng, T, C, N, zeros=0.0)
    ln = rng.integers(0, C + 1, T).astype(np.int32)
    ln[0], ln[1] = 0, C
    W, b = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    poison_v, poison_i = vals.copy(), idx.copy()
    for t in range(T):
        poison_v[t, ln[t]:] = np.nan
        poison_i[t, ln[t]:] = N + 5
    want = np.stack([(vals[t, :ln[t], None].astype(np.float64) * W[idx[t, :ln[t]]]).sum(0) + b for t in range(T)])
    a = torch.from_numpy(poison_v).requires_grad_()
    Wt = torch.from_numpy(W).requires_grad_()
    out = ops.decode(torch.from_numpy(poison_i), a, Wt, torch.from_numpy(b), torch.from_numpy(ln))
    assert np.allclose(out.detach().numpy(), want, rtol=1e-5, atol=1e-5)
    out.sum().backward()
    live = np.arange(C)[None] < ln[:, None]
    assert np.isfinite(a.grad.numpy()).all() and np.isfinite(Wt.grad.numpy()).all()
    assert np.array_equal(a.grad.numpy() != 0, live)                                 # (W rows sum to non-zero values)
    lmax = torch.from_numpy(np.full(T, C + 9, np.int32))                             # clamped
    full = ops.decode(torch.from_numpy(idx), torch.from_numpy(vals), torch.from_numpy(W), None, lmax)
    assert np.allclose(full.numpy(), np.einsum("tc,tcd->td", vals, W[idx]), rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError):
        ops.decode(torch.from_numpy(idx), torch.from_numpy(vals), torch.from_numpy(W), None)   # no lengths: HIP only, as ever


def test_workspace_helper_returns_zero_outside_the_envelope():
    from msae import _hip

    lib = _hip.load()
    assert lib.msae_batch_kth_ws_bytes(1, 1) == lib.msae_batch_kth_ws_bytes(8192, 128) == lib.msae_batch_kth_ws_bytes(4096, 4096)
    assert lib.msae_batch_kth_ws_bytes(1, 1) == 4 * 256 * 4
    for T, C in ((0, 8), (-1, 8), (8, 0), (8, -3), (4097, 4096), (1 << 24, 2), ((1 << 24) + 1, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.msae_batch_kth_ws_bytes(T, C) == 0, (T, C)
    # the entry refuses the same shapes, and a missing workspace, before it looks at a pointer
    assert lib.msae_batch_kth_f32(None, 0, 8, 8, 1, None, None, None, 0, None) == -1
    assert lib.msae_batch_kth_f32(None, 4097, 4096, 4096, 1, None, None, None, 0, None) == -1


# ---- the public interface --------------------------------------------------------------------------------------------------
def _sae(activation="batchtopk", d=16, N=64, k=4, **cfg):
    from msae import Sae, SaeConfig

    return Sae(d, SaeConfig(num_latents=N, k=k, activation=activation, **cfg), device="cpu")


def test_config_fields_defaults_and_errors():
    from msae import SaeConfig

    assert SaeConfig().activation == "topk" and SaeConfig().batch_cap == 0 and SaeConfig(k=8).cap == 8
    assert "activation" not in SaeConfig().to_dict() and "batch_cap" not in SaeConfig().to_dict()
    assert SaeConfig(k=8, activation="batchtopk").cap == 32 and SaeConfig(k=100, activation="batchtopk").cap == 256
    assert SaeConfig(k=8, activation="batchtopk", batch_cap=48).cap == 48
    assert SaeConfig(k=8, activation="batchtopk").to_dict()["activation"] == "batchtopk"
    assert "batch_cap" not in SaeConfig(k=8, activation="batchtopk").to_dict()
    assert SaeConfig(k=8, activation="batchtopk", batch_cap=48).to_dict()["batch_cap"] == 48
    for bad in (dict(activation="jumprelu"), dict(activation="batchtopk", multi_topk=True),
                dict(k=8, activation="batchtopk", batch_cap=4), dict(batch_cap=-1), dict(k=300, activation="batchtopk"),
                dict(k=8, activation="batchtopk", batch_cap=5000)):
        with pytest.raises(ValueError):
            SaeConfig(**bad)


def test_checkpoint_roundtrip_and_an_untouched_topk_format(tmp_path):
    from msae import Sae

    topk = _sae("topk")
    assert sorted(topk.state_dict()) == ["W_dec", "b_dec", "encoder.bias", "encoder.weight"] and not hasattr(topk, "threshold")
    topk.save_to_disk(tmp_path / "topk")
    assert json.loads((tmp_path / "topk" / "cfg.json").read_text()) == {
        "expansion_factor": 32, "normalize_decoder": True, "num_latents": 64, "k": 4, "multi_topk": False, "signed": False,
        "d_in": 16}
    sae = _sae(batch_cap=12)
    assert sorted(sae.state_dict()) == ["W_dec", "b_dec", "encoder.bias", "encoder.weight", "threshold"]
    assert sae.threshold.dtype == torch.float32 and sae.threshold.shape == () and float(sae.threshold) == -1.0
    assert [n for n, _ in sae.named_parameters()] == [n for n, _ in topk.named_parameters()]      # a buffer, not a parameter
    sae.set_threshold(0.375)
    sae.save_to_disk(tmp_path / "b")
    cfg = json.loads((tmp_path / "b" / "cfg.json").read_text())
    assert cfg["activation"] == "batchtopk" and cfg["batch_cap"] == 12 and cfg["k"] == 4
    back = Sae.load_from_disk(tmp_path / "b")
    assert back.cfg == sae.cfg and float(back.threshold) == 0.375 and back.cfg.cap == 12
    for n, t in sae.state_dict().items():
        assert torch.equal(t, back.state_dict()[n]), n
    assert Sae.load_from_disk(tmp_path / "topk").cfg == topk.cfg


def test_errors_of_the_threshold_encode():
    from msae.features import FeatureEdits

    sae, topk = _sae(), _sae("topk")
    x = torch.zeros(3, 16)
    with pytest.raises(RuntimeError, match="not learned"):
        sae.encode(x)                                              # the buffer is still -1
    for s in (sae, topk):
        for kw in (dict(set_feature=3, set_value=1.0), dict(zero_feature=2),
                   dict(edits=FeatureEdits(64, {3: 1.0}, device="cpu"))):
            with pytest.raises(ValueError, match="threshold"):
                s.encode(x, threshold=0.5, **kw)
        with pytest.raises(NotImplementedError, match="table"):
            s.encode(x.clone().requires_grad_(), threshold=torch.zeros(64))
        with pytest.raises(ValueError):
            s.encode(x, threshold=torch.zeros(63))                 # neither a scalar nor [N]
        with pytest.raises(ValueError):
            s.encode(x, threshold=0.5, cap=0)
    with pytest.raises(ValueError):
        topk.encode(x, cap=8)                                      # cap / return_lengths without a threshold
    with pytest.raises(ValueError):
        topk.encode(x, return_lengths=True)
    with pytest.raises(ValueError):
        topk.set_threshold(1.0)
    for bad in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            sae.set_threshold(bad)


def test_what_is_not_built_says_so():
    from msae.features import FeatureEdits
    from msae.features.hooks import attribution_sae_hook, clamp_features_max, clamp_features_rows, sae_reconstruct
    from msae.features.patching.utils import sae_splice_hook
    from msae.parallel import ShardedSae

    sae = _sae()
    x = torch.zeros(3, 16)
    mod = torch.nn.Linear(2, 2)
    with pytest.raises(NotImplementedError, match="batchtopk"):
        sae.recon_error(x)
    with pytest.raises(NotImplementedError, match="batchtopk"):
        sae.intervene(x, FeatureEdits(64, {3: 1.0}, device="cpu"))
    with pytest.raises(NotImplementedError, match="batchtopk"):
        sae_reconstruct(sae, x)
    with pytest.raises(NotImplementedError, match="batchtopk"):
        clamp_features_max(sae, 3, mod)
    with pytest.raises(NotImplementedError, match="batchtopk"):
        clamp_features_rows(sae, [3, None], mod)
    with pytest.raises(NotImplementedError, match="batchtopk"):
        attribution_sae_hook({"m": sae}, {mod: "m"}, {})
    with pytest.raises(NotImplementedError, match="batchtopk"):
        sae_splice_hook({"m": sae}, {mod: "m"}, {})
    with pytest.raises(NotImplementedError, match="threshold"):
        ShardedSae.encode(object.__new__(ShardedSae), x, threshold=0.5)
    assert len(mod._forward_hooks) == 0


# ---- trainer bookkeeping ---------------------------------------------------------------------------------------------------
def _cpu_train_step(sae, **kw):
    """SaeTrainStep with the forward restated in dense torch ops around the NEW ops' host paths, and a plain Adam."""
    from msae import ops
    from msae.sae.sae import BatchForwardOutput
    from msae.train import SaeTrainStep

    class CpuTrainStep(SaeTrainStep):
        def _forward(self, x, dead_mask):
            s = self.sae
            pre = torch.relu((x - s.b_dec) @ s.encoder.weight.T + s.encoder.bias)
            acts, idx = pre.topk(s.cfg.cap, dim=-1)
            kept, lengths, theta, n_sat = ops.batch_select(acts, idx, s.cfg.k)
            out = ops.decode(idx, kept, s.W_dec, s.b_dec, lengths)
            fvu = (out - x).pow(2).sum() / (x - x.mean(0)).pow(2).sum()
            zero = out.new_zeros(())
            return BatchForwardOutput(out, kept, idx, fvu, zero, zero, lengths=lengths, theta=theta, n_saturated=n_sat)

        def _update(self, lr):
            with torch.no_grad():
                for p in self.params:
                    p.add_(p.grad, alpha=-lr)
                    p.grad = None

    return CpuTrainStep(sae, lr=1e-3, **kw)


def test_a_feature_named_only_by_dropped_slots_has_not_fired():
    import synth

    d, N, k, C, T = 16, 64, 2, 8, 12
    sae = _sae(d=d, N=N, k=k, batch_cap=C)
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, N, seed=9)
    with torch.no_grad():
        sae.encoder.weight.copy_(torch.from_numpy(W_enc)); sae.encoder.bias.copy_(torch.from_numpy(b_enc))
        sae.W_dec.copy_(torch.from_numpy(W_dec)); sae.b_dec.copy_(torch.from_numpy(b_dec))
    ts = _cpu_train_step(sae, micro_acc_steps=2, threshold_lr=0.25)
    x = torch.from_numpy(synth.activations(T, d, seed=3, bf16=False, n_outlier=1))
    # what the two chunks select, before the step moves the weights
    listed, kept, thetas = set(), set(), []
    with torch.no_grad():
        for chunk in x.chunk(2):
            out = ts._forward(chunk, None)
            live = torch.arange(C)[None] < out.lengths[:, None]
            listed |= set(out.latent_indices.flatten().tolist())
            kept |= set(out.latent_indices[live].tolist())
            thetas.append(float(out.theta))
            assert int(out.lengths.sum()) >= chunk.shape[0] * k
    assert kept < listed, "the test needs a feature that only dropped slots name"
    res = ts.step(x)
    since = ts.num_tokens_since_fired
    for f in range(N):
        assert int(since[f]) == (0 if f in kept else T), f
    # theta: the first chunk's value is copied, the second is folded in at the trainer's rate
    want = np.float32(thetas[0]) + np.float32(0.25) * (np.float32(thetas[1]) - np.float32(thetas[0]))
    assert float(sae.threshold) == pytest.approx(float(want), rel=1e-6)
    assert float(res["theta"]) == pytest.approx(sum(thetas) / 2, rel=1e-6) and res["n_saturated"].dtype == torch.int32
    # a non-finite theta is skipped on the device
    before = float(sae.threshold)
    ts._fold_threshold(torch.tensor(float("inf")))
    ts._fold_threshold(torch.tensor(float("nan")))
    assert float(sae.threshold) == before
    # a TopK trainer's result has no new keys
    from msae.train import SaeTrainStep
    assert SaeTrainStep(_sae("topk")).batch_topk is False
