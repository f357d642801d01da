"""CPU: the JumpReLU activation without a GPU -- SaeConfig / Sae plumbing of activation="jump", the
plain-torch host path of ops.jump_select against the sorting restatement (tests/jump_ref.py), the equality with a literal
dense JumpReLU in float64 whenever no row saturates, three SaeTrainStep steps against a literal float64 loop, and the exact
zero of the threshold gradient when nothing lies inside the band."""
import json
import math

import numpy as np
import pytest
import torch

import jump_ref as ref

F64 = torch.float64


# ---- configuration and checkpoints ---------------------------------------------------------------------------------------------
def test_config_defaults_and_errors():
    from msae import SaeConfig

    assert SaeConfig.ACTIVATIONS == ("topk", "batchtopk", "jump")
    cfg = SaeConfig(k=8, activation="jump")
    assert cfg.jump_bandwidth == 1e-3 and cfg.jump_init == 1e-3 and cfg.cap == 32
    assert SaeConfig(k=100, activation="jump").cap == 256 and SaeConfig(k=8, activation="jump", batch_cap=20).cap == 20
    for kw in (dict(activation="jumprelu"), dict(activation="jump", multi_topk=True),
               dict(activation="jump", matryoshka=[64, 128], num_latents=128), dict(activation="jump", batch_cap=257),
               dict(activation="jump", k=300), dict(activation="jump", k=8, batch_cap=4),
               dict(activation="jump", jump_bandwidth=0.0), dict(activation="jump", jump_bandwidth=-1.0),
               dict(activation="jump", jump_bandwidth=float("inf")), dict(activation="jump", jump_bandwidth=float("nan")),
               dict(activation="jump", jump_init=0.0), dict(activation="jump", jump_init=float("nan")),
               dict(activation="jump", jump_init=float("inf"))):
        with pytest.raises(ValueError):
            SaeConfig(**kw)
    with pytest.raises(ValueError, match="follow-up"):
        SaeConfig(activation="jump", matryoshka=[64, 128], num_latents=128)
    # the new fields are written for "jump" alone
    assert "jump_bandwidth" not in SaeConfig().to_dict() and "jump_init" not in SaeConfig(activation="batchtopk").to_dict()
    d = SaeConfig(activation="jump", jump_bandwidth=0.25, jump_init=0.5).to_dict()
    assert d["activation"] == "jump" and d["jump_bandwidth"] == 0.25 and d["jump_init"] == 0.5


def test_checkpoint_round_trip_and_untouched_formats(tmp_path):
    from msae import Sae, SaeConfig

    sae = Sae(16, SaeConfig(num_latents=96, k=4, activation="jump", jump_init=0.5, jump_bandwidth=0.25))
    assert sae.log_threshold.dtype == torch.float32 and sae.log_threshold.shape == (96,) and sae.log_threshold.requires_grad
    assert torch.equal(sae.log_threshold.detach(), torch.full((96,), math.log(0.5), dtype=torch.float32))
    with torch.no_grad():
        sae.log_threshold.add_(torch.linspace(-1, 1, 96))
    sae.save_to_disk(tmp_path / "jump")
    cfg = json.loads((tmp_path / "jump" / "cfg.json").read_text())
    assert cfg["activation"] == "jump" and cfg["jump_bandwidth"] == 0.25 and cfg["jump_init"] == 0.5
    back = Sae.load_from_disk(tmp_path / "jump")
    assert back.cfg == sae.cfg and torch.equal(back.log_threshold, sae.log_threshold)
    assert set(sae.state_dict()) == {"encoder.weight", "encoder.bias", "W_dec", "b_dec", "log_threshold"}
    # TopK and BatchTopK: state dict and cfg.json are what they were
    for act, keys in (("topk", set()), ("batchtopk", {"threshold"})):
        other = Sae(16, SaeConfig(num_latents=96, k=4, activation=act))
        assert set(other.state_dict()) == {"encoder.weight", "encoder.bias", "W_dec", "b_dec"} | keys
        other.save_to_disk(tmp_path / act)
        c = json.loads((tmp_path / act / "cfg.json").read_text())
        assert not any(k.startswith("jump") for k in c) and ("activation" in c) == (act != "topk")
        assert not hasattr(other, "log_threshold")


def test_set_threshold_truncate_and_guards():
    from msae import Sae, SaeConfig
    from msae.features import hooks
    from msae.parallel import ShardedSae

    sae = Sae(16, SaeConfig(num_latents=96, k=4, activation="jump"))
    sae.set_threshold(0.75)
    assert torch.equal(sae.log_threshold.detach(), torch.full((96,), math.log(0.75), dtype=torch.float32))
    table = torch.linspace(0.1, 2.0, 96)
    sae.set_threshold(table)
    assert torch.equal(sae.log_threshold.detach(), table.log())
    for bad in (0.0, -1.0, float("inf"), float("nan"), torch.zeros(96), torch.ones(95), torch.full((96,), float("inf"))):
        with pytest.raises(ValueError):
            sae.set_threshold(bad)
    with pytest.raises(ValueError):
        Sae(16, SaeConfig(num_latents=96, k=4)).set_threshold(1.0)                  # a TopK Sae has nothing to set
    cut = sae.truncate(48)
    assert cut.log_threshold.shape == (48,) and torch.equal(cut.log_threshold, sae.log_threshold[:48])
    assert cut.log_threshold.data_ptr() == sae.log_threshold.data_ptr()             # a view, as the other parameters
    x = torch.zeros(3, 16)
    for call in (lambda: sae.recon_error(x), lambda: sae.intervene(x, None), lambda: hooks.sae_reconstruct(sae, x),
                 lambda: ShardedSae.from_sae(sae)):
        with pytest.raises(NotImplementedError, match="jump"):
            call()
    with pytest.raises(NotImplementedError, match="per-feature threshold table"):
        sae.train()
        sae.encode(x, threshold=torch.ones(96))                                     # a foreign table: still not built


# ---- the host path against the restatement -------------------------------------------------------------------------------------
def _hostile(seed, T=23, C=9, N=50, eps=0.25):
    rng = np.random.default_rng(seed)
    theta = (0.9 + 0.6 * rng.random(N)).astype(np.float32)
    theta[7] = np.inf                                                               # never kept, never in the band
    vals, idx = ref.lists_around(rng, T, C, N, theta, eps)
    ref.plant_hostile(vals, idx, theta, eps)
    return vals, idx, theta, eps


def _bits(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("wide", [False, True])
def test_host_path_equals_the_restatement_on_hostile_values(wide):
    from msae import ops

    vals, idx, theta, eps = _hostile(3)
    sel = ref.select(vals, idx, theta, eps)
    assert sel["kept"].any() and sel["near"].any() and (~sel["kept"] & ~sel["near"]).any()
    assert (sel["band"] & sel["kept"]).any() and (sel["kept"] & ~sel["band"]).any()
    i_t = torch.from_numpy(idx if wide else idx.astype(np.int32))
    a = torch.from_numpy(vals).requires_grad_()
    th = torch.from_numpy(theta).requires_grad_()
    kept, io, ln, reach, l0, n_sat = ops.jump_select(a, i_t, th, eps)
    assert np.array_equal(_bits(kept.detach()), _bits(sel["vals"])) and np.array_equal(io.numpy(), sel["idx"])
    assert io.dtype == i_t.dtype and ln.dtype == reach.dtype == torch.int32 and l0.dtype == torch.float32
    assert np.array_equal(ln.numpy(), sel["len"]) and np.array_equal(reach.numpy(), sel["reach"])
    assert float(l0.detach()) == sel["l0"] and int(n_sat) == int(sel["saturated"].sum())
    assert not any(t.requires_grad for t in (io, ln, reach, n_sat)) and kept.requires_grad and l0.requires_grad
    # the raw filter: the slot map and accumulating counters
    c_l0, c_sat = torch.full((), 5, dtype=torch.int64), torch.full((), 7, dtype=torch.int32)
    out = ops.jump_filter(torch.from_numpy(vals), i_t, torch.from_numpy(theta), eps, l0=c_l0, n_saturated=c_sat)
    assert np.array_equal(out[4].numpy(), sel["src"]) and int(c_l0) == 5 + sel["l0"] and int(c_sat) == 7 + int(sel["saturated"].sum())
    # the backward: the routing copy exactly, g_theta inside the derived bound
    rng = np.random.default_rng(9)
    g = rng.standard_normal(vals.shape).astype(np.float32)
    s = np.float32(0.375)
    (kept * torch.from_numpy(g)).sum().add(l0 * float(s)).backward()
    g_in, g_theta, abs_sum, n_f = ref.backward(vals, idx, theta, eps, sel, g, s)
    assert np.array_equal(_bits(a.grad), _bits(g_in))
    err = np.abs(th.grad.numpy().astype(np.float64) - g_theta)
    assert (err <= ref.g_theta_bound(n_f, abs_sum)).all() and n_f.max() >= 2 and (n_f == 0).any()
    assert (th.grad.numpy()[n_f == 0] == 0).all() and th.grad[7] == 0
    # the [:, :C] view of a wider list
    wide_v = torch.from_numpy(np.concatenate([vals, np.full((vals.shape[0], 3), 9.0, np.float32)], 1))
    wide_i = torch.from_numpy(np.concatenate([idx, np.zeros((vals.shape[0], 3), np.int64)], 1))
    k2 = ops.jump_select(wide_v[:, :vals.shape[1]], wide_i[:, :vals.shape[1]], torch.from_numpy(theta), eps)
    assert np.array_equal(_bits(k2[0]), _bits(sel["vals"])) and np.array_equal(k2[2].numpy(), sel["len"])


def test_host_path_edges_of_the_band():
    """a exactly at theta_f (a tie: kept and in the band), at theta_f + h and theta_f - h (outside: the comparisons are strict)"""
    from msae import ops

    eps = 0.25
    theta = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    vals = np.array([[1.125, 1.0, np.nextafter(np.float32(1.125), np.float32(0)), np.nextafter(np.float32(0.875), np.float32(2)),
                      0.875, 0.5]], np.float32)
    idx = np.arange(6, dtype=np.int64)[None]
    sel = ref.select(vals, idx, theta, eps)
    assert sel["kept"].tolist() == [[True, True, True, False, False, False]]
    assert sel["near"].tolist() == [[False, False, False, True, False, False]]
    assert sel["band"].tolist() == [[False, True, True, True, False, False]]
    out = ops.jump_select(torch.from_numpy(vals), torch.from_numpy(idx), torch.from_numpy(theta), eps)
    assert int(out[2]) == 3 and int(out[3]) == 4 and np.array_equal(out[1].numpy(), sel["idx"])
    with pytest.raises(ValueError):
        ops.jump_select(torch.zeros(2, 257), torch.zeros(2, 257, dtype=torch.int64), torch.ones(300), eps)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.jump_select(torch.from_numpy(vals), torch.from_numpy(idx), torch.from_numpy(theta), bad)


# ---- equality with the dense definition, in float64 ----------------------------------------------------------------------------
T_, D_, N_, EPS_ = 37, 16, 96, 0.25


def _dense_setup(seed=4):                                     # (a seed whose top-32 lists saturate no row: asserted below)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T_, D_, generator=g, dtype=F64)
    W = torch.randn(N_, D_, generator=g, dtype=F64)
    W = W / W.norm(dim=1, keepdim=True)
    P = dict(We=W.clone(), be=0.05 * torch.randn(N_, generator=g, dtype=F64), Wd=W.clone(),
             bd=0.1 * torch.randn(D_, generator=g, dtype=F64), th=0.9 + 0.6 * torch.rand(N_, generator=g, dtype=F64))
    return x, {n: p.requires_grad_() for n, p in P.items()}


def _loss(sae_out, x, l0, alpha=0.03):
    return (sae_out - x).pow(2).sum() / (x - x.mean(0)).pow(2).sum() + alpha * l0 / x.shape[0]


def _dense_run(x, P):
    pre = torch.relu((x - P["bd"]) @ P["We"].T + P["be"])
    z, l0 = ref.DenseJump.apply(pre, P["th"], EPS_)
    out = z @ P["Wd"] + P["bd"]
    grads = torch.autograd.grad(_loss(out, x, l0), list(P.values()))
    return out.detach(), l0.detach(), grads, pre.detach()


def _list_run(x, P, C):
    from msae import ops

    pre = torch.relu((x - P["bd"]) @ P["We"].T + P["be"])
    acts, idx = pre.topk(C, dim=1, sorted=True)
    kept, io, ln, reach, l0, n_sat = ops.jump_select(acts, idx, P["th"], EPS_)
    live = torch.arange(C) < reach[:, None]                                         # the decode reads kept + near
    out = (torch.where(live, kept, torch.zeros((), dtype=F64))[..., None] * P["Wd"][io]).sum(1) + P["bd"]
    grads = torch.autograd.grad(_loss(out, x, l0), list(P.values()))
    return out.detach(), l0.detach(), grads, int(n_sat)


def test_lists_equal_the_dense_definition_when_no_row_saturates():
    x, P = _dense_setup()
    out_d, l0_d, grads_d, pre = _dense_run(x, P)
    # the restatement alone says so: no row of the top-32 lists reaches min(theta) - h
    vals, idx = pre.topk(32, dim=1, sorted=True)
    sel = ref.select(vals.numpy(), idx.numpy(), P["th"].detach().numpy(), EPS_)
    assert int(sel["saturated"].sum()) == 0 and sel["band"].sum() > 20
    out_l, l0_l, grads_l, n_sat = _list_run(x, P, 32)
    assert n_sat == 0 and float(l0_l) == float(l0_d) == sel["l0"]
    assert float((out_l - out_d).abs().max()) <= 1e-12
    for name, a, b in zip(P, grads_l, grads_d):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    assert float(grads_d[-1].abs().max()) > 0


def test_saturated_rows_are_counted_when_the_cap_is_too_small():
    x, P = _dense_setup()
    _, _, _, pre = _dense_run(x, P)
    vals, idx = pre.topk(13, dim=1, sorted=True)
    sel = ref.select(vals.numpy(), idx.numpy(), P["th"].detach().numpy(), EPS_)
    _, _, _, n_sat = _list_run(x, P, 13)
    assert n_sat == int(sel["saturated"].sum()) > 0


# ---- three training steps against a literal float64 loop --------------------------------------------------------------------------
def _jump_forward64(sae, x, dead_mask):
    """Sae.forward's "jump" branch in dense torch ops, in the parameters' dtype (ops.jump_select's host path does the rest)"""
    from msae import ops
    from msae.sae.sae import JumpForwardOutput

    pre = torch.relu((x - sae.b_dec) @ sae.encoder.weight.T + sae.encoder.bias)
    acts, idx = pre.topk(sae.cfg.cap, dim=1, sorted=True)
    kept, io, ln, reach, l0, n_sat = ops.jump_select(acts, idx, sae.log_threshold.exp(), sae.cfg.jump_bandwidth)
    out = (kept[..., None] * sae.W_dec[io]).sum(1) + sae.b_dec
    tv = (x - x.mean(0)).pow(2).sum()
    e = out - x
    aux = out.new_zeros(())
    if dead_mask is not None and (nd := int(dead_mask.sum())) > 0:
        k_aux = x.shape[-1] // 2
        scale = min(nd / k_aux, 1.0)
        av, ai = torch.where(dead_mask[None], pre, -torch.inf).topk(min(k_aux, nd), sorted=False)
        aux = scale * ((av[..., None] * sae.W_dec[ai]).sum(1) + sae.b_dec - e).pow(2).sum() / tv
    return JumpForwardOutput(out, kept, io, e.pow(2).sum() / tv, aux, out.new_zeros(()), lengths=ln, reach=reach,
                             l0=l0 / x.shape[0], n_saturated=n_sat)


HYP = dict(lr=3e-3, auxk_alpha=1 / 32, dead_feature_threshold=60, micro_acc_steps=2, l0_alpha=0.02, l0_warmup_steps=2)
EPS_NORM = float(torch.finfo(F64).eps)                     # sae.py:252: the eps of the dtype the decoder is held in


def _train_setup():
    import synth
    from msae import Sae, SaeConfig

    d, N, k = 16, 96, 4
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(d, N, seed=51)
    sae = Sae(d, SaeConfig(num_latents=N, k=k, activation="jump", batch_cap=32, jump_init=1.5, jump_bandwidth=0.25))
    with torch.no_grad():
        for p, a in ((sae.encoder.weight, W_enc), (sae.encoder.bias, b_enc), (sae.W_dec, W_dec), (sae.b_dec, b_dec)):
            p.copy_(torch.from_numpy(a))
        sae.log_threshold.add_(torch.linspace(-0.3, 0.3, N))
    xs = [torch.from_numpy(synth.activations(37, d, seed=70 + s, bf16=False, n_outlier=0)).to(F64) for s in range(3)]
    return sae, xs


def _literal_loop(sae0, xs):
    """the trainer's loop on float64 leaves with a literal dense JumpReLU: autograd, torch.optim.Adam, clip_grad_norm_"""
    names = ("encoder.weight", "encoder.bias", "W_dec", "b_dec", "log_threshold")
    P = {n: torch.nn.Parameter(dict(sae0.named_parameters())[n].detach().to(F64).clone()) for n in names}
    We, be, Wd, bd, lt = P.values()
    opt = torch.optim.Adam(list(P.values()), lr=HYP["lr"], betas=(0.9, 0.999), eps=1e-8)
    N = We.shape[0]
    counts, did_fire = torch.zeros(N, dtype=torch.long), torch.zeros(N, dtype=torch.bool)
    eps = sae0.cfg.jump_bandwidth
    log = []
    for t, x in enumerate(xs):
        with torch.no_grad():
            Wd.data /= torch.norm(Wd.data, dim=1, keepdim=True) + EPS_NORM
        dead_mask = counts > HYP["dead_feature_threshold"]
        chunks = x.chunk(HYP["micro_acc_steps"])
        weight = HYP["l0_alpha"] * min(1.0, t / HYP["l0_warmup_steps"])
        stats = dict(fvu=0.0, aux=0.0, l0=0.0, dead=int(dead_mask.sum()))
        for chunk in chunks:
            pre = torch.relu((chunk - bd) @ We.T + be)
            z, n_kept = ref.DenseJump.apply(pre, lt.exp(), eps)
            out = z @ Wd + bd
            tv = (chunk - chunk.mean(0)).pow(2).sum()
            e = out - chunk
            fvu = e.pow(2).sum() / tv
            aux = out.new_zeros(())
            if (nd := int(dead_mask.sum())) > 0:
                k_aux = chunk.shape[-1] // 2
                scale = min(nd / k_aux, 1.0)
                av, ai = torch.where(dead_mask[None], pre, -torch.inf).topk(min(k_aux, nd), sorted=False)
                aux = scale * ((av[..., None] * Wd[ai]).sum(1) + bd - e).pow(2).sum() / tv
            l0 = n_kept / chunk.shape[0]
            (fvu + HYP["auxk_alpha"] * aux + weight * l0).div(len(chunks)).backward()
            did_fire |= (z.detach() > 0).any(0)
            for n, v in (("fvu", fvu), ("aux", aux), ("l0", l0)):
                stats[n] += float(v.detach()) / len(chunks)
        torch.nn.utils.clip_grad_norm_(list(P.values()), 1.0)
        with torch.no_grad():
            Wd.grad -= (Wd.grad * Wd.data).sum(1, keepdim=True) * Wd.data
        stats["g_lt"] = lt.grad.detach().clone()
        opt.step()
        opt.zero_grad()
        counts += x.shape[0]
        counts[did_fire] = 0
        did_fire.zero_()
        log.append((stats, counts.clone()))
    return {n: p.detach() for n, p in P.items()}, log


def test_three_training_steps_equal_a_literal_float64_loop():
    from msae.train import SaeTrainStep

    sae, xs = _train_setup()
    want, log = _literal_loop(sae, xs)

    class CpuTrainStep(SaeTrainStep):
        def _forward(self, hiddens, dead_mask):
            out = _jump_forward64(self.sae, hiddens, dead_mask)
            assert int(out.n_saturated) == 0                   # the lists are the dense definition (the test above)
            return out

        def _update(self, lr):
            torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
            self.sae.remove_gradient_parallel_to_decoder_directions()
            self.seen_g = self.sae.log_threshold.grad.detach().clone()
            b1, b2 = self.betas
            with torch.no_grad():
                for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq):
                    m.mul_(b1).add_(p.grad, alpha=1 - b1)
                    v.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                    p.addcdiv_(m / (1 - b1 ** self.t), (v / (1 - b2 ** self.t)).sqrt() + self.eps, value=-lr)
                    p.grad = None

    ts = CpuTrainStep(sae, **HYP)
    assert any(p is sae.log_threshold for p in ts.params)
    sae.double()                                               # the same Parameter objects, now float64 leaves
    ts.exp_avg, ts.exp_avg_sq = [m.double() for m in ts.exp_avg], [v.double() for v in ts.exp_avg_sq]
    assert ts.current_l0_weight == 0.0
    for t, (x, (stats, counts)) in enumerate(zip(xs, log)):
        res = ts.step(x)
        assert res["stepped"] and int(res["n_saturated"]) == 0
        # step() keeps fvu and auxk_loss in a float32 vector whatever the model's dtype: each chunk's value rounded on the way
        # in, one addition, one division -- at most 4 roundings of 2^-24 each; everything else stays float64
        for key, name, tol in (("fvu", "fvu", 4 * 2.0 ** -24), ("auxk_loss", "aux", 4 * 2.0 ** -24), ("l0", "l0", 1e-12)):
            assert abs(float(res[key]) - stats[name]) <= tol * abs(stats[name]), (t, key, float(res[key]), stats[name])
        assert float((ts.seen_g - stats["g_lt"]).abs().max()) <= 1e-12 * float(stats["g_lt"].abs().max()), t
        assert torch.equal(ts.num_tokens_since_fired, counts), t
    assert log[0][0]["dead"] == 0 and log[2][0]["dead"] > 0 and log[2][0]["aux"] > 0, "the AuxK term must run with a dead mask"
    assert ts.current_l0_weight == HYP["l0_alpha"] and float(log[2][0]["g_lt"].abs().max()) > 0
    for n, p in sae.named_parameters():
        err = float((p.detach() - want[n]).abs().max())
        assert err <= 1e-12 * float(want[n].abs().max()), (n, err)
    assert not torch.equal(want["log_threshold"], _train_setup()[0].log_threshold.detach().double())


def test_sae_forward_on_the_host_with_a_dense_encoder(monkeypatch):
    """Sae.forward's own "jump" branch (jump_select, the reach decode, the mean l0) with the HIP encoder and the AuxK decode
    replaced by dense torch ops: float32 against the float64 composition above, selections exactly."""
    from msae import ops
    from msae.sae import utils as seam

    sae, xs = _train_setup()
    x = xs[0].float()
    dead = torch.zeros(96, dtype=torch.bool)
    dead[::7] = True

    def sparse_encode(x, W_enc, b_enc, b_dec, k, dead_mask=None, k_aux=0, k_multi=0, **kw):
        pre = torch.relu((x - b_dec) @ W_enc.T + b_enc)
        out = [pre.topk(k, dim=1, sorted=True)]
        if k_aux:
            out.append(torch.where(dead_mask[None], pre, -torch.inf).topk(k_aux, sorted=False))
        return [(v, i) for v, i in out]

    monkeypatch.setattr(ops, "sparse_encode", sparse_encode)
    monkeypatch.setattr(seam, "decoder_impl", lambda idx, acts, W_T: (acts[..., None] * W_T.mT[idx]).sum(-2))
    out = sae(x, dead)
    sae64, _ = _train_setup()
    sae64.double()
    want = _jump_forward64(sae64, xs[0], dead)
    assert type(out).__name__ == "JumpForwardOutput" and out.latent_acts.shape == (37, 32)
    assert torch.equal(out.lengths, want.lengths) and torch.equal(out.reach, want.reach)
    assert torch.equal(out.latent_indices, want.latent_indices) and int(out.n_saturated) == 0
    assert float(out.l0.detach()) == float(np.float32(int(want.lengths.sum())) / np.float32(37)) and bool((out.reach > out.lengths).any())
    # float32 against float64: an encoder dot product of 16 terms, a decode chain of at most 32, a sum of 37 * 16 squares
    tol = float(ref.gamma(16 + 32 + 37 * 16 + 8))
    for name in ("fvu", "auxk_loss", "sae_out"):
        a, b = getattr(out, name).double(), getattr(want, name)
        assert float((a.detach() - b.detach()).abs().max()) <= tol * float(b.detach().abs().max()), name
    (out.fvu + out.l0).backward()
    assert float(sae.log_threshold.grad.abs().max()) > 0 and sae.W_dec.grad is not None


# ---- exact zero ----------------------------------------------------------------------------------------------------------------
def test_nothing_in_the_band_leaves_the_thresholds_bit_unchanged():
    from msae.train import SaeTrainStep

    sae, xs = _train_setup()
    sae.cfg.jump_bandwidth = 1e-30                             # no entry lies within 5e-31 of its threshold
    before = sae.log_threshold.detach().clone()
    seen = {}

    class CpuTrainStep(SaeTrainStep):
        def _forward(self, hiddens, dead_mask):
            return _jump_forward64(self.sae, hiddens, dead_mask)

        def _update(self, lr):
            seen["grad"] = self.sae.log_threshold.grad.detach().clone()
            b1, b2 = self.betas
            with torch.no_grad():
                for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq):
                    m.mul_(b1).add_(p.grad, alpha=1 - b1)
                    v.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                    p.addcdiv_(m / (1 - b1 ** self.t), (v / (1 - b2 ** self.t)).sqrt() + self.eps, value=-lr)
                    p.grad = None

    ts = CpuTrainStep(sae, lr=1e-2, l0_alpha=0.5)
    res = ts.step(xs[0].float())
    assert float(res["l0"]) > 0 and seen["grad"].dtype == torch.float32
    assert torch.equal(seen["grad"], torch.zeros_like(seen["grad"]))                # exactly zero, every feature
    assert np.array_equal(_bits(sae.log_threshold.detach()), _bits(before))
    assert not torch.equal(sae.encoder.bias.detach(), torch.zeros(96))              # (the step moved the rest)
