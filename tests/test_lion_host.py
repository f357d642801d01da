"""CPU: the sign-momentum entry point is exported under the unchanged ABI version and rejects bad arguments before it touches a
device, and SaeTrainStep's `optimizer` / `betas` arguments, its state and its checkpoints behave as msae/train.py documents."""
import pytest
import torch

EINVAL = -1


def _ts(optimizer="adam", **kw):
    from msae import Sae, SaeConfig
    from msae.train import SaeTrainStep

    sae = Sae(16, SaeConfig(num_latents=64, k=4))
    return SaeTrainStep(sae, optimizer=optimizer, **kw)


def test_symbol_is_exported_and_the_abi_version_stays():
    from msae import _hip

    lib = _hip.load()
    assert hasattr(lib, "msae_lion_rows_f32") and "msae_lion_rows_f32" in _hip.PROTOTYPES
    assert lib.msae_abi_version() == 4 == _hip.ABI_VERSION


def test_argument_errors_come_before_any_device_work():
    from msae import _hip

    f = _hip.load().msae_lion_rows_f32
    p = 4096                                        # never dereferenced: every call below fails its argument check

    def call(W=p, G=p, M=p, rows=4, d=8):
        return f(W, G, M, rows, d, None, 1.0, 0, 1e-3, 0.9, 0.99, -1.0, None, 0, None, None)

    for bad in (dict(W=None), dict(G=None), dict(M=None), dict(rows=0), dict(rows=-3), dict(d=0), dict(d=-8)):
        assert call(**bad) == EINVAL, bad


def test_optimizer_argument_checks():
    with pytest.raises(ValueError, match="optimizer"):
        _ts("x", lr=1e-3)
    for name in ("lion", "signum"):
        with pytest.raises(ValueError, match="lr"):
            _ts(name)
        with pytest.raises(ValueError, match="8-bit momentum"):
            _ts(name, lr=1e-3, optim_bits=8)
    with pytest.raises(ValueError, match="beta1 == beta2"):
        _ts("signum", lr=1e-3, betas=(0.9, 0.99))
    assert _ts().betas == (0.9, 0.999) and _ts("lion", lr=1e-3).betas == (0.9, 0.99)
    assert _ts("signum", lr=1e-3).betas == (0.9, 0.9) and _ts("signum", lr=1e-3, betas=(0.95, 0.95)).betas == (0.95, 0.95)
    assert _ts("lion", lr=1e-3, betas=(0.95, 0.98)).betas == (0.95, 0.98) and _ts(betas=(0.8, 0.95)).betas == (0.8, 0.95)


def test_state_and_state_dict_keys():
    adam = _ts()
    assert set(adam.state_dict()) == {"step", "global_step", "exp_avg", "exp_avg_sq", "num_tokens_since_fired"}
    assert all(v is not None for v in adam.exp_avg_sq)
    numel = sum(p.numel() for p in adam.params)
    assert adam.optimizer_state_bytes == 8 * numel
    for name, betas in (("lion", (0.9, 0.99)), ("signum", (0.9, 0.9))):
        ts = _ts(name, lr=1e-3)
        sd = ts.state_dict()
        assert set(sd) == {"step", "global_step", "exp_avg", "exp_avg_sq", "num_tokens_since_fired", "optimizer", "betas"}
        assert sd["optimizer"] == name and tuple(sd["betas"]) == betas
        assert all(v is None for v in ts.exp_avg_sq) and all(s8 is None for s8 in ts.state8)
        assert all(m is not None and not bool(m.any()) for m in ts.exp_avg)
        assert ts.optimizer_state_bytes == 4 * numel


def test_loading_across_optimisers_is_refused():
    adam, lion, signum = _ts(), _ts("lion", lr=1e-3), _ts("signum", lr=1e-3)
    for dst, src in ((adam, lion), (lion, adam), (lion, signum), (signum, lion)):
        with pytest.raises(ValueError) as e:
            dst.load_state_dict(src.state_dict())
        assert repr(dst.optimizer) in str(e.value) and repr(src.optimizer) in str(e.value)
    sd = lion.state_dict()
    sd["step"] = 7
    sd["exp_avg"] = [torch.full_like(m, 0.5) for m in lion.exp_avg]
    other = _ts("lion", lr=1e-3)
    other.load_state_dict(sd)
    assert other.t == 7 and all(bool((m == 0.5).all()) for m in other.exp_avg) and all(v is None for v in other.exp_avg_sq)
    adam2 = _ts()
    adam2.load_state_dict(adam.state_dict())         # an Adam checkpoint loads as it always did
