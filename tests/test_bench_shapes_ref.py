"""The checker of tests/test_gpu_bench_shapes.py has teeth (no GPU needed).

tests/bench_shapes_ref.py is run on a small SAE with the C oracle's answer standing in for the kernels' output: levels A, B
and C must accept it, and must reject each way a subtly wrong kernel would show -- a top-k member replaced by the (k + 1)-th
feature, a value moved by more than its bound, two slots swapped, a duplicated index, one reconstruction element moved beyond
its bound, one flipped mantissa bit.  "Would fail if the kernel were wrong" is shown here, not by breaking a kernel on a GPU.
"""
import numpy as np
import pytest
import torch

import bench_shapes_ref as ref
import synth
from oracle import oracle

D, N, T, K = 256, 4096, 64, 8


@pytest.fixture(scope="module")
def case():
    W_enc, b_enc, W_dec, b_dec = synth.sae_weights(D, N, seed=31)
    x = torch.from_numpy(synth.activations(T, D, seed=32)).to(torch.bfloat16)
    xf = x.float().numpy()
    v, i = oracle.encode_topk(xf, W_enc, b_enc, b_dec, K)
    r = oracle.decode(i, v, W_dec, b_dec)
    f64 = ref.F64Reference(*(torch.from_numpy(a) for a in (W_enc, b_enc, b_dec, W_dec)), chunk_bytes=24 * N * 8)
    out = {"top_acts": torch.from_numpy(v), "top_indices": torch.from_numpy(i.astype(np.int64)), "sae_out": torch.from_numpy(r),
           "status": torch.zeros(T, dtype=torch.int32)}
    return {"host": (W_enc, b_enc, W_dec, b_dec), "x": x, "out": out, "f64": f64}


def _edited(out, **kw):
    new = {k: v.clone() for k, v in out.items()}
    new.update(kw)
    return new


def test_all_levels_accept_the_oracle_answer(case):
    out, f64, x = case["out"], case["f64"], case["x"]
    st = f64.check_encode(x, out["top_acts"], out["top_indices"], "oracle")
    assert 0.0 < st["max_ratio"] < 1.0            # several token chunks (24 tokens each), every value well inside its bound
    assert st["wide_gap"] > 0 and st["wide_gap_matched"] == st["wide_gap"]
    rd = f64.check_decode(out["top_acts"], out["top_indices"], out["sae_out"], "oracle")
    assert 0.0 < rd["max_ratio_recon"] < 1.0
    hist = ref.level_a(out, _edited(out), "oracle")
    assert hist == {"verified": T, "fallback": 0, "unresolved": 0, "wrong": 0}
    rows = ref.sample_rows(T, out["status"].numpy())
    assert ref.level_c(oracle, case["host"], x, out, rows, K) == len(rows)


def _widest_gap_token(case):
    """(token, the f64 (k + 1)-th feature, its f32 value as the oracle computes it): the token whose f64 gap between the k-th
    and the (k + 1)-th value is the largest multiple of the bound."""
    f64, x = case["f64"], case["x"]
    P, B = f64.pre_acts(x)
    top = torch.topk(P, K + 1, dim=1)
    gap = top.values[:, K - 1] - top.values[:, K]
    b2 = torch.maximum(B.gather(1, top.indices[:, K - 1:K]), B.gather(1, top.indices[:, K:K + 1])).squeeze(1)
    t = int((gap / b2).argmax())
    # v' <= P' + B', so P_k - v' > gap - B >= 2 B >= B(n_k) + B(n'): the check MUST reject the swap on this token
    assert float(gap[t]) > 3.0 * float(b2[t]), "construction: the sample needs a token whose gap exceeds 2 B with room"
    n_next = int(top.indices[t, K])
    W_enc, b_enc, _, b_dec = case["host"]
    pre = oracle.pre_acts(x[t:t + 1].float().numpy(), W_enc, b_enc, b_dec)
    return t, n_next, float(pre[0, n_next])


def test_level_b_rejects_a_member_replaced_by_the_next_feature(case):
    out, f64, x = case["out"], case["f64"], case["x"]
    t, n_next, v_next = _widest_gap_token(case)
    v, i = out["top_acts"].clone(), out["top_indices"].clone()
    assert n_next not in i[t].tolist() and v_next <= float(v[t, -1])
    i[t, -1], v[t, -1] = n_next, v_next          # a well-formed list with the right value for its feature: only a member is missing
    with pytest.raises(AssertionError, match="not returned"):
        f64.check_encode(x, v, i, "swap")
    wrong = _edited(out, top_acts=v, top_indices=i)
    with pytest.raises(AssertionError, match="VERIFIED tokens differ"):
        ref.level_a(wrong, out, "swap")
    with pytest.raises(AssertionError, match="indices differ from the C oracle"):
        ref.level_c(oracle, case["host"], x, wrong, np.array([t]), K)


def test_level_b_rejects_a_value_moved_by_more_than_its_bound(case):
    out, f64, x = case["out"], case["f64"], case["x"]
    _, B = f64.pre_acts(x)
    t, j = 17, 3
    bound = float(B[t, int(out["top_indices"][t, j])])
    gap_up = float(out["top_acts"][t, j - 1] - out["top_acts"][t, j])
    gap_dn = float(out["top_acts"][t, j] - out["top_acts"][t, j + 1])
    v = out["top_acts"].clone()
    # 2.5 B: outside the bound whatever the f32 value's own error (at most B), and the order of the list stays intact
    step = 2.5 * bound
    assert step < max(gap_up, gap_dn), "construction: the moved value must not cross a neighbour"
    v[t, j] += step if step < gap_up else -step
    with pytest.raises(AssertionError, match="further than B"):
        f64.check_encode(x, v, out["top_indices"], "moved")
    # ... and half a bound is accepted: the rejection above is the bound's, not any difference's
    v2 = out["top_acts"].clone()
    v2[t, j] += (0.25 * bound) if 0.25 * bound < gap_up else -(0.25 * bound)
    f64.check_encode(x, v2, out["top_indices"], "moved a little")


def test_level_b_rejects_swapped_slots_and_duplicates(case):
    out, f64, x = case["out"], case["f64"], case["x"]
    v, i = out["top_acts"].clone(), out["top_indices"].clone()
    v[5, [2, 3]], i[5, [2, 3]] = v[5, [3, 2]], i[5, [3, 2]]
    with pytest.raises(AssertionError, match="descending"):
        f64.check_encode(x, v, i, "swapped")
    i = out["top_indices"].clone()
    i[9, 4] = i[9, 1]
    with pytest.raises(AssertionError, match="not distinct"):
        f64.check_encode(x, out["top_acts"], i, "duplicate")
    i = out["top_indices"].clone()
    i[9, 4] = N
    with pytest.raises(AssertionError, match="out of range"):
        f64.check_encode(x, out["top_acts"], i, "range")
    # equal values must come in ascending index order
    v, i = out["top_acts"].clone(), out["top_indices"].clone()
    v[11, 1] = v[11, 0]
    i[11, [0, 1]] = i[11, [0, 1]].sort(descending=True).values
    with pytest.raises(AssertionError, match="tie"):
        ref.F64Reference.check_structure(v, i, N, "tie")


def test_level_b_rejects_a_reconstruction_element_beyond_its_bound(case):
    out, f64 = case["out"], case["f64"]
    v, i, r = out["top_acts"], out["top_indices"], out["sae_out"].clone()
    t, c = 40, 123
    bound = ref.gamma(K + 1) * float(f64.b_dec[c].abs().double() + (v[t].double() * f64.W_dec[i[t], c].double()).abs().sum())
    r[t, c] += 2.5 * bound
    with pytest.raises(AssertionError, match="reconstruction elements lie outside"):
        f64.check_decode(v, i, r, "recon")
    r = out["sae_out"].clone()
    r[t, c] = float("nan")
    with pytest.raises(AssertionError, match="reconstruction elements lie outside"):
        f64.check_decode(v, i, r, "recon nan")


@pytest.mark.parametrize("field", ["top_acts", "sae_out"])
def test_level_a_flags_one_flipped_mantissa_bit(case, field):
    out = case["out"]
    flipped = out[field].clone()
    flipped.view(torch.int32)[33, 5] ^= 1
    mism = ref.token_bit_mismatch(flipped, out[field], zero_exempt=(field == "top_acts"))
    assert mism.nonzero().flatten().tolist() == [33]
    with pytest.raises(AssertionError, match="VERIFIED tokens differ"):
        ref.level_a(_edited(out, **{field: flipped}), out, "bit")
    assert not ref.same_bits(_edited(out, **{field: flipped}), out) and ref.same_bits(_edited(out), out)
    with pytest.raises(AssertionError, match="differ"):
        ref.level_c(oracle, case["host"], case["x"], _edited(out, **{field: flipped}), np.array([32, 33]), K)


def test_level_a_status_rules(case):
    """Only +0 against -0 among the values is exempt; a wrong fallback token is wrong all the same (but not "verified and
    wrong"); status codes >= 2 and a fallback share above the cap fail."""
    out = case["out"]
    z = _edited(out)
    z["top_acts"][3, -1] = 0.0
    nz = _edited(z)
    nz["top_acts"][3, -1] = -0.0
    assert not ref.token_bit_mismatch(nz["top_acts"], z["top_acts"], zero_exempt=True).any()
    assert ref.token_bit_mismatch(nz["top_acts"], z["top_acts"]).tolist().count(True) == 1
    st = out["status"].clone()
    st[7] = 1
    flipped = out["top_acts"].clone()
    flipped.view(torch.int32)[7, 0] ^= 1
    with pytest.raises(AssertionError, match="values differ on 1 tokens"):
        ref.level_a(_edited(out, top_acts=flipped, status=st), out, "fallback token")
    st = out["status"].clone()
    st[7] = 2 | (64 << 8)
    with pytest.raises(AssertionError, match="status code >= 2"):
        ref.level_a(_edited(out, status=st), out, "unresolved")
    st = out["status"].clone()
    st[:2] = 1                                   # 2 of 64 = 0.031 > 0.03
    with pytest.raises(AssertionError, match="exact-fallback share"):
        ref.level_a(_edited(out, status=st), out, "cap")
    assert ref.level_a(_edited(out, status=st), out, "certified cap", max_fallback=1.0)["fallback"] == 2


def test_sample_rows_hold_the_named_rows():
    for T_ in (8192, 2880, 65536):
        status = np.zeros(T_, dtype=np.int32)
        fb = np.arange(100, T_, 97)[:50]
        status[fb] = 1 | (4 << 8)
        rows = ref.sample_rows(T_, status, seed=0)
        want = {0, 255, 256, 257, T_ - 1} | {b + o for b in range(2048, T_, 2048) for o in (-1, 0)}
        assert want <= set(rows.tolist())
        assert len(set(rows.tolist())) == len(rows) and rows.min() >= 0 and rows.max() < T_
        plain = ref.sample_rows(T_, None, seed=0)
        assert len(plain) == max(64, len(want) + 16) and set(plain.tolist()) <= set(rows.tolist())
        extra = set(rows.tolist()) - set(plain.tolist())
        assert len(extra) == min(32, len(set(fb.tolist()) - set(plain.tolist()))) and extra <= set(fb.tolist())
        assert np.array_equal(rows, ref.sample_rows(T_, status, seed=0))          # a fixed seed: the same sample every run


def test_tiles_per_workgroup_of_the_bench_shapes():
    """256 CUs: 32 x 496 main tiles and 32 x 16 sample tiles at T = 8192, N = 131072 -> 62 and 2 per workgroup."""
    assert ref.tiles_per_workgroup(8192, 131072, 256) == (62, 2)
    assert ref.tiles_per_workgroup(2880, 131072, 256) == (24, 1)          # 12 x 496 = 5952 tiles: 23.25 -> 24; 192 sample tiles
    assert ref.tiles_per_workgroup(65536, 131072, 256) == (496, 16)
    assert ref.tiles_per_workgroup(8192, 131072, 256, "fp8") == (64, 2)
    assert ref.tiles_per_workgroup(8192, 262144, 256) == (124, 4)         # the shape that showed the round-6 LDS race
