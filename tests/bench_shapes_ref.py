"""Three reference levels for every-token checks of encode -> TopK -> decode at the benchmark's shapes
(tests/test_gpu_bench_shapes.py; the checker's own teeth are shown on the CPU by tests/test_bench_shapes_ref.py).

A.  `exact_path` + `level_a`: every token, bit for bit, against the exact HIP path (ops.pre_acts -> ops.topk -> ops.decode in
    chunks -- the idea of test_gpu_hostile._exact / _compare, extended by the reconstruction).  Values, indices and
    reconstruction are compared as int32 bit patterns; the one exemption is _compare's: +0 against -0 among the values.

B.  `F64Reference`: every token against float64 computed with plain torch -- no kernel of this project.  The operation is
        a32 = x.float() - b_dec          (an f32 elementwise subtraction: part of the specification)
        P   = a32.double() @ W.double().T + b.double()          then the ReLU
    and an f32 evaluation of it, in ANY summation order, with or without fused multiply-adds, differs from P by at most
        B(t, n) = gamma_{d+1} (sum_i |a32_i W_ni| + |b_n|),   gamma_m = m u / (1 - m u),  u = 2^-24
    (d products and d additions of which the bias is one more: Higham, Accuracy and Stability of Numerical Algorithms, section
    3.1).  The sum comes from a second f64 GEMM on absolute values -- this file uses that form, not the looser |a| |W_n|.  The
    ReLU is 1-Lipschitz, so the bound carries to relu(P).  The error of the f64 GEMMs themselves is nine orders below B.
    Asserted for EVERY token, no exclusions:
      * indices in range and distinct, values descending, ties ordered by ascending index;
      * |v - relu(P)[t, idx]| <= B(t, idx) for each returned value;
      * relu(P)[t, n] <= v_k + B(t, n) + B(t, idx_k) for every feature n not returned.
    Set equality with the f64 top-k is NOT asserted (B is of the order of the gap between the k-th and the (k + 1)-th value at
    width 131072; levels A and C carry it); how many tokens have a gap above 2 B and match the f64 set is counted, as information.
    Reconstruction: R = b_dec + sum_j v_j W_dec[i_j].double() from the RETURNED (v, i); every element within
        gamma_{k+1} (|b_dec_c| + sum_j |v_j W_dec[i_j, c]|).

C.  `sample_rows` + `level_c`: a token sample against the C oracle on the CPU (oracle.encode_topk, oracle.decode), bit for bit.
    The sample holds rows 0, 255, 256, 257, T - 1, the rows on either side of every multiple of 2048 inside the call (those of
    8192 are among them), seeded random rows up to 64 in all (at least 16 random ones: a 65536-token call has 62 boundary
    rows), and up to 32 tokens of status 1 -- the in-call exact fallback's outputs, which level A compares with the same
    kernel family.

`tiles_per_workgroup` restates the candidate GEMM's launch for the coverage line of each case.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of f32


def gamma(m: int) -> float:
    return m * U / (1.0 - m * U)


# ---- level A --------------------------------------------------------------------------------------------------------------
def exact_path(ops, x, W_enc, b_enc, b_dec, W_dec, k, chunk=2048):
    """The exact HIP path on every token, in chunks of `chunk` tokens (a [chunk, N] f32 pre-activation at a time)."""
    vs, ids, rs = [], [], []
    for t0 in range(0, x.shape[0], chunk):
        pre = ops.pre_acts(x[t0:t0 + chunk], W_enc, b_enc, b_dec)
        v, i = ops.topk(pre, k)
        del pre
        vs.append(v); ids.append(i); rs.append(ops.decode(i, v, W_dec, b_dec))
    return {"top_acts": torch.cat(vs), "top_indices": torch.cat(ids), "sae_out": torch.cat(rs)}


def token_bit_mismatch(got: torch.Tensor, ref: torch.Tensor, zero_exempt: bool = False) -> torch.Tensor:
    """[T] bool: the token's row of f32 `got` differs from `ref` in some int32 bit pattern (NaN == NaN by its bits).
    zero_exempt: an element that is zero on both sides counts as equal whatever its sign (_compare's exemption)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == torch.float32, (got.shape, ref.shape, got.dtype, ref.dtype)
    diff = got.contiguous().view(torch.int32) != ref.contiguous().view(torch.int32)
    if zero_exempt:
        diff &= ~((got == 0) & (ref == 0))
    return diff.flatten(1).any(dim=1)


def level_a(out: dict, exact: dict, what: str, max_fallback: float = 0.03) -> dict:
    """out / exact: {"top_acts", "top_indices", "sae_out"} (+ out["status"]).  -> {"verified", "fallback", "unresolved",
    "wrong"} where wrong = VERIFIED tokens that differ from the exact path (the dangerous kind: reported on its own)."""
    T = out["top_acts"].shape[0]
    code = out["status"] & 0xFF
    bad_i = (out["top_indices"] != exact["top_indices"]).any(dim=1)
    bad_v = token_bit_mismatch(out["top_acts"], exact["top_acts"], zero_exempt=True)
    bad_r = token_bit_mismatch(out["sae_out"], exact["sae_out"])
    bad = bad_i | bad_v | bad_r
    hist = {"verified": int((code == 0).sum()), "fallback": int((code == 1).sum()), "unresolved": int((code >= 2).sum()),
            "wrong": int((bad & (code == 0)).sum())}
    first = bad.nonzero().flatten()[:8].tolist()
    assert hist["wrong"] == 0, f"{what}: {hist['wrong']} VERIFIED tokens differ from the exact path (first {first}) {hist}"
    assert hist["unresolved"] == 0, f"{what}: status code >= 2 on {hist['unresolved']} tokens {hist}"
    assert int(bad_i.sum()) == 0, f"{what}: indices differ on {int(bad_i.sum())} tokens (first {first})"
    assert int(bad_v.sum()) == 0, f"{what}: values differ on {int(bad_v.sum())} tokens (first {first})"
    assert int(bad_r.sum()) == 0, f"{what}: reconstruction differs on {int(bad_r.sum())} tokens (first {first})"
    assert hist["fallback"] <= max_fallback * T, f"{what}: exact-fallback share above {max_fallback}: {hist}"
    return hist


def same_bits(a: dict, b: dict) -> bool:
    """Two calls returned the same (values, indices, reconstruction), bit for bit."""
    return bool(torch.equal(a["top_indices"], b["top_indices"])
                and not token_bit_mismatch(a["top_acts"], b["top_acts"]).any()
                and not token_bit_mismatch(a["sae_out"], b["sae_out"]).any())


# ---- level B --------------------------------------------------------------------------------------------------------------
class F64Reference:
    """float64 restatement of one SAE in plain torch (any device).  Holds W_enc.double() and its absolute value (8 N d bytes
    each); tokens go through in chunks whose [chunk, N] f64 pre-activations take about `chunk_bytes`."""

    def __init__(self, W_enc, b_enc, b_dec, W_dec, chunk_bytes: int = 1 << 30):
        self.N, self.d = W_enc.shape
        self.Wt = W_enc.double().t()
        self.Wt_abs = self.Wt.abs()
        self.b_enc, self.b_dec, self.W_dec = b_enc, b_dec, W_dec
        self.chunk_bytes = chunk_bytes

    def with_bias(self, b_enc) -> "F64Reference":
        """The same weights under another encoder bias (shares the f64 copies)."""
        other = object.__new__(F64Reference)
        other.__dict__.update(self.__dict__)
        other.b_enc = b_enc
        return other

    def pre_acts(self, x):
        """-> (relu(P), B) for the tokens of x: [T, N] f64 each."""
        a32 = x.float() - self.b_dec
        P = a32.double() @ self.Wt
        S = a32.abs().double() @ self.Wt_abs
        if self.b_enc is not None:
            P += self.b_enc.double()
            S += self.b_enc.abs().double()
        return P.clamp_(min=0.0), S.mul_(gamma(self.d + 1))

    @staticmethod
    def check_structure(v, i, N, what=""):
        """Every token: indices in range and distinct, values descending, ties by ascending index."""
        assert i.dtype == torch.int64 and v.dtype == torch.float32 and v.shape == i.shape
        assert not bool(torch.isnan(v).any()), f"{what}: NaN among the returned values"
        out_of_range = ((i < 0) | (i >= N)).any(dim=1)
        assert not bool(out_of_range.any()), f"{what}: index out of range on tokens {out_of_range.nonzero().flatten()[:8].tolist()}"
        s = i.sort(dim=1).values
        dup = (s[:, 1:] == s[:, :-1]).any(dim=1)
        assert not bool(dup.any()), f"{what}: indices not distinct on tokens {dup.nonzero().flatten()[:8].tolist()}"
        up = (v[:, :-1] < v[:, 1:]).any(dim=1)
        assert not bool(up.any()), f"{what}: values not in descending order on tokens {up.nonzero().flatten()[:8].tolist()}"
        tie = ((v[:, :-1] == v[:, 1:]) & (i[:, :-1] >= i[:, 1:])).any(dim=1)
        assert not bool(tie.any()), f"{what}: tie not in ascending index order on tokens {tie.nonzero().flatten()[:8].tolist()}"

    def check_encode(self, x, v, i, what="") -> dict:
        """Every token of (v, i) = top-k of x against relu(P) and B.  -> {"max_ratio": largest |v - P| / B, "wide_gap":
        tokens whose f64 gap between the k-th and (k + 1)-th value exceeds 2 B (B = the larger of the two features' bounds),
        "wide_gap_matched": those among them whose index set equals the f64 top-k}."""
        T, k = v.shape
        self.check_structure(v, i, self.N, what)
        chunk = max(1, self.chunk_bytes // (self.N * 8))
        max_ratio, n_val, n_out, wide, matched = 0.0, 0, 0, 0, 0
        first_val, first_out = None, None
        for t0 in range(0, T, chunk):
            P, B = self.pre_acts(x[t0:t0 + chunk])
            vc, ic = v[t0:t0 + chunk].double(), i[t0:t0 + chunk]
            Pv, Bv = P.gather(1, ic), B.gather(1, ic)
            err = (vc - Pv).abs()
            bad = err > Bv
            if bool(bad.any()) and first_val is None:
                t, j = bad.nonzero()[0].tolist()
                first_val = (t0 + t, j, int(ic[t, j]), float(vc[t, j]), float(Pv[t, j]), float(Bv[t, j]))
            n_val += int(bad.sum())
            ratio = torch.where(Bv > 0, err / Bv, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            max_ratio = max(max_ratio, float(ratio.max()))
            # information: the f64 top-(k + 1) and its gap (before P is edited below)
            if k < self.N:
                top = torch.topk(P, k + 1, dim=1)
                gap = top.values[:, k - 1] - top.values[:, k]
                b2 = torch.maximum(B.gather(1, top.indices[:, k - 1:k]), B.gather(1, top.indices[:, k:k + 1])).squeeze(1)
                w = gap > 2.0 * b2
                same = (ic.sort(dim=1).values == top.indices[:, :k].sort(dim=1).values).all(dim=1)
                wide += int(w.sum()); matched += int((w & same).sum())
                del top
            # features not returned: relu(P)[n] - B[n] <= v_k + B[idx_k]
            P.sub_(B).scatter_(1, ic, float("-inf"))
            worst = P.max(dim=1)
            miss = worst.values > vc[:, -1] + Bv[:, -1]
            if bool(miss.any()) and first_out is None:
                t = int(miss.nonzero()[0])
                first_out = (t0 + t, int(worst.indices[t]), float(worst.values[t]), float(vc[t, -1]), float(Bv[t, -1]))
            n_out += int(miss.sum())
            del P, B
        assert n_val == 0, (f"{what}: {n_val} returned values lie further than B from the f64 pre-activation; first (token, slot, "
                            f"feature, v, P, B) = {first_val}")
        assert n_out == 0, (f"{what}: on {n_out} tokens a feature that was not returned exceeds v_k + B(n) + B(idx_k); first (token, "
                            f"feature, P - B(n), v_k, B(idx_k)) = {first_out}")
        return {"max_ratio": max_ratio, "wide_gap": wide, "wide_gap_matched": matched}

    def check_decode(self, v, i, recon, what="") -> dict:
        """Every element of the reconstruction of the RETURNED (v, i) against f64.  -> {"max_ratio_recon"}."""
        T, k = v.shape
        d = self.W_dec.shape[1]
        assert recon.shape == (T, d) and recon.dtype == torch.float32
        g = gamma(k + 1)
        chunk = max(1, self.chunk_bytes // (k * d * 8))
        bd = self.b_dec.double()
        n_bad, first, max_ratio = 0, None, 0.0
        for t0 in range(0, T, chunk):
            prod = self.W_dec[i[t0:t0 + chunk]].double().mul_(v[t0:t0 + chunk].double().unsqueeze(-1))     # [c, k, d]
            R = prod.sum(dim=1).add_(bd)
            bound = prod.abs_().sum(dim=1).add_(bd.abs()).mul_(g)
            del prod
            err = (recon[t0:t0 + chunk].double() - R).abs_()
            bad = ~(err <= bound)                      # (a NaN in the reconstruction fails too)
            if bool(bad.any()) and first is None:
                t, c = bad.nonzero()[0].tolist()
                first = (t0 + t, c, float(recon[t0 + t, c]), float(R[t, c]), float(bound[t, c]))
            n_bad += int(bad.sum())
            ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
            max_ratio = max(max_ratio, float(ratio.max()))
        assert n_bad == 0, (f"{what}: {n_bad} reconstruction elements lie outside gamma_(k+1) (|b_dec| + sum |v W_dec|) of f64; "
                            f"first (token, column, got, f64, bound) = {first}")
        return {"max_ratio_recon": max_ratio}


# ---- level C --------------------------------------------------------------------------------------------------------------
def sample_rows(T: int, status=None, seed: int = 0, n: int = 64, n_random_min: int = 16, n_fallback: int = 32) -> np.ndarray:
    """Sorted token rows of level C (module docstring).  `status`: the call's per-token codes (array-like) or None."""
    must = {0, 255, 256, 257, T - 1}
    for b in range(2048, T, 2048):
        must.update((b - 1, b))
    must = {r for r in must if 0 <= r < T}
    rest = np.setdiff1d(np.arange(T), np.fromiter(must, dtype=np.int64))
    n_rand = min(len(rest), max(n - len(must), n_random_min))
    rng = np.random.default_rng(seed)
    rows = must | set(rng.choice(rest, n_rand, replace=False).tolist())
    if status is not None:
        fb = np.flatnonzero((np.asarray(status) & 0xFF) == 1)
        fb = fb[~np.isin(fb, np.fromiter(rows, dtype=np.int64))]
        if len(fb) > n_fallback:
            fb = rng.choice(fb, n_fallback, replace=False)
        rows |= set(int(r) for r in fb)
    return np.array(sorted(rows), dtype=np.int64)


def level_c(oracle, host, x, out, rows, k, what="") -> int:
    """The sampled tokens against the C oracle, bit for bit.  host = (W_enc, b_enc, W_dec, b_dec) as numpy f32 arrays."""
    W_enc, b_enc, W_dec, b_dec = host
    r = torch.from_numpy(rows).to(x.device)
    xs = x.index_select(0, r).float().cpu().numpy()
    ref_v, ref_i = oracle.encode_topk(xs, W_enc, b_enc, b_dec, k)
    ref_r = oracle.decode(ref_i, ref_v, W_dec, b_dec)
    got_i = out["top_indices"].index_select(0, r).cpu().numpy()
    got_v = out["top_acts"].index_select(0, r).cpu().numpy()
    got_r = out["sae_out"].index_select(0, r).cpu().numpy()
    bad_i = (got_i != ref_i.astype(np.int64)).any(axis=1)
    bad_v = (got_v.view(np.uint32) != ref_v.view(np.uint32)).any(axis=1)
    bad_r = (got_r.view(np.uint32) != ref_r.view(np.uint32)).any(axis=1)
    assert not bad_i.any(), f"{what}: indices differ from the C oracle on tokens {rows[bad_i][:8].tolist()}"
    assert not bad_v.any(), f"{what}: values differ from the C oracle on tokens {rows[bad_v][:8].tolist()}"
    assert not bad_r.any(), f"{what}: reconstruction differs from the C oracle on tokens {rows[bad_r][:8].tolist()}"
    return len(rows)


# ---- coverage line --------------------------------------------------------------------------------------------------------
GEMM_BM = GEMM_BN = 256       # csrc/encode_fused.hip: GemmI8 / GemmI8Cert / GemmF8 = GemmCfg<256, 256, ...>
SAMPLE_STRIDE = 32            # csrc/encode_defs.h


def tiles_per_workgroup(T: int, N: int, n_cu: int, mode: str = "int8"):
    """(main, sample) output tiles the busiest persistent workgroup of the candidate GEMM walks.  csrc/gemm_mfma.h gemm_launch:
    nM x nN tiles of GEMM_BM x GEMM_BN over the padded batch; the grid is one workgroup per CU, rounded down to a multiple
    of 8 (these configurations hold more than 80 KiB of LDS: per_cu = 1), or one per tile when there are fewer tiles.  The
    sample pass scores N / SAMPLE_STRIDE features; the int8 and certified main passes leave those out (MAIN_SKIPS_SAMPLE)."""
    grid = max(8, n_cu // 8 * 8)
    nM = -(-T // GEMM_BM)
    n_sample = N // SAMPLE_STRIDE
    n_main = N - n_sample if mode in ("int8", "certified", "dither_off") else N
    per_wg = lambda tiles: -(-tiles // grid) if tiles > grid else 1
    return per_wg(nM * (n_main // GEMM_BN)), per_wg(nM * (n_sample // GEMM_BN))
