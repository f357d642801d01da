"""Cases, inputs and the child process of tests/test_gpu_perturbed_schedule.py.

The perturbed-schedule variant of the library (csrc/build.sh -> msae/_lib/libmsae_hip_perturb.so; csrc/tuning.h: MSAE_PERTURB,
MSAE_GRID_CAP = 8) delays waves pseudo-randomly at the hand-synchronised hand-overs of the fused encoder and runs the looping
launches on 8 workgroups, so that every workgroup walks several tiles at small shapes.  The library path is read once per
process, hence a process of its own:

    MSAE_HIP_LIB=multimodal-sae_amd/msae/_lib/libmsae_hip_perturb.so python tests/perturbed_runner.py <dir>

<dir> holds what the parent (the product library) wrote: cases.json -- the resolved cases -- and <case>.npz with
  exact_v, exact_i   the exact path of every token: ops.topk(ops.pre_acts(...)) with the case's edits applied to the latents
  status             the product's fused encode of the same inputs under the same dither seed
This child regenerates the inputs from the same seeds, runs the same fused encode on the variant under each of
PERTURB_SEEDS and requires of EVERY token: values and indices bit-identical to the exact path, no status 2, status equal to
the product's.  It prints per case the wall time and the (pass, tiles, grid) record of every candidate-GEMM launch, asserts the
tiles per workgroup a case names, stops at the first case that is wrong, and ends with the table of probe sites against visits:
a declared site nobody visited is an error (a case is missing).  Exit status 0 iff everything held.
"""
import ctypes
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "tests", REPO / "multimodal-sae_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

VARIANT = REPO / "multimodal-sae_amd" / "msae" / "_lib" / "libmsae_hip_perturb.so"
DITHER_SEED = 0xD17E5
# Six schedules per case (the issue asks for two; a case costs milliseconds): on the re-created d74ff0c defect one (seed, case)
# pair of case 1 shows a wrong token in about 5 of 8 runs (profiles/perturb_sensitivity.txt), twelve pairs miss it with 1e-5
PERTURB_SEEDS = tuple(0x5EED0001 + j for j in range(6))
COARSE = {"bf16": 0, "int8": 1, "fp8": 2}


def base_cases():
    """The cases before the parent resolves the edited features of case 6.  d = 256 with N % 8192 == 0 is the smallest family
    with the fused fast path; the weight-stream kernel and the small path exist from d = 1024 on (d % 1024 == 0), so cases 4
    and 5 run at both widths: d = 256 as one row of candidate-GEMM tiles, d = 1024 on the routes they are named after.
    tiles: the least tiles per workgroup BOTH candidate-GEMM passes must show in the launch record (0: only printed)."""
    c = []

    def add(name, d, N, T, k, kind="trained_like", tiles=0, **kw):
        c.append(dict(name=name, d=d, N=N, T=T, k=k, kind=kind, tiles=tiles, seed=len(c) + 1, coarse="int8", certified=False,
                      set_feature=-1, set_value=0.0, zero_feature=-1, env={}, shards=0, rows="residual", bias_shift=0.0) | kw)

    # 1: int8 default, GEMM route.  N = 65536: the sample pass is 4 x 8 = 32 tiles (S = 2048 columns), the main pass 4 x 248 =
    # 992; on 8 workgroups 4 and 124 tiles each
    add("1-int8-trained", 256, 65536, 1024, 32, tiles=4)
    add("1-int8-gauss", 256, 65536, 1024, 32, kind="gauss", tiles=4)
    # 2: the other operand types of case 1
    add("2-bf16", 256, 65536, 1024, 32, tiles=4, coarse="bf16")
    add("2-fp8", 256, 65536, 1024, 32, tiles=4, coarse="fp8")
    add("2-certified", 256, 65536, 1024, 32, tiles=4, certified=True)
    # 3: row padding (two row tiles, the second mostly padding) and the four-wave select of k = 256
    add("3-T257", 256, 16384, 257, 32)
    add("3-T300", 256, 16384, 300, 32)
    add("3-k256", 256, 16384, 512, 256)
    # 4 / 5: <= 256 tokens and <= 16 tokens
    for d in (256, 1024):
        for T in (17, 64, 256):
            add(f"4-stream-d{d}-T{T}", d, 16384, T, 32)
    for d in (256, 1024):
        for T in (1, 2, 5, 16):
            add(f"5-small-d{d}-T{T}", d, 8192, T, 32)
    # 6: case 1 with hook edits (features resolved by the parent from case 1's exact result)
    add("6-set-feature", 256, 65536, 1024, 32, tiles=4, seed=1, edit="set")
    add("6-zero-feature", 256, 65536, 1024, 32, tiles=4, seed=1, edit="zero")
    # 7: feature-sharded legs, G = 2 emulated on one device
    add("7-sharded-G2", 256, 16384, 1024, 32, shards=2)
    # 8: all-zero rows and rows with fewer than k positive latents among ordinary ones: the exact fallback's row list is
    # non-empty and its capped launches loop (16 column tiles per workgroup, the rows over 8 workgroups)
    add("8-fallback-rows", 256, 16384, 600, 32, kind="gauss", rows="mixed", bias_shift=-3.0)
    # 9: the feature-major first round of the re-score (forced: the shape is below where it pays)
    add("9-feature-major", 256, 16384, 1024, 32, env={"MSAE_FM": "1"})
    return c


def make_inputs(case, dev):
    """-> W [N, d], b [N], b_dec [d] f32, x [T, d] bf16 from the case's seeds (hostile.py: outlier dims, massive tokens)."""
    import torch

    import hostile

    W, b, bd = hostile.weights(case["kind"], case["N"], case["d"], dev, seed=case["seed"])
    b = (b + case["bias_shift"]).contiguous()
    T, d = case["T"], case["d"]
    x = hostile.activations(T, d, dev, seed=100 + case["seed"])
    if case["rows"] == "mixed":
        # with b_enc ~ -3: an ordinary token has ~12 % positive latents; x = b_dec + 0.93 N(0, 1) has Poisson(~10) of 16384
        # (P(z > 3.2)), fewer than k = 32; x = 0 has none.  The first 8 tokens stay ordinary (they are held to the oracle, which
        # lists no zero activations).
        g = torch.Generator(device=dev).manual_seed(9000 + case["seed"])
        sparse = (bd + 0.93 * torch.randn(T, d, generator=g, device=dev)).to(torch.bfloat16)
        t = torch.arange(T, device=dev)
        few = (t >= 8) & (t % 7 == 2)
        zero = (t >= 8) & (t % 5 == 3)
        x = torch.where(few[:, None], sparse, x)
        x = torch.where(zero[:, None], torch.zeros_like(x), x)
    return W, b, bd, x.contiguous()


class _Env:
    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def run_fused(case, W, b, bd, x):
    """The case's fused encode on whatever library this process loaded -> (vals, idx, status) as numpy arrays."""
    import torch

    from msae import ops
    from msae.parallel import default_candidates

    ops.set_dither("on", seed=DITHER_SEED)
    ops.set_coarse_mode(case["coarse"])
    edits = dict(set_feature=case["set_feature"], zero_feature=case["zero_feature"])
    try:
        with _Env(case["env"]), torch.no_grad():
            if case["shards"]:
                G, N, k = case["shards"], case["N"], case["k"]
                n_loc, C = N // G, default_candidates(k, G)
                recs = []
                for g in range(G):
                    lo = g * n_loc
                    prep = ops.prepare_encoder(W[lo:lo + n_loc])
                    recs.append(ops.shard_candidates(x, b[lo:lo + n_loc].contiguous(), bd, prep, n_loc, k, lo, C))
                v, i, st = ops.rescore_candidates(x, W, b, bd, k, torch.stack(recs).contiguous(), C)
            else:
                prep = ops.prepare_encoder(W)
                v, i, st = ops.encode_topk(x, W, b, bd, prep, case["k"], set_value=case["set_value"],
                                           coarse_mode=COARSE[case["coarse"]], certified=case["certified"], **edits)
            torch.cuda.synchronize()
    finally:                                   # (process defaults: the parent is the suite's pytest process)
        ops.set_coarse_mode("default")
        ops.set_dither("default", 0)
    return v.cpu().numpy(), i.cpu().numpy().astype("int64"), st.cpu().numpy()


def run_exact(case, W, b, bd, x, chunk=256):
    """The exact path of every token, chunked: top-k of the f32 latents with the case's edits applied to them."""
    import numpy as np
    import torch

    from msae import ops

    vs, ix = [], []
    with torch.no_grad():
        for t0 in range(0, case["T"], chunk):
            lat = ops.pre_acts(x[t0:t0 + chunk], W, b, bd)
            if case["set_feature"] >= 0:
                lat[:, case["set_feature"]] = case["set_value"]
            if case["zero_feature"] >= 0:
                lat[:, case["zero_feature"]] = 0.0
            v, i = ops.topk(lat, case["k"])
            vs.append(v.cpu().numpy())
            ix.append(i.cpu().numpy().astype("int64"))
            del lat
    return np.concatenate(vs), np.concatenate(ix)


class Probes:
    """The variant-only exports, bound here: msae._hip.PROTOTYPES mirrors include/msae.h, which does not know them."""

    def __init__(self, lib):
        self.lib = lib
        for name, res, args in (("msae_perturb_set_seed", ctypes.c_int, [ctypes.c_uint]), ("msae_perturb_reset", ctypes.c_int, []),
                                ("msae_perturb_hits", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]),
                                ("msae_perturb_site_name", ctypes.c_char_p, [ctypes.c_int]),
                                ("msae_perturb_launches", ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args

    def reset(self):
        rc = self.lib.msae_perturb_reset()
        assert rc == 0, f"msae_perturb_reset: HIP error {rc}"

    def seed(self, s):
        rc = self.lib.msae_perturb_set_seed(s)
        assert rc == 0, f"msae_perturb_set_seed: HIP error {rc}"

    def hits(self):
        buf = (ctypes.c_ulonglong * 256)()
        n = self.lib.msae_perturb_hits(buf, 256)
        assert 0 < n <= 256, f"msae_perturb_hits: {n}"
        return [(self.lib.msae_perturb_site_name(s).decode(), int(buf[s])) for s in range(n)]

    def launches(self):
        """(pass, tiles, grid) of the candidate-GEMM launches since the last call."""
        buf = (ctypes.c_int * (3 * 64))()
        n = self.lib.msae_perturb_launches(buf, 64)
        return [("sample" if buf[3 * j] == 0 else "main", int(buf[3 * j + 1]), int(buf[3 * j + 2])) for j in range(n)]


def check_tiles(case, recs):
    """The launch record's coverage bound: both passes ran, each workgroup of each walked >= case['tiles'] tiles."""
    if not case["tiles"]:
        return None
    for kind in ("sample", "main"):
        mine = [r for r in recs if r[0] == kind]
        if not mine:
            return f"no {kind} pass in the launch record {recs}"
        for _, tiles, grid in mine:
            if tiles // grid < case["tiles"]:
                return f"{kind} pass: {tiles} tiles on {grid} workgroups = {tiles // grid} per workgroup, {case['tiles']} wanted"
    return None


def main(argv) -> int:
    if len(argv) != 2:
        print(__doc__)
        return 2
    if Path(os.environ.get("MSAE_HIP_LIB", "")).name != VARIANT.name:
        print(f"start this runner with MSAE_HIP_LIB={VARIANT} in its environment")
        return 2
    import numpy as np
    import torch

    from encode_routes import same_bits
    from msae import _hip

    t_start = time.perf_counter()
    work = Path(argv[1])
    cases = json.loads((work / "cases.json").read_text())
    dev = torch.device("cuda:0")
    probes = Probes(_hip.load())
    probes.reset()
    total = 0.0
    for pseed in PERTURB_SEEDS:
        probes.seed(pseed)
        for case in cases:
            ref = np.load(work / f"{case['name']}.npz")
            W, b, bd, x = make_inputs(case, dev)
            torch.cuda.synchronize()
            probes.launches()
            t0 = time.perf_counter()
            v, i, st = run_fused(case, W, b, bd, x)
            dt = time.perf_counter() - t0
            total += dt
            recs = probes.launches()
            same = same_bits(v, ref["exact_v"]) & same_bits(i, ref["exact_i"])
            wrong, unresolved, moved = np.flatnonzero(~same), np.flatnonzero(st >= 2), np.flatnonzero(st != ref["status"])
            why = check_tiles(case, recs)
            good = not len(wrong) and not len(unresolved) and not len(moved) and why is None
            print(f"{'ok:' if good else 'WRONG:'} {case['name']} seed {pseed:#x}: {dt:.2f} s; T = {case['T']}, status 1 on "
                  f"{int((st == 1).sum())} tokens (product {int((ref['status'] == 1).sum())}); launches (pass, tiles, grid) {recs}",
                  flush=True)
            if not good:
                print(f"  tokens not bit-equal to the exact path: {len(wrong)} {wrong[:16].tolist()} (status there "
                      f"{st[wrong[:16]].tolist()}); status 2: {unresolved[:16].tolist()}; status differs from the product's on "
                      f"{len(moved)} tokens {moved[:16].tolist()}: variant {st[moved[:16]].tolist()}, product "
                      f"{ref['status'][moved[:16]].tolist()}; tiles: {why}", flush=True)
                return 1
            del W, b, bd, x
    print(f"wall time: the cases' encodes {total:.1f} s, the child from its start {time.perf_counter() - t_start:.1f} s")
    missing = 0
    print("site visits:")
    for name, n in probes.hits():
        print(f"  {n:12d}  {name}")
        missing += n == 0
    if missing:
        print(f"WRONG: {missing} declared probe sites were never visited -- a case is missing")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
