"""GPU: the fused encoder under a perturbed schedule -- every token, bit for bit, with the waves running at other relative speeds.

The suite's value, shape and edge tests exercise ONE schedule per kernel, and at their shapes a persistent workgroup of the
candidate GEMM gets one output tile.  The one silent-wrong bug of this project (d74ff0c: the EARLY side-buffer pair written
under slower waves' epilogue reads) needed several tiles per workgroup and showed only at N = 262144, T = 8192.  The
perturbed-schedule variant of the library (csrc/tuning.h: MSAE_PERTURB, MSAE_GRID_CAP = 8; csrc/build.sh builds it beside the
product) delays waves pseudo-randomly at every hand-synchronised hand-over and runs the looping launches on 8 workgroups; this
test runs the fused-encode pipeline on it at small shapes.

The library path is read once per process, so the variant runs in ONE fresh child (tests/perturbed_runner.py, which also holds
the cases and their inputs).  This process -- the product library -- computes per case, from fixed seeds,
  (a) the exact path of every token, ops.topk(ops.pre_acts(...)) in chunks, and holds its first 8 tokens to oracle.encode_topk;
  (b) the product's fused encode under ops.set_dither("on", seed), every token of which must equal (a) as well;
the child requires of every token of every case, under six perturbation seeds (two were asked for; a case costs
milliseconds): values and indices bit-identical to (a), no status 2, status identical to (b) -- timing must not decide which
tokens fall back.  There is no tolerance anywhere.

Coverage the child asserts (and prints): both candidate-GEMM passes of cases 1, 2 and 6 walk >= 4 tiles per workgroup
(d = 256, N = 65536, T = 1024: the sample pass is 4 x 8 = 32 tiles, the main pass 4 x 248 = 992, on 8 workgroups 4 and 124
each; N = 32768 would give the sample pass 2), and every probe site declared in csrc/tuning.h is visited at least once.

Time (MI355X): the child process took CHILD_MEASURED_S = 4.7 s (2.4 s of it work -- the 162 encodes 1.9 s, the rest generating
inputs -- and 2.3 s interpreter start, importing torch and initialising HIP with everything warm), this whole test 9.7 s.
Three times the measurement is 14 s; CHILD_LIMIT_S = 40 leaves the start-up, which a cold machine stretches and the work does
not, another 26 s: a child killed at its limit counts as a hang, and no test waits for this limit to run out.
"""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

import perturbed_runner as pr
from encode_routes import np32, same_bits
from oracle import oracle

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
CHILD_MEASURED_S = 4.7
CHILD_LIMIT_S = 40


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from msae import _hip

    _hip.load()
    return torch.device("cuda:0")


def _resolve_edits(case, exact_i):
    """Case 6's features from case 1's exact result: the sample feature (index = 13 mod 32) that is in the most tokens' top-k
    is forced to a value that puts it at the head of every list; the most frequent top-k member of all is zeroed."""
    counts = np.bincount(exact_i.reshape(-1), minlength=case["N"])
    if case["edit"] == "set":
        sample = np.arange(13, case["N"], 32)
        case["set_feature"], case["set_value"] = int(sample[np.argmax(counts[sample])]), 123.5
        assert counts[case["set_feature"]] > 0, "no sample feature in any top-k"
    else:
        case["zero_feature"] = int(np.argmax(counts))


def test_every_token_under_perturbed_schedules(dev, tmp_path):
    from msae import ops

    assert pr.VARIANT.exists(), (f"{pr.VARIANT} is missing: build it with `sh multimodal-sae_amd/csrc/build.sh` "
                                 "(python __graft_entry__.py)")
    cases, first = pr.base_cases(), {}
    for case in cases:
        if "edit" in case:
            _resolve_edits(case, first["exact_i"])
        W, b, bd, x = pr.make_inputs(case, dev)
        ev, ei = pr.run_exact(case, W, b, bd, x)
        rv, ri = oracle.encode_topk(np32(x[:8]), np32(W), np32(b), np32(bd), case["k"], set_feature=case["set_feature"],
                                    set_value=case["set_value"], zero_feature=case["zero_feature"])
        n8 = min(8, case["T"])
        assert same_bits(ev[:n8], rv[:n8]).all() and same_bits(ei[:n8], ri[:n8].astype(np.int64)).all(), \
            f"{case['name']}: the exact path differs from the oracle on the first tokens"
        v, i, st = pr.run_fused(case, W, b, bd, x)
        same = same_bits(v, ev) & same_bits(i, ei)
        print(f"{case['name']}: product status 0 / 1 / 2 on {int((st == 0).sum())} / {int((st == 1).sum())} / {int((st >= 2).sum())} "
              f"of {case['T']} tokens")
        assert (st < 2).all() and same.all(), \
            f"{case['name']}: the PRODUCT's fused encode differs from the exact path on tokens {np.flatnonzero(~same)[:16].tolist()}"
        np.savez(tmp_path / f"{case['name']}.npz", exact_v=ev, exact_i=ei, status=st)
        if not first:
            first = dict(exact_i=ei)
        del W, b, bd, x
        ops.release_workspaces()
    (tmp_path / "cases.json").write_text(json.dumps(cases))
    torch.cuda.synchronize()

    env = dict(os.environ, MSAE_HIP_LIB=str(pr.VARIANT))
    for name in ("MSAE_FM", "MSAE_NO_SMALL_PATH", "MSAE_NO_SKINNY", "MSAE_LPR", "MSAE_COARSE", "MSAE_DITHER"):
        env.pop(name, None)
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, str(REPO / "tests" / "perturbed_runner.py"), str(tmp_path)]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT_S + 60)
    print(r.stdout[-60000:])
    print(f"the child process took {time.perf_counter() - t0:.1f} s of its {CHILD_LIMIT_S} s")
    # a child that died by a signal or at its limit (timeout: 124 / 137) may have left the device faulted: nothing more runs here
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-6000:]}\n{r.stderr[-3000:]}"
    assert r.stdout.count("ok:") == len(pr.PERTURB_SEEDS) * len(cases) and "WRONG" not in r.stdout, r.stdout[-6000:]
