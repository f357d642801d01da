"""The measurements of profiles/transcoder.txt at d = 4096, N = 131072, T = 8192, k = 32: the skip
forward (in-place accumulate against GEMM + add), the weight gradient with its two transposes priced separately, and one
training step of a TopK auto-encoder, a transcoder and a skip transcoder in one process.

    python tools/transcoder_bench.py [OUT.txt]"""
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "multimodal-sae_amd")]
import torch

from msae import Sae, SaeConfig, ops
from msae.train import SaeTrainStep

dev = torch.device("cuda:0")
d, N, T, k = 4096, 131072, 8192, 32
out = open(sys.argv[1] if len(sys.argv) > 1 else "/dev/null", "w")


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(T, d, device=dev, generator=g)
W = torch.randn(d, d, device=dev, generator=g) / 64
yhat = torch.randn(T, d, device=dev, generator=g)
flop = 2.0 * T * d * d
say(f"shape d={d} N={N} T={T} k={k}; one GEMM = {flop / 1e9:.1f} GFLOP; times in ms as median (min .. max) of 10")
for name, fn in (("skip forward, in-place accumulate (gemm_nt_add_)", lambda: ops.gemm_nt_add_(yhat, x, W)),
                 ("skip forward, _dense_gemm_nt + add", lambda: yhat.add_(ops._dense_gemm_nt(x, W))),
                 ("_dense_gemm_nt alone", lambda: ops._dense_gemm_nt(x, W))):
    m, lo, hi = timed(fn)
    say(f"{name}: {m:.3f} ({lo:.3f} .. {hi:.3f})  {flop / m / 1e9:.1f} TFLOP/s")
gout = torch.randn(T, d, device=dev, generator=g)
grad = torch.zeros(d, d, device=dev)
m, lo, hi = timed(lambda: (gout.t().contiguous(), x.t().contiguous()))
say(f"weight gradient, the two transposes (torch copies): {m:.3f} ({lo:.3f} .. {hi:.3f})")
gt, xt = gout.t().contiguous(), x.t().contiguous()
m, lo, hi = timed(lambda: ops.gemm_nt_add_(grad, gt, xt))
say(f"weight gradient, gemm_nt(g^T, x^T) accumulate=1: {m:.3f} ({lo:.3f} .. {hi:.3f})  {flop / m / 1e9:.1f} TFLOP/s")
m, lo, hi = timed(lambda: ops.gemm_nt_add_(grad, gout.t().contiguous(), x.t().contiguous()))
say(f"weight gradient, transposes + GEMM: {m:.3f} ({lo:.3f} .. {hi:.3f})")
del gt, xt, gout, grad, yhat, W
torch.cuda.empty_cache()

y = torch.randn(T, d, device=dev, generator=g)
for name, kw in (("TopK auto-encoder", {}), ("transcoder", dict(transcode=True)),
                 ("skip transcoder", dict(transcode=True, skip_connection=True))):
    sae = Sae(d, SaeConfig(num_latents=N, k=k, **kw), device=dev)
    if kw:
        with torch.no_grad():
            sae.W_dec.copy_(sae.encoder.weight)          # (a trained decoder: zeros would make the backward trivial)
    ts = SaeTrainStep(sae, lr=1e-4)
    step = (lambda: ts.step(x, y)) if kw else (lambda: ts.step(x))
    m, lo, hi = timed(step, warm=3, reps=8)
    say(f"training step, {name}: {m:.3f} ({lo:.3f} .. {hi:.3f})")
    del sae, ts, step
    torch.cuda.empty_cache()
out.close()
