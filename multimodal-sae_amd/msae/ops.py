"""PyTorch-ROCm custom ops (``torch.ops.msae.*``) over the C ABI of libmsae_hip.so.

These are the operators the drop-in ``Sae`` module (msae/sae/sae.py) and the feature cache
(msae/features/cache.py) are built from.  Reference call sites they replace:

    msae::pre_acts      nn.Linear + relu                     sae_auto_interp/sae/sae.py:172-177
    msae::topk          Tensor.topk                          sae/sae.py:179-181, features/cache.py:210
    msae::encode_topk   Sae.encode, fused (+ hook edits)     sae/sae.py:183-185, steering.py:113-114
    msae::decode        decoder_impl / TritonDecoder.apply   sae/utils.py:107-129, kernels.py:403-429
    msae::sparsify      scatter_ + Cache.get_nonzeros/add    features/cache.py:214-217,42-92
    msae::pooled_acts   pre_acts(h).mean(0) per segment      tools/probe_activations.py:109-126
    msae::probe_maps    latents[:, :, idx]                   tools/probe_activations.py:126
    msae::row_inv_norms F.normalize's 1 / max(norm, eps)     features/stats.py:80-81
    msae::rows_topk     torch.mm + torch.topk, fused         features/stats.py:35-37,83,107
    msae::pre_acts_features  pre_acts(x)[..., features]      sae/sae.py:207-225 (AuxK: the dead latents only)
    msae::recon_curve   decode + e.pow(2).sum() per checkpoint  sae/sae.py:190,201 (one pass for several sparsities)
    msae::support_refit least-squares coefficients on the encoder's support (no reference counterpart)
    batch_kth, list_filter, batch_select, decode(lengths=)   BatchTopK on top-C lists (no reference counterpart)
    gemm_nt_add_, skip_add                                    a transcoder's dense skip term, accumulated in place

All ops run on the tensor's device on the current stream, never synchronise (``sparsify`` reads one
int64 back, as ``torch.nonzero`` does), and raise on CPU tensors.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import dataclasses
import os
import weakref
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _hip

_WS: "collections.OrderedDict" = collections.OrderedDict()
_WS_MAX_STREAMS = 8      # scratch buffers kept alive: the most recently used (device, stream) pairs


def _workspace(dev: torch.device, nbytes: int) -> Tensor:
    """Grow-only scratch buffer per (device, stream) -- calls enqueued on different streams may run
    concurrently and must not share scratch (uint8, 256-B aligned by the caching allocator).  At most
    _WS_MAX_STREAMS buffers stay alive (least recently used first out; a dropped buffer goes back to the
    caching allocator, which keeps it valid for the kernels already enqueued on its stream)."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = None
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
    _WS[key] = ws                      # most recently used last
    while len(_WS) > _WS_MAX_STREAMS:
        _WS.popitem(last=False)
    return ws


_WS_EPOCH = [0]


def workspace_epoch() -> int:
    """Bumped whenever cached scratch buffers are dropped: anything that captured their addresses (a HIP graph of the hooks'
    S = 1 step) re-captures."""
    return _WS_EPOCH[0]


def release_workspaces() -> None:
    """Drop every cached scratch buffer (they are re-created on demand)."""
    _WS_EPOCH[0] += 1
    _WS.clear()
    _CERT_CACHE.clear()
    _OPTS_CACHE.clear()


# ---- per-call options of the fused encoder (struct msae_options) ------------------------------------------
# The shared library keeps no state: coarse mode, band width, diagnostics and the stage profile travel with
# every call.  `Options` is the host-side mirror; `_defaults` is what the ops of THIS Python process use when a
# call does not bring its own (a convenience of the host layer, set by set_coarse_mode() & co.).
class StageProfile:
    """Handle of msae_profile_create: HIP events at the stage boundaries of every fused encode that carries it."""

    STAGES = 6

    def __init__(self, max_steps: int):
        self.max_steps = max_steps
        self._h = ctypes.c_void_p()
        _hip.check(_hip.load().msae_profile_create(max_steps, ctypes.byref(self._h)), "msae_profile_create")

    @property
    def handle(self):
        return self._h

    def read(self):
        """-> float32 array [n_steps, 6] of stage times in ms; restarts the handle."""
        import numpy as np

        buf = (ctypes.c_float * (self.max_steps * self.STAGES))()
        n = ctypes.c_int(0)
        _hip.check(_hip.load().msae_profile_read(self._h, buf, ctypes.byref(n)), "msae_profile_read")
        return np.array(buf[:], dtype=np.float32).reshape(self.max_steps, self.STAGES)[: n.value]

    def close(self):
        if self._h:
            _hip.load().msae_profile_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Options:
    COARSE = {"default": -1, "bf16": 0, "int8": 1, "fp8": 2}
    DITHER = {"default": 0, "on": 1, "off": 2}

    def __init__(self, coarse: str = "default", guard_z: float = 0.0, status_detail: bool = False,
                 profile: Optional[StageProfile] = None, exact: bool = False, dither: str = "default",
                 dither_seed: int = 0):
        self.coarse, self.guard_z, self.status_detail, self.profile = coarse, guard_z, status_detail, profile
        self.exact = exact
        self.dither, self.dither_seed = dither, int(dither_seed)   # msae_options::dither / dither_seed (0: drawn per call)
        self.rows_rescored: Optional[Tensor] = None     # device int32 [T] (msae_options::rows_rescored) or None
        self.certified = False                          # msae_options::certified (+ the operand buffer of the call)
        self.certified_operands: Optional[Tensor] = None

    def struct(self) -> "_hip.MsaeOptions":
        o = _hip.MsaeOptions()
        o.size = ctypes.sizeof(_hip.MsaeOptions)
        o.coarse_mode = self.COARSE[self.coarse]
        o.guard_z = float(self.guard_z)
        o.status_detail = int(bool(self.status_detail))
        o.profile = self.profile.handle if self.profile is not None else None
        o.exact = int(bool(self.exact))
        o.dither = self.DITHER[self.dither]
        o.dither_seed = self.dither_seed & 0xFFFFFFFFFFFFFFFF
        o.rows_rescored = self.rows_rescored.data_ptr() if self.rows_rescored is not None else None
        o.certified = int(bool(self.certified))
        o.certified_operands = self.certified_operands.data_ptr() if self.certified_operands is not None else None
        return o

    def ref(self):
        self._keep = self.struct()        # keeps the struct alive for the duration of the call
        return ctypes.byref(self._keep)


_defaults = Options()


class _OptsRef:
    """A filled msae_options struct and its byref, built once per distinct content (the S = 1 latency path is
    host-bound: two ctypes structs per call showed up as +10 us per decode step)."""
    __slots__ = ("struct", "_ref", "profile", "cert_ops")

    def __init__(self, o: Options):
        self.struct, self.profile = o.struct(), o.profile          # (keeps the profile handle alive)
        self.cert_ops = o.certified_operands                       # (... and the certified operand buffer)
        self._ref = ctypes.byref(self.struct)

    def ref(self):
        return self._ref


_OPTS_CACHE: dict = {}
_WS_BYTES_CACHE: dict = {}


_DITHER_NAME = {0: "default", 1: "on", 2: "off"}


def _opts(coarse_mode: int = -1, guard_z: float = 0.0, status_detail: bool = False, exact: bool = False,
          dither: int = 0, dither_seed: int = 0, cert_ops: Optional[Tensor] = None) -> _OptsRef:
    """Options of one call: explicit arguments win, the process defaults fill the rest."""
    coarse = _defaults.coarse if coarse_mode < 0 else {0: "bf16", 1: "int8", 2: "fp8"}[coarse_mode]
    z = guard_z if guard_z > 0.0 else _defaults.guard_z
    detail = bool(status_detail or _defaults.status_detail)
    exact = bool(exact or _defaults.exact)
    dith = _DITHER_NAME[dither] if dither else _defaults.dither
    seed = dither_seed if dither_seed else _defaults.dither_seed
    prof, rows = _defaults.profile, _defaults.rows_rescored
    if cert_ops is not None:
        # a certified call brings its 2 N d-byte operand buffer: built per call and never cached -- a cache entry would pin the
        # buffer of every weight version a training / evaluation loop has been through; the call is milliseconds
        o = Options(coarse, z, detail, prof, exact, dith, seed)
        o.certified, o.certified_operands = True, cert_ops
        o.rows_rescored = rows
        return _OptsRef(o)
    key = (coarse, z, detail, id(prof) if prof is not None else 0, exact, rows.data_ptr() if rows is not None else 0,
           dith, seed)
    ref = _OPTS_CACHE.get(key)
    if ref is None or ref.profile is not prof:
        if len(_OPTS_CACHE) > 64:
            _OPTS_CACHE.clear()
        o = Options(coarse, z, detail, prof, exact, dith, seed)
        o.rows_rescored = rows
        ref = _OPTS_CACHE[key] = _OptsRef(o)
    return ref


def _encode_ws_bytes(lib, T: int, d: int, N: int, k: int, opts: _OptsRef) -> int:
    """msae_encode_topk_ws_bytes, memoised (a pure function of the shape and the coarse mode)."""
    key = (T, d, N, k, opts.struct.coarse_mode, os.environ.get("MSAE_COARSE") if opts.struct.coarse_mode < 0 else None,
           os.environ.get("MSAE_FM"), opts.struct.certified,
           # (the library reads the switch at every call, and the small-T plan is the larger one: a size memoised with the switch
           # set would be too small for the same shape without it)
           os.environ.get("MSAE_NO_SMALL_PATH") if T <= 16 else None)
    n = _WS_BYTES_CACHE.get(key)
    if n is None:
        if len(_WS_BYTES_CACHE) > 4096:
            _WS_BYTES_CACHE.clear()
        n = _WS_BYTES_CACHE[key] = lib.msae_encode_topk_ws_bytes(T, d, N, k, opts.ref())
    return n


@contextlib.contextmanager
def profiling(profile: StageProfile):
    """Fused encodes issued inside the block record their stage boundaries into `profile`."""
    prev, _defaults.profile = _defaults.profile, profile
    try:
        yield profile
    finally:
        _defaults.profile = prev


@contextlib.contextmanager
def rescore_rows(buf: Tensor):
    """Fused encodes of <= buf.numel() tokens issued inside the block write their per-token re-score statistics
    (msae_options::rows_rescored: [bit 30: first round feature-major] | rounds << 24 | first-round rows << 12 | rows of W_enc
    read; 0 = not verified by the large-batch re-score) into `buf` (device int32)."""
    assert buf.is_cuda and buf.dtype == torch.int32 and buf.is_contiguous()
    prev, _defaults.rows_rescored = _defaults.rows_rescored, buf
    try:
        yield buf
    finally:
        _defaults.rows_rescored = prev


@contextlib.contextmanager
def _without_rows():
    prev, _defaults.rows_rescored = _defaults.rows_rescored, None
    try:
        yield
    finally:
        _defaults.rows_rescored = prev


def _opts_for(T: int, dev) -> "_OptsRef":
    """The process defaults as the options of a call of T tokens on `dev` (see encode_topk: the statistics buffer only
    where it is large enough)."""
    rows = _defaults.rows_rescored
    if rows is not None and (T > rows.numel() or rows.device != dev):
        with _without_rows():
            return _opts()
    return _opts()


_DEBUG_BOUNDS = os.environ.get("MSAE_DEBUG_BOUNDS", "0") not in ("", "0")


def set_debug_bounds(on: bool) -> None:
    """Debug mode (environment MSAE_DEBUG_BOUNDS=1): decode and its backward read the kernels' out-of-range flag
    back after the call (one host synchronisation per call) and raise IndexError -- the analogue of the reference's
    tl.device_assert(i < N) (sae/kernels.py:276,389).  Off: out-of-range indices are skipped silently."""
    global _DEBUG_BOUNDS
    _DEBUG_BOUNDS = bool(on)


def _bounds_flag(dev) -> Optional[Tensor]:
    return torch.zeros(1, dtype=torch.int32, device=dev) if _DEBUG_BOUNDS else None


def _check_bounds(flag: Optional[Tensor], what: str) -> None:
    if flag is not None and int(flag.item()) != 0:
        raise IndexError(f"{what}: a latent index lies outside [0, num_latents)")


def _f32c(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is None:
        return None
    return t.detach().to(torch.float32).contiguous()


def _act(x: Tensor) -> Tensor:
    x = x.detach()
    if x.dtype not in _hip.DTYPE_CODE:
        x = x.to(torch.float32)
    return x.contiguous()


# ------------------------------------------------------------------------------------------------
@torch.library.custom_op("msae::pre_acts", mutates_args=())
def pre_acts(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor]) -> Tensor:
    """relu((x - b_dec) @ W_enc.T + b_enc) -> dense [..., N] f32 (exact f32 MFMA path)."""
    dev = _hip.require_device(x, W_enc, b_enc, b_dec)
    lib = _hip.load()
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    assert xa.shape[-1] == d, f"x last dim {xa.shape[-1]} != d_in {d}"
    T = xa.numel() // d
    out = torch.empty(*xa.shape[:-1], N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_pre_acts_f32(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(W),
                                         _hip.ptr(be), _hip.ptr(bd), T, d, N, 1, _hip.ptr(out),
                                         _hip.stream_of(xa)), "msae_pre_acts_f32")
    return out


@pre_acts.register_fake
def _(x, W_enc, b_enc, b_dec):
    return x.new_empty(*x.shape[:-1], W_enc.shape[0], dtype=torch.float32)


def _dense_gemm_nt(a: Tensor, b: Tensor) -> Tensor:
    """a [M, K] @ b[P, K]^T -> [M, P] f32 on the exact f32 MFMA kernel (msae_pre_acts_f32 without bias / ReLU)."""
    lib = _hip.load()
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    if out.numel():
        with torch.cuda.device(a.device):
            _hip.check(lib.msae_pre_acts_f32(_hip.ptr(a), 0, _hip.ptr(b), None, None, a.shape[0], a.shape[1],
                                             b.shape[0], 0, _hip.ptr(out), _hip.stream_of(a)), "msae_pre_acts_f32")
    return out


def _pre_acts_setup(ctx, inputs, output):
    x, W_enc, b_enc, b_dec = inputs
    ctx.save_for_backward(x, W_enc, b_dec, output)
    ctx.has = (b_enc is not None, b_dec is not None)


def _pre_acts_backward(ctx, grad_out):
    """The dense graph of the reference's nn.Linear + relu (sae.py:172-177): legacy callers that differentiate
    pre_acts -> [mask] -> select_topk -> decode (features/patching/utils.py:41-49, tools/*.py) get the same
    gradients as from torch autograd -- two dense GEMMs on the exact f32 MFMA kernel.  (The fused
    Sae.encode(zero_feature=...) path has the sparse backward and never builds [T, N] gradients.)"""
    x, W_enc, b_dec, out = ctx.saved_tensors
    N, d = W_enc.shape
    g = (grad_out.reshape(-1, N).float() * (out.reshape(-1, N) > 0)).contiguous()       # relu'
    need_x, need_W, need_be, need_bd = ctx.needs_input_grad
    g_x = g_W = g_be = g_bd = None
    if need_x or (need_bd and ctx.has[1]):
        da = _dense_gemm_nt(g, W_enc.detach().float().t())                 # [T, N] @ [N, d]
        g_x = da.view(x.shape).to(x.dtype) if need_x else None
        g_bd = -da.sum(0) if (need_bd and ctx.has[1]) else None
    if need_W:
        a = x.detach().reshape(-1, d).float()
        if ctx.has[1]:
            a = a - b_dec.detach().float()
        g_W = _dense_gemm_nt(g.t(), a.t()).to(W_enc.dtype)                 # [N, T] @ [T, d]
    if need_be and ctx.has[0]:
        g_be = g.sum(0)
    return g_x, g_W, g_be, g_bd


pre_acts.register_autograd(_pre_acts_backward, setup_context=_pre_acts_setup)


# ---- the skip term of a transcoder (csrc/skip_gemm.hip) ----------------------------------------------
@torch.library.custom_op("msae::gemm_nt_add_", mutates_args=("C",))
def _gemm_nt_add(C: Tensor, a: Tensor, B: Tensor, accumulate: bool) -> None:
    M, K = a.shape
    P = B.shape[0]
    if not C.is_cuda:
        # the host has no exact-chain route (pre_acts has none either): float32 matmul, the meaning and not the bits
        s = a.detach().to(torch.float32) @ B.detach().to(torch.float32).t()
        C.copy_(C + s if accumulate else s)
        return
    dev = _hip.require_device(C, a, B)
    aa, Bc = _act(a), _f32c(B)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_gemm_nt_acc_f32(_hip.ptr(aa), _hip.DTYPE_CODE[aa.dtype], _hip.ptr(Bc), M, K, P,
                                                    _hip.ptr(C), C.stride(0), int(accumulate), _hip.stream_of(C)),
                   "msae_gemm_nt_acc_f32")


def gemm_nt_add_(C: Tensor, a: Tensor, B: Tensor, accumulate: bool = True) -> Tensor:
    """C[m][p] += sum_j a[m][j] B[p][j], in place (accumulate=False: C = the sum): a [M, K] in f32 / bf16 / f16, B [P, K]
    f32, C f32 [M, P] with unit column stride and a row stride >= P (a row-sliced or column-sliced view works; what lies
    between the rows is not touched).  The sum is the ascending-j f32 fma chain of the exact encoder GEMM, joined to C by one
    f32 add: no atomics, the same bits on every run (include/msae.h, msae_gemm_nt_acc_f32).  Host tensors take a float32
    torch matmul: the same meaning, not the same bits.  No autograd: `skip_add` is the differentiable form."""
    if C.dim() != 2 or a.dim() != 2 or B.dim() != 2 or C.dtype != torch.float32:
        raise ValueError(f"gemm_nt_add_: C (f32), a and B must be matrices, got {tuple(C.shape)} {C.dtype}, {tuple(a.shape)}, "
                         f"{tuple(B.shape)}")
    if a.shape[1] != B.shape[1] or a.shape[1] < 1 or B.shape[0] < 1 or tuple(C.shape) != (a.shape[0], B.shape[0]):
        raise ValueError(f"gemm_nt_add_: a [M, K], B [P, K] and C [M, P] do not fit: {tuple(a.shape)}, {tuple(B.shape)}, "
                         f"{tuple(C.shape)}")
    if C.shape[0] and (C.stride(1) != 1 or C.stride(0) < C.shape[1]):
        raise ValueError(f"gemm_nt_add_: C needs unit column stride and a row stride >= {C.shape[1]}, got {C.stride()}")
    if C.shape[0]:
        _gemm_nt_add(C, a, B, bool(accumulate))
    return C


_SKIP_GRAD_IN_PLACE = False


@contextlib.contextmanager
def skip_grad_in_place():
    """Inside the block the backward of `skip_add` ADDS its weight gradient into an existing contiguous float32 W_skip.grad
    with the kernel's own epilogue (gradient accumulation: no [d_out, d_in] temporary, no separate add; the same bits as
    autograd's grad + g_W) and hands autograd None for W_skip.  That is a side effect on .grad which autograd does not see: a
    hook registered on W_skip with register_hook is handed None in place of the gradient for that backward, whether a
    post-accumulate hook (the data-parallel exchange hangs on those) still fires is the autograd engine's business and is
    not relied on, and torch.autograd.grad(loss, [W_skip]) would change .grad and report W_skip as unused.  So it is opt-in:
    SaeTrainStep enters it around `backward()` on a single rank, nothing else does."""
    global _SKIP_GRAD_IN_PLACE
    prev, _SKIP_GRAD_IN_PLACE = _SKIP_GRAD_IN_PLACE, True
    try:
        yield
    finally:
        _SKIP_GRAD_IN_PLACE = prev


class _SkipAdd(torch.autograd.Function):
    """dec_out += x W_skip^T in place.  Backward: g passes through to dec_out; g_W = g^T x as gemm_nt(g^T, x^T), returned to
    autograd -- or, inside `skip_grad_in_place()` and where W_skip is a leaf that holds a .grad already, accumulated into that
    .grad by the kernel (see there for what that costs); g_x = g W_skip only where x requires grad.  The GEMM's K is the token
    count: one that is no multiple of 4 takes the tile's element-load staging (the same bits, not measured)."""

    @staticmethod
    def forward(ctx, dec_out, x, W_skip):
        d_out, d_in = W_skip.shape
        gemm_nt_add_(dec_out.view(-1, d_out), x.detach().reshape(-1, d_in), W_skip.detach())
        ctx.mark_dirty(dec_out)
        ctx.save_for_backward(x, W_skip)
        return dec_out

    @staticmethod
    def backward(ctx, g):
        x, W_skip = ctx.saved_tensors
        d_out, d_in = W_skip.shape
        _, need_x, need_W = ctx.needs_input_grad
        g2 = g.reshape(-1, d_out)
        g_x = g_W = None
        if need_W:
            # the two transposes are torch copies (a TN staging path in the tile is a follow-up: DESIGN.md section 8)
            gt = g2.to(torch.float32).t().contiguous()
            xt = x.detach().reshape(-1, d_in).t().contiguous()
            grad = W_skip.grad if _SKIP_GRAD_IN_PLACE and W_skip.is_leaf else None
            if grad is not None and grad.dtype == torch.float32 and grad.is_contiguous() and grad.device == g.device:
                gemm_nt_add_(grad, gt, xt)
            else:
                g_W = gemm_nt_add_(torch.empty(d_out, d_in, dtype=torch.float32, device=g.device), gt, xt, accumulate=False)
                g_W = g_W.to(W_skip.dtype)
        if need_x:
            Wt = W_skip.detach().to(torch.float32).t()
            gx = _dense_gemm_nt(g2.to(torch.float32), Wt) if g.is_cuda else g2.to(torch.float32) @ Wt.t()
            g_x = gx.view(x.shape).to(x.dtype)
        return g, g_x, g_W


def skip_add(dec_out: Tensor, x: Tensor, W_skip: Tensor) -> Tensor:
    """The dense skip connection of a transcoder: dec_out [..., d_out] (f32, contiguous; the decode's output) += x [..., d_in]
    W_skip [d_out, d_in]^T, IN PLACE (one T x d_out pass and one allocation less than a GEMM and an add), as one autograd
    node.  Returns dec_out.  Token counts divisible by 4 keep the weight gradient's GEMM (K = T) on the tile's vector staging;
    any other count runs its element-load staging (the same bits)."""
    d_out, d_in = W_skip.shape
    if dec_out.dtype != torch.float32 or not dec_out.is_contiguous() or dec_out.shape[-1] != d_out or x.shape[-1] != d_in \
            or dec_out.shape[:-1] != x.shape[:-1]:
        raise ValueError(f"skip_add: dec_out must be contiguous f32 [..., {d_out}] and x [..., {d_in}] over the same tokens, "
                         f"got {tuple(dec_out.shape)} {dec_out.dtype}, {tuple(x.shape)}")
    if torch.is_grad_enabled() and (dec_out.requires_grad or x.requires_grad or W_skip.requires_grad):
        return _SkipAdd.apply(dec_out, x, W_skip)
    gemm_nt_add_(dec_out.view(-1, d_out), x.reshape(-1, d_in), W_skip)
    return dec_out


@torch.library.custom_op("msae::topk", mutates_args=())
def topk(latents: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """Canonical top-k along the last dim: values descending, ties by ascending index; int64 idx."""
    dev = _hip.require_device(latents)
    lib = _hip.load()
    lat = _f32c(latents)
    N = lat.shape[-1]
    T = lat.numel() // N
    vals = torch.empty(*lat.shape[:-1], k, dtype=torch.float32, device=dev)
    idx = torch.empty(*lat.shape[:-1], k, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_topk_f32(_hip.ptr(lat), T, N, k, _hip.ptr(vals), _hip.ptr(idx), None, 0,
                                     _hip.stream_of(lat)), "msae_topk_f32")
    return vals, idx.to(torch.int64)


@topk.register_fake
def _(latents, k):
    return (latents.new_empty(*latents.shape[:-1], k, dtype=torch.float32),
            latents.new_empty(*latents.shape[:-1], k, dtype=torch.int64))


def _topk_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.in_shape, ctx.in_dtype = inputs[0].shape, inputs[0].dtype


def _topk_backward(ctx, g_vals, _g_idx):
    """Tensor.topk's backward: the values' gradient scattered to the selected positions (sae.py:179-181)."""
    idx, = ctx.saved_tensors
    g = torch.zeros(ctx.in_shape, dtype=g_vals.dtype, device=g_vals.device)
    g.scatter_(-1, idx, g_vals)
    return g.to(ctx.in_dtype), None


topk.register_autograd(_topk_backward, setup_context=_topk_setup)


# ---- exact encode over a feature subset (csrc/encode_f32.hip) -----------------------------------------
TOPK_MAX_K = 16384           # msae_topk_f32's limit: the k winners live in LDS


def _pre_acts_features_into(xa: Tensor, W: Tensor, be: Optional[Tensor], bd: Optional[Tensor], feats: Tensor,
                            out: Tensor, ld: int, relu: int = 1) -> None:
    """msae_pre_acts_features_f32 on prepared operands: xa [T, d] (f32 / bf16 / f16, contiguous), feats int32 [M], out a
    buffer of at least T * ld floats."""
    (N, d), T, M = W.shape, xa.shape[0], feats.numel()
    with torch.cuda.device(xa.device):
        _hip.check(_hip.load().msae_pre_acts_features_f32(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(W), _hip.ptr(be),
                                                          _hip.ptr(bd), _hip.ptr(feats), M, T, d, N, relu, _hip.ptr(out),
                                                          ld, _hip.stream_of(xa)), "msae_pre_acts_features_f32")


@torch.library.custom_op("msae::pre_acts_features", mutates_args=())
def pre_acts_features(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor],
                      features: Tensor) -> Tensor:
    """relu((x - b_dec) @ W_enc[features].T + b_enc[features]) -> [..., M] f32 without the dense [..., N] latents: column m
    is bit for bit column features[m] of `pre_acts` (include/msae.h, "exact encode over a feature subset").  features: int32
    device tensor [M], any order, repeats allowed, entries outside [0, N) clamped.  The result is a view of a buffer whose
    rows are M rounded up to 4 floats apart (so that a top-k over it takes its vector loads).  No autograd."""
    dev = _hip.require_device(x, W_enc, b_enc, b_dec, features)
    assert features.dtype == torch.int32 and features.dim() == 1, \
        f"features must be a 1-d int32 tensor, got {features.dtype} {tuple(features.shape)}"
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    assert xa.shape[-1] == d, f"x last dim {xa.shape[-1]} != d_in {d}"
    feats = features.detach().contiguous()
    M = feats.numel()
    ld = (M + 3) & ~3
    out = torch.empty(*xa.shape[:-1], ld, dtype=torch.float32, device=dev)
    if M and out.numel():
        _pre_acts_features_into(xa.reshape(-1, d), W, be, bd, feats, out, ld)
    return out[..., :M]


@pre_acts_features.register_fake
def _(x, W_enc, b_enc, b_dec, features):
    M = features.shape[0]
    return x.new_empty(*x.shape[:-1], (M + 3) & ~3, dtype=torch.float32)[..., :M]


def rows_per_chunk(T: int, M: int, max_ws_bytes: int = 256 << 20) -> int:
    """Token rows per chunk of `topk_within`: the largest multiple of 128 (the GEMM's row tile) whose [rows, ld] f32
    buffer, ld = M rounded up to 4, stays within max_ws_bytes -- at least 128, at most T."""
    ld = max((M + 3) & ~3, 4)
    rows = max(max_ws_bytes // (ld * 4) // 128 * 128, 128)
    return min(rows, T)


def topk_within(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor], features: Tensor, k: int, *,
                max_ws_bytes: int = 256 << 20) -> Tuple[Tensor, Tensor]:
    """The canonical top-k of every token's latents WITHIN a feature list -> (vals [T, k] f32, idx [T, k] int64, global
    feature ids): what `where(mask, pre_acts(x), -inf).topk(k)` returns for the mask of an ascending `features` (int32
    device tensor [M]), bit for bit, without the dense latents.  Ties: value descending, then ascending position in the
    list.  x [T, d].  T is walked in chunks of `rows_per_chunk(T, M, max_ws_bytes)` rows: each chunk's [rows, M] latents go
    into one reused buffer (the default cap is the Infinity Cache's 256 MiB), its top-k straight into the output rows.
    Nothing is read back to the host.  1 <= k <= min(M, 16384), else ValueError.  No autograd."""
    assert features.dtype == torch.int32 and features.dim() == 1, \
        f"features must be a 1-d int32 tensor, got {features.dtype} {tuple(features.shape)}"
    M = features.numel()
    if not 1 <= k <= min(M, TOPK_MAX_K):
        raise ValueError(f"topk_within: k must be in [1, min(len(features), {TOPK_MAX_K})], got k = {k} with "
                         f"{M} features")
    dev = _hip.require_device(x, W_enc, b_enc, b_dec, features)
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    assert xa.dim() == 2 and xa.shape[1] == d, f"x must be [T, {d}], got {tuple(xa.shape)}"
    feats = features.detach().contiguous()
    T = xa.shape[0]
    vals = torch.empty(T, k, dtype=torch.float32, device=dev)
    idx = torch.empty(T, k, dtype=torch.int64, device=dev)
    if T == 0:
        return vals, idx
    ld = (M + 3) & ~3
    rows = rows_per_chunk(T, M, max_ws_bytes)
    buf = torch.empty(rows * ld, dtype=torch.float32, device=dev)
    lib = _hip.load()
    for t0 in range(0, T, rows):
        n = min(rows, T - t0)
        _pre_acts_features_into(xa[t0:t0 + n], W, be, bd, feats, buf, ld)
        with torch.cuda.device(dev):
            _hip.check(lib.msae_topk_map_i64_f32(_hip.ptr(buf), n, M, k, ld, _hip.ptr(feats), _hip.ptr(vals[t0:t0 + n]),
                                                 _hip.ptr(idx[t0:t0 + n]), _hip.stream_of(xa)), "msae_topk_map_i64_f32")
    return vals, idx


# ------------------------------------------------------------------------------------------------
@torch.library.custom_op("msae::pooled_acts", mutates_args=())
def pooled_acts(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor], segments: Tensor,
                chunks: Optional[Tensor], reduce: int) -> Tensor:
    """Per segment s (int32 [S, 2] device rows [start, end) over x's [T, d] rows): the mean (reduce 0) or max (1) over its
    tokens of relu((x - b_dec) @ W_enc.T + b_enc) -> [S, N] f32, without the dense [T, N] latents.  `chunks`: int32 [C, 2]
    device segment ranges of msae.sae.probe.plan_chunks, or None (one per segment).  include/msae.h: numerics contract."""
    dev = _hip.require_device(x, W_enc, b_enc, b_dec, segments, chunks)
    lib = _hip.load()
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    assert xa.dim() == 2 and xa.shape[1] == d, f"x must be [T, {d}], got {tuple(xa.shape)}"
    seg = segments.contiguous()
    ch = None if chunks is None else chunks.contiguous()
    S = seg.shape[0]
    out = torch.empty(S, N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_pooled_acts_f32(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(W), _hip.ptr(be), _hip.ptr(bd),
                                            xa.shape[0], d, N, _hip.ptr(seg), S, _hip.ptr(ch),
                                            0 if ch is None else ch.shape[0], reduce, _hip.ptr(out), _hip.stream_of(xa)),
                   "msae_pooled_acts_f32")
    return out


@pooled_acts.register_fake
def _(x, W_enc, b_enc, b_dec, segments, chunks, reduce):
    return x.new_empty(segments.shape[0], W_enc.shape[0], dtype=torch.float32)


@torch.library.custom_op("msae::probe_maps", mutates_args=())
def probe_maps(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor], segments: Tensor,
               indices: Tensor) -> Tensor:
    """maps[t, j] = relu((x[t] - b_dec) @ W_enc[indices[s, j]] + b_enc[...]) for the tokens t of segment s, 0 elsewhere ->
    [T, k] f32, bit-identical to pre_acts(x)[t, indices[s, j]]."""
    dev = _hip.require_device(x, W_enc, b_enc, b_dec, segments, indices)
    lib = _hip.load()
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    assert xa.dim() == 2 and xa.shape[1] == d, f"x must be [T, {d}], got {tuple(xa.shape)}"
    seg = segments.contiguous()
    idx = indices.to(torch.int32).contiguous()
    S, k = idx.shape
    assert seg.shape[0] == S, f"{seg.shape[0]} segments but {S} rows of indices"
    maps = torch.empty(xa.shape[0], k, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_probe_maps_f32(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(W), _hip.ptr(be), _hip.ptr(bd),
                                           xa.shape[0], d, N, _hip.ptr(seg), S, _hip.ptr(idx), k, _hip.ptr(maps),
                                           _hip.stream_of(xa)), "msae_probe_maps_f32")
    return maps


@probe_maps.register_fake
def _(x, W_enc, b_enc, b_dec, segments, indices):
    return x.new_empty(x.shape[0], indices.shape[1], dtype=torch.float32)


# ---- neighbours / top logits (features/stats.py:12-47,76-120) -----------------------------------------------------------
ROWS_TOPK_MAX_K = 64


def _no_grad_inputs(what: str, *tensors: Optional[Tensor]) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is an inference path: call it under torch.no_grad() or on detached inputs")


@torch.library.custom_op("msae::row_inv_norms", mutates_args=())
def _row_inv_norms(W: Tensor) -> Tensor:
    dev = _hip.require_device(W)
    lib = _hip.load()
    Wc = _f32c(W)
    assert Wc.dim() == 2, f"W must be [N, d], got {tuple(Wc.shape)}"
    N, d = Wc.shape
    inv = torch.empty(N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_row_inv_norms_f32(_hip.ptr(Wc), N, d, _hip.ptr(inv), _hip.stream_of(Wc)),
                   "msae_row_inv_norms_f32")
    return inv


@_row_inv_norms.register_fake
def _(W):
    return W.new_empty(W.shape[0], dtype=torch.float32)


def row_inv_norms(W: Tensor) -> Tensor:
    """inv[n] = the f32 nearest to 1 / max(||W[n]||_2, 1e-12) (F.normalize's clamp), norms summed in f64 in a fixed order
    (bit-reproducible) -> [N] f32.  Inference only."""
    _no_grad_inputs("ops.row_inv_norms", W)
    return _row_inv_norms(W)


@torch.library.custom_op("msae::rows_topk", mutates_args=())
def _rows_topk(Q: Tensor, K: Tensor, k: int, q_rows: Optional[Tensor], q_scale: Optional[Tensor],
               k_scale: Optional[Tensor], exclude: Optional[Tensor], chunks: int) -> Tuple[Tensor, Tensor]:
    dev = _hip.require_device(Q, K, q_rows, q_scale, k_scale, exclude)
    lib = _hip.load()
    # (a view whose storage offset breaks the 16-B alignment stays a view: the kernel takes its generic staging path)
    Qc = Q.detach() if (Q.dtype == torch.float32 and Q.is_contiguous()) else _f32c(Q)
    Kc = K.detach() if (K.dtype == torch.float32 and K.is_contiguous()) else _f32c(K)
    assert Qc.dim() == 2 and Kc.dim() == 2 and Qc.shape[1] == Kc.shape[1], \
        f"Q [Qn, d] and K [N, d] must share d, got {tuple(Qc.shape)} and {tuple(Kc.shape)}"
    (Qn, d), N = Qc.shape, Kc.shape[0]
    rows = None if q_rows is None else q_rows.detach().to(torch.int32).contiguous()
    M = Qn if rows is None else rows.numel()
    qs, ks = _f32c(q_scale), _f32c(k_scale)
    ex = None if exclude is None else exclude.detach().to(torch.int32).contiguous()
    if not 1 <= k <= ROWS_TOPK_MAX_K or k > N - (0 if ex is None else 1):
        raise ValueError(f"k must be in [1, min({ROWS_TOPK_MAX_K}, keys{' - 1' if ex is not None else ''})], got k = {k} "
                         f"with {N} keys")
    assert qs is None or qs.numel() == M, f"q_scale has {qs.numel()} entries for {M} queries"
    assert ks is None or ks.numel() == N, f"k_scale has {ks.numel()} entries for {N} keys"
    assert ex is None or ex.numel() == M, f"exclude has {ex.numel()} entries for {M} queries"
    vals = torch.empty(M, k, dtype=torch.float32, device=dev)
    idx = torch.empty(M, k, dtype=torch.int64, device=dev)      # written directly: no widening pass
    if M == 0:
        return vals, idx
    nbytes = lib.msae_rows_topk_ws_bytes(M, N, k, chunks)
    if nbytes == 0:
        raise ValueError(f"rows_topk: chunks = {chunks} is out of range for k = {k} (chunks * k <= 8192)")
    ws = _workspace(dev, nbytes)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_rows_topk_i64_f32(_hip.ptr(Qc), Qn, _hip.ptr(rows), M, _hip.ptr(Kc), N, d, _hip.ptr(qs),
                                              _hip.ptr(ks), _hip.ptr(ex), k, chunks, _hip.ptr(vals), _hip.ptr(idx),
                                              _hip.ptr(ws), ws.numel(), _hip.stream_of(Qc)), "msae_rows_topk_i64_f32")
    return vals, idx


@_rows_topk.register_fake
def _(Q, K, k, q_rows, q_scale, k_scale, exclude, chunks):
    M = Q.shape[0] if q_rows is None else q_rows.numel()
    return Q.new_empty(M, k, dtype=torch.float32), Q.new_empty(M, k, dtype=torch.int64)


def rows_topk(Q: Tensor, K: Tensor, k: int, q_rows: Optional[Tensor] = None, q_scale: Optional[Tensor] = None,
              k_scale: Optional[Tensor] = None, exclude: Optional[Tensor] = None, chunks: int = 0) -> Tuple[Tensor, Tensor]:
    """The canonical top-k (value descending, index ascending) of every row of (Q[q_rows] @ K.T) * q_scale[:, None] *
    k_scale[None, :] without the dense [M, N] product -> (vals f32 [M, k], idx int64 [M, k]).  Q [Qn, d], K [N, d] f32;
    q_rows int [M] (None: every row of Q; entries outside [0, Qn) are clamped); q_scale [M], k_scale [N] f32 or None;
    exclude int [M]: a key index each query skips (< 0: none); 1 <= k <= 64; chunks: 0 = chosen by the library.  The bits are
    include/msae.h's contract ("neighbours"): the dots are pre_acts's, the two scales separate f32 multiplies, and the
    result does not depend on `chunks` or on the other queries of the call.  Inference only."""
    _no_grad_inputs("ops.rows_topk", Q, K, q_scale, k_scale)
    return _rows_topk(Q, K, k, q_rows, q_scale, k_scale, exclude, chunks)


def set_coarse_mode(mode: str) -> None:
    """Default operand type of the fused encoder's candidate pass for this process's ops: "int8", "bf16", "fp8" (e4m3
    operands -- BASELINE configs[4]; its prepared operands take the int8 ones' place, so prepare under the mode you encode in) or
    "default" (environment MSAE_COARSE, else int8).  Outputs do not depend on it (candidates are re-scored
    exactly); speed does.  A host-layer default: the library itself takes the mode per call (msae_options)."""
    if mode not in Options.COARSE:
        raise ValueError(f"coarse mode {mode!r}: expected one of {sorted(Options.COARSE)}")
    _defaults.coarse = mode


def set_guard_z(z: float) -> None:
    """Default width of the candidate pass's error band in standard deviations of its per-(token, feature)
    rounding noise (library default 7; 0 restores it).  Verified results do not depend on it; rows read per token do."""
    if z != 0.0 and not (0.25 <= z <= 64.0):
        raise ValueError("guard z must lie in [0.25, 64] (or 0 for the default)")
    _defaults.guard_z = float(z)


def set_exact(on: bool) -> None:
    """Default of msae_options::exact for this process's ops: every fused encode computes every token by the exact path
    (no statistical contract; ~20x slower on large batches)."""
    _defaults.exact = bool(on)


def set_dither(mode: str = "default", seed: int = 0) -> None:
    """Default of msae_options::dither / dither_seed for this process's ops: "on" rounds the int8 operands stochastically
    (activations per encode call, weights per prepare / refresh) so that the fused encoder's miss bound holds for EVERY input
    (include/msae.h); "off" is round-to-nearest with the statistical noise model; "default" = environment MSAE_DITHER, else on.
    seed != 0 pins the hash seed of every call (reproducible candidate sets); 0 lets the library draw one per call."""
    if mode not in Options.DITHER:
        raise ValueError(f"dither mode {mode!r}: expected one of {sorted(Options.DITHER)}")
    _defaults.dither, _defaults.dither_seed = mode, int(seed)


def set_certified(on: bool) -> None:
    """Default of msae_options::certified for this process's ops: every fused encode runs the certified candidate pass (two
    int8 planes per operand, deterministic band: include/msae.h) -- its operands are built on first use per (weight, bias)
    version and cached (`prepare_encoder_certified`)."""
    _defaults.certified = bool(on)


_CERT_CACHE: "collections.OrderedDict" = collections.OrderedDict()
_CERT_NOTED: set = set()          # shapes whose "no certified pass -> exact path" warning has been given


def prepare_encoder_certified(W_enc: Tensor, b_enc: Optional[Tensor]) -> Optional[Tensor]:
    """msae_encoder_prepare_certified: the certified pass's operand buffer for (W_enc, b_enc), or None when the shape has no
    certified pass (the library then runs the exact path).  Cached per (pointer, version) of both tensors, two most recent
    (weights edited through `.data` do not bump the version: call release_workspaces() after such an edit)."""
    dev = _hip.require_device(W_enc, b_enc)
    lib = _hip.load()
    key = (dev, W_enc.data_ptr(), W_enc._version, tuple(W_enc.shape), 0 if b_enc is None else b_enc.data_ptr(),
           0 if b_enc is None else b_enc._version)
    hit = _CERT_CACHE.get(key)
    # (the entry remembers WHICH tensor objects it was built from, weakly: the key is addresses and version counters, and the
    # caching allocator hands a freed parameter's address to the next model of the same shape)
    if hit is not None and hit[1]() is W_enc and (b_enc is None or hit[2]() is b_enc):
        _CERT_CACHE.move_to_end(key)
        return hit[0]
    W, b = _f32c(W_enc), _f32c(b_enc)
    N, d = W.shape
    nbytes = lib.msae_encoder_certified_bytes(N, d)
    if nbytes == 0:
        return None
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_encoder_prepare_certified(_hip.ptr(W), _hip.ptr(b), N, d, _hip.ptr(buf), _hip.stream_of(W)),
                   "msae_encoder_prepare_certified")
    _CERT_CACHE[key] = (buf, weakref.ref(W_enc), weakref.ref(b_enc) if b_enc is not None else None)
    while len(_CERT_CACHE) > 2:
        _CERT_CACHE.popitem(last=False)
    return buf


def invalidate_certified(W_enc: Optional[Tensor] = None) -> None:
    """Forget the certified operand buffers built from `W_enc` (all of them when None).  The cache trusts the tensors' version
    counters, which an edit through `.data` does not bump: `Sae.invalidate_prepared` calls this, so the documented
    remedy after such an edit covers `encode(certified=True)` as well -- a stale certified buffer would rank features by
    the OLD weights and a token could verify with a wrong top-k."""
    if W_enc is None:
        _CERT_CACHE.clear()
        return
    for key in [k for k in _CERT_CACHE if k[1] == W_enc.data_ptr() or _CERT_CACHE[k][1]() is W_enc]:
        _CERT_CACHE.pop(key, None)


def coarse_in_force() -> str:
    """The candidate pass's operand type an encode issued NOW would resolve to: the process default, else the environment's
    MSAE_COARSE, else int8 (the library's rule, csrc/encode_defs.h resolve_opts)."""
    if _defaults.coarse != "default":
        return _defaults.coarse
    e = os.environ.get("MSAE_COARSE", "")[:1]
    return {"b": "bf16", "f": "fp8"}.get(e, "int8")


def dither_in_force() -> bool:
    """Whether an encode / prepare issued NOW rounds the int8 operands stochastically (process default, else MSAE_DITHER)."""
    if _defaults.dither != "default":
        return _defaults.dither == "on"
    return os.environ.get("MSAE_DITHER", "1")[:1] != "0"


def set_status_detail(on: bool) -> None:
    """Diagnostics: tokens recomputed inside the call report 1 | reason << 8 instead of 1."""
    _defaults.status_detail = bool(on)


def prepare_encoder(W_enc: Tensor, out: Optional[Tensor] = None, active_mode_only: bool = False,
                    tokens_next: int = 0) -> Tensor:
    """Coarse-pass operands of the encoder weights for the fused path (bf16 copy, int8 quantisation,
    sampled rows).  Once per weight load; `out` + `active_mode_only` is the per-step refresh of a
    training loop (rebuilds only what the coarse mode in force reads, into the same buffer; `tokens_next` > 0: only what
    ONE following encode of that many tokens reads -- msae_encoder_refresh_for)."""
    dev = _hip.require_device(W_enc)
    lib = _hip.load()
    W = _f32c(W_enc)
    N, d = W.shape
    nbytes = lib.msae_encoder_prepared_bytes(N, d)
    if out is None or out.numel() != nbytes or out.device != dev:
        out, active_mode_only = torch.empty(nbytes, dtype=torch.uint8, device=dev), False
    with torch.cuda.device(dev):
        if active_mode_only and tokens_next > 0:
            _hip.check(lib.msae_encoder_refresh_for(_hip.ptr(W), N, d, _hip.ptr(out), int(tokens_next), _opts().ref(),
                                                    _hip.stream_of(W)), "msae_encoder_refresh_for")
        elif active_mode_only:
            _hip.check(lib.msae_encoder_refresh(_hip.ptr(W), N, d, _hip.ptr(out), _opts().ref(), _hip.stream_of(W)),
                       "msae_encoder_refresh")
        else:
            _hip.check(lib.msae_encoder_prepare_opts(_hip.ptr(W), N, d, _hip.ptr(out), _opts().ref(), _hip.stream_of(W)),
                       "msae_encoder_prepare_opts")
    return out


_TRAIN_PREPARED: dict = {}
# key -> (weight version, coarse mode, covers batches of <= 256 tokens, weak reference to the weight tensor).  The reference
# pins the entry to ONE tensor object: the key is an address, and the caching allocator hands a freed parameter's address to
# the next model of the same shape -- whose version counter can stand at the same value (the certified cache met exactly that).
_TRAIN_FRESH: dict = {}


def _train_key(W_enc: Tensor):
    return (W_enc.device, W_enc.data_ptr(), tuple(W_enc.shape))


def train_operand_buffer(W_enc: Tensor) -> Tensor:
    """The per-parameter operand buffer of the training loop (allocated on first use): what `adam_rows_(refresh=...)`
    rebuilds inside the optimiser pass and `_refresh_train_operands` hands to the next encode."""
    key = _train_key(W_enc)
    buf = _TRAIN_PREPARED.get(key)
    if buf is None:
        nbytes = _hip.load().msae_encoder_prepared_bytes(W_enc.shape[0], W_enc.shape[1])
        if len(_TRAIN_PREPARED) > 8:
            _TRAIN_PREPARED.clear(); _TRAIN_FRESH.clear()
        buf = _TRAIN_PREPARED[key] = torch.empty(nbytes, dtype=torch.uint8, device=W_enc.device)
    return buf


def mark_train_operands_fresh(W_enc: Tensor, tokens_next: int) -> None:
    """The optimiser pass has just rebuilt train_operand_buffer(W_enc) from the updated weight (its version as of now)."""
    _TRAIN_FRESH[_train_key(W_enc)] = (W_enc._version, coarse_in_force(), tokens_next <= 256, weakref.ref(W_enc))


def invalidate_train_operands(W_enc: Optional[Tensor] = None) -> None:
    """Forget that the training loop's operand buffer of `W_enc` (all buffers when None) is fresh: the next training encode
    rebuilds it.  `_refresh_train_operands` trusts the tensor's version counter, which `p.data.copy_()` / `.data.mul_()`, a
    custom C op or an external optimiser writing through `.data` do NOT bump: call this wherever the weight is
    edited that way (`Sae.invalidate_prepared`, which `Sae.load_from_disk` ends with, does).  MSAE_DEBUG_OPERANDS=1 rebuilds
    before every training encode regardless."""
    if W_enc is None:
        _TRAIN_FRESH.clear()
    else:
        _TRAIN_FRESH.pop(_train_key(W_enc), None)


def _refresh_train_operands(W_enc: Tensor, tokens: int) -> Tensor:
    """Per-step operands of a weight that changes every step: one buffer per parameter, rebuilt in
    place for the coarse mode in force and for the batch size of the ONE encode that follows (it runs in that mode on
    `tokens` tokens; the buffer is rebuilt before it is read again) -- unless the optimiser pass that produced this
    version of the weight has already rebuilt it (adam_rows_(refresh=...): no second sweep over W_enc)."""
    key = _train_key(W_enc)
    fresh = _TRAIN_FRESH.get(key) if os.environ.get("MSAE_DEBUG_OPERANDS", "0") in ("", "0") else None
    if fresh is not None and fresh[:2] == (W_enc._version, coarse_in_force()) and fresh[3]() is W_enc \
            and (tokens > 256 or fresh[2]) and key in _TRAIN_PREPARED:
        return _TRAIN_PREPARED[key]
    buf = prepare_encoder(W_enc, _TRAIN_PREPARED.get(key), active_mode_only=True, tokens_next=tokens)
    if len(_TRAIN_PREPARED) > 8 and key not in _TRAIN_PREPARED:
        _TRAIN_PREPARED.clear(); _TRAIN_FRESH.clear()
    _TRAIN_PREPARED[key] = buf
    _TRAIN_FRESH[key] = (W_enc._version, coarse_in_force(), tokens <= 256, weakref.ref(W_enc))
    return buf


@torch.library.custom_op("msae::encode_topk", mutates_args=())
def encode_topk(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor],
                prepared: Optional[Tensor], k: int, set_feature: int = -1, set_value: float = 0.0,
                zero_feature: int = -1, coarse_mode: int = -1, guard_z: float = 0.0,
                status_detail: bool = False, exact: bool = False, dither: int = 0,
                dither_seed: int = 0, certified: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """Fused Sae.encode -> (top_acts f32 [...,k], top_indices int64 [...,k], status int32 [...]).
    coarse_mode (-1 default / 0 bf16 / 1 int8), guard_z (0 = default), status_detail and exact (every token by the
    exact path: include/msae.h, msae_options::exact), dither (0 default / 1 on / 2 off) and dither_seed (0 = drawn by the
    library) and certified (the two-plane pass with the deterministic band; its operand buffer comes from
    prepare_encoder_certified's cache) are this call's msae_options; what is left at its default comes from the process
    defaults (set_coarse_mode & co.)."""
    dev = _hip.require_device(x, W_enc, b_enc, b_dec, prepared)
    lib = _hip.load()
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    assert xa.shape[-1] == d, f"x last dim {xa.shape[-1]} != d_in {d}"
    T = xa.numel() // d
    # the kernels write every element of all three outputs (int64 indices directly: no widening pass)
    vals = torch.empty(*xa.shape[:-1], k, dtype=torch.float32, device=dev)
    idx = torch.empty(*xa.shape[:-1], k, dtype=torch.int64, device=dev)
    status = torch.empty(xa.shape[:-1], dtype=torch.int32, device=dev)
    if T == 0:
        return vals, idx, status
    cert_ops = None
    if (certified or _defaults.certified) and not (exact or _defaults.exact):
        cert_ops = prepare_encoder_certified(W_enc, b_enc)
        if cert_ops is None:
            exact = True                 # a shape without the certified pass: the exact path is the certified answer
            if (N, d) not in _CERT_NOTED:                           # ... and ~20x the time on large batches: say so, once per shape
                _CERT_NOTED.add((N, d))
                import warnings

                warnings.warn(f"certified encode: no certified pass for num_latents = {N}, d_in = {d} (it needs num_latents % 8192 "
                              "== 0 and d_in % 128 == 0, d_in <= 65536); these encodes run the exact f32 path -- the same "
                              "answer, ~20x slower on large batches (include/msae.h, msae_options::certified)", stacklevel=3)
    opts = _opts(coarse_mode, guard_z, status_detail, exact, dither, dither_seed, cert_ops)
    rows = _defaults.rows_rescored
    if rows is not None and (T > rows.numel() or rows.device != dev):
        # rescore_rows(buf) serves encodes of <= buf.numel() tokens on buf's device; a larger call inside the block runs
        # WITHOUT the statistics instead of writing past the buffer
        with _without_rows():
            opts = _opts(coarse_mode, guard_z, status_detail, exact, dither, dither_seed, cert_ops)
    ws = _workspace(dev, _encode_ws_bytes(lib, T, d, N, k, opts))
    with torch.cuda.device(dev):
        _hip.check(lib.msae_encode_topk_i64(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(W),
                                            _hip.ptr(be), _hip.ptr(bd), _hip.ptr(prepared), T, d, N, k,
                                            set_feature, set_value, zero_feature, _hip.ptr(vals),
                                            _hip.ptr(idx), _hip.ptr(status), _hip.ptr(ws), ws.numel(),
                                            opts.ref(), _hip.stream_of(xa)), "msae_encode_topk_i64")
    return vals, idx, status


@encode_topk.register_fake
def _(x, W_enc, b_enc, b_dec, prepared, k, set_feature=-1, set_value=0.0, zero_feature=-1, coarse_mode=-1,
      guard_z=0.0, status_detail=False, exact=False, dither=0, dither_seed=0, certified=False):
    return (x.new_empty(*x.shape[:-1], k, dtype=torch.float32),
            x.new_empty(*x.shape[:-1], k, dtype=torch.int64),
            x.new_empty(x.shape[:-1], dtype=torch.int32))


# ---- set-valued hook edits on the top-k list (csrc/edit_topk.hip) ------------------------------------
EDIT_TOPK_MAX_SELECTED = 4096       # k + E: msae_encode_topk's own limit on k


@torch.library.custom_op("msae::edit_topk", mutates_args=())
def _edit_topk(vals_in: Tensor, idx_in: Tensor, edit_feat: Tensor, edit_val: Tensor, edit_kind: Tensor,
               num_latents: int, k: int) -> Tuple[Tensor, Tensor]:
    dev = _hip.require_device(vals_in, idx_in, edit_feat, edit_val, edit_kind)
    lib = _hip.load()
    assert vals_in.shape == idx_in.shape and vals_in.dim() >= 1, \
        f"vals_in and idx_in must share a shape [..., kk], got {tuple(vals_in.shape)} and {tuple(idx_in.shape)}"
    assert idx_in.dtype in (torch.int32, torch.int64), f"idx_in must be int32 or int64, got {idx_in.dtype}"
    E, kk = edit_feat.numel(), vals_in.shape[-1]
    assert edit_val.numel() == E and edit_kind.numel() == E, "the edit table's three arrays must have one length"
    v_in = _f32c(vals_in)
    i_in = idx_in.detach().contiguous()
    ef = edit_feat.detach().to(torch.int32).contiguous()
    ev = _f32c(edit_val)
    ek = edit_kind.detach().to(torch.int32).contiguous()
    T = v_in.numel() // max(kk, 1)
    vals = torch.empty(*v_in.shape[:-1], k, dtype=torch.float32, device=dev)
    idx = torch.empty(*v_in.shape[:-1], k, dtype=i_in.dtype, device=dev)
    wide = i_in.dtype == torch.int64
    fn, name = (lib.msae_edit_topk_i64_f32, "msae_edit_topk_i64_f32") if wide else (lib.msae_edit_topk_f32, "msae_edit_topk_f32")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(v_in), _hip.ptr(i_in), T, kk, _hip.ptr(ef), _hip.ptr(ev), _hip.ptr(ek), E, num_latents, k,
                      _hip.ptr(vals), _hip.ptr(idx), _hip.stream_of(v_in)), name)
    return vals, idx


@_edit_topk.register_fake
def _(vals_in, idx_in, edit_feat, edit_val, edit_kind, num_latents, k):
    return (vals_in.new_empty(*vals_in.shape[:-1], k, dtype=torch.float32),
            idx_in.new_empty(*idx_in.shape[:-1], k))


def edit_topk(vals_in: Tensor, idx_in: Tensor, edit_feat: Tensor, edit_val: Tensor, edit_kind: Tensor, num_latents: int,
              k: int, *, cur: Optional[Tensor] = None, col: Optional[Tensor] = None, want_gain: bool = False):
    """The canonical top-k of the EDITED latents from an unedited top-kk list -> (vals f32 [..., k], idx [..., k] in
    idx_in's dtype, int32 or int64).  vals_in / idx_in [..., kk]: encode_topk's output for kk >= k + E without edits;
    edit_feat int [E] strictly ascending in [0, num_latents), edit_val f32 [E], edit_kind int [E] (0 set, 1 zero) -- the
    arrays of a msae.features.FeatureEdits.  Exact: include/msae.h, "set-valued hook edits".  Nothing is read back; the
    arguments the library would refuse (kk < k + E, k + E > num_latents, k + E > 4096, E < 1) raise ValueError here.
    cur (f32 [..., C]: the edited features' exact latents, `pre_acts_features` over edit_feat) selects the VALUED form
    (include/msae.h, "value-dependent edits"): kinds 2 scale, 3 add, 4 floor, 5 cap read column col[e] (int32 [E]; None:
    column e) of their token's row; want_gain=True appends gain f32 [..., k], the factor of each slot's gradient.  CPU
    tensors take a plain-torch host path in the valued form."""
    E, kk = edit_feat.numel(), vals_in.shape[-1]
    if E < 1 or k < 1 or kk < k + E or k + E > num_latents or k + E > EDIT_TOPK_MAX_SELECTED:
        raise ValueError(f"edit_topk: need E >= 1, k >= 1, kk >= k + E and k + E <= min(num_latents, {EDIT_TOPK_MAX_SELECTED}); "
                         f"got kk = {kk}, k = {k}, E = {E}, num_latents = {num_latents}")
    _no_grad_inputs("ops.edit_topk", vals_in, edit_val)
    if cur is None:
        if col is not None or want_gain:
            raise ValueError("edit_topk: col= and want_gain= belong to the valued form: pass cur= as well")
        return _edit_topk(vals_in, idx_in, edit_feat, edit_val, edit_kind, num_latents, k)
    _check_cur("edit_topk", vals_in, idx_in, cur, col, E)
    _no_grad_inputs("ops.edit_topk", cur)
    if not vals_in.is_cuda:
        lead = vals_in.shape[:-1]
        cols = torch.arange(E) if col is None else col.long()
        v, i, g, _ = _edit_topk_valued_host(vals_in.reshape(-1, kk).float(), idx_in.reshape(-1, kk), edit_feat, edit_val,
                                            edit_kind, cur.reshape(-1, cur.shape[-1]).float(), cols, k)
        vals, idx, gain = v.reshape(*lead, k), i.reshape(*lead, k), g.reshape(*lead, k)
    else:
        vals, idx, gain = _edit_topk_valued(vals_in, idx_in, edit_feat, edit_val, edit_kind, cur, col, num_latents, k,
                                            want_gain)
    return (vals, idx, gain) if want_gain else (vals, idx)


# ---- value-dependent edits: scale, add, floor, cap (msae_edit_topk_valued_*) ---------------------------
def _check_cur(what: str, vals_in: Tensor, idx_in: Tensor, cur, col, n_entries: int) -> None:
    if vals_in.shape != idx_in.shape:
        raise ValueError(f"{what}: vals_in {tuple(vals_in.shape)} and idx_in {tuple(idx_in.shape)} must share a shape")
    if idx_in.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: idx_in must be int32 or int64, got {idx_in.dtype}")
    if not isinstance(cur, Tensor) or cur.dtype != torch.float32:
        raise ValueError(f"{what}: cur must be a float32 tensor (ops.pre_acts_features' output)")
    if cur.dim() != vals_in.dim() or tuple(cur.shape[:-1]) != tuple(vals_in.shape[:-1]) or cur.shape[-1] < 1:
        raise ValueError(f"{what}: cur must have shape {tuple(vals_in.shape[:-1])} + (C,) with C >= 1, got {tuple(cur.shape)}")
    if cur.device != vals_in.device:
        raise ValueError(f"{what}: cur lives on {cur.device}, the list on {vals_in.device}")
    if col is not None and (not isinstance(col, Tensor) or col.dtype not in (torch.int32, torch.int64) or
                            col.numel() != n_entries):
        raise ValueError(f"{what}: col must be an int32 or int64 tensor with one column per table entry ({n_entries})")


def _cur_rows(cur: Tensor) -> Tuple[Tensor, int]:
    """cur [..., C] -> (a [T, C] tensor the kernels can read, its row stride): the column-sliced view that
    pre_acts_features returns is passed as it is, anything else is copied."""
    C = cur.shape[-1]
    c2 = cur.detach()
    try:
        c2 = c2.view(-1, C)
    except RuntimeError:
        c2 = c2.reshape(-1, C).contiguous()
    T = c2.shape[0]
    ld = c2.stride(0) if T > 1 else C
    room = c2.untyped_storage().nbytes() // 4 - c2.storage_offset()
    if c2.stride(1) != 1 or ld < C or T * ld > room:
        c2, ld = c2.contiguous(), C
    return c2, ld


def _edit_topk_valued_host(v_in: Tensor, i_in: Tensor, feat: Tensor, val: Tensor, kind: Tensor, cur: Tensor, cols: Tensor,
                           k: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The valued list edit of ONE table in plain torch: v_in / i_in [T, kk], feat / val / kind [E], cur [T, C], cols int64
    [E] -> (vals [T, k], idx [T, k], gain [T, k], edited bool [T, k]).  The same candidate set as the kernel -- the first
    k + E entries minus the edited features', plus one entry per table row -- ordered by three stable sorts (index
    ascending, value descending with -0 folded onto +0, dropped entries last)."""
    T, E, C = v_in.shape[0], feat.numel(), cur.shape[1]
    feat, kind, val = feat.long(), kind.long(), val.float()
    c = cur[:, cols.clamp(0, C - 1)]                                        # [T, E]
    v = val[None].expand(T, E)
    new = torch.where(kind == 1, torch.zeros_like(c), v)                    # ZERO, and SET for every other kind ...
    new = torch.where(kind == 2, c * v, new)
    new = torch.where(kind == 3, c + v, new)
    new = torch.where(kind == 4, torch.maximum(c, v), new)
    new = torch.where(kind == 5, torch.minimum(c, v), new)
    on = c > 0
    one, zero = torch.ones_like(c), torch.zeros_like(c)
    gain = torch.where(kind == 2, torch.where(on, v, zero), zero)
    gain = torch.where(kind == 3, torch.where(on, one, zero), gain)
    gain = torch.where(kind == 4, torch.where(on & (c >= v), one, zero), gain)
    gain = torch.where(kind == 5, torch.where(on & (c <= v), one, zero), gain)
    L = k + E
    lv, li = v_in[:, :L], i_in[:, :L].long()
    dropped = torch.isin(li, feat)
    cand_v = torch.cat([lv, new], 1)
    cand_v = torch.where(cand_v == 0, torch.zeros_like(cand_v), cand_v)     # the rank key folds -0 onto +0
    cand_i = torch.cat([li, feat[None].expand(T, E)], 1)
    cand_g = torch.cat([torch.ones_like(lv), gain], 1)
    cand_e = torch.cat([torch.zeros_like(dropped), torch.ones(T, E, dtype=torch.bool)], 1)
    cand_d = torch.cat([dropped, torch.zeros(T, E, dtype=torch.bool)], 1)
    order = torch.sort(cand_i, dim=1, stable=True).indices
    order = order.gather(1, torch.sort(cand_v.gather(1, order), dim=1, descending=True, stable=True).indices)
    order = order.gather(1, torch.sort(cand_d.gather(1, order).to(torch.uint8), dim=1, stable=True).indices)[:, :k]
    return (cand_v.gather(1, order), cand_i.gather(1, order).to(i_in.dtype), cand_g.gather(1, order),
            cand_e.gather(1, order))


@torch.library.custom_op("msae::edit_topk_valued", mutates_args=())
def _edit_topk_valued(vals_in: Tensor, idx_in: Tensor, edit_feat: Tensor, edit_val: Tensor, edit_kind: Tensor, cur: Tensor,
                      col: Optional[Tensor], num_latents: int, k: int, want_gain: bool) -> Tuple[Tensor, Tensor, Tensor]:
    dev = _hip.require_device(vals_in, idx_in, edit_feat, edit_val, edit_kind, cur, col)
    lib = _hip.load()
    E, kk = edit_feat.numel(), vals_in.shape[-1]
    assert edit_val.numel() == E and edit_kind.numel() == E, "the edit table's three arrays must have one length"
    v_in = _f32c(vals_in)
    i_in = idx_in.detach().contiguous()
    ef = edit_feat.detach().to(torch.int32).contiguous()
    ev = _f32c(edit_val)
    ek = edit_kind.detach().to(torch.int32).contiguous()
    ec = None if col is None else col.detach().to(torch.int32).contiguous()
    T = v_in.numel() // max(kk, 1)
    c2, ld = _cur_rows(cur)
    assert c2.shape[0] == T, f"cur must hold one row per token ({T}), got {tuple(cur.shape)}"
    vals = torch.empty(*v_in.shape[:-1], k, dtype=torch.float32, device=dev)
    idx = torch.empty(*v_in.shape[:-1], k, dtype=i_in.dtype, device=dev)
    gain = torch.empty(*v_in.shape[:-1], k if want_gain else 0, dtype=torch.float32, device=dev)
    wide = i_in.dtype == torch.int64
    fn, name = (lib.msae_edit_topk_valued_i64_f32, "msae_edit_topk_valued_i64_f32") if wide else \
        (lib.msae_edit_topk_valued_f32, "msae_edit_topk_valued_f32")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(v_in), _hip.ptr(i_in), T, kk, _hip.ptr(ef), _hip.ptr(ev), _hip.ptr(ek), E, num_latents, k,
                      _hip.ptr(c2), ld, _hip.ptr(ec), _hip.ptr(vals), _hip.ptr(idx),
                      _hip.ptr(gain) if want_gain else None, _hip.stream_of(v_in)), name)
    return vals, idx, gain


@_edit_topk_valued.register_fake
def _(vals_in, idx_in, edit_feat, edit_val, edit_kind, cur, col, num_latents, k, want_gain):
    return (vals_in.new_empty(*vals_in.shape[:-1], k, dtype=torch.float32),
            idx_in.new_empty(*idx_in.shape[:-1], k),
            vals_in.new_empty(*vals_in.shape[:-1], k if want_gain else 0, dtype=torch.float32))


# ---- the same with one edit table per token (msae_edit_topk_rows_*) ------------------------------------
def _group_ids(group_of: Tensor, G: int) -> Tensor:
    """The tokens' group ids as the contiguous int32 the kernels read."""
    go = group_of.detach()
    if go.dtype != torch.int32:         # an id beyond int32 must stay outside [0, G): clamp on the device, then narrow
        go = go.clamp(-1, G).to(torch.int32)
    return go.contiguous()


@torch.library.custom_op("msae::edit_topk_rows", mutates_args=())
def _edit_topk_rows(vals_in: Tensor, idx_in: Tensor, group_of: Tensor, group_off: Tensor, edit_feat: Tensor,
                    edit_val: Tensor, edit_kind: Tensor, e_max: int, num_latents: int, k: int,
                    want_mask: bool) -> Tuple[Tensor, Tensor, Tensor]:
    dev = _hip.require_device(vals_in, idx_in, group_of, group_off, edit_feat, edit_val, edit_kind)
    lib = _hip.load()
    assert vals_in.shape == idx_in.shape and vals_in.dim() >= 1, \
        f"vals_in and idx_in must share a shape [..., kk], got {tuple(vals_in.shape)} and {tuple(idx_in.shape)}"
    assert idx_in.dtype in (torch.int32, torch.int64), f"idx_in must be int32 or int64, got {idx_in.dtype}"
    E_total, kk, G = edit_feat.numel(), vals_in.shape[-1], group_off.numel() - 1
    assert edit_val.numel() == E_total and edit_kind.numel() == E_total, "the edit table's three arrays must have one length"
    v_in = _f32c(vals_in)
    i_in = idx_in.detach().contiguous()
    T = v_in.numel() // max(kk, 1)
    assert group_of.numel() == T, f"group_of must hold one id per token ({T}), got {tuple(group_of.shape)}"
    go = _group_ids(group_of, G)
    gf = group_off.detach().to(torch.int32).contiguous()
    ef = edit_feat.detach().to(torch.int32).contiguous()
    ev = _f32c(edit_val)
    ek = edit_kind.detach().to(torch.int32).contiguous()
    vals = torch.empty(*v_in.shape[:-1], k, dtype=torch.float32, device=dev)
    idx = torch.empty(*v_in.shape[:-1], k, dtype=i_in.dtype, device=dev)
    edited = torch.empty(*v_in.shape[:-1], k if want_mask else 0, dtype=torch.uint8, device=dev)
    wide = i_in.dtype == torch.int64
    fn, name = (lib.msae_edit_topk_rows_i64_f32, "msae_edit_topk_rows_i64_f32") if wide else \
        (lib.msae_edit_topk_rows_f32, "msae_edit_topk_rows_f32")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(v_in), _hip.ptr(i_in), T, kk, _hip.ptr(go), _hip.ptr(gf), G, _hip.ptr(ef), _hip.ptr(ev),
                      _hip.ptr(ek), E_total, e_max, num_latents, k, _hip.ptr(vals), _hip.ptr(idx),
                      _hip.ptr(edited) if want_mask else None, _hip.stream_of(v_in)), name)
    return vals, idx, edited


@_edit_topk_rows.register_fake
def _(vals_in, idx_in, group_of, group_off, edit_feat, edit_val, edit_kind, e_max, num_latents, k, want_mask):
    return (vals_in.new_empty(*vals_in.shape[:-1], k, dtype=torch.float32),
            idx_in.new_empty(*idx_in.shape[:-1], k),
            vals_in.new_empty(*vals_in.shape[:-1], k if want_mask else 0, dtype=torch.uint8))


@torch.library.custom_op("msae::edit_topk_rows_valued", mutates_args=())
def _edit_topk_rows_valued(vals_in: Tensor, idx_in: Tensor, group_of: Tensor, group_off: Tensor, edit_feat: Tensor,
                           edit_val: Tensor, edit_kind: Tensor, cur: Tensor, col: Optional[Tensor], e_max: int,
                           num_latents: int, k: int, want_mask: bool,
                           want_gain: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    dev = _hip.require_device(vals_in, idx_in, group_of, group_off, edit_feat, edit_val, edit_kind, cur, col)
    lib = _hip.load()
    E_total, kk, G = edit_feat.numel(), vals_in.shape[-1], group_off.numel() - 1
    assert edit_val.numel() == E_total and edit_kind.numel() == E_total, "the edit table's three arrays must have one length"
    v_in = _f32c(vals_in)
    i_in = idx_in.detach().contiguous()
    T = v_in.numel() // max(kk, 1)
    assert group_of.numel() == T, f"group_of must hold one id per token ({T}), got {tuple(group_of.shape)}"
    go = _group_ids(group_of, G)
    gf = group_off.detach().to(torch.int32).contiguous()
    ef = edit_feat.detach().to(torch.int32).contiguous()
    ev = _f32c(edit_val)
    ek = edit_kind.detach().to(torch.int32).contiguous()
    ec = None if col is None else col.detach().to(torch.int32).contiguous()
    c2, ld = _cur_rows(cur)
    assert c2.shape[0] == T, f"cur must hold one row per token ({T}), got {tuple(cur.shape)}"
    vals = torch.empty(*v_in.shape[:-1], k, dtype=torch.float32, device=dev)
    idx = torch.empty(*v_in.shape[:-1], k, dtype=i_in.dtype, device=dev)
    edited = torch.empty(*v_in.shape[:-1], k if want_mask else 0, dtype=torch.uint8, device=dev)
    gain = torch.empty(*v_in.shape[:-1], k if want_gain else 0, dtype=torch.float32, device=dev)
    wide = i_in.dtype == torch.int64
    fn, name = (lib.msae_edit_topk_rows_valued_i64_f32, "msae_edit_topk_rows_valued_i64_f32") if wide else \
        (lib.msae_edit_topk_rows_valued_f32, "msae_edit_topk_rows_valued_f32")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(v_in), _hip.ptr(i_in), T, kk, _hip.ptr(go), _hip.ptr(gf), G, _hip.ptr(ef), _hip.ptr(ev),
                      _hip.ptr(ek), E_total, e_max, num_latents, k, _hip.ptr(c2), ld, _hip.ptr(ec), _hip.ptr(vals),
                      _hip.ptr(idx), _hip.ptr(edited) if want_mask else None, _hip.ptr(gain) if want_gain else None,
                      _hip.stream_of(v_in)), name)
    return vals, idx, edited, gain


@_edit_topk_rows_valued.register_fake
def _(vals_in, idx_in, group_of, group_off, edit_feat, edit_val, edit_kind, cur, col, e_max, num_latents, k, want_mask,
      want_gain):
    return (vals_in.new_empty(*vals_in.shape[:-1], k, dtype=torch.float32),
            idx_in.new_empty(*idx_in.shape[:-1], k),
            vals_in.new_empty(*vals_in.shape[:-1], k if want_mask else 0, dtype=torch.uint8),
            vals_in.new_empty(*vals_in.shape[:-1], k if want_gain else 0, dtype=torch.float32))


def _edit_topk_rows_valued_host(v_in: Tensor, i_in: Tensor, group_of: Tensor, row_edits, cur: Tensor, cols: Tensor, k: int):
    """The valued per-token edit in plain torch: every group's tokens through `_edit_topk_valued_host` with that group's
    slice; the others copy their first k entries (gain 1, edited 0).  v_in / i_in [T, kk], group_of [T], cols int64
    [E_total]."""
    T = v_in.shape[0]
    vals, idx = v_in[:, :k].clone(), i_in[:, :k].clone()
    gain, edited = torch.ones(T, k), torch.zeros(T, k, dtype=torch.uint8)
    off = row_edits.offsets.tolist()
    for g in range(len(off) - 1):
        a, b = off[g], off[g + 1]
        rows = torch.nonzero(group_of == g).flatten()
        if b <= a or rows.numel() == 0:
            continue
        v, i, gn, ed = _edit_topk_valued_host(v_in[rows], i_in[rows], row_edits.feat[a:b], row_edits.val[a:b],
                                              row_edits.kind[a:b], cur[rows], cols[a:b], k)
        vals[rows], idx[rows], gain[rows], edited[rows] = v, i, gn, ed.to(torch.uint8)
    return vals, idx, edited, gain


def edit_topk_rows(vals_in: Tensor, idx_in: Tensor, group_of: Tensor, row_edits, num_latents: int, k: int,
                   want_mask: bool = False, *, cur: Optional[Tensor] = None, col: Optional[Tensor] = None,
                   want_gain: bool = False):
    """`edit_topk` with one edit table PER TOKEN -> (vals f32 [..., k], idx [..., k] in idx_in's dtype[, edited uint8
    [..., k]]).  vals_in / idx_in [..., kk]: encode_topk's output for kk >= k + E_max without edits; group_of int32 / int64
    [...]: the group of every token, any id outside [0, G) = unedited (the first k entries are copied); row_edits: a
    msae.features.RowEdits (offsets [G + 1], feat / val / kind [E_total], E_max).  `edited` (want_mask=True): 1 where the slot
    came from an edit entry.  Exact per token: include/msae.h, "per-token edit tables".  Nothing is read back; the arguments
    the library would refuse raise ValueError here.  cur (f32 [..., C], `pre_acts_features` over row_edits.union) selects the
    VALUED form as in `edit_topk`: col int32 [E_total] (row_edits.col; None: entry e of the concatenated table reads column
    e), want_gain=True appends gain f32 [..., k] (1 on unedited tokens).  CPU tensors take a plain-torch host path in the
    valued form."""
    kk, e_max, G = vals_in.shape[-1], int(row_edits.E_max), int(row_edits.G)
    if G < 1 or e_max < 1 or k < 1 or kk < k + e_max or k + e_max > min(num_latents, EDIT_TOPK_MAX_SELECTED):
        raise ValueError(f"edit_topk_rows: need G >= 1, E_max >= 1, k >= 1, kk >= k + E_max and k + E_max <= min(num_latents, "
                         f"{EDIT_TOPK_MAX_SELECTED}); got kk = {kk}, k = {k}, E_max = {e_max}, G = {G}, "
                         f"num_latents = {num_latents}")
    if vals_in.shape != idx_in.shape:
        raise ValueError(f"edit_topk_rows: vals_in {tuple(vals_in.shape)} and idx_in {tuple(idx_in.shape)} must share a shape")
    if idx_in.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"edit_topk_rows: idx_in must be int32 or int64, got {idx_in.dtype}")
    if not isinstance(group_of, Tensor) or group_of.dtype not in (torch.int32, torch.int64):
        raise ValueError("edit_topk_rows: group_of must be an int32 or int64 tensor")
    if tuple(group_of.shape) != tuple(vals_in.shape[:-1]):
        raise ValueError(f"edit_topk_rows: group_of must have one id per token, shape {tuple(vals_in.shape[:-1])}, got "
                         f"{tuple(group_of.shape)}")
    _no_grad_inputs("ops.edit_topk_rows", vals_in, row_edits.val)
    if cur is None:
        if col is not None or want_gain:
            raise ValueError("edit_topk_rows: col= and want_gain= belong to the valued form: pass cur= as well")
        vals, idx, edited = _edit_topk_rows(vals_in, idx_in, group_of, row_edits.offsets, row_edits.feat, row_edits.val,
                                            row_edits.kind, e_max, num_latents, k, want_mask)
        return (vals, idx, edited) if want_mask else (vals, idx)
    _check_cur("edit_topk_rows", vals_in, idx_in, cur, col, int(row_edits.E_total))
    _no_grad_inputs("ops.edit_topk_rows", cur)
    if not vals_in.is_cuda:
        lead = vals_in.shape[:-1]
        cols = torch.arange(int(row_edits.E_total)) if col is None else col.long()
        out = _edit_topk_rows_valued_host(vals_in.reshape(-1, kk).float(), idx_in.reshape(-1, kk), group_of.reshape(-1),
                                          row_edits, cur.reshape(-1, cur.shape[-1]).float(), cols, k)
        vals, idx, edited, gain = (o.reshape(*lead, k) for o in out)
    else:
        vals, idx, edited, gain = _edit_topk_rows_valued(vals_in, idx_in, group_of, row_edits.offsets, row_edits.feat,
                                                         row_edits.val, row_edits.kind, cur, col, e_max, num_latents, k,
                                                         want_mask, want_gain)
    return (vals, idx) + ((edited,) if want_mask else ()) + ((gain,) if want_gain else ())


# ---- error-preserving interventions (csrc/delta_decode.hip) -------------------------------------------
DELTA_DECODE_MAX_K = 4096           # the encoder's own limit on k + E


def _list_rows(vals: Tensor, idx: Tensor, k: int) -> Tuple[Tensor, Tensor, int]:
    """A top-k list [..., k] -> (vals f32, idx, leading dimension) the kernel reads in place: a 2-d view with unit column
    stride (the first k columns of an over-fetched [T, kk] output) is passed with its row stride, anything else contiguous."""
    v, i = vals.detach(), idx.detach()
    if v.dtype != torch.float32:
        v = v.to(torch.float32)
    T = v.numel() // k
    if (v.dim() == 2 and i.dim() == 2 and v.stride(1) == 1 and i.stride(1) == 1 and v.stride(0) == i.stride(0) and
            (T == 1 or v.stride(0) >= k)):
        return v, i, max(int(v.stride(0)), k)
    return v.contiguous(), i.contiguous(), k


def _delta_decode_into(x: Tensor, plain_acts: Tensor, plain_idx: Tensor, edit_acts: Tensor, edit_idx: Tensor, W_dec: Tensor,
                       out: Tensor) -> None:
    dev = _hip.require_device(x, plain_acts, plain_idx, edit_acts, edit_idx, W_dec, out)
    lib = _hip.load()
    W = _f32c(W_dec)
    N, d = W.shape
    k = plain_acts.shape[-1]
    T = x.numel() // d
    if T == 0:
        return
    pv, pi, ld_p = _list_rows(plain_acts, plain_idx, k)
    qv, qi, ld_q = _list_rows(edit_acts, edit_idx, k)
    wide = pi.dtype == torch.int64
    fn, name = (lib.msae_delta_decode_i64_f32, "msae_delta_decode_i64_f32") if wide else \
        (lib.msae_delta_decode_f32, "msae_delta_decode_f32")
    flag = _bounds_flag(dev)
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(x), _hip.DTYPE_CODE[x.dtype], _hip.ptr(pv), _hip.ptr(pi), ld_p, _hip.ptr(qv), _hip.ptr(qi), ld_q,
                      _hip.ptr(W), T, k, N, d, _hip.ptr(out), _hip.ptr(flag), _hip.stream_of(x)), name)
    _check_bounds(flag, name)


@torch.library.custom_op("msae::delta_decode", mutates_args=())
def _delta_decode(x: Tensor, plain_acts: Tensor, plain_idx: Tensor, edit_acts: Tensor, edit_idx: Tensor,
                  W_dec: Tensor) -> Tensor:
    xa = x.detach().contiguous()
    out = torch.empty_like(xa)
    _delta_decode_into(xa, plain_acts, plain_idx, edit_acts, edit_idx, W_dec, out)
    return out


@_delta_decode.register_fake
def _(x, plain_acts, plain_idx, edit_acts, edit_idx, W_dec):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("msae::delta_decode_out", mutates_args=("out",))
def _delta_decode_out(x: Tensor, plain_acts: Tensor, plain_idx: Tensor, edit_acts: Tensor, edit_idx: Tensor,
                      W_dec: Tensor, out: Tensor) -> None:
    _delta_decode_into(x.detach(), plain_acts, plain_idx, edit_acts, edit_idx, W_dec, out)


@_delta_decode_out.register_fake
def _(x, plain_acts, plain_idx, edit_acts, edit_idx, W_dec, out):
    return None


def delta_decode(x: Tensor, plain_acts: Tensor, plain_idx: Tensor, edit_acts: Tensor, edit_idx: Tensor, W_dec: Tensor,
                 out: Optional[Tensor] = None) -> Tensor:
    """x + (decode(edited list) - decode(plain list)) in x's dtype, gathering only the entries in which the two lists
    differ (include/msae.h, "error-preserving interventions"): a token whose lists agree keeps x's own bits.
    x [..., d] f32 / bf16 / f16; plain_acts / plain_idx and edit_acts / edit_idx [..., k] with x's leading shape (or [T, k]),
    idx int32 or int64 (one type for both lists); the plain list may be the non-contiguous `[:, :k]` view of an over-fetched
    [T, kk] encode -- it is read in place.  W_dec [N, d].  `out`: a contiguous tensor of x's shape and dtype, or x itself
    (in place: untouched tokens are not even written).  Nothing is read back; bad arguments raise ValueError before any
    device work."""
    if x.dim() < 1 or W_dec.dim() != 2 or x.shape[-1] != W_dec.shape[1]:
        raise ValueError(f"delta_decode: x [..., d] and W_dec [N, d] must share d, got {tuple(x.shape)} and {tuple(W_dec.shape)}")
    if x.dtype not in _hip.DTYPE_CODE:
        raise ValueError(f"delta_decode: x must be float32, bfloat16 or float16, got {x.dtype}")
    if plain_acts.shape != plain_idx.shape or edit_acts.shape != edit_idx.shape or plain_acts.shape != edit_acts.shape \
            or plain_acts.dim() < 1:
        raise ValueError("delta_decode: the four list tensors must share one shape [..., k], got "
                         f"{tuple(plain_acts.shape)}, {tuple(plain_idx.shape)}, {tuple(edit_acts.shape)}, {tuple(edit_idx.shape)}")
    k = plain_acts.shape[-1]
    if not 1 <= k <= DELTA_DECODE_MAX_K:
        raise ValueError(f"delta_decode: k must be in [1, {DELTA_DECODE_MAX_K}], got {k}")
    T = x.numel() // max(x.shape[-1], 1)
    if x.shape[-1] < 1 or plain_acts.numel() != T * k or \
            (plain_acts.dim() != 2 and tuple(plain_acts.shape[:-1]) != tuple(x.shape[:-1])):
        raise ValueError(f"delta_decode: the lists must hold one row per token of x {tuple(x.shape)}, got "
                         f"{tuple(plain_acts.shape)}")
    if plain_idx.dtype != edit_idx.dtype or plain_idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"delta_decode: plain_idx and edit_idx must both be int32 or both int64, got {plain_idx.dtype} and "
                         f"{edit_idx.dtype}")
    if plain_acts.dtype != torch.float32 or edit_acts.dtype != torch.float32:
        raise ValueError(f"delta_decode: the lists' values must be float32, got {plain_acts.dtype} and {edit_acts.dtype}")
    if out is not None:
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise ValueError(f"delta_decode: out must be a contiguous {x.dtype} tensor of shape {tuple(x.shape)} on {x.device}")
        if not x.is_contiguous():       # (then out is not x: out is contiguous)
            x = x.contiguous()
    _no_grad_inputs("ops.delta_decode", x, plain_acts, edit_acts)
    if out is None:
        return _delta_decode(x, plain_acts, plain_idx, edit_acts, edit_idx, W_dec)
    _delta_decode_out(x, plain_acts, plain_idx, edit_acts, edit_idx, W_dec, out)
    return out


# ---- reconstruction error against sparsity (csrc/recon.hip) -------------------------------------------
RECON_MAX_K = 4096
RECON_MAX_CHECKPOINTS = 16


def _recon_curve_host(x: Tensor, vals: Tensor, idx: Tensor, W_dec: Tensor, b_dec: Tensor, ks: Sequence[int]):
    """The meaning of msae_recon_curve_f32 in plain torch (f32 terms, float64 sums rounded to f32): not its bits."""
    W, b = W_dec.detach().to(torch.float32), b_dec.detach().to(torch.float32)
    N, d = W.shape
    k = vals.shape[-1]
    xf = x.detach().reshape(-1, d).to(torch.float32)
    v, i = vals.detach().reshape(-1, k).to(torch.float32), idx.detach().reshape(-1, k).to(torch.int64)
    ok = (i >= 0) & (i < N) & (v != 0)
    v, i = torch.where(ok, v, torch.zeros_like(v)), torch.where(ok, i, torch.zeros_like(i))
    mom = torch.empty(xf.shape[0], len(ks), 3, dtype=torch.float32, device=xf.device)
    for c, kc in enumerate(ks):
        rows = torch.where(ok[:, :kc, None], v[:, :kc, None] * W[i[:, :kc]], torch.zeros((), dtype=torch.float32, device=W.device))
        r = rows.sum(1) + b
        e = r - xf
        for m, term in enumerate((e * e, xf * r, r * r)):
            mom[:, c, m] = term.sum(-1, dtype=torch.float64).to(torch.float32)
    return mom, (xf * xf).sum(-1, dtype=torch.float64).to(torch.float32)


@torch.library.custom_op("msae::recon_curve", mutates_args=())
def _recon_curve(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor,
                 ks: Sequence[int]) -> Tuple[Tensor, Tensor]:
    d = W_dec.shape[1]
    T = x.numel() // d
    C = len(ks)
    if not x.is_cuda:
        return _recon_curve_host(x, top_acts, top_indices, W_dec, b_dec, ks)
    dev = _hip.require_device(x, top_acts, top_indices, W_dec, b_dec)
    lib = _hip.load()
    xa, W, bd = x.detach().contiguous(), _f32c(W_dec), _f32c(b_dec)
    N = W.shape[0]
    k = top_acts.shape[-1]
    mom = torch.empty(T, C, 3, dtype=torch.float32, device=dev)
    xx = torch.empty(T, dtype=torch.float32, device=dev)
    if T == 0:
        return mom, xx
    v, i, ld = _list_rows(top_acts, top_indices, k)
    wide = i.dtype == torch.int64
    fn, name = (lib.msae_recon_curve_i64_f32, "msae_recon_curve_i64_f32") if wide else \
        (lib.msae_recon_curve_f32, "msae_recon_curve_f32")
    ks_host = (ctypes.c_int32 * C)(*ks)             # read during the call: copied into the launch arguments
    flag = _bounds_flag(dev)
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(v), _hip.ptr(i), ld, _hip.ptr(W), _hip.ptr(bd), T, k, N,
                      d, ks_host, C, _hip.ptr(mom), _hip.ptr(xx), _hip.ptr(flag), _hip.stream_of(xa)), name)
    _check_bounds(flag, name)
    return mom, xx


@_recon_curve.register_fake
def _(x, top_acts, top_indices, W_dec, b_dec, ks):
    T = x.numel() // W_dec.shape[1]
    return x.new_empty((T, len(ks), 3), dtype=torch.float32), x.new_empty((T,), dtype=torch.float32)


def recon_ks(ks, k: int, what: str = "recon_curve") -> list:
    """The checkpoint list as validated Python ints: strictly ascending, inside [0, k], 1 to 16 of them."""
    if isinstance(ks, Tensor):
        ks = ks.detach().cpu().reshape(-1).tolist()
    try:
        out = [int(c) for c in ks]
        same = all(float(c) == float(o) for c, o in zip(ks, out))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: ks must be a sequence of integers, got {ks!r}") from None
    if not same:
        raise ValueError(f"{what}: ks must be integers, got {list(ks)!r}")
    if not 1 <= len(out) <= RECON_MAX_CHECKPOINTS:
        raise ValueError(f"{what}: between 1 and {RECON_MAX_CHECKPOINTS} checkpoints, got {len(out)}")
    if out[0] < 0 or out[-1] > k or any(a >= b for a, b in zip(out, out[1:])):
        raise ValueError(f"{what}: ks must be strictly ascending inside [0, {k}], got {out}")
    return out


def recon_curve(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor, ks) -> Tuple[Tensor, Tensor]:
    """Reconstruction error at several sparsities in one pass (include/msae.h, "reconstruction error against sparsity"):
    -> (mom [..., C, 3] f32, xx [...] f32) with mom[..., c, :] = (|r - x|^2, x . r, |r|^2) of the reconstruction r from the
    first ks[c] entries of each token's list (+ b_dec) and xx = |x|^2.  x [..., d] f32 / bf16 / f16; top_acts / top_indices
    [..., k] with x's leading shape (or [T, k]), indices int32 or int64; the `[:, :k]` view of an over-fetched [T, kk] list
    is read in place.  W_dec [N, d], b_dec [d].  ks: strictly ascending integers in [0, k], at most 16.  On a HIP device
    the fused kernel (bit-defined per token); elsewhere a plain-torch composition with the same meaning, not the same
    bits.  Nothing is read back; bad arguments raise ValueError before any device work."""
    if x.dim() < 1 or W_dec.dim() != 2 or x.shape[-1] != W_dec.shape[1] or x.shape[-1] < 1:
        raise ValueError(f"recon_curve: x [..., d] and W_dec [N, d] must share d, got {tuple(x.shape)} and {tuple(W_dec.shape)}")
    if b_dec is None or b_dec.dim() != 1 or b_dec.shape[0] != W_dec.shape[1]:
        raise ValueError(f"recon_curve: b_dec must be [d] = [{W_dec.shape[1]}], got "
                         f"{None if b_dec is None else tuple(b_dec.shape)}")
    if x.dtype not in _hip.DTYPE_CODE:
        raise ValueError(f"recon_curve: x must be float32, bfloat16 or float16, got {x.dtype}")
    if top_acts.shape != top_indices.shape or top_acts.dim() < 1:
        raise ValueError(f"recon_curve: top_acts and top_indices must share one shape [..., k], got {tuple(top_acts.shape)} "
                         f"and {tuple(top_indices.shape)}")
    k = top_acts.shape[-1]
    if not 1 <= k <= RECON_MAX_K:
        raise ValueError(f"recon_curve: k must be in [1, {RECON_MAX_K}], got {k}")
    T = x.numel() // x.shape[-1]
    if top_acts.numel() != T * k or (top_acts.dim() != 2 and tuple(top_acts.shape[:-1]) != tuple(x.shape[:-1])):
        raise ValueError(f"recon_curve: the list must hold one row per token of x {tuple(x.shape)}, got {tuple(top_acts.shape)}")
    if top_indices.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"recon_curve: top_indices must be int32 or int64, got {top_indices.dtype}")
    if top_acts.dtype != torch.float32:
        raise ValueError(f"recon_curve: the list's values must be float32, got {top_acts.dtype}")
    devs = {t.device for t in (x, top_acts, top_indices, W_dec, b_dec)}
    if len(devs) != 1:
        raise ValueError(f"recon_curve: all tensors must be on one device, got {sorted(str(d) for d in devs)}")
    ks = recon_ks(ks, k)
    _no_grad_inputs("ops.recon_curve", x, top_acts)
    mom, xx = _recon_curve(x, top_acts, top_indices, W_dec.detach(), b_dec.detach(), ks)      # (weights are constants here)
    lead = tuple(x.shape[:-1])
    return mom.view(*lead, len(ks), 3), xx.view(lead)


# ---- least-squares refit on the encoder's support (csrc/refit.hip) ------------------------------------
REFIT_MAX_S = 64


class RefitRaw(NamedTuple):
    """ops.support_refit's outputs (include/msae.h, "support refit"), all f32 but n_dependent (int32)."""
    coef: Tensor
    """The least-squares coefficients on the live support, [..., s]; 0 for a dead or dependent slot."""
    gain: Tensor
    """z_j^2, [..., s]: yy - gain[..., :kappa].sum(-1) is the optimal squared error of the top-kappa support."""
    err_fit: Tensor
    """|y - D^T coef|^2, [...]."""
    err_enc: Tensor
    """|y - D^T vals|^2, [...]: the encoder's own error on the same s slots."""
    yy: Tensor
    """|x - b_dec|^2, [...]."""
    n_dependent: Tensor
    """Live slots dropped as linearly dependent on the slots before them, [...] int32."""


def refit_tau(d: int, s: int) -> float:
    """The dependence threshold of msae_support_refit_f32, 2 gamma_{d+s} with u = 2^-24, rounded to f32 as the kernel's is."""
    nu = (d + s) * 2.0 ** -24
    return float(torch.tensor(2.0 * nu / (1.0 - nu), dtype=torch.float64).to(torch.float32))


def _support_refit_host(x: Tensor, vals: Tensor, idx: Tensor, W_dec: Tensor, b_dec: Tensor, s: int):
    """The meaning of msae_support_refit_f32 in float64 torch (the f32 inputs, the same support and dependence rule, float64
    arithmetic rounded to f32 at the end): not its bits."""
    W, b = W_dec.detach().to(torch.float64), b_dec.detach().to(torch.float32)
    N, d = W.shape
    k = vals.shape[-1]
    y = (x.detach().reshape(-1, d).to(torch.float32) - b).to(torch.float64)
    v, i = vals.detach().reshape(-1, k)[:, :s].to(torch.float64), idx.detach().reshape(-1, k)[:, :s].to(torch.int64)
    T = y.shape[0]
    live = (i >= 0) & (i < N) & (v != 0)
    v = torch.where(live, v, torch.zeros_like(v))
    D = W[torch.where(live, i, torch.zeros_like(i))] * live[..., None]          # [T, s, d], zero rows for dead slots
    G, h = D @ D.transpose(1, 2), (D @ y[..., None])[..., 0]
    tau = refit_tau(d, s)
    L = torch.zeros(T, s, s, dtype=torch.float64, device=y.device)
    z = torch.zeros(T, s, dtype=torch.float64, device=y.device)
    ok = torch.zeros(T, s, dtype=torch.bool, device=y.device)
    one = torch.ones((), dtype=torch.float64, device=y.device)
    for j in range(s):
        p = G[:, j, j] - L[:, j, :j].square().sum(-1)
        ok[:, j] = live[:, j] & (p > tau * G[:, j, j])
        r = torch.where(ok[:, j], p, one).sqrt()
        col = (G[:, j:, j] - (L[:, j:, :j] @ L[:, j, :j, None])[..., 0]) / r[:, None]
        L[:, j:, j] = torch.where(ok[:, j, None], col, torch.zeros_like(col))
        L[:, j, j] = r
        zj = (h[:, j] - (L[:, j, :j] * z[:, :j]).sum(-1)) / r
        z[:, j] = torch.where(ok[:, j], zj, torch.zeros_like(zj))
    c = torch.zeros_like(z)
    for j in range(s - 1, -1, -1):
        cj = (z[:, j] - (L[:, j + 1:, j] * c[:, j + 1:]).sum(-1)) / L[:, j, j]
        c[:, j] = torch.where(ok[:, j], cj, torch.zeros_like(cj))
    e_fit = y - (c[:, None, :] @ D)[:, 0]
    e_enc = y - (v[:, None, :] @ D)[:, 0]
    f32 = torch.float32
    return (c.to(f32), z.square().to(f32), e_fit.square().sum(-1).to(f32), e_enc.square().sum(-1).to(f32),
            y.square().sum(-1).to(f32), (live & ~ok).sum(-1).to(torch.int32))


@torch.library.custom_op("msae::support_refit", mutates_args=())
def _support_refit(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor,
                   s: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    d = W_dec.shape[1]
    T = x.numel() // d
    if not x.is_cuda:
        return _support_refit_host(x, top_acts, top_indices, W_dec, b_dec, s)
    dev = _hip.require_device(x, top_acts, top_indices, W_dec, b_dec)
    lib = _hip.load()
    xa, W, bd = x.detach().contiguous(), _f32c(W_dec), _f32c(b_dec)
    N = W.shape[0]
    coef, gain = (torch.empty(T, s, dtype=torch.float32, device=dev) for _ in range(2))
    err_fit, err_enc, yy = (torch.empty(T, dtype=torch.float32, device=dev) for _ in range(3))
    n_dep = torch.empty(T, dtype=torch.int32, device=dev)
    if T == 0:
        return coef, gain, err_fit, err_enc, yy, n_dep
    v, i, ld = _list_rows(top_acts, top_indices, top_acts.shape[-1])
    wide = i.dtype == torch.int64
    fn, name = (lib.msae_support_refit_i64_f32, "msae_support_refit_i64_f32") if wide else \
        (lib.msae_support_refit_f32, "msae_support_refit_f32")
    flag = _bounds_flag(dev)
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(v), _hip.ptr(i), ld, _hip.ptr(W), _hip.ptr(bd), T, s, N,
                      d, _hip.ptr(coef), _hip.ptr(gain), _hip.ptr(err_fit), _hip.ptr(err_enc), _hip.ptr(yy), _hip.ptr(n_dep),
                      _hip.ptr(flag), _hip.stream_of(xa)), name)
    _check_bounds(flag, name)
    return coef, gain, err_fit, err_enc, yy, n_dep


@_support_refit.register_fake
def _(x, top_acts, top_indices, W_dec, b_dec, s):
    T = x.numel() // W_dec.shape[1]
    f = lambda *shape: x.new_empty(shape, dtype=torch.float32)
    return f(T, s), f(T, s), f(T), f(T), f(T), x.new_empty((T,), dtype=torch.int32)


def support_refit(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor,
                  s: Optional[int] = None) -> RefitRaw:
    """Least-squares refit of each token's coefficients on the support its list chose (include/msae.h, "support refit"):
    min_c |(x - b_dec) - W_dec[idx[:s]]^T c|^2 per token, the optimal error at every prefix of the support (`gain`), and the
    refit's and the encoder's own squared errors measured directly.  x [..., d] f32 / bf16 / f16; top_acts / top_indices
    [..., k] with x's leading shape (or [T, k]), indices int32 or int64; W_dec [N, d], b_dec [d].  `s`: refit the first s
    slots (None: all k); 1 <= s <= min(k, 64) -- a longer list is refit on its first 64 slots by passing s=64, read in
    place.  On a HIP device the fused kernel (bit-defined per token); elsewhere a float64 torch composition with the same
    meaning, not the same bits.  Nothing is read back; bad arguments raise ValueError before any device work."""
    if x.dim() < 1 or W_dec.dim() != 2 or x.shape[-1] != W_dec.shape[1] or x.shape[-1] < 1:
        raise ValueError(f"support_refit: x [..., d] and W_dec [N, d] must share d, got {tuple(x.shape)} and {tuple(W_dec.shape)}")
    if b_dec is None or b_dec.dim() != 1 or b_dec.shape[0] != W_dec.shape[1]:
        raise ValueError(f"support_refit: b_dec must be [d] = [{W_dec.shape[1]}], got "
                         f"{None if b_dec is None else tuple(b_dec.shape)}")
    if x.dtype not in _hip.DTYPE_CODE:
        raise ValueError(f"support_refit: x must be float32, bfloat16 or float16, got {x.dtype}")
    if top_acts.shape != top_indices.shape or top_acts.dim() < 1 or top_acts.shape[-1] < 1:
        raise ValueError(f"support_refit: top_acts and top_indices must share one shape [..., k], got {tuple(top_acts.shape)} "
                         f"and {tuple(top_indices.shape)}")
    k = top_acts.shape[-1]
    if s is None:
        s = k
    if isinstance(s, bool) or not isinstance(s, int):
        raise ValueError(f"support_refit: s must be an integer, got {s!r}")
    if not 1 <= s <= min(k, REFIT_MAX_S):
        raise ValueError(f"support_refit: s must be in [1, min(k, {REFIT_MAX_S})] = [1, {min(k, REFIT_MAX_S)}], got {s} "
                         f"(a longer list is refit on its first {REFIT_MAX_S} slots with s={REFIT_MAX_S})")
    T = x.numel() // x.shape[-1]
    if top_acts.numel() != T * k or (top_acts.dim() != 2 and tuple(top_acts.shape[:-1]) != tuple(x.shape[:-1])):
        raise ValueError(f"support_refit: the list must hold one row per token of x {tuple(x.shape)}, got {tuple(top_acts.shape)}")
    if top_indices.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"support_refit: top_indices must be int32 or int64, got {top_indices.dtype}")
    if top_acts.dtype != torch.float32:
        raise ValueError(f"support_refit: the list's values must be float32, got {top_acts.dtype}")
    devs = {t.device for t in (x, top_acts, top_indices, W_dec, b_dec)}
    if len(devs) != 1:
        raise ValueError(f"support_refit: all tensors must be on one device, got {sorted(str(d) for d in devs)}")
    if W_dec.shape[1] > 1 << 22:
        raise ValueError(f"support_refit: d must be at most {1 << 22}, got {W_dec.shape[1]}")
    _no_grad_inputs("ops.support_refit", x, top_acts)
    coef, gain, err_fit, err_enc, yy, n_dep = _support_refit(x, top_acts, top_indices, W_dec.detach(), b_dec.detach(), s)
    lead = tuple(x.shape[:-1])
    return RefitRaw(coef.view(*lead, s), gain.view(*lead, s), err_fit.view(lead), err_enc.view(lead), yy.view(lead),
                    n_dep.view(lead))


def shard_candidates(x: Tensor, b_enc_shard: Optional[Tensor], b_dec: Optional[Tensor], prepared_shard: Tensor,
                     N_shard: int, k: int, row_offset: int, C: int, set_feature: int = -1,
                     zero_feature: int = -1) -> Tensor:
    """Feature-sharded group, sender side (msae_shard_candidates): -> records uint8 [T, record_bytes(C)]."""
    dev = _hip.require_device(x, b_enc_shard, b_dec, prepared_shard)
    lib = _hip.load()
    xa, be, bd = _act(x), _f32c(b_enc_shard), _f32c(b_dec)
    d = xa.shape[-1]
    T = xa.numel() // d
    stride = lib.msae_shard_record_bytes(C)
    recs = torch.empty(T, stride, dtype=torch.uint8, device=dev)
    if T == 0:
        return recs
    opts = _opts_for(T, dev)
    ws = _workspace(dev, _encode_ws_bytes(lib, T, d, N_shard, k, opts))
    with torch.cuda.device(dev):
        _hip.check(lib.msae_shard_candidates(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(be), _hip.ptr(bd),
                                             _hip.ptr(prepared_shard), T, d, N_shard, k, row_offset, C, set_feature,
                                             zero_feature, _hip.ptr(recs), _hip.ptr(ws), ws.numel(), opts.ref(),
                                             _hip.stream_of(xa)), "msae_shard_candidates")
    return recs


def rescore_candidates(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor], k: int,
                       records: Tensor, C: int, T_valid: Optional[int] = None, set_feature: int = -1,
                       set_value: float = 0.0, zero_feature: int = -1) -> Tuple[Tensor, Tensor, Tensor]:
    """Feature-sharded group, owner side (msae_rescore_candidates): records uint8 [G, T, record_bytes(C)] of
    this rank's T tokens -> (top_acts f32 [T, k], top_indices int64 [T, k] global ids, status int32 [T])."""
    dev = _hip.require_device(x, W_enc, b_enc, b_dec, records)
    lib = _hip.load()
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    T = xa.numel() // d
    G = records.shape[0]
    assert records.dtype == torch.uint8 and records.is_contiguous() and records.shape[1] == T, records.shape
    assert records.shape[2] == lib.msae_shard_record_bytes(C)
    T_valid = T if T_valid is None else T_valid
    vals = torch.zeros(T, k, dtype=torch.float32, device=dev) if T_valid < T else torch.empty(T, k, dtype=torch.float32, device=dev)
    idx = torch.zeros(T, k, dtype=torch.int64, device=dev) if T_valid < T else torch.empty(T, k, dtype=torch.int64, device=dev)
    status = torch.zeros(T, dtype=torch.int32, device=dev) if T_valid < T else torch.empty(T, dtype=torch.int32, device=dev)
    if T_valid == 0:
        return vals, idx, status
    ws = _workspace(dev, lib.msae_rescore_candidates_ws_bytes(T, d, N, k, G, C))
    with torch.cuda.device(dev):
        _hip.check(lib.msae_rescore_candidates(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(W), _hip.ptr(be),
                                               _hip.ptr(bd), T, T_valid, d, N, k, G, C, _hip.ptr(records), set_feature,
                                               set_value, zero_feature, _hip.ptr(vals), _hip.ptr(idx),
                                               _hip.ptr(status), _hip.ptr(ws), ws.numel(), _opts_for(T, dev).ref(),
                                               _hip.stream_of(xa)),
                   "msae_rescore_candidates")
    return vals, idx, status


# ---- decoder (differentiable, mirrors TritonDecoder: kernels.py:403-429) ---------------------------
def _idx32(top_indices: Tensor) -> Tensor:
    return top_indices.detach().to(torch.int32).contiguous()


def _decode_prefix_host(top_indices: Tensor, top_acts: Tensor, W_dec: Tensor, b_dec: Optional[Tensor], lengths: Tensor) -> Tensor:
    """The meaning of msae_decode_prefix_f32 in plain torch (not its bits): the slots behind a row's length count for nothing,
    whatever they hold."""
    C = top_acts.shape[-1]
    live = torch.arange(C, device=top_acts.device) < lengths.reshape(*top_acts.shape[:-1], 1).clamp(0, C)
    N = W_dec.shape[0]
    ok = live & (top_indices >= 0) & (top_indices < N)
    v = torch.where(ok, top_acts.detach().to(torch.float32), torch.zeros((), dtype=torch.float32, device=top_acts.device))
    i = torch.where(ok, top_indices, torch.zeros_like(top_indices)).long()
    out = (v[..., None] * W_dec.detach().to(torch.float32)[i]).sum(-2)
    return out if b_dec is None else out + b_dec.detach().to(torch.float32)


@torch.library.custom_op("msae::decode", mutates_args=())
def decode(top_indices: Tensor, top_acts: Tensor, W_dec: Tensor, b_dec: Optional[Tensor],
           lengths: Optional[Tensor] = None) -> Tensor:
    """sum_j top_acts[:, j] * W_dec[top_indices[:, j]] (+ b_dec);  W_dec is [N, d] row-major.  `lengths` (int32, one per row;
    clamped to [0, k]): only the first lengths[a] entries of row a are read -- msae_decode_prefix_f32, whose cost follows
    sum(lengths); on a filtered list (ops.list_filter / ops.batch_select) the same bits as without it.  With `lengths`, host
    tensors take a plain-torch path with the same meaning."""
    assert top_indices.shape == top_acts.shape, "indices / acts shape mismatch"  # kernels.py:193
    if lengths is not None and not top_acts.is_cuda:
        return _decode_prefix_host(top_indices, top_acts, W_dec, b_dec, lengths)
    dev = _hip.require_device(top_indices, top_acts, W_dec, b_dec, lengths)
    lib = _hip.load()
    acts, W, bd = _f32c(top_acts), _f32c(W_dec), _f32c(b_dec)
    pre = "msae_decode" if lengths is None else "msae_decode_prefix"
    if top_indices.dtype == torch.int64:      # Tensor.topk's index type: read as it is, no narrowing copy
        idx, name = top_indices.detach().contiguous(), pre + "_i64_f32"
    else:
        idx, name = _idx32(top_indices), pre + "_f32"
    fn = getattr(lib, name)
    N, d = W.shape
    k = idx.shape[-1]
    A = idx.numel() // k
    out = torch.empty(*idx.shape[:-1], d, dtype=torch.float32, device=dev)
    flag = _bounds_flag(dev)
    with torch.cuda.device(dev):
        if lengths is None:
            _hip.check(fn(_hip.ptr(idx), _hip.ptr(acts), _hip.ptr(W), _hip.ptr(bd), A, k, N, d, _hip.ptr(out),
                          _hip.ptr(flag), _hip.stream_of(acts)), "%s" % name)
        else:
            if lengths.numel() != A:
                raise ValueError(f"decode: lengths must hold one entry per row ({A}), got {tuple(lengths.shape)}")
            ln = lengths.detach().to(torch.int32).contiguous()
            _hip.check(fn(_hip.ptr(idx), _hip.ptr(acts), _hip.ptr(ln), _hip.ptr(W), _hip.ptr(bd), A, k, N, d, _hip.ptr(out),
                          _hip.ptr(flag), _hip.stream_of(acts)), "%s" % name)
    _check_bounds(flag, name)
    return out


@decode.register_fake
def _(top_indices, top_acts, W_dec, b_dec, lengths=None):
    return top_acts.new_empty(*top_acts.shape[:-1], W_dec.shape[1], dtype=torch.float32)


_WGRAD_COLLECT: Optional[dict] = None


@contextlib.contextmanager
def collect_wgrad_sumsq():
    """Weight-gradient kernels launched inside the block also write the squared norm of every gradient row (while it is in
    registers) and record it: {weight data_ptr: [calls, gradient data_ptr, row_sumsq f32 [N]]}.  The trainer's
    clip_grad_norm_ total (train/sae/sae/trainer.py:390) is then a 512-KB sum instead of another read of the 2 GiB
    gradient -- valid for a parameter whose .grad IS the one recorded tensor (exactly one call, no accumulation)."""
    global _WGRAD_COLLECT
    prev, _WGRAD_COLLECT = _WGRAD_COLLECT, {}
    try:
        yield _WGRAD_COLLECT
    finally:
        _WGRAD_COLLECT = prev


_WGRAD_ROWSUM: Optional[list] = None      # set by _SparseEncode.backward around its weight-gradient call


@torch.library.custom_op("msae::decode_bwd", mutates_args=())
def decode_bwd(top_indices: Tensor, top_acts: Tensor, W_dec: Tensor, grad_out: Tensor,
               need_acts: bool, need_w: bool) -> Tuple[Tensor, Tensor]:
    dev = _hip.require_device(top_indices, top_acts, W_dec, grad_out)
    lib = _hip.load()
    idx, acts, W, g = _idx32(top_indices), _f32c(top_acts), _f32c(W_dec), _f32c(grad_out)
    N, d = W.shape
    k = idx.shape[-1]
    A = idx.numel() // k
    g_acts = torch.empty_like(acts) if need_acts else acts.new_empty(0)
    g_w = torch.empty_like(W) if need_w else W.new_empty(0)   # the kernel writes every row
    flag = _bounds_flag(dev)
    with torch.cuda.device(dev):
        st = _hip.stream_of(g)
        if need_acts:
            _hip.check(lib.msae_decode_bwd_acts_f32(_hip.ptr(idx), _hip.ptr(g), _hip.ptr(W), A, k, N, d,
                                                    _hip.ptr(g_acts), _hip.ptr(flag), st), "msae_decode_bwd_acts_f32")
        if need_w:
            ws = _workspace(dev, lib.msae_decode_bwd_wdec_ws_bytes(A, k, N))
            rowsq = torch.empty(N, dtype=torch.float32, device=dev) if _WGRAD_COLLECT is not None else None
            rowsum = torch.empty(N, dtype=torch.float32, device=dev) if _WGRAD_ROWSUM is not None else None
            # the weight-gradient kernel works on whole f32x4 columns: a width that is no multiple of four runs zero-padded to
            # the next one (columns are independent fma chains, the zero columns add exactly 0 to the row's squared norm)
            d4 = (d + 3) // 4 * 4
            g4 = g if d4 == d else torch.nn.functional.pad(g.reshape(-1, d), (0, d4 - d))
            g_w4 = g_w if d4 == d else torch.empty(N, d4, dtype=torch.float32, device=dev)
            _hip.check(lib.msae_decode_bwd_wdec_f32(_hip.ptr(idx), _hip.ptr(acts), _hip.ptr(g4), A, k, N,
                                                    d4, _hip.ptr(g_w4), _hip.ptr(rowsq), _hip.ptr(rowsum), _hip.ptr(flag),
                                                    _hip.ptr(ws), ws.numel(), st),
                       "msae_decode_bwd_wdec_f32")
            if d4 != d:
                g_w.copy_(g_w4[:, :d])
            if rowsum is not None:
                _WGRAD_ROWSUM.append(rowsum)
            if rowsq is not None:
                ent = _WGRAD_COLLECT.setdefault(W_dec.data_ptr(), [0, 0, None])
                ent[0] += 1
                ent[1], ent[2] = g_w.data_ptr(), rowsq
    _check_bounds(flag, "msae_decode_bwd")
    return g_acts, g_w


@decode_bwd.register_fake
def _(top_indices, top_acts, W_dec, grad_out, need_acts, need_w):
    return (torch.empty_like(top_acts, dtype=torch.float32) if need_acts else top_acts.new_empty(0),
            torch.empty_like(W_dec, dtype=torch.float32) if need_w else W_dec.new_empty(0))


def _decode_setup(ctx, inputs, output):
    top_indices, top_acts, W_dec, b_dec, lengths = inputs
    if lengths is not None:
        # the slots behind a row's length were not read and may hold anything: the backward kernels (width C) get them as
        # activation 0 on feature 0, and their activation gradient is 0
        C = top_acts.shape[-1]
        live = torch.arange(C, device=top_acts.device) < lengths.reshape(*top_acts.shape[:-1], 1).clamp(0, C)
        top_acts = torch.where(live, top_acts.detach(), torch.zeros((), dtype=top_acts.dtype, device=top_acts.device))
        top_indices = torch.where(live, top_indices, torch.zeros_like(top_indices))
        ctx.live = live
    else:
        ctx.live = None
    ctx.save_for_backward(top_indices, top_acts, W_dec)
    ctx.has_bdec = b_dec is not None


def _decode_bwd_host(top_indices: Tensor, top_acts: Tensor, W_dec: Tensor, grad_out: Tensor, need_acts: bool, need_w: bool):
    """decode_bwd's meaning in plain torch, for the host path of decode(lengths=)."""
    i = top_indices.long()
    g_acts = (grad_out[..., None, :] * W_dec[i]).sum(-1) if need_acts else None
    g_w = None
    if need_w:
        g_w = torch.zeros_like(W_dec)
        g_w.index_add_(0, i.reshape(-1), (top_acts[..., None] * grad_out[..., None, :]).reshape(-1, W_dec.shape[1]))
    return g_acts, g_w


def _decode_backward(ctx, grad_out):
    top_indices, top_acts, W_dec = ctx.saved_tensors
    need_acts, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
    g_acts = g_w = g_b = None
    if need_acts or need_w:
        if grad_out.is_cuda:
            ga, gw = decode_bwd(top_indices, top_acts, W_dec, grad_out.contiguous(), need_acts, need_w)
        else:
            ga, gw = _decode_bwd_host(top_indices, top_acts, W_dec.detach(), grad_out, need_acts, need_w)
        g_acts = ga.to(top_acts.dtype) if need_acts else None
        if g_acts is not None and ctx.live is not None:
            g_acts = torch.where(ctx.live, g_acts, torch.zeros((), dtype=g_acts.dtype, device=g_acts.device))
        g_w = gw.to(W_dec.dtype) if need_w else None
    if ctx.has_bdec and ctx.needs_input_grad[3]:
        g_b = grad_out.reshape(-1, grad_out.shape[-1]).sum(0)
    return None, g_acts, g_w, g_b, None


decode.register_autograd(_decode_backward, setup_context=_decode_setup)


# ---- nested decode: Matryoshka prefixes (csrc/nested_decode.hip) ------------------------------------------
NESTED_MAX_GROUPS = 8
NESTED_MAX_K = 4096


def nested_bounds(bounds, N: int, what: str = "nested_decode") -> tuple:
    """The prefix sizes as validated Python ints: 1 to 8 of them, at least 1, strictly ascending, the last one N."""
    if isinstance(bounds, Tensor):
        bounds = bounds.detach().cpu().reshape(-1).tolist()
    try:
        out = tuple(int(b) for b in bounds)
        same = all(float(b) == float(o) for b, o in zip(bounds, out))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: bounds must be a sequence of integers, got {bounds!r}") from None
    if not same:
        raise ValueError(f"{what}: bounds must be integers, got {list(bounds)!r}")
    if not 1 <= len(out) <= NESTED_MAX_GROUPS:
        raise ValueError(f"{what}: between 1 and {NESTED_MAX_GROUPS} prefix sizes, got {len(out)}")
    if out[0] < 1 or any(a >= b for a, b in zip(out, out[1:])):
        raise ValueError(f"{what}: prefix sizes must be at least 1 and strictly ascending, got {list(out)}")
    if out[-1] != N:
        raise ValueError(f"{what}: the last prefix size must be the number of latents {N}, got {out[-1]}")
    return out


def _nested_bounds_dev(bounds: tuple, dev: torch.device) -> Tensor:
    """The bounds as an int32 tensor on `dev`: a pinned staging copy and an asynchronous transfer on the current stream (no
    host synchronisation; the caching host allocator keeps the staging block until the copy has run)."""
    host = torch.tensor(bounds, dtype=torch.int32)
    return host.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else host


def _nested_check(what: str, x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor, bounds,
                  lengths: Optional[Tensor]) -> tuple:
    if x.dim() < 1 or W_dec.dim() != 2 or x.shape[-1] != W_dec.shape[1] or x.shape[-1] < 1:
        raise ValueError(f"{what}: x [..., d] and W_dec [N, d] must share d, got {tuple(x.shape)} and {tuple(W_dec.shape)}")
    if b_dec is None or b_dec.dim() != 1 or b_dec.shape[0] != W_dec.shape[1]:
        raise ValueError(f"{what}: b_dec must be [d] = [{W_dec.shape[1]}], got {None if b_dec is None else tuple(b_dec.shape)}")
    if x.dtype not in _hip.DTYPE_CODE:
        raise ValueError(f"{what}: x must be float32, bfloat16 or float16, got {x.dtype}")
    if top_acts.shape != top_indices.shape or top_acts.dim() < 1:
        raise ValueError(f"{what}: top_acts and top_indices must share one shape [..., k], got {tuple(top_acts.shape)} and "
                         f"{tuple(top_indices.shape)}")
    k = top_acts.shape[-1]
    if not 1 <= k <= NESTED_MAX_K:
        raise ValueError(f"{what}: k must be in [1, {NESTED_MAX_K}], got {k}")
    T = x.numel() // x.shape[-1]
    if top_acts.numel() != T * k or (top_acts.dim() != 2 and tuple(top_acts.shape[:-1]) != tuple(x.shape[:-1])):
        raise ValueError(f"{what}: the list must hold one row per token of x {tuple(x.shape)}, got {tuple(top_acts.shape)}")
    if top_indices.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: top_indices must be int32 or int64, got {top_indices.dtype}")
    if top_acts.dtype != torch.float32:
        raise ValueError(f"{what}: the list's values must be float32, got {top_acts.dtype}")
    if lengths is not None and lengths.numel() != T:
        raise ValueError(f"{what}: lengths must hold one entry per token ({T}), got {tuple(lengths.shape)}")
    devs = {t.device for t in (x, top_acts, top_indices, W_dec, b_dec) + (() if lengths is None else (lengths,))}
    if len(devs) != 1:
        raise ValueError(f"{what}: all tensors must be on one device, got {sorted(str(d) for d in devs)}")
    return nested_bounds(bounds, W_dec.shape[0], what)


def nested_group_major(top_acts: Tensor, top_indices: Tensor, bounds: tuple, lengths: Optional[Tensor] = None):
    """The group-major order of include/msae.h ("nested decode") in plain torch -> (vals [T, k], idx [T, k] int64,
    group [T, k] int64, order [T, k]): each row stably sorted by group(index); an entry behind the row's length or with an
    index outside [0, N) comes last with value 0, index 0 and group G.  `vals` is a differentiable function of top_acts."""
    k = top_acts.shape[-1]
    N, G = bounds[-1], len(bounds)
    v, i = top_acts.reshape(-1, k), top_indices.detach().reshape(-1, k).long()
    ok = (i >= 0) & (i < N)
    if lengths is not None:
        ok = ok & (torch.arange(k, device=v.device) < lengths.detach().reshape(-1, 1).clamp(0, k))
    edges = torch.tensor(bounds, dtype=torch.int64) if not v.is_cuda else _nested_bounds_dev(bounds, v.device).long()
    grp = torch.where(ok, torch.bucketize(i, edges, right=True), torch.full_like(i, G))
    order = torch.sort(grp, dim=1, stable=True).indices
    v = torch.where(ok, v, torch.zeros((), dtype=v.dtype, device=v.device))
    i = torch.where(ok, i, torch.zeros_like(i))
    return torch.gather(v, 1, order), torch.gather(i, 1, order), torch.gather(grp, 1, order), order


def nested_composed(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor, bounds: tuple,
                    lengths: Optional[Tensor] = None):
    """The nested decode composed of existing differentiable pieces -> (out [T, d], sq [T, G], [e_0 .. e_{G-1}]): the stable
    sort of the group key, then one masked decode of the reordered list per prefix (ops.decode on a HIP device -- r_g then
    has the fused kernel's bits --, plain torch on the host) and one squared-error pass each.  Ordinary autograd reaches
    top_acts, W_dec, b_dec and x.  The fallback of ops.nested_reconstruct and the second opinion of its tests."""
    d = W_dec.shape[1]
    xf = x.reshape(-1, d).to(torch.float32)
    v, i, grp, _ = nested_group_major(top_acts, top_indices, bounds, lengths)
    zero = torch.zeros((), dtype=v.dtype, device=v.device)
    rs, es, sqs = [], [], []
    for g in range(len(bounds)):
        vg = torch.where(grp <= g, v, zero)
        if v.is_cuda:
            r = decode(i, vg, W_dec, b_dec)
        else:
            r = (vg[..., None] * W_dec.to(torch.float32)[i]).sum(-2) + b_dec.to(torch.float32)
        e = r - xf
        rs.append(r)
        es.append(e)
        sqs.append((e * e).sum(-1))
    return rs[-1], torch.stack(sqs, 1), es


def _nested_decode_device(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor, bounds: tuple,
                          lengths: Optional[Tensor], want_residuals: bool):
    dev = _hip.require_device(x, top_acts, top_indices, W_dec, b_dec, lengths)
    lib = _hip.load()
    N, d = W_dec.shape
    G = len(bounds)
    k = top_acts.shape[-1]
    xa, W, bd = x.detach().reshape(-1, d).contiguous(), _f32c(W_dec), _f32c(b_dec)
    T = xa.shape[0]
    out = torch.empty(T, d, dtype=torch.float32, device=dev)
    sq = torch.empty(T, G, dtype=torch.float32, device=dev)
    E = torch.empty(G, T, d, dtype=torch.float32, device=dev) if want_residuals else None
    if T == 0:
        return out, sq, E
    v, i, ld = _list_rows(top_acts, top_indices, k)
    ln = None if lengths is None else lengths.detach().reshape(-1).to(torch.int32).contiguous()
    wide = i.dtype == torch.int64
    fn, name = (lib.msae_nested_decode_i64_f32, "msae_nested_decode_i64_f32") if wide else \
        (lib.msae_nested_decode_f32, "msae_nested_decode_f32")
    b_host = (ctypes.c_int32 * G)(*bounds)             # read during the call: copied into the launch arguments
    flag = _bounds_flag(dev)
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(v), _hip.ptr(i), ld, _hip.ptr(ln), b_host, G,
                      _hip.ptr(W), _hip.ptr(bd), T, k, N, d, _hip.ptr(out), _hip.ptr(E), _hip.ptr(sq), _hip.ptr(flag),
                      _hip.stream_of(xa)), name)
    _check_bounds(flag, name)
    return out, sq, E


def nested_decode(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor, bounds,
                  lengths: Optional[Tensor] = None, want_residuals: bool = False):
    """Every prefix's reconstruction error in one pass (include/msae.h, "nested decode") -> (out [T, d] f32, sq [T, G] f32,
    E [G, T, d] f32 or None).  bounds: the prefix sizes m_0 < ... < m_{G-1} = N, G <= 8.  r_g decodes the entries of the
    list with index < m_g (in group-major order: a stable partition of the list by group), out = r_{G-1}, E[g] = r_g - x,
    sq[:, g] = |E[g]|^2 per token.  x [..., d] f32 / bf16 / f16; top_acts / top_indices [..., k] (k <= 4096; int32 or int64;
    a `[:, :k]` view is read in place); lengths (int32 per token): only the first lengths[t] entries of a row are read.  On
    a HIP device the fused kernel (bit-defined per token); on the host `nested_composed`, the same meaning in plain torch.
    Not differentiable (ops.nested_reconstruct is); nothing is read back."""
    bounds = _nested_check("nested_decode", x, top_acts, top_indices, W_dec, b_dec, bounds, lengths)
    _no_grad_inputs("ops.nested_decode", x, top_acts)
    if not x.is_cuda:
        with torch.no_grad():
            out, sq, es = nested_composed(x, top_acts, top_indices, W_dec, b_dec, bounds, lengths)
        return out, sq, (torch.stack(es) if want_residuals else None)
    return _nested_decode_device(x, top_acts, top_indices, W_dec.detach(), b_dec.detach(), bounds, lengths, want_residuals)


def nested_combine_(E: Tensor, coef: Tensor, grad_full: Optional[Tensor] = None) -> Tensor:
    """In place on E [G, T, d] (msae_nested_combine_f32): S[g] = coef[g] E[g] + S[g + 1] from the last plane down, with
    S[G] = grad_full [T, d] or +0, every step one fmaf.  coef: a device f32 [G].  Returns E."""
    G, T, d = E.shape
    if E.dtype != torch.float32 or not E.is_contiguous() or not 1 <= G <= NESTED_MAX_GROUPS:
        raise ValueError(f"nested_combine_: E must be a contiguous float32 [G <= {NESTED_MAX_GROUPS}, T, d], got "
                         f"{E.dtype} {tuple(E.shape)}")
    if coef.numel() != G or (grad_full is not None and grad_full.numel() != T * d):
        raise ValueError("nested_combine_: coef must be [G] and grad_full [T, d]")
    dev = _hip.require_device(E, coef, grad_full)
    lib = _hip.load()
    cf, gf = _f32c(coef), _f32c(grad_full)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_nested_combine_f32(_hip.ptr(E), _hip.ptr(cf), _hip.ptr(gf), T, d, G, _hip.stream_of(E)),
                   "msae_nested_combine_f32")
    return E


def nested_decode_bwd(top_indices: Tensor, top_acts: Tensor, W_dec: Tensor, planes: Tensor, bounds: tuple,
                      need_acts: bool, need_w: bool) -> Tuple[Tensor, Tensor]:
    """ops.decode_bwd with the gradient row taken from plane group(index) of planes [G, T, d] (include/msae.h, "nested
    decode"): the same two kernels in their grouped form, the same workspace, and the same part in collect_wgrad_sumsq
    and the encoder backward's row sums."""
    dev = _hip.require_device(top_indices, top_acts, W_dec, planes)
    lib = _hip.load()
    idx, acts, W, g = _idx32(top_indices), _f32c(top_acts), _f32c(W_dec), _f32c(planes)
    N, d = W.shape
    G = len(bounds)
    k = idx.shape[-1]
    A = idx.numel() // k
    if tuple(g.shape) != (G, A, d) or bounds[-1] != N:
        raise ValueError(f"nested_decode_bwd: planes must be [G, T, d] = [{G}, {A}, {d}] and the last bound {N}, got "
                         f"{tuple(g.shape)} and {bounds[-1]}")
    bdev = _nested_bounds_dev(bounds, dev)
    g_acts = torch.empty_like(acts) if need_acts else acts.new_empty(0)
    g_w = torch.empty_like(W) if need_w else W.new_empty(0)   # the kernel writes every row
    flag = _bounds_flag(dev)
    with torch.cuda.device(dev):
        st = _hip.stream_of(g)
        if need_acts:
            _hip.check(lib.msae_decode_bwd_acts_grouped_f32(_hip.ptr(idx), _hip.ptr(g), _hip.ptr(bdev), G, _hip.ptr(W), A, k,
                                                            N, d, _hip.ptr(g_acts), _hip.ptr(flag), st),
                       "msae_decode_bwd_acts_grouped_f32")
        if need_w:
            ws = _workspace(dev, lib.msae_decode_bwd_wdec_ws_bytes(A, k, N))
            rowsq = torch.empty(N, dtype=torch.float32, device=dev) if _WGRAD_COLLECT is not None else None
            rowsum = torch.empty(N, dtype=torch.float32, device=dev) if _WGRAD_ROWSUM is not None else None
            d4 = (d + 3) // 4 * 4           # whole f32x4 columns, as decode_bwd: zero columns add exactly 0
            g4 = g if d4 == d else torch.nn.functional.pad(g, (0, d4 - d))
            g_w4 = g_w if d4 == d else torch.empty(N, d4, dtype=torch.float32, device=dev)
            _hip.check(lib.msae_decode_bwd_wdec_grouped_f32(_hip.ptr(idx), _hip.ptr(acts), _hip.ptr(g4), _hip.ptr(bdev), G, A,
                                                            k, N, d4, _hip.ptr(g_w4), _hip.ptr(rowsq), _hip.ptr(rowsum),
                                                            _hip.ptr(flag), _hip.ptr(ws), ws.numel(), st),
                       "msae_decode_bwd_wdec_grouped_f32")
            if d4 != d:
                g_w.copy_(g_w4[:, :d])
            if rowsum is not None:
                _WGRAD_ROWSUM.append(rowsum)
            if rowsq is not None:
                ent = _WGRAD_COLLECT.setdefault(W_dec.data_ptr(), [0, 0, None])
                ent[0] += 1
                ent[1], ent[2] = g_w.data_ptr(), rowsq
    _check_bounds(flag, "msae_decode_bwd_grouped")
    return g_acts, g_w


class _NestedReconstruct(torch.autograd.Function):
    """nested decode + per-prefix squared error as ONE node: forward msae_nested_decode_f32 (the residual planes E are
    kept only when a gradient is needed), backward msae_nested_combine_f32 on E in place and the two grouped decoder
    backward kernels.  x is a constant."""

    @staticmethod
    def forward(ctx, x, top_acts, top_indices, W_dec, b_dec, bounds, lengths):
        need = any(ctx.needs_input_grad[n] for n in (1, 3, 4))
        out, sq, E = _nested_decode_device(x, top_acts, top_indices, W_dec.detach(), b_dec.detach(), bounds, lengths, need)
        ctx.bounds = bounds
        ctx.set_materialize_grads(False)
        if need:
            acts, idx = top_acts.detach(), top_indices
            live = None
            if lengths is not None:
                # as ops.decode: the slots behind a row's length reach the backward kernels as activation 0 on feature 0
                k = acts.shape[-1]
                live = torch.arange(k, device=acts.device) < lengths.reshape(*acts.shape[:-1], 1).clamp(0, k)
                acts = torch.where(live, acts, torch.zeros((), dtype=acts.dtype, device=acts.device))
                idx = torch.where(live, idx, torch.zeros_like(idx))
            ctx.save_for_backward(E, _idx32(idx), acts, W_dec, live)
            ctx.spent = False
        return out, sq.sum(0)

    @staticmethod
    def backward(ctx, g_out, g_sq):
        E, idx, acts, W_dec, live = ctx.saved_tensors
        if ctx.spent:
            raise RuntimeError("ops.nested_reconstruct: the backward folds the gradients into the saved residuals in place; "
                               "a second backward through the same node is not supported")
        ctx.spent = True
        G = len(ctx.bounds)
        coef = torch.zeros(G, dtype=torch.float32, device=E.device) if g_sq is None else g_sq.to(torch.float32) * 2.0
        S = nested_combine_(E, coef, g_out)
        need_acts, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        g_acts = g_w = g_b = None
        if need_acts or need_w:
            ga, gw = nested_decode_bwd(idx, acts, W_dec, S, ctx.bounds, need_acts, need_w)
            if need_acts:
                g_acts = ga.to(acts.dtype)
                if live is not None:
                    g_acts = torch.where(live, g_acts, torch.zeros((), dtype=g_acts.dtype, device=g_acts.device))
            g_w = gw.to(W_dec.dtype) if need_w else None
        if ctx.needs_input_grad[4]:
            g_b = S[0].sum(0)
        return None, g_acts, None, g_w, g_b, None, None


def nested_reconstruct(x: Tensor, top_acts: Tensor, top_indices: Tensor, W_dec: Tensor, b_dec: Tensor, bounds,
                       lengths: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The Matryoshka reconstruction as one differentiable step -> (sae_out [T, d], sq_sum [G]): sae_out decodes the whole
    list, sq_sum[g] = sum over the tokens of |r_g - x|^2 for the reconstruction r_g from the entries with index < bounds[g]
    (include/msae.h, "nested decode").  Gradients reach top_acts, W_dec and b_dec, from sq_sum and from sae_out.  For a HIP
    float32 x that does not require grad this is ONE autograd node over the fused kernels; otherwise (x requires grad, another
    dtype, the host) the composed expression `nested_composed` under ordinary autograd."""
    bounds = _nested_check("nested_reconstruct", x, top_acts, top_indices, W_dec, b_dec, bounds, lengths)
    if x.is_cuda and x.dtype == torch.float32 and not (torch.is_grad_enabled() and x.requires_grad):
        return _NestedReconstruct.apply(x, top_acts, top_indices, W_dec, b_dec, bounds, lengths)
    out, sq, _ = nested_composed(x, top_acts, top_indices, W_dec, b_dec, bounds, lengths)
    return out, sq.sum(0)


# ---- batch-level selection: capped BatchTopK and threshold filters on top-C lists (csrc/batch_select.hip) ------
BATCH_KTH_MAX_VALUES = 1 << 24      # msae_batch_kth_f32's envelope: T * C
LIST_FILTER_MAX_C = 4096            # the encoder's own limit on a list's width


def _list2d(vals: Tensor, idx: Optional[Tensor], what: str, host_f64: bool = False) -> Tuple[Tensor, Optional[Tensor], int, int, int]:
    """A list [..., C] -> ([T, C] views whose rows are read in place where the last dimension is dense, T, C, ld)."""
    if vals.dim() < 1 or vals.shape[-1] < 1:
        raise ValueError(f"{what}: the list must be [..., C] with C >= 1, got {tuple(vals.shape)}")
    if vals.dtype != torch.float32 and not (host_f64 and vals.dtype == torch.float64 and not vals.is_cuda):
        raise ValueError(f"{what}: the list's values must be float32, got {vals.dtype}")
    C = vals.shape[-1]
    T = vals.numel() // C
    if idx is not None:
        if idx.shape != vals.shape:
            raise ValueError(f"{what}: values and indices must share one shape, got {tuple(vals.shape)} and {tuple(idx.shape)}")
        if idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: indices must be int32 or int64, got {idx.dtype}")
        if idx.device != vals.device:
            raise ValueError(f"{what}: values and indices must be on one device")
    v = vals.detach()
    strided = v.dim() == 2 and v.stride(1) == 1 and v.stride(0) >= C and (
        idx is None or (idx.stride(1) == 1 and idx.stride(0) == v.stride(0)))
    if strided and T > 0:                 # the [:, :C] view of a wider list
        return v, idx, T, C, v.stride(0)
    v = v.reshape(T, C).contiguous()
    return v, (None if idx is None else idx.detach().reshape(T, C).contiguous()), T, C, C


def _batch_kth_host(v: Tensor, K: int) -> Tuple[Tensor, Tensor]:
    pos = v[v > 0]
    n = pos.numel()
    n_pos = torch.tensor(n, dtype=torch.int32, device=v.device)
    if n == 0:
        return torch.full((), float("inf"), dtype=torch.float32, device=v.device), n_pos
    return torch.sort(pos, descending=True).values[min(K, n) - 1].clone(), n_pos


def batch_kth(vals: Tensor, K: int) -> Tuple[Tensor, Tensor]:
    """theta of capped BatchTopK (include/msae.h, "batch-level selection", step 2) -> (theta f32 scalar, n_pos int32 scalar),
    both on vals' device: the K-th largest of the entries with v > 0 of the list vals [..., C] (a [:, :C] view of a wider
    2-d list is read in place), the smallest of them when there are fewer than K, +inf when there are none; n_pos = how
    many there are.  Exact and bit-reproducible (an integer radix select); nothing is read back.  On a HIP device T * C may
    be at most 2^24; host tensors take a torch.sort."""
    K = int(K)
    if K < 1:
        raise ValueError(f"batch_kth: K must be positive, got {K}")
    v, _, T, C, ld = _list2d(vals, None, "batch_kth")
    if not v.is_cuda:
        return _batch_kth_host(v, K)
    theta = torch.empty((), dtype=torch.float32, device=v.device)
    n_pos = torch.empty((), dtype=torch.int32, device=v.device)
    if T == 0:
        return theta.fill_(float("inf")), n_pos.zero_()
    if T * C > BATCH_KTH_MAX_VALUES:
        raise ValueError(f"batch_kth: T * C = {T * C} exceeds {BATCH_KTH_MAX_VALUES}: select over chunks of the batch")
    lib = _hip.load()
    ws = _workspace(v.device, lib.msae_batch_kth_ws_bytes(T, C))
    with torch.cuda.device(v.device):
        _hip.check(lib.msae_batch_kth_f32(_hip.ptr(v), T, C, ld, K, _hip.ptr(theta), _hip.ptr(n_pos), _hip.ptr(ws), ws.numel(),
                                          _hip.stream_of(v)), "msae_batch_kth_f32")
    return theta, n_pos


def _list_filter_host(v: Tensor, i: Tensor, theta: Tensor, theta_feat: Optional[Tensor], N: int):
    if theta_feat is None:
        keep = (v > 0) & (v >= theta)
    else:
        ok = (i >= 0) & (i < N)
        keep = ok & (v > 0) & (v >= theta_feat[torch.where(ok, i, torch.zeros_like(i)).long()])
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices         # kept first, each part in list order
    lengths = keep.sum(1).to(torch.int32)
    live = torch.arange(v.shape[1], device=v.device) < lengths[:, None]
    vo = torch.where(live, torch.gather(v, 1, order), torch.zeros((), dtype=v.dtype, device=v.device))
    n_sat = ((v[:, -1] > 0) & (v[:, -1] >= theta)).sum().to(torch.int32)
    return vo, torch.gather(i, 1, order), lengths, n_sat


def list_filter(vals: Tensor, idx: Tensor, theta, theta_feat: Optional[Tensor] = None,
                n_saturated: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Steps 3-6 of include/msae.h, "batch-level selection" -> (vals_out [..., C] f32, idx_out [..., C], lengths int32 [...],
    n_saturated int32 scalar).  An entry of the list vals / idx [..., C] (C <= 4096; a [:, :C] view is read in place) is
    kept iff v > 0 && v >= theta, or with a per-feature table theta_feat f32 [N] iff 0 <= idx < N && v > 0 &&
    v >= theta_feat[idx]; every row is partitioned stably, kept entries first, and the dropped slots come out with
    activation +0.0 and their own index.  theta: a float or a one-element tensor (kept on the device); in table mode it is
    the FLOOR of the saturation test and defaults (None) to theta_feat.min().  n_saturated: an int32 device scalar to ADD
    this call's count of rows with v_last > 0 && v_last >= theta to (None: a fresh zero).  Not differentiable; nothing is
    read back."""
    v, i, T, C, ld = _list2d(vals, idx, "list_filter")
    if C > LIST_FILTER_MAX_C:
        raise ValueError(f"list_filter: C must be at most {LIST_FILTER_MAX_C}, got {C}")
    dev = v.device
    N = 0
    if theta_feat is not None:
        if not isinstance(theta_feat, Tensor) or theta_feat.dim() != 1 or theta_feat.numel() < 1:
            raise ValueError("list_filter: theta_feat must be a 1-d tensor [N]")
        theta_feat = theta_feat.detach().to(dev, torch.float32).contiguous()
        N = theta_feat.numel()
        if theta is None:
            theta = theta_feat.min()
    if theta is None:
        raise ValueError("list_filter: theta is required without a per-feature table")
    if isinstance(theta, Tensor):
        if theta.numel() != 1:
            raise ValueError(f"list_filter: theta must hold one element, got {tuple(theta.shape)}")
        th = theta.detach().to(dev, torch.float32).reshape(())
    else:
        th = torch.full((), float(theta), dtype=torch.float32, device=dev)
    if n_saturated is not None and (n_saturated.dtype != torch.int32 or n_saturated.numel() != 1 or n_saturated.device != dev):
        raise ValueError("list_filter: n_saturated must be an int32 scalar on the list's device")
    lead = tuple(vals.shape[:-1])
    if not v.is_cuda:
        vo, io, lengths, n_sat = _list_filter_host(v, i, th, theta_feat, N)
        if n_saturated is not None:
            n_sat = n_saturated.add_(n_sat.reshape(n_saturated.shape))
        return vo.view(*lead, C), io.view(*lead, C), lengths.view(lead), n_sat
    lib = _hip.load()
    vo = torch.empty(T, C, dtype=torch.float32, device=dev)
    io = torch.empty(T, C, dtype=i.dtype, device=dev)
    lengths = torch.empty(T, dtype=torch.int32, device=dev)
    n_sat = n_saturated if n_saturated is not None else torch.zeros((), dtype=torch.int32, device=dev)
    fn, name = (lib.msae_list_filter_i64_f32, "msae_list_filter_i64_f32") if i.dtype == torch.int64 else \
        (lib.msae_list_filter_f32, "msae_list_filter_f32")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(v), _hip.ptr(i), T, C, ld, _hip.ptr(th), _hip.ptr(theta_feat), N, _hip.ptr(vo), _hip.ptr(io),
                      _hip.ptr(lengths), _hip.ptr(n_sat), _hip.stream_of(v)), name)
    return vo.view(*lead, C), io.view(*lead, C), lengths.view(lead), n_sat


class _BatchSelect(torch.autograd.Function):
    """batch_kth + list_filter as one autograd node: the gradient of a kept entry passes, a dropped slot's is 0."""

    @staticmethod
    def forward(ctx, acts, idx, k):
        C = acts.shape[-1]
        theta, _ = batch_kth(acts, max((acts.numel() // C) * k, 1))
        kept, _, lengths, n_sat = list_filter(acts, idx, theta)
        ctx.save_for_backward(kept)
        ctx.mark_non_differentiable(lengths, theta, n_sat)
        return kept, lengths, theta, n_sat

    @staticmethod
    def backward(ctx, g, _gl, _gt, _gn):
        kept, = ctx.saved_tensors
        return torch.where(kept > 0, g, torch.zeros((), dtype=g.dtype, device=g.device)), None, None


def batch_select(acts: Tensor, idx: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Capped BatchTopK over canonical top-C lists (include/msae.h, "batch-level selection"): of the T rows of acts / idx
    [..., C] (value descending, as ops.encode_topk / ops.sparse_encode return them) keep the entries at or above the
    (T * k)-th largest positive value of the whole batch -> (acts_kept [..., C], lengths int32 [...], theta f32 scalar,
    n_saturated int32 scalar), all on the device, no host synchronisation.  The kept entries are a prefix of every row, so
    `idx` serves acts_kept unchanged; the dropped slots hold +0.0.  One autograd node: the backward is the gradient times
    the keep mask."""
    if int(k) < 1 or int(k) > acts.shape[-1]:
        raise ValueError(f"batch_select: k must be in [1, C = {acts.shape[-1]}], got {k}")
    return _BatchSelect.apply(acts, idx, int(k))


# ---- JumpReLU selection: learned per-feature thresholds on top-C lists (csrc/jump_select.hip) -----------------------
JUMP_MAX_C = 256                    # msae_jump_filter_f32's envelope: one wave per token


def jump_half_band(bandwidth: float) -> float:
    """h = 0.5f * eps as the kernels get it: eps rounded to f32, halved in f32 (exact)."""
    return 0.5 * ctypes.c_float(bandwidth).value


def _jump_classes(v: Tensor, i: Tensor, theta: Tensor, h: float):
    """(kept, near, band, theta_f) of include/msae.h, "JumpReLU selection", elementwise in f32."""
    N = theta.numel()
    ok = (i >= 0) & (i < N) & (v > 0)
    th = theta[torch.where(ok, i, torch.zeros_like(i)).long()]
    kept = ok & (v >= th)
    near = ok & ~kept & ((th - v) < h)
    band = ok & ((v - th).abs() < h)
    return kept, near, band, th


def _jump_filter_host(v: Tensor, i: Tensor, theta: Tensor, h: float, floor: Tensor):
    kept, near, _, _ = _jump_classes(v, i, theta, h)
    part = torch.where(kept, 0, torch.where(near, 1, 2)).to(torch.int8)
    order = torch.sort(part, dim=1, stable=True).indices                           # kept, near, rest: each in list order
    lengths = kept.sum(1).to(torch.int32)
    reach = lengths + near.sum(1).to(torch.int32)
    live = torch.arange(v.shape[1], device=v.device) < lengths[:, None]
    vo = torch.where(live, torch.gather(v, 1, order), torch.zeros((), dtype=v.dtype, device=v.device))
    n_sat = ((v[:, -1] > 0) & (v[:, -1] >= floor)).sum().to(torch.int32)
    return vo, torch.gather(i, 1, order), lengths, reach, order.to(torch.uint8), lengths.sum(dtype=torch.int64), n_sat


def _jump_bwd_host(v: Tensor, i: Tensor, theta: Tensor, h: float, eps: float, src: Tensor, lengths: Tensor, g: Tensor, s: Tensor):
    C = v.shape[1]
    order = src.long()
    live = torch.arange(C, device=v.device) < lengths[:, None]
    zero = torch.zeros((), dtype=g.dtype, device=g.device)
    g_in = torch.zeros_like(g).scatter_(1, order, torch.where(live, g, zero))
    g_at = torch.zeros_like(g).scatter_(1, order, g)                               # the upstream gradient by INPUT slot
    _, _, band, th = _jump_classes(v, i, theta, h)
    # (the kernel's c is -fmaf(theta_f, g, s) / eps: here the sum in double, rounded once, so that theta g and s may cancel)
    c = (-(th.double() * g_at.double() + s.double()) / eps).to(v.dtype)
    g_theta = torch.zeros(theta.numel(), dtype=v.dtype, device=v.device)
    g_theta.index_add_(0, i[band].long(), c[band])
    return g_in, g_theta


def jump_filter(vals: Tensor, idx: Tensor, theta: Tensor, bandwidth: float, l0: Optional[Tensor] = None,
                n_saturated: Optional[Tensor] = None):
    """The forward of include/msae.h, "JumpReLU selection" -> (vals_out [..., C] f32, idx_out [..., C], lengths int32 [...],
    reach int32 [...], src uint8 [T, C], l0 int64 scalar, n_saturated int32 scalar).  vals / idx [..., C] with C <= 256 (a
    [:, :C] view is read in place), theta f32 [N], bandwidth > 0.  l0 / n_saturated: device counters to ADD to (None: fresh
    zeros).  Not differentiable (ops.jump_select is); nothing is read back."""
    v, i, T, C, ld = _list2d(vals, idx, "jump_filter", host_f64=True)
    if C > JUMP_MAX_C:
        raise ValueError(f"jump_filter: C must be at most {JUMP_MAX_C}, got {C}")
    if not isinstance(theta, Tensor) or theta.dim() != 1 or theta.numel() < 1:
        raise ValueError("jump_filter: theta must be a 1-d tensor [N]")
    h = jump_half_band(bandwidth) if v.dtype == torch.float32 else 0.5 * float(bandwidth)
    if not (h > 0 and h != float("inf")):
        raise ValueError(f"jump_filter: the bandwidth must be positive and finite, got {bandwidth}")
    dev = v.device
    theta = theta.detach().to(dev, v.dtype).contiguous()
    N = theta.numel()
    floor = theta.min() - h
    lead = tuple(vals.shape[:-1])
    for name, t, dt in (("l0", l0, torch.int64), ("n_saturated", n_saturated, torch.int32)):
        if t is not None and (t.dtype != dt or t.numel() != 1 or t.device != dev):
            raise ValueError(f"jump_filter: {name} must be a {dt} scalar on the list's device")
    if not v.is_cuda:
        vo, io, lengths, reach, src, n_kept, n_sat = _jump_filter_host(v, i, theta, h, floor)
        n_kept = n_kept if l0 is None else l0.add_(n_kept.reshape(l0.shape))
        n_sat = n_sat if n_saturated is None else n_saturated.add_(n_sat.reshape(n_saturated.shape))
        return vo.view(*lead, C), io.view(*lead, C), lengths.view(lead), reach.view(lead), src, n_kept, n_sat
    lib = _hip.load()
    vo = torch.empty(T, C, dtype=torch.float32, device=dev)
    io = torch.empty(T, C, dtype=i.dtype, device=dev)
    lengths = torch.empty(T, dtype=torch.int32, device=dev)
    reach = torch.empty(T, dtype=torch.int32, device=dev)
    src = torch.empty(T, C, dtype=torch.uint8, device=dev)
    n_kept = l0 if l0 is not None else torch.zeros((), dtype=torch.int64, device=dev)
    n_sat = n_saturated if n_saturated is not None else torch.zeros((), dtype=torch.int32, device=dev)
    fn, name = (lib.msae_jump_filter_i64_f32, "msae_jump_filter_i64_f32") if i.dtype == torch.int64 else \
        (lib.msae_jump_filter_f32, "msae_jump_filter_f32")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(v), _hip.ptr(i), T, C, ld, _hip.ptr(theta), N, h, _hip.ptr(floor), _hip.ptr(vo), _hip.ptr(io),
                      _hip.ptr(lengths), _hip.ptr(reach), _hip.ptr(src), _hip.ptr(n_kept), _hip.ptr(n_sat),
                      _hip.stream_of(v)), name)
    return vo.view(*lead, C), io.view(*lead, C), lengths.view(lead), reach.view(lead), src, n_kept, n_sat


def jump_bwd(vals: Tensor, idx: Tensor, theta: Tensor, bandwidth: float, src: Tensor, lengths: Tensor, reach: Tensor,
             g: Tensor, s: Tensor) -> Tuple[Tensor, Tensor]:
    """The backward of include/msae.h, "JumpReLU selection" -> (g_in [T, C] f32, g_theta [N] f32): vals / idx / theta /
    bandwidth as jump_filter got them, src / lengths / reach as it returned them, g [T, C] the gradient of its vals_out and
    s (a one-element f32 tensor) the gradient of the float l0.  Bit-reproducible; nothing is read back."""
    v, i, T, C, ld = _list2d(vals, idx, "jump_bwd", host_f64=True)
    dev = v.device
    theta = theta.detach().to(dev, v.dtype).contiguous()
    N = theta.numel()
    h, eps = jump_half_band(bandwidth), ctypes.c_float(bandwidth).value
    if v.dtype == torch.float64:           # (host tensors only: the definition itself, in double)
        h, eps = 0.5 * float(bandwidth), float(bandwidth)
    g = g.detach().to(v.dtype).reshape(T, C).contiguous()
    s = s.detach().to(dev, v.dtype).reshape(())
    ln, rc = lengths.reshape(T), reach.reshape(T)
    if not v.is_cuda:
        return _jump_bwd_host(v, i, theta, h, eps, src.reshape(T, C), ln, g, s)
    lib = _hip.load()
    g_in = torch.empty(T, C, dtype=torch.float32, device=dev)
    g_theta = torch.empty(N, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.msae_jump_bwd_ws_bytes(T, C, N)) if T > 0 else None
    fn, name = (lib.msae_jump_bwd_i64_f32, "msae_jump_bwd_i64_f32") if i.dtype == torch.int64 else \
        (lib.msae_jump_bwd_f32, "msae_jump_bwd_f32")
    with torch.cuda.device(dev):
        _hip.check(fn(_hip.ptr(v), _hip.ptr(i), T, C, ld, _hip.ptr(theta), N, h, eps, _hip.ptr(src.contiguous()),
                      _hip.ptr(ln.contiguous()), _hip.ptr(rc.contiguous()), _hip.ptr(g), _hip.ptr(s), _hip.ptr(g_in),
                      _hip.ptr(g_theta), _hip.ptr(ws), 0 if ws is None else ws.numel(), _hip.stream_of(v)), name)
    return g_in, g_theta


class _JumpSelect(torch.autograd.Function):
    """jump_filter as one autograd node with the straight-through backward jump_bwd."""

    @staticmethod
    def forward(ctx, acts, idx, theta, bandwidth):
        kept, idx_out, lengths, reach, src, n_kept, n_sat = jump_filter(acts, idx, theta, bandwidth)
        v, i, _, _, _ = _list2d(acts, idx, "jump_select", host_f64=True)
        ctx.save_for_backward(v, i, theta.detach(), src, lengths, reach)
        ctx.bandwidth, ctx.shape = bandwidth, acts.shape
        l0 = n_kept.to(v.dtype)
        ctx.mark_non_differentiable(idx_out, lengths, reach, n_sat)
        return kept, idx_out, lengths, reach, l0, n_sat

    @staticmethod
    def backward(ctx, g, _gi, _gl, _gr, g_l0, _gn):
        v, i, theta, src, lengths, reach = ctx.saved_tensors
        if g is None:
            g = torch.zeros(ctx.shape, dtype=v.dtype, device=v.device)
        if g_l0 is None:
            g_l0 = torch.zeros((), dtype=v.dtype, device=v.device)
        g_in, g_theta = jump_bwd(v, i, theta, ctx.bandwidth, src, lengths, reach, g, g_l0)
        return g_in.view(ctx.shape), None, g_theta, None


def jump_select(acts: Tensor, idx: Tensor, theta: Tensor, bandwidth: float):
    """JumpReLU with per-feature thresholds over canonical top-C lists (include/msae.h, "JumpReLU selection"): an entry of
    acts / idx [..., C] (C <= 256) is kept iff its index lies in [0, N), a > 0 and a >= theta[idx] -- ops.list_filter's table
    rule -> (acts_kept [..., C], idx_out [..., C], lengths int32 [...], reach int32 [...], l0 f32 scalar, n_saturated int32
    scalar), all on the device, no host synchronisation.  Every row is partitioned stably: the kept entries, then the dropped
    ones inside the straight-through band (theta - a < bandwidth / 2), then the rest, the dropped slots with activation +0.0;
    reach counts the first two parts, l0 = sum(lengths).  One autograd node: acts_kept and l0 are differentiable, gradients
    reach acts (the kept entries') and theta (the rectangle-kernel pseudo-derivatives of the band entries, summed per
    feature in a fixed order: bit-reproducible).  Host tensors take a plain-torch path with the same meaning (float64 lists
    too: the definition evaluated in double)."""
    bandwidth = float(bandwidth)
    if not (bandwidth > 0 and bandwidth != float("inf")):
        raise ValueError(f"jump_select: the bandwidth must be positive and finite, got {bandwidth}")
    if not isinstance(theta, Tensor) or theta.dim() != 1 or theta.numel() < 1:
        raise ValueError("jump_select: theta must be a 1-d tensor [N]")
    if acts.shape[-1] > JUMP_MAX_C:
        raise ValueError(f"jump_select: C must be at most {JUMP_MAX_C}, got {acts.shape[-1]}")
    return _JumpSelect.apply(acts, idx, theta, bandwidth)


# ---- cache sparsify ---------------------------------------------------------------------------------
def sparsify(top_acts: Tensor, top_indices: Tensor, num_latents: int, row_base: int = 0,
             thresh: float = 1e-5, filter_bitmap: Optional[Tensor] = None, sync: bool = True):
    """[B, S, k] top-k -> (locations [nnz, 3] int64, activations [nnz] f32) in the reference cache's
    record order (row, pos, feature ascending); |v| > thresh and optional feature bitmap applied.

    sync=True reads nnz back (one int64, as `torch.nonzero` does) and returns exactly-sized tensors.
    sync=False never touches the host: returns (locations [B*S*k, 3], activations [B*S*k], nnz) with the
    first nnz rows valid and nnz a device int64 scalar -- for loops inside a forward hook that must stay
    stream-ordered (msae/features/cache.py collects these and reads the counts back once per flush)."""
    dev = _hip.require_device(top_acts, top_indices, filter_bitmap)
    lib = _hip.load()
    assert top_acts.dim() == 3 and top_acts.shape == top_indices.shape
    B, S, k = top_acts.shape
    vals, idx = _f32c(top_acts), _idx32(top_indices)
    counts = torch.empty(B * S + 1, dtype=torch.int64, device=dev)
    fb = None if filter_bitmap is None else filter_bitmap.to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        st = _hip.stream_of(vals)
        _hip.check(lib.msae_sparsify_count(_hip.ptr(vals), _hip.ptr(idx), B, S, k, thresh, _hip.ptr(fb),
                                           num_latents, _hip.ptr(counts), st), "msae_sparsify_count")
        nnz = int(counts[-1].item()) if sync else B * S * k   # the one host read (torch.nonzero does the same)
        loc = torch.empty(nnz, 3, dtype=torch.int64, device=dev)
        act = torch.empty(nnz, dtype=torch.float32, device=dev)
        if nnz:
            _hip.check(lib.msae_sparsify_write(_hip.ptr(vals), _hip.ptr(idx), B, S, k, thresh,
                                               _hip.ptr(fb), num_latents, row_base, _hip.ptr(counts),
                                               _hip.ptr(loc), _hip.ptr(act), st), "msae_sparsify_write")
    return (loc, act) if sync else (loc, act, counts[-1])


def merge_topk_gathered(gathered: Tensor, T: int, G: int, kl: int, k: int):
    """Canonical top-k of the all-gathered per-shard pairs (int32 [G*2, T, kl]) on the device.
    -> (vals f32 [T,k], idx int64 [T,k], flagged int32 [T])."""
    dev = _hip.require_device(gathered)
    lib = _hip.load()
    assert gathered.dtype == torch.int32 and gathered.is_contiguous() and gathered.numel() == G * 2 * T * kl
    vals = torch.empty(T, k, dtype=torch.float32, device=dev)
    idx = torch.empty(T, k, dtype=torch.int32, device=dev)
    flagged = torch.empty(T, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(lib.msae_merge_topk(_hip.ptr(gathered), T, G, kl, k, _hip.ptr(vals), _hip.ptr(idx),
                                       _hip.ptr(flagged), _hip.stream_of(gathered)), "msae_merge_topk")
    return vals, idx.to(torch.int64), flagged


def merge_topk_gathered_masked_(gathered: Tensor, T: int, G: int, kl: int, k: int, mask: Tensor, vals: Tensor,
                                idx: Tensor) -> None:
    """msae_merge_topk_masked: rows t of (vals f32 [T,k], idx int64 [T,k]) with mask[t] != 0 (int32 [T]) become the
    canonical top-k of the gathered pairs, in place; the other rows keep what they hold."""
    dev = _hip.require_device(gathered, mask, vals, idx)
    assert gathered.dtype == torch.int32 and gathered.is_contiguous() and gathered.numel() == G * 2 * T * kl
    assert mask.dtype == torch.int32 and mask.numel() == T and mask.is_contiguous()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.is_contiguous() and idx.is_contiguous()
    assert vals.shape == (T, k) and idx.shape == (T, k)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_merge_topk_masked(_hip.ptr(gathered), T, G, kl, k, _hip.ptr(mask), _hip.ptr(vals),
                                                      None, _hip.ptr(idx), _hip.stream_of(gathered)),
                   "msae_merge_topk_masked")


def compact_flags(flags: Tensor) -> Tuple[Tensor, Tensor]:
    """flags int32 [T] -> (rows int32 [T]: the flagged t in ascending order in rows[:n], n int32 [1]), all on the
    device: the redo list `encode_topk_rows_` takes.  Nothing is read back."""
    dev = _hip.require_device(flags)
    assert flags.dtype == torch.int32 and flags.is_contiguous()
    T = flags.numel()
    rows = torch.empty(max(T, 1), dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_compact_flags(_hip.ptr(flags), T, _hip.ptr(rows), _hip.ptr(n),
                                                  _hip.stream_of(flags)), "msae_compact_flags")
    return rows, n


def encode_topk_rows_(x: Tensor, W_enc: Tensor, b_enc: Optional[Tensor], b_dec: Optional[Tensor], rows: Tensor,
                      n_rows: Tensor, k: int, vals: Tensor, idx: Tensor, status: Optional[Tensor] = None,
                      set_feature: int = -1, set_value: float = 0.0, zero_feature: int = -1) -> None:
    """msae_encode_topk_rows: the exact Sae.encode of the tokens rows[:n_rows] (device-side list and count) of
    x [T, d], written to rows of vals f32 [T, k] / idx int64 [T, k] (/ status int32 [T] = 1) in place.  The work is
    sized on the device; nothing is read back."""
    dev = _hip.require_device(x, W_enc, b_enc, b_dec, rows, n_rows, vals, idx, status)
    lib = _hip.load()
    xa, W, be, bd = _act(x), _f32c(W_enc), _f32c(b_enc), _f32c(b_dec)
    N, d = W.shape
    T = xa.numel() // d
    assert rows.dtype == torch.int32 and n_rows.dtype == torch.int32 and rows.numel() >= T
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.is_contiguous() and idx.is_contiguous()
    assert vals.shape == (T, k) and idx.shape == (T, k)
    if T == 0:
        return
    ws = _workspace(dev, lib.msae_encode_topk_rows_ws_bytes(T, N))
    with torch.cuda.device(dev):
        _hip.check(lib.msae_encode_topk_rows(_hip.ptr(xa), _hip.DTYPE_CODE[xa.dtype], _hip.ptr(W), _hip.ptr(be),
                                             _hip.ptr(bd), _hip.ptr(rows), _hip.ptr(n_rows), T, d, N, k, set_feature,
                                             float(set_value), zero_feature, _hip.ptr(vals), _hip.ptr(idx),
                                             _hip.ptr(status), _hip.ptr(ws), ws.numel(), _hip.stream_of(xa)),
                   "msae_encode_topk_rows")


# ---- trainable encoder (training forward, sae.py:193-247) -------------------------------------------
AUXK_PATHS = ("dense", "subset")


class _SparseEncode(torch.autograd.Function):
    """pre_acts + the three TopK selections of Sae.forward as ONE autograd node with a SPARSE
    backward.  The reference back-propagates a dense [T, N] gradient through topk -> relu ->
    nn.Linear (a second full GEMM, dW = g^T a); only the selected (token, latent) pairs carry
    gradient, so here
        dW_enc[n] += g[t,j] * a[t]      -> msae_decode_bwd_wdec_f32 (sparse outer-product accumulate)
        da[t]      = sum_j g[t,j] W_enc[n_tj]  -> msae_decode_f32 over W_enc (gather matmul)
        db_enc[n] += g[t,j]  ;  dx = da ;  db_dec = -sum_t da[t]
    with g masked by relu'(pre) = (value > 0)."""

    @staticmethod
    def forward(ctx, x, W_enc, b_enc, b_dec, k, dead_mask, k_aux, k_multi, prepared=None, set_feature=-1,
                set_value=0.0, zero_feature=-1, edit_set=None, auxk_path="dense", dead_list=None, edit_group=None):
        vals, idxs = [], []
        edits = set_feature >= 0 or zero_feature >= 0 or edit_set is not None
        assert not (edits and (k_aux > 0 or k_multi > 0)), "hook edits apply to the plain top-k only"
        row_mask = gain = None
        valued = edit_set is not None and getattr(edit_set, "value_dependent", False)
        if edit_set is not None and edit_group is not None:
            # one table per token (msae.features.RowEdits + the tokens' group ids): the same two steps, and the kernel says
            # which output slots hold an edit's own value -- a feature-wide mask is wrong once the tables differ per token
            assert set_feature < 0 and zero_feature < 0, "edits= and the scalar edit arguments are mutually exclusive"
            v, i, _ = encode_topk(x, W_enc, b_enc, b_dec,
                                  prepared if prepared is not None else _refresh_train_operands(W_enc, x.shape[0]),
                                  k + edit_set.E_max)
            if valued:  # scale / add / floor / cap: the kernel reads the features' exact latents and returns each slot's gain
                cur = pre_acts_features(x, W_enc, b_enc, b_dec, edit_set.union)
                v, i, row_mask, gain = edit_topk_rows(v, i, edit_group, edit_set, W_enc.shape[0], k, want_mask=True, cur=cur,
                                                      col=edit_set.col, want_gain=True)
            else:
                v, i, row_mask = edit_topk_rows(v, i, edit_group, edit_set, W_enc.shape[0], k, want_mask=True)
            vals.append(v); idxs.append(i)
        elif edit_set is not None:
            # a SET of edits (msae.features.FeatureEdits): the unedited encode over-fetches k + E entries, edit_topk re-ranks
            # each list with the edits applied (exact: DESIGN.md section 7d) -- the same two steps as the inference path
            assert set_feature < 0 and zero_feature < 0, "edits= and the scalar edit arguments are mutually exclusive"
            v, i, _ = encode_topk(x, W_enc, b_enc, b_dec,
                                  prepared if prepared is not None else _refresh_train_operands(W_enc, x.shape[0]),
                                  k + edit_set.E)
            if valued:
                cur = pre_acts_features(x, W_enc, b_enc, b_dec, edit_set.feat)
                v, i, gain = edit_topk(v, i, edit_set.feat, edit_set.val, edit_set.kind, W_enc.shape[0], k, cur=cur,
                                       want_gain=True)
            else:
                v, i = edit_topk(v, i, edit_set.feat, edit_set.val, edit_set.kind, W_enc.shape[0], k)
            vals.append(v); idxs.append(i)
        elif k_aux == 0 and max(k, k_multi) <= 256:
            # no AuxK term: the fused encoder gives the canonical top-max(k, 4k); the top-k is its
            # prefix (same order), and the dense [T, N] latents are never built.  `prepared`: operands
            # of a weight that does not change between calls (inference hooks); None = training step
            kk = max(k, k_multi)
            v, i, _ = encode_topk(x, W_enc, b_enc, b_dec,
                                  prepared if prepared is not None else _refresh_train_operands(W_enc, x.shape[0]), kk,
                                  set_feature, set_value, zero_feature)
            vals.append(v[..., :k].contiguous()); idxs.append(i[..., :k].contiguous())
            if k_multi > 0:
                vals.append(v); idxs.append(i)
        elif auxk_path == "subset" and k_aux > 0 and max(k, k_multi) <= 256:
            # AuxK without the dense latents: the main and Multi-TopK selections from the fused encoder
            # as above, the AuxK selection from the exact GEMM over the dead features only -- the same bits as the branch below
            kk = max(k, k_multi)
            v, i, _ = encode_topk(x, W_enc, b_enc, b_dec,
                                  prepared if prepared is not None else _refresh_train_operands(W_enc, x.shape[0]), kk)
            vals.append(v[..., :k].contiguous()); idxs.append(i[..., :k].contiguous())
            if dead_list is None:      # ascending, built on the device (the one host read: the list's length)
                dead_list = torch.nonzero(dead_mask).flatten().to(torch.int32)
            va, ia = topk_within(x, W_enc, b_enc, b_dec, dead_list, k_aux)
            vals.append(va); idxs.append(ia)
            if k_multi > 0:
                vals.append(v); idxs.append(i)
        else:
            pre = pre_acts(x, W_enc, b_enc, b_dec)
            if set_feature >= 0:
                pre[..., set_feature] = set_value
            if zero_feature >= 0:
                pre[..., zero_feature] = 0.0
            v, i = topk(pre, k)
            vals.append(v); idxs.append(i)
            if k_aux > 0:
                dead_pre = torch.where(dead_mask[None], pre, -torch.inf)            # sae.py:217-220
                v, i = topk(dead_pre, k_aux)        # LDS-resident selection: k_aux <= 16384 (d_in <= 32768)
                vals.append(v); idxs.append(i)
            if k_multi > 0:
                v, i = topk(pre, k_multi)                                           # sae.py:233
                vals.append(v); idxs.append(i)
        ctx.save_for_backward(x, W_enc, b_dec, torch.cat(idxs, -1), torch.cat(vals, -1))
        ctx.splits = [t.shape[-1] for t in vals]
        ctx.set_feature = set_feature
        ctx.edit_mask = None if edit_set is None or row_mask is not None or gain is not None else edit_set.mask
        ctx.row_mask = row_mask if gain is None else None
        ctx.gain = gain          # value-dependent edits: dL'/dL per slot -- 0 at SET / ZERO slots, 1 at unedited ones
        ctx.has_b_enc = b_enc is not None
        out = []
        for v, i in zip(vals, idxs):
            out += [v, i]
        for i in idxs:
            ctx.mark_non_differentiable(i)
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        x, W_enc, b_dec, idx_cat, val_cat = ctx.saved_tensors
        g = [grads[2 * j] if grads[2 * j] is not None else
             torch.zeros(val_cat.shape[0], n, device=val_cat.device) for j, n in enumerate(ctx.splits)]
        g_cat = torch.cat(g, -1).float() * (val_cat > 0)           # relu'
        if ctx.set_feature >= 0:                                   # a latent overwritten by a constant carries no gradient
            g_cat = g_cat * (idx_cat != ctx.set_feature)
        if ctx.edit_mask is not None:                              # ... and neither does one of a set of edited latents
            g_cat = g_cat * ~ctx.edit_mask[idx_cat]
        if ctx.row_mask is not None:                               # ... per token: the slots that came from an edit entry
            g_cat = g_cat * ~ctx.row_mask.bool()
        if ctx.gain is not None:                                   # ... or scaled by the edit's own derivative
            g_cat = g_cat * ctx.gain
        a = x.float() if b_dec is None else x.float() - b_dec     # (None: a transcoder's encoder reads x as it is)
        need_x, need_W, need_be, need_bd = ctx.needs_input_grad[:4]
        need_bd = need_bd and b_dec is not None
        g_x = g_W = g_be = g_bd = None
        rowsum = None
        if need_W:
            # the weight-gradient kernel also sums every feature's latent gradients (ascending pair order): the encoder-bias
            # gradient without index_add_'s atomics, and the vector s of the b_dec gradient -(s^T W_enc) below
            global _WGRAD_ROWSUM
            prev, _WGRAD_ROWSUM = _WGRAD_ROWSUM, []
            try:
                _, g_W = decode_bwd(idx_cat, g_cat, W_enc, a.contiguous(), False, True)
                rowsum = _WGRAD_ROWSUM[0] if _WGRAD_ROWSUM else None
            finally:
                _WGRAD_ROWSUM = prev
        if need_be and ctx.has_b_enc:
            g_be = rowsum if rowsum is not None else torch.zeros(W_enc.shape[0], device=g_cat.device).index_add_(
                0, idx_cat.reshape(-1), g_cat.reshape(-1))
        if need_bd and not need_x and rowsum is not None and W_enc.shape[1] % 4 == 0:
            g_bd = weighted_row_sum(W_enc, rowsum, -1.0)          # ONE streaming read of W_enc (training: x is a constant)
        elif need_x or need_bd:
            da = decode(idx_cat, g_cat, W_enc, None)
            g_x = da.to(x.dtype) if need_x else None
            g_bd = -da.sum(0) if need_bd else None
        return g_x, g_W, g_be, g_bd, None, None, None, None, None, None, None, None, None, None, None, None


def sparse_encode(x: Tensor, W_enc: Tensor, b_enc: Tensor, b_dec: Tensor, k: int,
                  dead_mask: Optional[Tensor] = None, k_aux: int = 0, k_multi: int = 0, *,
                  prepared: Optional[Tensor] = None, set_feature: int = -1, set_value: float = 0.0,
                  zero_feature: int = -1, edits=None, auxk_path: str = "dense", dead_list: Optional[Tensor] = None,
                  edit_group: Optional[Tensor] = None):
    """-> [(acts, idx)] for the top-k, (optional) AuxK and (optional) Multi-TopK selections.
    Differentiable w.r.t. x, W_enc, b_enc, b_dec through the selected latents (the graph of the
    reference's pre_acts -> [mask] -> topk, sae.py:172-185, patching/utils.py:43-49).  `edits`: a
    msae.features.FeatureEdits instead of the scalar edit arguments; an edited latent carries no gradient.  A
    msae.features.RowEdits comes with `edit_group` (int tensor x.shape[:-1]: every token's group): the same per token.
    auxk_path: "dense" (pre_acts + three top-k over [T, N]) or "subset": with k_aux > 0 and max(k, k_multi) <= 256 the AuxK
    selection comes from `topk_within` over the dead features (dead_list: their ascending int32 device list, built from
    dead_mask when None) and the other two from the fused encoder -- the same selections bit for bit; in every other case
    the value changes nothing."""
    if auxk_path not in AUXK_PATHS:
        raise ValueError(f"auxk_path must be one of {AUXK_PATHS}, got {auxk_path!r}")
    lead = x.shape[:-1]
    if (edit_group is not None) != hasattr(edits, "offsets"):
        raise ValueError("sparse_encode: edit_group goes with a msae.features.RowEdits, and a RowEdits needs it")
    if edit_group is not None:
        if tuple(edit_group.shape) != tuple(lead):
            raise ValueError(f"sparse_encode: edit_group must have shape {tuple(lead)}, got {tuple(edit_group.shape)}")
        edit_group = edit_group.reshape(-1)
    out = _SparseEncode.apply(x.reshape(-1, x.shape[-1]), W_enc, b_enc, b_dec, k, dead_mask, k_aux, k_multi, prepared,
                              set_feature, float(set_value), zero_feature, edits, auxk_path, dead_list,
                              edit_group)                              # the node works on [T, d]
    if len(lead) != 1:
        out = tuple(o.reshape(*lead, o.shape[-1]) for o in out)
    return [(out[2 * j], out[2 * j + 1]) for j in range(len(out) // 2)]


# ---- parameter-sized passes of one optimisation step (csrc/train.hip) --------------------------------
def unit_norm_rows_(W: Tensor, eps: float) -> Tensor:
    """W /= ||W||_row + eps, in place, one read + one write (sae.py:249-255)."""
    dev = _hip.require_device(W)
    assert W.dtype == torch.float32 and W.dim() == 2 and W.is_contiguous()
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_unit_norm_rows_f32(_hip.ptr(W), W.shape[0], W.shape[1], float(eps),
                                                       _hip.stream_of(W)), "msae_unit_norm_rows_f32")
    return W


def grad_sumsq_(accum: Tensor, g: Tensor) -> Tensor:
    """accum (f32 device scalar) += sum(g^2): the total-norm half of clip_grad_norm_, no host sync."""
    dev = _hip.require_device(g, accum)
    assert g.dtype == torch.float32 and g.is_contiguous() and accum.dtype == torch.float32 and accum.numel() == 1
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_grad_sumsq_f32(_hip.ptr(g), g.numel(), _hip.ptr(accum), _hip.stream_of(g)),
                   "msae_grad_sumsq_f32")
    return accum


def weighted_row_sum(W: Tensor, s: Tensor, scale: float = 1.0) -> Tensor:
    """scale * sum_n s[n] W[n, :] -> [d] f32, summed in a fixed order; rows with s[n] == 0 are not read
    (msae_weighted_row_sum_f32)."""
    dev = _hip.require_device(W, s)
    lib = _hip.load()
    Wc, sc = _f32c(W), _f32c(s)
    N, d = Wc.shape
    assert sc.numel() == N
    out = torch.empty(d, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.msae_weighted_row_sum_ws_bytes(N, d))
    with torch.cuda.device(dev):
        _hip.check(lib.msae_weighted_row_sum_f32(_hip.ptr(Wc), _hip.ptr(sc), N, d, float(scale), _hip.ptr(out), _hip.ptr(ws),
                                                 ws.numel(), _hip.stream_of(Wc)), "msae_weighted_row_sum_f32")
    return out


def sum_into_(accum: Tensor, v: Tensor) -> Tensor:
    """accum (f32 device scalar) += sum(v), summed in a fixed order (msae_sum_f32): the total of a weight gradient's
    per-row squared norms (collect_wgrad_sumsq)."""
    dev = _hip.require_device(accum, v)
    assert v.dtype == torch.float32 and v.is_contiguous() and accum.dtype == torch.float32 and accum.numel() == 1
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_sum_f32(_hip.ptr(v), v.numel(), _hip.ptr(accum), _hip.stream_of(v)), "msae_sum_f32")
    return accum


def _kernel_rows(p: Tensor) -> Tuple[int, int]:
    """[rows, d] as the Adam passes see a parameter: a matrix as it is, a vector as [numel / 1024, 1024] when that
    divides and as one row otherwise (any row length works without the projection)."""
    if p.dim() == 2:
        return p.shape[0], p.shape[1]
    d = 1024 if p.numel() % 1024 == 0 else p.numel()
    return p.numel() // d, d


def _opt_rows_args(p: Tensor, g: Tensor, moments: Sequence[Tensor], total_sumsq: Optional[Tensor], max_norm: float,
                   project: bool, renorm_eps: Optional[float], refresh: Optional[Tensor], tokens_next: int):
    """What the optimiser row passes share: the checks on p, g and the float32 `moments`, and the two runs of C arguments
    around an optimiser's own constants -> (device, head, tail).  head = rows, d, total_sumsq, max_norm, project;
    tail = renorm_eps, prepared, T_next, opts, stream (tail[-1:] is what a call without tails takes)."""
    dev = _hip.require_device(p, g, *moments, refresh)
    for t in (p, g, *moments):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == p.shape
    assert p.dim() == 2 or not project, "the projection is a row operation on a [rows, d] matrix"
    assert p.dim() == 2 or (renorm_eps is None and refresh is None), "renorm / refresh are row operations on a [rows, d] matrix"
    head = (*_kernel_rows(p), _hip.ptr(total_sumsq), float(max_norm), int(project))
    tail = (float(renorm_eps) if renorm_eps is not None else -1.0, _hip.ptr(refresh), int(tokens_next), _opts().ref(),
            _hip.stream_of(p))
    return dev, head, tail


def adam_rows_(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: int, lr: float, *,
               total_sumsq: Optional[Tensor] = None, max_norm: float = 1.0, project: bool = False,
               betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, renorm_eps: Optional[float] = None,
               refresh: Optional[Tensor] = None, tokens_next: int = 0) -> None:
    """One fused pass: clip by the global gradient norm, optionally remove the component of each
    gradient row parallel to the parameter row (sae.py:257-271), Adam update of p, m, v in place.
    `renorm_eps` (the decoder): rows divided by their norm + eps after the update -- the NEXT step's
    set_decoder_norm_to_unit_norm (sae.py:249-255), same bits, no extra sweep.  `refresh` (the encoder weight; a
    train_operand_buffer): the coarse-pass operands of the updated rows for the next encode of `tokens_next` tokens,
    as prepare_encoder(..., active_mode_only=True, tokens_next=...) would rebuild them (msae_adam_rows_fused_f32)."""
    dev, head, tail = _opt_rows_args(p, g, (m, v), total_sumsq, max_norm, project, renorm_eps, refresh, tokens_next)
    fused = renorm_eps is not None or refresh is not None
    name = "msae_adam_rows_fused_f32" if fused else "msae_adam_rows_f32"
    with torch.cuda.device(dev):
        _hip.check(getattr(_hip.load(), name)(
            _hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), *head, float(lr), float(betas[0]), float(betas[1]), float(eps),
            int(step), *(tail if fused else tail[-1:])), name)


def lion_rows_(p: Tensor, g: Tensor, m: Tensor, lr: float, *,
               total_sumsq: Optional[Tensor] = None, max_norm: float = 1.0, project: bool = False,
               betas: Tuple[float, float] = (0.9, 0.99), renorm_eps: Optional[float] = None,
               refresh: Optional[Tensor] = None, tokens_next: int = 0) -> None:
    """adam_rows_ with a sign-momentum update (msae_lion_rows_f32): same clip, projection, `renorm_eps` and `refresh` /
    `tokens_next` tails; p -= lr * sign(lerp(m, g, 1 - betas[0])), m = lerp(m, g, 1 - betas[1]) in place.  Lion; with
    betas[0] == betas[1] it is Signum.  One moment, no bias correction, no weight decay."""
    dev, head, tail = _opt_rows_args(p, g, (m,), total_sumsq, max_norm, project, renorm_eps, refresh, tokens_next)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_lion_rows_f32(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), *head, float(lr), float(betas[0]),
                                                  float(betas[1]), *tail), "msae_lion_rows_f32")


# ---- blockwise 8-bit Adam moments (the "adam8" format of include/msae.h) ---------------------------------
@dataclasses.dataclass
class Adam8State:
    """The Adam moments of one parameter in 8 bits: e4m3 codes of m (`m8`) and of sqrt(v) (`r8`), shaped like the
    parameter, and one float32 scale per block of 256 consecutive elements of a kernel row (`sm`, `sr`)."""
    m8: Tensor
    r8: Tensor
    sm: Tensor
    sr: Tensor

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors())

    def tensors(self) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        return self.m8, self.r8, self.sm, self.sr


def adam8_state(p: Tensor, *, _any_size: bool = False) -> Optional[Adam8State]:
    """A zeroed Adam8State for `p`, or None when its shape keeps float32 moments (msae_adam8_blocks: d % 4, d > 8192,
    fewer than 4096 elements, a vector 1024 does not divide).  `_any_size` is for the tests: it skips the 4096-element
    floor, which is policy and no limit of the kernel."""
    rows, d = _kernel_rows(p)
    nb = _hip.load().msae_adam8_blocks(rows, d)
    if nb == 0 and _any_size and d % 4 == 0:
        nb = rows * -(-d // 256)
    if nb == 0:
        return None
    return Adam8State(torch.zeros(p.shape, dtype=torch.uint8, device=p.device), torch.zeros(p.shape, dtype=torch.uint8, device=p.device),
                      torch.zeros(nb, dtype=torch.float32, device=p.device), torch.zeros(nb, dtype=torch.float32, device=p.device))


def _adam8_args(state: Adam8State, like: Tensor):
    rows, d = _kernel_rows(like)
    for t in (state.m8, state.r8):
        assert t.dtype == torch.uint8 and t.is_contiguous() and t.shape == like.shape
    for t in (state.sm, state.sr):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == rows * -(-d // 256)
    return [_hip.ptr(t) for t in state.tensors()], rows, d


def adam8_rows_(p: Tensor, g: Tensor, state: Adam8State, step: int, lr: float, *,
                total_sumsq: Optional[Tensor] = None, max_norm: float = 1.0, project: bool = False,
                betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, renorm_eps: Optional[float] = None,
                refresh: Optional[Tensor] = None, tokens_next: int = 0) -> None:
    """adam_rows_ with the moments carried in an Adam8State (msae_adam8_rows_f32): same clip, projection, update, renorm
    and operand refresh; the update uses this step's float32 moments, the state keeps their 8-bit codes.  Raises
    _hip.MsaeNotImplemented for a shape the kernel does not take."""
    _hip.require_device(p, *state.tensors())
    dev, head, tail = _opt_rows_args(p, g, (), total_sumsq, max_norm, project, renorm_eps, refresh, tokens_next)
    ptrs, _, _ = _adam8_args(state, p)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_adam8_rows_f32(_hip.ptr(p), _hip.ptr(g), *ptrs, *head, float(lr), float(betas[0]),
                                                   float(betas[1]), float(eps), int(step), *tail), "msae_adam8_rows_f32")


def adam8_quantize(m: Tensor, v: Tensor) -> Adam8State:
    """float32 moments -> an Adam8State (msae_adam8_quantize_f32); raises _hip.MsaeNotImplemented for a shape the
    format does not take."""
    dev = _hip.require_device(m, v)
    for t in (m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == m.shape
    state = adam8_state(m, _any_size=True)
    if state is None:
        _hip.check(-4, "adam8_quantize")
    ptrs, rows, d = _adam8_args(state, m)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_adam8_quantize_f32(_hip.ptr(m), _hip.ptr(v), *ptrs, rows, d, _hip.stream_of(m)),
                   "msae_adam8_quantize_f32")
    return state


def adam8_dequantize(state: Adam8State) -> Tuple[Tensor, Tensor]:
    """-> (m, v) float32, shaped like the parameter: the values adam8_rows_ computes with (msae_adam8_dequantize_f32)."""
    dev = _hip.require_device(*state.tensors())
    m = torch.empty(state.m8.shape, dtype=torch.float32, device=dev)
    v = torch.empty_like(m)
    ptrs, rows, d = _adam8_args(state, m)
    with torch.cuda.device(dev):
        _hip.check(_hip.load().msae_adam8_dequantize_f32(*ptrs, _hip.ptr(m), _hip.ptr(v), rows, d, _hip.stream_of(m)),
                   "msae_adam8_dequantize_f32")
    return m, v
