"""Forward-hook bodies that splice the SAE reconstruction into the LLM, on the fused path.

Reference hooks replaced (behaviour identical, dense `[T, N]` latents never materialised):
  * steering     features/steering.py:102-128 (dup. tools/model_steering.py:62-79):
        latents = pre_acts(h); if S != 1: latents[:, :, f] = clamp; topk; decode(top[0]) -> fp16
  * attribution  features/patching/utils.py:33-58:
        latents = pre_acts(h.flatten(0,1)); latents[:, off] *= 0; topk; decode -> fp16 view(B,S,d)
The latent edits are arguments of the fused encode kernel (`set_feature`, `zero_feature`); a LIST of features -- the
reference's indexing takes one -- goes through `FeatureEdits`: an over-fetching encode and the list edit kernel
(msae/features/edits.py).
"""
from __future__ import annotations

from typing import Callable, Dict, Mapping, Optional, Sequence

import torch
from torch import Tensor

from ..sae import Sae
from .edits import EDIT_MODES, FeatureEdits, RowEdits, as_off_features


def _topk_sae_only(sae, what: str) -> None:
    """The steering and attribution hooks edit per-token top-k lists: not built for a "batchtopk" or "jump" Sae (DESIGN.md
    section 8)."""
    if getattr(getattr(sae, "cfg", None), "activation", "topk") == "batchtopk":
        raise NotImplementedError(f"{what} is not built for an Sae with activation='batchtopk': the hooks edit per-token "
                                  "top-k lists (Sae.encode(threshold=) + Sae.decode(lengths=) are its inference path)")
    if getattr(getattr(sae, "cfg", None), "activation", "topk") == "jump":
        raise NotImplementedError(f"{what} is not built for an Sae with activation='jump': the hooks edit per-token "
                                  "top-k lists (Sae.encode + Sae.decode(lengths=) are its inference path)")


def _autoencoder_only(sae, what: str) -> None:
    """These hooks replace a layer's output by a reconstruction of that SAME output: a transcoder (SaeConfig.transcode)
    predicts a module's output from its INPUT and is spliced in by `transcoder_hook`."""
    if getattr(getattr(sae, "cfg", None), "transcode", False):
        raise ValueError(f"{what} replaces a layer's output by a reconstruction of that same output; this Sae is a transcoder "
                         "(SaeConfig.transcode): splice it in with msae.features.hooks.transcoder_hook / Sae.transcode")


def sae_reconstruct(sae, hidden: Tensor, *, set_feature: int = -1, set_value: float = 0.0,
                    zero_feature: int = -1, out_dtype: Optional[torch.dtype] = None,
                    differentiable: Optional[bool] = None, edits: Optional[FeatureEdits] = None,
                    edit_group: Optional[Tensor] = None, preserve_error: bool = False) -> Tensor:
    """[..., d] hidden states -> SAE reconstruction of the same shape.  `sae` is an `Sae` module or a
    feature-sharded engine (msae.parallel.ShardedSae over an N/G slice of the encoder per rank, SURVEY 8f rank 4:
    "N-sharded across 8 GPUs"; every rank must hold the same hidden states): same edits, by GLOBAL feature id, same
    bits out.  `edits`: a set of edits instead of the scalar arguments (single-GPU `Sae` only); with a `RowEdits`,
    `edit_group` as in `Sae.encode` (None: row b of a [G, S, d] input uses group b).

    `preserve_error=True` (single-GPU `Sae` only) returns hidden + (decode(encode(hidden, edits)) -
    decode(encode(hidden))) in the hidden state's OWN dtype instead: the reconstruction error is carried along, so a
    position no edit touches comes out bit-identical to the input (`out_dtype` with it is a ValueError).  Under no_grad it
    is `Sae.intervene` with an edit (a scalar set_feature / zero_feature becomes a one-entry FeatureEdits: the hooks build it
    once, at registration) and the hidden state itself -- no SAE call -- without one.  Under autograd it is
    out = y_Q + (hidden - y_P).detach() from the differentiable encode and decode, y_P from a no_grad plain encode (y_Q.detach()
    when nothing is edited): the error term is a constant of the forward, so the gradients with respect to the latents and
    the SAE's parameters are exactly the reconstruct path's.  Its values agree with the fused path's within the derived
    bound of tests/intervene_ref.py (the cancelled entries round differently), not bitwise."""
    _autoencoder_only(sae, "sae_reconstruct")
    _topk_sae_only(sae, "sae_reconstruct")
    if preserve_error:
        return _reconstruct_preserving(sae, hidden, set_feature, set_value, zero_feature, out_dtype, differentiable, edits,
                                       edit_group)
    flat = hidden.reshape(-1, hidden.shape[-1])
    if isinstance(edits, RowEdits) or edit_group is not None:
        if not isinstance(sae, Sae):
            raise NotImplementedError("per-row edits run on the single-GPU msae.Sae only: a feature-sharded engine takes "
                                      "one feature")
        # (the groups are resolved against the UNFLATTENED input: "row b uses group b" is a statement about [G, S, d])
        top = sae.encode(hidden, differentiable=differentiable, edits=edits, edit_group=edit_group)
        k = top.top_acts.shape[-1]
        out = sae.decode(top.top_acts.reshape(-1, k), top.top_indices.reshape(-1, k))
    elif isinstance(sae, Sae):
        top = sae.encode(flat, set_feature=set_feature, set_value=set_value, zero_feature=zero_feature,
                         differentiable=differentiable, edits=edits)
        out = sae.decode(top.top_acts, top.top_indices)
    else:   # engine interface: encode -> (acts, global ids, status), decode(acts, ids)
        ed = {} if edits is None else {"edits": edits}      # (an engine raises NotImplementedError on a set of edits)
        acts, idx, _ = sae.encode(flat.contiguous(), set_feature=set_feature, set_value=set_value,
                                  zero_feature=zero_feature, **ed)
        out = sae.decode(acts, idx)
    return out.to(out_dtype or hidden.dtype).view(hidden.shape)


def _scalar_edits(sae, set_feature: int, set_value: float, zero_feature: int) -> Optional[FeatureEdits]:
    """The scalar hook arguments as a FeatureEdits (ZERO over SET, as the kernel applies them), or None without an edit."""
    if set_feature < 0 and zero_feature < 0:
        return None
    return FeatureEdits(sae.num_latents, set={int(set_feature): float(set_value)} if set_feature >= 0 else None,
                        zero=[int(zero_feature)] if zero_feature >= 0 else None, device=sae.device)


def _reconstruct_preserving(sae, hidden: Tensor, set_feature: int, set_value: float, zero_feature: int, out_dtype,
                            differentiable, edits, edit_group) -> Tensor:
    """sae_reconstruct(preserve_error=True): see there."""
    if out_dtype is not None:
        raise ValueError("sae_reconstruct: preserve_error=True returns the hidden state's own dtype (unedited positions come "
                         "out identical to the input); it does not take out_dtype")
    if not isinstance(sae, Sae):
        raise NotImplementedError("preserve_error runs on the single-GPU msae.Sae only: a feature-sharded engine "
                                  "reconstructs (preserve_error=False)")
    if edits is not None and (set_feature >= 0 or zero_feature >= 0):
        raise ValueError("sae_reconstruct: pass either edits= or the scalar set_feature / zero_feature arguments, not both")
    if edit_group is not None and not isinstance(edits, RowEdits):
        raise ValueError("sae_reconstruct: edit_group names the groups of a RowEdits")
    if differentiable is None:
        differentiable = hidden.requires_grad
    if not (torch.is_grad_enabled() and differentiable):
        if edits is None:
            edits = _scalar_edits(sae, set_feature, set_value, zero_feature)
        if edits is None:
            return hidden                       # nothing edited: the model is left untouched, exactly
        with torch.no_grad():
            return sae.intervene(hidden, edits, edit_group)
    # autograd: today's differentiable reconstruction of the edited latents plus a CONSTANT error term
    k = sae.cfg.k
    shaped = hidden if isinstance(edits, RowEdits) else hidden.reshape(-1, hidden.shape[-1])
    top = sae.encode(shaped, set_feature=set_feature, set_value=set_value, zero_feature=zero_feature, differentiable=True,
                     edits=edits, edit_group=edit_group)
    y_q = sae.decode(top.top_acts.reshape(-1, k), top.top_indices.reshape(-1, k)).view(hidden.shape)
    if edits is None and set_feature < 0 and zero_feature < 0:
        y_p = y_q.detach()
    else:
        with torch.no_grad():
            plain = sae.encode(hidden.detach().reshape(-1, hidden.shape[-1]))
            y_p = sae.decode(plain.top_acts, plain.top_indices).view(hidden.shape)
    return (y_q + (hidden.detach().to(y_q.dtype) - y_p)).to(hidden.dtype)


def _replace_first(outputs, new0):
    if isinstance(outputs, tuple):
        return (new0,) + tuple(outputs[1:])
    return new0


class _DecodeStepGraph:
    """The S = 1 step of the steering hook -- encode, decode, cast: ~8 kernel launches through two custom ops -- captured ONCE
    into a HIP graph and replayed (round-5 verdict, item 9).  A generation step of an 8B model is host-bound; the hook's two
    op dispatches + ctypes calls (~17 us each) sit on that critical path up to 512 times per feature
    (features/steering.py:86).  A replay is one copy into the captured input and one graph launch.

    The library's entry points allocate nothing and never synchronise, which is what makes them capturable
    (tests/test_gpu_parity.py::test_encode_and_decode_replay_from_a_hip_graph).  The graph holds raw pointers, so it is keyed on
    everything it captured -- the prepared operand buffer, the parameters' storage and versions, the workspace epoch
    (ops.release_workspaces) -- and re-captured when any of them changes; a capture that fails once (an exotic build, a
    stream in capture already) switches the hook to the eager path for good.  The replayed dither seed is the captured one:
    fine for inputs that do not know it (include/msae.h)."""

    def __init__(self):
        self.key = None
        self.graph = None
        self.x = self.out = None
        self.keep = None
        self.failed = False

    @staticmethod
    def _key(sae, h: Tensor):
        from .. import ops

        w, bias, wd, bd = sae.encoder.weight, sae.encoder.bias, sae.W_dec, sae.b_dec
        prep = sae._prepared_weights()
        return (h.dtype, h.device, tuple(h.shape), ops.workspace_epoch(), 0 if prep is None else prep.data_ptr(),
                w.data_ptr(), w._version, bias.data_ptr(), bias._version, wd.data_ptr(), wd._version, bd.data_ptr(), bd._version,
                ops._defaults.coarse, ops._defaults.guard_z, ops._defaults.exact, getattr(ops._defaults, "certified", False))

    def __call__(self, sae, h: Tensor) -> Optional[Tensor]:
        """h [B, d] (B = 1: clamp_features_max; one step of B rows: clamp_features_rows) -> fp16 reconstruction [B, d] (a
        fresh tensor), or None: take the eager path.  The key holds the shape: another B is another capture."""
        if self.failed or torch.cuda.is_current_stream_capturing():
            return None
        key = self._key(sae, h)
        if key != self.key:
            try:
                self._capture(sae, h, key)
            except Exception:  # noqa: BLE001 -- any capture problem: the eager path is always right
                self.failed, self.graph, self.key = True, None, None
                return None
        self.x.copy_(h)
        self.graph.replay()
        return self.out.clone()

    def _capture(self, sae, h: Tensor, key) -> None:
        body = lambda t: sae_reconstruct(sae, t, out_dtype=torch.float16)
        x = h.clone()
        with torch.cuda.device(h.device):            # (a hook on a layer of another device than the current one)
            side = torch.cuda.Stream(device=h.device)
            side.wait_stream(torch.cuda.current_stream(h.device))
            with torch.cuda.stream(side):
                for _ in range(2):                   # workspaces and the prepared operands exist before the capture
                    body(x)
            torch.cuda.current_stream(h.device).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                out = body(x)
        self.graph, self.x, self.out, self.key = g, x, out, key
        # what the graph captured by address stays alive as long as the graph does: the operand buffer and the side stream's
        # scratch buffer (ops._workspace keeps only the most recently used streams' buffers)
        from .. import ops

        self.keep = (sae._prepared_weights(), ops._WS.get((h.device, side.cuda_stream)), side)


def _check_mode(mode, what: str) -> str:
    if mode not in EDIT_MODES:
        raise ValueError(f"{what}: mode must be one of {EDIT_MODES}, got {mode!r}")
    return mode


def _steering_edits(sae, feature, k: float, mode: str = "set"):
    """`feature` of clamp_features_max -> (set_feature for the in-kernel scalar route or -1, FeatureEdits or None).  A mode
    other than "set" (scale / add / floor / cap: `k` is the edit's parameter) always takes the
    FeatureEdits route: the in-kernel scalar edit is a SET."""
    _check_mode(mode, "clamp_features_max")
    if isinstance(feature, FeatureEdits):
        return -1, feature
    if isinstance(feature, Mapping):
        table = feature
    elif isinstance(feature, Tensor) and feature.dim() > 0:
        table = {int(f): float(k) for f in feature.reshape(-1).tolist()}
    elif isinstance(feature, (list, tuple, range)) or (hasattr(feature, "__iter__") and not isinstance(feature, Tensor)):
        table = {int(f): float(k) for f in feature}
    elif mode == "set":
        return int(feature), None                   # today's path, unchanged
    else:
        table = {int(feature): float(k)}
    if not isinstance(sae, Sae):
        raise NotImplementedError("clamping a set of features, and every mode but 'set', runs on the single-GPU msae.Sae "
                                  "only: a feature-sharded engine sets one feature")
    return -1, FeatureEdits(sae.num_latents, device=sae.device, **{mode: table})


def clamp_features_max(sae, feature, hooked_module: torch.nn.Module, k: float = 10, graph_step: Optional[bool] = None,
                       preserve_error: bool = False, mode: str = "set"):
    """Register the steering hook (steering.py:102-128): on prefill (S != 1) the feature's latent
    is set to `k` before TopK; every call replaces the layer output by the fp16 reconstruction.
    `feature`: an int (the in-kernel edit), a sequence or tensor of ints (`latents[:, :, f] = k` with a list: all
    clamped to `k`), or a mapping feature -> value; a set is uploaded once, here, as a FeatureEdits.
    `sae`: an `Sae`, or a `ShardedSae` engine (the S = 1 decode steps then stream N/G rows of the encoder per rank
    and exchange 8 k_loc bytes; the decode of so few tokens is local on every rank).
    `graph_step`: replay the S = 1 step from a captured HIP graph (_DecodeStepGraph); default: on for a single-GPU `Sae`
    under no_grad unless MSAE_HOOK_GRAPH=0.
    `preserve_error` (single-GPU `Sae` only): the prefill output is h + the decoded EDIT in h's own
    dtype (`Sae.intervene`), the S = 1 steps return the layer output unchanged -- no SAE call, no captured graph.
    `mode` (single-GPU `Sae` only unless "set"): what `k`, or a mapping's value, does to the feature's
    own latent c on prefill -- "set" (c := k, the reference's clamp), "scale" (c k), "add" (c + k), "floor" (max(c, k)),
    "cap" (min(c, k)); it applies to an int, a sequence or a mapping, not to a prebuilt FeatureEdits."""
    import os

    _autoencoder_only(sae, "clamp_features_max")
    _topk_sae_only(sae, "clamp_features_max")
    if preserve_error:
        return _clamp_preserving(sae, hooked_module, _preserving_edits(sae, feature, k, mode))
    if graph_step is None:
        graph_step = os.environ.get("MSAE_HOOK_GRAPH", "1") not in ("0", "")
    step_graph = _DecodeStepGraph() if (graph_step and isinstance(sae, Sae)) else None
    set_feature, edits = _steering_edits(sae, feature, k, mode)

    def hook(module, _, outputs):
        h = outputs[0] if isinstance(outputs, tuple) else outputs
        prefill = h.shape[1] != 1
        if (step_graph is not None and not prefill and h.shape[0] == 1 and h.is_cuda and not torch.is_grad_enabled()
                and not sae.training):
            out = step_graph(sae, h[0])
            if out is not None:
                return _replace_first(outputs, out.unsqueeze(0))
        out = sae_reconstruct(sae, h[0], set_feature=set_feature if prefill else -1, set_value=float(k),
                              out_dtype=torch.float16, edits=edits if prefill else None).unsqueeze(0)
        return _replace_first(outputs, out)

    handle = hooked_module.register_forward_hook(hook)
    handle.step_graph = step_graph          # (diagnostics / tests: the captured S = 1 step, or None)
    return [handle]


def _preserving_edits(sae, feature, k: float, mode: str = "set") -> FeatureEdits:
    """`feature` of clamp_features_max(preserve_error=True) -> the FeatureEdits of the prefill, built once."""
    if not isinstance(sae, Sae):
        raise NotImplementedError("preserve_error runs on the single-GPU msae.Sae only: a feature-sharded engine "
                                  "reconstructs (preserve_error=False)")
    set_feature, edits = _steering_edits(sae, feature, k, mode)
    return edits if edits is not None else _scalar_edits(sae, set_feature, float(k), -1)


def _clamp_preserving(sae, hooked_module: torch.nn.Module, edits):
    """The error-preserving steering hook of both clamps: prefill through Sae.intervene, S = 1 steps untouched."""
    rows = isinstance(edits, RowEdits)

    def hook(module, _, outputs):
        h = outputs[0] if isinstance(outputs, tuple) else outputs
        if h.shape[1] == 1:                     # a decode step: no clamp there, so nothing to add
            return outputs
        if rows and h.shape[0] != edits.G:
            raise ValueError(f"clamp_features_rows: {edits.G} rows of features, a batch of {h.shape[0]}")
        return _replace_first(outputs, sae_reconstruct(sae, h, edits=edits, preserve_error=True))

    handle = hooked_module.register_forward_hook(hook)
    handle.step_graph = None                    # (no _DecodeStepGraph: the S = 1 step makes no SAE call)
    handle.edits = edits
    return [handle]


def _row_spec(element, k: float, mode: str = "set"):
    """One element of clamp_features_rows' `features` -> a RowEdits group (None, a FeatureEdits or a dict spec)."""
    if element is None or isinstance(element, FeatureEdits):
        return element
    if isinstance(element, Mapping):
        return {mode: element}
    if isinstance(element, Tensor):
        element = element.reshape(-1).tolist()
    if isinstance(element, (list, tuple, range)):
        return {mode: {int(f): float(k) for f in element}} if len(element) else None
    return {mode: {int(element): float(k)}}


def clamp_features_rows(sae, features: Sequence, hooked_module: torch.nn.Module, k: float = 10,
                        graph_step: Optional[bool] = None, preserve_error: bool = False, mode="set"):
    """The steering hook for a BATCH whose rows steer different features: `features` has one element
    per batch row -- an int, a list of ints (all clamped to `k`), a mapping feature -> value, or None for an unedited row
    (the batch's baseline).  On prefill (S != 1) row b's latents are clamped per element b before TopK; every call replaces
    the whole [B, S, d] layer output by the fp16 reconstruction.  The tables are validated and uploaded once, here, as a
    RowEdits.  The S = 1 step of the batch ([B, 1, d], no edit) replays from a captured HIP graph like clamp_features_max's
    (`graph_step`: default on under no_grad unless MSAE_HOOK_GRAPH=0).  Single-GPU `Sae` only.  The prefill's batch size
    must equal len(features) (ValueError).  `preserve_error`: as in clamp_features_max -- row b's prefill output is
    h[b] + its decoded edit, a row of None and every S = 1 step keep the layer's output bit for bit.  `mode`: as in
    clamp_features_max, one string for every row or a sequence with one string per row."""
    import os

    if not isinstance(sae, Sae):
        raise NotImplementedError("clamp_features_rows runs on the single-GPU msae.Sae only: a feature-sharded engine takes "
                                  "one feature (clamp_features_max)")
    _autoencoder_only(sae, "clamp_features_rows")
    _topk_sae_only(sae, "clamp_features_rows")
    if isinstance(features, (Mapping, Tensor, str)) or not hasattr(features, "__len__"):
        raise ValueError("clamp_features_rows: features must be a sequence with one element per batch row")
    if graph_step is None:
        graph_step = os.environ.get("MSAE_HOOK_GRAPH", "1") not in ("0", "")
    if isinstance(mode, str):
        modes = [_check_mode(mode, "clamp_features_rows")] * len(features)
    else:
        modes = [_check_mode(m, "clamp_features_rows") for m in mode]
        if len(modes) != len(features):
            raise ValueError(f"clamp_features_rows: {len(features)} rows of features, {len(modes)} modes")
    edits = RowEdits(sae.num_latents, [_row_spec(f, k, m) for f, m in zip(features, modes)], device=sae.device)
    if preserve_error:
        return _clamp_preserving(sae, hooked_module, edits)
    step_graph = _DecodeStepGraph() if graph_step else None

    def hook(module, _, outputs):
        h = outputs[0] if isinstance(outputs, tuple) else outputs
        if h.shape[1] != 1:
            if h.shape[0] != edits.G:
                raise ValueError(f"clamp_features_rows: {edits.G} rows of features, a batch of {h.shape[0]}")
            return _replace_first(outputs, sae_reconstruct(sae, h, out_dtype=torch.float16, edits=edits))
        if step_graph is not None and h.is_cuda and not torch.is_grad_enabled() and not sae.training:
            out = step_graph(sae, h[:, 0])
            if out is not None:
                return _replace_first(outputs, out.unsqueeze(1))
        return _replace_first(outputs, sae_reconstruct(sae, h, out_dtype=torch.float16))

    handle = hooked_module.register_forward_hook(hook)
    handle.step_graph = step_graph          # (diagnostics / tests: the captured S = 1 step, or None)
    handle.edits = edits
    return [handle]


def attribution_sae_hook(sae_dict: Dict[str, Sae], module_to_name: Dict[torch.nn.Module, str],
                         cache: Dict[str, Tensor], off_features=None, edit_group: Optional[Tensor] = None,
                         preserve_error: bool = False) -> Callable:
    """Hook body of get_model_forward_cache_with_sae (patching/utils.py:33-58).  `off_features`: None, an int, or a
    sequence / tensor of ints (`mask[:, off_features] = 0` takes any of them); or a RowEdits with `edit_group` as in
    `Sae.encode`: another ablation per batch row.  `preserve_error`: the layer output is
    h + (decode(ablated) - decode(plain)) in h's own dtype -- the ablation's effect in the model itself, not in a model that
    runs on reconstructions; sae_reconstruct states the autograd rule."""
    per_module: dict = {}         # a list of features becomes one FeatureEdits per hooked Sae, built at its first call
    for sae in sae_dict.values():
        _autoencoder_only(sae, "attribution_sae_hook")
        _topk_sae_only(sae, "attribution_sae_hook")

    def hook(module, inputs, outputs):
        h = outputs[0] if isinstance(outputs, tuple) else outputs
        name = module_to_name[module]
        sae = sae_dict[name]
        if name not in per_module:
            zero, edits = as_off_features(off_features, sae)
            if preserve_error and zero >= 0:    # the scalar route as a one-entry table, built once per hooked Sae
                if not isinstance(sae, Sae):
                    raise NotImplementedError("preserve_error runs on the single-GPU msae.Sae only")
                zero, edits = -1, _scalar_edits(sae, -1, 0.0, zero)
            per_module[name] = (zero, edits)
        zero, edits = per_module[name]
        if preserve_error:
            out = sae_reconstruct(sae, h, edits=edits, edit_group=edit_group, differentiable=torch.is_grad_enabled(),
                                  preserve_error=True)
        else:
            out = sae_reconstruct(sae, h, zero_feature=zero, edits=edits, edit_group=edit_group,
                                  out_dtype=torch.float16, differentiable=torch.is_grad_enabled())
        cache[name] = out
        return _replace_first(outputs, out)

    return hook


def transcoder_hook(sae: Sae, module: torch.nn.Module, edits=None, out_dtype: Optional[torch.dtype] = None):
    """Splice a transcoder (SaeConfig.transcode) in place of `module`: a forward hook that replaces the
    module's OUTPUT by `sae.transcode(module input)` -- the first positional input [B, S, d_in] -> [B, S, d_out] in
    `out_dtype` (None: the replaced output's own dtype).  `edits` (a FeatureEdits, or a RowEdits whose group b is batch row
    b) apply on prefill only (S != 1), as the clamps' do; every call, the S = 1 steps included, runs eagerly (a captured
    S = 1 step is a follow-up: DESIGN.md section 8).  Inference only."""
    if not isinstance(sae, Sae) or not sae.cfg.transcode:
        raise ValueError("transcoder_hook takes a transcoder (an msae.Sae with SaeConfig.transcode): an auto-encoder is spliced "
                         "in on a layer's output (clamp_features_max, sae_splice_hook)")
    if edits is not None:
        edits.check(sae.num_latents, sae.cfg.k, sae.device)

    def hook(mod, inputs, outputs):
        if not inputs:
            raise ValueError("transcoder_hook: the hooked module was called without a positional input")
        x = inputs[0]
        old = outputs[0] if isinstance(outputs, tuple) else outputs
        prefill = x.dim() < 3 or x.shape[1] != 1
        with torch.no_grad():
            out = sae.transcode(x.detach(), edits=edits if prefill else None)
        return _replace_first(outputs, out.to(out_dtype or old.dtype))

    handle = module.register_forward_hook(hook)
    handle.step_graph = None                    # (eager on every call)
    handle.edits = edits
    return [handle]
