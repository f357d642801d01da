"""SteeringController -- per-feature clamped generation (reference features/steering.py:13-128).
The forward hook is `msae.features.hooks.clamp_features_max` (fused encode with the clamp applied
inside the kernel); generation itself is HF `generate`.  `batch_features=B` puts B features into the rows of ONE
`generate` (`clamp_features_rows`: another clamp per batch row)."""
from __future__ import annotations

import os
from typing import List

import torch

from ..sae import Sae
from .edits import EDIT_MODES
from .hooks import clamp_features_max, clamp_features_rows


class SteeringController:
    """`sae`: an `Sae`, or a feature-sharded `msae.parallel.ShardedSae` engine -- then EVERY rank of the engine's
    group must run the same controller on the same prompt and feature list (they meet in the engine's collectives
    at every hooked forward).
    `batch_features` = B > 1 (single-GPU `Sae` only): `run()` takes the feature list in chunks of B, repeats the
    processor's inputs along the batch, generates once per chunk and decodes each row; same result keys and values as
    the default B = 1, which runs the reference's loop unchanged.  The rows share one prompt.
    `preserve_error` (single-GPU `Sae` only): the hooks add the decoded clamp to the layer's own output
    instead of replacing it by the reconstruction, so `clamped_resps` differs from `original_resps` -- the un-hooked model --
    by the edit alone.
    `mode` (single-GPU `Sae` only unless "set"): what `k` does to the steered feature's own latent c on
    the prompt -- "set" (the reference's clamp, at every position), "scale" (c k: amplify it where it fires), "add",
    "floor", "cap"."""

    def __init__(self, sae, module_name: str, feature_idx: List[int], model, processor,
                 prompt: str, image_path: str = None, k: float = 50, batch_features: int = 1,
                 preserve_error: bool = False, mode: str = "set"):
        if mode not in EDIT_MODES:
            raise ValueError(f"mode must be one of {EDIT_MODES}, got {mode!r}")
        if mode != "set" and not isinstance(sae, Sae):
            raise NotImplementedError(f"mode={mode!r} runs on the single-GPU msae.Sae only: a feature-sharded engine sets "
                                      "one feature")
        self.mode = mode
        if int(batch_features) < 1:
            raise ValueError(f"batch_features must be >= 1, got {batch_features}")
        if int(batch_features) > 1 and not isinstance(sae, Sae):
            raise NotImplementedError("batch_features > 1 runs on the single-GPU msae.Sae only: a feature-sharded engine "
                                      "takes one feature per generation")
        if preserve_error and not isinstance(sae, Sae):
            raise NotImplementedError("preserve_error runs on the single-GPU msae.Sae only: a feature-sharded engine "
                                      "reconstructs")
        self.batch_features = int(batch_features)
        self.preserve_error = bool(preserve_error)
        self.sae, self.feature_idx, self.model, self.k = sae, feature_idx, model, k
        self.module_name, self.processor = module_name, processor
        self.hooked_module = model.language_model.get_submodule(module_name)
        local_rank = os.environ.get("LOCAL_RANK")
        self.ddp = local_rank is not None
        self.rank = int(local_rank) if local_rank is not None else 0
        content = [{"type": "text", "text": prompt}]
        self.image = None
        if image_path is not None:
            from PIL import Image

            self.image = Image.open(image_path)
            content.append({"type": "image"})
        self.prompt = processor.apply_chat_template([{"role": "user", "content": content}],
                                                    add_generation_prompt=True)
        self.inputs = processor(images=self.image, text=self.prompt, return_tensors="pt").to(model.device)

    def clamp_features_max(self, sae, feature: int, hooked_module, k: float = 10):
        kw = {} if self.mode == "set" else {"mode": self.mode}
        if self.preserve_error:
            return clamp_features_max(sae, feature, hooked_module, k=k, preserve_error=True, **kw)
        return clamp_features_max(sae, feature, hooked_module, k=k, **kw)

    def _generate(self) -> str:
        kw = {}
        world = getattr(self.sae, "world", 1)
        if not isinstance(self.sae, Sae) and world > 1:
            # feature-sharded engine: all ranks meet in its collectives at every hooked forward, so their generation
            # loops must take the same number of steps.  Same RNG state on every rank (the model's generation_config
            # may sample), and HF's `synced_gpus`: a rank whose sequence hit EOS keeps stepping until all have.
            # -- seeded ONCE per controller (re-seeding in every _generate made every sampled steering
            # generation replay the same random stream); later generations continue the ranks' common stream
            if not getattr(self, "_ranks_seeded", False):
                torch.manual_seed(0x5AE)
                self._ranks_seeded = True
            kw["synced_gpus"] = True
        with torch.no_grad():
            output = self.model.generate(**self.inputs, max_new_tokens=512, **kw)
        cont = output[:, self.inputs["input_ids"].shape[-1]:]
        return self.processor.batch_decode(cont, skip_special_tokens=True)[0]

    def _generate_rows(self, n: int) -> List[str]:
        """One generation of the prompt repeated n times along the batch -> the n continuations."""
        inputs = {}
        for key, v in self.inputs.items():
            if isinstance(v, torch.Tensor):
                inputs[key] = v.repeat(n, *([1] * (v.dim() - 1)))
            elif isinstance(v, (list, tuple)):
                inputs[key] = type(v)(list(v) * n)
            else:
                inputs[key] = v
        kw = {}
        # rows that end early are padded: HF generate needs a pad id for that, the processor's tokenizer has it
        pad = getattr(getattr(self.processor, "tokenizer", None), "pad_token_id", None)
        if pad is not None and getattr(getattr(self.model, "generation_config", None), "pad_token_id", None) is None:
            kw["pad_token_id"] = pad
        with torch.no_grad():
            output = self.model.generate(**inputs, max_new_tokens=512, **kw)
        cont = output[:, self.inputs["input_ids"].shape[-1]:]
        return self.processor.batch_decode(cont, skip_special_tokens=True)

    def _run_batched(self, original: str) -> dict:
        results, B = {}, self.batch_features
        feats = list(self.feature_idx)
        for lo in range(0, len(feats), B):
            chunk = feats[lo:lo + B]                 # (a short last chunk generates a smaller batch)
            handles = clamp_features_rows(self.sae, chunk, self.hooked_module, k=self.k,
                                          **({"preserve_error": True} if self.preserve_error else {}),
                                          **({} if self.mode == "set" else {"mode": self.mode}))
            try:
                texts = self._generate_rows(len(chunk))
            finally:
                for h in handles:
                    h.remove()
            for idx, clamped in zip(chunk, texts):
                results[f"{self.module_name}_feature{idx}"] = {
                    "original_resps": original, "clamped_resps": clamped, "idx": idx}
        return results

    def run(self) -> dict:
        original = self._generate()
        if self.batch_features > 1:
            return self._run_batched(original)
        results = {}
        for idx in self.feature_idx:
            handles = self.clamp_features_max(self.sae, idx, self.hooked_module, k=self.k)
            try:
                clamped = self._generate()
            finally:
                for h in handles:
                    h.remove()
            results[f"{self.module_name}_feature{idx}"] = {
                "original_resps": original, "clamped_resps": clamped, "idx": idx}
        return results
