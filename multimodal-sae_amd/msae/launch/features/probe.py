"""python -m msae.launch.features.probe -m <model> --sae-path ... --module-name model.layers.24 -i <image> [-i <image> ...]
[-t <text>] -k 10 [--interval a-b] -s <save dir>   (reference tools/probe_activations.py).

Which SAE features an image (or a prompt) activates, and where: the hooked layer's output is captured for every input, and
ONE Sae.probe call ranks the features of each input (one segment per input) by their mean activation over its tokens and
returns the chosen features' per-token activations.  Writes
  filters.json           {module: [feature idx, ...]}: the input for the cache / explain / steering launchers (the union of
                         every input's ranking, in order of first appearance)
  probe.json             {module: [{"image", "text", "indices", "values"}, ...]}: each input's ranking
  images/feat_{idx}.png  the activation mask over the base image (one image), images/<n>/feat_{idx}.png (several)."""
from __future__ import annotations

import argparse
import json
import os
from typing import List, Optional, Tuple

import torch

from ...features.images import activation_images
from ...utils import ddp_setup, load_single_sae, maybe_load_llava_model


def parse_argument(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model", "-m", type=str, default="llava-hf/llama3-llava-next-8b-hf",
                   help="The model name of your trained model")
    p.add_argument("--sae-path", type=str, help="The path to your sae, can be hub or local")
    p.add_argument("--module-name", type=str, default="model.layers.24", help="The module name of your sae")
    p.add_argument("--image-path", "-i", type=str, action="append", default=None,
                   help="The path to your image (repeat for several: they are probed as one batch, one segment each)")
    p.add_argument("--text", "-t", type=str, default=None, help="The text you want to ask the model")
    p.add_argument("--top-k", "-k", type=int, default=10, help="The top k features you want to probe")
    p.add_argument("--interval", type=str, default=None,
                   help="The interval of top k features, e.g. 10-20 probes the features ranked 10 to 20 (0-based, end "
                        "exclusive)")
    p.add_argument("--save-to", "-s", type=str, default="./results/probe_activations",
                   help="The path to store your stored_activations")
    return p.parse_args(argv)


def interval_of(args) -> Tuple[int, int]:
    """[first, end) of the ranking to keep: --interval a-b, else [0, top_k) (tools/probe_activations.py:79-82)."""
    if args.interval is None:
        return 0, args.top_k
    parts = [int(i) for i in args.interval.split("-")]
    if len(parts) != 2 or not 0 <= parts[0] < parts[1]:
        raise ValueError(f"--interval must be a-b with 0 <= a < b, got {args.interval!r}")
    return parts[0], parts[1]


def build_prompt(processor, text: Optional[str], has_image: bool) -> str:
    """The chat-template prompt of tools/probe_activations.py:87-106."""
    if text is not None:
        conversation = [{"role": "user", "content": [{"type": "text", "text": text}]}]
        if has_image:
            conversation[0]["content"].append({"type": "image"})
        return processor.apply_chat_template(conversation, add_generation_prompt=True)
    return "<image>"


def capture_hidden(model, hooked_module, inputs, device) -> torch.Tensor:
    """One forward; the hooked layer's first output [1, L, d] (the existing hooks see the same tuple / tensor)."""
    captured = {}

    def hook(module, _, outputs):
        h = outputs[0] if isinstance(outputs, (tuple, list)) else outputs
        captured["h"] = h.detach().clone()

    handle = hooked_module.register_forward_hook(hook)
    try:
        with torch.no_grad():
            kw = {"input_ids": inputs["input_ids"].to(device)}
            for key in ("pixel_values", "image_sizes", "attention_mask"):
                if key in inputs and inputs[key] is not None:
                    kw[key] = inputs[key].to(device)
            model(**kw)
    finally:
        handle.remove()
    return captured["h"]


def probe_inputs(sae, hidden: List[torch.Tensor], skip_first: bool, k: int):
    """The captured [1, L_i, d] states as one [sum L_i, d] batch, one segment per input (minus the BOS token when
    `skip_first`), through ONE Sae.probe call.  -> (ProbeOutput, segments)."""
    flat = torch.cat([h.reshape(-1, h.shape[-1]) for h in hidden], dim=0)
    segments, off = [], 0
    for h in hidden:
        L = h.reshape(-1, h.shape[-1]).shape[0]
        segments.append((off + (1 if skip_first else 0), off + L))
        off += L
    return sae.probe(flat, k, segments=segments), segments


def main(argv=None):
    args = parse_argument(argv)
    first, end = interval_of(args)
    images = args.image_path or []
    assert images or args.text is not None, "Image and text can no both be None"
    ddp, rank, world = ddp_setup()
    device = f"cuda:{rank}"
    sae = load_single_sae(args.sae_path, args.module_name, device=device)
    model, processor = maybe_load_llava_model(args.model, rank=rank, dtype=torch.float16, hf_token=None)
    from transformers import AutoTokenizer

    tokenizer = AutoTokenizer.from_pretrained(args.model)
    hooked_module = model.language_model.get_submodule(args.module_name)
    # the reference's rule: with the llama tokenizer and no text, the first (BOS) token is not part of the image
    skip_first = "llama" in str(getattr(tokenizer, "name_or_path", "")) and args.text is None

    from PIL import Image

    opened = [Image.open(p) for p in images] or [None]
    hidden = []
    for image in opened:
        prompt = build_prompt(processor, args.text, image is not None)
        inputs = processor(images=image, text=prompt, return_tensors="pt").to(model.device)
        hidden.append(capture_hidden(model, hooked_module, inputs, model.device))
    out, segments = probe_inputs(sae, hidden, skip_first, end)
    values, indices, maps = out.values.cpu(), out.indices.cpu(), out.maps.cpu()

    if rank == 0:
        os.makedirs(args.save_to, exist_ok=True)
        entries, union = [], []
        for n, (image_path, image) in enumerate(zip(images or [None], opened)):
            idx = indices[n, first:end].tolist()
            entries.append({"image": image_path, "text": args.text, "indices": idx,
                            "values": values[n, first:end].tolist()})
            union += [i for i in idx if i not in union]
            if image is None:
                continue
            b, e = segments[n]
            rows = [maps[b:e, j] for j in range(first, end)]
            image_dir = os.path.join(args.save_to, "images") if len(images) == 1 else \
                os.path.join(args.save_to, "images", str(n))
            os.makedirs(image_dir, exist_ok=True)
            for i, im in zip(idx, activation_images(image, rows)):
                im.save(os.path.join(image_dir, f"feat_{i}.png"))
        with open(os.path.join(args.save_to, "filters.json"), "w") as f:
            json.dump({args.module_name: union}, f)
        with open(os.path.join(args.save_to, "probe.json"), "w") as f:
            json.dump({args.module_name: entries}, f, indent=2)
    if ddp:
        import torch.distributed as dist

        dist.barrier()


if __name__ == "__main__":
    main()
