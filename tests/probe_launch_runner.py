"""Executed under `python -m torch.distributed.run --nproc-per-node 1 ... tests/probe_launch_runner.py <dir>` by
tests/test_gpu_probe.py: runs msae.launch.features.probe through its real `main()` with the HF model / processor /
tokenizer loaders replaced by the stand-ins of tests/fakes.py (no checkpoint, no network), and writes what Sae.probe gives
on the hidden states the hook captures (restated here with a forward hook of its own) as expect_<run>.json."""
import json
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (REPO, REPO / "tests", REPO / "multimodal-sae_amd"):
    sys.path.insert(0, str(p))

import torch

import fakes
from launch_runner import build_sae_checkpoint


class LlamaNamedTokenizer(fakes.FakeSlowTokenizer):
    name_or_path = "fake/llama3-llava-next-tiny"


def expected(model, processor, sae, module, images, text, k, skip_first):
    hidden = []

    def hook(_m, _i, outputs):
        hidden.append(outputs[0].detach().clone())

    h = model.language_model.get_submodule(module).register_forward_hook(hook)
    with torch.no_grad():
        for img in images or [None]:
            prompt = "<image>" if text is None else text + (" <image>" if img is not None else "")
            inputs = processor(images=img, text=prompt, return_tensors="pt").to(model.device)
            model(**{key: inputs[key].to(model.device) for key in ("input_ids", "pixel_values", "image_sizes",
                                                                      "attention_mask")})
    h.remove()
    flat = torch.cat([x.reshape(-1, x.shape[-1]) for x in hidden])
    segs, off = [], 0
    for x in hidden:
        L = x.shape[1]
        segs.append((off + int(skip_first), off + L))
        off += L
    out = sae.probe(flat, k, segments=segs)
    return {"indices": out.indices.cpu().tolist()}


def main():
    out = Path(sys.argv[1])
    rank = int(os.environ.get("LOCAL_RANK", "0"))
    vocab = 40
    import transformers
    from PIL import Image

    import msae.launch.features.probe as lp
    from msae import Sae

    transformers.AutoTokenizer.from_pretrained = classmethod(lambda cls, *a, **k: LlamaNamedTokenizer(vocab))

    def fake_model_loader(model_name, rank, dtype, hf_token=None):
        return fakes.TinyLlava(vocab=vocab).to(f"cuda:{rank}"), fakes.FakeProcessor(vocab)

    lp.maybe_load_llava_model = fake_model_loader
    real_setup, state = lp.ddp_setup, {}

    def setup_once(timeout_s=None):          # the process group is initialised by the first main() only
        if "v" not in state:
            state["v"] = real_setup(timeout_s)
        return state["v"]

    lp.ddp_setup = setup_once
    sae_dir = out / "saes"
    if rank == 0:
        build_sae_checkpoint(sae_dir, ["layers.1"], d=64, N=1024, k=8)
    paths = []
    for i in range(2):
        p = out / f"img{i}.png"
        Image.new("RGB", (40, 30), (30 * i, 90, 200 - 50 * i)).save(p)
        paths.append(str(p))

    # one image, no text (BOS skipped: llama tokenizer), the top 6
    lp.main(["-m", "llava-tiny", "--sae-path", str(sae_dir), "--module-name", "layers.1", "-i", paths[0], "-k", "6",
             "-s", str(out / "one")])
    # two images with a question, one batch; the features ranked 2..7
    lp.main(["-m", "llava-tiny", "--sae-path", str(sae_dir), "--module-name", "layers.1", "-i", paths[0], "-i", paths[1],
             "-t", "what is this", "--interval", "2-7", "-s", str(out / "two")])

    model = fakes.TinyLlava(vocab=vocab).to(f"cuda:{rank}")
    processor = fakes.FakeProcessor(vocab)
    sae = Sae.load_from_disk(sae_dir / "layers.1", device=f"cuda:{rank}")
    images = [Image.open(p) for p in paths]
    one = expected(model, processor, sae, "layers.1", images[:1], None, 6, True)
    two = expected(model, processor, sae, "layers.1", images, "what is this", 7, False)
    two["indices"] = [row[2:7] for row in two["indices"]]
    (out / "expect_one.json").write_text(json.dumps(one))
    (out / "expect_two.json").write_text(json.dumps(two))

    import torch.distributed as dist

    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
