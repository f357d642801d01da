"""CPU: the host side of Sae.probe -- segment forms and their validation, the chunk plan of the pooled kernel, the numpy
restatement of the numerics contract on hand-computed cases, the mask renderer, the SAE loader and the launcher's command
line -- and the new C-ABI symbols."""
import re

import numpy as np
import pytest
import torch

import probe_ref
from conftest import REPO


# ---- segments -------------------------------------------------------------------------------------------------------
def test_default_segments():
    from msae.sae.probe import parse_segments

    assert parse_segments(None, (3, 5, 16)) == ("host", [(0, 5), (5, 10), (10, 15)])
    assert parse_segments(None, (7, 16)) == ("host", [(0, 7)])
    with pytest.raises(ValueError):
        parse_segments(None, (16,))
    with pytest.raises(ValueError):
        parse_segments(None, (1, 2, 3, 16))


def test_host_segments_with_gaps_are_accepted():
    from msae.sae.probe import parse_segments

    segs = [(1, 4), (4, 5), (9, 20)]
    assert parse_segments(segs, (20, 8)) == ("host", segs)
    assert parse_segments([[0, 2], (np.int64(5), np.int32(6))], (2, 3, 8)) == ("host", [(0, 2), (5, 6)])
    assert parse_segments(torch.tensor([[0, 3], [3, 6]]), (6, 8)) == ("host", [(0, 3), (3, 6)])   # a CPU tensor: host


@pytest.mark.parametrize("bad", [
    [],                                  # nothing to probe
    [(0, 3), (2, 5)],                    # overlap
    [(4, 6), (0, 2)],                    # unsorted
    [(3, 3)],                            # empty
    [(5, 2)],                            # inverted
    [(-1, 2)],                           # before 0
    [(0, 11)],                           # past T = 10
    [(0.0, 2)],                          # not ints
    [(True, 2)],
    [(0, 1, 2)],                         # not a pair
    [5],
    "0-3",
    7,
])
def test_host_segment_errors(bad):
    from msae.sae.probe import parse_segments

    with pytest.raises(ValueError):
        parse_segments(bad, (10, 8))


# ---- chunk plan -----------------------------------------------------------------------------------------------------
def _check_plan(segs, chunks, budget=None):
    covered = [i for a, b in chunks for i in range(a, b)]
    assert covered == list(range(len(segs))), "every segment exactly once, in order"
    for a, b in chunks:
        assert a < b
        for i in range(a, b - 1):
            assert segs[i][1] == segs[i + 1][0], "a chunk never spans a gap"
        if budget is not None and b - a > 1:
            assert sum(e - s for s, e in segs[a:b]) <= budget


@pytest.mark.parametrize("N", [1000, 32768, 131072])
@pytest.mark.parametrize("n_cu", [8, 256])
def test_plan_chunks_equal_segments(N, n_cu):
    from msae.sae.probe import TILE, WORKGROUPS_PER_CU, plan_chunks

    segs = [(i * 576, (i + 1) * 576) for i in range(64)]
    chunks = plan_chunks(segs, N, n_cu)
    strips = -(-N // TILE)
    want = max(1, -(-2 * n_cu * WORKGROUPS_PER_CU // strips))
    budget = -(-(-(-64 * 576 // want)) // TILE) * TILE
    _check_plan(segs, chunks, budget)
    sizes = [sum(e - s for s, e in segs[a:b]) for a, b in chunks]
    assert max(sizes) - min(sizes) <= TILE * 5 or len(chunks) == 1     # balanced: every chunk but the last is full
    assert all(budget - sz < 576 for sz in sizes[:-1])                   # ... up to one segment
    if strips >= 2 * n_cu * WORKGROUPS_PER_CU:
        assert chunks == [(0, 64)]                                        # wide SAE: the strips fill the machine
    else:
        assert len(chunks) >= min(64, want)


def test_plan_chunks_gaps_long_segments_and_balance():
    from msae.sae.probe import TILE, plan_chunks

    # one long segment stays one chunk whatever the budget: segments are never split
    assert plan_chunks([(0, 2880)], 1000, 256) == [(0, 1)]
    # gaps cut chunks even when the budget would allow more
    segs = [(0, 10), (10, 20), (25, 30), (30, 40)]
    assert plan_chunks(segs, 131072, 256) == [(0, 2), (2, 4)]
    # the budget is total / wanted chunks rounded up to whole tiles: 8 x 576 over 4 chunks -> 1152 tokens each
    segs = [(i * 576, (i + 1) * 576) for i in range(8)]
    assert plan_chunks(segs, 128 * 256, 256) == [(0, 2), (2, 4), (4, 6), (6, 8)]
    # ragged: a chunk closes before the segment that would overflow it
    segs, o = [], 0
    for L in (100, 300, 40, 700, 5, 5, 5, 1000, 1):
        segs.append((o, o + L))
        o += L
    chunks = plan_chunks(segs, 128, 3)          # 1 strip, 12 wanted -> budget 256
    _check_plan(segs, chunks, 2 * TILE)
    assert plan_chunks([], 128, 3) == []


# ---- numerics restatement on hand-computed cases ----------------------------------------------------------------------
def test_restatement_mean_max_topk_maps_by_hand():
    v = np.array([[0.0, 1.0, 2.0, 0.5],
                  [0.0, 3.0, 2.0, 0.5],
                  [4.0, 0.0, 2.0, 0.0],
                  [1.0, 1.0, 0.0, 7.0],
                  [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    segs = [(0, 3), (3, 4), (4, 5)]
    mean = probe_ref.pooled(v, segs, "mean")
    np.testing.assert_array_equal(mean, np.array([[4 / 3, 4 / 3, 2.0, 1 / 3], [1, 1, 0, 7], [0, 0, 0, 0]], dtype=np.float32))
    mx = probe_ref.pooled(v, segs, "max")
    np.testing.assert_array_equal(mx, np.array([[4, 3, 2, 0.5], [1, 1, 0, 7], [0, 0, 0, 0]], dtype=np.float32))
    vals, idx = probe_ref.topk(mean, 3)
    np.testing.assert_array_equal(idx, [[2, 0, 1], [3, 0, 1], [0, 1, 2]])     # ties (4/3, 4/3) and zeros: ascending index
    np.testing.assert_array_equal(vals[0], np.float32([2.0, 4 / 3, 4 / 3]))
    m = probe_ref.maps(v, [(1, 3), (3, 4)], idx[:2])
    np.testing.assert_array_equal(m, np.array([[0, 0, 0], [2, 0, 3], [2, 4, 0], [7, 1, 1], [0, 0, 0]], dtype=np.float32))


def test_restatement_mean_is_the_sequential_f64_chain():
    # the f64 sum in ascending order, then one rounding: 2^24 + 1 + 1 ... differs from a pairwise / f32 sum
    col = np.array([2.0 ** 30, 1.0, 1.0, 1.0, -0.0 + 3.0], dtype=np.float32)[:, None]
    want = np.float32((((2.0 ** 30 + 1.0) + 1.0) + 1.0 + 3.0) / 5.0)
    assert probe_ref.pooled(col, [(0, 5)], "mean")[0, 0] == want
    # clamping as the kernel does for device segments; an empty segment is 0
    v = np.arange(12, dtype=np.float32).reshape(6, 2)
    np.testing.assert_array_equal(probe_ref.pooled(v, [(-4, 2), (5, 99), (3, 3), (4, 1)], "mean"),
                                  np.float32([[1, 2], [10, 11], [0, 0], [0, 0]]))


# ---- masks ------------------------------------------------------------------------------------------------------------
def test_mask_and_composite_pixels():
    from PIL import Image

    from msae.features.images import activation_image, base_grid, upsample_mask

    acts = np.zeros(576, dtype=np.float32)
    acts[:24] = 1.0                        # the first grid row fires
    grid = base_grid(acts)
    assert grid.shape == (24, 24) and grid[0].min() == 1.0 and grid[1:].max() == 0.0
    # the mask before resizing: 224 where the activation is below 1e-5
    m = np.asarray(upsample_mask(torch.from_numpy(grid), (24, 24)))
    assert m[0].max() == 0 and (m[1:] == 224).all()
    img = Image.new("RGB", (10, 10), (200, 100, 50))
    out = np.asarray(activation_image(img, torch.from_numpy(acts), (48, 48)))
    assert out.shape == (48, 48, 3)
    assert (out[0] == (200, 100, 50)).all()                  # firing row: the image (mask 0)
    assert (out[-1] == np.round(np.array([200, 100, 50]) * (255 - 224) / 255)).all()   # silent: 224/255 black over it
    # a shorter row (a toy model's sequence) is padded with zeros
    assert base_grid(np.ones(5, dtype=np.float32)).sum() == 5


# ---- loader and launcher ----------------------------------------------------------------------------------------------
def test_load_single_sae_from_disk(tmp_path):
    from msae import Sae, SaeConfig
    from msae.utils import load_single_sae

    sae = Sae(16, SaeConfig(num_latents=64, k=4))
    with torch.no_grad():
        sae.encoder.weight.normal_()
    sae.save_to_disk(tmp_path / "layers.3")
    got = load_single_sae(str(tmp_path), "layers.3", device="cpu")
    assert got.num_latents == 64 and torch.equal(got.encoder.weight, sae.encoder.weight)


def test_launcher_arguments():
    from msae.launch.features.probe import interval_of, parse_argument

    a = parse_argument(["-m", "m", "--sae-path", "p", "--module-name", "layers.2", "-i", "a.png", "-i", "b.png",
                        "-t", "hi", "-k", "7", "-s", "out"])
    assert (a.model, a.sae_path, a.module_name, a.image_path, a.text, a.top_k, a.save_to) == \
        ("m", "p", "layers.2", ["a.png", "b.png"], "hi", 7, "out")
    assert interval_of(a) == (0, 7)
    a = parse_argument(["--sae-path", "p", "-i", "a.png", "--interval", "10-20"])
    assert a.module_name == "model.layers.24" and a.image_path == ["a.png"] and interval_of(a) == (10, 20)
    for bad in ("20-10", "3", "1-2-3"):
        with pytest.raises(ValueError):
            interval_of(parse_argument(["--interval", bad]))


def test_launcher_prompt():
    from msae.launch.features.probe import build_prompt

    class P:
        def apply_chat_template(self, conv, add_generation_prompt=True):
            return repr(conv)

    assert build_prompt(P(), None, True) == "<image>"
    assert "'type': 'image'" in build_prompt(P(), "what", True)
    assert "'type': 'image'" not in build_prompt(P(), "what", False)


# ---- C ABI ----------------------------------------------------------------------------------------------------------
def test_probe_symbols_declared_and_bound():
    from msae import _hip

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "msae.h").read_text(), flags=re.S)
    for name in ("msae_pooled_acts_f32", "msae_probe_maps_f32"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _hip.PROTOTYPES
    lib = _hip.load()
    assert lib.msae_abi_version() == 4
    # argument errors come back before anything touches a device
    assert lib.msae_pooled_acts_f32(None, 0, None, None, None, 10, 8, 16, None, 1, None, 0, 2, None, None) == -1
    assert lib.msae_probe_maps_f32(None, 0, None, None, None, 10, 8, 16, None, 1, None, 257, None, None) == -1


def test_sae_probe_methods_validate_on_the_host():
    from msae import Sae, SaeConfig

    sae = Sae(8, SaeConfig(num_latents=32, k=4))
    x = torch.randn(10, 8)
    with pytest.raises(ValueError):
        sae.probe(x, 0)
    with pytest.raises(ValueError):
        sae.probe(x, 33, maps=False)
    with pytest.raises(ValueError):
        sae.pooled_acts(x, reduce="sum")
    with pytest.raises(ValueError):
        sae.probe(x, 4, segments=[(0, 20)])
    with pytest.raises(RuntimeError, match="inference"):
        sae.probe(x.requires_grad_(True), 4)
    with pytest.raises(RuntimeError, match="MI355X|HIP"):      # no CPU path
        sae.probe(x.detach(), 4)
