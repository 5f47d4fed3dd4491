"""Host side of the 8-bit image boundary (edtr_amd/imageio.py, evalutil's argument checks, the edtr_amd.restore command line): the numpy
restatements the device kernels are tested against are themselves checked here against Pillow's recorded output
(tests/golden/pillow_bicubic.npz, tools/make_imageio_goldens.py), a live Pillow where one is installed, and CPU torch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# input (h, w) -> output (h, w): the pairs the resize rule was first verified on
LIVE_PAIRS = [((100, 150), (341, 512)), ((375, 500), (384, 512)), ((1200, 900), (512, 384)), ((37, 53), (37, 200)),
              ((64, 64), (33, 64)), ((480, 640), (720, 960)), ((333, 500), (111, 167))]


def test_reference_resize_equals_the_recorded_pillow_output(golden_dir):
    from edtr_amd import imageio
    g = np.load(os.path.join(golden_dir, "pillow_bicubic.npz"))
    names = [str(n) for n in g["names"]]
    assert len(names) >= 5
    kinds = set()
    for n in names:
        src, want = g[f"{n}_in"], g[f"{n}_out"]
        assert max(src.shape[:2] + want.shape[:2]) <= 256
        got = imageio.resize_u8_reference(src, want.shape[1], want.shape[0])
        assert got.dtype == np.uint8 and got.shape == want.shape
        diff = int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max())
        print(f"[{n}] {src.shape[:2]} -> {want.shape[:2]} max diff {diff}")
        assert diff == 0, n
        (h, w), (oh, ow) = src.shape[:2], want.shape[:2]
        kinds |= {"up"} if oh > h and ow > w else set()
        kinds |= {"wide"} if h > 2 * oh and w > 2 * ow else set()
        kinds |= {"one_axis"} if (oh == h) != (ow == w) else set()
        kinds |= {"odd"} if h % 2 and w % 2 and oh % 2 and ow % 2 else set()
        kinds |= {"one_wide"} if w == 1 else set()
    assert kinds == {"up", "wide", "one_axis", "odd", "one_wide"}, kinds        # the file covers what it is meant to cover


def test_reference_resize_equals_a_live_pillow():
    from edtr_amd import imageio
    try:
        from PIL import Image
    except ImportError:
        print("Pillow is not installed: only its recorded outputs (the test above) are compared")
        return
    for k, ((h, w), (oh, ow)) in enumerate(LIVE_PAIRS):
        img = np.random.default_rng(100 + k).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        want = np.array(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
        got = imageio.resize_u8_reference(img, ow, oh)
        assert int(np.abs(got.astype(np.int32) - want.astype(np.int32)).max()) == 0, ((h, w), (oh, ow))


def test_resize_coeffs_shape_and_windows():
    from edtr_amd import imageio
    for n_in, n_out in ((53, 200), (256, 50), (1, 31), (64, 64), (2048, 512)):
        bounds, coefs = imageio.resize_coeffs(n_in, n_out)
        assert bounds.dtype == np.int32 and coefs.dtype == np.int32
        assert bounds.shape == (n_out, 2) and coefs.shape[0] == n_out
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all()
        assert (bounds[:, 1] <= coefs.shape[1]).all()
        assert (np.abs(coefs.sum(1) - (1 << 22)) <= coefs.shape[1]).all()         # normalised weights, each rounded once
        for i in (0, n_out - 1):
            assert (coefs[i, bounds[i, 1]:] == 0).all()


def test_demo_size_follows_the_reference():
    from edtr_amd import imageio
    assert imageio.demo_size(640, 480) == (512, 384)
    assert imageio.demo_size(150, 100) == (512, 341)
    assert imageio.demo_size(100, 150) == (341, 512)
    assert imageio.demo_size(512, 512) == (512, 512)
    # 500 x 333: 333 * 512 / 500 = 340.99 -> round gives 341, truncation would give 340
    assert imageio.demo_size(500, 333) == (512, 341) and int(333 * (512 / 500)) == 340
    # round-half-even of Python's round, as int(round(x)) in demo.py:82: 1024 x 5 -> 2.5 -> 2
    assert imageio.demo_size(1024, 5) == (512, 2)
    assert imageio.demo_size(500, 333, scale=0.5) == (250, 166)                    # int(): 166.5 -> 166
    assert imageio.demo_size(101, 77, scale=1.5) == (151, 115)


def test_ingest_table_is_the_float64_quotient_rounded_once():
    from edtr_amd import imageio
    want = (np.arange(256) / 255.0).astype(np.float32)
    assert imageio.INGEST_TABLE.dtype == np.float32 and imageio.INGEST_TABLE.shape == (256,)
    assert np.array_equal(imageio.INGEST_TABLE.view(np.uint32), want.view(np.uint32))
    img = np.random.default_rng(0).integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    assert np.array_equal(imageio.INGEST_TABLE[img], (img / 255.0).astype(np.float32))      # demo.py:85


def _torch_emit(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(x).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).numpy()       # torchvision save_image


def test_emit_rule_equals_save_image_on_cpu_torch():
    from edtr_amd import imageio
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-0.2, 1.2, 200000), rng.normal(0.5, 0.4, 100000)]).astype(np.float32)
    assert np.array_equal(imageio.emit_reference(x), _torch_emit(x))
    # both sides of every .5 boundary: the neighbours of (k + 0.5) / 255 in fp32, three steps each way
    k = np.arange(0, 256, dtype=np.float64)
    edge = ((k + 0.5) / 255.0).astype(np.float32)
    around = [edge]
    lo, hi = edge.copy(), edge.copy()
    for _ in range(3):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        around += [lo.copy(), hi.copy()]
    b = np.concatenate(around + [np.array([0.0, -0.0, 1.0, 1.0 + 2e-3, -1e-3, 255.0, -7.0, np.inf, -np.inf], dtype=np.float32)])
    got = imageio.emit_reference(b)
    assert np.array_equal(got, _torch_emit(b))
    assert len(set(got[:256 * 7].reshape(7, 256)[:, 100].tolist())) == 2               # the boundary really is straddled
    # values where one fused multiply-add differs from the two roundings
    cand = rng.uniform(0.0, 1.0, 2000000).astype(np.float32)
    two = (cand * np.float32(255.0)).astype(np.float32) + np.float32(0.5)
    fused = (cand.astype(np.float64) * 255.0 + 0.5).astype(np.float32)                  # exact product and sum, rounded once = fmaf
    pick = cand[two != fused]                       # the fp32 value before the truncation differs between the two forms
    assert pick.size > 1000, "no candidate tells the fused form from the two-rounding form"
    assert np.array_equal(imageio.emit_reference(pick), _torch_emit(pick))
    # (the BYTES of the two forms agree on every such value found here: an integer is representable, so a rounding of up to half an
    #  ulp moves the sum onto k + 1 in both forms or in neither.  The rule is still stated — and implemented — as two roundings.)
    print(f"{pick.size} values with different fp32 intermediates, {int((np.trunc(two) != np.trunc(fused)).sum())} with different bytes")
    assert imageio.emit_reference(np.array([np.nan], dtype=np.float32))[0] == 0         # documented: NaN -> 0


def test_batch_extent_mirrors_the_reference_paddings():
    from edtr_amd import evalutil, imageio
    for h, w in ((150, 100), (512, 700), (64, 64), (129, 640)):
        x = torch.zeros(1, 3, h, w)
        want = tuple(evalutil.pad_to_multiples_of(evalutil.pad_if_smaller(x, 512), 64).shape[2:])
        assert imageio.batch_extent([(h, w)], min_size=512, multiple=64) == want
        assert imageio.batch_extent([(h, w)], multiple=64) == (-(-h // 64) * 64, -(-w // 64) * 64)    # main/seg/test_edtr.py:114
    assert imageio.batch_extent([(10, 20), (30, 5)]) == (30, 20)
    assert imageio.batch_extent([(10, 20)], size=(32, 48)) == (32, 48)
    with pytest.raises(ValueError):
        imageio.batch_extent([(40, 20)], size=(32, 48))


class _FakeCldm:
    unet = torch.nn.Linear(1, 1)


def test_restore_dataset_argument_check_knows_seg():
    from edtr_amd import evalutil, rng
    with pytest.raises(ValueError, match="pad_mode"):
        evalutil.restore_dataset(_FakeCldm(), None, None, [], pad_mode="segment")
    with pytest.raises(ValueError, match="pad_mode"):
        evalutil.restore_dataset(_FakeCldm(), None, None, [], pad_mode="bogus", seed=1)
    for mode in ("batch", "demo", "seg"):                                              # nothing to restore: the checks alone run
        assert evalutil.restore_dataset(_FakeCldm(), None, None, [], pad_mode=mode, seed=3, return_uint8=True) == ([], None)
    # the seeded ids of "seg" are those of "demo": one image per chunk, image k carries id k
    for world in (1, 3):
        for rank in range(world):
            assert rng.shard_chunk_ids(7, rank, world, 4, "seg") == rng.shard_chunk_ids(7, rank, world, 4, "demo")
    assert rng.shard_chunk_ids(3, 0, 1, 8, "seg") == [[0], [1], [2]]
    with pytest.raises(ValueError):
        rng.shard_chunk_ids(3, 0, 1, 8, "bogus")


def test_restore_command_line_help_needs_no_gpu():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "edtr_amd.restore", "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input", "--output", "--config", "--seed", "--scale"):
        assert flag in r.stdout
