"""`degrade.degrade_files(..., geometry=, masks=)` on the device: three tiny PNGs and their label maps go through the reference's
segmentation geometry before the degradation; without the new keywords the files are byte for byte what `degrade_batch` gives."""
import os

import numpy as np
import pytest
import torch

from edtr_amd import degrade, imageio, labels

pytestmark = pytest.mark.gpu

EXTENTS = (("a", (24, 40)), ("b", (33, 21)), ("c", (24, 40)))
VOC_LIKE = [v for rgb in ((0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0)) for v in rgb] + [0] * (3 * 252)


def _config():
    return degrade.DegradeConfig(blur_kernel_size=7, kernel_list=degrade.KERNEL_TYPES, kernel_prob=(1,) * 6, blur_sigma=(0.3, 2.0),
                                 downsample_range=(1.0, 2.5), noise_range=(1.0, 20.0), jpeg_range=(30.0, 95.0), gray_noise_prob=0.5,
                                 resize_back=True, resize_modes=degrade.MODES)


@pytest.fixture()
def folder(tmp_path):
    """three images and their masks: one mode "P" mask (palette indices, as VOC's are), two mode "L" """
    from PIL import Image
    src, msk = tmp_path / "in", tmp_path / "masks"
    src.mkdir()
    msk.mkdir()
    gen = np.random.default_rng(5)
    raws, maps = {}, {}
    for name, (h, w) in EXTENTS:
        raws[name] = gen.integers(0, 256, (h, w, 3), dtype=np.uint8)
        maps[name] = gen.integers(0, 4, (h, w), dtype=np.uint8)
        maps[name][0, :3] = 255
        Image.fromarray(raws[name]).save(src / f"{name}.png")
        im = Image.fromarray(maps[name])
        if name == "a":
            im.putpalette(VOC_LIKE)             # (turns the image into mode "P" and keeps its bytes as the indices)
            assert im.mode == "P"
        im.save(msk / f"{name}.png")
        assert np.array_equal(np.array(Image.open(msk / f"{name}.png")), maps[name])
    return tmp_path, sorted(str(p) for p in src.iterdir()), str(msk), raws, maps


def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.mode, np.array(im)


@pytest.mark.parametrize("crop_type,out_size", [("center", 20), ("none", 40)])
def test_geometry_and_masks(folder, crop_type, out_size):
    tmp, paths, msk, raws, maps = folder
    geo = labels.SegGeometry(gt_size=32, resize_range=(0.75, 1.25), out_size=out_size, crop_type=crop_type, hflip=True)
    cfg, seed = _config(), 3
    out = tmp / "out"
    written = degrade.degrade_files(paths, str(out), cfg, seed, batch_size=2, geometry=geo, masks=msk)
    assert len(written) == 3
    for k, ((gt_path, lq_path), (name, hw)) in enumerate(zip(written, EXTENTS)):
        assert os.path.exists(gt_path) and os.path.exists(lq_path) and os.path.exists(out / "mask" / f"{name}.png")
        geom = labels.draw_geometry(geo, seed, k, hw)
        want_gt, want_mask = labels.prepare_pair(raws[name], maps[name], geom)
        ref_gt, ref_mask = labels.prepare_pair_reference(raws[name], maps[name], geom)
        mode, got_mask = _read(out / "mask" / f"{name}.png")
        assert mode == "L" and np.array_equal(got_mask, want_mask.cpu().numpy()) and np.array_equal(got_mask, ref_mask)
        mode, got_gt = _read(gt_path)
        assert mode == "RGB" and np.array_equal(got_gt, want_gt.cpu().numpy()) and np.array_equal(got_gt, ref_gt)
        # lq/ is the degradation of the prepared image under the draws of image k: ids and draws are the geometry-free ones
        batch, sizes = imageio.ingest([got_gt])
        lq = degrade.degrade_batch(batch, [degrade.draw_params(cfg, seed, k)], seed, [k], sizes)[0]
        want_lq = imageio.emit(lq[None].contiguous(), [tuple(lq.shape[1:])])[0].cpu().numpy()
        assert np.array_equal(_read(lq_path)[1], want_lq) and want_lq.shape == got_gt.shape


def test_without_the_new_keywords_the_bytes_are_degrade_batchs(folder):
    tmp, paths, msk, raws, maps = folder
    cfg, seed = _config(), 3
    written = degrade.degrade_files(paths, str(tmp / "plain"), cfg, seed, batch_size=2)
    assert not os.path.exists(tmp / "plain" / "mask")
    for k, ((gt_path, lq_path), (name, hw)) in enumerate(zip(written, EXTENTS)):
        assert np.array_equal(_read(gt_path)[1], raws[name])
        batch, sizes = imageio.ingest([raws[name]])
        lq = degrade.degrade_batch(batch, [degrade.draw_params(cfg, seed, k)], seed, [k], sizes)[0]
        want = imageio.emit(lq[None].contiguous(), [tuple(lq.shape[1:])])[0].cpu().numpy()
        assert np.array_equal(_read(lq_path)[1], want)
    # masks alone: copied through as mode "L", images untouched
    again = degrade.degrade_files(paths, str(tmp / "masks_only"), cfg, seed, batch_size=2, masks=msk)
    for (gt1, lq1), (gt2, lq2), (name, _) in zip(written, again, EXTENTS):
        for f1, f2 in ((gt1, gt2), (lq1, lq2)):
            with open(f1, "rb") as a, open(f2, "rb") as b:
                assert a.read() == b.read()
        mode, m = _read(tmp / "masks_only" / "mask" / f"{name}.png")
        assert mode == "L" and np.array_equal(m, maps[name])
