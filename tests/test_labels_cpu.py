"""The host side of edtr_amd/labels.py, without a GPU: the numpy restatements against Pillow's NEAREST results and the reference's
own calculate_mat / compute_iou / convert2color (tests/golden/labels.npz, written by tools/make_labels_goldens.py), the geometry
draws, and the C ABI's rules for the four new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from edtr_amd import degrade, labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (from h, from w, to h, to w): the extents the issue names
NEAREST_CASES = [(2, 2, 7, 15), (3, 2, 21, 7), (1, 5, 1, 1), (5, 1, 3, 9), (2, 64, 23, 33), (9, 9, 9, 9), (281, 500, 307, 546)]


def closed_form_index(n_in, n_out):
    """floor((x + 0.5) n_in / n_out): the textbook NEAREST rule, which Pillow does NOT follow"""
    return np.minimum(np.floor((np.arange(int(n_out)) + 0.5) * (int(n_in) / int(n_out))).astype(np.int32), int(n_in) - 1)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "labels.npz"))


def test_golden_holds_the_named_extents(golden):
    assert [tuple(int(v) for v in row) for row in golden["nearest_cases"]] == NEAREST_CASES


@pytest.mark.parametrize("case", range(len(NEAREST_CASES)))
@pytest.mark.parametrize("channels", [1, 3])
def test_nearest_restatement_equals_pillow(golden, case, channels):
    h, w, oh, ow = NEAREST_CASES[case]
    src, want = golden[f"nearest{case}_c{channels}_in"], golden[f"nearest{case}_c{channels}_out"]
    assert src.shape[:2] == (h, w) and want.shape[:2] == (oh, ow)
    assert np.array_equal(labels.resize_nearest_reference(src, (oh, ow)), want)


def test_the_cases_tell_the_accumulating_rule_from_the_closed_form(golden):
    """Without columns where the two rules disagree the comparison above would pass on the wrong rule; and at those columns the
    closed form must really give other bytes than Pillow did."""
    differing = 0
    for case, (h, w, oh, ow) in enumerate(NEAREST_CASES):
        xa, xc = labels.nearest_index(w, ow), closed_form_index(w, ow)
        ya, yc = labels.nearest_index(h, oh), closed_form_index(h, oh)
        n = int((xa != xc).sum() + (ya != yc).sum())
        if n:
            src, want = golden[f"nearest{case}_c3_in"], golden[f"nearest{case}_c3_out"]
            assert not np.array_equal(src[yc][:, xc], want), "the closed form reproduced Pillow where the index tables differ"
        differing += n
    assert differing >= 4
    assert (labels.nearest_index(2, 7) != closed_form_index(2, 7)).any()
    assert (labels.nearest_index(500, 546) != closed_form_index(500, 546)).any()


def test_nearest_index_edges():
    assert labels.nearest_index(5, 1).tolist() == [2]
    assert labels.nearest_index(1, 4).tolist() == [0, 0, 0, 0]
    assert labels.nearest_index(9, 9).tolist() == list(range(9))
    for n_in, n_out in ((7, 1000), (1000, 7), (3, 3)):
        idx = labels.nearest_index(n_in, n_out)
        assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() <= n_in - 1 and (np.diff(idx) >= 0).all()
    with pytest.raises(ValueError):
        labels.nearest_index(0, 3)


def test_confusion_restatement_equals_calculate_mat(golden):
    mat, pred = labels.confusion_reference(golden["conf_logits"], golden["conf_target"], 21, return_pred=True)
    assert mat.dtype == np.int64 and np.array_equal(mat, golden["conf_mat"])
    assert int(mat.sum()) == int((golden["conf_target"] < 21).sum())
    assert np.array_equal(pred, torch.from_numpy(golden["conf_logits"]).argmax(1).numpy())


def test_argmax_restatement_is_torchs_cpu_rule():
    nan, inf = float("nan"), float("inf")
    rows = np.array([[1.0, 1.0, 0.0, -2.0], [3.0, 3.0, 3.0, 1.0], [-0.0, 0.0, -1.0, -1.0], [0.0, -0.0, -1.0, -1.0], [inf, 2.0, inf, 0.0],
                     [9.0, nan, 1.0, 0.0], [1.0, nan, 5.0, nan], [-inf, -inf, -inf, -inf], [nan, nan, nan, nan]], dtype=np.float32)
    logits = rows.T.reshape(1, 4, 3, 3).copy()
    for t in (torch.from_numpy(logits), torch.from_numpy(logits).half(), torch.from_numpy(logits).bfloat16()):
        want = t.argmax(1).numpy()
        assert np.array_equal(labels.argmax_reference(t.float().numpy()), want)
    assert labels.argmax_reference(logits).reshape(-1).tolist() == [0, 0, 0, 0, 0, 1, 1, 0, 0]


def test_confusion_restatement_sizes_and_checks():
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((2, 5, 4, 6)).astype(np.float32)
    target = rng.integers(0, 5, size=(2, 4, 6)).astype(np.uint8)
    whole = labels.confusion_reference(logits, target)
    parts = labels.confusion_reference(logits[:1, :, :1, :1], target[:1, :1, :1]) + labels.confusion_reference(logits[1:, :, :3, :5], target[1:, :3, :5])
    assert np.array_equal(labels.confusion_reference(logits, target, sizes=[(1, 1), (3, 5)]), parts)
    assert np.array_equal(labels.confusion_reference(logits, target, sizes=[(4, 6), (4, 6)]), whole)
    with pytest.raises(ValueError):
        labels.confusion_reference(logits, target, sizes=[(5, 6), (4, 6)])
    with pytest.raises(ValueError):
        labels.confusion_reference(logits, target, n=4)


def test_compute_iou_equals_the_reference(golden):
    assert np.array_equal(labels.compute_iou(golden["conf_mat"]), golden["conf_iou"], equal_nan=True)
    assert labels.compute_iou(golden["conf_mat"]).dtype == np.float32
    assert labels.mean_iou(golden["conf_mat"]) == float(golden["conf_miou"]) or (np.isnan(golden["conf_miou"]) and np.isnan(labels.mean_iou(golden["conf_mat"])))
    got = labels.compute_iou(golden["iou_mat"])
    assert np.array_equal(got, golden["iou_out"], equal_nan=True)


def test_compute_iou_beyond_exact_fp32_sums_stays_within_the_summation_bound(golden):
    """Row and column sums above 2^24 (a whole validation set): numpy's and torch's orders of the 21 additions may round differently.
    Each sum of 21 non-negative fp32 terms is within 20 * 2^-24 relative of the exact sum in any order, the union rows + columns -
    diagonal is at least as large as either sum (no cancellation), so two evaluations differ by at most about (2 * 20 + 5) * 2^-24
    each, 100 * 2^-24 between them."""
    mat, want = golden["iou_big_mat"], golden["iou_big_out"]
    assert int(mat.sum(0).min()) > 1 << 24 and int(mat.sum(1).min()) > 1 << 24
    got = labels.compute_iou(mat)
    rel = np.abs(got.astype(np.float64) - want.astype(np.float64)) / want.astype(np.float64)
    print(f"compute_iou against the reference beyond 2^24: max relative difference {rel.max():.3e}, {int((got != want).sum())} of {got.size} differ")
    assert rel.max() <= 100 * 2.0 ** -24


def test_compute_iou_is_nan_for_an_absent_class(golden):
    got = labels.compute_iou(golden["iou_mat"])
    assert np.isnan(got[7]) and int(np.isnan(got).sum()) == 1
    assert np.isnan(labels.mean_iou(golden["iou_mat"]))          # the reference's mean is NaN too: not "fixed"
    mat = np.array([[3, 1], [0, 0]])
    assert labels.compute_iou(mat).tolist() == [0.75, 0.0]


def test_colorize_restatement_equals_convert2color(golden):
    got = labels.colorize_reference(golden["color_labels"], golden["ref_palette"])
    assert got.dtype == np.uint8 and np.array_equal(got, golden["color_out"])
    lab = golden["color_labels"]
    assert (got[(lab == 255) | (lab == 21) | (lab == 200)] == 0).all()          # the labels the table does not name come out black
    assert np.array_equal(labels.colorize_reference(lab, golden["ref_palette"][:21]), golden["color_out"])      # a short table: zero beyond it


def test_voc_palette_is_the_bit_reversal_map():
    pal = labels.voc_palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[:6].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128]]
    assert pal[15].tolist() == [192, 128, 128] and pal[20].tolist() == [0, 64, 128] and pal[255].tolist() == [224, 224, 192]
    assert len({tuple(c) for c in pal.tolist()}) == 256


def test_window_restatement_is_pad_crop_and_flip():
    rng = np.random.default_rng(5)
    for shape in ((5, 7), (5, 7, 3)):
        x = rng.integers(0, 255, size=shape, dtype=np.uint8)
        pad = [(0, 4), (0, 2)] + ([(0, 0)] if len(shape) == 3 else [])
        padded = np.pad(x, pad, mode="constant", constant_values=255)
        assert np.array_equal(labels.window_reference(x, (9, 9), fill=255), padded)
        assert np.array_equal(labels.window_reference(x, (3, 4), (1, 3)), x[1:4, 3:7])
        assert np.array_equal(labels.window_reference(x, (6, 6), (2, 1), fill=255), padded[2:8, 1:7])
        assert np.array_equal(labels.window_reference(x, (6, 6), (2, 1), hflip=True, fill=255), padded[2:8, 1:7][:, ::-1])
        assert np.array_equal(labels.window_reference(x, (6, 6), (2, 1), vflip=True, fill=255), padded[2:8, 1:7][::-1])
        assert np.array_equal(labels.window_reference(x, (6, 6), (2, 1), hflip=True, vflip=True, fill=255), padded[2:8, 1:7][::-1, ::-1])
        assert (labels.window_reference(x, (2, 3), (-4, 20), fill=9) == 9).all()
        assert (labels.window_reference(x, (2, 2), (-1, -1), fill=9)[1, 1] == x[0, 0]).all()


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def test_resized_extent_is_the_references_expression():
    # int(gt_size * w / h * r) / int(gt_size * r), in that order of operations (datasets/segmentation.py:86-92)
    for (h, w) in ((375, 500), (500, 333)):
        for r in (0.5, 1.0, 1.37):
            if w >= h:
                want = (int(560 * r), int(560 * w / h * r))
            else:
                want = (int(560 * h / w * r), int(560 * r))
            assert labels.resized_extent(560, h, w, r) == want
    assert labels.resized_extent(560, 375, 500, 1.0) == (560, 746)
    assert labels.resized_extent(560, 375, 500, 0.5) == (280, 373)
    assert labels.resized_extent(560, 375, 500, 1.37) == (767, 1022)
    assert labels.resized_extent(560, 500, 333, 1.0) == (840, 560)
    assert labels.resized_extent(560, 500, 333, 0.5) == (420, 280)
    assert labels.resized_extent(560, 500, 333, 1.37) == (1151, 767)


def test_draw_geometry_is_deterministic_and_keyed_on_seed_and_id():
    cfg = labels.SegGeometry(gt_size=560, resize_range=(0.5, 2.0), out_size=512, crop_type="random", hflip=True)
    a, b = labels.draw_geometry(cfg, 7, 3, (375, 500)), labels.draw_geometry(cfg, 7, 3, (375, 500))
    assert a == b
    others = [labels.draw_geometry(cfg, s, k, (375, 500)) for s, k in ((7, 4), (8, 3), (7, 5), (9, 9))]
    assert any(o.size != a.size for o in others) and any(o.origin != a.origin for o in others)
    flips = {labels.draw_geometry(cfg, 1, k, (375, 500)).hflip for k in range(32)}
    assert flips == {False, True}
    assert not any(labels.draw_geometry(labels.SegGeometry(hflip=False), 1, k, (375, 500)).hflip for k in range(32))


def test_draw_geometry_crop_types_and_padding():
    hw = (375, 500)
    for k in range(16):
        rnd = labels.draw_geometry(labels.SegGeometry(560, (0.5, 2.0), 512, "random", True), 11, k, hw)
        ctr = labels.draw_geometry(labels.SegGeometry(560, (0.5, 2.0), 512, "center", True), 11, k, hw)
        non = labels.draw_geometry(labels.SegGeometry(560, (0.5, 2.0), 512, "none", True), 11, k, hw)
        assert rnd.size == ctr.size == non.size and rnd.pad == ctr.pad == non.pad             # the same r for every crop type
        rh, rw = rnd.size
        assert rnd.pad == (max(512 - rh, 0), max(512 - rw, 0))                                  # padding only when smaller, per side
        H, W = rh + rnd.pad[0], rw + rnd.pad[1]
        assert ctr.origin == ((H - 512) // 2, (W - 512) // 2) and ctr.out_hw == (512, 512)
        assert 0 <= rnd.origin[0] <= H - 512 and 0 <= rnd.origin[1] <= W - 512 and rnd.out_hw == (512, 512)
        assert non.origin == (0, 0) and non.out_hw == (H, W)
    small = labels.draw_geometry(labels.SegGeometry(100, None, 512, "center"), 0, 0, hw)
    assert small.size == (100, 133) and small.pad == (412, 379) and small.origin == (0, 0)
    large = labels.draw_geometry(labels.SegGeometry(600, None, 512, "center"), 0, 0, hw)
    assert large.size == (600, 800) and large.pad == (0, 0) and large.origin == (44, 144)
    nopad = labels.draw_geometry(labels.SegGeometry(100, None, None, "none"), 0, 0, hw)
    assert nopad.pad == (0, 0) and nopad.out_hw == (100, 133)
    origins = {labels.draw_geometry(labels.SegGeometry(600, None, 512, "random"), 2, k, hw).origin for k in range(24)}
    assert len(origins) > 12


def test_geometry_configuration():
    with pytest.raises(NotImplementedError):
        labels.SegGeometry(rotation=True)
    with pytest.raises(ValueError):
        labels.SegGeometry(crop_type="middle")
    with pytest.raises(ValueError):
        labels.SegGeometry(out_size=None, crop_type="center")
    ref_yaml = {"dataset": {"train": {"target": "x", "params": {"root": "r", "gt_size": 560, "resize_range": [0.5, 2.0], "out_size": 512,
                                                                 "crop_type": "random", "hflip": True, "rotation": False, "blur_kernel_size": 41}}}}
    cfg = labels.SegGeometry.from_dict(ref_yaml)
    assert (cfg.gt_size, list(cfg.resize_range), cfg.out_size, cfg.crop_type, cfg.hflip, cfg.rotation) == (560, [0.5, 2.0], 512, "random", True, False)
    assert labels.SegGeometry.from_dict({"gt_size": 64, "crop_type": "none"}).gt_size == 64
    with pytest.raises(ValueError):
        labels.SegGeometry.from_dict({"dataset": {}})


def test_draw_params_do_not_move_when_geometry_is_drawn():
    def same(a, b):
        assert type(a) is type(b)
        for k, v in vars(a).items():
            w = getattr(b, k)
            assert (v is None and w is None) or (np.array_equal(v, w) if isinstance(v, np.ndarray) else v == w), k

    cfg1, cfg2 = degrade.DegradeConfig(), degrade.RealESRGANConfig()
    geo = labels.SegGeometry(560, (0.5, 2.0), 512, "random", True)
    for s, k in ((0, 0), (5, 17), (2 ** 40, 2 ** 32 - 1)):
        before1, before2 = degrade.draw_params(cfg1, s, k), degrade.draw_params2(cfg2, s, k)
        labels.draw_geometry(geo, s, k, (375, 500))
        same(before1, degrade.draw_params(cfg1, s, k))
        same(before2, degrade.draw_params2(cfg2, s, k))
    # and the geometry's stream is its own: not the first draws of the degradation's generator
    g = np.random.default_rng([5, 17])
    own = np.random.default_rng([5, 17, labels.GEOMETRY_WORD])
    assert g.uniform() != own.uniform()


def test_prepare_pair_restatement_on_a_small_pair():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(37, 23, 3), dtype=np.uint8)
    mask = rng.integers(0, 21, size=(37, 23), dtype=np.uint8)
    geom = labels.draw_geometry(labels.SegGeometry(16, None, 24, "center", False), 0, 0, (37, 23))
    assert geom.size == (25, 16) and geom.pad == (0, 8) and geom.origin == (0, 0) and geom.out_hw == (24, 24)
    gt, m = labels.prepare_pair_reference(img, mask, geom)
    assert gt.shape == (24, 24, 3) and m.shape == (24, 24)
    assert (gt[:, 16:] == 0).all() and (m[:, 16:] == 255).all()
    assert np.array_equal(m[:, :16], labels.resize_nearest_reference(mask, (25, 16))[:24])
    with pytest.raises(ValueError):
        labels.paired_mask_reference(mask, (20, 30), center_crop=24)
    pm = labels.paired_mask_reference(mask, (40, 30), center_crop=24)
    assert np.array_equal(pm, labels.resize_nearest_reference(mask, (40, 30))[8:32, 3:27])


# ---- the C ABI's rules for the new entry points ----------------------------------------------------------------------------------------
NEW_SYMBOLS = ("edtr_seg_confusion", "edtr_label_resize_nearest", "edtr_label_window", "edtr_label_colorize")


def test_new_symbols_are_declared_bound_and_exported_at_abi_10():
    from edtr_amd import build, lib
    assert "labels.hip" in build.SOURCES
    assert lib.ABI_VERSION == 10
    assert lib.SEG_MAX_CLASSES == 32            # "n > 32" of the refusals below
    assert (lib.LOGITS_F32, lib.LOGITS_F16, lib.LOGITS_BF16) == (0, 1, 2)
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert name in lib.DECLARED_SYMBOLS and hasattr(handle, name)


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    """NULL pointers, non-positive extents, n > 32 and a sizes entry outside the slot are refused on the host (no device is touched:
    this runs without a GPU)."""
    import ctypes
    from edtr_amd import build, lib
    build.build_library()
    h = lib.load()
    p = 4096            # a non-NULL, aligned stand-in: every call below fails its checks before the pointer is used
    assert h.edtr_seg_confusion(0, None, p, 1, 21, 4, 4, None, None, p, None, 0, None) == -1
    assert h.edtr_seg_confusion(0, p, p, 1, 21, 4, 4, None, None, None, None, 0, None) == -1
    assert h.edtr_seg_confusion(0, p, p, 1, 33, 4, 4, None, None, p, None, 0, None) == -5
    assert h.edtr_seg_confusion(0, p, p, 1, 0, 4, 4, None, None, p, None, 0, None) == -2
    assert h.edtr_seg_confusion(0, p, p, 1, 21, 0, 4, None, None, p, None, 0, None) == -2
    assert h.edtr_seg_confusion(3, p, p, 1, 21, 4, 4, None, None, p, None, 0, None) == -4
    assert h.edtr_seg_confusion(0, p, p, 1, 21, 4, 4, None, None, p, None, -1, None) == -2
    assert h.edtr_seg_confusion(0, p + 2, p, 1, 21, 4, 4, None, None, p, None, 0, None) == -3
    assert h.edtr_seg_confusion(0, p, p, 1, 21, 4, 4, None, None, p + 4, None, 0, None) == -3
    for bad in ((5, 4), (4, 5), (0, 4), (4, -1)):
        sizes = (ctypes.c_int32 * 2)(*bad)
        assert h.edtr_seg_confusion(0, p, p, 1, 21, 4, 4, sizes, p, p, None, 0, None) == -2
    assert h.edtr_seg_confusion(0, p, p, 1, 21, 4, 4, (ctypes.c_int32 * 2)(4, 4), None, p, None, 0, None) == -1      # host sizes without device sizes
    assert h.edtr_label_resize_nearest(None, 2, 2, 1, p, 3, 3, p, p, None) == -1
    assert h.edtr_label_resize_nearest(p, 2, 2, 1, p, 3, 3, None, p, None) == -1
    assert h.edtr_label_resize_nearest(p, 2, 2, 2, p, 3, 3, p, p, None) == -5
    assert h.edtr_label_resize_nearest(p, 2, 2, 1, p, 0, 3, p, p, None) == -2
    assert h.edtr_label_window(p, 2, 2, 1, None, 3, 3, 0, 0, 0, 0, 0, None) == -1
    assert h.edtr_label_window(p, 2, 2, 4, p, 3, 3, 0, 0, 0, 0, 0, None) == -5
    assert h.edtr_label_window(p, 2, 0, 1, p, 3, 3, 0, 0, 0, 0, 0, None) == -2
    assert h.edtr_label_window(p, 2, 2, 1, p, 3, 3, 0, 0, 2, 0, 0, None) == -4
    assert h.edtr_label_window(p, 2, 2, 1, p, 3, 3, 0, 0, 0, 0, 256, None) == -4
    assert h.edtr_label_colorize(p, 1, 2, 2, None, p, None) == -1
    assert h.edtr_label_colorize(p, 1, 0, 2, p, p, None) == -2
