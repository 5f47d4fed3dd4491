"""The host side of edtr_amd/boxes.py, without a GPU: the numpy restatements against the reference's own BoxCoder.decode,
sliding_windows, move_boxes, resize_boxes and postprocess_detections (tests/golden/boxes.npz, written by
tools/make_boxes_goldens.py), the NMS rule on hand-built cases, the scale-factor bilinear against torch's CPU interpolate,
`drawable`'s rules, and the C ABI's rules for the six new entry points."""
import math
import os
import re

import numpy as np
import pytest
import torch

from edtr_amd import boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "boxes.npz"))


def b4(*rows):
    return np.array(rows, dtype=F32).reshape(-1, 4)


# ---- restatements against the reference -------------------------------------------------------------------------------------------------
def test_decode_restatement_equals_the_reference_within_the_ulp_of_exp(golden):
    """Everything but exp is exact fp32 arithmetic in the reference's order; the clamp bounds exp at 62.5, and numpy's and torch's exp
    are each within an ulp: rtol 1e-6.  The golden holds rows that reach the clamp and rows that do not."""
    codes, props, want = golden["decode_codes"], golden["decode_proposals"], golden["decode_out"]
    got = boxes.decode_reference(codes, props)
    assert got.shape == want.shape == (24, 5, 4) and got.dtype == F32
    assert (codes[:, 2::4] / 5 > boxes.BBOX_XFORM_CLIP).any() and (codes[:, 2::4] / 5 < boxes.BBOX_XFORM_CLIP).any()
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_windows_equal_the_reference_bit_for_bit(golden):
    cases = [tuple(int(v) for v in row) for row in golden["window_cases"]]
    assert len(cases) >= 6
    for i, (W, H, tile, stride) in enumerate(cases):
        got = np.array(boxes.det_windows(W, H, tile, stride), dtype=np.int32).reshape(-1, 4)
        assert np.array_equal(got, golden[f"windows{i}"]), (W, H, tile, stride)
    # the edge rule is not tiling.py's: an image smaller than the tile gets ONE window that reaches past it
    assert boxes.det_windows(300, 200, 512, 256) == [(0, 0, 512, 512)]
    assert boxes.det_windows(160, 96, 64, 32)[-1] == (96, 32, 160, 96)
    with pytest.raises(ValueError):
        boxes.det_windows(0, 5, 4, 2)


def test_move_and_resize_restatements_equal_the_reference_bit_for_bit(golden):
    src = golden["boxes_in"]
    dx, dy = (int(v) for v in golden["move_dxdy"])
    assert np.array_equal(boxes.move_boxes_reference(src, dx, dy), golden["move_out"])
    orig, new = golden["resize_sizes"]
    assert np.array_equal(boxes.resize_boxes_reference(src, orig, new), golden["resize_out"])
    assert np.array_equal(boxes.box_transform_reference(src, shift=(dx, dy)), golden["move_out"])


@pytest.mark.parametrize("tag", ["voc", "coco"])
def test_detections_restatement_returns_the_recorded_kept_set(golden, tag):
    g = {k: golden[f"post_{tag}_{k}"] for k in ("logits", "codes", "proposals", "shape", "per_img", "boxes", "scores", "labels")}
    got = boxes.detections_reference(g["logits"], g["codes"], g["proposals"], tuple(int(v) for v in g["shape"]),
                                     detections_per_img=int(g["per_img"]))
    assert got["labels"].dtype == np.int64 and got["boxes"].dtype == F32 and got["scores"].dtype == F32
    assert np.array_equal(got["labels"], g["labels"])                  # the kept set, in the reference's order
    np.testing.assert_allclose(got["boxes"], g["boxes"], rtol=1e-5, atol=0)
    np.testing.assert_allclose(got["scores"], g["scores"], rtol=1e-5, atol=0)
    assert len(g["labels"]) == int(g["per_img"])                      # the top-k cut was reached
    assert (np.diff(got["scores"]) <= 0).all()


def test_softmax_restatement_against_torch():
    x = np.random.default_rng(3).normal(0, 3, (17, 91)).astype(F32)
    np.testing.assert_allclose(boxes.softmax_reference(x), torch.softmax(torch.from_numpy(x), -1).numpy(), rtol=1e-5, atol=0)


# ---- the NMS rule on hand-built cases --------------------------------------------------------------------------------------------------
def test_nms_chain_a_suppresses_b_which_therefore_does_not_suppress_c():
    """IoU(A, B) = 0.6 and IoU(B, C) = 0.6 exceed 0.5; IoU(A, C) = 0.36 does not: B is suppressed by A, so C stays"""
    bx = b4((0, 0, 10, 10), (0, 0, 10, 6), (0, 2.4, 10, 6))
    s = np.array([0.9, 0.8, 0.7], dtype=F32)
    assert boxes.iou_row_reference(bx[0], bx[1:2])[0] > 0.5 and boxes.iou_row_reference(bx[1], bx[2:3])[0] > 0.5
    assert boxes.iou_row_reference(bx[0], bx[2:3])[0] < 0.5
    assert boxes.nms_reference(bx, s, 0.5).tolist() == [0, 2]
    assert boxes.nms_reference(bx[1:], s[1:], 0.5).tolist() == [0]          # without A, B does suppress C


def test_nms_equal_scores_keep_ascending_index():
    bx = b4((0, 0, 10, 10), (0, 0, 10, 9), (20, 20, 30, 30), (20, 20, 30, 29))
    s = np.array([0.5, 0.5, 0.5, 0.5], dtype=F32)
    assert boxes.nms_reference(bx, s, 0.5).tolist() == [0, 2]
    assert boxes.nms_reference(bx[::-1], s, 0.5).tolist() == [0, 2]         # the earlier of a tie wins, whichever box that is
    assert boxes.rank_order_reference(np.array([0.5, 0.7, 0.5, 0.7], dtype=F32)).tolist() == [1, 3, 0, 2]


def test_nms_orders_nan_first_and_zeroes_alike():
    s = np.array([0.1, np.nan, -0.0, 0.0, np.inf, -np.inf, -np.nan], dtype=F32)
    assert boxes.rank_order_reference(s).tolist() == torch.sort(torch.from_numpy(s), descending=True, stable=True)[1].tolist()


def test_nms_identical_boxes_with_different_labels_are_both_kept():
    bx = b4((0, 0, 10, 10), (0, 0, 10, 10), (0, 0, 10, 10))
    s = np.array([0.9, 0.8, 0.7], dtype=F32)
    assert boxes.batched_nms_reference(bx, s, np.array([1, 2, 1]), 0.5).tolist() == [0, 1]
    assert boxes.nms_reference(bx, s, 0.5).tolist() == [0]
    # labels are compared as int64, not folded into 32 bits or into the coordinates
    assert boxes.batched_nms_reference(bx, s, np.array([1, 1 + (1 << 32), 1], dtype=np.int64), 0.5).tolist() == [0, 1]


def test_nms_zero_area_box_suppresses_nothing_and_is_not_suppressed():
    """two identical zero-area boxes: inter 0, union 0, IoU NaN, and NaN is not greater than the threshold"""
    bx = b4((5, 5, 5, 5), (5, 5, 5, 5), (0, 0, 10, 10))
    s = np.array([0.9, 0.8, 0.7], dtype=F32)
    assert np.isnan(boxes.iou_row_reference(bx[0], bx[1:2])[0])
    assert boxes.nms_reference(bx, s, 0.0).tolist() == [0, 1, 2]


def test_nms_iou_equal_to_the_threshold_is_kept():
    bx = b4((0, 0, 10, 10), (0, 0, 10, 5), (0, 0, 10, 5.5))
    s = np.array([0.9, 0.8, 0.7], dtype=F32)
    assert boxes.iou_row_reference(bx[0], bx[1:2])[0] == F32(0.5)
    assert boxes.nms_reference(bx[:2], s[:2], 0.5).tolist() == [0, 1]          # 0.5 > 0.5 is false
    assert boxes.nms_reference(bx[[0, 2]], s[:2], 0.5).tolist() == [0]         # 0.55 > 0.5


def test_nms_max_out_form_pads_and_counts():
    bx = b4((0, 0, 10, 10), (20, 0, 30, 10), (40, 0, 50, 10), (0, 0, 10, 9))
    s = np.array([0.9, 0.8, 0.7, 0.6], dtype=F32)
    full = boxes.nms_reference(bx, s, 0.5)
    assert full.tolist() == [0, 1, 2]
    for K in (2, 3, 5):
        keep, count = boxes.nms_reference(bx, s, 0.5, max_out=K)
        assert keep.dtype == np.int64 and keep.shape == (K,) and count.dtype == np.int32 and count.shape == (1,)
        assert int(count[0]) == min(K, 3) and keep[:int(count[0])].tolist() == full[:K].tolist() and (keep[int(count[0]):] == -1).all()
    empty = boxes.nms_reference(np.zeros((0, 4), dtype=F32), np.zeros(0, dtype=F32), 0.5)
    assert empty.shape == (0,) and empty.dtype == np.int64


def test_nms_restatement_against_an_independent_pairwise_loop():
    rng = np.random.default_rng(11)
    xy = rng.integers(0, 200, (150, 2))
    bx = np.concatenate([xy, xy + rng.integers(1, 80, (150, 2))], axis=1).astype(F32)
    s = (rng.integers(0, 16, 150) / 16).astype(F32)
    lab = rng.integers(0, 3, 150)
    order = sorted(range(150), key=lambda i: (-s[i], i))
    dead, keep = set(), []
    for a, i in enumerate(order):
        if i in dead:
            continue
        keep.append(i)
        for j in order[a + 1:]:
            if lab[j] == lab[i] and boxes.iou_row_reference(bx[i], bx[j:j + 1])[0] > F32(0.4):
                dead.add(j)
    assert boxes.batched_nms_reference(bx, s, lab, 0.4).tolist() == keep and 10 < len(keep) < 150


def test_malformed_inputs_raise_value_error():
    big = boxes.NMS_MAX_BOXES + 1
    for fn in (boxes.batched_nms_reference, boxes.batched_nms):          # the device wrapper refuses before it touches a device
        with pytest.raises(ValueError, match="at most 32768"):
            fn(np.zeros((big, 4), dtype=F32), np.zeros(big, dtype=F32), np.zeros(big, dtype=np.int64), 0.5)
        with pytest.raises(ValueError):
            fn(np.zeros((3, 5), dtype=F32), np.zeros(3, dtype=F32), None, 0.5)
        with pytest.raises(ValueError):
            fn(np.zeros((3, 4), dtype=F32), np.zeros(2, dtype=F32), None, 0.5)
        with pytest.raises(ValueError):
            fn(np.zeros((3, 4), dtype=F32), np.zeros(3, dtype=F32), np.zeros((3, 1), dtype=np.int64), 0.5)
        with pytest.raises(ValueError):
            fn(np.zeros((3, 4), dtype=F32), np.zeros(3, dtype=F32), None, 0.5, max_out=0)
    for fn in (boxes.detections_reference, boxes.detections):
        with pytest.raises(ValueError):
            fn(np.zeros((4, 3), dtype=F32), np.zeros((4, 8), dtype=F32), np.zeros((4, 4), dtype=F32), (10, 10))
        with pytest.raises(ValueError):
            fn(np.zeros((4, 1), dtype=F32), np.zeros((4, 4), dtype=F32), np.zeros((4, 4), dtype=F32), (10, 10))
    for fn in (boxes.box_transform_reference, boxes.box_transform):
        with pytest.raises(ValueError):
            fn(np.zeros((4, 3), dtype=F32), shift=(1, 1))
        with pytest.raises(ValueError):
            fn(np.zeros((4, 4), dtype=F32), mul=(2, 2), div=(2, 2))
    for fn in (boxes.bilinear_scale_reference, boxes.bilinear_scale):
        with pytest.raises(ValueError):
            fn(np.zeros((3, 4, 4), dtype=F32), 0.0)
        with pytest.raises(ValueError):
            fn(np.zeros((3, 4, 4), dtype=F32), 0.2)                         # floor(4 * 0.2) = 0
    with pytest.raises(ValueError):
        boxes.detect_reference(np.zeros((3, 8, 8), dtype=F32), lambda x: [], mode="fast")


# ---- the scale-factor bilinear ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale", [((3, 37, 53), 0.7), ((3, 96, 64), 512 / 750), ((3, 750, 500), 512 / 750), ((1, 5, 7), 0.7)])
def test_bilinear_scale_restatement_against_torch(shape, scale):
    """The output is a convex combination of four inputs in [0, 1] with at most six fp32 roundings and two rounded weights: atol 1e-6."""
    x = np.random.default_rng(5).uniform(0, 1, shape).astype(F32)
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[None], scale_factor=scale, mode="bilinear", align_corners=False)[0].numpy()
    got = boxes.bilinear_scale_reference(x, scale)
    assert got.shape == want.shape == (shape[0], math.floor(shape[1] * scale), math.floor(shape[2] * scale)) and got.dtype == F32
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def test_bilinear_scale_uses_the_reciprocal_scale_not_the_extent_ratio():
    """at 37 -> floor(25.9) = 25 rows, 1 / 0.7 and 37 / 25 differ, and the two rules give visibly different images"""
    from edtr_amd import degrade
    x = np.random.default_rng(6).uniform(0, 1, (1, 3, 37, 53)).astype(F32)
    by_scale = boxes.bilinear_scale_reference(x, 0.7)
    by_size = degrade.resize_reference(x, by_scale.shape[2:], "bilinear")
    assert by_scale.shape == by_size.shape and np.abs(by_scale - by_size).max() > 1e-3


# ---- drawable ---------------------------------------------------------------------------------------------------------------------------
def test_drawable_constants_are_the_reference_tables(golden):
    assert sorted(golden["coco_unnamed_labels"].tolist()) == sorted(boxes.COCO_UNUSED + (0,))
    assert sorted(golden["voc_tvmonitor_labels"].tolist()) == [0, boxes.VOC_TVMONITOR]
    assert golden["label_table_lengths"].tolist() == [20, 91]


def test_drawable_rules_voc():
    t = {"boxes": b4((12.9, 20.2, 50.7, 60.1),          # drawn, corners cut toward zero
                     (12, 20, 50, 60),                  # score at the threshold: not drawn (strictly greater)
                     (3, 4, 50, 60),                    # tvmonitor in the corner: dropped
                     (3, 4, 50, 60),                    # another class in the corner: drawn
                     (30, 4, 50, 60),                   # tvmonitor away from the corner: drawn
                     (-0.5, 4, 50, 60),                 # int(-0.5) = 0: inside
                     (-1.5, 4, 50, 60),                 # x1 = -1: outside
                     (10, 10, 100.5, 80),               # x2 = 100 = w: inside
                     (10, 10, 101, 80),                 # x2 > w
                     (10, 10, 50, 81)),                 # y2 > h
         "labels": np.array([7, 7, 20, 15, 20, 3, 3, 3, 3, 3]),
         "scores": np.array([0.9, 0.8, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9], dtype=F32)}
    d = boxes.drawable(t, (80, 100), score_threshold=0.8)
    assert d["index"].tolist() == [0, 3, 4, 5, 7]
    assert d["boxes"][0].tolist() == [12, 20, 50, 60] and d["boxes"][3].tolist() == [0, 4, 50, 60] and d["boxes"].dtype == np.int64
    assert d["labels"].tolist() == [7, 15, 20, 3, 3] and np.array_equal(d["scores"], t["scores"][d["index"]])
    # without scores nothing is masked
    d2 = boxes.drawable({"boxes": t["boxes"], "labels": t["labels"]}, (80, 100))
    assert d2["index"].tolist() == [0, 1, 3, 4, 5, 7] and "scores" not in d2
    # tensors are taken too
    d3 = boxes.drawable({k: torch.from_numpy(v) for k, v in t.items()}, (80, 100), score_threshold=0.8)
    assert d3["index"].tolist() == d["index"].tolist()
    with pytest.raises(ValueError):
        boxes.drawable({"boxes": b4((0, 0, 1, 1)), "labels": np.array([21])}, (80, 100))
    empty = boxes.drawable({"boxes": np.zeros((0, 4), dtype=F32), "labels": np.zeros(0, dtype=np.int64)}, (80, 100))
    assert empty["index"].shape == (0,) and empty["boxes"].shape == (0, 4)


def test_drawable_rules_coco():
    t = {"boxes": b4((12, 20, 50, 60), (12, 20, 50, 60), (3, 4, 50, 60), (12, 20, 50, 60)),
         "labels": np.array([1, 12, 72, 91]), "scores": np.array([0.9, 0.9, 0.9, 0.5], dtype=F32)}
    d = boxes.drawable(t, (80, 100), score_threshold=0.8, is_coco=True)
    assert d["index"].tolist() == [0, 2]                # 12 is an unused id; COCO has no corner rule; a masked box has label 0: unnamed


# ---- detect through the restatements ------------------------------------------------------------------------------------------------
def test_detect_reference_tile_mode_skips_an_empty_window_and_merges():
    calls = []

    def detnet(images):
        (img,) = images
        calls.append(img.shape)
        k = len(calls)
        if k == 2:          # a window with nothing at or above 0.6 contributes nothing
            return [{"boxes": b4((1, 1, 20, 20)), "scores": np.array([0.3], dtype=F32), "labels": np.array([4])}], None
        return [{"boxes": b4((0, 0, 30, 30), (2, 2, 31, 31)), "scores": np.array([0.9, 0.6], dtype=F32), "labels": np.array([k, k])}], None

    out = boxes.detect_reference(np.zeros((3, 96, 160), dtype=F32), detnet, mode="tile", tile=64, stride=32)
    wins = boxes.det_windows(160, 96, 64, 32)
    assert len(calls) == len(wins) == 8 and all(c == (3, 64, 64) for c in calls)
    assert len(out["labels"]) == 7 and 2 not in out["labels"].tolist()          # every window's labels differ: only the 0.6 duplicates go
    first = out["boxes"][np.argsort(out["labels"])][0]
    assert first.tolist() == [0, 0, 30, 30]


# ---- the C ABI's rules for the new entry points ----------------------------------------------------------------------------------------
NEW_SYMBOLS = ("edtr_boxes_rank", "edtr_boxes_nms", "edtr_boxes_candidates", "edtr_boxes_filter_shift", "edtr_boxes_transform", "edtr_boxes_bilinear_scale")


def test_new_symbols_are_declared_bound_and_exported_at_abi_10():
    from edtr_amd import build, lib
    assert "boxes.hip" in build.SOURCES
    assert lib.ABI_VERSION == 10
    assert lib.NMS_MAX_BOXES == boxes.NMS_MAX_BOXES == 32768
    assert (lib.BOX_SHIFT, lib.BOX_MUL, lib.BOX_DIV, lib.BOX_CLIP) == (1, 2, 4, 8)          # bits: they are ORed
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert name in lib.DECLARED_SYMBOLS and hasattr(handle, name)


def test_new_entry_points_reject_bad_arguments_before_any_launch():
    """NULL pointers, non-positive extents, too many boxes, misaligned boxes and unknown flags are refused on the host (no device is
    touched: this runs without a GPU)."""
    import ctypes
    from edtr_amd import build, lib
    build.build_library()
    h = lib.load()
    p = 4096            # a non-NULL, aligned stand-in: every call below fails its checks before the pointer is used
    assert h.edtr_boxes_rank(None, 4, p, None) == -1 and h.edtr_boxes_rank(p, 0, p, None) == -2 and h.edtr_boxes_rank(p, 32769, p, None) == -5
    assert h.edtr_boxes_nms(None, p, None, 0, 4, 0.5, p, p, p, 4, p, None) == -1
    assert h.edtr_boxes_nms(p, p, None, 0, 4, 0.5, p, None, p, 4, p, None) == -1
    assert h.edtr_boxes_nms(p, p, None, 0, 0, 0.5, p, p, p, 4, p, None) == -2
    assert h.edtr_boxes_nms(p, p, None, 0, 4, 0.5, p, p, p, 0, p, None) == -2
    assert h.edtr_boxes_nms(p, p, None, 0, 32769, 0.5, p, p, p, 4, p, None) == -5
    assert h.edtr_boxes_nms(p, p, p, 2, 4, 0.5, p, p, p, 4, p, None) == -4
    assert h.edtr_boxes_nms(p + 4, p, None, 0, 4, 0.5, p, p, p, 4, p, None) == -3
    assert h.edtr_boxes_nms(p, p, p + 4, 1, 4, 0.5, p, p, p, 4, p, None) == -3
    w = (ctypes.c_float * 4)(10, 10, 5, 5)
    w0 = (ctypes.c_float * 4)(10, 0, 5, 5)
    cand = lambda *a: h.edtr_boxes_candidates(*a, None)  # noqa: E731
    assert cand(p, p, p, 4, 21, 10.0, 10.0, 0.05, 0.01, w, 4.0, p, p, p, p, p, p, p, None) == -1
    assert cand(p, p, p, 4, 21, 10.0, 10.0, 0.05, 0.01, None, 4.0, p, p, p, p, p, p, p, p) == -1
    assert cand(p, p, p, 0, 21, 10.0, 10.0, 0.05, 0.01, w, 4.0, p, p, p, p, p, p, p, p) == -2
    assert cand(p, p, p, 4, 1, 10.0, 10.0, 0.05, 0.01, w, 4.0, p, p, p, p, p, p, p, p) == -2
    assert cand(p, p, p, 4, 21, 10.0, 10.0, 0.05, 0.01, w0, 4.0, p, p, p, p, p, p, p, p) == -2
    assert cand(p, p, p, 1 << 20, 21, 10.0, 10.0, 0.05, 0.01, w, 4.0, p, p, p, p, p, p, p, p) == -5
    assert cand(p, p + 4, p, 4, 21, 10.0, 10.0, 0.05, 0.01, w, 4.0, p, p, p, p, p, p, p, p) == -3
    assert h.edtr_boxes_filter_shift(p, p, None, 4, 0.6, 0.0, 0.0, p, p, p, p, 4, None) == -1
    assert h.edtr_boxes_filter_shift(p, p, p, 0, 0.6, 0.0, 0.0, p, p, p, p, 4, None) == -2
    assert h.edtr_boxes_filter_shift(p, p, p, 4, 0.6, 0.0, 0.0, p, p, p, p, 0, None) == -2
    assert h.edtr_boxes_filter_shift(p, p, p, 4, 0.6, 0.0, 0.0, p + 8, p, p, p, 4, None) == -3
    assert h.edtr_boxes_transform(None, p, 4, 1, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, None) == -1
    assert h.edtr_boxes_transform(p, p, 0, 1, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, None) == -2
    assert h.edtr_boxes_transform(p, p, 4, 16, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, None) == -4
    assert h.edtr_boxes_transform(p, p, 4, lib.BOX_MUL | lib.BOX_DIV, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, None) == -4
    assert h.edtr_boxes_transform(p, p + 4, 4, 1, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, None) == -3
    assert h.edtr_boxes_bilinear_scale(p, None, 3, 4, 4, 2, 2, 2.0, 2.0, None) == -1
    assert h.edtr_boxes_bilinear_scale(p, p, 3, 4, 4, 0, 2, 2.0, 2.0, None) == -2
    assert h.edtr_boxes_bilinear_scale(p, p, 3, 4, 4, 2, 2, 0.0, 2.0, None) == -2
