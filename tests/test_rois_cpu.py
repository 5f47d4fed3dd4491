"""Host side of edtr_amd/rois.py: the numpy restatements against the reference's own AnchorGenerator, concat_box_prediction_layers,
BoxCoder.decode and filter_proposals (tests/golden/proposals.npz, written by tools/make_proposals_goldens.py), the RoIAlign rule
against a scalar loop and against fp64 grid_sample, the level mapper, the bounds and the C ABI.  No GPU."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

from edtr_amd import boxes, rois

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "proposals.npz"))


def nested(a):
    return tuple(tuple(float(v) for v in row) for row in a)


def head_of(gold):
    L = len(gold["rpn_sizes"])
    return [gold[f"rpn_objectness{l}"] for l in range(L)], [gold[f"rpn_deltas{l}"] for l in range(L)]


def rpn_kwargs(gold, tag):
    (pre, post), (nms, score) = gold[f"rpn_{tag}_top_n"], gold[f"rpn_{tag}_thresh"]
    return dict(sizes=nested(gold["rpn_sizes"]), aspect_ratios=nested(gold["rpn_ratios"]), pre_nms_top_n=int(pre), post_nms_top_n=int(post),
                nms_thresh=float(nms), score_thresh=float(score))


# ---- anchors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["v2", "mobilenet", "ragged"])
def test_anchors_restatement_equals_the_reference_bit_for_bit(gold, tag):
    """the v2 detector's five levels, the mobilenet form (15 anchors per cell on 3 levels), a padded size no grid size divides"""
    want = gold[f"anchors_{tag}"]
    got = rois.anchors_reference(gold[f"anchors_{tag}_grids"], gold[f"anchors_{tag}_padded"], nested(gold[f"anchors_{tag}_sizes"]),
                                 nested(gold[f"anchors_{tag}_ratios"]))
    assert got.dtype == F32 and got.shape == want.shape and np.array_equal(got, want)
    if tag == "mobilenet":
        assert rois.cell_anchors(nested(gold["anchors_mobilenet_sizes"]), nested(gold["anchors_mobilenet_ratios"]))[0].shape == (15, 4)
    if tag == "ragged":
        assert any(p % g for p, gs in zip(gold["anchors_ragged_padded"], gold["anchors_ragged_grids"].T) for g in gs)


def test_cell_anchors_round_half_to_even_and_reject_ragged_arguments():
    cell = rois.cell_anchors(((5, 3),), ((1.0,),))[0]            # +-2.5 and +-1.5: torch.round and this go to the even neighbour
    assert cell.tolist() == [[-2, -2, 2, 2], [-2, -2, 2, 2]]
    with pytest.raises(ValueError):
        rois.cell_anchors(((32,), (64,)), ((1.0,),))
    with pytest.raises(ValueError):
        rois.anchors_reference([(4, 4)], (64, 64), ((32,), (64,)), ((1.0,), (1.0,)))


# ---- the proposal filter -----------------------------------------------------------------------------------------------------------------
def test_the_logical_index_is_the_row_of_concat_box_prediction_layers(gold):
    obj, deltas = head_of(gold)
    flat = np.concatenate([o.transpose(0, 2, 3, 1).reshape(o.shape[0], -1) for o in obj], axis=1)
    assert np.array_equal(flat, gold["rpn_flat_objectness"])
    anchors = rois.anchors_reference([o.shape[-2:] for o in obj], gold["rpn_padded"], nested(gold["rpn_sizes"]), nested(gold["rpn_ratios"]))
    codes = np.concatenate([d.reshape(d.shape[0], -1, 4, d.shape[2], d.shape[3]).transpose(0, 3, 4, 1, 2).reshape(d.shape[0], -1, 4) for d in deltas], axis=1)
    for n in range(codes.shape[0]):
        got = boxes.decode_reference(codes[n], anchors, (1.0, 1.0, 1.0, 1.0), exp=rois.torch_exp)[:, 0]
        assert np.array_equal(got, gold["rpn_decoded"][n])              # BoxCoder.decode, with the exponential it runs
        np.testing.assert_allclose(boxes.decode_reference(codes[n], anchors, (1.0, 1.0, 1.0, 1.0))[:, 0], gold["rpn_decoded"][n], rtol=1e-5, atol=1e-5)


def test_select_reference_is_topk_where_torch_defines_the_order(gold):
    obj, _ = head_of(gold)
    for pre in (1, 100, 4096):
        sel = rois.select_reference(obj, pre)
        col = 0
        for o in obj:
            flat = torch.from_numpy(o.transpose(0, 2, 3, 1).reshape(o.shape[0], -1).copy())
            k = min(pre, flat.shape[1])
            assert sel[:, col:col + k].tolist() == flat.topk(k, dim=1)[1].tolist()
            col += k
        assert sel.dtype == np.int32 and sel.shape[1] == col


def test_select_reference_resolves_ties_by_the_logical_index_and_puts_nan_first():
    o = np.zeros((1, 3, 2, 2), dtype=F32)               # all equal: the first k logical indices, whatever the memory order
    assert rois.select_reference([o], 5)[0].tolist() == [0, 1, 2, 3, 4]
    o[0, 2, 1, 0] = np.nan                              # logical (y W + x) A + a = (2 + 0) 3 + 2 = 8
    o[0, 1, 0, 1] = np.inf                              # (0 + 1) 3 + 1 = 4
    o[0, 0, 1, 1] = -0.0                                # equals 0.0
    o[0, 0, 0, 0] = -np.inf
    assert rois.select_reference([o], 12)[0].tolist() == [8, 4, 1, 2, 3, 5, 6, 7, 9, 10, 11, 0]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_proposals_reference_equals_the_recorded_filter_proposals(gold, tag):
    """Boxes bit for bit with the exponential the reference runs (`rois.torch_exp`), scores within the bound tests/test_gpu_boxes.py
    uses for softmax scores (rtol 1e-5); with numpy's own exp — which differs from torch's in the last bit for 39 % of arguments — the
    same boxes are kept and lie within 1e-5 relative, which the golden tool's choice of seed (no ill-conditioned corner, no two
    probabilities within 4 ulp) makes a fair bound."""
    obj, deltas = head_of(gold)
    sizes = [tuple(s) for s in gold["rpn_image_sizes"]]
    kw = rpn_kwargs(gold, tag)
    exact = rois.proposals_reference(obj, deltas, sizes, gold["rpn_padded"], exp=rois.torch_exp, **kw)
    plain = rois.proposals_reference(obj, deltas, sizes, gold["rpn_padded"], **kw)
    for n, ((b, s), (pb, ps)) in enumerate(zip(exact, plain)):
        want_b, want_s = gold[f"rpn_{tag}_boxes{n}"], gold[f"rpn_{tag}_scores{n}"]
        assert b.dtype == F32 and b.shape == want_b.shape and len(want_b) > 0 and np.array_equal(b, want_b)
        np.testing.assert_allclose(s, want_s, rtol=1e-5, atol=0)
        assert pb.shape == want_b.shape
        np.testing.assert_allclose(pb, want_b, rtol=1e-5, atol=0)
        np.testing.assert_allclose(ps, want_s, rtol=1e-5, atol=0)
        assert boxes.cancellation_ratio(want_b, sizes[n]) <= 40


def test_candidates_reference_clamps_clips_and_filters():
    """hand-built: a delta beyond the exp clamp, a box that leaves the image, one thinner than min_size, a score threshold of 0.5, and
    a level that contributes nothing"""
    sizes, ratios = ((8,), (16,)), ((1.0,), (1.0,))
    obj = [np.full((1, 1, 2, 2), 2.0, dtype=F32), np.full((1, 1, 1, 1), -3.0, dtype=F32)]           # level 1: prob 0.047 < 0.5
    deltas = [np.zeros((1, 4, 2, 2), dtype=F32), np.zeros((1, 4, 1, 1), dtype=F32)]
    deltas[0][0, 2, 0, 0] = 9.0                          # dw beyond log(1000 / 16): the width is 8 * 62.5, cut by the image
    deltas[0][0, 0, 0, 1] = 10.0                         # moved right out of the image: both x clamp to w, width 0 < min_size
    deltas[0][0, 3, 1, 0] = -12.0                        # height 8 exp(-12) < 1e-3
    obj[0][0, 0, 1, 1] = -1.0                            # prob 0.27 < 0.5
    sel = rois.select_reference(obj, 10)
    (b, p, lvl), = rois.candidates_reference(obj, deltas, sel, [(16, 20)], (16, 20), sizes, ratios, 10, score_thresh=0.5)
    assert lvl.tolist() == [0] and b.tolist() == [[0.0, 0.0, 20.0, 4.0]] and abs(p[0] - 1 / (1 + np.exp(-2.0))) < 1e-7
    (b, p, lvl), = rois.candidates_reference(obj, deltas, sel, [(16, 20)], (16, 20), sizes, ratios, 10, score_thresh=0.0)
    assert lvl.tolist() == [0, 0, 1] and len(b) == 3


def test_nms_ranks_by_probability_not_by_logit():
    """two saturated logits on different levels give equal probabilities: the tie goes to the earlier candidate, not to the greater logit"""
    cand = [(np.array([[0, 0, 10, 10], [0, 0, 10, 10.5]], dtype=F32), rois.sigmoid_reference(np.array([40.0, 50.0], dtype=F32)),
             np.array([0, 0], dtype=np.int32))]
    assert cand[0][1].tolist() == [1.0, 1.0]
    (b, s), = rois.nms_stage_reference(cand, 0.7, 1)
    assert b.tolist() == [[0, 0, 10, 10]]


def test_bounds_raise_value_error():
    o = [np.zeros((1, 3, 2, 2), dtype=F32)] * 9
    with pytest.raises(ValueError):
        rois.select_reference(o[:1], 4097)
    with pytest.raises(ValueError):
        rois.select_reference(o[:1], 0)
    with pytest.raises(ValueError):
        rois.level_table([(2, 2)] * 9, (64, 64), [np.zeros((3, 4), dtype=F32)] * 9)
    with pytest.raises(ValueError):
        rois.level_table([(4096, 4096)], (4096, 4096), [np.zeros((1, 4), dtype=F32)])
    with pytest.raises(ValueError):
        rois.roi_align_reference([np.zeros((1, 1, 4, 4), dtype=F32)], [np.zeros((1, 4), dtype=F32)], [(16, 16)], 7, 0)
    with pytest.raises(ValueError):
        rois.roi_align_reference([np.zeros((1, 1, 4, 4), dtype=F32)], [np.zeros((1, 4), dtype=F32)], [(16, 16)], 9, 8)


# ---- RoIAlign ----------------------------------------------------------------------------------------------------------------------------
def roi_case(gold):
    feats = [gold[f"roi_features{l}"] for l in range(3)]
    batch, flat = gold["roi_batch"], gold["roi_rois"]
    return feats, [flat[batch == n] for n in range(2)], [tuple(s) for s in gold["roi_image_sizes"]]


def test_roi_align_restatement_equals_the_scalar_loop_bit_for_bit(gold):
    feats, per_image, sizes = roi_case(gold)
    s0, k0 = gold["roi_canonical"]
    got = rois.roi_align_reference(feats, per_image, sizes, 7, 2, canonical_scale=float(s0), canonical_level=float(k0))
    assert got.dtype == F32 and np.array_equal(got, gold["roi_out"])
    single = rois.roi_align_reference(feats[:1], per_image, sizes, 3, 3)
    assert np.array_equal(single, gold["roi_out_single"])
    levels = rois.roi_levels_reference(gold["roi_rois"], 2, 4, float(s0), float(k0))
    assert set(levels.tolist()) == {0, 1, 2}                                                   # every level is used
    outside = np.all(got.reshape(len(got), -1) == 0, axis=1)
    assert outside.sum() == 4                                                                  # the rois wholly outside an image


def test_roi_align_restatement_against_fp64_grid_sample_on_interior_boxes(gold):
    """Where every sample lies inside [0, W - 1] x [0, H - 1], roi_align's interpolation and grid_sample(align_corners=True) are one
    rule.  Measured when the goldens were made: the restatement lies 5.287e-06 (max abs, unit-normal features, 40 boxes, 7 x 7 bins of
    2 x 2 samples) from the fp64 result; the bound is 4 times that."""
    H, W = gold["gs_feature"].shape[-2:]
    got = rois.roi_align_reference([gold["gs_feature"][None]], [gold["gs_rois"]], [(H, W)], 7, 2)
    err = float(np.abs(got.astype(np.float64) - gold["gs_out"]).max())
    print(f"max |restatement - fp64 grid_sample| = {err:.3e}")
    assert err <= 4 * 5.287e-06


def test_level_mapper(gold):
    """2000 random boxes whose level value lies at least 1e-3 from an integer (the golden tool picked the seed; nothing is filtered
    here), hand-built boxes of 56^2 ... 896^2 where sqrt, the division and log2 are exact, one far below k_min and one far above k_max"""
    value = gold["map_value"]
    assert np.abs(value - np.round(value)).min() >= 1e-3 and len(value) == 2000
    for k_min, k_max in ((2, 5), (2, 4), (3, 3)):
        want = np.clip(np.floor(value), k_min, k_max).astype(np.int64) - k_min
        assert rois.roi_levels_reference(gold["map_rois"], k_min, k_max).tolist() == want.tolist()
        assert set(want.tolist()) == set(range(k_max - k_min + 1))
    hand = rois.roi_levels_reference(gold["map_hand_rois"], 2, 5)
    assert hand.tolist() == [0, 1, 2, 3, 3, 0, 3] and np.clip(gold["map_hand_value"], 2, 5).tolist() == [2, 3, 4, 5, 5, 2, 5]
    assert rois.roi_levels_reference(gold["map_hand_rois"], 1, 7).tolist() == [1, 2, 3, 4, 5, 0, 6]
    degenerate = np.array([[5, 5, 5, 9], [9, 9, 5, 5], [0, 0, np.nan, 4]], dtype=F32)           # zero area, negative sides, NaN
    assert rois.roi_levels_reference(degenerate, 2, 5).tolist() == [0, 3 - 3, 0]


def test_level_scales():
    scales, k_min, k_max = rois.level_scales([(200, 336), (100, 168), (50, 84), (25, 42)], [(800, 1344), (750, 1333)])
    assert scales == [0.25, 0.125, 0.0625, 0.03125] and (k_min, k_max) == (2, 5)
    assert rois.level_scales([(16, 24)], [(50, 81), (64, 96)]) == ([0.25], 2, 2)
    with pytest.raises(ValueError):
        rois.level_scales([(16, 48)], [(64, 96)])
    with pytest.raises(ValueError):
        rois.level_scales([(25, 42), (2, 3), (1, 1)], [(100, 168)])             # 2^-2, 2^-6, 2^-7: levels 3 .. 5 of the mapper are missing


# ---- the composed detector on the host ------------------------------------------------------------------------------------------------
def test_assemble_detector_reference_runs_the_seven_steps_and_rejects_unknown_thresholds():
    torch.manual_seed(3)
    calls = []

    def features_fn(images):
        calls.append("features")
        batch = torch.stack(list(images))
        return batch, [(64, 96)], [(128, 192)], {"0": batch[:, :, ::4, ::4].contiguous(), "1": batch[:, :, ::8, ::8].contiguous()}

    class Head(torch.nn.Module):
        def forward(self, feats):
            calls.append("rpn_head")
            return [f[:, :3] * 2 for f in feats], [torch.cat([f * 0.1] * 4, dim=1) for f in feats]

    box_head = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 49, 16), torch.nn.ReLU())

    class Predictor(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c, self.r = torch.nn.Linear(16, 4), torch.nn.Linear(16, 16)

        def forward(self, x):
            calls.append("predictor")
            return self.c(x), self.r(x)

    trace = {}
    detnet = rois.assemble_detector_reference(features_fn, Head(), box_head, Predictor(), trace=trace, sizes=((16,), (32,)),
                                              aspect_ratios=((0.5, 1.0, 2.0),) * 2, rpn_pre_nms_top_n=50, rpn_post_nms_top_n=20, box_score_thresh=0.0)
    out = detnet([torch.randn(3, 64, 96)])
    assert calls == ["features", "rpn_head", "predictor"] and len(out) == 1
    assert out[0]["boxes"].dtype == F32 and out[0]["boxes"].shape[1] == 4 and 0 < len(out[0]["scores"]) <= 100
    b = out[0]["boxes"]                                                        # resized to the original 128 x 192
    assert b.min() >= 0 and b[:, 2].max() <= 192 and b[:, 3].max() <= 128 and np.all(b[:, 2] >= b[:, 0])
    assert trace["pooled"].shape == (len(trace["proposals"][0][0]), 3, 7, 7) and len(trace["proposals"][0][0]) <= 20
    with pytest.raises(TypeError):
        rois.assemble_detector_reference(features_fn, Head(), box_head, Predictor(), nms=0.5)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("edtr_rpn_anchors", "edtr_rpn_select", "edtr_rpn_candidates", "edtr_roi_align")


def test_the_new_symbols_are_declared_bound_exported_and_the_abi_is_still_10():
    from edtr_amd import build, lib
    assert all(s in lib.DECLARED_SYMBOLS for s in SYMBOLS)
    assert lib.ABI_VERSION == 10
    assert "rois.hip" in build.GLUE_SOURCES and "rois.hip" not in build.SOURCES
    assert "glue.h" in [os.path.basename(d) for d in build.object_deps("rois.hip")]
    assert (lib.RPN_MAX_LEVELS, lib.RPN_MAX_PRE_NMS, lib.ROI_MAX_TAPS) == (rois.RPN_MAX_LEVELS, rois.RPN_MAX_PRE_NMS, rois.ROI_MAX_TAPS)
    assert rois.RPN_MAX_LEVELS * rois.RPN_MAX_PRE_NMS == boxes.NMS_MAX_BOXES
    # the decode lives once, in glue.h, and both units call it
    src = {n: open(os.path.join(ROOT, "edtr_amd", "csrc", n)).read() for n in ("glue.h", "boxes.hip", "rois.hip")}
    assert "f32x4 decode_box(" in src["glue.h"] and "decode_box(" in src["boxes.hip"] and "decode_box(" in src["rois.hip"]
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == 10 and all(hasattr(handle, s) for s in SYMBOLS)


def test_the_entry_points_reject_bad_arguments_before_any_launch():
    import ctypes as C
    from edtr_amd import build, lib
    build.build_library()
    h = lib.load()
    p = 4096            # a non-NULL, aligned stand-in: every call below fails its checks before the pointer is used
    NULL, SHAPE, ALIGN, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -5

    def table(rows):
        flat = [v for r in rows for v in r]
        return (C.c_int32 * len(flat))(*flat)

    def ptrs(*v):
        return (C.c_void_p * len(v))(*v)
    one = table([(4, 4, 3, 16, 16)])

    def select(**kw):
        a = dict(dt=0, obj=ptrs(p), levels=one, L=1, N=2, pre=100, sel=p)
        a.update(kw)
        return h.edtr_rpn_select(*a.values(), None)
    assert select(levels=None) == NULL and select(obj=None) == NULL and select(sel=None) == NULL and select(obj=ptrs(None)) == NULL
    assert select(L=0) == SHAPE and select(pre=0) == SHAPE and select(N=0) == SHAPE and select(levels=table([(0, 4, 3, 1, 1)])) == SHAPE
    assert select(L=9) == UNSUPPORTED and select(pre=4097) == UNSUPPORTED and select(N=65536) == UNSUPPORTED
    assert select(levels=table([(4096, 4096, 1, 1, 1)])) == UNSUPPORTED                      # 2^24 anchors on one level
    assert select(dt=3) == DTYPE and select(obj=ptrs(p + 2)) == ALIGN and select(dt=1, obj=ptrs(p + 1)) == ALIGN and select(sel=p + 2) == ALIGN

    def cand(**kw):
        a = dict(dt=0, obj=ptrs(p), deltas=ptrs(p), levels=one, L=1, N=2, pre=100, cells=p, sel=p, sizes=p, clip=4.0, min_size=1e-3, score=0.0,
                 boxes=p, probs=p, level=p, counts=p)
        a.update(kw)
        return h.edtr_rpn_candidates(*a.values(), None)
    assert cand(deltas=None) == NULL and cand(cells=None) == NULL and cand(counts=None) == NULL and cand(deltas=ptrs(None)) == NULL
    assert cand(N=0) == SHAPE and cand(L=9) == UNSUPPORTED and cand(dt=7) == DTYPE
    assert cand(cells=p + 4) == ALIGN and cand(boxes=p + 8) == ALIGN and cand(probs=p + 2) == ALIGN and cand(deltas=ptrs(p + 2)) == ALIGN

    def anchors(**kw):
        a = dict(levels=one, L=1, cells=p, out=p)
        a.update(kw)
        return h.edtr_rpn_anchors(*a.values(), None)
    assert anchors(cells=None) == NULL and anchors(levels=None) == NULL and anchors(L=0) == SHAPE and anchors(L=9) == UNSUPPORTED and anchors(out=p + 4) == ALIGN
    assert anchors(levels=table([(4, 4, 3, -1, 16)])) == SHAPE

    hw, sc = (C.c_int32 * 2)(4, 4), (C.c_float * 1)(0.25)

    def pool(**kw):
        a = dict(dt=0, feats=ptrs(p), hw=hw, scales=sc, L=1, N=1, C=8, rois=p, batch=p, K=5, P=7, S=2, k_min=2, k_max=2, s0=224.0, k0=4.0, out=p)
        a.update(kw)
        return h.edtr_roi_align(*a.values(), None)
    assert pool(feats=None) == NULL and pool(rois=None) == NULL and pool(batch=None) == NULL and pool(out=None) == NULL and pool(feats=ptrs(None)) == NULL
    assert pool(K=0) == SHAPE and pool(C=0) == SHAPE and pool(P=0) == SHAPE and pool(S=0) == SHAPE and pool(hw=(C.c_int32 * 2)(0, 4)) == SHAPE
    assert pool(scales=(C.c_float * 1)(0.0)) == SHAPE and pool(s0=0.0) == SHAPE and pool(k_max=1) == SHAPE
    assert pool(L=9) == UNSUPPORTED and pool(N=65536) == UNSUPPORTED and pool(P=9, S=8) == UNSUPPORTED
    assert pool(dt=5) == DTYPE and pool(rois=p + 8) == ALIGN and pool(out=p + 2) == ALIGN and pool(dt=2, feats=ptrs(p + 1)) == ALIGN
