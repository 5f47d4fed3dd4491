"""The launches of edtr_amd/rois.py (csrc/rois.hip) against their numpy restatements: by equality wherever neither exp nor log2 enters.
Where exp enters (decoding, sigmoid) the hand-built cases are chosen so that it is exact or cut away, and the seeded ones are compared
within the bound tests/test_gpu_boxes.py uses (1e-5 relative) on inputs whose decisions the golden tool kept clear; the NMS is then
restated from the device's own candidates, so that one ulp of exp cannot flip an order.  Where log2 enters (the level of a roi) every
roi lies at least 1e-3 from a level boundary, which makes the level integer-exact."""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from edtr_amd import boxes, coco, rois

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32 = np.float32
TORCH_DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "proposals.npz"))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.float().cpu().numpy() if isinstance(t, torch.Tensor) and t.is_floating_point() else (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))


def nested(a):
    return tuple(tuple(float(v) for v in row) for row in a)


# ---- anchors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["v2", "mobilenet", "ragged"])
def test_anchors_launch_equals_the_reference_bit_for_bit(gold, tag):
    args = (gold[f"anchors_{tag}_grids"], gold[f"anchors_{tag}_padded"], nested(gold[f"anchors_{tag}_sizes"]), nested(gold[f"anchors_{tag}_ratios"]))
    got = rois.anchors(*args)
    assert got.dtype == torch.float32 and got.is_cuda and np.array_equal(host(got), gold[f"anchors_{tag}"])
    assert np.array_equal(host(got), rois.anchors_reference(*args))


# ---- select ----------------------------------------------------------------------------------------------------------------------------
# level sizes 1, 63, 64, 65, 1000, 1001, 4097 and one that takes many rounds of the 1024-lane workgroup, as (A, H, W): with A > 1 the
# memory order differs from the logical order.  (70 000 is no multiple of 3; 3 x 6 x 3889 = 70 002 is the next size with A = 3.)
SELECT_LEVELS = [(1, 1, 1), (3, 3, 7), (1, 8, 8), (5, 1, 13), (2, 20, 25), (7, 11, 13), (1, 17, 241), (3, 6, 3889)]
_SELECT = {}


def select_case(kind):
    """two images with different contents per level, shared by the tests that need it and left unchanged.
    "ties": image 0 holds sixteenths (every key many times: the threshold bucket straddles any cut), image 1 one value only;
    "special": NaN, +-inf, +-0.0 and denormals repeated, against unit normals in image 1;
    "normal": unit normals times 3 (no ties), image 1 negated so that the keys of both signs are exercised"""
    if kind not in _SELECT:
        rng = np.random.default_rng([11, len(kind)])
        out = []
        for A, H, W in SELECT_LEVELS:
            n = A * H * W
            if kind == "ties":
                a = np.stack([rng.integers(-8, 9, n) / 16, np.full(n, 0.25)])
            elif kind == "special":
                pool = np.array([0.1, np.nan, -0.0, 0.0, np.inf, -np.inf, -np.nan, 0.1, 1e-40, -1e-40, 2.5, -2.5], dtype=F32)
                a = np.stack([pool[rng.integers(0, len(pool), n)], rng.normal(0, 1, n)])
            else:
                a = rng.normal(0, 3, n)
                a = np.stack([a, -a])
            out.append(a.astype(F32).reshape(2, A, H, W))
        _SELECT[kind] = out
    return _SELECT[kind]


@pytest.mark.parametrize("pre", [1, 100, 1000, 4096])
@pytest.mark.parametrize("kind", ["normal", "ties", "special"])
def test_select_equals_the_restatement_index_for_index(kind, pre):
    """k = 1, k cutting through runs of equal keys, k >= the level's size (every level but the last two at 4096)"""
    obj = select_case(kind)
    want = rois.select_reference(obj, pre)
    got = rois.rpn_select([dev(o) for o in obj], pre)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(host(got), want)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_select_widens_sixteen_bit_scores_exactly(dt):
    obj = [dev(o, TORCH_DT[dt]) for o in select_case("normal")]             # rounding to 16 bits makes ties of its own
    want = rois.select_reference([host(o) for o in obj], 1000)
    assert np.array_equal(host(rois.rpn_select(obj, 1000)), want)
    spec = [dev(o, TORCH_DT[dt]) for o in select_case("special")]
    assert np.array_equal(host(rois.rpn_select(spec, 64)), rois.select_reference([host(o) for o in spec], 64))


def test_select_takes_a_non_contiguous_view_and_rejects_what_is_out_of_bounds():
    o = dev(select_case("normal")[5])
    view = o.permute(0, 1, 3, 2)                                            # [2, 7, 13, 11], strided
    assert not view.is_contiguous()
    assert np.array_equal(host(rois.rpn_select([view], 50)), rois.select_reference([host(view)], 50))
    with pytest.raises(ValueError):
        rois.rpn_select([o], 4097)
    with pytest.raises(ValueError):
        rois.rpn_select([o] * 9, 10)
    with pytest.raises(TypeError):
        rois.rpn_select([o.double()], 10)


# ---- candidates ------------------------------------------------------------------------------------------------------------------------
def test_candidates_hand_built_bit_for_bit():
    """deltas beyond the clamp (cut by the image), a box leaving the image, one thinner than min_size, score_thresh 0.5, a level that
    contributes nothing; every exp that survives is exp(0) = 1, so the boxes are equal bit for bit"""
    sizes, ratios = ((8,), (16,)), ((1.0,), (1.0,))
    obj = [np.full((2, 1, 2, 2), 2.0, dtype=F32), np.full((2, 1, 1, 1), -3.0, dtype=F32)]
    deltas = [np.zeros((2, 4, 2, 2), dtype=F32), np.zeros((2, 4, 1, 1), dtype=F32)]
    deltas[0][0, 2, 0, 0] = 9.0
    deltas[0][0, 0, 0, 1] = 10.0
    deltas[0][0, 3, 1, 0] = -12.0
    obj[0][0, 0, 1, 1] = -1.0
    obj[1][1] = 3.0                                                         # image 1: every level contributes, clipped to 12 x 14
    image_sizes = [(16, 20), (12, 14)]
    for thresh in (0.5, 0.0):
        sel = rois.rpn_select([dev(o) for o in obj], 10)
        want = rois.candidates_reference(obj, deltas, host(sel), image_sizes, (16, 20), sizes, ratios, 10, score_thresh=thresh)
        b, p, lvl, counts = rois.rpn_candidates([dev(o) for o in obj], [dev(d) for d in deltas], sel, image_sizes, (16, 20), sizes, ratios, 10,
                                                score_thresh=thresh)
        assert host(counts).tolist() == [len(w[0]) for w in want]
        for n, (wb, wp, wl) in enumerate(want):
            m = len(wb)
            assert np.array_equal(host(b[n, :m]), wb) and host(lvl[n, :m]).tolist() == wl.tolist()
            np.testing.assert_allclose(host(p[n, :m]), wp, rtol=1e-5, atol=0)
    assert want[0][2].tolist() == [0, 0, 1] and want[1][2].tolist() == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_proposals_on_the_recorded_head_outputs(gold, tag, dt):
    """staged: the selection by equality; the candidates' count and levels by equality, boxes and probabilities within 1e-5 relative
    (boxes to an absolute 1e-5 of a pixel as well: a candidate, unlike a kept box, may hug the origin); the NMS by equality with the
    restatement run on the device's own candidates.  In fp32 the result also meets the reference's recorded filter_proposals output."""
    L = len(gold["rpn_sizes"])
    obj = [dev(gold[f"rpn_objectness{l}"], TORCH_DT[dt]) for l in range(L)]
    deltas = [dev(gold[f"rpn_deltas{l}"], TORCH_DT[dt]) for l in range(L)]
    image_sizes, padded = [tuple(s) for s in gold["rpn_image_sizes"]], tuple(gold["rpn_padded"])
    (pre, post), (nms, score) = gold[f"rpn_{tag}_top_n"], gold[f"rpn_{tag}_thresh"]
    kw = dict(sizes=nested(gold["rpn_sizes"]), aspect_ratios=nested(gold["rpn_ratios"]))
    trace = {}
    got = rois.proposals(obj, deltas, image_sizes, padded, pre_nms_top_n=int(pre), post_nms_top_n=int(post), nms_thresh=float(nms),
                         score_thresh=float(score), trace=trace, **kw)
    h_obj, h_del = [host(o) for o in obj], [host(d) for d in deltas]
    sel = rois.select_reference(h_obj, int(pre))
    assert np.array_equal(host(trace["selected"]), sel)
    cand = rois.candidates_reference(h_obj, h_del, sel, image_sizes, padded, kw["sizes"], kw["aspect_ratios"], int(pre), float(score))
    counts = host(trace["cand_counts"]).tolist()
    assert counts == [len(c[0]) for c in cand]
    own = []
    for n, (cb, cp, cl) in enumerate(cand):
        db, dp, dl = (host(trace[k][n, :counts[n]]) for k in ("cand_boxes", "cand_probs", "cand_level"))
        assert dl.tolist() == cl.tolist()
        np.testing.assert_allclose(db, cb, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(dp, cp, rtol=1e-5, atol=0)
        own.append((db, dp, dl))
    want = rois.nms_stage_reference(own, float(nms), int(post))
    for n, ((b, s), (wb, ws)) in enumerate(zip(got, want)):
        assert b.dtype == torch.float32 and b.is_cuda and np.array_equal(host(b), wb) and np.array_equal(host(s), ws)
        if dt == "fp32":
            assert host(b).shape == gold[f"rpn_{tag}_boxes{n}"].shape
            np.testing.assert_allclose(host(b), gold[f"rpn_{tag}_boxes{n}"], rtol=1e-5, atol=0)
            np.testing.assert_allclose(host(s), gold[f"rpn_{tag}_scores{n}"], rtol=1e-5, atol=0)


# ---- RoIAlign --------------------------------------------------------------------------------------------------------------------------
PYRAMID = [(25, 42), (13, 21), (7, 11)]             # a 100 x 168 image at 1/4, 1/8, 1/16, as an FPN on odd extents gives them
IMAGE_SIZES = [(100, 168), (90, 150)]
_ROI = {}


def features_case(C, levels=PYRAMID, N=2, seed=5):
    key = (C, tuple(levels), N, seed)
    if key not in _ROI:
        rng = np.random.default_rng([seed, C])
        _ROI[key] = [rng.normal(0, 1, (N, C, h, w)).astype(F32) for h, w in levels]
    return _ROI[key]


def roi_case(k, image_sizes=IMAGE_SIZES, seed=1, lo=2.0, hi=5.0):
    """k random rois per image whose mapper value 4 + log2(s / 224) is uniform in [lo, hi] and at least 1e-3 from an integer (asserted,
    not filtered: the seed is fixed), plus per image the rois that leave it on each side, lie wholly outside it, are narrower than a
    feature pixel and end exactly at its edge"""
    key = (k, tuple(image_sizes), seed, lo, hi)
    if key not in _ROI:
        rng = np.random.default_rng([seed, k])
        out = []
        for h, w in image_sizes:
            s = 224.0 * 2.0 ** (rng.uniform(lo, hi, k) - 4.0)
            aspect = rng.uniform(0.6, 1.6, k)
            bw, bh = s * np.sqrt(aspect), s / np.sqrt(aspect)
            x1, y1 = rng.uniform(-8, w * 0.7, k), rng.uniform(-8, h * 0.7, k)
            hand = [[-30, 5, 12, 30], [w - 10, 5, w + 40, 30], [5, -30, 30, 12], [5, h - 10, 30, h + 40], [-200, -200, -120, -150],
                    [w + 100, h + 100, w + 160, h + 190], [10.2, 11.1, 10.5, 11.3], [w - 20, h - 20, w, h], [0, 0, w, h]]
            out.append(np.concatenate([np.stack([x1, y1, x1 + bw, y1 + bh], axis=1), np.array(hand, dtype=np.float64)]).astype(F32))
        d = np.concatenate(out).astype(np.float64)
        value = 4.0 + np.log2(np.sqrt((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])) / 224.0)
        assert np.abs(value - np.round(value)).min() >= 1e-3, "pick another seed: a roi lies on a level boundary"
        _ROI[key] = out
    return _ROI[key]


@pytest.mark.parametrize("C", [1, 3, 64, 65, 256])
def test_roi_align_equals_the_restatement_bit_for_bit(C):
    """rois of two images on three levels, every level used; the channel counts straddle the workgroup's chunk of 64"""
    feats, per_image = features_case(C), roi_case(6)
    want = rois.roi_align_reference(feats, per_image, IMAGE_SIZES)
    got = rois.roi_align(OrderedDict((str(i), dev(f)) for i, f in enumerate(feats)), [dev(r) for r in per_image], IMAGE_SIZES)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (2 * 15, C, 7, 7)
    assert np.array_equal(host(got), want)
    flat = np.concatenate(per_image)
    assert set(rois.roi_levels_reference(flat, 2, 4).tolist()) == {0, 1, 2}
    assert np.all(want[[10, 11, 25, 26]] == 0) and np.any(want[[6, 7, 8, 9, 12, 13, 14]] != 0)           # wholly outside; on the borders


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (25, 42)])
def test_roi_align_single_level_form(hw):
    """one level: no mapper.  A 1 x 1 and a 2 x 3 map take the y_low >= H - 1 branch for every sample; other bin and sample counts"""
    image = [(hw[0] * 4, hw[1] * 4)] * 2
    feats, per_image = features_case(3, [hw]), roi_case(5, tuple(image), seed=2)
    for P, S in ((7, 2), (3, 3), (1, 1), (8, 8)):
        want = rois.roi_align_reference(feats, per_image, image, P, S)
        assert np.array_equal(host(rois.roi_align([dev(f) for f in feats], [dev(r) for r in per_image], image, P, S)), want)


def test_roi_align_counts_of_rois():
    """K = 0 (no launch), 1, 1000; an image without rois; only one level of three used"""
    feats = features_case(3)
    d = [dev(f) for f in feats]
    empty = rois.roi_align(d, [torch.zeros((0, 4), device=DEV)] * 2, IMAGE_SIZES)
    assert tuple(empty.shape) == (0, 3, 7, 7) and empty.dtype == torch.float32
    one = [np.zeros((0, 4), dtype=F32), np.array([[3.5, 4.25, 60.0, 44.0]], dtype=F32)]
    assert np.array_equal(host(rois.roi_align(d, [dev(r) for r in one], IMAGE_SIZES)), rois.roi_align_reference(feats, one, IMAGE_SIZES))
    many = roi_case(491, seed=16)                                           # 2 x (491 + 9) = 1000
    assert sum(len(r) for r in many) == 1000
    assert np.array_equal(host(rois.roi_align(d, [dev(r) for r in many], IMAGE_SIZES)), rois.roi_align_reference(feats, many, IMAGE_SIZES))
    small = [r[:5] * F32(0.05) for r in roi_case(6)]                        # everything far below k_min: the finest level only
    assert set(rois.roi_levels_reference(np.concatenate(small), 2, 4).tolist()) == {0}
    assert np.array_equal(host(rois.roi_align(d, [dev(r) for r in small], IMAGE_SIZES)), rois.roi_align_reference(feats, small, IMAGE_SIZES))


def test_roi_align_level_mapper_on_the_recorded_boxes(gold):
    """the 2000 recorded boxes (at least 1e-3 from every level boundary) and the hand-built ones: each level's plane holds its own
    index, so the pooled value names the level the device chose"""
    levels = [(64, 64), (32, 32), (16, 16), (8, 8)]
    feats = [np.full((1, 1, h, w), float(l + 1), dtype=F32) for l, (h, w) in enumerate(levels)]
    boxes_in = np.concatenate([gold["map_rois"], gold["map_hand_rois"]])
    want = rois.roi_levels_reference(boxes_in, 2, 5)
    fp64 = np.clip(np.floor(np.concatenate([gold["map_value"], gold["map_hand_value"]])), 2, 5).astype(np.int64) - 2
    assert want.tolist() == fp64.tolist()
    # 8 x 8 bins of one sample: the sample of bin (0, 0) lies a sixteenth of the roi from its corner, inside the map for all but the
    # hand-built roi of 30 000 x 20 000.  (Four weights that sum to 1 within rounding: the value is the level's index to 1e-6.)
    got = host(rois.roi_align([dev(f) for f in feats], [dev(boxes_in)], [(256, 256)], 8, 1))[:, 0, 0, 0]
    inside = got != 0
    assert inside.sum() == len(boxes_in) - 1 and np.abs(got - np.rint(got)).max() < 1e-5
    assert (np.rint(got[inside]) - 1).astype(np.int64).tolist() == want[inside].tolist()


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_roi_align_widens_sixteen_bit_features_exactly(dt):
    feats = [dev(f, TORCH_DT[dt]) for f in features_case(5)]
    per_image = roi_case(6)
    want = rois.roi_align_reference([host(f) for f in feats], per_image, IMAGE_SIZES)
    assert np.array_equal(host(rois.roi_align(feats, [dev(r) for r in per_image], IMAGE_SIZES)), want)


def test_roi_align_copies_a_non_contiguous_view_and_rejects_bad_arguments():
    feats, per_image = features_case(6), roi_case(6)
    views = [dev(f)[:, ::2] for f in feats]                                 # every second channel, strided
    assert not views[0].is_contiguous()
    want = rois.roi_align_reference([f[:, ::2] for f in feats], per_image, IMAGE_SIZES)
    assert np.array_equal(host(rois.roi_align(views, [dev(r) for r in per_image], IMAGE_SIZES)), want)
    d = [dev(f) for f in feats]
    with pytest.raises(ValueError):
        rois.roi_align(d, [dev(r) for r in per_image], IMAGE_SIZES, 9, 8)           # 72 taps per axis
    with pytest.raises(ValueError):
        rois.roi_align(d, [dev(r) for r in per_image], IMAGE_SIZES, 7, 0)           # the adaptive ratio is not provided
    with pytest.raises(ValueError):
        rois.roi_align(d, [dev(per_image[0])], IMAGE_SIZES)                         # one list of rois for two images
    with pytest.raises(ValueError):
        rois.roi_align([d[0], d[2]], [dev(r) for r in per_image], IMAGE_SIZES)      # levels 2 and 4 without 3
    with pytest.raises(TypeError):
        rois.roi_align([f.double() for f in d], [dev(r) for r in per_image], IMAGE_SIZES)


# ---- the composed detector -------------------------------------------------------------------------------------------------------------
class RpnHead(torch.nn.Module):
    def __init__(self, C, A):
        super().__init__()
        self.conv, self.cls, self.box = torch.nn.Conv2d(C, C, 3, padding=1), torch.nn.Conv2d(C, A, 1), torch.nn.Conv2d(C, 4 * A, 1)

    def forward(self, feats):
        hidden = [torch.relu(self.conv(f)) for f in feats]
        return [self.cls(h) * 4 for h in hidden], [self.box(h) for h in hidden]


class Predictor(torch.nn.Module):
    def __init__(self, D, classes):
        super().__init__()
        self.cls, self.box = torch.nn.Linear(D, classes), torch.nn.Linear(D, 4 * classes)

    def forward(self, x):
        return self.cls(x) * 6, self.box(x)


def test_assemble_detector_equals_the_flow_through_the_restatements():
    """seeded two-layer stand-ins for the four learned parts, a 64 x 96 image padded into a 64 x 96 batch next to a 50 x 81 one, 3
    levels.  Staged: every non-learned step is restated on the host from what the device's step was given (the trace), so that the
    learned parts' own rounding, which differs between a CPU and a GPU, is not what is compared."""
    torch.manual_seed(7)
    C, A, classes = 8, 3, 5
    stem = torch.nn.Conv2d(3, C, 3, padding=1).to(DEV)
    rpn_head = RpnHead(C, A).to(DEV)
    box_head = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(C * 49, 32), torch.nn.ReLU()).to(DEV)
    predictor = Predictor(32, classes).to(DEV)
    sizes_in = [(64, 96), (50, 81)]

    def features_fn(images):
        batch = torch.zeros((len(images), 3, 64, 96), device=DEV)
        for n, im in enumerate(images):
            batch[n, :, :im.shape[1], :im.shape[2]] = im
        x = torch.relu(stem(batch))
        feats = OrderedDict((str(l), torch.nn.functional.avg_pool2d(x, 4 * 2 ** l).contiguous()) for l in range(3))
        return batch, sizes_in[:len(images)], [(128, 192), (75, 120)][:len(images)], feats

    kw = dict(sizes=((8,), (16,), (32,)), aspect_ratios=((0.5, 1.0, 2.0),) * 3, rpn_pre_nms_top_n=100, rpn_post_nms_top_n=40, box_score_thresh=0.05,
              box_detections_per_img=20)
    rng = np.random.default_rng(9)
    images = [dev(rng.random((3, h, w), dtype=F32)) for h, w in sizes_in]
    trace, ref_trace = {}, {}
    out = rois.assemble_detector(features_fn, rpn_head, box_head, predictor, trace=trace, **kw)(images)
    want = rois.assemble_detector_reference(features_fn, rpn_head, box_head, predictor, replay=trace, trace=ref_trace, **kw)(images)

    assert np.array_equal(host(trace["selected"]), ref_trace["selected"])
    counts = host(trace["cand_counts"]).tolist()
    assert counts == [len(c[0]) for c in ref_trace["candidates"]]
    for n, (cb, cp, cl) in enumerate(ref_trace["candidates"]):
        np.testing.assert_allclose(host(trace["cand_boxes"][n, :counts[n]]), cb, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(host(trace["cand_probs"][n, :counts[n]]), cp, rtol=1e-5, atol=0)
    # from here on the restatement is fed the device's proposals: its own differ from them by an ulp of exp
    props = [(host(b), host(s)) for b, s in trace["proposals"]]
    for (b, s), (wb, ws) in zip(props, ref_trace["proposals"]):
        assert 0 < len(b) <= 40 and b.shape == wb.shape
        np.testing.assert_allclose(b, wb, rtol=1e-5, atol=1e-5)
        assert np.array_equal(s, ws)                                        # the replayed probabilities
    feats = [host(f) for f in trace["features"].values()]
    pooled = rois.roi_align_reference(feats, [b for b, _ in props], sizes_in)
    d = np.concatenate([b for b, _ in props]).astype(np.float64)
    value = 4.0 + np.log2(np.maximum(np.sqrt(np.maximum((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]), 0)), 1e-30) / 224.0)
    clear = np.abs(value - np.round(value)) >= 1e-3                         # a proposal on a level boundary may go either way
    assert clear.sum() >= len(d) - 2 and np.array_equal(host(trace["pooled"])[clear], pooled[clear])
    start = 0
    for n, (b, _) in enumerate(props):
        rows = slice(start, start + len(b))
        start += len(b)
        det = boxes.detections_reference(host(trace["class_logits"][rows]), host(trace["box_regression"][rows]), b, sizes_in[n], 0.05, 0.5, 20)
        det["boxes"] = boxes.resize_boxes_reference(det["boxes"], sizes_in[n], [(128, 192), (75, 120)][n])
        assert host(out[n]["labels"]).tolist() == det["labels"].tolist() and out[n]["labels"].dtype == torch.int64
        np.testing.assert_allclose(host(out[n]["boxes"]), det["boxes"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(host(out[n]["scores"]), det["scores"], rtol=1e-5, atol=0)
        assert want[n]["labels"].tolist() == det["labels"].tolist()         # the whole flow on the host, from its own proposals
        np.testing.assert_allclose(want[n]["boxes"], det["boxes"], rtol=1e-5, atol=1e-5)
    assert len(out) == len(want) == 2 and all(set(o) == {"boxes", "scores", "labels"} for o in out)

    # the output is what coco.evaluate takes
    detnet = rois.assemble_detector(features_fn, rpn_head, box_head, predictor, **kw)
    _, gt = coco.scene(np.random.default_rng(4), 0, 6, n_labels=classes, image_id=1)
    res = coco.evaluate([images[0]], [gt], lambda ims: detnet(ims), n_labels=classes)
    assert res["stats"].shape == (12,) and "mAP@0.5" in res


# ---- symbols and errors ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve_and_the_abi_is_still_10():
    from edtr_amd import lib
    handle = lib.load()
    assert handle.edtr_abi_version() == 10
    for name in ("edtr_rpn_anchors", "edtr_rpn_select", "edtr_rpn_candidates", "edtr_roi_align"):
        assert name in lib.DECLARED_SYMBOLS and getattr(handle, name) is not None


def test_shape_null_and_alignment_errors_answer_the_error_codes():
    import ctypes as C
    from edtr_amd import lib
    h = lib.load()
    x = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = x.data_ptr()
    one = (C.c_int32 * 5)(4, 4, 3, 16, 16)
    tab = (C.c_void_p * 1)(p)
    assert h.edtr_rpn_select(0, tab, one, 1, 2, 100, None, None) == -1
    assert h.edtr_rpn_select(0, tab, one, 1, 0, 100, p, None) == -2
    assert h.edtr_rpn_select(0, tab, one, 1, 2, 100, p + 2, None) == -3
    assert h.edtr_rpn_select(9, tab, one, 1, 2, 100, p, None) == -4
    assert h.edtr_rpn_select(0, tab, one, 1, 2, 4097, p, None) == -5
    hw, sc = (C.c_int32 * 2)(4, 4), (C.c_float * 1)(0.25)
    assert h.edtr_roi_align(0, tab, hw, sc, 1, 1, 8, p + 8, p, 5, 7, 2, 2, 2, 224.0, 4.0, p, None) == -3
    assert h.edtr_roi_align(0, tab, hw, sc, 1, 1, 8, p, None, 5, 7, 2, 2, 2, 224.0, 4.0, p, None) == -1
    assert h.edtr_roi_align(0, tab, hw, sc, 1, 1, 8, p, p, 0, 7, 2, 2, 2, 224.0, 4.0, p, None) == -2
    assert h.edtr_roi_align(0, tab, hw, sc, 1, 1, 8, p, p, 5, 9, 8, 2, 2, 224.0, 4.0, p, None) == -5
    torch.cuda.synchronize()
