"""Host side of edtr_amd/targets.py: the numpy restatements against the reference's own Matcher, BoxCoder.encode,
BalancedPositiveNegativeSampler, assign_targets_to_anchors, select_training_samples, compute_loss and fastrcnn_loss
(tests/golden/targets.npz, written by tools/make_targets_goldens.py), the NaN and first-maximum rules against torch.max, the sampler's
frequencies, the two new purposes of the seeded stream, the bounds and the C ABI.  No GPU."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

from edtr_amd import rng, rois, targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
N = 3


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "targets.npz"))


def source_of(gold):
    return rng.NoiseSource(int(gold["seed"]), gold["image_ids"].tolist())


def targets_of(gold):
    return [{"boxes": gold[f"gt_boxes{n}"], "labels": gold[f"gt_labels{n}"]} for n in range(N)]


@pytest.fixture(scope="module")
def rpn_flow(gold):
    high, low, batch, fraction = gold["rpn_params"]
    return targets.rpn_targets_reference(gold["anchors"], targets_of(gold), high=high, low=low, batch_size_per_image=int(batch),
                                         positive_fraction=fraction, source=source_of(gold), draw=int(gold["draw"]), log=targets.torch_log)


@pytest.fixture(scope="module")
def roi_flow(gold):
    high, low, batch, fraction = gold["roi_params"]
    return targets.roi_targets_reference([gold[f"roi_input{n}"] for n in range(N)], targets_of(gold), high=high, low=low,
                                         batch_size_per_image=int(batch), positive_fraction=fraction, weights=tuple(gold["roi_weights"]),
                                         source=source_of(gold), draw=int(gold["draw"]), log=targets.torch_log)


# ---- matching ----------------------------------------------------------------------------------------------------------------------------
def test_the_anchors_of_the_fixture_are_the_projects_own(gold):
    got = rois.anchors_reference(gold["grids"], gold["padded"], tuple(map(tuple, gold["sizes"])), tuple(map(tuple, gold["ratios"])))
    assert got.shape == (1512, 4) and np.array_equal(got, gold["anchors"]) and got.shape[0] > targets.TILE


def test_matcher_restatement_reproduces_the_all_zero_row_quirk(gold):
    assert targets.match_quality_reference(gold["q35"], 0.7, 0.3, True).tolist() == gold["q35_matched"].tolist() == [0, 2, 2, 0, 2]
    assert targets.match_quality_reference(gold["q35"], 0.7, 0.3, False).tolist() == gold["q35_plain"].tolist() == [0, -2, 2, -2, -1]


def test_match_restatement_equals_the_reference_on_the_fixture(gold):
    high, low = gold["rpn_params"][:2]
    got = targets.match_reference(gold["anchors"], [gold[f"gt_boxes{n}"] for n in range(N)], high, low, True)
    assert all(g.dtype == np.int32 for g in got) and np.array_equal(np.stack(got), gold["rpn_matched"])
    m0 = got[0]
    assert {-1, -2} <= set(m0.tolist()) and (m0 >= 0).any()                     # values on every side of both thresholds
    assert (got[1] == 0).all() and (got[2] == 0).all()                          # overlaps nothing: all restored; no ground truth: zeros
    # the midway box's two anchors are both restored; of the two identical boxes the first wins everywhere
    iou = targets.iou_reference(gold["gt_boxes0"], gold["anchors"])
    tied = np.nonzero(iou[1] == iou[1].max())[0]
    assert tied.size == 2 and iou[1].max() < F32(high) and (m0[tied] == 1).all()
    assert 3 in m0 and 4 not in m0
    quirk = targets.match_reference(gold["anchors"], [gold["gt6"]], high, low, True)[0]
    assert np.array_equal(quirk, gold["quirk6_matched"]) and (quirk >= 0).all()


def test_first_maximum_and_nan_rules_are_torch_max(gold):
    rs = np.random.default_rng(5)
    q = (rs.integers(0, 4, (6, 200)) / 4).astype(F32)                           # many ties
    q[2, 10] = q[4, 10] = np.nan
    q[5, 11] = np.nan
    q[:, 12] = 0.0
    val, idx = targets.best_reference(q)
    tv, ti = torch.from_numpy(q).max(dim=0)
    assert np.array_equal(idx, ti.numpy()) and np.array_equal(val, tv.numpy(), equal_nan=True)
    assert idx[10] == 2 and idx[11] == 5 and idx[12] == 0
    # a NaN best keeps its index through both thresholds; a NaN highest restores nothing
    m = targets.match_quality_reference(q, 0.7, 0.3, True)
    assert m[10] == 2 and m[11] == 5
    nan_row = np.array([[np.nan, 0.1, 0.1], [0.2, 0.5, 0.1]], dtype=F32)
    assert targets.match_quality_reference(nan_row, 0.7, 0.3, True).tolist() == [0, 1, -1]
    # NaN coordinates propagate through the IoU as torch's max / min / clamp do
    b = np.array([[0, 0, 4, 4], [np.nan, 0, 4, 4], [1, 1, 3, 3]], dtype=F32)
    t = torch.from_numpy(b)
    wh = (torch.min(t[:, None, 2:], t[:, 2:]) - torch.max(t[:, None, :2], t[:, :2])).clamp(min=0)
    area = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    inter = wh[..., 0] * wh[..., 1]
    assert np.array_equal(targets.iou_reference(b, b), (inter / (area[:, None] + area - inter)).numpy(), equal_nan=True)


# ---- the RPN flow ------------------------------------------------------------------------------------------------------------------------
def test_rpn_flow_restatement_equals_the_reference(gold, rpn_flow):
    f = rpn_flow
    assert np.array_equal(f["matched"], gold["rpn_matched"]) and f["labels"].dtype == F32 and np.array_equal(f["labels"], gold["rpn_labels"])
    want = gold["rpn_regression"]
    assert f["regression"].dtype == F32 and np.array_equal(f["regression"][..., :2], want[..., :2])                # dx, dy: bit for bit
    assert np.array_equal(f["regression"][..., 2:], want[..., 2:])                                                  # dw, dh: with torch's log
    assert np.isneginf(want[2, :, 2:]).all()                                                                        # no ground truth: the zero box
    assert np.array_equal(f["mask_pos"], gold["rpn_mask_pos"]) and np.array_equal(f["mask_neg"], gold["rpn_mask_neg"])
    assert f["mask_pos"].dtype == np.uint8 and np.array_equal(f["counts"], gold["rpn_counts"])
    assert gold["rpn_counts"].tolist() == [[5, 251], [128, 0], [0, 256]]        # fewer positives, more positives and no negative, none
    for n in range(N):
        k = int(f["counts"][n].sum())
        assert np.array_equal(f["sampled"][n, :k], np.nonzero(f["mask_pos"][n] | f["mask_neg"][n])[0]) and (f["sampled"][n, k:] == -1).all()
    # with numpy's log the last two columns stay within the measured tolerance
    mine = targets.rpn_targets_reference(gold["anchors"], targets_of(gold), source=source_of(gold), draw=int(gold["draw"]))["regression"]
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(mine), ok) and np.abs(mine[ok] - want[ok]).max() <= float(gold["tol_rpn_dwdh"])


def test_rpn_loss_meets_compute_loss(gold, rpn_flow):
    t = {k: torch.from_numpy(v) for k, v in rpn_flow.items()}
    obj = torch.from_numpy(gold["rpn_objectness"]).requires_grad_()
    deltas = torch.from_numpy(gold["rpn_deltas"]).requires_grad_()
    got = targets.rpn_loss(obj, deltas, t)
    for g, want, tol in zip(got, gold["rpn_loss"], gold["tol_rpn_loss"]):
        print(f"\n[rpn_loss] got {float(g.detach()):.9f} want {want:.9f} tol {tol:.2e}")
        assert abs(float(g.detach()) - want) <= tol
    (got[0] + got[1]).backward()
    picked = (t["mask_pos"] | t["mask_neg"]).reshape(-1).bool()
    assert torch.isfinite(obj.grad).all() and torch.isfinite(deltas.grad).all()
    assert (obj.grad.reshape(-1)[~picked] == 0).all() and (deltas.grad[~t["mask_pos"].reshape(-1).bool()] == 0).all()


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------
def test_sampler_restatement_on_equal_keys(gold):
    batch, fraction = gold["eq_params"]
    mp, mn, sampled, counts = targets.sample_reference([gold["eq_labels"]], int(batch), fraction, keys=[gold["eq_keys"]])
    assert np.array_equal(mp[0], gold["eq_mask_pos"]) and np.array_equal(mn[0], gold["eq_mask_neg"])
    # positives 0, 2, 5, 6, 11 with keys 5, 5, 5, 2, 7: three of them are 6, then 0 and 2 (equal keys go to the smaller index)
    assert np.nonzero(mp[0])[0].tolist() == [0, 2, 6] and np.nonzero(mn[0])[0].tolist() == [1, 4, 8]
    assert counts.tolist() == [[3, 3]] and sampled.tolist() == [[0, 1, 2, 4, 6, 8]]


def test_sampler_counts_are_the_references():
    src = rng.NoiseSource(1, [0])
    lab = np.array([1] * 3 + [0] * 2 + [-1] * 4)
    _, _, sampled, counts = targets.sample_reference([lab], 8, 0.5, src)
    assert counts.tolist() == [[3, 2]] and sampled[0].tolist() == [0, 1, 2, 3, 4, -1, -1, -1]          # fewer of both than asked
    assert targets.sample_reference([np.array([2, 3, 0, 0])], 4, 0.26, src)[3].tolist() == [[1, 2]]  # int(4 x 0.26) = 1
    assert targets.sample_reference([np.zeros(5)], 4, 0.5, src)[3].tolist() == [[0, 4]]


def test_sampler_selects_every_box_with_frequency_k_over_n():
    lab = np.array([1] * 10 + [0] * 12 + [-1] * 2)
    src = rng.NoiseSource(20281, [5])
    draws = 2000
    hits = np.zeros(lab.size)
    for d in range(draws):
        mp, mn, _, counts = targets.sample_reference([lab], 8, 0.5, src, draw=d, purpose=rng.PURPOSE_SAMPLE_ROI)
        hits += mp[0] + mn[0]
        assert counts.tolist() == [[4, 4]]
    for rows, p in ((slice(0, 10), 4 / 10), (slice(10, 22), 4 / 12)):
        sd = np.sqrt(p * (1 - p) / draws)
        assert np.abs(hits[rows] / draws - p).max() <= 5 * sd
    assert (hits[22:] == 0).all()


def test_the_sample_of_an_image_does_not_depend_on_its_batch():
    lab = [np.array([1, 0] * 20), np.array([0, 1, 1, 0] * 9)]
    both = targets.sample_reference(lab, 8, 0.5, rng.NoiseSource(3, [11, 12]), draw=4)
    alone = targets.sample_reference(lab[1:], 8, 0.5, rng.NoiseSource(3, [12]), draw=4)
    assert np.array_equal(both[0][1], alone[0][0]) and np.array_equal(both[2][1], alone[2][0])
    assert not np.array_equal(both[2][1], targets.sample_reference(lab[1:], 8, 0.5, rng.NoiseSource(3, [12]), draw=5)[2][0])


def test_the_sampler_purposes_are_raw_words_only():
    assert (rng.PURPOSE_SAMPLE_RPN, rng.PURPOSE_SAMPLE_ROI) == (8, 9)
    a, b = (rng.uniform_words_reference(3, [1, 9], p, 2, 16) for p in rng.SAMPLE_PURPOSES)
    assert a.dtype == np.uint32 and a.shape == (2, 16) and not np.array_equal(a, b)
    for p in rng.SAMPLE_PURPOSES:
        with pytest.raises(ValueError):
            rng.normal_reference(3, [1], p, 0, 16)
        with pytest.raises(ValueError):
            rng.stream_reference(3, [1], p, 0, 16)
    with pytest.raises(ValueError):
        rng.uniform_words_reference(3, [1], 10, 0, 16)
    with pytest.raises(ValueError):
        targets.sample_keys_reference(rng.NoiseSource(3, [1]), 5, 0, rng.PURPOSE_STEP, 0)
    assert np.array_equal(targets.sample_keys_reference(rng.NoiseSource(3, [1, 9]), 13, 2, 8, 1), a[1, :13])


# ---- the RoI flow ------------------------------------------------------------------------------------------------------------------------
def test_roi_flow_restatement_equals_the_reference(gold, roi_flow):
    f = roi_flow
    high, low = gold["roi_params"][:2]
    props = [np.concatenate([gold[f"roi_input{n}"], gold[f"gt_boxes{n}"]]) for n in range(N)]
    matched = targets.match_reference(props, [gold[f"gt_boxes{n}"] for n in range(N)], high, low, False)
    for n in range(N):
        assert props[n].shape[0] % 256 and np.array_equal(np.clip(matched[n], 0, None), gold[f"roi_all_matched{n}"])
        assert np.array_equal(targets.labels_reference(matched[n], "roi", gold[f"gt_labels{n}"]), gold[f"roi_all_labels{n}"])
        k = int(f["counts"][n].sum())
        assert k == gold[f"roi_labels{n}"].shape[0]
        assert np.array_equal(f["proposals"][n, :k], gold[f"roi_proposals{n}"]) and np.array_equal(f["labels"][n, :k], gold[f"roi_labels{n}"])
        assert np.array_equal(f["matched"][n, :k], gold[f"roi_matched{n}"]) and f["labels"].dtype == f["matched"].dtype == np.int64
        assert np.array_equal(f["regression_targets"][n, :k], gold[f"roi_targets{n}"])                     # all four columns, with torch's log
        assert (f["labels"][n, k:] == -1).all() and not f["proposals"][n, k:].any() and not f["regression_targets"][n, k:].any()
    assert f["counts"].tolist() == [[16, 48], [16, 48], [0, 64]]                    # more positives than int(64 x 0.25); none without ground truth


def test_fastrcnn_loss_meets_the_references(gold, roi_flow):
    t = {k: torch.from_numpy(v) for k, v in roi_flow.items()}
    logits = torch.from_numpy(gold["roi_logits"]).requires_grad_()
    regression = torch.from_numpy(gold["roi_box_regression"]).requires_grad_()
    got = targets.fastrcnn_loss(logits, regression, t)
    for g, want, tol in zip(got, gold["roi_loss"], gold["tol_roi_loss"]):
        print(f"\n[fastrcnn_loss] got {float(g.detach()):.9f} want {want:.9f} tol {tol:.2e}")
        assert abs(float(g.detach()) - want) <= tol
    (got[0] + got[1]).backward()
    assert torch.isfinite(logits.grad).all() and torch.isfinite(regression.grad).all()


def test_an_unfilled_slot_adds_nothing_to_the_losses(gold):
    """three boxes for a batch of 8: five slots stay empty, and the loss over all eight rows of logits is the reference's over the
    three it kept, within the tolerance the golden tool measured for this case"""
    tg = [{"boxes": gold["pad_gt"], "labels": gold["pad_label"]}]
    f = targets.roi_targets_reference([gold["pad_props"]], tg, batch_size_per_image=8, source=rng.NoiseSource(int(gold["seed"]), gold["image_ids"][:1]),
                                      draw=int(gold["draw"]), log=targets.torch_log)
    assert f["counts"].tolist() == [[2, 1]] and f["labels"][0].tolist() == [3, 0, 3, -1, -1, -1, -1, -1]
    t = {k: torch.from_numpy(v) for k, v in f.items()}
    got = targets.fastrcnn_loss(torch.from_numpy(gold["pad_logits"]), torch.from_numpy(gold["pad_box_regression"]), t)
    for g, want, tol in zip(got, gold["pad_loss"], gold["tol_pad_loss"]):
        print(f"\n[fastrcnn_loss, 3 of 8 slots] got {float(g):.9f} want {want:.9f} tol {tol:.2e}")
        assert abs(float(g) - want) <= tol


# ---- bounds and the C ABI ----------------------------------------------------------------------------------------------------------------
def test_bounds_raise_value_error():
    box = np.array([[0, 0, 4, 4]], dtype=F32)
    with pytest.raises(ValueError):
        targets.ragged_table([5], [targets.MAX_GT + 1])
    with pytest.raises(ValueError):
        targets.ragged_table([1 << 24], [1])
    with pytest.raises(ValueError):
        targets.ragged_table([1] * 65536, [0] * 65536)
    with pytest.raises(ValueError):
        targets.ragged_table([0], [1])
    assert targets.ragged_table([3, 2], [1, 0]) == [(0, 0), (3, 1), (5, 1)]
    with pytest.raises(ValueError):
        targets.sample_reference([np.zeros(4)], targets.MAX_BATCH + 1, 0.5, rng.NoiseSource(1, [0]))
    with pytest.raises(ValueError):
        targets.sample_reference([np.zeros(4)], 8, 1.5, rng.NoiseSource(1, [0]))
    with pytest.raises(ValueError):
        targets.match_reference(box, [box], 0.3, 0.7, False)
    with pytest.raises(ValueError):
        targets.match_reference(box, [np.zeros((targets.MAX_GT + 1, 4), dtype=F32)], 0.7, 0.3, False)


SYMBOLS = ("edtr_targets_match", "edtr_targets_encode", "edtr_targets_sample", "edtr_targets_gather")


def test_the_new_symbols_are_declared_bound_exported_and_the_abi_is_still_10():
    from edtr_amd import build, lib
    assert all(s in lib.DECLARED_SYMBOLS for s in SYMBOLS)
    assert lib.ABI_VERSION == 10
    assert "targets.hip" in build.GLUE_SOURCES and "targets.hip" not in build.SOURCES
    deps = [os.path.basename(d) for d in build.object_deps("targets.hip")]
    assert "glue.h" in deps and "philox.h" in deps
    caps = (lib.TARGETS_MAX_GT, lib.TARGETS_MAX_BATCH, lib.TARGETS_TILE, lib.TARGETS_RPN, lib.TARGETS_ROI)
    assert caps == (targets.MAX_GT, targets.MAX_BATCH, targets.TILE, targets.FORM_RPN, targets.FORM_ROI)
    assert (lib.NOISE_SAMPLE_RPN, lib.NOISE_SAMPLE_ROI) == rng.SAMPLE_PURPOSES
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

    def table(*rows):
        flat = [v for r in rows for v in r]
        return (C.c_int32 * len(flat))(*flat)
    two = table((0, 0), (10, 2), (25, 2))
    w = (C.c_float * 4)(1, 1, 1, 1)

    def match(**kw):
        a = dict(boxes=p, shared=0, gt=p, gl=p, th=two, t=p, N=2, high=0.7, low=0.3, allow=1, form=0, w=w, bv=p, bi=p, part=p, words=4, m=p, lab=p, reg=p)
        a.update(kw)
        return h.edtr_targets_match(*a.values(), None)
    assert match(th=None) == NULL and match(t=None) == NULL and match(boxes=None) == NULL and match(gt=None) == NULL and match(part=None) == NULL
    assert match(form=1, gl=None) == NULL and match(w=None) == NULL and match(lab=None) == NULL
    assert match(N=0) == SHAPE and match(th=table((1, 0), (10, 2), (25, 2))) == SHAPE and match(th=table((0, 0), (0, 2), (25, 2))) == SHAPE
    assert match(high=0.3, low=0.7) == SHAPE and match(high=float("nan")) == SHAPE and match(words=3) == SHAPE and match(shared=1) == SHAPE
    assert match(w=(C.c_float * 4)(1, float("nan"), 1, 1)) == SHAPE
    assert match(N=65536) == UNSUPPORTED and match(th=table((0, 0), (10, 1025), (25, 1025))) == UNSUPPORTED
    assert match(th=table((0, 0), (1 << 24, 1), ((1 << 24) + 5, 1))) == UNSUPPORTED
    assert match(form=2) == DTYPE and match(allow=2) == DTYPE and match(shared=2) == DTYPE
    assert match(boxes=p + 4) == ALIGN and match(gt=p + 8) == ALIGN and match(reg=p + 4) == ALIGN and match(m=p + 2) == ALIGN
    assert match(form=1, lab=p + 4) == ALIGN and match(form=1, gl=p + 4) == ALIGN

    def encode(**kw):
        a = dict(ref=p, prop=p, K=5, w=w, out=p)
        a.update(kw)
        return h.edtr_targets_encode(*a.values(), None)
    assert encode(ref=None) == NULL and encode(w=None) == NULL and encode(out=None) == NULL and encode(K=0) == SHAPE
    assert encode(K=(1 << 30) + 1) == UNSUPPORTED and encode(prop=p + 4) == ALIGN and encode(out=p + 8) == ALIGN

    def sample(**kw):
        a = dict(lab=p, form=0, th=two, t=p, N=2, batch=256, max_pos=128, seed=1, ids=None, base=0, draw=0, purpose=8, keys=None, mp=p, mn=p, s=p, c=p)
        a.update(kw)
        return h.edtr_targets_sample(*a.values(), None)
    assert sample(lab=None) == NULL and sample(th=None) == NULL and sample(mp=None) == NULL and sample(c=None) == NULL
    assert sample(batch=0) == SHAPE and sample(max_pos=257) == SHAPE and sample(max_pos=-1) == SHAPE and sample(draw=1 << 32) == SHAPE
    assert sample(base=-1) == SHAPE and sample(batch=4097, max_pos=0) == UNSUPPORTED and sample(N=65536) == UNSUPPORTED
    assert sample(purpose=1) == DTYPE and sample(purpose=10) == DTYPE and sample(form=3) == DTYPE
    assert sample(lab=p + 2) == ALIGN and sample(form=1, lab=p + 4) == ALIGN and sample(s=p + 2) == ALIGN and sample(ids=p + 4) == ALIGN and sample(keys=p + 2) == ALIGN

    def gather(**kw):
        a = dict(boxes=p, gt=p, m=p, lab=p, th=two, t=p, N=2, s=p, batch=64, w=w, ob=p, ol=p, om=p, ot=p)
        a.update(kw)
        return h.edtr_targets_gather(*a.values(), None)
    assert gather(boxes=None) == NULL and gather(gt=None) == NULL and gather(s=None) == NULL and gather(w=None) == NULL and gather(ot=None) == NULL
    assert gather(batch=0) == SHAPE and gather(batch=4097) == UNSUPPORTED and gather(th=table((0, 0), (10, 2000), (25, 2000))) == UNSUPPORTED
    assert gather(boxes=p + 4) == ALIGN and gather(ol=p + 4) == ALIGN and gather(ot=p + 8) == ALIGN and gather(s=p + 2) == ALIGN
