"""The detection-score rule on the host (edtr_amd/coco.py): the numpy restatement of COCO's per-image matching against an independent
per-pair scalar writing of the same rule, with every branch of the walk shown to be taken; `accumulate` / `summarize` against closed
forms; the handling of records (shards, duplicates, the image-id order); and the C ABI's checks of `edtr_coco_match`, which refuse
bad arguments before any launch.  No GPU is needed."""
import os
import re

import numpy as np

from edtr_amd import coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
EPS = 2.0 ** -52            # np.spacing(1): the term in precision's denominator
TOL = 1e-12                 # absorbs that term's 2e-16 and nothing else


def scenes(seed, n, d, g, n_labels, **kw):
    rng = np.random.default_rng(seed)
    return [coco.scene(rng, d, g, n_labels, image_id=i, **kw) for i in range(n)]


def assert_records_equal(a, b):
    for name, dtype in coco.DET_FIELDS + coco.GT_FIELDS:
        assert a[name].dtype == np.dtype(dtype) == b[name].dtype, name
        assert np.array_equal(a[name], b[name]), name


def target(boxes, labels, image_id, iscrowd=None):
    t = {"boxes": np.array(boxes, dtype=F32).reshape(-1, 4), "labels": np.array(labels, dtype=np.int64), "image_id": image_id}
    if iscrowd is not None:
        t["iscrowd"] = np.array(iscrowd, dtype=np.int64)
    return t


def dets(boxes, scores, labels):
    return {"boxes": np.array(boxes, dtype=F32).reshape(-1, 4), "scores": np.array(scores, dtype=F32), "labels": np.array(labels, dtype=np.int64)}


def stats_of(pairs, n_labels):
    recs = coco.merge_records([coco.match_reference(d, g, n_labels=n_labels) for d, g in pairs])
    return coco.summarize(coco.accumulate(recs, n_labels))


# ---- the rule, written twice ---------------------------------------------------------------------------------------------------------
def test_every_branch_of_the_walk_is_taken_and_both_writings_agree():
    counts = {}
    for det, gt in scenes(231, 8, 24, 12, 1):
        assert_records_equal(coco.match_reference(det, gt, counts, n_labels=1), coco.match_naive(det, gt, n_labels=1))
    print(counts)
    assert set(counts) == set(coco.BRANCHES)
    for branch in coco.BRANCHES:
        assert counts[branch] > 0, branch


def test_three_labels_and_labels_outside_the_range():
    for det, gt in scenes(232, 4, 24, 12, 3) + scenes(233, 2, 24, 12, 3, label_span=(-1, 5)):
        ref = coco.match_reference(det, gt, n_labels=3)
        assert_records_equal(ref, coco.match_naive(det, gt, n_labels=3))
        out = (det["labels"] < 0) | (det["labels"] >= 3)
        assert np.all(ref["label"][out] == -1) and np.all(ref["rank"][out] == -1) and not ref["match"][out].any() and not ref["ignore"][out].any()
        assert np.array_equal(ref["label"][~out], det["labels"][~out]) and np.all(ref["rank"][~out] >= 0)
    assert out.any() and (~out).any()


def test_ranks_from_100_on_exist_and_carry_zero_words():
    (det, gt), = scenes(234, 1, 130, 12, 1)
    ref = coco.match_reference(det, gt, n_labels=1)
    assert_records_equal(ref, coco.match_naive(det, gt, n_labels=1))
    assert sorted(ref["rank"].tolist()) == list(range(130))
    late = ref["rank"] >= 100
    assert late.sum() == 30 and not ref["match"][late].any() and not ref["ignore"][late].any()
    assert ref["match"][~late].any() and ref["ignore"][~late].any()
    order = np.argsort(ref["rank"])
    assert np.array_equal(order, np.argsort(-det["scores"], kind="mergesort"))


def test_the_device_count_form_is_the_slice():
    (det, gt), = scenes(235, 1, 24, 12, 2)
    part = {k: v[:10] for k, v in det.items()}
    assert_records_equal(coco.match_reference({**det, "count": np.array([10], dtype=np.int32)}, gt, n_labels=2),
                         coco.match_reference(part, gt, n_labels=2))


def test_iou_is_pycocotools_box_iou():
    d = np.array([[0, 0, 10, 10]], dtype=F32)
    g = np.array([[5, 0, 15, 10], [10, 0, 20, 10], [0, 0, 5, 10], [0, 0, 5, 10]], dtype=F32)
    got = coco.iou_reference(d, g, [False, False, False, True])
    assert got.tolist() == [[50 / 150, 0.0, 50 / 100, 50 / 100]]         # a touching box is 0; a crowd divides by the detection's area
    g2 = np.array([[0, 0, 5, 5]], dtype=F32)
    assert coco.iou_reference(d, g2, [False]).tolist() == [[0.25]] and coco.iou_reference(d, g2, [True]).tolist() == [[0.25]]
    assert coco.iou_reference(g2, d, [True]).tolist() == [[1.0]]


# ---- accumulate / summarize against closed forms ---------------------------------------------------------------------------------------
def test_one_ground_truth_with_an_identical_detection():
    want = 1.0 / (1.0 + EPS)
    for box, populated in (([0, 0, 16, 16], 3), ([0, 0, 40, 40], 4), ([0, 0, 100, 100], 5)):
        s = stats_of([(dets([box], [0.9], [0]), target([box], [0], 7))], 1)["stats"]
        for i in range(6):
            if i in (0, 1, 2, populated):
                assert abs(s[i] - want) <= TOL, (i, s[i])
            else:
                assert s[i] == -1.0
        assert [s[6], s[7], s[8], s[6 + populated]] == [1.0, 1.0, 1.0, 1.0] and sorted(s[9:].tolist())[:2] == [-1.0, -1.0]


def test_hit_miss_hit():
    gt = target([[0, 0, 40, 40], [60, 60, 100, 100]], [0, 0], 1)
    det = dets([[0, 0, 40, 40], [200, 200, 240, 240], [60, 60, 100, 100]], [0.9, 0.8, 0.7], [0, 0, 0])
    out = stats_of([(det, gt)], 1)
    s = out["stats"]
    want = (51 + 50 * (2 / 3)) / 101
    assert abs(s[1] - want) <= TOL and abs(s[0] - want) <= TOL and abs(s[2] - want) <= TOL         # IoU 1: every threshold alike
    assert s[6] == 0.5 and s[7] == 1.0 and s[8] == 1.0
    assert abs(out["mAP@0.5"] - 100 * want) <= 100 * TOL and out["mAP@[0.5:0.95]"] == 100.0 * s[0]


def test_labels_without_detections_or_without_ground_truth_and_empty_images():
    box = [0, 0, 40, 40]
    perfect = (dets([box], [0.9], [0]), target([box], [0], 1))
    base = stats_of([perfect], 3)["stats"]
    assert abs(base[0] - 1 / (1 + EPS)) <= TOL
    # label 1 has ground truth and no detection: precision 0 and recall 0, and it counts in the mean
    missed = (dets(np.zeros((0, 4)), [], []), target([box], [1], 2))
    recs = coco.merge_records([coco.match_reference(d, g, n_labels=3) for d, g in (perfect, missed)])
    acc = coco.accumulate(recs, 3)
    assert np.all(acc["precision"][:, :, 1, 0, :] == 0) and np.all(acc["recall"][:, 1, 0, :] == 0) and np.all(acc["precision"][:, :, 2] == -1)
    s = coco.summarize(acc)["stats"]
    assert abs(s[0] - 0.5 / (1 + EPS)) <= TOL and s[8] == 0.5
    # label 2 has detections and no ground truth: it stays at -1 and is left out of the mean
    stray = (dets([box], [0.95], [2]), target(np.zeros((0, 4)), [], 3))
    acc = coco.accumulate(coco.merge_records([coco.match_reference(d, g, n_labels=3) for d, g in (perfect, stray)]), 3)
    assert np.all(acc["precision"][:, :, 2] == -1) and np.all(acc["recall"][:, 2] == -1)
    assert np.array_equal(coco.summarize(acc)["stats"], base)
    # an image with neither changes nothing
    empty = (dets(np.zeros((0, 4)), [], []), target(np.zeros((0, 4)), [], 4))
    assert np.array_equal(stats_of([perfect, empty], 3)["stats"], base)
    none = coco.summarize(coco.accumulate(coco.merge_records([coco.match_reference(*empty, n_labels=3)]), 3))
    assert np.all(none["stats"] == -1)


# ---- record handling ---------------------------------------------------------------------------------------------------------------------
def test_shards_in_any_order_give_the_whole():
    recs = [coco.match_reference(d, g, n_labels=3) for d, g in scenes(236, 6, 24, 12, 3)]
    whole = coco.merge_records(recs)
    assert np.all(np.diff(whole["image"]) >= 0) and np.all(np.diff(whole["gt_image"]) >= 0)
    want = coco.accumulate(whole, 3)
    assert np.any(want["precision"] > 0)
    for split in ([[5, 2], [0], [4, 3, 1]], [[3], [2], [1], [0], [5], [4]], [[5, 4, 3, 2, 1, 0]]):
        shards = [coco.merge_records([recs[i] for i in part]) for part in split]
        assert_records_equal(coco.merge_records(shards), whole)
        got = coco.accumulate(coco.merge_records(shards), 3)
        assert np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"])
    # an image that two shards hold is taken from the first of them
    other = dict(recs[2], score=recs[2]["score"] * F32(0.5))
    assert_records_equal(coco.merge_records(recs + [other]), whole)
    assert not np.array_equal(coco.merge_records([other] + recs)["score"], whole["score"])


def test_the_image_id_order_decides_equal_scores():
    """two images of one label with one ground truth each; one holds a hit and one a miss, both with score 0.5.  The hit first:
    precision 1 up to recall 0.5, then nothing reaches recall 1: AP = 51 / 101.  The miss first: precision 1 / 2 up to recall 0.5."""
    box = [0, 0, 40, 40]
    def run(hit_id, miss_id):
        hit = (dets([box], [0.5], [0]), target([box], [0], hit_id))
        miss = (dets([[100, 100, 140, 140]], [0.5], [0]), target([box], [0], miss_id))
        return stats_of([miss, hit], 1)["stats"][1]
    assert abs(run(1, 2) - 51 / 101 / (1 + EPS)) <= TOL
    assert abs(run(2, 1) - 51 / 101 / 2) <= TOL


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_declared_bound_exported_and_built_behind_the_glue_wall():
    from edtr_amd import build, lib
    assert "edtr_coco_match" in lib.DECLARED_SYMBOLS
    assert "coco.hip" in build.GLUE_SOURCES and "glue.h" in [os.path.basename(d) for d in build.object_deps("coco.hip")]
    caps = (lib.COCO_MAX_DET, lib.COCO_MAX_GT, lib.COCO_MAX_LABELS, lib.COCO_MAX_THRESHOLDS, lib.COCO_KEEP)
    assert (coco.MAX_DET, coco.MAX_GT, coco.MAX_LABELS, len(coco.THRESHOLDS), coco.KEEP) == caps
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == lib.ABI_VERSION == 10 and hasattr(handle, "edtr_coco_match")


def test_the_entry_point_rejects_bad_arguments_before_any_launch():
    from edtr_amd import build, lib
    build.build_library()
    h = lib.load()
    p = 4096            # a non-NULL, aligned stand-in: every call below fails its checks before the pointer is used

    def call(**kw):
        a = dict(db=p, ds=p, dl=p, n=4, count=None, gb=p, gl=p, ga=p, gc=p, g=4, i64=1, n_labels=3, image=0, thr=p, n_thr=10, areas=p,
                 r0=p, r1=p, r2=p, r3=p, r4=p, r5=p, doff=p, cap=16, g0=p, g1=p, g2=p, goff=p, gcap=16)
        a.update(kw)
        return h.edtr_coco_match(*a.values(), None)
    assert call(db=None) == -1 and call(gc=None) == -1 and call(thr=None) == -1 and call(r4=None) == -1 and call(goff=None) == -1
    assert call(n=-1) == -2 and call(g=-1) == -2 and call(n_labels=0) == -2 and call(n_thr=0) == -2 and call(cap=0) == -2 and call(gcap=0) == -2
    assert call(n=1025) == -5 and call(g=1025) == -5 and call(n_labels=257) == -5 and call(n_thr=11) == -5
    assert call(i64=2) == -4
    assert call(db=p + 4) == -3 and call(gb=p + 8) == -3 and call(dl=p + 4) == -3 and call(r5=p + 4) == -3 and call(count=p + 2) == -3
    assert call(db=None, ds=None, dl=None, n=0, gb=None, gl=None, ga=None, gc=None, g=0) == 0      # an image with neither: nothing to launch
