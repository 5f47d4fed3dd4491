"""The host side of the device accumulate (edtr_amd/coco.py, csrc/coco_acc.hip): the ONE order that serves every (area range, maxDets,
threshold) and the single forward walk over it, shown to reproduce `accumulate` exactly; the score classes of `order_keys` against
numpy's own argsort; the summation order of `summarize_ordered_reference` against `summarize`; and the C ABI's checks, which refuse
bad arguments before any launch.  No GPU is needed."""
import os
import re

import numpy as np
import pytest

from edtr_amd import coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
SYMBOLS = ("edtr_coco_accumulate_workspace", "edtr_coco_order", "edtr_coco_accumulate", "edtr_coco_summarize")


def records_of(seed, ids, d, g, n_labels, **kw):
    rng = np.random.default_rng(seed)
    return coco.merge_records([coco.match_reference(*coco.scene(rng, d, g, n_labels, image_id=i, **kw), n_labels=n_labels) for i in ids])


def assert_acc_equal(got, want):
    assert np.array_equal(got["precision"], want["precision"]) and np.array_equal(got["recall"], want["recall"])


IDS = {"ascending": list(range(12)), "descending": list(range(40, 28, -1)), "shuffled": [5, 17, 2, 11, 29, 3, 23, 7, 13, 19, 31, 1],
       "negative": [-7, 4, -2 ** 31, 2 ** 31 - 1, 0, -1, 9, -300, 512, 511, -512, -513]}


@pytest.mark.parametrize("ids", list(IDS))
def test_walking_the_one_order_reproduces_accumulate_exactly(ids):
    rec = records_of(len(ids), IDS[ids], 40, 16, 3, label_span=(-1, 4))
    want = coco.accumulate(rec, 3)
    o = coco.accumulate_order_reference(rec, 3)
    assert o["order"].dtype == np.int32 and o["seg_start"].dtype == np.int32 and o["seg_start"].shape == (4,)
    assert o["seg_start"][0] == 0 and o["seg_start"][-1] == o["order"].shape[0]
    kept = (rec["label"] >= 0) & (rec["rank"] >= 0) & (rec["rank"] < coco.KEEP)
    assert sorted(o["order"].tolist()) == np.nonzero(kept)[0].tolist() and (~kept).any()
    assert_acc_equal(coco.accumulate_ordered_reference(rec, 3, o), want)
    assert (want["precision"] > 0).any() and (want["recall"] > 0).any()
    # the rows may arrive in any order: the key decides, not the arrival
    perm = np.random.default_rng(1).permutation(rec["image"].shape[0])
    moved = {**rec, **{name: rec[name][perm] for name, _ in coco.DET_FIELDS}}
    assert_acc_equal(coco.accumulate_ordered_reference(moved, 3), want)
    assert np.array_equal(perm[coco.accumulate_order_reference(moved, 3)["order"]], o["order"])


def test_more_than_a_hundred_detections_and_a_label_without_ground_truth():
    rng = np.random.default_rng(5)
    pairs = [coco.scene(rng, 130, 30, 1, image_id=i) for i in (3, 1)] + [coco.scene(rng, 20, 0, 2, image_id=2, label_span=(1, 2))]
    rec = coco.merge_records([coco.match_reference(d, g, n_labels=3) for d, g in pairs])
    want = coco.accumulate(rec, 3)
    assert_acc_equal(coco.accumulate_ordered_reference(rec, 3), want)
    assert (rec["rank"] >= coco.KEEP).sum() == 60 and np.all(want["precision"][:, :, 1:] == -1)
    assert not np.array_equal(want["recall"][..., 0], want["recall"][..., 2])


@pytest.mark.parametrize("npig", [1, 3, 7, 100, 101])
def test_the_bin_of_a_true_positive_comes_from_the_division_itself(npig):
    """every true-positive count 1 .. npig is reached, with false positives in between; at npig = 100 ceil(recThr npig) differs from
    the division for 14 thresholds"""
    n = 2 * npig
    rec = coco._empty_records()
    hit = np.arange(n) % 2 == 1
    rec.update(image=np.arange(n, dtype=np.int32) // 100, label=np.zeros(n, np.int32), score=(1.0 - np.arange(n) / (4.0 * n)).astype(F32),
               rank=(np.arange(n) % 100).astype(np.int32), match=np.where(hit, np.uint64(2 ** 40 - 1), np.uint64(0)), ignore=np.zeros(n, np.uint64),
               gt_image=np.zeros(npig, np.int32), gt_label=np.zeros(npig, np.int32), gt_ignore=np.full(npig, 0b1110, np.uint8))
    want = coco.accumulate(rec, 1)
    assert_acc_equal(coco.accumulate_ordered_reference(rec, 1), want)
    assert want["recall"][0, 0, 0, 2] == 1.0 and np.all(want["precision"][:, :, 0, 1:] == -1) and np.all(want["precision"][:, :, 0, 0, 2] > 0)
    need = np.array([next(c for c in range(npig + 1) if F64(c) / F64(npig) >= r) for r in coco.RECALL_THRESHOLDS])
    wrong = int(np.count_nonzero(need != np.ceil(coco.RECALL_THRESHOLDS * npig)))
    assert wrong == (14 if npig == 100 else 0)


def test_order_keys_are_numpys_stable_argsort_of_the_negated_fp64_score():
    x = np.array([np.nan, np.inf, 1, 0.0, -0.0, -1, -np.inf, np.nan], dtype=F32)
    keys = coco.order_keys(x)
    assert keys.dtype == np.uint32
    assert np.array_equal(np.argsort(keys, kind="stable"), np.argsort(-x.astype(F64), kind="mergesort"))
    assert keys[3] == keys[4] and keys[0] == keys[7] == keys.max() and keys[1] == keys.min() and keys[6] == np.sort(keys)[-3]
    rng = np.random.default_rng(0)
    many = np.concatenate([x, rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(F32), (rng.integers(-8, 9, 512) / 8).astype(F32),
                           np.array([1e-45, -1e-45, 3.4e38, -3.4e38], dtype=F32)])
    with np.errstate(invalid="ignore"):         # (a signalling NaN among the random bit patterns)
        assert np.array_equal(np.argsort(coco.order_keys(many), kind="stable"), np.argsort(-many.astype(F64), kind="mergesort"))
    # and in the records: equal scores fall through to image, then rank
    rec = coco._empty_records()
    rec.update(image=np.array([2, 1, 1, 0, 0, 0, 3, 3], np.int32), label=np.zeros(8, np.int32), score=x[[3, 4, 0, 7, 1, 6, 2, 5]],
               rank=np.array([0, 1, 0, 2, 0, 1, 0, 1], np.int32), match=np.zeros(8, np.uint64), ignore=np.zeros(8, np.uint64))
    assert coco.accumulate_order_reference(rec, 1)["order"].tolist() == [4, 6, 1, 0, 7, 5, 3, 2]


def test_the_ordered_summation_stays_within_1e_10_of_summarize():
    for seed, labels in ((1, 3), (2, 20)):
        acc = coco.accumulate(records_of(seed, range(10), 40, 16, labels), labels)
        got, want = coco.summarize_ordered_reference(acc), coco.summarize(acc)
        assert got["stats"].dtype == F64 and got["stats"].shape == (12,)
        assert np.max(np.abs(got["stats"] - want["stats"])) <= 1e-10 and np.all(want["stats"][:3] > 0)
        assert abs(got["mAP@[0.5:0.95]"] - want["mAP@[0.5:0.95]"]) <= 1e-8 and got["mAP@0.5"] == 100.0 * got["stats"][1]
    nothing = {"precision": -np.ones((10, 101, 2, 4, 3)), "recall": -np.ones((10, 2, 4, 3))}
    assert np.array_equal(coco.summarize_ordered_reference(nothing)["stats"], -np.ones(12))
    assert np.array_equal(coco.summarize(nothing)["stats"], -np.ones(12))
    # a worst case for the bound: 256 labels of entries spread over [0, 1]
    rng = np.random.default_rng(3)
    big = {"precision": rng.random((10, 101, 256, 4, 3)), "recall": rng.random((10, 256, 4, 3))}
    big["precision"][:, :, ::7] = -1.0
    big["recall"][:, ::7] = -1.0
    assert np.max(np.abs(coco.summarize_ordered_reference(big)["stats"] - coco.summarize(big)["stats"])) <= 1e-10


def test_from_host_refuses_rows_that_repeat_before_anything_reaches_a_device():
    rec = records_of(9, [0, 1], 10, 4, 2)
    twice = {name: np.concatenate([rec[name], rec[name]]) for name, _ in coco.DET_FIELDS + coco.GT_FIELDS}
    with pytest.raises(ValueError, match="repeat"):
        coco.Records.from_host(twice, 2, "cpu")


def test_evaluate_refuses_an_unknown_accumulate_before_anything_runs():
    with pytest.raises(ValueError, match='"host" or "device"'):
        coco.evaluate([None], [None], None, 1, accumulate="both")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_bound_exported_and_built_behind_the_glue_wall():
    from edtr_amd import build, lib
    assert all(s in lib.DECLARED_SYMBOLS for s in SYMBOLS)
    assert lib.ABI_VERSION == 10
    assert "coco_acc.hip" in build.GLUE_SOURCES and "coco_acc.hip" not in build.SOURCES
    assert "glue.h" in [os.path.basename(d) for d in build.object_deps("coco_acc.hip")]
    assert lib.COCO_ACC_TILE == coco.ACC_TILE
    assert lib.COCO_ACC_MAX_ROWS == coco.ACC_MAX_ROWS >= 2 ** 20
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == 10 and all(hasattr(handle, s) for s in SYMBOLS)
    assert [len(getattr(handle, s).argtypes) for s in SYMBOLS] == [2, 14, 18, 6]


def test_workspace_sizes_are_monotone_and_refuse_what_the_launches_refuse():
    from edtr_amd import build, lib
    build.build_library()
    ws = lib.load().edtr_coco_accumulate_workspace
    sizes = [ws(c, 80) for c in (1, 1023, 1024, 1025, 6400, 100000, 2 ** 20, coco.ACC_MAX_ROWS)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[1] == sizes[2] < sizes[3]
    assert sizes[0] == 2 * 16 * 1024 + 16 * 80 and sizes[-1] == 2 * 16 * coco.ACC_MAX_ROWS + 16 * 80
    assert ws(1024, 1) < ws(1024, 256)
    assert ws(0, 80) == 0 and ws(coco.ACC_MAX_ROWS + 1, 80) == 0 and ws(1024, 0) == 0 and ws(1024, 257) == 0


def test_the_entry_points_reject_bad_arguments_before_any_launch():
    from edtr_amd import build, lib
    build.build_library()
    h = lib.load()
    p, big = 4096, 1 << 40          # a non-NULL, aligned stand-in: every call below fails its checks before the pointer is used

    def order(**kw):
        a = dict(image=p, label=p, score=p, rank=p, off=p, cap=2000, n_labels=3, ws=p, ws_bytes=big, order=p, seg=p, kept=p, status=p)
        a.update(kw)
        return h.edtr_coco_order(*a.values(), None)
    assert order(image=None) == -1 and order(off=None) == -1 and order(ws=None) == -1 and order(order=None) == -1 and order(status=None) == -1
    assert order(cap=0) == -2 and order(n_labels=0) == -2 and order(ws_bytes=h.edtr_coco_accumulate_workspace(2000, 3) - 1) == -2
    assert order(cap=coco.ACC_MAX_ROWS + 1) == -5 and order(n_labels=257) == -5
    assert order(ws=p + 8) == -3 and order(rank=p + 2) == -3 and order(seg=p + 2) == -3 and order(score=p + 1) == -3

    def acc(**kw):
        a = dict(order=p, seg=p, match=p, ignore=p, rank=p, cap=2000, gl=p, gi=p, goff=p, gcap=50, n_labels=3, thr=p, ws=p, ws_bytes=big,
                 precision=p, recall=p, status=p)
        a.update(kw)
        return h.edtr_coco_accumulate(*a.values(), None)
    assert acc(order=None) == -1 and acc(gi=None) == -1 and acc(thr=None) == -1 and acc(recall=None) == -1 and acc(status=None) == -1
    assert acc(cap=0) == -2 and acc(gcap=0) == -2 and acc(n_labels=-1) == -2 and acc(ws_bytes=16) == -2
    assert acc(cap=coco.ACC_MAX_ROWS + 1) == -5 and acc(gcap=2 ** 30 + 1) == -5 and acc(n_labels=257) == -5
    assert acc(match=p + 4) == -3 and acc(precision=p + 4) == -3 and acc(ws=p + 4) == -3 and acc(goff=p + 1) == -3

    def summ(**kw):
        a = dict(precision=p, recall=p, n_labels=3, status=p, out=p)
        a.update(kw)
        return h.edtr_coco_summarize(*a.values(), None)
    assert summ(precision=None) == -1 and summ(status=None) == -1 and summ(out=None) == -1
    assert summ(n_labels=0) == -2 and summ(n_labels=257) == -5 and summ(out=p + 4) == -3 and summ(status=p + 2) == -3
