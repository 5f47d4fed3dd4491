"""The detection-score launch on the device (csrc/coco.hip, include/edtr_hip.h "Detection scores") against its numpy restatement
(edtr_amd/coco.py), by EQUALITY: w and h are fp32 differences, everything after is correctly rounded fp64 in a stated order on both
sides, and no transcendental enters.  Inputs come from `coco.scene`, whose boxes lie on a grid of 8 so that IoUs are small rationals:
ties between ground truths, IoUs exactly at a threshold and equal scores are everywhere (tests/test_coco_cpu.py shows that every
branch of the walk is taken on them).  Shapes: none of one side, one of each, one short of, at and one past the 64 lanes of the
wave, more than 100 detections of one label (ranks from 100 on), and more detections than two passes of the compaction."""
import numpy as np
import pytest
import torch

from edtr_amd import coco

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
SHAPES = [(0, 5), (5, 0), (1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (300, 40)]
LABEL_SETS = {"one": (1, None), "three": (3, None), "outside": (3, (-1, 5))}       # n_labels, the span the labels are drawn from


def on_dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v for k, v in d.items()}


_CASES = {}


def case(d, g, labels, image_id=0):
    """(det, gt, the restatement's records): computed once per case, shared and left unchanged"""
    key = (d, g, labels, image_id)
    if key not in _CASES:
        n_labels, span = LABEL_SETS[labels]
        det, gt = coco.scene(np.random.default_rng([d, g, n_labels, image_id]), d, g, n_labels, image_id=image_id, label_span=span)
        _CASES[key] = (det, gt, coco.match_reference(det, gt, n_labels=n_labels))
    return _CASES[key]


def assert_records_equal(got, want):
    for name, dtype in coco.DET_FIELDS + coco.GT_FIELDS:
        assert got[name].dtype == np.dtype(dtype), name
        assert np.array_equal(got[name], want[name]), name


def concat(recs):
    return {name: np.concatenate([r[name] for r in recs]) for name, _ in coco.DET_FIELDS + coco.GT_FIELDS}


@pytest.mark.parametrize("labels", list(LABEL_SETS))
@pytest.mark.parametrize("d,g", SHAPES)
def test_records_equal_the_restatement_word_for_word(d, g, labels):
    det, gt, want = case(d, g, labels)
    rec = coco.Records(max(d, 1), LABEL_SETS[labels][0], DEV, gt_capacity=max(g, 1))
    rec.update(on_dev(det), on_dev(gt))
    got = rec.to_host()
    assert_records_equal(got, want)
    if (d, g, labels) == (130, 130, "one"):
        late = got["rank"] >= 100
        assert late.sum() == 30 and not got["match"][late].any() and not got["ignore"][late].any() and got["match"][~late].any()
    if labels == "outside" and d >= 63:
        assert (got["label"] == -1).any() and (got["label"] >= 0).any() and (got["gt_label"] == -1).any()
    if d >= 63 and g >= 40:
        assert got["match"].any() and got["ignore"].any() and (got["match"] & ~got["ignore"]).any()


def test_defaults_for_area_and_crowd_and_host_inputs():
    """no "area" and no "iscrowd" in the target: (x2 - x1) * (y2 - y1) in fp32 and no crowd; host arrays are uploaded"""
    det, gt, _ = case(65, 65, "three")
    bare = {k: gt[k] for k in ("boxes", "labels", "image_id")}
    rec = coco.Records(65, 3, DEV)
    rec.update(det, bare)
    assert_records_equal(rec.to_host(), coco.match_reference(det, bare, n_labels=3))


def test_the_device_count_form_equals_the_slice_and_never_reads_past_it():
    det, gt, _ = case(65, 65, "three")
    count = 37
    want = coco.match_reference({k: v[:count] for k, v in det.items()}, gt, n_labels=3)
    poisoned = {k: v.copy() for k, v in det.items()}
    poisoned["boxes"][count:] = np.nan
    poisoned["scores"][count:] = np.nan
    poisoned["labels"][count:] = 1
    assert_records_equal(coco.match_reference({**poisoned, "count": np.array([count], dtype=np.int32)}, gt, n_labels=3), want)
    rec = coco.Records(65, 3, DEV)
    rec.update({**on_dev(poisoned), "count": torch.tensor([count], dtype=torch.int32, device=DEV)}, on_dev(gt))
    got = rec.to_host()
    assert got["image"].shape[0] == count
    assert_records_equal(got, want)


def five():
    return [case(d, g, "three", image_id=7 * i + 3) for i, (d, g) in enumerate([(65, 20), (0, 5), (130, 70), (5, 0), (24, 12)])]


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_five_images_in_a_row_equal_five_restatement_calls_with_no_host_sync():
    cases = five()
    rec = coco.Records(sum(c[0]["scores"].shape[0] for c in cases), 3, DEV, gt_capacity=sum(c[1]["labels"].shape[0] for c in cases))
    resident = [(on_dev(det), on_dev(gt)) for det, gt, _ in cases]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")         # a synchronising call inside the loop raises
    try:
        for det, gt in resident:
            rec.update(det, gt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_records_equal(rec.to_host(), concat([c[2] for c in cases]))
    with pytest.raises(ValueError, match="recorded before"):
        rec.update(*resident[0])


def test_capacity_one_short_drops_the_last_rows_and_to_host_raises():
    cases = five()
    want = concat([c[2] for c in cases])
    total, gt_total = want["image"].shape[0], want["gt_image"].shape[0]
    rec = coco.Records(total - 1, 3, DEV, gt_capacity=gt_total - 1)
    for det, gt, _ in cases:
        rec.update(on_dev(det), on_dev(gt))
    assert rec.offsets.cpu().tolist() == [total, gt_total]                  # the offsets are the true totals
    for name, _ in coco.DET_FIELDS + coco.GT_FIELDS:
        rows = total - 1 if name in dict(coco.DET_FIELDS) else gt_total - 1
        col = rec.fields[name].cpu().numpy()
        assert col.shape[0] == rows + 1
        assert np.array_equal(col[:rows].view(want[name].dtype), want[name][:rows]), name
        assert np.all(col[rows:].view(np.uint8) == coco.Records.GUARD), name      # the guard row behind the arrays is untouched
    with pytest.raises(RuntimeError, match="larger capacity"):
        rec.to_host()


class Stub:
    """a detector that returns prepared detections on the device, as the dict itself or as the reference's ([dict], extra)"""
    def __init__(self, prepared, as_list):
        self.prepared, self.as_list, self.calls = prepared, as_list, 0

    def __call__(self, images):
        assert len(images) == 1 and images[0].is_cuda
        out = self.prepared[self.calls]
        self.calls += 1
        return ([out], None) if self.as_list else out


@pytest.mark.parametrize("as_list", [False, True])
def test_evaluate_end_to_end_equals_the_restatement(as_list):
    cases = [case(24, 12, "outside", image_id=100 - 9 * i) for i in range(8)]           # ids descending: the merge sorts them
    want_records = coco.merge_records([c[2] for c in cases])
    want = coco.summarize(coco.accumulate(want_records, 3))
    stub = Stub([on_dev(c[0]) for c in cases], as_list)
    images = [torch.zeros((3, 8, 8), device=DEV) for _ in cases]
    got = coco.evaluate(images, [c[1] for c in cases], stub, n_labels=3)
    assert stub.calls == 8
    assert got["stats"].dtype == np.float64 and np.array_equal(got["stats"], want["stats"]) and np.all(got["stats"][:3] > 0)
    assert got["mAP@[0.5:0.95]"] == want["mAP@[0.5:0.95]"] and got["mAP@0.5"] == want["mAP@0.5"] == 100.0 * got["stats"][1]
    assert got["precision"].shape == (10, 101, 3, 4, 3) and got["recall"].shape == (10, 3, 4, 3)
    assert_records_equal(coco.merge_records([got["records"]]), want_records)


def test_error_codes_come_back_without_a_launch():
    from edtr_amd import lib, ops
    h, s = lib.load(), ops.stream_ptr()
    det, gt, _ = case(65, 65, "three")
    rec = coco.Records(8, 3, DEV)
    d, g = on_dev(det), on_dev(gt)
    crowd, area = g["iscrowd"].to(torch.uint8), g["area"]
    f = rec.fields

    def call(**kw):
        a = dict(db=d["boxes"].data_ptr(), ds=d["scores"].data_ptr(), dl=d["labels"].data_ptr(), n=65, count=None, gb=g["boxes"].data_ptr(),
                 gl=g["labels"].data_ptr(), ga=area.data_ptr(), gc=crowd.data_ptr(), g=65, i64=1, n_labels=3, image=0,
                 thr=rec.thresholds.data_ptr(), n_thr=10, areas=rec.areas.data_ptr(), r0=f["image"].data_ptr(), r1=f["label"].data_ptr(),
                 r2=f["score"].data_ptr(), r3=f["rank"].data_ptr(), r4=f["match"].data_ptr(), r5=f["ignore"].data_ptr(),
                 doff=rec.det_offset.data_ptr(), cap=8, g0=f["gt_image"].data_ptr(), g1=f["gt_label"].data_ptr(), g2=f["gt_ignore"].data_ptr(),
                 goff=rec.gt_offset.data_ptr(), gcap=8)
        a.update(kw)
        return h.edtr_coco_match(*a.values(), s)
    assert call(ds=None) == -1 and call(r4=None) == -1
    assert call(n=1025) == -5 and call(g=1025) == -5 and call(n_labels=257) == -5
    assert call(db=d["boxes"].data_ptr() + 4) == -3
    torch.cuda.synchronize()
    assert rec.offsets.cpu().tolist() == [0, 0] and rec.to_host()["image"].shape[0] == 0          # nothing ran
    big = coco.scene(np.random.default_rng(0), 1025, 4, 3)
    with pytest.raises(ValueError, match="at most 1024"):
        rec.update(*big)
    with pytest.raises(ValueError, match="n_labels"):
        coco.Records(8, 257, DEV)
