"""`Records.accumulate` / `stats` / `result` on the device (csrc/coco_acc.hip, include/edtr_hip.h "Detection scores") against the
host's `accumulate`, by EQUALITY on `order`, `seg_start`, `precision` and `recall`: the key is a strict total order, the counts are
integers and every fp64 operation is correctly rounded in a stated order on both sides.  `stats` equals
`summarize_ordered_reference` bit for bit and stays within 1e-10 of `summarize`.  Records are built on the host with
`match_reference` and uploaded with `Records.from_host`, unless a test says otherwise.  Shapes: around the 1024-row tile of the sort
(none, one, one short of, at, one past, several tiles and a remainder), with the capacity at the count and well above it."""
import numpy as np
import pytest
import torch

from edtr_amd import coco

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = np.float32, np.float64
TILE = coco.ACC_TILE
ALL = coco.DET_FIELDS + coco.GT_FIELDS


def on_dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v for k, v in d.items()}


def host_records(seed, ids, d, g, n_labels, **kw):
    rng = np.random.default_rng(seed)
    return coco.merge_records([coco.match_reference(*coco.scene(rng, d, g, n_labels, image_id=i, **kw), n_labels=n_labels) for i in ids])


def first_rows(rec, n):
    """the records with only their first n detection rows (every ground truth stays)"""
    return {name: rec[name][:n] if (name, dtype) in coco.DET_FIELDS else rec[name] for name, dtype in ALL}


def check(rec_dev, rec_host, n_labels):
    """accumulate on the device against the host on the same records; returns the host's result"""
    want, want_order = coco.accumulate(rec_host, n_labels), coco.accumulate_order_reference(rec_host, n_labels)
    got = rec_dev.accumulate()
    o = rec_dev.order_to_host()
    assert o["status"] == 0
    assert o["order"].dtype == np.int32 and np.array_equal(o["order"], want_order["order"])
    assert np.array_equal(o["seg_start"], want_order["seg_start"])
    assert got["precision"].shape == want["precision"].shape and got["recall"].shape == want["recall"].shape
    assert np.array_equal(got["precision"].cpu().numpy(), want["precision"])
    assert np.array_equal(got["recall"].cpu().numpy(), want["recall"])
    ordered = coco.summarize_ordered_reference(want)
    res = rec_dev.result()
    assert res["stats"].dtype == F64 and np.array_equal(res["stats"], ordered["stats"])
    assert np.max(np.abs(res["stats"] - coco.summarize(want)["stats"])) <= 1e-10
    assert res["mAP@[0.5:0.95]"] == ordered["mAP@[0.5:0.95]"] and res["mAP@0.5"] == ordered["mAP@0.5"]
    return want


def guards_intact(rec):
    raw = rec.buffer.cpu().numpy()
    for name, (at, rows, dt) in rec._layout.items():
        assert np.all(raw[at + (rows - 1) * dt.itemsize:at + rows * dt.itemsize] == coco.Records.GUARD), name
    raw = rec._acc["buffer"].cpu().numpy()
    for name, (at, nbytes, _) in rec._acc["layout"].items():
        assert np.all(raw[at + nbytes:(at + nbytes + 7) // 8 * 8 + 8] == coco.Records.GUARD), name


_BIG = {}


def big():
    """5 tiles and a row of one label, 100 detections an image, with ties everywhere: computed once, shared and left unchanged"""
    if not _BIG:
        _BIG["rec"] = host_records(11, range(52), 100, 6, 1)
        assert _BIG["rec"]["image"].shape[0] >= 5 * TILE + 1 and np.all(_BIG["rec"]["label"] == 0) and np.all(_BIG["rec"]["rank"] < coco.KEEP)
    return _BIG["rec"]


@pytest.mark.parametrize("spare", [0, 3 * TILE + 7])
@pytest.mark.parametrize("rows", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 5 * TILE + 1])
def test_the_sort_around_its_tile_with_the_capacity_at_and_above_the_count(rows, spare):
    """one label, so its segment straddles every tile boundary; a spare capacity leaves idle workgroups and merge passes that only copy"""
    host = first_rows(big(), rows)
    rec = coco.Records.from_host(host, 1, DEV, capacity=max(rows + spare, 1))
    want = check(rec, host, 1)
    if rows >= TILE - 1:
        assert (want["precision"] > 0).any() and (want["recall"][..., 0] < want["recall"][..., 2]).any()
    guards_intact(rec)


def test_the_order_of_a_million_rows_and_eighty_labels():
    """2^20 + 5 rows: 1025 tiles and eleven merge passes, the last of them with a partner of one tile; rows without a label and with
    labels past n_labels among them, scores in eighths so that most keys are decided by image and rank"""
    n = 2 ** 20 + 5
    rng = np.random.default_rng(7)
    host = coco._empty_records()
    host.update(image=(np.arange(n) // 128 - 4000).astype(np.int32), label=rng.integers(-1, 82, n).astype(np.int32), score=(rng.integers(0, 9, n) / 8).astype(F32),
                rank=(np.arange(n) % 128).astype(np.int32), match=np.zeros(n, np.uint64), ignore=np.zeros(n, np.uint64))
    perm = rng.permutation(n)
    host.update({name: host[name][perm] for name, _ in coco.DET_FIELDS})
    rec = coco.Records.from_host(host, 80, DEV)
    rec.accumulate()
    o, ref = rec.order_to_host(), coco.accumulate_order_reference(host, 80)
    assert o["status"] == 0 and 0 < ref["order"].shape[0] < n
    assert np.array_equal(o["order"], ref["order"]) and np.array_equal(o["seg_start"], ref["seg_start"])
    guards_intact(rec)


def test_equal_scores_across_images_recorded_in_descending_id_order():
    """`scene`'s scores are eighths, equal across images; the images are recorded live with descending ids, so the key and not the
    arrival order decides"""
    rng = np.random.default_rng(21)
    pairs = [coco.scene(rng, 60, 20, 3, image_id=i, label_span=(-1, 4)) for i in range(30, 18, -1)]
    rec = coco.Records(60 * len(pairs), 3, DEV, gt_capacity=20 * len(pairs))
    for det, gt in pairs:
        rec.update(on_dev(det), on_dev(gt))
    host = coco.merge_records([rec.to_host()])
    assert np.unique(host["score"]).size <= 8 and not np.array_equal(host["image"], rec.to_host()["image"])
    got = rec.accumulate()
    want = coco.accumulate(host, 3)
    assert np.array_equal(got["precision"].cpu().numpy(), want["precision"]) and np.array_equal(got["recall"].cpu().numpy(), want["recall"])
    live = rec.to_host()
    o = rec.order_to_host()
    ref = coco.accumulate_order_reference(live, 3)
    assert np.array_equal(o["order"], ref["order"]) and np.array_equal(o["seg_start"], ref["seg_start"])
    assert (live["label"] == -1).any()
    guards_intact(rec)


def test_nan_zero_and_infinite_scores_take_numpys_places():
    x = np.array([np.nan, np.inf, 1, 0.0, -0.0, -1, -np.inf, np.nan], dtype=F32)
    host = coco._empty_records()
    host.update(image=np.array([2, 1, 1, 0, 0, 0, 3, 3], np.int32), label=np.zeros(8, np.int32), score=x[[3, 4, 0, 7, 1, 6, 2, 5]],
                rank=np.array([0, 1, 0, 2, 0, 1, 0, 1], np.int32), match=np.array([1, 0, 1, 1, 0, 1, 1, 0], np.uint64) * np.uint64(2 ** 40 - 1),
                ignore=np.array([0, 0, 0, 1, 0, 0, 0, 0], np.uint64) * np.uint64(2 ** 40 - 1), gt_image=np.zeros(5, np.int32), gt_label=np.zeros(5, np.int32),
                gt_ignore=np.array([0, 0, 2, 4, 8], np.uint8))
    rec = coco.Records.from_host(host, 1, DEV)
    check(rec, host, 1)
    assert rec.order_to_host()["order"].tolist() == [4, 6, 1, 0, 7, 5, 3, 2]


def test_rows_without_a_label_and_ranks_past_a_hundred_are_left_out():
    rng = np.random.default_rng(31)
    pairs = [coco.scene(rng, 130, 30, 1, image_id=9), coco.scene(rng, 80, 20, 3, image_id=4, label_span=(-1, 4)), coco.scene(rng, 130, 30, 1, image_id=2)]
    host = coco.merge_records([coco.match_reference(d, g, n_labels=3) for d, g in pairs])
    assert (host["rank"] >= coco.KEEP).sum() == 60 and (host["label"] == -1).any()
    want = check(coco.Records.from_host(host, 3, DEV), host, 3)
    r = want["recall"][:, 0, 0]
    assert (r[:, 0] < r[:, 1]).any() and (r[:, 1] < r[:, 2]).any()          # the three maxDets differ


def test_labels_with_only_ground_truth_only_detections_or_neither_and_empty_records():
    rng = np.random.default_rng(41)
    pairs = [coco.scene(rng, 40, 16, 2, image_id=i) for i in range(4)]
    for det, gt in pairs:
        gt["labels"] = np.where(gt["labels"] == 1, 2, 0)            # label 1: detections only; label 2: ground truth only; label 3: neither
    host = coco.merge_records([coco.match_reference(d, g, n_labels=4) for d, g in pairs])
    want = check(coco.Records.from_host(host, 4, DEV), host, 4)
    assert np.all(want["precision"][:, :, 1] == -1) and np.all(want["recall"][:, 3] == -1)
    assert np.all(want["precision"][:, :, 2, 0] == 0) and np.all(want["recall"][:, 2, 0] == 0) and (want["precision"][:, :, 0] > 0).any()
    empty = coco._empty_records()
    rec = coco.Records.from_host(empty, 2, DEV)
    want = check(rec, empty, 2)
    assert np.all(want["precision"] == -1) and np.array_equal(rec.result()["stats"], -np.ones(12))


@pytest.mark.parametrize("npig", [1, 3, 7, 100, 101])
def test_every_true_positive_count_up_to_npig_with_false_positives_between(npig):
    n = 2 * npig
    host = coco._empty_records()
    hit = np.arange(n) % 2 == 1
    host.update(image=np.arange(n, dtype=np.int32) // 100, label=np.zeros(n, np.int32), score=(1.0 - np.arange(n) / (4.0 * n)).astype(F32),
                rank=(np.arange(n) % 100).astype(np.int32), match=np.where(hit, np.uint64(2 ** 40 - 1), np.uint64(0)), ignore=np.zeros(n, np.uint64),
                gt_image=np.zeros(npig, np.int32), gt_label=np.zeros(npig, np.int32), gt_ignore=np.full(npig, 0b1110, np.uint8))
    want = check(coco.Records.from_host(host, 1, DEV), host, 1)
    assert want["recall"][0, 0, 0, 2] == 1.0 and np.all(want["precision"][:, :, 0, 1:] == -1)


def five():
    sizes = [(65, 20), (0, 5), (130, 70), (5, 0), (24, 12)]
    return [coco.scene(np.random.default_rng([d, g, 3, 7 * i + 3]), d, g, 3, image_id=7 * i + 3) for i, (d, g) in enumerate(sizes)]


def test_a_capacity_one_short_sets_the_status_and_result_raises():
    pairs = five()
    total, gt_total = sum(p[0]["scores"].shape[0] for p in pairs), sum(p[1]["labels"].shape[0] for p in pairs)
    rec = coco.Records(total - 1, 3, DEV, gt_capacity=gt_total)
    for det, gt in pairs:
        rec.update(on_dev(det), on_dev(gt))
    rec.accumulate()
    o = rec.order_to_host()
    assert o["status"] & 1 and rec.offsets.cpu().tolist() == [total, gt_total]
    # rows past the capacity do not exist: the order is that of the rows that fitted
    fitted = first_rows({name: np.concatenate([coco.match_reference(d, g, n_labels=3)[name] for d, g in pairs]) for name, _ in ALL}, total - 1)
    ref = coco.accumulate_order_reference(fitted, 3)
    assert np.array_equal(o["order"], ref["order"]) and np.array_equal(o["seg_start"], ref["seg_start"])
    with pytest.raises(RuntimeError, match="larger capacity"):
        rec.result()
    guards_intact(rec)
    short_gt = coco.Records(total, 3, DEV, gt_capacity=gt_total - 1)
    for det, gt in pairs:
        short_gt.update(on_dev(det), on_dev(gt))
    with pytest.raises(RuntimeError, match="larger capacity"):
        short_gt.result()
    guards_intact(short_gt)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_live_records_accumulate_and_stats_with_no_host_sync():
    pairs = five()
    rec = coco.Records(sum(p[0]["scores"].shape[0] for p in pairs), 3, DEV, gt_capacity=sum(p[1]["labels"].shape[0] for p in pairs))
    resident = [(on_dev(det), on_dev(gt)) for det, gt in pairs]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")         # a synchronising call raises
    try:
        for det, gt in resident:
            rec.update(det, gt)
        acc = rec.accumulate()
        stats = rec.stats()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert stats.is_cuda and stats.dtype == torch.float64 and stats.shape == (12,)
    host = coco.merge_records([rec.to_host()])
    want = coco.accumulate(host, 3)
    assert np.array_equal(acc["precision"].cpu().numpy(), want["precision"]) and np.array_equal(acc["recall"].cpu().numpy(), want["recall"])
    assert np.array_equal(stats.cpu().numpy(), coco.summarize_ordered_reference(want)["stats"])
    assert np.max(np.abs(stats.cpu().numpy() - coco.summarize(want)["stats"])) <= 1e-10
    assert np.array_equal(rec.result()["stats"], stats.cpu().numpy()) and np.all(rec.result()["stats"][:3] > 0)


class Stub:
    """a detector that returns prepared detections on the device"""
    def __init__(self, prepared):
        self.prepared, self.calls = prepared, 0

    def __call__(self, images):
        self.calls += 1
        return self.prepared[self.calls - 1]


def test_evaluate_on_the_device_equals_evaluate_on_the_host():
    rng = np.random.default_rng(51)
    pairs = [coco.scene(rng, 24, 12, 3, image_id=100 - 9 * i, label_span=(-1, 5)) for i in range(8)]           # ids descending
    images = [torch.zeros((3, 8, 8), device=DEV) for _ in pairs]
    prepared, targets = [on_dev(p[0]) for p in pairs], [p[1] for p in pairs]
    host = coco.evaluate(images, targets, Stub(prepared), n_labels=3)
    dev = coco.evaluate(images, targets, Stub(prepared), n_labels=3, accumulate="device")
    assert set(dev) == set(host) - {"records"}
    assert isinstance(dev["precision"], np.ndarray) and np.array_equal(dev["precision"], host["precision"]) and np.array_equal(dev["recall"], host["recall"])
    assert dev["stats"].dtype == F64 and np.max(np.abs(dev["stats"] - host["stats"])) <= 1e-10 and np.all(dev["stats"][:3] > 0)
    assert np.array_equal(dev["stats"], coco.summarize_ordered_reference(host)["stats"])
    assert abs(dev["mAP@[0.5:0.95]"] - host["mAP@[0.5:0.95]"]) <= 1e-8 and dev["mAP@0.5"] == 100.0 * dev["stats"][1]
    asked = coco.evaluate(images, targets, Stub(prepared), n_labels=3, accumulate="device", return_records=True)
    for name, _ in ALL:
        assert np.array_equal(asked["records"][name], host["records"][name]), name


def test_error_codes_come_back_without_a_launch_and_too_many_rows_are_refused():
    from edtr_amd import lib, ops
    h, s = lib.load(), ops.stream_ptr()
    rec = coco.Records(8, 3, DEV)
    st = rec._acc_state()
    before = st["buffer"].clone()
    f, ws = rec.fields, st["workspace"]

    def order(**kw):
        a = dict(image=f["image"].data_ptr(), label=f["label"].data_ptr(), score=f["score"].data_ptr(), rank=f["rank"].data_ptr(),
                 off=rec.det_offset.data_ptr(), cap=8, n_labels=3, ws=ws.data_ptr(), ws_bytes=ws.numel(), order=st["order"].data_ptr(),
                 seg=st["seg_start"].data_ptr(), kept=st["n_kept"].data_ptr(), status=st["status"].data_ptr())
        a.update(kw)
        return h.edtr_coco_order(*a.values(), s)
    assert order(rank=None) == -1 and order(cap=0) == -2 and order(ws_bytes=ws.numel() - 1) == -2 and order(cap=coco.ACC_MAX_ROWS + 1) == -5
    assert order(ws=ws.data_ptr() + 8) == -3
    torch.cuda.synchronize()
    assert torch.equal(st["buffer"], before)                    # nothing ran
    with pytest.raises(ValueError, match="orders at most"):
        coco.Records(coco.ACC_MAX_ROWS + 1, 3, DEV, gt_capacity=8).accumulate()
