"""Detection scores: what the reference's detection test ends in.  `main/det/test_edtr.py:138-190` hands every image's detections
to `CocoEvaluator.update` (utils/detection.py:422-480) and reports `mAP@[0.5:0.95]` and `mAP@0.5`.  Here the per-image half of that —
pycocotools' `COCOeval.evaluateImg` for every label, IoU threshold and area range — is one launch per image that appends to a running
record on the device (include/edtr_hip.h "Detection scores", csrc/coco.hip), and `accumulate` / `summarize` run on the host from ONE
copy at the end — or on the device as well (`Records.accumulate` / `stats` / `result`, csrc/coco_acc.hip), from which 104 bytes are
copied.  The detector stays outside: `evaluate` takes any callable, as `labels.evaluate` takes any `segnet`.

pycocotools is not a dependency of this project, so — as with NMS in `boxes` — everything is pinned to the RULE written out below, which
is `COCOeval.evaluateImg`, `accumulate`, `_summarizeDets` and `maskUtils.iou` for boxes.  `match_reference` is the normative numpy
restatement (the launch is tested against it by equality: no transcendental enters), `match_naive` an independent second writing as a
plain per-pair scalar loop.

THE RULE.  Per image: detections `boxes` fp32 [d, 4] xyxy, `scores` fp32 [d], `labels` [d]; ground truth `boxes` fp32 [g, 4] xyxy,
`labels`, `area` fp32 [g] (as the data set hands it over; default (x2 - x1) * (y2 - y1) in fp32), `iscrowd` [g].
  * constants: thresholds T = linspace(0.5, 0.95, 10) in fp64; area ranges A = [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10];
    maxDets = (1, 10, 100); recall thresholds linspace(0, 1, 101).
  * coordinates: w = x2 - x1 and h = y2 - y1 in fp32 (`convert_to_xywh`, `convert_to_coco_api`); everything after is fp64, each
    operation rounded, none contracted.  A detection's area is w * h.
  * IoU: iw = min(dx + dw, gx + gw) - max(dx, gx), ih alike; 0 if iw <= 0 or ih <= 0; otherwise i = iw * ih, u = da for a crowd
    ground truth and (da + ga) - i for any other (ga = gw * gh), iou = i / u.
  * per label in [0, n_labels): rank the detections by `boxes.score_keys` descending, ties by index (argsort(-score, "mergesort"));
    ranks 0 .. 99 are matched.
  * per area range [lo, hi]: a ground truth is ignored iff it is a crowd or its area lies outside [lo, hi]; the ground truths are
    walked not-ignored first, then ignored, each group in input order.
  * per threshold t, walk the kept detections in rank order with best = min(t, 1 - 1e-10) and m = none; for each ground truth in
    order: skip it if it is matched at this t and no crowd; stop if m is a not-ignored ground truth and this one is ignored; skip it if
    iou < best; otherwise best = iou, m = this one (an equal IoU moves m on).  A matched detection takes the ignore flag of m and marks
    m matched; an unmatched one is ignored iff its own area lies outside [lo, hi].
RECORDS.  One row per detection in input order: `image`, `label` (-1 outside [0, n_labels)), `score`, `rank` within (image, label)
(-1 for label -1), and two uint64 words `match` and `ignore` with bit 4 t + a for threshold t and area range a; both words are zero
for rank >= 100 and for label -1.  One row per ground truth in input order: `gt_image`, `gt_label` (or -1), `gt_ignore` with bit a.
`accumulate` and `summarize` are written out in their docstrings."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import boxes as _boxes

F32, F64 = np.float32, np.float64
THRESHOLDS = np.linspace(0.5, 0.95, 10)
AREA_RANGES = np.array([[0.0, 1e10], [0.0, 32.0 ** 2], [32.0 ** 2, 96.0 ** 2], [96.0 ** 2, 1e10]], dtype=F64)
MAX_DETS = (1, 10, 100)
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
KEEP = 100                                  # EDTR_COCO_KEEP: the largest maxDets
MAX_DET, MAX_GT, MAX_LABELS = 1024, 1024, 256     # EDTR_COCO_MAX_*: one image's detections and ground truths, the label values
BRANCHES = ("skip_matched", "break", "tie", "eq_thr", "match_ignored", "crowd_again", "unmatched_out")
DET_FIELDS = (("image", np.int32), ("label", np.int32), ("score", F32), ("rank", np.int32), ("match", np.uint64), ("ignore", np.uint64))
GT_FIELDS = (("gt_image", np.int32), ("gt_label", np.int32), ("gt_ignore", np.uint8))
ACC_TILE, ACC_MAX_ROWS = 1024, 1 << 22      # EDTR_COCO_ACC_*: the sort tile of `Records.accumulate` and the most rows it orders
assert THRESHOLDS[0] == 0.5 and THRESHOLDS[5] == 0.75       # the device's summarize takes AP50 and AP75 at these two indices


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative)
# ----------------------------------------------------------------------------------------------------------------------------------
def _host(v, dtype) -> np.ndarray:
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v).astype(dtype)


def _image_id(target) -> int:
    v = target["image_id"]
    if hasattr(v, "is_cuda") and v.is_cuda:
        raise TypeError("image_id must be an int or a host tensor: reading it from the device would be a host sync per image")
    return int(np.asarray(v).reshape(-1)[0])


def _inputs(det: dict, gt: dict, n_labels: Optional[int]):
    """one image's arrays on the host in the rule's types; rows at or past det["count"] do not exist"""
    db = _host(det["boxes"], F32).reshape(-1, 4)
    ds, dl = _host(det["scores"], F32).reshape(-1), _host(det["labels"], np.int64).reshape(-1)
    if ds.shape[0] != db.shape[0] or dl.shape[0] != db.shape[0]:
        raise ValueError("detections take one score and one label per box")
    if det.get("count") is not None:
        c = min(max(int(_host(det["count"], np.int64).reshape(-1)[0]), 0), db.shape[0])
        db, ds, dl = db[:c], ds[:c], dl[:c]
    gb = _host(gt["boxes"], F32).reshape(-1, 4)
    gl = _host(gt["labels"], np.int64).reshape(-1)
    area = _host(gt["area"], F32).reshape(-1) if gt.get("area") is not None else (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
    crowd = _host(gt["iscrowd"], np.int64).reshape(-1) != 0 if gt.get("iscrowd") is not None else np.zeros(gb.shape[0], dtype=bool)
    if not (gl.shape[0] == area.shape[0] == crowd.shape[0] == gb.shape[0]):
        raise ValueError("ground truth takes one label, one area and one crowd flag per box")
    if db.shape[0] > MAX_DET or gb.shape[0] > MAX_GT:
        raise ValueError(f"an image takes at most {MAX_DET} detections and {MAX_GT} ground truths, got {db.shape[0]} and {gb.shape[0]}")
    if n_labels is None:
        n_labels = int(max(dl.max(initial=-1), gl.max(initial=-1))) + 1
    return db, ds, dl, gb, gl, area.astype(F32), crowd, int(n_labels), _image_id(gt)


def iou_reference(det_boxes, gt_boxes, crowd) -> np.ndarray:
    """fp64 [d, g]: `maskUtils.iou` for boxes by the rule above — w and h in fp32, the rest in fp64, each step rounded, with
    min(a, b) = a if a < b else b and max alike"""
    d = np.asarray(det_boxes, dtype=F32).reshape(-1, 4)
    g = np.asarray(gt_boxes, dtype=F32).reshape(-1, 4)
    dx, dy, dw, dh = (v.astype(F64)[:, None] for v in (d[:, 0], d[:, 1], d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]))
    gx, gy, gw, gh = (v.astype(F64)[None, :] for v in (g[:, 0], g[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]))
    da, ga = dw * dh, gw * gh
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dr, gr = dx + dw, gx + gw
        iw = np.where(dr < gr, dr, gr) - np.where(dx > gx, dx, gx)
        db, gb = dy + dh, gy + gh
        ih = np.where(db < gb, db, gb) - np.where(dy > gy, dy, gy)
        inter = iw * ih
        union = np.where(np.asarray(crowd, dtype=bool)[None, :], np.broadcast_to(da, inter.shape), (da + ga) - inter)
        return np.where((iw > 0) & (ih > 0), inter / union, 0.0)


def _empty_records() -> dict:
    return {k: np.zeros(0, dtype=t) for k, t in DET_FIELDS + GT_FIELDS}


def _gt_records(gl, area, crowd, n_labels, image_id) -> dict:
    ar = area.astype(F64)
    bits = np.zeros(gl.shape[0], dtype=np.uint8)
    for a, (lo, hi) in enumerate(AREA_RANGES):
        bits |= ((crowd | (ar < lo) | (ar > hi)).astype(np.uint8) << np.uint8(a)).astype(np.uint8)
    known = (gl >= 0) & (gl < n_labels)
    return {"gt_image": np.full(gl.shape[0], image_id, dtype=np.int32), "gt_label": np.where(known, gl, -1).astype(np.int32), "gt_ignore": bits}


def match_reference(det: dict, gt: dict, counts: Optional[dict] = None, n_labels: Optional[int] = None) -> dict:
    """One image's records by THE RULE of this module's docstring (normative).  ``det``: {"boxes", "scores", "labels"} and optionally
    "count" (rows at or past it do not exist); ``gt``: {"boxes", "labels", "image_id"} and optionally "area", "iscrowd"; numpy arrays or
    tensors.  ``n_labels``: labels outside [0, n_labels) are recorded as -1 with zero words (None: one more than the largest label).
    With ``counts`` a dict, the seven branches of the walk are tallied into it (`BRANCHES`):
      skip_matched   a ground truth passed over because it is matched at this threshold and no crowd
      break          the walk stopped at the first ignored ground truth after a not-ignored match
      tie            a later ground truth with an IoU EQUAL to the best so far took the match
      eq_thr         a ground truth was accepted with an IoU exactly equal to the threshold
      match_ignored  a detection matched an ignored ground truth
      crowd_again    a crowd that was already matched at this threshold was matched once more
      unmatched_out  an unmatched detection whose own area lies outside the range
    Returns a dict of arrays, `DET_FIELDS` and `GT_FIELDS`."""
    db, ds, dl, gb, gl, area, crowd, n_labels, image_id = _inputs(det, gt, n_labels)
    if counts is not None:
        for b in BRANCHES:
            counts.setdefault(b, 0)
    tally = counts if counts is not None else dict.fromkeys(BRANCHES, 0)
    d = db.shape[0]
    rec = _gt_records(gl, area, crowd, n_labels, image_id)
    known = (dl >= 0) & (dl < n_labels)
    rank = np.full(d, -1, dtype=np.int32)
    match, ignore = [0] * d, [0] * d
    keys = _boxes.score_keys(ds).astype(np.int64)
    d_area = (db[:, 2] - db[:, 0]).astype(F64) * (db[:, 3] - db[:, 1]).astype(F64)
    for k in np.unique(dl[known]).tolist():
        di = np.nonzero(dl == k)[0]
        order = di[np.argsort(-keys[di], kind="stable")]
        rank[order] = np.arange(order.size, dtype=np.int32)
        kept = order[:KEEP]
        gi = np.nonzero(gl == k)[0]
        ious = iou_reference(db[kept], gb[gi], crowd[gi])
        for a, (lo, hi) in enumerate(AREA_RANGES):
            g_ign = (rec["gt_ignore"][gi] >> a) & 1
            walk = np.argsort(g_ign, kind="stable")
            ign, crd = g_ign[walk].astype(bool).tolist(), crowd[gi][walk].tolist()
            rows = ious[:, walk].tolist()
            outside = ((d_area[kept] < lo) | (d_area[kept] > hi)).tolist()
            for t, thr in enumerate(THRESHOLDS.tolist()):
                bit = 1 << (4 * t + a)
                taken = [False] * len(ign)
                for r, i in enumerate(kept.tolist()):
                    row, best, m = rows[r], min(thr, 1 - 1e-10), -1
                    for s in range(len(ign)):
                        if taken[s] and not crd[s]:
                            tally["skip_matched"] += 1
                            continue
                        if m > -1 and not ign[m] and ign[s]:
                            tally["break"] += 1
                            break
                        if row[s] < best:
                            continue
                        tally["tie"] += m > -1 and row[s] == best
                        tally["eq_thr"] += row[s] == thr
                        best, m = row[s], s
                    if m == -1:
                        if outside[r]:
                            tally["unmatched_out"] += 1
                            ignore[i] |= bit
                        continue
                    tally["crowd_again"] += taken[m]
                    taken[m] = True
                    match[i] |= bit
                    if ign[m]:
                        tally["match_ignored"] += 1
                        ignore[i] |= bit
    rec.update(image=np.full(d, image_id, dtype=np.int32), label=np.where(known, dl, -1).astype(np.int32), score=ds, rank=rank,
               match=np.array(match, dtype=np.uint64).reshape(d), ignore=np.array(ignore, dtype=np.uint64).reshape(d))
    return rec


def match_naive(det: dict, gt: dict, n_labels: Optional[int] = None) -> dict:
    """The same records by a plain per-pair scalar loop in the order pycocotools runs (thresholds outermost, one IoU evaluated per
    pair where it is needed, python floats for fp64 and numpy scalars for the fp32 differences): the independent second writing
    `match_reference` is checked against, as tools/make_boxes_goldens.py does for NMS."""
    db, ds, dl, gb, gl, area, crowd, n_labels, image_id = _inputs(det, gt, n_labels)
    keys = [int(v) for v in _boxes.score_keys(ds)]

    def xywh(b):
        return float(b[0]), float(b[1]), float(F32(b[2]) - F32(b[0])), float(F32(b[3]) - F32(b[1]))

    def iou(i, j):
        (dx, dy, dw, dh), (gx, gy, gw, gh) = xywh(db[i]), xywh(gb[j])
        iw = min(dx + dw, gx + gw) - max(dx, gx)
        ih = min(dy + dh, gy + gh) - max(dy, gy)
        if iw <= 0 or ih <= 0:
            return 0.0
        inter = iw * ih
        return inter / (dw * dh if crowd[j] else (dw * dh + gw * gh) - inter)

    d, g = db.shape[0], gb.shape[0]
    out = {"image": [image_id] * d, "label": [-1] * d, "score": ds, "rank": [-1] * d, "match": [0] * d, "ignore": [0] * d,
           "gt_image": [image_id] * g, "gt_label": [-1] * g, "gt_ignore": [0] * g}
    for j in range(g):
        if 0 <= gl[j] < n_labels:
            out["gt_label"][j] = int(gl[j])
        for a, (lo, hi) in enumerate(AREA_RANGES.tolist()):
            if crowd[j] or float(area[j]) < lo or float(area[j]) > hi:
                out["gt_ignore"][j] |= 1 << a
    for k in range(n_labels):
        dets = sorted((i for i in range(d) if dl[i] == k), key=lambda i: (-keys[i], i))
        for r, i in enumerate(dets):
            out["label"][i], out["rank"][i] = k, r
        dets = dets[:KEEP]
        for a, (lo, hi) in enumerate(AREA_RANGES.tolist()):
            mine = [j for j in range(g) if gl[j] == k]
            gts = [j for j in mine if not out["gt_ignore"][j] >> a & 1] + [j for j in mine if out["gt_ignore"][j] >> a & 1]
            for t, thr in enumerate(THRESHOLDS.tolist()):
                matched = set()
                for i in dets:
                    best, m = min(thr, 1 - 1e-10), None
                    for j in gts:
                        j_ignored = bool(out["gt_ignore"][j] >> a & 1)
                        if j in matched and not crowd[j]:
                            continue
                        if m is not None and not (out["gt_ignore"][m] >> a & 1) and j_ignored:
                            break
                        v = iou(i, j)
                        if v < best:
                            continue
                        best, m = v, j
                    if m is None:
                        dx, dy, dw, dh = xywh(db[i])
                        if dw * dh < lo or dw * dh > hi:
                            out["ignore"][i] |= 1 << (4 * t + a)
                        continue
                    matched.add(m)
                    out["match"][i] |= 1 << (4 * t + a)
                    if out["gt_ignore"][m] >> a & 1:
                        out["ignore"][i] |= 1 << (4 * t + a)
    return {name: np.array(out[name], dtype=dtype).reshape(-1) for name, dtype in DET_FIELDS + GT_FIELDS}


def merge_records(shards: Sequence[dict]) -> dict:
    """`CocoEvaluator.synchronize_between_processes`: the shards' records concatenated, unique by image id (an image that several shards
    hold is taken from the first of them), sorted by image id; rows of one image keep their order.  Within a shard an image id occurs
    once (`Records.update` refuses a second one)."""
    seen: set = set()
    parts = []
    for shard in shards:
        ids = set(np.unique(shard["image"]).tolist()) | set(np.unique(shard["gt_image"]).tolist())
        fresh = np.array(sorted(ids - seen), dtype=np.int64)
        seen |= ids
        dk, gk = np.isin(shard["image"], fresh), np.isin(shard["gt_image"], fresh)
        parts.append({name: np.asarray(shard[name])[dk if (name, dtype) in DET_FIELDS else gk] for name, dtype in DET_FIELDS + GT_FIELDS})
    if not parts:
        return _empty_records()
    out = {name: np.concatenate([p[name] for p in parts]).astype(dtype) for name, dtype in DET_FIELDS + GT_FIELDS}
    do, go = np.argsort(out["image"], kind="stable"), np.argsort(out["gt_image"], kind="stable")
    return {name: out[name][do if (name, dtype) in DET_FIELDS else go] for name, dtype in DET_FIELDS + GT_FIELDS}


def accumulate(records: dict, n_labels: int) -> dict:
    """`COCOeval.accumulate` from the records of a whole data set (each image once: `merge_records`).
    {"precision": fp64 [T, R, K, A, M], "recall": fp64 [T, K, A, M]} with T = 10 thresholds, R = 101 recall thresholds, K =
    ``n_labels``, A = 4 area ranges, M = 3 maxDets; both start at -1.  For each label k, area range a and M in maxDets:
      * the images in ascending id, in each the detections of label k with rank < M in rank order; all of them sorted stably by
        score descending — so equal scores stay in image order, then in rank order;
      * tp = match & ~ignore and fp = ~match & ~ignore per threshold, cumulated along that order;
      * npig = the ground truths of label k not ignored in range a; 0 leaves the -1 (a label without ground truth anywhere falls out of
        every mean, as pycocotools' catIds drops it);
      * rc = tp / npig, pr = tp / (fp + tp + spacing(1)); recall[t, k, a, m] = rc[-1], or 0 without detections;
      * pr is made non-increasing from the right, and precision[t, r, k, a, m] = pr[searchsorted(rc, recThr[r], "left")], 0 past the end."""
    K = int(n_labels)
    T, R, A, M = len(THRESHOLDS), len(RECALL_THRESHOLDS), len(AREA_RANGES), len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    label, rank = np.asarray(records["label"]), np.asarray(records["rank"])
    by_image = np.lexsort((rank, np.asarray(records["image"])))              # image ascending, then rank
    bits = np.arange(T, dtype=np.uint64) * np.uint64(4)
    for k in range(K):
        g_ign = np.asarray(records["gt_ignore"])[np.asarray(records["gt_label"]) == k]
        rows = by_image[(label[by_image] == k) & (rank[by_image] >= 0) & (rank[by_image] < KEEP)]
        if g_ign.size == 0 and rows.size == 0:
            continue
        for a in range(A):
            npig = int(np.count_nonzero((g_ign >> a) & 1 == 0))
            if npig == 0:
                continue
            shift = (bits + np.uint64(a))[:, None]
            for m, max_det in enumerate(MAX_DETS):
                sel = rows[rank[rows] < max_det]
                sel = sel[np.argsort(-np.asarray(records["score"])[sel].astype(F64), kind="mergesort")]
                dtm = ((np.asarray(records["match"])[sel][None, :] >> shift) & np.uint64(1)).astype(bool)
                dig = ((np.asarray(records["ignore"])[sel][None, :] >> shift) & np.uint64(1)).astype(bool)
                tps = np.cumsum(dtm & ~dig, axis=1).astype(F64)
                fps = np.cumsum(~dtm & ~dig, axis=1).astype(F64)
                for t in range(T):
                    tp, fp = tps[t], fps[t]
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if tp.size else 0.0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    inds = np.searchsorted(rc, RECALL_THRESHOLDS, side="left")
                    q = np.zeros(R)
                    q[inds < tp.size] = pr[inds[inds < tp.size]]
                    precision[t, :, k, a, m] = q
    return {"precision": precision, "recall": recall}


def summarize(acc: dict) -> dict:
    """`COCOeval._summarizeDets`: {"stats": fp64 [12], "mAP@[0.5:0.95]": 100 stats[0], "mAP@0.5": 100 stats[1]} — the reference's two
    keys (utils/detection.py:462-478).  stats: AP over all thresholds, AP at 0.5, AP at 0.75, AP small / medium / large (maxDets 100);
    AR at maxDets 1, 10, 100, AR small / medium / large (maxDets 100); each the mean of the entries > -1, and -1 where there are none."""
    def mean(x):
        x = x[x > -1]
        return float(np.mean(x)) if x.size else -1.0

    def ap(a, t=None):
        p = acc["precision"] if t is None else acc["precision"][np.nonzero(THRESHOLDS == t)[0]]
        return mean(p[:, :, :, a, len(MAX_DETS) - 1])

    def ar(a, m):
        return mean(acc["recall"][:, :, a, m])

    stats = np.array([ap(0), ap(0, 0.5), ap(0, 0.75), ap(1), ap(2), ap(3), ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)], dtype=F64)
    return {"stats": stats, "mAP@[0.5:0.95]": 100.0 * float(stats[0]), "mAP@0.5": 100.0 * float(stats[1])}


_host_accumulate, _host_summarize = accumulate, summarize


def order_keys(scores) -> np.ndarray:
    """uint32 whose ascending order, ties kept, is `argsort(-scores.astype(F64), kind="mergesort")` — the order `accumulate` puts the
    scores in.  A greater score has a smaller key; +0.0 and -0.0 share one; +inf has the smallest, -inf the greatest of the numbers;
    every NaN has the one key after all of them.  NOT `boxes.score_keys`, which is ascending and puts the NaNs first in a descending
    sort."""
    s = np.ascontiguousarray(np.asarray(scores, dtype=F32).reshape(-1))
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), u, ~(u | np.uint32(0x80000000)))
    key = np.where(s == 0, np.uint32(0x7FFFFFFF), key)
    return np.where(np.isnan(s), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def accumulate_order_reference(records: dict, n_labels: int) -> dict:
    """THE ORDER of `accumulate` (normative for `edtr_coco_order`).  For each (k, a, M) `accumulate` takes the images in ascending id,
    in each the detections of label k with rank < M in rank order, and sorts them stably by `order_keys`.  A stable sort of a filtered
    subsequence is the subsequence of the stable sort, so ONE order of all rows serves every (a, M, t): the rows with 0 <= label <
    ``n_labels`` and 0 <= rank < KEEP, ascending by the composite key (label, `order_keys`(score), image, rank).  (image, label, rank) is
    unique per row, so the key is a strict total order and the result does not depend on the sorting algorithm.
    {"order": int32 [n_kept] row indices in key order, "seg_start": int32 [n_labels + 1]: label k's rows are order[seg_start[k] :
    seg_start[k + 1]]}."""
    label, rank = np.asarray(records["label"]), np.asarray(records["rank"])
    rows = np.nonzero((label >= 0) & (label < int(n_labels)) & (rank >= 0) & (rank < KEEP))[0]
    keys = order_keys(np.asarray(records["score"])[rows])
    order = rows[np.lexsort((rank[rows], np.asarray(records["image"])[rows], keys, label[rows]))].astype(np.int32)
    seg_start = np.searchsorted(label[order], np.arange(int(n_labels) + 1), side="left").astype(np.int32)
    return {"order": order, "seg_start": seg_start}


def accumulate_ordered_reference(records: dict, n_labels: int, order: Optional[dict] = None) -> dict:
    """`accumulate` again, as `edtr_coco_accumulate` computes it: ONE forward walk of each label's segment of the order, no per-row
    array of precisions.  Per (k, a, t, M), over the segment's rows with rank < M: the j-th true positive, with fp_j false positives
    before it, has P_j = j / ((fp_j + j) + spacing(1)) and rc_j = j / npig in fp64.  `accumulate`'s pr falls between true positives
    and `searchsorted(rc, recThr[r], "left")` lands on one, so after the envelope from the right
        precision[r] = max{P_j : rc_j >= recThr[r]},   0 where no j qualifies.
    recThr rises with r: P_j counts for r < cnt_j = #{r : recThr[r] <= rc_j} (from the fp64 division itself; ceil(recThr npig) is
    wrong for 14 thresholds at npig = 100), is folded by max into bin cnt_j - 1 of 101, and a suffix maximum over the bins ends it.
    recall = J / npig with J the true positives.  Equal to `accumulate` bit for bit (tests/test_coco_acc_cpu.py)."""
    K = int(n_labels)
    T, R, A, M = len(THRESHOLDS), len(RECALL_THRESHOLDS), len(AREA_RANGES), len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    o = accumulate_order_reference(records, K) if order is None else order
    rank, match, ignore = np.asarray(records["rank"]), np.asarray(records["match"]), np.asarray(records["ignore"])
    for k in range(K):
        seg = np.asarray(o["order"])[int(o["seg_start"][k]):int(o["seg_start"][k + 1])]
        g_ign = np.asarray(records["gt_ignore"])[np.asarray(records["gt_label"]) == k]
        for a in range(A):
            npig = int(np.count_nonzero((g_ign >> a) & 1 == 0))
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                sel = seg[rank[seg] < max_det]
                for t in range(T):
                    bit = np.uint64(4 * t + a)
                    mt, ig = ((match[sel] >> bit) & np.uint64(1)).astype(bool), ((ignore[sel] >> bit) & np.uint64(1)).astype(bool)
                    at = np.nonzero(mt & ~ig)[0]
                    j = np.arange(1, at.size + 1).astype(F64)
                    fp = np.cumsum(~mt & ~ig)[at].astype(F64)
                    p, rc = j / ((fp + j) + np.spacing(1)), j / F64(npig)
                    bins = np.zeros(R)
                    np.maximum.at(bins, np.searchsorted(RECALL_THRESHOLDS, rc, side="right") - 1, p)
                    precision[t, :, k, a, m] = np.maximum.accumulate(bins[::-1])[::-1]
                    recall[t, k, a, m] = F64(at.size) / F64(npig)
    return {"precision": precision, "recall": recall}


def summarize_ordered_reference(acc: dict) -> dict:
    """`summarize` with a summation order of its own that the shape alone decides (np.mean's pairwise order is numpy's private
    business); `edtr_coco_summarize` equals this bit for bit.  For each statistic, over its slice x [t, r, k] (a recall statistic
    has one r):
      s_tk = the entries > -1 added over r in index order, from 0;  s_k = s_tk added over t in index order, from 0;
      S = s_k added over k in index order, from 0;  the statistic = S / count of the entries > -1, or -1 where that is 0.
    Within 1e-10 of `summarize`: two sums of at most 10 * 101 * 256 terms in [0, 1], each within n 2^-53 relative of the exact sum."""
    def mean(x):                                                # x [t, r, k]
        keep = x > -1
        s_tk = np.zeros((x.shape[0], x.shape[2]))
        for r in range(x.shape[1]):
            s_tk = s_tk + np.where(keep[:, r], x[:, r], 0.0)
        s_k = np.zeros(x.shape[2])
        for t in range(x.shape[0]):
            s_k = s_k + s_tk[t]
        total = F64(0.0)
        for k in range(x.shape[2]):
            total = total + s_k[k]
        count = int(np.count_nonzero(keep))
        return float(total / F64(count)) if count else -1.0

    p, rc, last = np.asarray(acc["precision"]), np.asarray(acc["recall"]), len(MAX_DETS) - 1

    def ap(a, t=slice(None)):
        return mean(p[t, :, :, a, last])

    def ar(a, m):
        return mean(rc[:, None, :, a, m])

    stats = np.array([ap(0), ap(0, slice(0, 1)), ap(0, slice(5, 6)), ap(1), ap(2), ap(3), ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)],
                     dtype=F64)
    return {"stats": stats, "mAP@[0.5:0.95]": 100.0 * float(stats[0]), "mAP@0.5": 100.0 * float(stats[1])}


def scene(rng, n_det: int, n_gt: int, n_labels: int = 1, image_id: int = 0, label_span: Optional[Sequence[int]] = None):
    """A synthetic image's (det, gt) whose IoUs are small rationals, so that ties and threshold hits happen: a 128 x 128 image with
    every corner on a grid of 8.  A box: x0, y0 ~ integers(0, 15), w ~ integers(1, 1 + min(6, 16 - x0)) and h alike, in grid units; with
    probability 0.2 it reaches the image's edge instead, so that every area range is populated.  Ground truth: crowd with probability
    0.2, area w * h.  Detections: half are copies of random ground truths with x2 and y2 each grown by 0 or 1 grid step, half fresh
    boxes; scores integers(1, 9) / 8, so equal scores abound.  Labels ~ integers(*label_span), by default [0, n_labels).  The tests'
    and the timing tool's generator."""
    def fresh(n):
        x0, y0 = rng.integers(0, 15, n), rng.integers(0, 15, n)
        w = rng.integers(1, 1 + np.minimum(6, 16 - x0))
        h = rng.integers(1, 1 + np.minimum(6, 16 - y0))
        edge = rng.random(n) < 0.2
        return np.stack([x0, y0, np.where(edge, 16, x0 + w), np.where(edge, 16, y0 + h)], axis=1).astype(np.int64)

    lo, hi = (0, n_labels) if label_span is None else label_span
    gb = fresh(n_gt)
    gt = {"boxes": (gb * 8).astype(F32), "labels": rng.integers(lo, hi, n_gt).astype(np.int64), "iscrowd": (rng.random(n_gt) < 0.2).astype(np.int64),
          "image_id": int(image_id)}
    gt["area"] = ((gt["boxes"][:, 2] - gt["boxes"][:, 0]) * (gt["boxes"][:, 3] - gt["boxes"][:, 1])).astype(F32)
    db = fresh(n_det)
    dl = rng.integers(lo, hi, n_det).astype(np.int64)
    if n_gt:
        copies = np.nonzero(rng.random(n_det) < 0.5)[0]
        src = rng.integers(0, n_gt, copies.size)
        db[copies] = gb[src]
        db[copies, 2:] = np.minimum(db[copies, 2:] + rng.integers(0, 2, (copies.size, 2)), 16)
        dl[copies] = gt["labels"][src]
    det = {"boxes": (db * 8).astype(F32), "scores": (rng.integers(1, 9, n_det) / 8).astype(F32), "labels": dl}
    return det, gt


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _round8(v: int) -> int:
    return (int(v) + 7) // 8 * 8


def _rows(boxes, *per_row) -> int:
    """the row count of [n, 4] boxes with [n] companions (numpy arrays or tensors)"""
    if getattr(boxes, "ndim", 0) != 2 or boxes.shape[1] != 4:
        raise ValueError(f"boxes are [n, 4], got {tuple(getattr(boxes, 'shape', ()))}")
    n = int(boxes.shape[0])
    for v in per_row:
        if getattr(v, "ndim", 0) != 1 or int(v.shape[0]) != n:
            raise ValueError(f"one value per box: got {tuple(getattr(v, 'shape', ()))} for {n} boxes")
    return n


class Records:
    """The running record of a data set's matching on the device: `update` appends one image by `edtr_coco_match` (two launches, no
    host sync: both offsets stay on the device), `to_host` makes the single copy and returns the records `accumulate` takes.
    ``capacity`` detection rows and ``gt_capacity`` ground-truth rows (default: as many).  Every field lives in ONE device buffer, each
    with a guard row behind it that no launch may write; rows that do not fit are dropped on the device, the offsets move on all the
    same, and `to_host` then raises."""
    GUARD = 0x5A

    def __init__(self, capacity: int, n_labels: int, device=None, gt_capacity: Optional[int] = None):
        import torch
        from .imageio import _device
        self.capacity, self.gt_capacity = int(capacity), int(capacity if gt_capacity is None else gt_capacity)
        self.n_labels = int(n_labels)
        if self.capacity <= 0 or self.gt_capacity <= 0 or max(self.capacity, self.gt_capacity) > 1 << 30:
            raise ValueError(f"capacities must lie in [1, 2^30], got {capacity} and {gt_capacity}")
        if not 0 < self.n_labels <= MAX_LABELS:
            raise ValueError(f"n_labels must lie in [1, {MAX_LABELS}], got {n_labels}")
        self.device = _device(device)
        self._layout, at = {}, 8                                # bytes 0 .. 7: the two offsets
        for name, dtype in sorted(DET_FIELDS + GT_FIELDS, key=lambda f: -np.dtype(f[1]).itemsize):
            rows = (self.capacity if (name, dtype) in DET_FIELDS else self.gt_capacity) + 1
            self._layout[name] = (at, rows, np.dtype(dtype))
            at = _round8(at + rows * np.dtype(dtype).itemsize)
        host = np.full(at, self.GUARD, dtype=np.uint8)
        host[:8] = 0
        self.buffer = torch.from_numpy(host).to(self.device)
        view = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
        self.fields = {name: self.buffer[at:at + rows * dt.itemsize].view(torch.float32 if dt == F32 else view[dt.itemsize])
                       for name, (at, rows, dt) in self._layout.items()}
        self.offsets = self.buffer[:8].view(torch.int32)
        self.det_offset, self.gt_offset = self.offsets[0:1], self.offsets[1:2]
        self.thresholds = torch.from_numpy(THRESHOLDS.copy()).to(self.device)
        self.areas = torch.from_numpy(AREA_RANGES.copy()).to(self.device)
        self.recall_thresholds = torch.from_numpy(RECALL_THRESHOLDS.copy()).to(self.device)
        self.image_ids: set = set()
        self._acc = None                                        # the buffers of `accumulate`, made at its first call
        self._acc_fresh = self._stats_fresh = False

    @classmethod
    def from_host(cls, records: dict, n_labels: int, device=None, capacity: Optional[int] = None, gt_capacity: Optional[int] = None) -> "Records":
        """Records on the device from records on the host (`DET_FIELDS`, `GT_FIELDS`: what `to_host` and `merge_records` return), with
        exactly their rows as capacity unless larger ones are given: the multi-rank flow is gather -> `merge_records` -> `from_host` -> `accumulate`.  The rows may
        come in any order (the key of `accumulate_order_reference` decides), but (image, label, rank) must not repeat among the rows
        with a label: the order would not be strict."""
        import torch
        cols = {name: np.ascontiguousarray(np.asarray(records[name]).astype(dtype).reshape(-1)) for name, dtype in DET_FIELDS + GT_FIELDS}
        n, g = cols["image"].shape[0], cols["gt_image"].shape[0]
        if any(cols[name].shape[0] != (n if (name, dtype) in DET_FIELDS else g) for name, dtype in DET_FIELDS + GT_FIELDS):
            raise ValueError("every detection field takes one value per detection row and every ground-truth field one per ground truth")
        known = cols["label"] >= 0
        triples = np.stack([cols["image"][known], cols["label"][known], cols["rank"][known]], axis=1)
        triples = triples[np.lexsort((triples[:, 2], triples[:, 1], triples[:, 0]))]
        if np.any(np.all(triples[1:] == triples[:-1], axis=1)):
            raise ValueError("records repeat an (image, label, rank) row: merge the shards with merge_records first")
        if (capacity is not None and capacity < n) or (gt_capacity is not None and gt_capacity < g):
            raise ValueError(f"{n} detection and {g} ground-truth rows do not fit capacities of {capacity} and {gt_capacity}")
        rec = cls(max(n, 1) if capacity is None else capacity, n_labels, device, gt_capacity=max(g, 1) if gt_capacity is None else gt_capacity)
        for name, col in cols.items():
            if col.shape[0]:
                rec.fields[name][:col.shape[0]].copy_(torch.from_numpy(col.view(np.int64) if col.dtype == np.uint64 else col))
        rec.offsets.copy_(torch.tensor([n, g], dtype=torch.int32))
        rec.image_ids = set(cols["image"].tolist()) | set(cols["gt_image"].tolist())
        return rec

    def _acc_state(self) -> dict:
        """the output buffers of `accumulate` / `stats` in ONE device buffer, each with 8 guard bytes behind it, and the workspace"""
        if self._acc is None:
            import torch
            from . import lib as L
            ws = int(L.load().edtr_coco_accumulate_workspace(self.capacity, self.n_labels))
            if ws <= 0:
                raise ValueError(f"accumulate on the device orders at most {ACC_MAX_ROWS} rows, these records hold {self.capacity}")
            T, R, K, A, M = len(THRESHOLDS), len(RECALL_THRESHOLDS), self.n_labels, len(AREA_RANGES), len(MAX_DETS)
            sizes = (("precision", T * R * K * A * M, torch.float64), ("recall", T * K * A * M, torch.float64), ("stats", 13, torch.float64),
                     ("order", self.capacity, torch.int32), ("seg_start", K + 1, torch.int32), ("n_kept", 1, torch.int32), ("status", 1, torch.int32))
            layout, at = {}, 0
            for name, count, dt in sizes:
                nbytes = count * (8 if dt == torch.float64 else 4)
                layout[name] = (at, nbytes, dt)
                at = _round8(at + nbytes) + 8
            buffer = torch.full((at,), self.GUARD, dtype=torch.uint8, device=self.device)
            self._acc = {"buffer": buffer, "layout": layout, "workspace": torch.empty(ws, dtype=torch.uint8, device=self.device)}
            self._acc.update({name: buffer[at:at + nbytes].view(dt) for name, (at, nbytes, dt) in layout.items()})
        return self._acc

    def accumulate(self) -> dict:
        """`accumulate` of everything recorded so far, on the device: {"precision": fp64 [T, R, K, A, M], "recall": fp64 [T, K, A, M]} as
        device tensors, bit for bit what `accumulate(self.to_host(), n_labels)` returns when each image was recorded once.  The sort of
        `edtr_coco_order` and the walk of `edtr_coco_accumulate`; no host sync, and no row count reaches the host: an overflow of the
        capacity shows in `result`.  The tensors are this object's and are overwritten by the next call."""
        from . import ops
        st = self._acc_state()
        ops.launch(ops.make_coco_order(rec=self.fields, det_offset=self.det_offset, capacity=self.capacity, n_labels=self.n_labels,
                                       workspace=st["workspace"], order=st["order"], seg_start=st["seg_start"], n_kept=st["n_kept"], status=st["status"]))
        ops.launch(ops.make_coco_accumulate(order=st["order"], seg_start=st["seg_start"], rec=self.fields, capacity=self.capacity,
                                            gt_offset=self.gt_offset, gt_capacity=self.gt_capacity, n_labels=self.n_labels,
                                            recall_thresholds=self.recall_thresholds, workspace=st["workspace"], precision=st["precision"],
                                            recall=st["recall"], status=st["status"]))
        self._acc_fresh, self._stats_fresh = True, False
        T, R, K, A, M = len(THRESHOLDS), len(RECALL_THRESHOLDS), self.n_labels, len(AREA_RANGES), len(MAX_DETS)
        return {"precision": st["precision"].view(T, R, K, A, M), "recall": st["recall"].view(T, K, A, M)}

    def order_to_host(self) -> dict:
        """what the last `accumulate` sorted, copied to the host (for tests and debugging; `accumulate_order_reference`'s dict plus
        the status word): {"order": int32 [n_kept], "seg_start": int32 [n_labels + 1], "status": int}"""
        if self._acc is None or not self._acc_fresh:
            raise RuntimeError("accumulate() has not run since the last update")
        n_kept = int(self._acc["n_kept"].cpu()[0])
        return {"order": self._acc["order"][:n_kept].cpu().numpy(), "seg_start": self._acc["seg_start"].cpu().numpy(),
                "status": int(self._acc["status"].cpu()[0])}

    def stats(self):
        """The 12 statistics of `summarize_ordered_reference` as an fp64 [12] device tensor (`edtr_coco_summarize` on the result of
        `accumulate`, which is run first if an image was recorded since).  No host sync."""
        from . import ops
        if not self._acc_fresh:
            self.accumulate()
        st = self._acc_state()
        ops.launch(ops.make_coco_summarize(precision=st["precision"], recall=st["recall"], n_labels=self.n_labels, status=st["status"], out=st["stats"]))
        self._stats_fresh = True
        return st["stats"][:12]

    def result(self) -> dict:
        """{"stats": fp64 [12], "mAP@[0.5:0.95]", "mAP@0.5"} on the host after ONE copy of 104 bytes: the statistics and the status word.
        Raises RuntimeError, as `to_host` does, if more rows were appended than a capacity holds."""
        if not self._stats_fresh:
            self.stats()
        raw = self._acc["stats"].cpu().numpy()
        if int(raw[12:].view(np.int64)[0]) != 0:
            raise RuntimeError(f"more rows were appended than records of {self.capacity} detection and {self.gt_capacity} ground-truth rows hold: "
                               f"pass a larger capacity")
        stats = raw[:12].copy()
        return {"stats": stats, "mAP@[0.5:0.95]": 100.0 * float(stats[0]), "mAP@0.5": 100.0 * float(stats[1])}

    def update(self, det: dict, target: dict) -> None:
        """Append one image: ``det`` = {"boxes" fp32 [n, 4], "scores" fp32 [n], "labels" [n]} and optionally "count" (int32 [1] on the
        device: rows at or past it do not exist and are never read), ``target`` = the reference's annotation dict {"boxes", "labels",
        "image_id"} and optionally "area" (default (x2 - x1) * (y2 - y1) in fp32) and "iscrowd" (default 0).  Host arrays cost one
        upload each; nothing is read back."""
        import torch
        from . import ops
        dev = self.device
        image_id = _image_id(target)
        if image_id in self.image_ids:
            raise ValueError(f"image id {image_id} was recorded before")
        if not -2 ** 31 <= image_id < 2 ** 31:
            raise ValueError(f"image ids are int32, got {image_id}")
        n = _rows(det["boxes"], det["scores"], det["labels"])
        g = _rows(target["boxes"], target["labels"])
        if n > MAX_DET or g > MAX_GT:
            raise ValueError(f"an image takes at most {MAX_DET} detections and {MAX_GT} ground truths, got {n} and {g}")
        db, ds = _boxes._f32_on(det["boxes"], dev, "boxes"), _boxes._f32_on(det["scores"], dev, "scores")
        dl = _boxes._labels_on(torch.as_tensor(det["labels"]).to(torch.int64), dev)
        count = det.get("count")
        if count is not None and (not isinstance(count, torch.Tensor) or count.dtype != torch.int32 or count.numel() != 1 or count.device != db.device):
            raise TypeError("count must be an int32 [1] tensor on the records' device")
        gb = _boxes._f32_on(target["boxes"], dev, "boxes")
        gl = _boxes._labels_on(torch.as_tensor(target["labels"]).to(torch.int64), dev)
        area = target.get("area")
        area = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]) if area is None else _boxes._f32_on(torch.as_tensor(area).to(torch.float32), dev, "area")
        crowd = target.get("iscrowd")
        crowd = torch.zeros(g, dtype=torch.uint8, device=dev) if crowd is None else (torch.as_tensor(crowd).to(dev) != 0).to(torch.uint8)
        if area.ndim != 1 or area.shape[0] != g or crowd.ndim != 1 or crowd.shape[0] != g:
            raise ValueError("ground truth takes one area and one crowd flag per box")
        self.image_ids.add(image_id)
        self._acc_fresh = self._stats_fresh = False
        if n == 0 and g == 0:
            return
        ops.launch(ops.make_coco_match(det_boxes=db, det_scores=ds, det_labels=dl, count=count, gt_boxes=gb, gt_labels=gl, gt_area=area.contiguous(),
                                       gt_crowd=crowd.contiguous(), n_labels=self.n_labels, image_id=image_id, thresholds=self.thresholds,
                                       areas=self.areas, rec=self.fields, det_offset=self.det_offset, capacity=self.capacity,
                                       gt_offset=self.gt_offset, gt_capacity=self.gt_capacity))

    def to_host(self) -> dict:
        """The single device -> host copy: the records as a dict of numpy arrays (`DET_FIELDS`, `GT_FIELDS`).  Raises RuntimeError if more
        rows were appended than the capacity holds, or if a guard row was written."""
        raw = self.buffer.cpu().numpy()
        n_det, n_gt = (int(v) for v in raw[:8].view(np.int32))
        out = {}
        for name, (at, rows, dt) in self._layout.items():
            col = raw[at:at + rows * dt.itemsize].view(dt)
            if not np.all(col[rows - 1:].view(np.uint8) == self.GUARD):
                raise RuntimeError(f"the guard row behind '{name}' was written")
            out[name] = col[:min(max(n_det if name in dict(DET_FIELDS) else n_gt, 0), rows - 1)].copy()
        if not 0 <= n_det <= self.capacity or not 0 <= n_gt <= self.gt_capacity:
            raise RuntimeError(f"{n_det} detections and {n_gt} ground truths were appended to records of {self.capacity} and {self.gt_capacity} "
                               f"rows: pass a larger capacity")
        return out


def evaluate(images, targets, detnet, n_labels: int, mode: str = "direct", capacity: Optional[int] = None, *, accumulate: str = "host",
             return_records: bool = False, **detect_kwargs) -> dict:
    """The tail of the reference's detection test (main/det/test_edtr.py:138-190): for every image (fp32 [3, h, w] on the device, as
    `evalutil.restore_dataset` returns them) `boxes.detect(image, detnet, mode, **detect_kwargs)` — in "direct" mode ``detnet([image])`` may
    also return the detection dict {"boxes", "scores", "labels"[, "count"]} itself — and one `Records.update` against the image's target,
    the reference's annotation dict ("boxes", "labels", "area", "iscrowd", "image_id").  No host sync in the loop and ONE device -> host
    copy at the end; targets that are not on the device yet cost one upload each.  ``capacity``: detection rows of the record, by
    default 100 per image (a detector's `detections_per_img`); more raise RuntimeError after the copy.
    Returns {"stats": fp64 [12], "mAP@[0.5:0.95]", "mAP@0.5" (in percent, the reference's two keys), "precision", "recall", "records"}.
    ``accumulate``: "host" (the default) copies the records and runs `accumulate` and `summarize` there; "device" runs
    `Records.accumulate` and `Records.result` instead — precision and recall are bit for bit the same, the statistics are those of
    `summarize_ordered_reference` (within 1e-10 of `summarize`), and no record leaves the device: "records" is then returned only with
    ``return_records`` (which the host path always does).  precision and recall are copied to the host for the same keys; a caller
    that wants the one small copy alone keeps a `Records` and calls `result`."""
    if accumulate not in ("host", "device"):
        raise ValueError(f'accumulate is "host" or "device", got {accumulate!r}')
    images, targets = list(images), list(targets)
    if not images or len(images) != len(targets):
        raise ValueError(f"evaluate needs as many targets as images, got {len(targets)} for {len(images)}")
    rec = None
    for image, target in zip(images, targets):
        if mode == "direct":
            out = detnet([image])
            det = out if isinstance(out, dict) else dict(_boxes._first(out))
        else:
            det = _boxes.detect(image, detnet, mode=mode, **detect_kwargs)
        if rec is None:
            gt_rows = max(1, sum(int(t["boxes"].shape[0]) for t in targets))
            rec = Records(capacity or KEEP * len(images), n_labels, det["boxes"].device, gt_capacity=gt_rows)
        rec.update(det, target)
    if accumulate == "device":
        acc = rec.accumulate()
        out = {**rec.result(), "precision": acc["precision"].cpu().numpy(), "recall": acc["recall"].cpu().numpy()}
        if return_records:
            out["records"] = rec.to_host()
        return out
    records = rec.to_host()
    acc = _host_accumulate(records, n_labels)
    return {**summarize(acc), "precision": acc["precision"], "recall": acc["recall"], "records": records}
