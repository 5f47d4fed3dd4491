#!/usr/bin/env python
"""Time the detector's training-target flows (edtr_amd/targets.py) on the device and write profiles/targets_timing.json:

  rpn_targets   the v2 detector's shape: an 800 x 1344 batch of 2 images, five levels from 200 x 336 down, A = 3 (268 569 anchors), 20
                ground truths per image, 0.7 / 0.3 with low-quality matches, 256 / 0.5: the whole call (anchors, the two match launches
                with the encoding of every anchor, the sampler), and its parts;
  roi_targets   2 x 2000 proposals against the same ground truths, 0.5 / 0.5, 512 / 0.25, weights (10, 10, 5, 5).

Beside each, torch's own chain on the same device, written as the reference runs it: the dense IoU matrix, max(dim=0), the thresholds,
max(dim=1) / == / where of set_low_quality_matches_, the labels, encode_boxes, and the sampler with its two torch.randperm and its
torch.where per image.  The matched indices, labels and regression targets of the two sides are compared in the same run (the samples
cannot be: randperm draws others); the counts of what differs are recorded, not asserted.

ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case with the cases of a
group taking turns; the median, the fastest and the slowest window are kept (tools/bench_boxes.py's method).  Inputs are resident on
the device; the wrappers' allocations and table uploads are inside.  Recorded with the kernel source hash, not gated.  Commit the file
only after this has run on the device.

    python tools/bench_targets.py [--out profiles/targets_timing.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edtr_amd import rng, rois, targets  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from bench_boxes import measure  # noqa: E402
from bench_labels import REPEATS, WARMUP, WINDOW_S  # noqa: E402

PADDED = (800, 1344)
GRIDS = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
N, G, PROPOSALS = 2, 20, 2000


def ground_truth(dev):
    rs = np.random.default_rng(2030)
    out = []
    for _ in range(N):
        w, h = rs.uniform(30, 400, G), rs.uniform(30, 400, G)
        x1, y1 = rs.uniform(0, PADDED[1] - w), rs.uniform(0, PADDED[0] - h)
        out.append({"boxes": torch.from_numpy(np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)).to(dev),
                    "labels": torch.from_numpy(rs.integers(1, 91, G)).to(dev)})
    return out


def proposals_for(gt, dev):
    """what the RPN hands the box head in training: most boxes anywhere, a fifth of them near a ground truth"""
    rs = np.random.default_rng(2031)
    out = []
    for t in gt:
        g = t["boxes"].cpu().numpy().astype(np.float64)
        w, h = rs.uniform(20, 300, PROPOSALS), rs.uniform(20, 300, PROPOSALS)
        x1, y1 = rs.uniform(0, PADDED[1] - w), rs.uniform(0, PADDED[0] - h)
        b = np.stack([x1, y1, x1 + w, y1 + h], axis=1)
        k = PROPOSALS // 5
        src = g[rs.integers(0, G, k)]
        side = np.stack([src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]] * 2, axis=1)
        b[:k] = src + rs.normal(0, 0.1, (k, 4)) * side
        out.append(torch.from_numpy(b.astype(np.float32)).to(dev))
    return out


def torch_iou(a, b):
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area_a[:, None] + area_b - inter)


def torch_matcher(q, high, low, allow):
    vals, matches = q.max(dim=0)
    every = matches.clone() if allow else None
    below, between = vals < low, (vals >= low) & (vals < high)
    matches[below] = -1
    matches[between] = -2
    if allow:
        highest, _ = q.max(dim=1)
        pred = torch.where(q == highest[:, None])[1]
        matches[pred] = every[pred]
    return matches


def torch_encode(g, p, weights):
    wx, wy, ww, wh = weights
    ew, eh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    ecx, ecy = p[:, 0] + 0.5 * ew, p[:, 1] + 0.5 * eh
    gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    gcx, gcy = g[:, 0] + 0.5 * gw, g[:, 1] + 0.5 * gh
    return torch.stack((wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * torch.log(gw / ew), wh * torch.log(gh / eh)), dim=1)


def torch_sampler(labels, batch, fraction):
    pos, neg = [], []
    for lab in labels:
        positive, negative = torch.where(lab >= 1)[0], torch.where(lab == 0)[0]
        num_pos = min(positive.numel(), int(batch * fraction))
        num_neg = min(negative.numel(), batch - num_pos)
        p = positive[torch.randperm(positive.numel(), device=lab.device)[:num_pos]]
        q = negative[torch.randperm(negative.numel(), device=lab.device)[:num_neg]]
        mp, mn = torch.zeros_like(lab, dtype=torch.uint8), torch.zeros_like(lab, dtype=torch.uint8)
        mp[p] = 1
        mn[q] = 1
        pos.append(mp)
        neg.append(mn)
    return pos, neg


def torch_rpn_chain(anchors, gt):
    """assign_targets_to_anchors, BoxCoder.encode and the sampler of compute_loss"""
    labels, regression, matched = [], [], []
    for t in gt:
        m = torch_matcher(torch_iou(t["boxes"], anchors), 0.7, 0.3, True)
        lab = (m >= 0).to(torch.float32)
        lab[m == -1] = 0.0
        lab[m == -2] = -1.0
        labels.append(lab)
        matched.append(m)
        regression.append(torch_encode(t["boxes"][m.clamp(min=0)], anchors, (1.0, 1.0, 1.0, 1.0)))
    pos, neg = torch_sampler(labels, 256, 0.5)
    return matched, labels, regression, pos, neg


def torch_roi_chain(proposals, gt):
    """select_training_samples"""
    out = []
    props = [torch.cat((p, t["boxes"])) for p, t in zip(proposals, gt)]
    labels, matched = [], []
    for p, t in zip(props, gt):
        m = torch_matcher(torch_iou(t["boxes"], p), 0.5, 0.5, False)
        lab = t["labels"][m.clamp(min=0)].to(torch.int64)
        lab[m == -1] = 0
        lab[m == -2] = -1
        labels.append(lab)
        matched.append(m.clamp(min=0))
    pos, neg = torch_sampler(labels, 512, 0.25)
    for p, t, lab, m, mp, mn in zip(props, gt, labels, matched, pos, neg):
        idx = torch.where(mp | mn)[0]
        out.append((p[idx], lab[idx], m[idx], torch_encode(t["boxes"][m[idx]], p[idx], (10.0, 10.0, 5.0, 5.0))))
    return out, labels, matched


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case, the cases of one group taking turns; ms = the median window per call, ms_min / ms_max the spread; "
                        "inputs resident on the device, the wrappers' allocations and table uploads included"}
    gt = ground_truth(dev)
    src = rng.NoiseSource(2032, [0, 1])
    anchors = rois.anchors(GRIDS, PADDED)
    gt_boxes = [t["boxes"] for t in gt]

    # the two sides agree before anything is timed
    mine = targets.rpn_targets(GRIDS, PADDED, gt, source=src, draw=0)
    t_matched, t_labels, t_regression, t_pos, _ = torch_rpn_chain(anchors, gt)
    finite = torch.isfinite(torch.stack(t_regression)) & torch.isfinite(mine.regression)
    check = {"matched_differ": int((mine.matched != torch.stack(t_matched)).sum()), "labels_differ": int((mine.labels != torch.stack(t_labels)).sum()),
             "regression_max_abs": float((mine.regression - torch.stack(t_regression))[finite].abs().max()),
             "sampled_counts": mine.counts.cpu().tolist(), "torch_sampled_positives": [int(p.sum()) for p in t_pos]}
    m = targets.match(anchors, gt_boxes, 0.7, 0.3, True, "rpn", weights=targets.RPN_WEIGHTS)
    group = measure({"rpn_targets": lambda: targets.rpn_targets(GRIDS, PADDED, gt, source=src, draw=0),
                     "match_and_encode_launches": lambda: targets.match(anchors, gt_boxes, 0.7, 0.3, True, "rpn", weights=targets.RPN_WEIGHTS),
                     "sample_launch": lambda: targets.sample(m.labels, 256, 0.5, src, 0, rng.PURPOSE_SAMPLE_RPN, m.table, m.table_host),
                     "torch_chain": lambda: torch_rpn_chain(anchors, gt),
                     "torch_chain_without_sampler": lambda: [torch_encode(t["boxes"][torch_matcher(torch_iou(t["boxes"], anchors), 0.7, 0.3, True).clamp(min=0)],
                                                                          anchors, (1.0, 1.0, 1.0, 1.0)) for t in gt]})
    group.update(anchors=int(anchors.shape[0]), images=N, ground_truths_per_image=G, agreement=check,
                 dense_iou_bytes_per_image=int(4 * G * anchors.shape[0]))
    result["rpn_targets"] = group

    props = proposals_for(gt, dev)
    mine = targets.roi_targets(props, gt, source=src, draw=0)
    _, t_labels, t_matched = torch_roi_chain(props, gt)
    mm = targets.match([torch.cat((p, t["boxes"])) for p, t in zip(props, gt)], gt_boxes, 0.5, 0.5, False, "roi", gt_labels=[t["labels"] for t in gt])
    check = {"matched_differ": int((mm.matched.clamp(min=0) != torch.cat(t_matched)).sum()), "labels_differ": int((mm.labels != torch.cat(t_labels)).sum()),
             "sampled_counts": mine.counts.cpu().tolist()}
    group = measure({"roi_targets": lambda: targets.roi_targets(props, gt, source=src, draw=0), "torch_chain": lambda: torch_roi_chain(props, gt)})
    group.update(proposals_per_image=PROPOSALS, images=N, ground_truths_per_image=G, agreement=check)
    result["roi_targets"] = group

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
