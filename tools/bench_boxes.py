#!/usr/bin/env python
"""Time the detection-box launches (edtr_amd/boxes.py) on the device and write profiles/boxes_timing.json:

  batched_nms   n = 1000, 4096 and 19 000 candidates with 20 labels, in the exact-length form (which reads the count) and in the
                max_out = 100 form (no host sync, the walk ends after 100 kept); the counting rank alone (`boxes.rank_order`, the
                first of the three launches: what choosing an O(n^2), deterministic, atomic-free sort costs); and beside them the
                one part of the job torch has on this device, a stable descending `torch.sort` of the scores
  detections    P = 1000 proposals with C = 21 and C = 91 classes, whole call; beside it torch's own chain for the parts torch has:
                softmax, the box decoding, the clip, the two filters and the sort of the surviving scores (no NMS: torch has none)

ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case with the cases of a
group taking turns; the median, the fastest and the slowest window are kept (tools/bench_labels.py's method).  Inputs are resident on
the device; the wrappers' allocations and their 4-byte count reads are inside.  Recorded with the kernel source hash, not gated.
Commit the file only after this has run on the device.

    python tools/bench_boxes.py [--out profiles/boxes_timing.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edtr_amd import boxes  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from bench_labels import REPEATS, WARMUP, WINDOW_S, window_ms  # noqa: E402


def measure(fns: dict) -> dict:
    iters = {}
    for name, fn in fns.items():
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(10, int(np.ceil(WINDOW_S * 1e3 / window_ms(fn, 10))))
    samples = {name: [] for name in fns}
    for _ in range(REPEATS):
        for name, fn in fns.items():
            samples[name].append(window_ms(fn, iters[name]))
    return {name: {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "calls_per_window": iters[name],
                   "windows": REPEATS, "window_ms": [float(x) for x in v]} for name, v in samples.items()}


def nms_inputs(n: int, labels: int, dev):
    """n candidates as a detector emits them: n / 40 objects in a 1333 x 800 image, each with about 40 jittered candidates (a tenth
    of a side off in position and extent), uniform scores, `labels` labels by object with one candidate in ten mislabelled"""
    rng = np.random.default_rng([n, labels])
    objects = max(1, n // 40)
    oxy, owh = rng.uniform(0, (1100, 650), (objects, 2)), rng.uniform(30, 300, (objects, 2))
    olab = rng.integers(1, labels + 1, objects)
    which = rng.integers(0, objects, n)
    wh = owh[which] * rng.uniform(0.9, 1.1, (n, 2))
    xy = oxy[which] + owh[which] * rng.uniform(-0.1, 0.1, (n, 2))
    bx = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    lab = np.where(rng.uniform(0, 1, n) < 0.1, rng.integers(1, labels + 1, n), olab[which]).astype(np.int64)
    to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return to(bx), to(rng.uniform(0, 1, n).astype(np.float32)), to(lab)


def head_inputs(P: int, C: int, hw, dev):
    rng = np.random.default_rng([P, C])
    h, w = hw
    x1, y1 = rng.uniform(0, w * 0.8, P), rng.uniform(0, h * 0.8, P)
    prop = np.stack([x1, y1, np.minimum(x1 + rng.uniform(8, w * 0.5, P), w), np.minimum(y1 + rng.uniform(8, h * 0.5, P), h)], axis=1)
    logits = rng.normal(0, 1, (P, C))
    logits[np.arange(P), rng.integers(0, C, P)] += rng.uniform(2, 6, P)
    codes = rng.normal(0, 0.5, (P, 4 * C))
    to = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)  # noqa: E731
    return to(logits), to(codes), to(prop)


def torch_head_chain(logits, codes, prop, hw, score_thresh=0.05, min_size=1e-2):
    """softmax, BoxCoder.decode_single, clip, the two filters, and a sort of what is left: what torch itself offers of the job"""
    P, C = logits.shape
    scores = torch.softmax(logits, -1)
    wd, ht = prop[:, 2] - prop[:, 0], prop[:, 3] - prop[:, 1]
    cx, cy = prop[:, 0] + 0.5 * wd, prop[:, 1] + 0.5 * ht
    dx, dy = codes[:, 0::4] / 10.0, codes[:, 1::4] / 10.0
    dw = torch.clamp(codes[:, 2::4] / 5.0, max=boxes.BBOX_XFORM_CLIP)
    dh = torch.clamp(codes[:, 3::4] / 5.0, max=boxes.BBOX_XFORM_CLIP)
    pcx, pcy = dx * wd[:, None] + cx[:, None], dy * ht[:, None] + cy[:, None]
    hw_, hh_ = 0.5 * torch.exp(dw) * wd[:, None], 0.5 * torch.exp(dh) * ht[:, None]
    bx = torch.stack((pcx - hw_, pcy - hh_, pcx + hw_, pcy + hh_), dim=2)
    bx = torch.stack((bx[..., 0].clamp(0, hw[1]), bx[..., 1].clamp(0, hw[0]), bx[..., 2].clamp(0, hw[1]), bx[..., 3].clamp(0, hw[0])), dim=2)
    bx, scores = bx[:, 1:].reshape(-1, 4), scores[:, 1:].reshape(-1)
    keep = torch.where((scores > score_thresh) & (bx[:, 2] - bx[:, 0] >= min_size) & (bx[:, 3] - bx[:, 1] >= min_size))[0]
    return bx[keep], torch.sort(scores[keep], descending=True, stable=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxes_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case, the cases of one group taking turns; ms = the median window per call, ms_min / ms_max the spread; "
                        "inputs resident on the device, the wrappers' allocations and 4-byte count reads included",
              "batched_nms": {}, "detections": {}}
    for n in (1000, 4096, 19000):
        bx, s, lab = nms_inputs(n, 20, dev)
        kept = int(boxes.batched_nms(bx, s, lab, 0.5).numel())
        group = measure({"launches": lambda: boxes.batched_nms(bx, s, lab, 0.5),
                         "launches_max_out_100": lambda: boxes.batched_nms(bx, s, lab, 0.5, max_out=100),
                         "rank_launch_only": lambda: boxes.rank_order(s),
                         "torch_sort_only": lambda: torch.sort(s, descending=True, stable=True)})
        group.update(n=n, labels=20, iou_threshold=0.5, kept=kept, mask_bytes=8 * n * math.ceil(n / 64), rank_comparisons=n * n)
        result["batched_nms"][str(n)] = group
    for C in (21, 91):
        hw = (800, 1333)
        logits, codes, prop = head_inputs(1000, C, hw, dev)
        cand = int(boxes.candidates(logits, codes, prop, hw)[0].shape[0])
        group = measure({"launches": lambda: boxes.detections(logits, codes, prop, hw),
                         "torch_chain_without_nms": lambda: torch_head_chain(logits, codes, prop, hw)})
        group.update(P=1000, C=C, candidates=cand, kept=int(boxes.detections(logits, codes, prop, hw)["labels"].numel()))
        result["detections"][f"C{C}"] = group
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
