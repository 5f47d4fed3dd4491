#!/usr/bin/env python
"""Time the detection-score path (edtr_amd/coco.py) on the device and write profiles/coco_timing.json:

  update      `Records.update` for one image with 100 detections / 20 ground truths / 20 labels and with 1000 / 200 / 80, inputs
              resident on the device (the record is rewound by zeroing its two offsets on the device, inside the timed call); beside
              it the host path it replaces on the same inputs: the detections copied to the host and `match_reference` there
  evaluate    `coco.evaluate` over 64 synthetic images (100 / 20 / 20 each) with a stub detector that returns prepared detections on
              the device: the loop, the one copy, `accumulate` and `summarize`; and how much of that the host-side `accumulate` +
              `summarize` are; beside it the same call with `accumulate="device"`
  accumulate  `Records.accumulate()` + `stats()` + `result()` (the sort, the walk, the 12 statistics and the one copy of 104 bytes,
              wrapper included) against the path they replace on the same records, `to_host()` + `accumulate` + `summarize` on this
              host, at 64 images x 100 detections / 20 ground truths / 20 labels (the shape of `evaluate` above), 1000 x 100 / 20 /
              80 labels and 5000 x 100 / 20 / 80 (500 000 rows); the records are made on the device by `Records.update`

ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case with the cases of a
group taking turns; the median, the fastest and the slowest window are kept (tools/bench_labels.py's method).  The host path is
timed with the wall clock, each call ending in the copies it needs.  Recorded with the kernel source hash, not gated.  Commit the file
only after this has run on the device.

    python tools/bench_coco.py [--out profiles/coco_timing.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edtr_amd import coco  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from bench_boxes import measure  # noqa: E402
from bench_labels import REPEATS, WARMUP, WINDOW_S  # noqa: E402


def wall_ms(fn, repeats: int = REPEATS) -> dict:
    """a host-side call: the median, fastest and slowest of ``repeats`` wall-clock runs after one warm-up"""
    fn()
    v = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "runs": repeats}


def on_dev(d: dict, dev) -> dict:
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v for k, v in d.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case; ms = the median window per call, ms_min / ms_max the spread; inputs resident on the device; "
                        "host_path: wall clock of the device -> host copies of one image's detections plus match_reference",
              "update": {}, "evaluate": {}, "accumulate": {}}
    for d, g, labels in ((100, 20, 20), (1000, 200, 80)):
        det, gt = coco.scene(np.random.default_rng([d, g, labels]), d, g, labels)
        ddet, dgt = on_dev(det, dev), on_dev(gt, dev)
        rec = coco.Records(d, labels, dev, gt_capacity=g)

        def update():
            rec.offsets.zero_()
            rec.image_ids.clear()
            rec.update(ddet, dgt)

        def host_path():
            return coco.match_reference({k: v.cpu() for k, v in ddet.items()}, gt, n_labels=labels)

        update()
        got, want = rec.to_host(), host_path()
        group = measure({"launches": update})
        group["host_path"] = wall_ms(host_path)
        group.update(detections=d, ground_truths=g, labels=labels,
                     equals_host_path=bool(all(np.array_equal(got[k], want[k]) for k, _ in coco.DET_FIELDS + coco.GT_FIELDS)))
        result["update"][f"{d}_{g}_{labels}"] = group
    n_images, (d, g, labels) = 64, (100, 20, 20)
    rng = np.random.default_rng(64)
    pairs = [coco.scene(rng, d, g, labels, image_id=i) for i in range(n_images)]
    prepared, targets = [on_dev(p[0], dev) for p in pairs], [on_dev(p[1], dev) for p in pairs]
    images = [torch.zeros((3, 8, 8), device=dev)] * n_images

    def evaluate():
        it = iter(prepared)
        return coco.evaluate(images, targets, lambda _: next(it), n_labels=labels)

    records = evaluate()["records"]
    group = {"whole_call": wall_ms(evaluate), "host_accumulate_summarize": wall_ms(lambda: coco.summarize(coco.accumulate(records, labels)))}

    def evaluate_device():
        it = iter(prepared)
        return coco.evaluate(images, targets, lambda _: next(it), n_labels=labels, accumulate="device")

    group["whole_call_device_accumulate"] = wall_ms(evaluate_device)
    group.update(images=n_images, detections=d, ground_truths=g, labels=labels, mAP=evaluate()["mAP@[0.5:0.95]"],
                 mAP_device_accumulate=evaluate_device()["mAP@[0.5:0.95]"])
    result["evaluate"][f"{n_images}_images"] = group
    for n_images, d, g, labels in ((64, 100, 20, 20), (1000, 100, 20, 80), (5000, 100, 20, 80)):
        rng = np.random.default_rng([n_images, labels])
        rec = coco.Records(n_images * d, labels, dev, gt_capacity=n_images * g)
        for i in range(n_images):
            rec.update(*coco.scene(rng, d, g, labels, image_id=i))

        def device_path():
            rec.accumulate()
            rec.stats()
            return rec.result()

        def host_path():
            return coco.summarize(coco.accumulate(rec.to_host(), labels))

        acc, got, want = rec.accumulate(), device_path(), coco.accumulate(rec.to_host(), labels)
        group = measure({"device": device_path})
        group["host_path"] = wall_ms(host_path)
        group.update(images=n_images, rows=n_images * d, ground_truths=n_images * g, labels=labels, mAP=got["mAP@[0.5:0.95]"],
                     speedup=group["host_path"]["ms"] / group["device"]["ms"],
                     equals_host_path=bool(np.array_equal(acc["precision"].cpu().numpy(), want["precision"])
                                           and np.array_equal(acc["recall"].cpu().numpy(), want["recall"])
                                           and np.max(np.abs(got["stats"] - coco.summarize(want)["stats"])) <= 1e-10))
        result["accumulate"][f"{n_images}_{d}_{g}_{labels}"] = group
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
