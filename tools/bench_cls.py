#!/usr/bin/env python
"""Time the classification-score path (edtr_amd/cls.py) on the device and write profiles/cls_timing.json:

  update      `Scores.update` at B = 32, C = 200 with 512 x 7 x 7 features and at B = 256, C = 1000 without, inputs resident on the
              device (the record is rewound by zeroing its two offsets on the device, inside the timed call); beside it torch's own
              chain on the same device and inputs: topk -> eq -> sum per k, and l1_loss(reduction='none').mean(dim=(1, 2, 3)).
              Torch's chain leaves its counts on the device as well, so neither side pays a copy.
  window      `cls.window` with both flips and the transpose on a 512 x 512 x 3 crop of a 600 x 600 image; beside it
              `labels.window` (no transpose) on the same crop and torch's flip + transpose + contiguous

ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case with the cases of a
group taking turns; the median, the fastest and the slowest window are kept (tools/bench_labels.py's method), wrapper included.
Recorded with the kernel source hash, not gated: no ratio is required of this path — what it delivers is a fixed order and no host
sync.  Commit the file only after this has run on the device.

    python tools/bench_cls.py [--out profiles/cls_timing.json]
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

from edtr_amd import cls, labels as seg_labels  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from bench_boxes import measure  # noqa: E402
from bench_labels import REPEATS, WARMUP, WINDOW_S  # noqa: E402

TOPK = (1, 5)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case; ms = the median window per call, ms_min / ms_max the spread; inputs resident on the device, "
                        "the Python wrapper included on both sides; torch_chain: topk -> eq -> sum per k (and l1_loss(...).mean) on the "
                        "same device, results left there",
              "update": {}, "window": {}}
    for B, C, feat_shape in ((32, 200, (512, 7, 7)), (256, 1000, None)):
        rng = np.random.default_rng([B, C])
        logits = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32)).to(dev)
        lab = torch.from_numpy(rng.integers(0, C, B)).to(dev)
        feats = (None, None)
        if feat_shape is not None:
            feats = tuple(torch.from_numpy(rng.standard_normal((B,) + feat_shape).astype(np.float32)).to(dev) for _ in range(2))
        scores = cls.Scores(B, TOPK, max(TOPK), dev, batch_capacity=1)

        def update():
            scores.offsets.zero_()
            scores.update(logits, lab, *feats)

        def torch_chain():
            pred = logits.topk(max(TOPK), 1, True, True)[1].t()
            correct = pred.eq(lab[None])
            out = [correct[:k].flatten().sum(dtype=torch.float32) * (100.0 / B) for k in TOPK]
            if feats[0] is not None:
                out.append(torch.nn.functional.l1_loss(feats[0], feats[1], reduction="none").mean(dim=(1, 2, 3)))
            return out

        update()
        got, ref = scores.to_host(), torch_chain()
        group = measure({"launches": update, "torch_chain": torch_chain})
        group.update(batch=B, classes=C, features=list(feat_shape) if feat_shape else None,
                     correct=[int(v) for v in got["correct"][0]],
                     equals_torch_counts=bool(all(float(cls.batch_accuracy(got["correct"][0, t], np.array(B))) == float(ref[t]) for t in range(len(TOPK)))))
        if feat_shape is not None:
            group["fd_max_abs_diff_to_torch"] = float(np.abs(got["fd"] - ref[-1].cpu().numpy()).max())
        result["update"][f"B{B}_C{C}" + ("_fd" if feat_shape else "")] = group
    src = torch.from_numpy(np.random.default_rng(512).integers(0, 256, (600, 600, 3), dtype=np.uint8)).to(dev)
    crop, origin = (512, 512), (44, 44)

    def torch_chain():
        return src[origin[0]:origin[0] + crop[0], origin[1]:origin[1] + crop[1]].flip(0, 1).transpose(0, 1).contiguous()

    same = bool(torch.equal(cls.window(src, crop, origin, True, True, True), torch_chain()))
    group = measure({"transpose": lambda: cls.window(src, crop, origin, True, True, True),
                     "no_transpose": lambda: cls.window(src, crop, origin, True, True, False),
                     "labels_window": lambda: seg_labels.window(src, crop, origin, True, True),
                     "torch_chain": torch_chain})
    group.update(source=[600, 600, 3], crop=list(crop), equals_torch=same)
    result["window"]["512x512x3"] = group
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
