#!/usr/bin/env python
"""Time `labels.coarse_confusion` (edtr_seg_confusion_coarse: coarse logits -> confusion matrix in one launch) on the device beside
what the project offered for the same job before it, in the same process on the same device — `torch.nn.functional.interpolate` of
the coarse logits to the mask's extent on the device, then `labels.confusion` — and write profiles/labels_coarse_timing.json:

  1 x 21 x 64 x 64 -> 512 x 512     the reference's test loop (batch 1)
  8 x 21 x 64 x 64 -> 512 x 512     the shape tools/bench_labels.py times `confusion` at
  1 x 21 x 47 x 63 -> 375 x 500     a VOC extent, non-integer ratio, rows that are no multiple of a tile

each with fp32 and bf16 logits, and for the batch of 8 in fp32 the launch under grid caps of 1, 2, 4 and 8 workgroups per compute
unit.  The method is tools/bench_labels.py's: ms per call from device events around windows of at least 0.2 s of back-to-back calls,
five windows per case, the two paths taking turns, the median kept with the fastest and the slowest; inputs resident, the wrappers'
allocations included.  Whether the two paths give the same matrix is recorded (bf16 may differ in a few pixels: torch's device
kernel blends in its own operation order).  Recorded with the kernel source hash, not gated.  Commit the file only after this has
run on the device.

    python tools/bench_coarse_confusion.py [--out profiles/labels_coarse_timing.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_labels import REPEATS, WARMUP, WINDOW_S, measure  # noqa: E402
from edtr_amd import labels  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402

N = 21
SHAPES = {"test_loop_1x64x64_to_512x512": (1, (64, 64), (512, 512)),
          "batch_8x64x64_to_512x512": (8, (64, 64), (512, 512)),
          "voc_1x47x63_to_375x500": (1, (47, 63), (375, 500))}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labels_coarse_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    result = {"compute_units": cus, "device": torch.cuda.get_device_name(0), "source_hash": source_hash(), "warmup": WARMUP,
              "window_s": WINDOW_S, "windows": REPEATS, "classes": N,
              "method": "tools/bench_labels.py's: device events around windows of at least `window_s` seconds of back-to-back calls after "
                        "`warmup` calls; `windows` windows per case, the two paths taking turns; ms = the median window per call; inputs "
                        "resident on the device, the wrappers' allocations included.  one_launch = labels.coarse_confusion; "
                        "interpolate_then_confusion = F.interpolate(coarse, size, mode='bilinear') on the device, then labels.confusion; "
                        "bytes = what each path has to move, computed from the shapes",
              "shapes": {}}
    for key, (B, ihw, size) in SHAPES.items():
        target = torch.randint(0, N, (B,) + size, generator=gen, dtype=torch.uint8)
        target[:, :8] = 255
        target = target.to(dev)
        base = torch.randn((B, N) + ihw, generator=gen)
        entry = {"coarse": [B, N, *ihw], "size": list(size)}
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            coarse = base.to(dtype).to(dev).contiguous()
            mat = torch.zeros((N, N), dtype=torch.int64, device=dev)

            def one_launch(coarse=coarse, mat=mat):
                return labels.coarse_confusion(coarse, target, N, mat=mat)

            def parent_path(coarse=coarse, mat=mat):
                return labels.confusion(F.interpolate(coarse, size=size, mode="bilinear", align_corners=False), target, N, mat=mat)

            a, b = labels.coarse_confusion(coarse, target, N), labels.confusion(F.interpolate(coarse, size=size, mode="bilinear"), target, N)
            full = float(B * N * size[0] * size[1] * coarse.element_size())
            small = float(coarse.numel() * coarse.element_size() + target.numel())
            group = measure({"one_launch": one_launch, "interpolate_then_confusion": parent_path},
                            {"one_launch": small, "interpolate_then_confusion": small + 2 * full})
            ratios = [p / o for p, o in zip(group["interpolate_then_confusion"]["window_ms"], group["one_launch"]["window_ms"])]
            group["same_matrix"] = bool(torch.equal(a, b))
            group["pixels_counted_elsewhere"] = int((a - b).abs().sum().item()) // 2
            group["parent_over_one_launch"] = {"median": float(np.median(ratios)), "min": float(min(ratios)), "max": float(max(ratios))}
            if key.startswith("batch") and dtype == torch.float32:
                caps = {"default": 0, **{f"{m}_per_cu": m * cus for m in (1, 2, 4, 8)}}
                sweep = measure({k: (lambda cap=cap: labels.coarse_confusion(coarse, target, N, mat=mat, max_blocks=cap)) for k, cap in caps.items()},
                                {k: small for k in caps})
                group["max_blocks_sweep"] = {k: {"max_blocks": caps[k], **{q: v[q] for q in ("ms", "ms_min", "ms_max")}} for k, v in sweep.items()}
            entry[name] = group
        result["shapes"][key] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps({k: {d: {"one_launch_ms": v[d]["one_launch"]["ms"], "parent_ms": v[d]["interpolate_then_confusion"]["ms"],
                              "ratio": v[d]["parent_over_one_launch"]["median"]} for d in ("fp32", "bf16")}
                      for k, v in result["shapes"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
