#!/usr/bin/env python
"""Time the detector's input transform (edtr_amd/detinput.py `transform`, one launch) on the device beside torch's own chain on the
same device, and write profiles/det_transform_timing.json.

The chain is what the reference's `GeneralizedRCNNTransform.forward` runs, image by image: `(x - mean) / std`,
`F.interpolate(scale_factor=, mode="bilinear", recompute_scale_factor=True)` with the scale formed as the reference forms it, then
`new_full` and one `copy_` per image.  Its mean and std are resident tensors (the reference uploads them on every call; that is not
charged).  Three shapes, fp32:

  one      one 3 x 512 x 512 image -> 800 x 800 (the detection test loop's shape)
  eight    eight of them -> 8 x 3 x 800 x 800
  ragged   375 x 500, 500 x 375, 333 x 500 and 512 x 512 -> 4 x 3 x 1088 x 1216

Before anything is timed both sides' outputs are compared: equal extents, values within 2e-4 (torch's device kernel contracts the
source coordinate; `tests/test_det_transform_cpu.py` holds the rule to the reference).  ms per call from device events around windows
of at least 0.2 s of back-to-back calls, five windows per case, the two sides taking turns (tools/bench_boxes.py's method); inputs
resident; the wrapper, its allocation of the batch and the descriptor upload are inside.  `ratio` = launch / chain, medians.
`kernel_only` replays one pre-built launch record into one batch (no wrapper): the kernel's own time and its rate over the bytes the
rule needs (every source byte once, every batch byte once).
Recorded with the kernel source hash, not gated.  Commit the file only after this has run on the device.

    python tools/bench_det_transform.py [--out profiles/det_transform_timing.json]
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

from edtr_amd import detinput, ops  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from bench_boxes import measure  # noqa: E402
from bench_labels import REPEATS, WARMUP, WINDOW_S  # noqa: E402

MIN_SIZE, MAX_SIZE, SIZE_DIVISIBLE = 800, 1333, 32
SHAPES = {"one": [(512, 512)], "eight": [(512, 512)] * 8, "ragged": [(375, 500), (500, 375), (333, 500), (512, 512)]}


def torch_chain(images, mean, std):
    resized = []
    for image in images:
        x = (image - mean[:, None, None]) / std[:, None, None]
        im_shape = torch.tensor(image.shape[-2:])
        scale = min(MIN_SIZE / min(im_shape), MAX_SIZE / max(im_shape))
        resized.append(torch.nn.functional.interpolate(x[None], scale_factor=scale, mode="bilinear", recompute_scale_factor=True,
                                                       align_corners=False)[0])
    H, W = detinput.batch_extent([r.shape[-2:] for r in resized], SIZE_DIVISIBLE)
    batch = resized[0].new_full((len(resized), resized[0].shape[0], H, W), 0)
    for i, r in enumerate(resized):
        batch[i, :, :r.shape[1], :r.shape[2]].copy_(r)
    return batch, [tuple(r.shape[-2:]) for r in resized]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_transform_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case, the launch and torch's chain taking turns; ms = the median window per call, ms_min / ms_max the "
                        "spread; inputs resident on the device, the wrapper, its batch allocation and the descriptor upload included; "
                        "ratio = launch / chain"}
    mean, std = torch.from_numpy(detinput.IMAGENET_MEAN).to(dev), torch.from_numpy(detinput.IMAGENET_STD).to(dev)
    rng = np.random.default_rng(2030)
    for name, shapes in SHAPES.items():
        images = [torch.from_numpy(rng.uniform(0, 1, (3, h, w)).astype(np.float32)).to(dev) for h, w in shapes]
        got, sizes, _ = detinput.transform(images, MIN_SIZE, MAX_SIZE, size_divisible=SIZE_DIVISIBLE)
        want, want_sizes = torch_chain(images, mean, std)
        assert sizes == want_sizes and got.shape == want.shape, (sizes, want_sizes)
        diff = float((got - want).abs().max())
        assert diff <= 2e-4, diff
        rec = detinput.transform_record(images, MIN_SIZE, MAX_SIZE, size_divisible=SIZE_DIVISIBLE)[0]
        group = measure({"launch": lambda: detinput.transform(images, MIN_SIZE, MAX_SIZE, size_divisible=SIZE_DIVISIBLE),
                         "torch_chain": lambda: torch_chain(images, mean, std),
                         "kernel_only": lambda: ops.launch(rec)})
        read, written = sum(12 * h * w for h, w in shapes), got.numel() * 4
        group.update(images=len(shapes), shapes=[list(s) for s in shapes], image_sizes=[list(s) for s in sizes], batch=list(got.shape),
                     max_abs_diff=diff, bytes_read=read, bytes_written=written, ratio=group["launch"]["ms"] / group["torch_chain"]["ms"],
                     kernel_gb_per_s=(read + written) / group["kernel_only"]["ms"] * 1e-6)
        result[name] = group
        print(f"{name}: launch {group['launch']['ms']:.4f} ms, torch chain {group['torch_chain']['ms']:.4f} ms, ratio {group['ratio']:.3f}; "
              f"the kernel alone {group['kernel_only']['ms']:.4f} ms, {group['kernel_gb_per_s']:.0f} GB/s", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
