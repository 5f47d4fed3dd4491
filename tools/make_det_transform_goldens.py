#!/usr/bin/env python
"""Write tests/golden/det_transform.npz for tests/test_det_transform_cpu.py.

The REFERENCE's own `GeneralizedRCNNTransform` (model/faster_rcnn.py:2266-2435) in eval mode, on the CPU, on seeded inputs:

  * the extents its `_resize_image_and_masks` produces for 2000 seeded (h, w, min_size, max_size) rows — the PASCAL / COCO-like sizes
    375 x 500, 500 x 375, 333 x 500, 480 x 640, 427 x 640 and 512 x 512 at 800 / 1333 first, then random shapes in 8 .. 200 at three
    settings (a one-channel image of zeros is resized; only its shape is recorded);
  * the full `forward` of four ragged sets: the batch, `image_sizes` and the resized target boxes;
  * per set `ref_err`, the reference's own max abs distance from itself run in fp64 on the same inputs with the same constants
    (mean and std are handed over as the doubles of their fp32 values, so that both runs normalise with the same numbers).

The reference calls `torchvision._is_tracing()`; the stand-in module gets that attribute here.  Only arrays go into the file, and
the archive is written with fixed time stamps: the same inputs give the same bytes.

    python tools/make_det_transform_goldens.py [--out tests/golden/det_transform.npz]       (needs the reference tree; see tools/ref_import.py)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_boxes_goldens import install_detection_stubs  # noqa: E402
from make_labels_goldens import write_npz  # noqa: E402

SEED = 20281
F = np.float32
NAMED = [(375, 500), (500, 375), (333, 500), (480, 640), (427, 640), (512, 512)]
SETTINGS = [(64, 100), (96, 160), (50, 333)]           # (min_size, max_size) of the random rows
ROWS = 2000
MEAN, STD = [0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25]
# (tag, image shapes (h, w), channels, kwargs of the transform)
SETS = [
    ("ragged", [(53, 47), (40, 167), (61, 163), (64, 64)], 3, dict(min_size=64, max_size=100, size_divisible=32)),
    ("odd", [(61, 163), (17, 9)], 3, dict(min_size=64, max_size=100, size_divisible=1)),
    ("fixed", [(33, 27), (20, 41)], 3, dict(min_size=64, max_size=100, size_divisible=32, fixed_size=(48, 40))),
    ("four", [(25, 21), (32, 32)], 4, dict(min_size=(16, 32), max_size=50, size_divisible=16)),
]


def extent_rows(frcnn) -> np.ndarray:
    rng = np.random.default_rng([SEED, ROWS])
    rows = [(h, w, 800, 1333) for h, w in NAMED]
    while len(rows) < ROWS:
        lo, hi = SETTINGS[len(rows) % len(SETTINGS)]
        rows.append((int(rng.integers(8, 201)), int(rng.integers(8, 201)), lo, hi))
    out = []
    with torch.no_grad():
        for h, w, lo, hi in rows:
            image, _ = frcnn._resize_image_and_masks(torch.zeros(1, h, w), lo, hi)
            out.append((h, w, lo, hi, image.shape[-2], image.shape[-1]))
    return np.array(out, dtype=np.int32)


def boxes_in(rng, h, w, n=5) -> np.ndarray:
    x1, y1 = rng.uniform(0, w * 0.7, n), rng.uniform(0, h * 0.7, n)
    return np.stack([x1, y1, x1 + rng.uniform(1, w * 0.3, n), y1 + rng.uniform(1, h * 0.3, n)], axis=1).astype(F)


def run_set(frcnn, shapes, C, kw, rng):
    mean, std = [float(F(v)) for v in MEAN[:C]], [float(F(v)) for v in STD[:C]]
    t = frcnn.GeneralizedRCNNTransform(kw["min_size"], kw["max_size"], mean, std, kw["size_divisible"], kw.get("fixed_size")).eval()
    images = [rng.uniform(0, 1, (C, h, w)).astype(F) for h, w in shapes]
    boxes = [boxes_in(rng, h, w) for h, w in shapes]
    with torch.no_grad():
        out, targets = t([torch.from_numpy(v) for v in images], [{"boxes": torch.from_numpy(b)} for b in boxes])
        out64, _ = t([torch.from_numpy(v).double() for v in images])
    assert out.tensors.dtype == torch.float32 and out64.tensors.dtype == torch.float64 and out.image_sizes == out64.image_sizes
    ref_err = float((out.tensors.double() - out64.tensors).abs().max())
    return images, boxes, out.tensors.numpy(), np.array(out.image_sizes, dtype=np.int32), [t["boxes"].numpy() for t in targets], ref_err


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "det_transform.npz"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    install_detection_stubs()
    sys.modules["torchvision"]._is_tracing = lambda: False
    import importlib
    frcnn = importlib.import_module("model.faster_rcnn")

    out = {"extent_rows": extent_rows(frcnn), "set_tags": np.array([s[0] for s in SETS])}
    print(f"{len(out['extent_rows'])} extent rows; 375 x 500 at 800 / 1333 -> {tuple(out['extent_rows'][0, 4:])}")
    for tag, shapes, C, kw in SETS:
        images, boxes, batch, sizes, resized, ref_err = run_set(frcnn, shapes, C, kw, np.random.default_rng([SEED, len(shapes), C]))
        lo = kw["min_size"]
        out.update({f"{tag}_min_size": np.array(lo if isinstance(lo, tuple) else (lo,), dtype=np.int32), f"{tag}_max_size": np.array(kw["max_size"], dtype=np.int32),
                    f"{tag}_size_divisible": np.array(kw["size_divisible"], dtype=np.int32),
                    f"{tag}_fixed_size": np.array(kw.get("fixed_size", ()), dtype=np.int32), f"{tag}_mean": np.array(MEAN[:C], dtype=F),
                    f"{tag}_std": np.array(STD[:C], dtype=F), f"{tag}_batch": batch, f"{tag}_image_sizes": sizes,
                    f"{tag}_ref_err": np.array(ref_err, dtype=np.float64)})
        for i, (v, b, r) in enumerate(zip(images, boxes, resized)):
            out[f"{tag}_image{i}"], out[f"{tag}_boxes{i}"], out[f"{tag}_resized_boxes{i}"] = v, b, r
        print(f"{tag}: batch {batch.shape}, image_sizes {sizes.tolist()}, ref_err {ref_err:.3e}")
    write_npz(args.out, out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
