#!/usr/bin/env python
"""Time RoIAlign's backward (edtr_amd/rois.py `roi_align_backward`) on the device and write profiles/roi_backward_timing.json.

The training shape of the reference's detector: 2 images of 800 x 1344, the four pooled levels from 200 x 336 down, 256 channels,
2 x 512 rois of detector-like sizes (tools/bench_proposals.py `roi_inputs`), 7 x 7 bins of 2 x 2 samples, fp32 and bf16 gradients out.
Three cases take turns:
  call          `rois.roi_align_backward`: the wrapper's allocations (outputs, workspace), the flat roi table and the launch pair;
  launch_pair   the pre-built record replayed alone (`ops.make_roi_align_backward`): the pre-pass and the gather;
  torch_grid_sample_composite_backward
                the backward of the only counterpart torch has on this device, the `F.grid_sample` composite that
                tools/bench_proposals.py times forward (zero padding instead of roi_align's border rule: a counterpart in cost, not
                in bits), by `torch.autograd.grad` on a graph built once.  Per image and level it expands the feature map over the
                rois, so its backward materialises one map per roi before it sums them, and it scatters with float atomics.
In the same run: two calls of the launch give equal bits (asserted); whether two backward passes of the composite do is recorded; and
over the rois whose samples all lie inside their map, where the two rules coincide, the largest difference between the two gradients
relative to the largest element is recorded.

ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case, the cases taking turns;
the median, the fastest and the slowest window are kept (tools/bench_boxes.py's method).  Recorded with the kernel source hash, not
gated.  Commit the file only after this has run on the device.

    python tools/bench_roi_backward.py [--out profiles/roi_backward_timing.json]
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

from edtr_amd import ops, rois  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from bench_boxes import measure  # noqa: E402
from bench_labels import REPEATS, WARMUP, WINDOW_S  # noqa: E402
from bench_proposals import GRIDS, PADDED, roi_inputs, torch_roi_composite  # noqa: E402

N, C, PER_IMAGE, P, S = 2, 256, 512, 7, 2


def composite(feats, per_image, scales, k_min, k_max):
    return torch.cat([torch_roi_composite([f[n:n + 1] for f in feats], bx, scales, k_min, k_max, P, S) for n, bx in enumerate(per_image)])


def inside(bx, scales, k_min, k_max, shapes):
    """the rois whose every sample lies in [0, W - 1] x [0, H - 1] of their level: there roi_align and grid_sample interpolate alike"""
    lv = rois.roi_levels_reference(bx, k_min, k_max)
    s = np.array(scales)[lv][:, None]
    b = bx * s
    H, W = np.array([sh[2] for sh in shapes])[lv], np.array([sh[3] for sh in shapes])[lv]
    return (b[:, 0] >= 0.5) & (b[:, 1] >= 0.5) & (b[:, 2] <= W - 1.5) & (b[:, 3] <= H - 1.5)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_backward_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case, the cases of one group taking turns; ms = the median window per call, ms_min / ms_max the spread; "
                        "inputs resident on the device",
              "images": N, "channels": C, "rois_per_image": PER_IMAGE, "output_size": P, "sampling_ratio": S}
    image_sizes = [PADDED] * N
    shapes = [(N, C, h, w) for h, w in GRIDS[:4]]
    flat = roi_inputs(dev, N * PER_IMAGE)
    per_image = [flat[n * PER_IMAGE:(n + 1) * PER_IMAGE].contiguous() for n in range(N)]
    scales, k_min, k_max = rois.level_scales([s[-2:] for s in shapes], image_sizes)
    lv = rois.roi_levels_reference(flat.cpu().numpy(), k_min, k_max)
    result["rois_per_level"] = np.bincount(lv, minlength=4).tolist()
    grad = torch.from_numpy(np.random.default_rng(2031).standard_normal((N * PER_IMAGE, C, P, P)).astype(np.float32)).to(dev)
    calm = inside(flat.cpu().numpy(), scales, k_min, k_max, shapes)
    result["rois_inside"] = int(calm.sum())
    calm_grad = grad * torch.from_numpy(calm.astype(np.float32)).to(dev)[:, None, None, None]

    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        feats = [torch.from_numpy(np.random.default_rng(2029).normal(0, 1, s).astype(np.float32)).to(dev).to(dtype).requires_grad_() for s in shapes]
        pooled = composite(feats, per_image, scales, k_min, k_max)

        def composite_backward(g=grad):
            return torch.autograd.grad(pooled, feats, g, retain_graph=True)

        first = rois.roi_align_backward(grad, shapes, per_image, image_sizes, P, S, dtype=dtype)
        second = rois.roi_align_backward(grad, shapes, per_image, image_sizes, P, S, dtype=dtype)
        assert all(torch.equal(a.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               b.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)) for a, b in zip(first, second)), "two calls differ"
        ca, cb = composite_backward(), composite_backward()
        mine, theirs = rois.roi_align_backward(calm_grad, shapes, per_image, image_sizes, P, S, dtype=dtype), composite_backward(calm_grad)
        peak = max(float(t.float().abs().max()) for t in theirs)
        flat_rois, batch = rois._flat_rois(per_image, N, dev)
        outs = [torch.empty(s, dtype=dtype, device=dev) for s in shapes]
        workspace = torch.empty(ops.roi_align_backward_workspace(N, N * PER_IMAGE, P, S), dtype=torch.uint8, device=dev)
        rec = ops.make_roi_align_backward(grad=grad, grads_out=outs, scales=scales, rois=flat_rois, batch_index=batch, workspace=workspace,
                                          sampling_ratio=S, k_min=k_min, k_max=k_max, canonical_scale=224.0, canonical_level=4.0)
        ops.launch(rec)
        assert all(torch.equal(a.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               b.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)) for a, b in zip(first, outs)), "the record differs"
        group = measure({"call": lambda: rois.roi_align_backward(grad, shapes, per_image, image_sizes, P, S, dtype=dtype),
                         "launch_pair": lambda: ops.launch(rec),
                         "torch_grid_sample_composite_backward": composite_backward})
        group.update(two_calls_equal_bits=True,
                     composite_two_backwards_equal_bits=bool(all(torch.equal(a, b) for a, b in zip(ca, cb))),
                     max_difference_inside_over_peak=max(float((a.float() - b.float()).abs().max()) for a, b in zip(mine, theirs)) / peak,
                     gradient_bytes=int(grad.numel() * 4), output_bytes=int(sum(o.numel() * o.element_size() for o in outs)),
                     workspace_bytes=int(workspace.numel()))
        result[name] = group
        del pooled, feats

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
