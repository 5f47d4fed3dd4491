#!/usr/bin/env python
"""Time the label-map launches (edtr_amd/labels.py) on the device and write profiles/labels_timing.json:

  confusion        edtr_seg_confusion at 8 x 21 x 512 x 512, fp32 and fp16 logits (smooth; fp32 also white noise), with and without the
                   argmax written, beside torch's own argmax -> mask -> n t + p -> bincount chain on the same device and the same
                   tensors (whether the two matrices are equal is recorded)
                   and the same launch under grid caps of 1, 2, 4 and 8 workgroups per compute unit (`max_blocks`)
  resize_nearest   a 1024 x 1024 label map and image -> 512 x 512
  window           a 560 x 746 label map and image -> the 512 x 512 centre crop, flipped
  colorize         8 x 512 x 512 labels -> RGB

ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case with the cases of a
group taking turns (the launch and torch's chain alternate); the median, the fastest and the slowest window are kept.  Inputs are
resident on the device; the wrappers' allocations are inside.  GB/s = the bytes the algorithm has to move (computed here from the
shapes) over the median: a call rate, not a kernel's share of peak.  Recorded with the kernel source hash, not gated.  Commit the
file only after this has run on the device.

    python tools/bench_labels.py [--out profiles/labels_timing.json]
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

from edtr_amd import labels  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402

WARMUP = 5
WINDOW_S = 0.2          # a timed window lasts at least this long: shorter ones measure the clock and the scheduler
REPEATS = 5             # windows per case, the cases of one group taken in turn
B, N, H, W = 8, 21, 512, 512


def window_ms(fn, iters: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def measure(fns: dict, nbytes: dict) -> dict:
    """Every case of ``fns`` warmed up, its call count chosen so that a window lasts WINDOW_S, then REPEATS rounds in which the cases
    take turns (so that a drift of the device hits all alike).  Per case: the median window, the fastest and the slowest."""
    iters = {}
    for name, fn in fns.items():
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(50, int(np.ceil(WINDOW_S * 1e3 / window_ms(fn, 50))))
    samples = {name: [] for name in fns}
    for _ in range(REPEATS):
        for name, fn in fns.items():
            samples[name].append(window_ms(fn, iters[name]))
    out = {}
    for name, v in samples.items():
        med = float(np.median(v))
        out[name] = {"ms": med, "ms_min": float(min(v)), "ms_max": float(max(v)), "calls_per_window": iters[name], "windows": REPEATS,
                     "bytes": nbytes[name], "gb_per_s": nbytes[name] / (med * 1e-3) / 1e9, "window_ms": [float(x) for x in v]}
    return out


def torch_confusion(logits, target, n):
    """calculate_mat(target, logits.argmax(1), n) as torch runs it: an int64 index per pixel, a mask, a bincount"""
    pred = logits.argmax(1).flatten()
    t = target.flatten().long()
    k = (t >= 0) & (t < n)
    return torch.bincount(n * t[k] + pred[k], minlength=n * n).reshape(n, n)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labels_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    target = torch.randint(0, N, (B, H, W), generator=gen, dtype=torch.uint8)
    target[:, :8] = 255
    target = target.to(dev)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    result = {"compute_units": cus, "workload": f"logits ({B}, {N}, {H}, {W}); label maps and images of 512 x 512", "device": torch.cuda.get_device_name(0),
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case, the cases of one group taking turns; ms = the median window per call, ms_min / ms_max the spread; "
                        "inputs resident on the device, the wrappers' allocations included; gb_per_s = algorithmic bytes / ms "
                        "(a call rate, not a kernel's share of peak)",
              "confusion": {}}
    for name, dtype in (("fp32", torch.float32), ("fp16", torch.float16)):
        # smooth logits (a low-resolution field, upsampled) so that neighbouring pixels mostly share a bin, as a real prediction's do;
        # for fp32 also white noise, where a lane merges nothing and a wave's LDS atomics spread over the bins
        coarse = torch.randn((B, N, H // 16, W // 16), generator=gen)
        logits = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear").to(dtype).to(dev).contiguous()
        equal = bool(torch.equal(labels.confusion(logits, target, N), torch_confusion(logits, target, N)))
        mat = torch.zeros((N, N), dtype=torch.int64, device=dev)
        nbytes = float(logits.numel() * logits.element_size() + target.numel())
        fns = {"launch": lambda: labels.confusion(logits, target, N, mat=mat),
               "launch_with_pred": lambda: labels.confusion(logits, target, N, mat=mat, return_pred=True),
               "torch_chain": lambda: torch_confusion(logits, target, N)}
        sizes = {"launch": nbytes, "launch_with_pred": nbytes + target.numel(), "torch_chain": nbytes}
        if dtype == torch.float32:
            noisy = torch.randn((B, N, H, W), generator=gen).to(dev)
            fns["launch_white_noise_logits"] = lambda: labels.confusion(noisy, target, N, mat=mat)
            sizes["launch_white_noise_logits"] = nbytes
        group = measure(fns, sizes)
        ratios = [t / o for t, o in zip(group["torch_chain"]["window_ms"], group["launch"]["window_ms"])]
        group["equals_torch_chain"] = equal
        group["torch_over_launch"] = {"median": float(np.median(ratios)), "min": float(min(ratios)), "max": float(max(ratios))}
        # the grid cap through max_blocks, as multiples of the device's compute units (0 = the default the library ships)
        caps = {"default": 0, **{f"{m}_per_cu": m * cus for m in (1, 2, 4, 8)}}
        sweep = measure({k: (lambda cap=cap: labels.confusion(logits, target, N, mat=mat, max_blocks=cap)) for k, cap in caps.items()},
                        {k: nbytes for k in caps})
        group["max_blocks_sweep"] = {k: {"max_blocks": caps[k], **{a: v[a] for a in ("ms", "ms_min", "ms_max")}} for k, v in sweep.items()}
        result["confusion"][name] = group
        del logits
    rng = np.random.default_rng(1)
    fns, sizes = {}, {}
    for ch, what in ((1, "mask"), (3, "image")):
        big = torch.from_numpy(rng.integers(0, 255, (1024, 1024, ch), dtype=np.uint8)).to(dev)
        mid = torch.from_numpy(rng.integers(0, 255, (560, 746, ch), dtype=np.uint8)).to(dev)
        fns[f"resize_nearest_{what}"] = lambda big=big: labels.resize_nearest(big, (512, 512))
        fns[f"window_{what}"] = lambda mid=mid: labels.window(mid, (512, 512), (24, 117), True, False, 255)
        sizes[f"resize_nearest_{what}"] = sizes[f"window_{what}"] = 2 * 512.0 * 512 * ch
    fns["colorize"], sizes["colorize"] = (lambda: labels.colorize(target)), 4.0 * target.numel()
    result["gathers"] = measure(fns, sizes)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
