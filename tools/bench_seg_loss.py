#!/usr/bin/env python
"""Time `labels.coarse_cross_entropy` forward + backward (edtr_seg_ce_forward / edtr_seg_ce_backward: the segmentation loss from coarse
logits, no [B, n, H, W] tensor in either direction) on the device beside torch's chain for the same job in the same process on the same
device — `F.interpolate(coarse, size, mode="bilinear")` -> `F.cross_entropy(ignore_index=255)` -> `backward()` — and write
profiles/seg_loss_timing.json:

  8 x 21 x 64 x 64 -> 512 x 512     the reference's training shape
  1 x 21 x 64 x 64 -> 512 x 512     one image

each with fp32 and bf16 logits.  The method is tools/bench_labels.py's: ms per call from device events around windows of at least 0.2 s
of back-to-back calls, five windows per case, the two sides taking turns, the median kept with the fastest and the slowest; inputs
resident, the wrappers' allocations included.  In the same run: the two sides' loss and gradient against each other, the peak of
`torch.cuda.max_memory_allocated` over one call of each side (above what was allocated before it), whether two runs of each side's
backward differ in bits, and the worst error of the device's exp on [-90, 0] and log on [1, 256] against fp64 in fp32 ulps ("ulp":
torch's device kernels, which call the same OCML expf / logf a HIP kernel's expf / logf compile to; tests/seg_loss_cases.py takes
twice these figures).  Recorded with the kernel source hash, not gated.  Commit the file only after this has run on the device.

    python tools/bench_seg_loss.py [--out profiles/seg_loss_timing.json]
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
SHAPES = {"train_8x64x64_to_512x512": (8, (64, 64), (512, 512)), "one_1x64x64_to_512x512": (1, (64, 64), (512, 512))}


def ulp_error(fn, ref, lo: float, hi: float, dev, samples: int = 1 << 22) -> dict:
    """worst |fn(x) - ref(x)| over `samples` evenly spaced fp32 arguments of [lo, hi], in ulps of the fp32 nearest to ref(x)"""
    x = torch.linspace(lo, hi, samples, dtype=torch.float64).float()
    got = fn(x.to(dev)).cpu().double()
    want = ref(x.double())
    ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()).astype(np.float32))).double().clamp_min(2.0 ** -149)
    err = ((got - want).abs() / ulp)
    k = int(err.argmax())
    return {"worst_ulp": float(np.ceil(float(err[k]))), "worst_ulp_exact": float(err[k]), "at": float(x[k]), "samples": samples, "interval": [lo, hi]}


def peak_bytes(call) -> int:
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = call()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - before)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_loss_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    result = {"compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "device": torch.cuda.get_device_name(0),
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS, "classes": N,
              "method": "tools/bench_labels.py's: device events around windows of at least `window_s` seconds of back-to-back calls after "
                        "`warmup` calls; `windows` windows per case, the two sides taking turns; ms = the median window per call, forward + "
                        "backward; inputs resident on the device, the wrappers' allocations included.  launches = labels.coarse_cross_entropy "
                        "and its backward; torch_chain = F.interpolate -> F.cross_entropy(ignore_index=255) -> backward on the same device; "
                        "peak_bytes = torch.cuda.max_memory_allocated over one call above what was allocated before it",
              "ulp": {"expf": ulp_error(torch.exp, torch.exp, -90.0, 0.0, dev), "logf": ulp_error(torch.log, torch.log, 1.0, 256.0, dev)},
              "shapes": {}}
    for key, (B, ihw, size) in SHAPES.items():
        target = torch.randint(0, N, (B,) + size, generator=gen, dtype=torch.uint8)
        target[:, :8] = 255
        target = target.to(dev)
        long_target = target.long()
        base = 4.0 * torch.randn((B, N) + ihw, generator=gen)
        entry = {"coarse": [B, N, *ihw], "size": list(size)}
        for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            coarse = base.to(dtype).to(dev).contiguous().requires_grad_(True)

            def launches(coarse=coarse):
                loss = labels.coarse_cross_entropy(coarse, target)
                return loss, torch.autograd.grad(loss, coarse)[0]

            def torch_chain(coarse=coarse):
                loss = F.cross_entropy(F.interpolate(coarse, size=size, mode="bilinear", align_corners=False).float(), long_target, ignore_index=255)
                return loss, torch.autograd.grad(loss, coarse)[0]

            (la, ga), (la2, ga2), (lb, gb), (lb2, gb2) = launches(), launches(), torch_chain(), torch_chain()
            group = measure({"launches": launches, "torch_chain": torch_chain}, {"launches": 0.0, "torch_chain": 0.0})
            ratios = [p / o for p, o in zip(group["torch_chain"]["window_ms"], group["launches"]["window_ms"])]
            group["torch_over_launches"] = {"median": float(np.median(ratios)), "min": float(min(ratios)), "max": float(max(ratios))}
            group["loss"] = {"launches": la.item(), "torch_chain": lb.item()}
            group["grad_max_abs_difference"] = float((ga.float() - gb.float()).abs().max())
            group["grad_max_abs"] = float(gb.float().abs().max())
            group["two_runs_differ_in_bits"] = {"launches": not (torch.equal(ga, ga2) and torch.equal(la, la2)),
                                                "torch_chain": not (torch.equal(gb, gb2) and torch.equal(lb, lb2))}
            group["peak_bytes"] = {"launches": peak_bytes(launches), "torch_chain": peak_bytes(torch_chain)}
            entry[name] = group
        result["shapes"][key] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps({"ulp": {k: v["worst_ulp_exact"] for k, v in result["ulp"].items()},
                      **{k: {d: {"launches_ms": v[d]["launches"]["ms"], "torch_ms": v[d]["torch_chain"]["ms"], "peak": v[d]["peak_bytes"],
                                 "differ": v[d]["two_runs_differ_in_bits"], "grad_diff": v[d]["grad_max_abs_difference"]} for d in ("fp32", "bf16")}
                         for k, v in result["shapes"].items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
