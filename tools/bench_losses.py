#!/usr/bin/env python
"""Time the training losses of `edtr_amd.losses` forward + backward (edtr_l1_forward / edtr_l1_backward: the weighted mean-L1 over a list
of feature pairs; edtr_cls_ce_forward / edtr_cls_ce_backward: the classifier's cross-entropy) on the device beside torch's own chain for
the same job in the same process on the same device — `F.l1_loss(a, b) * w` summed over the pairs, then `backward()`; `F.cross_entropy`,
then `backward()` — and write profiles/losses_timing.json:

  det_hlf        the detector's HLF term: four fp32 pairs, two of 2 x 256 x 200 x 336 and two of 2 x 256 x 100 x 168, weights 0.5
                 (main/det/train_edtr.py:194-197 at 2 images of 800 x 1344); the operands are larger than the Infinity Cache
  seg_c5         the segmenter's C5, 8 x 2048 x 64 x 64 (main/seg/train_edtr.py:218), fp32 and bf16
  cls_step       the classifier's step: cross-entropy of 32 x 1000 logits + feature matching of 32 x 512 x 7 x 7 features
                 (main/cls/train_edtr.py:207-213); launch-bound on both sides

The first operand of every pair requires grad, the second does not (the teacher's, or the clean image's, features).  The method is
tools/bench_seg_loss.py's: ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case,
the sides taking turns, the median kept with the fastest and the slowest; inputs resident, the wrappers' allocations included.  Beside
the two chains the L1 shapes time the forward launches and the backward launch on their own, for the byte rate each reaches (forward:
both operands read once; backward: both read once, one gradient written once) against the roughly 6.3 TB/s the device's memory is
known to sustain: reported, not asserted.  In the same run: the two sides' loss and gradient against each other, the peak of
`torch.cuda.max_memory_allocated` over one call of each side, whether two runs of each side differ in bits, and the worst error of the
device's log on [1, 65536] against fp64 in fp32 ulps ("ulp", measured as tools/bench_seg_loss.py does; tests/losses_cases.py takes twice
this figure).  "faster" is said of a shape only where every window ratio is above 1.1, the spread between devices of one kind.
Recorded with the kernel source hash, not gated.  Commit the file only after this has run on the device.

    python tools/bench_losses.py [--out profiles/losses_timing.json]
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
from bench_seg_loss import peak_bytes, ulp_error  # noqa: E402
from edtr_amd import losses  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402

ACHIEVABLE_TB_S = 6.3
L1_SHAPES = {
    "det_hlf_fp32": (torch.float32, [(2, 256, 200, 336), (2, 256, 100, 168), (2, 256, 200, 336), (2, 256, 100, 168)], [0.5, 0.5, 0.5, 0.5]),
    "seg_c5_fp32": (torch.float32, [(8, 2048, 64, 64)], [1.0]),
    "seg_c5_bf16": (torch.bfloat16, [(8, 2048, 64, 64)], [1.0]),
}


def verdict(ratios) -> str:
    if min(ratios) > 1.1:
        return "launches faster"
    if max(ratios) < 1.0 / 1.1:
        return "torch faster"
    return "within the 10 % the devices differ by"


def compare(group, mine, theirs, mine2, theirs2):
    """the values of both sides against each other and each side against its own second run"""
    (la, ga), (lb, gb) = mine, theirs
    ratios = [p / o for p, o in zip(group["torch_chain"]["window_ms"], group["launches"]["window_ms"])]
    group["torch_over_launches"] = {"median": float(np.median(ratios)), "min": float(min(ratios)), "max": float(max(ratios)), "verdict": verdict(ratios)}
    group["loss"] = {"launches": la.item(), "torch_chain": lb.item()}
    group["grad_max_abs_difference"] = max(float((x.float() - y.float()).abs().max()) for x, y in zip(ga, gb))
    group["grad_max_abs"] = max(float(y.float().abs().max()) for y in gb)
    same = lambda p, q: torch.equal(p[0], q[0]) and all(torch.equal(x, y) for x, y in zip(p[1], q[1]))
    group["two_runs_differ_in_bits"] = {"launches": not same(mine, mine2), "torch_chain": not same(theirs, theirs2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    result = {"compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "device": torch.cuda.get_device_name(0),
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS, "achievable_tb_per_s": ACHIEVABLE_TB_S,
              "method": "tools/bench_labels.py's: device events around windows of at least `window_s` seconds of back-to-back calls after "
                        "`warmup` calls; `windows` windows per case, the sides taking turns; ms = the median window per call; inputs resident on "
                        "the device, the wrappers' allocations included.  launches = losses.l1_mean / losses.cross_entropy and their backward "
                        "through autograd; torch_chain = F.l1_loss * w summed / F.cross_entropy -> backward on the same device; forward_only / "
                        "backward_only = the launches on their own, bytes = operands read once (+ one gradient written once); peak_bytes = "
                        "torch.cuda.max_memory_allocated over one call above what was allocated before it; the first operand of a pair "
                        "requires grad, the second does not",
              "ulp": {"logf": ulp_error(torch.log, torch.log, 1.0, 65536.0, dev)},
              "shapes": {}}
    for key, (dtype, shapes, weights) in L1_SHAPES.items():
        pairs = [(torch.randn(s, generator=gen).to(dtype).to(dev).requires_grad_(True), torch.randn(s, generator=gen).to(dtype).to(dev)) for s in shapes]
        firsts = [a for a, _ in pairs]
        plain = [(a.detach(), b) for a, b in pairs]
        elems = sum(a.numel() for a in firsts)
        size = firsts[0].element_size()
        one = torch.ones((), device=dev)

        def launches():
            loss = losses.l1_mean(pairs, weights)
            return loss, torch.autograd.grad(loss, firsts)

        def torch_chain():
            loss = sum(F.l1_loss(a.float(), b.float(), reduction="mean") * w for (a, b), w in zip(pairs, weights))
            return loss, torch.autograd.grad(loss, firsts)

        def forward_only():
            return losses.l1_mean(plain, weights)

        def backward_only():
            return losses.l1_mean_backward(plain, weights, one)

        mine, mine2, theirs, theirs2 = launches(), launches(), torch_chain(), torch_chain()
        group = measure({"launches": launches, "torch_chain": torch_chain, "forward_only": forward_only, "backward_only": backward_only},
                        {"launches": 5.0 * elems * size, "torch_chain": 0.0, "forward_only": 2.0 * elems * size, "backward_only": 3.0 * elems * size})
        compare(group, mine, theirs, mine2, theirs2)
        group["fraction_of_achievable"] = {k: group[k]["gb_per_s"] / (ACHIEVABLE_TB_S * 1e3) for k in ("launches", "forward_only", "backward_only")}
        del mine, mine2, theirs, theirs2
        group["peak_bytes"] = {"launches": peak_bytes(launches), "torch_chain": peak_bytes(torch_chain)}
        group["pairs"], group["weights"], group["dtype"], group["operand_bytes"] = [list(s) for s in shapes], weights, str(dtype), 2 * elems * size
        result["shapes"][key] = group
        del pairs, firsts, plain
        torch.cuda.empty_cache()

    # the classifier's step: the cross-entropy of the logits and the feature matching of the features, one backward for both
    logits = (4.0 * torch.randn((32, 1000), generator=gen)).to(dev).requires_grad_(True)
    labels = torch.randint(0, 1000, (32,), generator=gen).to(dev)
    feat = torch.randn((32, 512, 7, 7), generator=gen).to(dev).requires_grad_(True)
    feat_teacher = torch.randn((32, 512, 7, 7), generator=gen).to(dev)

    def launches():
        loss = losses.cross_entropy(logits, labels) + losses.l1_mean([(feat, feat_teacher)])
        return loss, torch.autograd.grad(loss, [logits, feat])

    def torch_chain():
        loss = F.cross_entropy(logits, labels, reduction="mean", label_smoothing=0.0) + F.l1_loss(feat, feat_teacher, reduction="mean")
        return loss, torch.autograd.grad(loss, [logits, feat])

    mine, mine2, theirs, theirs2 = launches(), launches(), torch_chain(), torch_chain()
    group = measure({"launches": launches, "torch_chain": torch_chain}, {"launches": 0.0, "torch_chain": 0.0})
    compare(group, mine, theirs, mine2, theirs2)
    group["peak_bytes"] = {"launches": peak_bytes(launches), "torch_chain": peak_bytes(torch_chain)}
    group["logits"], group["features"] = [32, 1000], [32, 512, 7, 7]
    result["shapes"]["cls_step_fp32"] = group

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps({"ulp_logf": result["ulp"]["logf"]["worst_ulp_exact"],
                      **{k: {"launches_ms": v["launches"]["ms"], "torch_ms": v["torch_chain"]["ms"], "ratio": v["torch_over_launches"],
                             "fwd_gb_s": v.get("forward_only", {}).get("gb_per_s"), "bwd_gb_s": v.get("backward_only", {}).get("gb_per_s"),
                             "peak": v["peak_bytes"], "differ": v["two_runs_differ_in_bits"], "grad_diff": v["grad_max_abs_difference"]}
                         for k, v in result["shapes"].items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
