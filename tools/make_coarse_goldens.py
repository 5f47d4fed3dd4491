#!/usr/bin/env python
"""Write tests/golden/coarse.npz for tests/test_coarse_cpu.py and tests/test_gpu_coarse.py: what the tail of the reference's
segmentation path makes of logits at the network's stride, in plain torch on the CPU —

    F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)      (model/deeplabv3.py:46)
    .argmax(1)                                                                    (main/seg/test_edtr.py:156)
    calculate_mat(mask.flatten(), pred.flatten(), n)                              (main/seg/test_edtr.py:159, the REFERENCE's function)

on two sets of seeded inputs with n = 21 and a batch of 2 (set (b): of 16):

  (a) standard-normal fp32 logits at (5, 7) -> (37, 51), (8, 8) -> (64, 64) and (9, 13) -> (65, 100): keys a{i}_coarse, a{i}_target,
      a{i}_pred, a{i}_mat;
  (b) a tie-prone set, logits rounded to multiples of 0.5, at (9, 13) -> (37, 51): keys b_coarse, b_target, b_pred, b_mat, and b_d,
      the largest absolute difference between `labels.upsample_logits_reference` and torch's upsample over this set.  Where the two
      disagree on a label they do so for a run of up to three pixels along a tie, about one image in three has such a run and most
      have none (2.7e-4 of the pixels over 128 such images), so the share of differing labels is a rate only over many images:
      a batch of 16, not of 2;
  (h) / (bf) the fp16 and bf16 roundings of 3 x standard-normal logits at (9, 13) -> (37, 51), interpolated by torch IN that type:
      h_coarse (fp16), bf_coarse (fp32 holding bf16 values), {h,bf}_pred and {h,bf}_d as in (b), between the widened 16-bit results.

Torch's CPU values are not the pinned rule (its CPU kernel forms the source coordinate differently from its GPU kernel and from the
written rule, and differs from it in the last bits of about half the words); they are recorded at the level of labels, with the
distance d that bounds where labels may differ.  Only arrays go into the file, written with fixed time stamps.

    python tools/make_coarse_goldens.py [--out tests/golden/coarse.npz]           (needs the reference tree; see tools/ref_import.py)
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ref_import  # noqa: E402
from make_labels_goldens import install_segmentation_stubs, write_npz  # noqa: E402

N_CLASSES = 21
BATCH = 2
TIE_BATCH = 16
SET_A = [((5, 7), (37, 51)), ((8, 8), (64, 64)), ((9, 13), (65, 100))]
TIE_CASE = ((9, 13), (37, 51))


def make_target(rng, size, batch: int = BATCH) -> np.ndarray:
    """uint8 [batch, H, W]: every class, the ignore label and two other values >= n"""
    t = rng.integers(0, N_CLASSES, size=(batch,) + size).astype(np.uint8)
    t[0].reshape(-1)[:N_CLASSES] = np.arange(N_CLASSES)
    t[1].reshape(-1)[:3] = (255, N_CLASSES, 200)
    return t


def torch_tail(seg, coarse_t: torch.Tensor, target: np.ndarray):
    """(upsampled logits widened to fp32, uint8 pred, int64 mat) by the three lines of the docstring"""
    with torch.no_grad():
        up = F.interpolate(coarse_t, size=target.shape[1:], mode="bilinear", align_corners=False)
        pred = up.argmax(1)
        mat = seg.calculate_mat(torch.from_numpy(target).long().flatten(), pred.flatten(), n=N_CLASSES)
    assert mat.dtype == torch.int64 and int(mat.sum()) == int((target < N_CLASSES).sum())
    return up.float().numpy(), pred.to(torch.uint8).numpy(), mat.numpy()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "coarse.npz"))
    args = ap.parse_args()
    from edtr_amd import labels
    install_segmentation_stubs()
    seg = ref_import.import_reference_file("ref_utils_segmentation", "utils/segmentation.py")
    rng = np.random.default_rng(20261)
    out = {"torch_version": np.array(torch.__version__), "a_cases": np.array([c[0] + c[1] for c in SET_A], dtype=np.int32),
           "tie_case": np.array(TIE_CASE[0] + TIE_CASE[1], dtype=np.int32)}

    for i, (ihw, size) in enumerate(SET_A):
        coarse = rng.standard_normal((BATCH, N_CLASSES) + ihw).astype(np.float32)
        target = make_target(rng, size)
        _, pred, mat = torch_tail(seg, torch.from_numpy(coarse), target)
        out.update({f"a{i}_coarse": coarse, f"a{i}_target": target, f"a{i}_pred": pred, f"a{i}_mat": mat})

    ihw, size = TIE_CASE
    coarse = (np.round(rng.standard_normal((TIE_BATCH, N_CLASSES) + ihw) * 2) / 2).astype(np.float32)
    target = make_target(rng, size, TIE_BATCH)
    up, pred, mat = torch_tail(seg, torch.from_numpy(coarse), target)
    d = np.abs(labels.upsample_logits_reference(coarse, size).astype(np.float64) - up).max()
    out.update(b_coarse=coarse, b_target=target, b_pred=pred, b_mat=mat, b_d=np.float64(d))
    report = [f"(b) d = {d:.3e}"]

    base = (3 * rng.standard_normal((BATCH, N_CLASSES) + ihw)).astype(np.float32)
    target = make_target(rng, size)
    for key, tdtype, name in (("h", torch.float16, "float16"), ("bf", torch.bfloat16, "bfloat16")):
        held = torch.from_numpy(base).to(tdtype)
        up, pred, _ = torch_tail(seg, held, target)
        widened = held.float().numpy()
        d = np.abs(labels.upsample_logits_reference(widened, size, name).astype(np.float64) - up).max()
        out.update({f"{key}_coarse": held.numpy() if tdtype == torch.float16 else widened, f"{key}_pred": pred, f"{key}_d": np.float64(d)})
        report.append(f"({key}) d = {d:.3e}")
    out["h_target"] = target

    write_npz(args.out, out)
    print(f"wrote {args.out}: torch {torch.__version__}, {len(out)} arrays, {os.path.getsize(args.out)} bytes; " + ", ".join(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
