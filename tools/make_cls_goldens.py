#!/usr/bin/env python
"""Write tests/golden/cls.npz for tests/test_cls_cpu.py and tests/test_gpu_cls.py:

  * the REFERENCE's own functions on recorded inputs, on the CPU: `calculate_accuracy` (utils/classification.py) for 1-D labels and
    2-D targets, `center_crop_arr` / `random_crop_arr` with a given `crop_pos` (datasets/utils.py) and `augment(return_status=True)`
    (datasets/augment.py) in all eight (hflip, vflip, rot90) states;
  * plain torch: `torch.topk` on the accuracy rows, the l1-mean expression of main/cls/test_edtr.py:153, the accuracy list-mean of
    :151,161 and torchvision's Normalize as the expression it is (`sub_` then `div_`; torchvision is not installed here).

The accuracy rows carry NO equal keys within a row: torch's topk is only defined there.  cv2 is not installed here either: `augment`
is given a numpy stand-in for the in-place `cv2.flip(src, code, dst)` it calls, so the flips of the golden are the stand-in's (the
archive says so in `flip_stand_in`); the transpose, the draws and their order are the reference's.

Only arrays go into the file, and the archive is written with fixed time stamps: the same inputs give the same bytes.

    python tools/make_cls_goldens.py [--out tests/golden/cls.npz]       (needs Pillow and the reference tree; see tools/ref_import.py)
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
from make_labels_goldens import install_segmentation_stubs, position_map, write_npz  # noqa: E402

ACC_BATCHES = (1, 3, 7, 8, 13)          # batch sizes of the recorded accuracy calls
ACC_CLASSES = 200
MEAN_BATCHES = [8] * 37 + [5]           # a data set of 301 images for the list-mean
FD_SHAPE = (3, 24, 7, 7)
FLIP_STAND_IN = "numpy stand-in for cv2.flip(src, code, dst): dst[...] = src[:, ::-1] for code 1, src[::-1] for code 0"


def flip(src, code, dst=None):
    """what `augment` needs of cv2.flip: code 1 mirrors the columns, code 0 the rows; written into dst (which may be src)"""
    assert code in (0, 1)
    out = (src[:, ::-1] if code == 1 else src[::-1]).copy()
    if dst is None:
        return out
    dst[...] = out
    return dst


def tie_free(rng, B: int, C: int) -> np.ndarray:
    """fp32 [B, C] with pairwise distinct values in every row"""
    base = (np.arange(C, dtype=np.float32) - C / 2) / 8
    return np.stack([rng.permutation(base) for _ in range(B)]).astype(np.float32)


def labels_for(rng, logits: np.ndarray) -> np.ndarray:
    """int64 [B]: by turns the best class, the third, the sixth and a random one"""
    order = np.argsort(-logits, axis=1)
    pick = [0, 2, 5]
    return np.array([order[b, pick[b % 4]] if b % 4 < 3 else rng.integers(0, logits.shape[1]) for b in range(logits.shape[0])], dtype=np.int64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cls.npz"))
    args = ap.parse_args()
    install_segmentation_stubs()
    ref_import.install_degrade_stubs()
    sys.modules["cv2"].flip = flip
    ref_cls = ref_import.import_reference_file("ref_utils_classification", "utils/classification.py")
    ref_utils = ref_import.import_reference_file("ref_datasets_utils", "datasets/utils.py")
    ref_aug = ref_import.import_reference_file("ref_datasets_augment", "datasets/augment.py")

    rng = np.random.default_rng(20261)
    out = {"flip_stand_in": np.array(FLIP_STAND_IN), "acc_batches": np.array(ACC_BATCHES, dtype=np.int32)}

    # calculate_accuracy(pred, label, topk=(1, 5)) and torch.topk on tie-free rows
    for i, B in enumerate(ACC_BATCHES):
        logits = tie_free(rng, B, ACC_CLASSES)
        lab = labels_for(rng, logits)
        res = ref_cls.calculate_accuracy(torch.from_numpy(logits), torch.from_numpy(lab), topk=(1, 5))
        assert all(r.dtype == torch.float32 for r in res)
        out[f"acc{i}_logits"], out[f"acc{i}_labels"] = logits, lab
        out[f"acc{i}_out"] = np.array([float(r) for r in res], dtype=np.float32)
        out[f"acc{i}_topk"] = torch.from_numpy(logits).topk(5, 1, True, True)[1].numpy().astype(np.int32)

    # 2-D targets: target.max(dim=1)[1] inside calculate_accuracy
    logits, target = tie_free(rng, 6, 17), tie_free(rng, 6, 17)
    target[:3] = np.eye(17, dtype=np.float32)[np.argsort(-logits[:3], axis=1)[:, [0, 1, 7]].diagonal()]      # one-hot rows: -0.0 / 0.0 ties elsewhere are fine for max
    res = ref_cls.calculate_accuracy(torch.from_numpy(logits), torch.from_numpy(target), topk=(1, 5))
    out.update(acc2d_logits=logits, acc2d_target=target, acc2d_out=np.array([float(r) for r in res], dtype=np.float32),
               acc2d_labels=torch.from_numpy(target).max(dim=1)[1].numpy().astype(np.int32))

    # the list-mean of main/cls/test_edtr.py:151,161 over a data set of many batches
    val_acc1, val_acc5, ns, acc, correct = [], [], [], [], []
    for B in MEAN_BATCHES:
        logits = tie_free(rng, B, 20)
        lab = np.where(rng.random(B) < 0.6, np.argsort(-logits, axis=1)[:, 0], rng.integers(0, 20, B)).astype(np.int64)
        a1, a5 = ref_cls.calculate_accuracy(torch.from_numpy(logits), torch.from_numpy(lab), topk=(1, 5))
        val_acc1 += [a1] * B
        val_acc5 += [a5] * B
        hit = torch.from_numpy(logits).topk(5, 1, True, True)[1].numpy() == lab[:, None]
        ns.append(B), acc.append([float(a1), float(a5)]), correct.append([int(hit[:, :1].sum()), int(hit.sum())])
    out.update(mean_n=np.array(ns, dtype=np.int32), mean_batch_acc=np.array(acc, dtype=np.float32), mean_correct=np.array(correct, dtype=np.int32),
               mean_acc1=np.float64(torch.tensor(val_acc1).mean().item()), mean_acc5=np.float64(torch.tensor(val_acc5).mean().item()))
    assert torch.tensor(val_acc1).dtype == torch.float32

    # every batch size below 300 with five counts each: correct_k * (100.0 / batch_size) on torch's fp32 count
    pairs = np.array([(n, c) for n in range(1, 300) for c in sorted({0, 1, n // 3, n // 2, n})], dtype=np.int32)
    scaled = [float(torch.tensor(float(c), dtype=torch.float32) * (100.0 / int(n))) for n, c in pairs]
    out.update(scale_pairs=pairs, scale_out=np.array(scaled, dtype=np.float32))

    # F.l1_loss(feat_res, feat_gt, reduction='none').mean(dim=(1, 2, 3))
    feat_res = rng.standard_normal(FD_SHAPE).astype(np.float32)
    feat_gt = (feat_res + 0.25 * rng.standard_normal(FD_SHAPE)).astype(np.float32)
    fd = F.l1_loss(input=torch.from_numpy(feat_res), target=torch.from_numpy(feat_gt), reduction="none").mean(dim=(1, 2, 3))
    out.update(fd_res=feat_res, fd_gt=feat_gt, fd_out=fd.numpy().astype(np.float32),
               fd_mean=np.float64(torch.tensor(fd.tolist()).mean().item()))

    # torchvision's Normalize as the expression it is, and the reference's inverse pair on its result
    x = rng.random((2, 3, 5, 7)).astype(np.float32)
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    inv_mean, inv_std = torch.tensor([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]), torch.tensor([1 / 0.229, 1 / 0.224, 1 / 0.225])
    y = torch.from_numpy(x).clone().sub_(mean[:, None, None]).div_(std[:, None, None])
    back = y.clone().sub_(inv_mean[:, None, None]).div_(inv_std[:, None, None])
    out.update(norm_x=x, norm_out=y.numpy(), norm_inv_out=back.numpy(), norm_constants=torch.stack([mean, std, inv_mean, inv_std]).numpy())

    # the crops, and augment in its eight states on a non-square 5 x 7 crop of a 9 x 11 position map
    src = position_map(9, 11, 3)
    out["geo_src"] = src
    out["geo_center5"] = np.ascontiguousarray(ref_utils.center_crop_arr(src, 5))
    out["geo_random5_pos"] = np.array([3, 4], dtype=np.int32)
    out["geo_random5"] = np.ascontiguousarray(ref_utils.random_crop_arr(src, 5, crop_pos=(3, 4)))
    out["geo_aug_origin"], out["geo_aug_hw"] = np.array([2, 3], dtype=np.int32), np.array([5, 7], dtype=np.int32)
    real_random = ref_aug.random.random
    try:
        for state in range(8):
            want = (bool(state & 1), bool(state & 2), bool(state & 4))
            draws = iter([0.25 if flag else 0.75 for flag in want])           # augment draws hflip, vflip, rot90 in this order
            ref_aug.random.random = lambda: next(draws)
            img, status = ref_aug.augment(src[2:7, 3:10].copy(), True, True, return_status=True)
            assert tuple(bool(s) for s in status) == want
            out[f"geo_aug{state}"] = np.ascontiguousarray(img)
    finally:
        ref_aug.random.random = real_random

    write_npz(args.out, out)
    print(f"wrote {args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
