#!/usr/bin/env python
"""Write tests/golden/boxes.npz for tests/test_boxes_cpu.py and tests/test_gpu_boxes.py: the REFERENCE's own functions on seeded
inputs, on the CPU —

  * `BoxCoder.decode` (model/util.py) on proposals and codes that reach the exp clamp;
  * `sliding_windows`, `move_boxes` (utils/detection.py) and `resize_boxes` (model/faster_rcnn.py);
  * `RoIHeads.postprocess_detections` (model/faster_rcnn.py), called unbound on a namespace that carries `box_coder`, `score_thresh`,
    `nms_thresh` and `detections_per_img`;
  * the labels for which `convert2label` names no class, and those it names "tvmonitor" (what `draw_box`'s rules turn on).

`torchvision.ops.boxes` is NOT available here, so it is stood in by the three functions below, written for this tool:
`clip_boxes_to_image`, `remove_small_boxes` and a `batched_nms` that is a deliberately naive per-pair Python loop over the rule
edtr_amd/boxes.py writes out (descending stable score order; a kept box suppresses the later boxes of its label whose fp32
inter / (area_i + area_j - inter) is strictly greater than the threshold).  NMS is therefore pinned to that written rule, not to
torchvision's binary.  Everything else in `postprocess_detections` — softmax, decode, the score filter, the top-k — is the reference's
own code running.

Only arrays go into the file, and the archive is written with fixed time stamps: the same inputs give the same bytes.

    python tools/make_boxes_goldens.py [--out tests/golden/boxes.npz]       (needs the reference tree; see tools/ref_import.py)
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ref_import  # noqa: E402
from make_labels_goldens import write_npz  # noqa: E402

SEED = 20261
WINDOW_CASES = [(160, 96, 64, 32), (512, 512, 512, 256), (750, 500, 512, 256), (300, 200, 512, 256), (1024, 768, 512, 256),
                (513, 512, 512, 256), (100, 130, 64, 48), (64, 64, 64, 64)]          # (W, H, tile, stride)


# ---- the stand-in for torchvision.ops.boxes ----------------------------------------------------------------------------------------
def clip_boxes_to_image(boxes, size):
    h, w = size
    x = boxes[..., 0::2].clamp(min=0, max=w)
    y = boxes[..., 1::2].clamp(min=0, max=h)
    return torch.stack((x, y), dim=boxes.dim()).reshape(boxes.shape)


def remove_small_boxes(boxes, min_size):
    ws, hs = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    return torch.where((ws >= min_size) & (hs >= min_size))[0]


def naive_batched_nms(boxes, scores, idxs, iou_threshold):
    """one pair at a time, fp32 scalars: the written rule and nothing else"""
    f = np.float32
    b = boxes.detach().numpy().astype(f)
    s = scores.detach().numpy().astype(f)
    lab = idxs.detach().numpy()
    order = sorted(range(len(s)), key=lambda i: (-np.inf if np.isnan(s[i]) else -float(s[i]), i))
    thr = f(iou_threshold)
    dead, keep = set(), []
    for a, i in enumerate(order):
        if i in dead:
            continue
        keep.append(i)
        area_i = f(f(b[i, 2] - b[i, 0]) * f(b[i, 3] - b[i, 1]))
        for j in order[a + 1:]:
            if j in dead or lab[j] != lab[i]:
                continue
            w = f(min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]))
            h = f(min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            inter = f(max(w, f(0)) * max(h, f(0)))
            area_j = f(f(b[j, 2] - b[j, 0]) * f(b[j, 3] - b[j, 1]))
            union = f(f(area_i + area_j) - inter)
            if union != 0 and f(inter / union) > thr:
                dead.add(j)
    return torch.tensor(keep, dtype=torch.int64)


def install_detection_stubs() -> None:
    """Stand-ins for what model/faster_rcnn.py, model/util.py and utils/detection.py import at module level.  Only
    `torchvision.ops.boxes` is CALLED by what this tool runs; the rest are names that have to exist.  The reference's `model` package is
    registered without running its __init__ (which builds the whole restoration stack)."""
    ref_import.install_degrade_stubs()            # torchvision, cv2, timm, ftfy, omegaconf
    tv = sys.modules["torchvision"]
    tv._is_tracing = lambda: False
    box_ops = ref_import._module("torchvision.ops.boxes", clip_boxes_to_image=clip_boxes_to_image, remove_small_boxes=remove_small_boxes,
                                 batched_nms=naive_batched_nms)
    name = lambda n: type(n, (torch.nn.Module,), {})  # noqa: E731
    tv.ops = ref_import._module("torchvision.ops", boxes=box_ops, roi_align=None, MultiScaleRoIAlign=name("MultiScaleRoIAlign"))
    ref_import._module("torchvision.ops.feature_pyramid_network", ExtraFPNBlock=name("ExtraFPNBlock"),
                       FeaturePyramidNetwork=name("FeaturePyramidNetwork"), LastLevelMaxPool=name("LastLevelMaxPool"))
    for mod, attrs in (("pycocotools", {}), ("pycocotools.mask", {}), ("pycocotools.coco", dict(COCO=None)),
                       ("pycocotools.cocoeval", dict(COCOeval=None)), ("accelerate", {}), ("accelerate.utils", dict(set_seed=lambda seed: None)),
                       ("utils", {}), ("utils.common", dict(copy_opt_file=None, print_attn_type=None, Logger=None))):
        if mod not in sys.modules:
            ref_import._module(mod, **attrs)
    sys.modules["pycocotools"].mask = sys.modules["pycocotools.mask"]
    if "model" not in sys.modules:
        pkg = types.ModuleType("model")
        pkg.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "model")]
        sys.modules["model"] = pkg


def head_inputs(rng, P, C, h, w):
    """proposals inside an h x w image, logits with a few confident classes per row, codes of the size a trained head emits (some
    beyond the exp clamp, some that shrink a box below min_size, some that leave the image)"""
    x1, y1 = rng.uniform(0, w * 0.8, P), rng.uniform(0, h * 0.8, P)
    bw, bh = rng.uniform(4, w * 0.5, P), rng.uniform(4, h * 0.5, P)
    # clusters: every third proposal repeats an earlier one with a small jitter, so that NMS has something to suppress
    for i in range(2, P, 3):
        j = rng.integers(0, i)
        x1[i], y1[i], bw[i], bh[i] = x1[j] + rng.uniform(-3, 3), y1[j] + rng.uniform(-3, 3), bw[j] * rng.uniform(0.9, 1.1), bh[j] * rng.uniform(0.9, 1.1)
    proposals = np.stack([x1, y1, np.minimum(x1 + bw, w), np.minimum(y1 + bh, h)], axis=1).astype(np.float32)
    logits = rng.normal(0, 1, (P, C)).astype(np.float32)
    hot = rng.integers(0, C, P)
    hot[2::3] = hot[rng.integers(0, 2, len(hot[2::3]))]
    logits[np.arange(P), hot] += rng.uniform(2, 6, P).astype(np.float32)
    codes = rng.normal(0, 0.5, (P, 4 * C)).astype(np.float32)
    codes[:, 2::4] *= 2
    codes[:, 3::4] *= 2
    codes[0, 2::4] = 30.0                 # dw / ww = 6 > log(1000 / 16): the clamp
    codes[1, 3::4] = -60.0                # exp(-12) h: a box thinner than min_size
    return logits, codes, proposals


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "boxes.npz"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    install_detection_stubs()
    import importlib
    util = importlib.import_module("model.util")
    frcnn = importlib.import_module("model.faster_rcnn")
    det = ref_import.import_reference_file("ref_utils_detection", "utils/detection.py")
    assert frcnn.box_ops.batched_nms is naive_batched_nms

    rng = np.random.default_rng(SEED)
    out = {}
    weights, clip = (10.0, 10.0, 5.0, 5.0), math.log(1000.0 / 16)
    coder = util.BoxCoder(weights, clip)

    # BoxCoder.decode
    logits, codes, proposals = head_inputs(rng, 24, 5, 300, 400)
    with torch.no_grad():
        dec = coder.decode(torch.from_numpy(codes), [torch.from_numpy(proposals)])
    assert dec.shape == (24, 5, 4) and dec.dtype == torch.float32
    out.update(decode_codes=codes, decode_proposals=proposals, decode_out=dec.numpy())

    # sliding_windows
    out["window_cases"] = np.array(WINDOW_CASES, dtype=np.int32)
    for i, (W, H, tile, stride) in enumerate(WINDOW_CASES):
        out[f"windows{i}"] = np.array(list(det.sliding_windows(W, H, tile=tile, stride=stride)), dtype=np.int32).reshape(-1, 4)

    # move_boxes, resize_boxes
    boxes = (rng.uniform(0, 700, (40, 4)) + rng.uniform(0, 1, (40, 4))).astype(np.float32)
    with torch.no_grad():
        moved = det.move_boxes(torch.from_numpy(boxes), dx=96, dy=37)
        resized = frcnn.resize_boxes(torch.from_numpy(boxes), [750, 500], [800, 533])
    out.update(boxes_in=boxes, move_dxdy=np.array([96, 37], dtype=np.int32), move_out=moved.numpy(),
               resize_sizes=np.array([[750, 500], [800, 533]], dtype=np.int32), resize_out=resized.numpy())

    # postprocess_detections, unbound, for one image and two heads: VOC's 21 classes and COCO's 91
    # The seed of each head is the first from SEED on whose REFERENCE output has no corner within a fortieth of a side of the origin
    # (`boxes.cancellation_ratio` has the reasoning): there exp's last bit, which numpy and torch may round differently, decides more
    # than 1e-5 of the coordinate.
    from edtr_amd import boxes as project_boxes
    for tag, P, C, hw, per_img in (("voc", 120, 21, (375, 500), 100), ("coco", 90, 91, (480, 640), 20)):
        for seed in range(SEED, SEED + 64):
            logits, codes, proposals = head_inputs(np.random.default_rng([seed, C]), P, C, *hw)
            head = types.SimpleNamespace(box_coder=coder, score_thresh=0.05, nms_thresh=0.5, detections_per_img=per_img)
            with torch.no_grad():
                b, s, lab = frcnn.RoIHeads.postprocess_detections(head, torch.from_numpy(logits), torch.from_numpy(codes),
                                                                   [torch.from_numpy(proposals)], [hw])
            if project_boxes.cancellation_ratio(b[0].numpy(), hw) <= 40:
                break
        else:
            raise SystemExit(f"no seed in [{SEED}, {SEED + 64}) gives a well-conditioned {tag} case")
        assert len(b) == 1 and 0 < len(b[0]) <= per_img
        out.update({f"post_{tag}_logits": logits, f"post_{tag}_codes": codes, f"post_{tag}_proposals": proposals,
                    f"post_{tag}_shape": np.array(hw, dtype=np.int32), f"post_{tag}_per_img": np.array(per_img, dtype=np.int32),
                    f"post_{tag}_seed": np.array(seed, dtype=np.int64),
                    f"post_{tag}_boxes": b[0].numpy(), f"post_{tag}_scores": s[0].numpy(), f"post_{tag}_labels": lab[0].numpy()})
        print(f"{tag}: seed {seed}, {len(b[0])} detections kept")

    # what draw_box's rules turn on: labels without a class, and the tvmonitor labels (label 0 names the table's last entry)
    out["coco_unnamed_labels"] = np.array([lab for lab in range(0, 92) if det.convert2label(lab - 1, is_coco=True) == "-"], dtype=np.int64)
    out["voc_tvmonitor_labels"] = np.array([lab for lab in range(0, 21) if det.convert2label(lab - 1, is_coco=False) == "tvmonitor"], dtype=np.int64)
    lengths = []
    for coco in (False, True):
        n = 0
        while _table_has(det, n + 1, coco):
            n += 1
        lengths.append(n)
    out["label_table_lengths"] = np.array(lengths, dtype=np.int64)          # (VOC, COCO): the largest label each table names

    write_npz(args.out, out)
    print(f"wrote {args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes")
    return 0


def _table_has(det, label: int, is_coco: bool) -> bool:
    try:
        det.convert2label(label - 1, is_coco=is_coco)
        return True
    except IndexError:
        return False


if __name__ == "__main__":
    sys.exit(main())
