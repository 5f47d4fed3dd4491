#!/usr/bin/env python
"""Time the region-proposal and RoI-pooling launches (edtr_amd/rois.py) on the device and write profiles/proposals_timing.json:

  proposals   the v2 detector's shape: one 800 x 1344 batch, five levels from 200 x 336 down, A = 3 (268 569 anchors), pre_nms_top_n =
              post_nms_top_n = 1000.  The whole call (two launches, the count reads, `boxes.batched_nms`); its two launches alone; the
              NMS alone on the same candidates; and beside them torch's own chain for the parts torch has on this device: permute and
              concatenate every level, decode every anchor, five topk, gather, sigmoid, clip, the two filters.  That chain has no NMS
              (torch has none), so it stands beside the two launches, and the NMS share is reported separately.
  roi_align   1000 rois x 256 channels on four levels (200 x 336 ... 25 x 42), 7 x 7 bins of 2 x 2 samples, fp32 and bf16 features;
              beside it the only counterpart torch has, a composite of the level mapper, `F.grid_sample` on 14 x 14 sample points per
              roi and a 2 x 2 average (zero padding instead of roi_align's border rule: a counterpart in cost, not in bits).

ms per call from device events around windows of at least 0.2 s of back-to-back calls, five windows per case with the cases of a
group taking turns; the median, the fastest and the slowest window are kept (tools/bench_boxes.py's method).  Inputs are resident on
the device; the wrappers' allocations, table uploads and count reads are inside.  Recorded with the kernel source hash, not gated.
Commit the file only after this has run on the device.

    python tools/bench_proposals.py [--out profiles/proposals_timing.json]
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

from edtr_amd import boxes, rois  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from bench_boxes import measure  # noqa: E402
from bench_labels import REPEATS, WARMUP, WINDOW_S  # noqa: E402

PADDED = (800, 1344)
GRIDS = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
A = 3


def head_outputs(dev):
    """what the RPN head of a trained detector emits on a photograph: mostly background (logits around -4), a few hundred confident
    anchors per level, deltas a fraction of an anchor"""
    rng = np.random.default_rng(2027)
    obj, deltas = [], []
    for h, w in GRIDS:
        o = rng.normal(-4, 1.5, (1, A, h, w)).astype(np.float32)
        hot = rng.random(o.shape) < 0.002
        o[hot] += rng.uniform(4, 9, int(hot.sum())).astype(np.float32)
        obj.append(torch.from_numpy(o).to(dev))
        deltas.append(torch.from_numpy(rng.normal(0, 0.3, (1, 4 * A, h, w)).astype(np.float32)).to(dev))
    return obj, deltas


def torch_chain(obj, deltas, anchors, image_size, pre=1000, min_size=1e-3, score_thresh=0.0):
    """concat_box_prediction_layers, BoxCoder.decode_single over every anchor, topk per level, gather, sigmoid, clip, the two filters"""
    N = obj[0].shape[0]
    flat_o = torch.cat([o.permute(0, 2, 3, 1).reshape(N, -1) for o in obj], dim=1)
    flat_d = torch.cat([d.view(N, -1, 4, d.shape[2], d.shape[3]).permute(0, 3, 4, 1, 2).reshape(N, -1, 4) for d in deltas], dim=1)
    wd, ht = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    cx, cy = anchors[:, 0] + 0.5 * wd, anchors[:, 1] + 0.5 * ht
    dw, dh = flat_d[..., 2].clamp(max=boxes.BBOX_XFORM_CLIP), flat_d[..., 3].clamp(max=boxes.BBOX_XFORM_CLIP)
    pcx, pcy = flat_d[..., 0] * wd + cx, flat_d[..., 1] * ht + cy
    hw_, hh_ = 0.5 * torch.exp(dw) * wd, 0.5 * torch.exp(dh) * ht
    prop = torch.stack((pcx - hw_, pcy - hh_, pcx + hw_, pcy + hh_), dim=2)
    idx, start = [], 0
    for o in obj:
        n = o[0].numel()
        idx.append(flat_o[:, start:start + n].topk(min(pre, n), dim=1)[1] + start)
        start += n
    idx = torch.cat(idx, dim=1)
    rows = torch.arange(N, device=idx.device)[:, None]
    prob, bx = torch.sigmoid(flat_o[rows, idx])[0], prop[rows, idx][0]
    bx = torch.stack((bx[:, 0].clamp(0, image_size[1]), bx[:, 1].clamp(0, image_size[0]), bx[:, 2].clamp(0, image_size[1]),
                      bx[:, 3].clamp(0, image_size[0])), dim=1)
    keep = torch.where((bx[:, 2] - bx[:, 0] >= min_size) & (bx[:, 3] - bx[:, 1] >= min_size) & (prob >= score_thresh))[0]
    return bx[keep], prob[keep]


def roi_inputs(dev, K=1000):
    rng = np.random.default_rng(2028)
    s = 224.0 * 2.0 ** (rng.uniform(1.0, 6.0, K) - 4.0)
    aspect = rng.uniform(0.5, 2.0, K)
    w, h = s * np.sqrt(aspect), s / np.sqrt(aspect)
    x1, y1 = rng.uniform(0, np.maximum(PADDED[1] - w, 1)), rng.uniform(0, np.maximum(PADDED[0] - h, 1))
    bx = np.stack([x1, y1, np.minimum(x1 + w, PADDED[1]), np.minimum(y1 + h, PADDED[0])], axis=1).astype(np.float32)
    return torch.from_numpy(bx).to(dev)


def torch_roi_composite(feats, bx, scales, k_min, k_max, P=7, S=2):
    """the level mapper, then per level F.grid_sample at roi_align's sample points and a mean over the S x S samples of a bin"""
    s = torch.sqrt((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1]))
    lvl = (torch.floor(4 + torch.log2(s / 224) + 1e-6).clamp(k_min, k_max) - k_min).to(torch.int64)
    out = torch.zeros((bx.shape[0], feats[0].shape[1], P, P), dtype=torch.float32, device=bx.device)
    t = (torch.arange(P * S, device=bx.device) // S + ((torch.arange(P * S, device=bx.device) % S) + 0.5) / S)[None]
    for l, f in enumerate(feats):
        pick = torch.where(lvl == l)[0]
        if not pick.numel():
            continue
        b = bx[pick] * scales[l]
        H, W = f.shape[-2:]
        bw, bh = (b[:, 2] - b[:, 0]).clamp(min=1) / P, (b[:, 3] - b[:, 1]).clamp(min=1) / P
        xs, ys = b[:, 0:1] + t * bw[:, None], b[:, 1:2] + t * bh[:, None]
        grid = torch.stack((2 * xs[:, None, :].expand(-1, P * S, -1) / (W - 1) - 1, 2 * ys[:, :, None].expand(-1, -1, P * S) / (H - 1) - 1), dim=-1)
        v = torch.nn.functional.grid_sample(f.float().expand(pick.numel(), -1, -1, -1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        out[pick] = v.view(pick.numel(), -1, P, S, P, S).mean(dim=(3, 5))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proposals_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
              "source_hash": source_hash(), "warmup": WARMUP, "window_s": WINDOW_S, "windows": REPEATS,
              "method": "device events around windows of at least `window_s` seconds of back-to-back calls after `warmup` calls; `windows` "
                        "windows per case, the cases of one group taking turns; ms = the median window per call, ms_min / ms_max the spread; "
                        "inputs resident on the device, the wrappers' allocations, table uploads and count reads included"}

    obj, deltas = head_outputs(dev)
    image_sizes = [PADDED]
    anchors = rois.anchors(GRIDS, PADDED)
    sel = rois.rpn_select(obj, 1000)
    cb, cp, cl, counts = rois.rpn_candidates(obj, deltas, sel, image_sizes, PADDED)
    m = int(counts[0].item())
    kept = int(rois.proposals(obj, deltas, image_sizes, PADDED)[0][0].shape[0])

    def two_launches():
        s = rois.rpn_select(obj, 1000)
        return rois.rpn_candidates(obj, deltas, s, image_sizes, PADDED)

    group = measure({"proposals": lambda: rois.proposals(obj, deltas, image_sizes, PADDED),
                     "select_and_candidates_launches": two_launches,
                     "select_launch_only": lambda: rois.rpn_select(obj, 1000),
                     "nms_only": lambda: boxes.batched_nms(cb[0, :m], cp[0, :m], cl[0, :m], 0.7, max_out=1000),
                     "anchors_launch": lambda: rois.anchors(GRIDS, PADDED),
                     "torch_chain_without_nms": lambda: torch_chain(obj, deltas, anchors, PADDED)})
    group.update(anchors=int(anchors.shape[0]), levels=len(GRIDS), A=A, pre_nms_top_n=1000, post_nms_top_n=1000, candidates=m, kept=kept)
    result["proposals"] = group

    bx = roi_inputs(dev)
    result["roi_align"] = {}
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        rng = np.random.default_rng(2029)
        feats = [torch.from_numpy(rng.normal(0, 1, (1, 256, h, w)).astype(np.float32)).to(dev).to(dtype) for h, w in GRIDS[:4]]
        scales, k_min, k_max = rois.level_scales([f.shape[-2:] for f in feats], image_sizes)
        group = measure({"launch": lambda: rois.roi_align(feats, [bx], image_sizes),
                         "torch_grid_sample_composite": lambda: torch_roi_composite(feats, bx, scales, k_min, k_max)})
        lv = rois.roi_levels_reference(bx.cpu().numpy(), k_min, k_max)
        group.update(rois=int(bx.shape[0]), channels=256, output_size=7, sampling_ratio=2, rois_per_level=np.bincount(lv, minlength=4).tolist(),
                     feature_bytes=int(sum(f.numel() * f.element_size() for f in feats)))
        result["roi_align"][name] = group

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
