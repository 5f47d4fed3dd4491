#!/usr/bin/env python
"""Write tests/golden/targets.npz for tests/test_targets_cpu.py and tests/test_gpu_targets.py.

The REFERENCE's own code, on the CPU, on hand-built and seeded inputs (model/faster_rcnn.py, model/util.py): `Matcher`,
`BoxCoder.encode`, `BalancedPositiveNegativeSampler`, `RegionProposalNetwork.assign_targets_to_anchors` and `compute_loss`,
`RoIHeads.select_training_samples` and `fastrcnn_loss` (the methods called unbound on a namespace that carries their collaborators).

Two stand-ins, both written for this tool:
  * `box_iou` does the job of `torchvision.ops.boxes.box_iou`, whose binary is not available here, by the rule edtr_amd/targets.py
    writes out, in torch's own fp32 operations: IoU is pinned to the written rule, as NMS and RoIAlign are;
  * `torch.randperm` is replaced, for the sampler calls only, by the stable argsort of the class's keys from the seeded stream
    (`rng.uniform_words_reference`): the reference's `positive[perm[:num_pos]]` then picks exactly the num_pos smallest keys.

Fixtures: the RPN geometry has 1512 anchors (padded 64 x 96, grids 16 x 24 / 8 x 12 / 4 x 6, three anchors per cell), more than one
tile of the match launches.  Three images: five ground truths — one equal to an anchor, one midway between two anchors (its best IoU
is shared, both are restored), two identical ones (equal IoU, the first wins) —, one ground truth that overlaps no anchor (its highest
IoU is 0 and `set_low_quality_matches_` restores every anchor), and none.  The tool asserts each of these properties and that no best
IoU lies within 4 ulp of a threshold.  The RoI flow takes 1511 proposals per image, a size no tile divides; a
last case fills three of an image's eight slots, for the loss over unfilled slots.

Tolerances are MEASURED here and stored: the reference's fp32 result against the fp64 evaluation of the same code on the same
fixture, or one fp32 ulp of the result where that is larger (the result is itself rounded to fp32), times ORDER = 4 for another
summation order or another log.  Only arrays go into the file, and the archive is written with fixed time stamps.

    python tools/make_targets_goldens.py [--out tests/golden/targets.npz]       (needs the reference tree; see tools/ref_import.py)
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_boxes_goldens import install_detection_stubs  # noqa: E402
from make_labels_goldens import write_npz  # noqa: E402
from make_proposals_goldens import reference_anchors  # noqa: E402

SEED = 20281
ORDER = 4.0
F = np.float32
PADDED, GRIDS = (64, 96), [(16, 24), (8, 12), (4, 6)]
SIZES, RATIOS = ((8,), (16,), (32,)), ((0.5, 1.0, 2.0),) * 3
IMAGE_IDS, DRAW = [7, 4_000_000_123, 19], 3
RPN = dict(high=0.7, low=0.3, batch=256, fraction=0.5)
ROI = dict(high=0.5, low=0.5, batch=64, fraction=0.25, weights=(10.0, 10.0, 5.0, 5.0))
N_PROPOSALS, N_CLASSES = 1511, 5


def box_iou(boxes1, boxes2):
    """the stand-in for torchvision.ops.boxes.box_iou: its published formula in torch's own operations"""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


class KeyedRandperm:
    """torch.randperm for the sampler: hands out, in the order the sampler asks, the stable argsort of the positives' and then the
    negatives' keys of each image"""

    def __init__(self, labels, keys):
        self.queue = []
        for lab, key in zip(labels, keys):
            lab = lab.numpy() if hasattr(lab, "numpy") else np.asarray(lab)
            for pick in (np.nonzero(lab >= 1)[0], np.nonzero(lab == 0)[0]):
                self.queue.append(torch.from_numpy(np.argsort(np.asarray(key)[pick], kind="stable")))

    def __call__(self, n, **kw):
        perm = self.queue.pop(0)
        assert perm.numel() == n, (perm.numel(), n)
        return perm

    def __enter__(self):
        self.saved, torch.randperm = torch.randperm, self
        return self

    def __exit__(self, *exc):
        torch.randperm = self.saved
        assert exc[0] is not None or not self.queue


def stream_keys(rng_mod, counts, purpose):
    return [rng_mod.uniform_words_reference(SEED, [i], purpose, DRAW, (c + 3) // 4 * 4)[0, :c] for i, c in zip(IMAGE_IDS, counts)]


def ulps_from(v, t) -> int:
    """the least distance in fp32 units of the last place between the positive values v and the threshold t"""
    v, t = np.asarray(v, dtype=F).view(np.int32).astype(np.int64), np.asarray(F(t)).view(np.int32).astype(np.int64)
    return int(np.abs(v - t).min())


def measured(fp32, fp64) -> float:
    """ORDER x the larger of |fp32 - fp64| and one fp32 ulp of the value, over the finite entries"""
    a, b = np.asarray(fp32, dtype=np.float64).reshape(-1), np.asarray(fp64, dtype=np.float64).reshape(-1)
    ok = np.isfinite(a) & np.isfinite(b)
    return float(ORDER * np.maximum(np.abs(a[ok] - b[ok]), np.abs(b[ok]) * 2.0 ** -23).max())


def ground_truth(anchors):
    """the three images' boxes and labels (see the module docstring)"""
    A0 = GRIDS[0][0] * GRIDS[0][1] * 3
    exact = anchors[A0 + (3 * 12 + 5) * 3 + 1]                       # a level-1 anchor, copied
    left = anchors[(6 * 24 + 9) * 3 + 1]                             # a level-0 anchor and its right-hand neighbour: the box midway
    midway = left + np.array([2.0, 0.0, 2.0, 0.0], dtype=F)          # (stride 4) has the same IoU with both
    twin = np.array([50.5, 20.25, 80.5, 52.75], dtype=F)
    g0 = np.stack([exact, midway, np.array([20.3, 10.7, 50.9, 41.2], dtype=F), twin, twin]).astype(F)
    g1 = np.array([[300.0, 300.0, 340.0, 340.0]], dtype=F)           # overlaps no anchor
    return [g0, g1, np.zeros((0, 4), dtype=F)], [np.array([3, 1, 4, 2, 2], dtype=np.int64), np.array([2], dtype=np.int64), np.zeros(0, dtype=np.int64)]


def proposals_for(rng, gt):
    """1511 boxes: random ones inside the padded batch and jittered copies of the ground truths on both sides of IoU 0.5"""
    x1, y1 = rng.uniform(-2, PADDED[1] * 0.8, N_PROPOSALS), rng.uniform(-2, PADDED[0] * 0.8, N_PROPOSALS)
    b = np.stack([x1, y1, x1 + rng.uniform(2, 50, N_PROPOSALS), y1 + rng.uniform(2, 40, N_PROPOSALS)], axis=1)
    if len(gt):
        k = 150
        src = gt[rng.integers(0, len(gt), k)].astype(np.float64)
        side = np.stack([src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]] * 2, axis=1)
        b[:k] = src + rng.normal(0, 0.12, (k, 4)) * side
    return b.astype(F)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "targets.npz"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    install_detection_stubs()
    import importlib
    util = importlib.import_module("model.util")
    frcnn = importlib.import_module("model.faster_rcnn")
    frcnn.box_ops.box_iou = box_iou
    from edtr_amd import rng as project_rng

    tt = torch.from_numpy
    anchors = reference_anchors(frcnn, util, PADDED, GRIDS, SIZES, RATIOS)
    assert anchors.shape == (1512, 4)
    gt, gt_labels = ground_truth(anchors)
    N, A = len(gt), anchors.shape[0]
    targets = [{"boxes": tt(b), "labels": tt(l)} for b, l in zip(gt, gt_labels)]
    out = dict(seed=np.array(SEED, dtype=np.int64), image_ids=np.array(IMAGE_IDS, dtype=np.int64), draw=np.array(DRAW, dtype=np.int64),
               padded=np.array(PADDED, dtype=np.int32), grids=np.array(GRIDS, dtype=np.int32), sizes=np.array(SIZES, dtype=np.float64),
               ratios=np.array(RATIOS, dtype=np.float64), anchors=anchors)
    for n in range(N):
        out[f"gt_boxes{n}"], out[f"gt_labels{n}"] = gt[n], gt_labels[n]

    # ---- Matcher: the 3 x 5 matrix with an all-zero row, and the fixture's properties -------------------------------------------------
    q35 = np.array([[0.8, 0.1, 0.2, 0.5, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0], [0.1, 0.4, 0.9, 0.2, 0.1]], dtype=F)
    m35 = util.Matcher(0.7, 0.3, True)(tt(q35).clone()).numpy()
    assert m35.tolist() == [0, 2, 2, 0, 2], m35
    out.update(q35=q35, q35_matched=m35.astype(np.int32), q35_plain=util.Matcher(0.7, 0.3, False)(tt(q35).clone()).numpy().astype(np.int32))

    matcher = util.Matcher(RPN["high"], RPN["low"], True)
    iou0 = box_iou(tt(gt[0]), tt(anchors))
    best = iou0.max(dim=0)[0].numpy()
    assert (iou0[1] == iou0[1].max()).sum() == 2 and float(iou0[1].max()) < RPN["high"], "the midway box shares its best IoU between two anchors"
    assert float(iou0[0].max()) == 1.0 and bool((iou0[3] == iou0[4]).all()) and float(iou0[3].max()) > 0
    assert (best < F(0.3)).any() and ((best >= F(0.3)) & (best < F(0.7))).any() and (best >= F(0.7)).any()
    assert min(ulps_from(best[best > 0], 0.3), ulps_from(best[best > 0], 0.7)) >= 4, "a best IoU within 4 ulp of a threshold"
    assert float(box_iou(tt(gt[1]), tt(anchors)).max()) == 0.0
    # the five ground truths and the one that overlaps nothing together: the quirk beside real matches
    gt6 = np.concatenate([gt[0], gt[1]])
    plain0 = util.Matcher(RPN["high"], RPN["low"], True)(box_iou(tt(gt[0]), tt(anchors))).numpy()
    quirk6 = util.Matcher(RPN["high"], RPN["low"], True)(box_iou(tt(gt6), tt(anchors))).numpy()
    assert (plain0 < 0).any() and (quirk6 >= 0).all()
    out.update(gt6=gt6, quirk6_matched=quirk6.astype(np.int32))
    rpn_matched = [matcher(box_iou(tt(g), tt(anchors))).numpy() if len(g) else np.zeros(A, dtype=np.int64) for g in gt]
    out["rpn_matched"] = np.stack(rpn_matched).astype(np.int32)

    # ---- the RPN flow: assign_targets_to_anchors, BoxCoder.encode, the sampler, compute_loss ------------------------------------------
    sampler = util.BalancedPositiveNegativeSampler(RPN["batch"], RPN["fraction"])
    ns = types.SimpleNamespace(box_similarity=box_iou, proposal_matcher=matcher, fg_bg_sampler=sampler)
    anchor_list = [tt(anchors)] * N
    labels, matched_gt = frcnn.RegionProposalNetwork.assign_targets_to_anchors(ns, anchor_list, targets)
    coder = util.BoxCoder((1.0, 1.0, 1.0, 1.0))
    regression = coder.encode(matched_gt, anchor_list)
    regression64 = util.encode_boxes(torch.cat(matched_gt).double(), torch.cat(anchor_list).double(), torch.ones(4, dtype=torch.float64))
    keys = stream_keys(project_rng, [A] * N, project_rng.PURPOSE_SAMPLE_RPN)
    with KeyedRandperm(labels, keys):
        pos, neg = sampler(labels)
    rng = np.random.default_rng([SEED, 1])
    objectness = rng.normal(0, 2, (N * A, 1)).astype(F)
    deltas = (torch.cat(regression).nan_to_num(0.0, 0.0, 0.0).numpy() + rng.normal(0, 0.3, (N * A, 4))).astype(F)
    with KeyedRandperm(labels, keys):
        loss = frcnn.RegionProposalNetwork.compute_loss(ns, tt(objectness), tt(deltas), labels, regression)
    with KeyedRandperm(labels, keys):
        loss64 = frcnn.RegionProposalNetwork.compute_loss(ns, tt(objectness).double(), tt(deltas).double(), [l.double() for l in labels],
                                                          [r.double() for r in regression64.split([A] * N)])
    counts = [(int(p.sum()), int(q.sum())) for p, q in zip(pos, neg)]
    assert counts[0][0] < 128 and counts[0][0] + counts[0][1] == 256, counts          # fewer positives than asked: negatives fill the batch
    assert counts[1] == (128, 0) and counts[2] == (0, 256), counts                    # more positives than asked and no negative; no positive
    out.update(rpn_labels=torch.stack(labels).numpy(), rpn_regression=torch.stack(list(regression)).numpy(),
               rpn_mask_pos=torch.stack(pos).numpy(), rpn_mask_neg=torch.stack(neg).numpy(), rpn_counts=np.array(counts, dtype=np.int32),
               rpn_objectness=objectness, rpn_deltas=deltas, rpn_loss=np.array([float(v) for v in loss], dtype=np.float64),
               rpn_params=np.array([RPN["high"], RPN["low"], RPN["batch"], RPN["fraction"]], dtype=np.float64),
               tol_rpn_dwdh=np.array(measured(torch.cat(regression)[:, 2:].numpy(), regression64[:, 2:].numpy())),
               tol_rpn_loss=np.array([measured(float(a), float(b)) for a, b in zip(loss, loss64)]))
    print(f"rpn: sampled (pos, neg) per image {counts}, losses {[float(v) for v in loss]}")

    # ---- the sampler on equal keys ----------------------------------------------------------------------------------------------------
    eq_labels = np.array([1, 0, 1, -1, 0, 1, 1, 0, 0, 2, 0, 1], dtype=np.int64)
    eq_keys = np.array([5, 9, 5, 1, 9, 5, 2, 9, 3, 5, 9, 7], dtype=np.uint32)
    small = util.BalancedPositiveNegativeSampler(6, 0.5)
    with KeyedRandperm([eq_labels], [eq_keys]):
        ep, en = small([tt(eq_labels)])
    out.update(eq_labels=eq_labels, eq_keys=eq_keys, eq_mask_pos=ep[0].numpy(), eq_mask_neg=en[0].numpy(), eq_params=np.array([6, 0.5]))

    # ---- the RoI flow: select_training_samples, fastrcnn_loss -------------------------------------------------------------------------
    rng = np.random.default_rng([SEED, 2])
    proposals = [proposals_for(rng, g) for g in gt]
    roi_sampler = util.BalancedPositiveNegativeSampler(ROI["batch"], ROI["fraction"])
    heads = types.SimpleNamespace(proposal_matcher=util.Matcher(ROI["high"], ROI["low"], False), fg_bg_sampler=roi_sampler,
                                  box_coder=util.BoxCoder(ROI["weights"]), has_mask=lambda: False)
    for name in ("check_targets", "add_gt_proposals", "assign_targets_to_proposals", "subsample"):
        setattr(heads, name, types.MethodType(getattr(frcnn.RoIHeads, name), heads))
    with_gt = [torch.cat([tt(p), tt(g)]) for p, g in zip(proposals, gt)]
    all_matched, all_labels = heads.assign_targets_to_proposals(with_gt, [tt(g) for g in gt], [tt(l) for l in gt_labels])
    roi_keys = stream_keys(project_rng, [len(p) for p in with_gt], project_rng.PURPOSE_SAMPLE_ROI)
    with KeyedRandperm(all_labels, roi_keys):
        s_props, s_matched, s_labels, s_targets = frcnn.RoIHeads.select_training_samples(heads, [tt(p) for p in proposals], targets)
    kept = [len(l) for l in s_labels]
    pos_kept = [int((l > 0).sum()) for l in s_labels]
    assert pos_kept[0] == 16 and kept == [64, 64, 64] and pos_kept[2] == 0, (kept, pos_kept)
    gt_of = [tt(g)[m] if len(g) else torch.zeros((len(m), 4)) for g, m in zip(gt, s_matched)]
    targets64 = util.encode_boxes(torch.cat(gt_of).double(), torch.cat(s_props).double(), torch.tensor(ROI["weights"], dtype=torch.float64))
    rows = sum(kept)
    logits = rng.normal(0, 2, (rows, N_CLASSES)).astype(F)
    box_regression = rng.normal(0, 0.5, (rows, 4 * N_CLASSES)).astype(F)
    roi_loss = frcnn.fastrcnn_loss(tt(logits), tt(box_regression), s_labels, list(s_targets))
    roi_loss64 = frcnn.fastrcnn_loss(tt(logits).double(), tt(box_regression).double(), s_labels, list(targets64.split(kept)))
    for n in range(N):
        out.update({f"roi_input{n}": proposals[n], f"roi_all_matched{n}": all_matched[n].numpy().astype(np.int32), f"roi_all_labels{n}": all_labels[n].numpy(),
                    f"roi_proposals{n}": s_props[n].numpy(), f"roi_matched{n}": s_matched[n].numpy(), f"roi_labels{n}": s_labels[n].numpy(),
                    f"roi_targets{n}": s_targets[n].numpy()})
    out.update(roi_params=np.array([ROI["high"], ROI["low"], ROI["batch"], ROI["fraction"]], dtype=np.float64), roi_weights=np.array(ROI["weights"]),
               roi_logits=logits, roi_box_regression=box_regression, roi_loss=np.array([float(v) for v in roi_loss], dtype=np.float64),
               tol_roi_dwdh=np.array(measured(torch.cat(list(s_targets))[:, 2:].numpy(), targets64[:, 2:].numpy())),
               tol_roi_loss=np.array([measured(float(a), float(b)) for a, b in zip(roi_loss, roi_loss64)]))
    print(f"roi: kept {kept}, positives {pos_kept}, losses {[float(v) for v in roi_loss]}")

    # ---- an image that fills fewer slots than the batch: two proposals and one ground truth for 8 slots -----------------------------
    pad_gt, pad_label = np.array([[2, 2, 20, 20]], dtype=F), np.array([3], dtype=np.int64)
    pad_props = np.array([[1, 1, 19, 21], [40, 40, 50, 50]], dtype=F)
    heads.fg_bg_sampler = util.BalancedPositiveNegativeSampler(8, 0.25)
    pad_all = heads.assign_targets_to_proposals([torch.cat([tt(pad_props), tt(pad_gt)])], [tt(pad_gt)], [tt(pad_label)])[1]
    pad_keys = [project_rng.uniform_words_reference(SEED, [IMAGE_IDS[0]], project_rng.PURPOSE_SAMPLE_ROI, DRAW, 4)[0, :3]]
    with KeyedRandperm(pad_all, pad_keys):
        p_props, p_matched, p_labels, p_targets = frcnn.RoIHeads.select_training_samples(heads, [tt(pad_props)], [{"boxes": tt(pad_gt), "labels": tt(pad_label)}])
    assert p_labels[0].tolist() == [3, 0, 3]
    pad_logits = rng.normal(0, 1, (8, N_CLASSES)).astype(F)
    pad_regression = rng.normal(0, 1, (8, 4 * N_CLASSES)).astype(F)
    pad_loss = frcnn.fastrcnn_loss(tt(pad_logits[:3]), tt(pad_regression[:3]), p_labels, list(p_targets))
    pad_targets64 = util.encode_boxes(tt(pad_gt)[p_matched[0]].double(), p_props[0].double(), torch.tensor(ROI["weights"], dtype=torch.float64))
    pad_loss64 = frcnn.fastrcnn_loss(tt(pad_logits[:3]).double(), tt(pad_regression[:3]).double(), p_labels, [pad_targets64])
    out.update(pad_gt=pad_gt, pad_label=pad_label, pad_props=pad_props, pad_logits=pad_logits, pad_box_regression=pad_regression,
               pad_loss=np.array([float(v) for v in pad_loss], dtype=np.float64),
               tol_pad_loss=np.array([measured(float(a), float(b)) for a, b in zip(pad_loss, pad_loss64)]))
    print("tolerances:", {k: out[k].tolist() for k in out if k.startswith("tol_")})

    write_npz(args.out, out)
    print(f"wrote {args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
