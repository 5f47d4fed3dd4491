#!/usr/bin/env python
"""Write tests/golden/proposals.npz for tests/test_rois_cpu.py and tests/test_gpu_rois.py.

The REFERENCE's own code, on the CPU, on seeded inputs (model/faster_rcnn.py, model/util.py):

  * `AnchorGenerator.forward` for the v2 detector's five levels, for the mobilenet form (15 anchors per cell on 3 levels) and for a
    padded size that no grid size divides;
  * `concat_box_prediction_layers`, `BoxCoder.decode` and `RegionProposalNetwork.filter_proposals` (called unbound on a namespace that
    carries the thresholds), for two images in one padded batch and two sets of thresholds.

`torchvision.ops.boxes` is not available here; `filter_proposals` runs with the three stand-ins of tools/make_boxes_goldens.py
(`clip_boxes_to_image`, `remove_small_boxes`, the naive per-pair `batched_nms`), so NMS is pinned to the written rule.  The seed of
the head outputs is the first from SEED on for which, in every image and under both sets of thresholds, no kept corner is
ill-conditioned (`boxes.cancellation_ratio` <= 40) and no two probabilities that reach the NMS lie within 4 ulp of each other
without being equal: two implementations of exp may then order them differently.

For RoIAlign nothing of the reference can run (its operator is compiled torchvision).  Recorded instead:

  * `roi_align_scalar`, a per-sample scalar loop over the rule that edtr_amd/rois.py writes out, in fp32 scalars, written for this
    tool and independently of the vectorised restatement (the `match_naive` pattern of the coco goldens);
  * fp64 `F.grid_sample(align_corners=True)` averaged over the samples, for boxes whose samples all lie inside [0, W - 1] x [0, H - 1],
    where roi_align's interpolation and grid_sample's coincide;
  * 2000 random boxes for the level mapper from the first seed for which canonical_level + log2(s / canonical_scale) is at least 1e-3
    from an integer for every box, with their levels worked out in fp64; and hand-built boxes whose levels are exact.

Only arrays go into the file, and the archive is written with fixed time stamps: the same inputs give the same bytes.

    python tools/make_proposals_goldens.py [--out tests/golden/proposals.npz]       (needs the reference tree; see tools/ref_import.py)
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

from make_boxes_goldens import install_detection_stubs, naive_batched_nms  # noqa: E402
from make_labels_goldens import write_npz  # noqa: E402

SEED = 20271
F = np.float32
# (tag, padded (h, w), grid sizes, sizes, aspect ratios)
ANCHOR_CASES = [
    ("v2", (64, 96), [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)], ((32,), (64,), (128,), (256,), (512,)), ((0.5, 1.0, 2.0),) * 5),
    ("mobilenet", (64, 96), [(4, 6), (2, 3), (1, 2)], ((32, 64, 128, 256, 512),) * 3, ((0.5, 1.0, 2.0),) * 3),
    ("ragged", (70, 100), [(18, 25), (9, 13), (5, 7)], ((16,), (32,), (64,)), ((0.5, 1.0, 2.0),) * 3),
]
RPN_PADDED, RPN_GRIDS = (64, 96), [(16, 24), (8, 12), (4, 6)]
RPN_SIZES, RPN_RATIOS = ((8,), (16,), (32,)), ((0.5, 1.0, 2.0),) * 3
RPN_IMAGE_SIZES = [(64, 96), (50, 81)]
# (tag, pre_nms_top_n, post_nms_top_n, nms_thresh, score_thresh): the coarsest level has 72 anchors, fewer than either pre_nms_top_n
RPN_CONFIGS = [("a", 100, 50, 0.7, 0.0), ("b", 200, 60, 0.5, 0.5)]


def reference_anchors(frcnn, util, padded, grids, sizes, ratios) -> np.ndarray:
    gen = frcnn.AnchorGenerator(sizes, ratios)
    images = util.ImageList(torch.zeros(1, 3, *padded), [padded])
    with torch.no_grad():
        out = gen(images, [torch.zeros(1, 1, h, w) for h, w in grids])
    assert len(out) == 1 and out[0].dtype == torch.float32
    return out[0].numpy()


def head_outputs(rng, N):
    """what an RPN head emits: logits around 0 with a spread that saturates no sigmoid, deltas of the size a trained head gives, a
    few beyond the exp clamp, a few that shrink a box below min_size"""
    obj, deltas = [], []
    for (h, w), ratio in zip(RPN_GRIDS, RPN_RATIOS):
        A = len(ratio)
        o = rng.normal(0, 2, (N, A, h, w)).astype(F)
        d = rng.normal(0, 0.3, (N, 4 * A, h, w)).astype(F)
        d[:, 2::4] *= 2
        d[:, 3::4] *= 2
        obj.append(o)
        deltas.append(d)
    # the best-scoring anchors of the finest level: one beyond the clamp, one thinner than min_size
    for n in range(N):
        o = obj[0][n]
        a, y, x = np.unravel_index(np.argsort(-o.reshape(-1))[:2], o.shape)
        deltas[0][n, 4 * a[0] + 2, y[0], x[0]] = 6.0
        deltas[0][n, 4 * a[1] + 3, y[1], x[1]] = -12.0
    return obj, deltas


def ulp_gap(p) -> int:
    """the least distance, in units of the last place, between two unequal values of fp32 p > 0"""
    v = np.unique(np.asarray(p, dtype=F)).view(np.int32).astype(np.int64)
    return int(np.diff(v).min()) if v.size > 1 else 1 << 30


def run_filter(frcnn, util, obj, deltas, anchors, pre, post, nms, score):
    ns = types.SimpleNamespace(pre_nms_top_n=lambda: pre, post_nms_top_n=lambda: post, nms_thresh=nms, score_thresh=score, min_size=1e-3)
    ns._get_top_n_idx = types.MethodType(frcnn.RegionProposalNetwork._get_top_n_idx, ns)
    coder = util.BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
    N = obj[0].shape[0]
    with torch.no_grad():
        t_obj, t_del = [torch.from_numpy(o) for o in obj], [torch.from_numpy(d) for d in deltas]
        per_level = [o[0].numel() for o in t_obj]
        flat_obj, flat_del = frcnn.concat_box_prediction_layers(t_obj, t_del)
        decoded = coder.decode(flat_del, [torch.from_numpy(anchors)] * N).view(N, -1, 4)
        boxes, scores = frcnn.RegionProposalNetwork.filter_proposals(ns, decoded, flat_obj, RPN_IMAGE_SIZES, per_level)
    return flat_obj.reshape(N, -1).numpy(), decoded.numpy(), [b.numpy() for b in boxes], [s.numpy() for s in scores]


# ---- RoIAlign: the rule, one sample at a time ----------------------------------------------------------------------------------------
def roi_align_scalar(features, scales, k_min, k_max, rois, batch, P, S, s0=224.0, k0=4.0):
    """fp32 scalars throughout; `features`: per level [N, C, H, W]; s0, k0: the mapper's canonical scale and level"""
    C = features[0].shape[1]
    out = np.zeros((len(rois), C, P, P), dtype=F)
    for r, (box, n) in enumerate(zip(rois, batch)):
        x1, y1, x2, y2 = (F(v) for v in box)
        level = 0
        if len(features) > 1:
            s = np.sqrt(F(F(x2 - x1) * F(y2 - y1)))
            t = np.floor(F(F(F(k0) + np.log2(F(s / F(s0)))) + F(1e-6)))
            level = int(min(max(t, k_min), k_max)) - k_min
        f = features[level][n]
        H, W = f.shape[-2:]
        sc = F(scales[level])
        x1, y1, x2, y2 = F(x1 * sc), F(y1 * sc), F(x2 * sc), F(y2 * sc)
        roi_w, roi_h = max(F(x2 - x1), F(1)), max(F(y2 - y1), F(1))
        bin_w, bin_h = F(roi_w / F(P)), F(roi_h / F(P))
        for c in range(C):
            for ph in range(P):
                for pw in range(P):
                    total = F(0)
                    for iy in range(S):
                        y = F(F(y1 + F(F(ph) * bin_h)) + F(F(F(F(iy) + F(0.5)) * bin_h) / F(S)))
                        for ix in range(S):
                            x = F(F(x1 + F(F(pw) * bin_w)) + F(F(F(F(ix) + F(0.5)) * bin_w) / F(S)))
                            if y < -1 or y > H or x < -1 or x > W:
                                continue
                            yy, xx = max(y, F(0)), max(x, F(0))
                            y_low, x_low = int(yy), int(xx)
                            if y_low >= H - 1:
                                y_high = y_low = H - 1
                                yy = F(y_low)
                            else:
                                y_high = y_low + 1
                            if x_low >= W - 1:
                                x_high = x_low = W - 1
                                xx = F(x_low)
                            else:
                                x_high = x_low + 1
                            ly, lx = F(yy - F(y_low)), F(xx - F(x_low))
                            hy, hx = F(F(1) - ly), F(F(1) - lx)
                            v = F(F(F(F(hy * hx) * f[c, y_low, x_low]) + F(F(hy * lx) * f[c, y_low, x_high])) + F(F(ly * hx) * f[c, y_high, x_low]))
                            v = F(v + F(F(ly * lx) * f[c, y_high, x_high]))
                            total = F(total + v)
                    out[r, c, ph, pw] = F(total / F(S * S))
    return out


def roi_cases(rng, image_sizes, per_image):
    """rois in image coordinates: random ones, and per image those that leave the image on each side, lie wholly outside it, are
    narrower than a feature pixel, and end exactly at the image's edge"""
    rois = []
    for (h, w) in image_sizes:
        x1, y1 = rng.uniform(-4, w * 0.8, per_image), rng.uniform(-4, h * 0.8, per_image)
        b = np.stack([x1, y1, x1 + rng.uniform(2, w * 0.9, per_image), y1 + rng.uniform(2, h * 0.9, per_image)], axis=1)
        hand = [[-30, 5, 12, 30], [w - 10, 5, w + 40, 30], [5, -30, 30, 12], [5, h - 10, 30, h + 40],         # straddling each border
                [-200, -200, -120, -150], [w + 100, h + 100, w + 160, h + 190],                               # wholly outside
                [10.2, 11.1, 10.5, 11.3], [w - 20, h - 20, w, h], [0, 0, w, h]]                               # thin; ending at the edge
        rois.append(np.concatenate([b, np.array(hand, dtype=np.float64)]).astype(F))
    return rois


def interior_cases(rng, H, W, n, P, S):
    """boxes in the coordinates of an H x W map (scale 1) whose every sample lies inside [0, W - 1] x [0, H - 1]"""
    x1, y1 = rng.uniform(0.5, W * 0.5, n), rng.uniform(0.5, H * 0.5, n)
    x2, y2 = np.minimum(x1 + rng.uniform(1.5, W * 0.5, n), W - 1.5), np.minimum(y1 + rng.uniform(1.5, H * 0.5, n), H - 1.5)
    return np.stack([x1, y1, x2, y2], axis=1).astype(F)


def grid_sample_pool(feature, rois, P, S):
    """fp64: the mean over S x S samples per bin of F.grid_sample(align_corners=True) at roi_align's sample points"""
    f = torch.from_numpy(feature.astype(np.float64))[None]                   # [1, C, H, W]
    H, W = f.shape[-2:]
    out = []
    for box in rois.astype(np.float64):
        x1, y1, x2, y2 = box
        bw, bh = max(x2 - x1, 1.0) / P, max(y2 - y1, 1.0) / P
        t = (np.arange(P * S) // S) + ((np.arange(P * S) % S) + 0.5) / S          # ph + (i + 0.5) / S
        ys, xs = y1 + t * bh, x1 + t * bw
        assert ys.min() >= 0 and ys.max() <= H - 1 and xs.min() >= 0 and xs.max() <= W - 1
        gy, gx = np.meshgrid(2 * ys / (H - 1) - 1, 2 * xs / (W - 1) - 1, indexing="ij")
        grid = torch.from_numpy(np.stack([gx, gy], axis=-1))[None]
        v = torch.nn.functional.grid_sample(f, grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
        out.append(v.reshape(-1, P, S, P, S).mean(dim=(2, 4)).numpy())
    return np.stack(out)


def mapper_cases(k_lo=-1.0, k_hi=7.0):
    """2000 boxes whose level value 4 + log2(s / 224) is uniform in [k_lo, k_hi] and at least 1e-3 from an integer"""
    for seed in range(SEED, SEED + 4096):
        rng = np.random.default_rng([seed, 2000])
        k = rng.uniform(k_lo, k_hi, 2000)
        s = 224.0 * 2.0 ** (k - 4.0)
        aspect = rng.uniform(0.5, 2.0, 2000)
        w, h = s * np.sqrt(aspect), s / np.sqrt(aspect)
        x1, y1 = rng.uniform(0, 64, 2000), rng.uniform(0, 64, 2000)
        b = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(F).astype(np.float64)
        value = 4.0 + np.log2(np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 224.0)
        if np.abs(value - np.round(value)).min() >= 1e-3:
            return seed, b.astype(F), value
    raise SystemExit("no seed gives 2000 boxes away from every level boundary")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "proposals.npz"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    install_detection_stubs()
    import importlib
    util = importlib.import_module("model.util")
    frcnn = importlib.import_module("model.faster_rcnn")
    assert frcnn.box_ops.batched_nms is naive_batched_nms
    from edtr_amd import boxes as project_boxes, rois as project_rois

    out = {}
    # AnchorGenerator
    for tag, padded, grids, sizes, ratios in ANCHOR_CASES:
        out.update({f"anchors_{tag}_padded": np.array(padded, dtype=np.int32), f"anchors_{tag}_grids": np.array(grids, dtype=np.int32),
                    f"anchors_{tag}_sizes": np.array(sizes, dtype=np.float64), f"anchors_{tag}_ratios": np.array(ratios, dtype=np.float64),
                    f"anchors_{tag}": reference_anchors(frcnn, util, padded, grids, sizes, ratios)})

    # concat_box_prediction_layers, BoxCoder.decode, filter_proposals
    anchors = reference_anchors(frcnn, util, RPN_PADDED, RPN_GRIDS, RPN_SIZES, RPN_RATIOS)
    N = len(RPN_IMAGE_SIZES)
    for seed in range(SEED, SEED + 1024):
        obj, deltas = head_outputs(np.random.default_rng([seed, N]), N)
        runs, clear = {}, all(np.unique(o[n]).size == o[n].size for o in obj for n in range(N))
        for tag, pre, post, nms, score in RPN_CONFIGS:
            runs[tag] = run_filter(frcnn, util, obj, deltas, anchors, pre, post, nms, score)
            cand = project_rois.candidates_reference(obj, deltas, project_rois.select_reference(obj, pre), RPN_IMAGE_SIZES, RPN_PADDED,
                                                     RPN_SIZES, RPN_RATIOS, pre, score)
            for n in range(N):
                clear &= project_boxes.cancellation_ratio(runs[tag][2][n], RPN_IMAGE_SIZES[n]) <= 40 and ulp_gap(cand[n][1]) > 4
                clear &= len(runs[tag][2][n]) > 0
        if clear:
            break
    else:
        raise SystemExit(f"no seed in [{SEED}, {SEED + 1024}) gives a well-conditioned proposal case")
    out.update(rpn_seed=np.array(seed, dtype=np.int64), rpn_padded=np.array(RPN_PADDED, dtype=np.int32),
               rpn_image_sizes=np.array(RPN_IMAGE_SIZES, dtype=np.int32), rpn_sizes=np.array(RPN_SIZES, dtype=np.float64),
               rpn_ratios=np.array(RPN_RATIOS, dtype=np.float64), rpn_flat_objectness=runs["a"][0], rpn_decoded=runs["a"][1])
    for l in range(len(RPN_GRIDS)):
        out[f"rpn_objectness{l}"], out[f"rpn_deltas{l}"] = obj[l], deltas[l]
    for tag, pre, post, nms, score in RPN_CONFIGS:
        out[f"rpn_{tag}_top_n"] = np.array([pre, post], dtype=np.int32)
        out[f"rpn_{tag}_thresh"] = np.array([nms, score], dtype=np.float64)
        for n in range(N):
            out[f"rpn_{tag}_boxes{n}"], out[f"rpn_{tag}_scores{n}"] = runs[tag][2][n], runs[tag][3][n]
        print(f"rpn {tag}: seed {seed}, {[len(b) for b in runs[tag][2]]} proposals kept")

    # RoIAlign: the scalar loop on three levels and two images
    rng = np.random.default_rng([SEED, 7])
    image_sizes = [(64, 96), (50, 81)]
    feats = [rng.normal(0, 1, (2, 3, h, w)).astype(F) for h, w in [(16, 24), (8, 12), (4, 6)]]
    rois = roi_cases(rng, image_sizes, 12)
    flat = np.concatenate(rois)
    batch = np.concatenate([np.full(len(r), n) for n, r in enumerate(rois)])
    # canonical scale 56, so that rois inside a 64 x 96 image reach all three levels; none within 1e-3 of a level boundary
    d = flat.astype(np.float64)
    value = 4.0 + np.log2(np.maximum(np.sqrt((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])), 1e-30) / 56.0)
    assert np.abs(value - np.round(value)).min() >= 1e-3 and set(np.clip(np.floor(value), 2, 4).astype(int)) == {2, 3, 4}
    out.update(roi_image_sizes=np.array(image_sizes, dtype=np.int32), roi_rois=flat, roi_batch=batch.astype(np.int32),
               roi_canonical=np.array([56.0, 4.0]), roi_out=roi_align_scalar(feats, [0.25, 0.125, 0.0625], 2, 4, flat, batch, 7, 2, 56.0, 4.0),
               roi_out_single=roi_align_scalar(feats[:1], [0.25], 2, 2, flat, batch, 3, 3))
    for l, f in enumerate(feats):
        out[f"roi_features{l}"] = f

    # RoIAlign against fp64 grid_sample on interior boxes
    H, W = 25, 42
    feature = rng.normal(0, 1, (2, H, W)).astype(F)
    inner = interior_cases(rng, H, W, 40, 7, 2)
    gs = grid_sample_pool(feature, inner, 7, 2)
    mine = project_rois.roi_align_reference([feature[None]], [inner], [(H, W)], 7, 2)
    print(f"grid_sample: max |restatement - fp64| over {len(inner)} interior boxes = {np.abs(mine - gs).max():.3e}")
    out.update(gs_feature=feature, gs_rois=inner, gs_out=gs)

    # the level mapper
    map_seed, map_rois, value = mapper_cases()
    hand = [[10, 10, 10 + s, 10 + s] for s in (56, 112, 224, 448, 896)] + [[5, 5, 5.5, 5.25], [0, 0, 30000, 20000]]
    out.update(map_seed=np.array(map_seed, dtype=np.int64), map_rois=map_rois, map_value=value, map_hand_rois=np.array(hand, dtype=F),
               map_hand_value=np.array([2, 3, 4, 5, 6, -100, 100], dtype=np.float64))
    print(f"mapper: seed {map_seed}, least distance from an integer {np.abs(value - np.round(value)).min():.2e}")

    write_npz(args.out, out)
    print(f"wrote {args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
