"""Region proposals and RoI pooling on the device: the two non-learned steps inside the reference's Faster R-CNN that `boxes` did not
cover.  `RegionProposalNetwork.forward` in eval mode (model/faster_rcnn.py:2068-2134, 2199-2213, over `AnchorGenerator`, :514-589)
turns the RPN head's outputs into at most `post_nms_top_n` proposals per image, and `MultiScaleRoIAlign(['0', '1', '2', '3'], 7, 2)`
pools every proposal from the feature level its size selects.  The reference imports both from compiled torchvision operators
(model/faster_rcnn.py:9), which do not exist on this stack.  With them a user can put the detector together from its learned parts —
backbone + FPN, `RPNHead`, box head and predictor, all plain torch and all outside this project — and this project's launches:
`proposals` and `roi_align` here, `boxes.detections` and `boxes.resize_boxes`; `assemble_detector` does exactly that.
`roi_align` is differentiable in its features (`roi_align_backward`, a deterministic gather: one writer per word, a fixed summation
order, no atomics), so `assemble_training_detector` puts the same parts together for the reference's "Train detnet" step
(main/det/train_edtr.py:203-241) with `targets`' launches and losses.

Three layers, as in `boxes`, `coco` and `cls`:
  * `anchors`, `rpn_select`, `rpn_candidates`, `proposals`, `roi_align`, `roi_align_backward`, `assemble_detector`,
    `assemble_training_detector`: thin wrappers over the launches of
    include/edtr_hip.h "Region proposals and RoI pooling" (kernels in csrc/rois.hip; torch tensors on the device, the caller's stream);
  * `*_reference`: the numpy restatement of each.  They are the NORMATIVE definition: the kernels are tested against them — by equality
    wherever neither `exp` (decoding, sigmoid) nor `log2` (the level of a roi) enters — and they against the reference's own
    `AnchorGenerator`, `concat_box_prediction_layers`, `BoxCoder.decode` and `filter_proposals` (tests/golden/proposals.npz);
  * host-side parameter code: `cell_anchors`, `level_table`, `level_scales`.

The head's outputs are read as the head writes them: per level objectness [N, A, H, W] and bbox_deltas [N, 4 A, H, W] with channel
4 a + c, fp32, fp16 or bf16 (widened exactly).  No `concat_box_prediction_layers` copy is made and the proposal path reads no anchor
tensor.  The LOGICAL index of an element of a level is i = (y W + x) A + a, the row that copy would have moved it to; ties are
resolved by it.

RoIAlign is pinned to the RULE written out under `roi_align_reference`, not to torchvision's binary, which is not installed where the
goldens are made (as `boxes` pins NMS).  The rule is torchvision's CPU kernel with aligned=False and a positive sampling ratio, each
step one rounded fp32 operation; the goldens hold a per-sample scalar loop of it written independently of the vectorised restatement,
and fp64 `F.grid_sample(align_corners=True)` for boxes whose samples all lie inside the feature map, where the two rules coincide.
NMS inside `proposals` is `boxes.batched_nms`, by the probability and per level, the reference's rule."""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import numpy as np

from . import boxes as _boxes
from .boxes import BBOX_XFORM_CLIP, F32

RPN_MAX_LEVELS = 8                      # EDTR_RPN_MAX_LEVELS: with RPN_MAX_PRE_NMS per level the NMS sees at most NMS_MAX_BOXES boxes
RPN_MAX_PRE_NMS = 4096                  # EDTR_RPN_MAX_PRE_NMS: the selection of one level is ranked in LDS
ROI_MAX_TAPS = 64                       # EDTR_ROI_MAX_TAPS: output_size * sampling_ratio
ROI_BWD_MAX_P = 16                      # EDTR_ROI_BWD_MAX_P: output_size of the backward (a chunk's staged gradient must fit the LDS)
LIMIT = 1 << 24
# fasterrcnn_resnet50_fpn_v2 (configs/det/demo.yaml:88-92): one size and three aspect ratios on each of five levels
RPN_SIZES = ((32,), (64,), (128,), (256,), (512,))
RPN_ASPECT_RATIOS = ((0.5, 1.0, 2.0),) * 5
LEVEL_EPS = 1e-6                        # LevelMapper's eps


# ----------------------------------------------------------------------------------------------------------------------------------
# host-side parameters
# ----------------------------------------------------------------------------------------------------------------------------------
def _host(v) -> np.ndarray:
    """numpy array or torch tensor (any float dtype, any device) as a contiguous fp32 numpy array; 16-bit values widen exactly"""
    if hasattr(v, "detach"):
        v = v.detach().float().cpu().numpy()
    return np.ascontiguousarray(v, dtype=F32)


def _level_list(v) -> list:
    return list(v.values()) if isinstance(v, dict) else list(v)


def cell_anchors(sizes, aspect_ratios) -> list:
    """`AnchorGenerator.generate_anchors` per level, in fp32 as it runs: h = sqrt(ratio), w = 1 / h, ws = w x sizes and hs = h x sizes
    flattened ratio-major, round_half_even(stack(-ws, -hs, ws, hs) / 2).  [fp32 [A_l, 4]] with A_l = ratios x sizes."""
    if len(sizes) != len(aspect_ratios) or not len(sizes):
        raise ValueError(f"sizes and aspect_ratios take one tuple per level each, got {len(sizes)} and {len(aspect_ratios)}")
    out = []
    for size, ratio in zip(sizes, aspect_ratios):
        s, r = np.asarray(size, dtype=F32).reshape(-1), np.asarray(ratio, dtype=F32).reshape(-1)
        if not s.size or not r.size:
            raise ValueError("every level takes at least one size and one aspect ratio")
        h_ratios = np.sqrt(r)
        w_ratios = F32(1) / h_ratios
        ws, hs = (w_ratios[:, None] * s[None, :]).reshape(-1), (h_ratios[:, None] * s[None, :]).reshape(-1)
        out.append(np.round(np.stack([-ws, -hs, ws, hs], axis=1) / F32(2)).astype(F32))
    return out


def level_table(grid_sizes, image_size, cells) -> list:
    """[(H, W, A, stride_h, stride_w)] per level: the strides are image_size // grid_size per axis (`AnchorGenerator.forward`), with
    ``image_size`` the padded batch extent (h, w).  Checks the bounds of the launches."""
    grid_sizes = [tuple(int(v) for v in g) for g in grid_sizes]
    if len(grid_sizes) != len(cells):
        raise ValueError(f"{len(grid_sizes)} feature levels for {len(cells)} levels of sizes / aspect_ratios")
    if not 0 < len(grid_sizes) <= RPN_MAX_LEVELS:
        raise ValueError(f"between 1 and {RPN_MAX_LEVELS} levels, got {len(grid_sizes)}")
    ih, iw = int(image_size[0]), int(image_size[1])
    table = []
    for (H, W), cell in zip(grid_sizes, cells):
        if H <= 0 or W <= 0 or ih <= 0 or iw <= 0:
            raise ValueError(f"extents must be positive, got a {H} x {W} grid on a {ih} x {iw} batch")
        A, sh, sw = int(cell.shape[0]), ih // H, iw // W
        if H * W * A >= LIMIT or H * sh >= LIMIT or W * sw >= LIMIT:
            raise ValueError(f"a level takes fewer than 2^24 anchors and coordinates below 2^24, got {H} x {W} x {A} at stride {sh} x {sw}")
        table.append((H, W, A, sh, sw))
    return table


def level_scales(feature_sizes, image_sizes):
    """`MultiScaleRoIAlign.setup_scales`: ([scale_l], k_min, k_max) with scale_l = 2 ** round(log2(H_l / H_img)), H_img the largest
    image height, the widths giving the same value (ValueError otherwise), k_min = -log2(scale_0) and k_max = -log2(scale_last).
    With more than one level the mapper addresses level t - k_min for t up to k_max, so k_max - k_min + 1 levels must exist
    (ValueError otherwise; torchvision raises an index error on the first roi mapped past the last level)."""
    mh, mw = max(int(s[0]) for s in image_sizes), max(int(s[1]) for s in image_sizes)
    scales = []
    for H, W in feature_sizes:
        if H <= 0 or W <= 0 or mh <= 0 or mw <= 0:
            raise ValueError(f"extents must be positive, got a {H} x {W} level for a {mh} x {mw} image")
        eh, ew = round(math.log2(float(H) / float(mh))), round(math.log2(float(W) / float(mw)))
        if eh != ew:
            raise ValueError(f"a {H} x {W} level of a {mh} x {mw} image has no single scale: 2^{eh} by height, 2^{ew} by width")
        scales.append(2.0 ** eh)
    k_min, k_max = int(-math.log2(scales[0])), int(-math.log2(scales[-1]))
    if len(scales) > 1 and k_max - k_min != len(scales) - 1:
        raise ValueError(f"{len(scales)} levels at scales {scales}: the mapper's levels {k_min} .. {k_max} would not all exist")
    return scales, k_min, k_max


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative)
# ----------------------------------------------------------------------------------------------------------------------------------
def anchors_reference(grid_sizes, image_size, sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS) -> np.ndarray:
    """`AnchorGenerator.forward` for one padded batch extent ``image_size`` = (h, w): fp32 [sum H_l W_l A_l, 4], level after level.
    Anchor i = (y W + x) A + a of a level is (float(x stride_w) + cell[a][0], float(y stride_h) + cell[a][1], float(x stride_w) +
    cell[a][2], float(y stride_h) + cell[a][3]) with `cell_anchors` and the strides of `level_table`: the shift is an integer, its
    conversion exact, so each value is one rounded fp32 sum."""
    cells = cell_anchors(sizes, aspect_ratios)
    out = []
    for (H, W, A, sh, sw), cell in zip(level_table(grid_sizes, image_size, cells), cells):
        sx, sy = (np.arange(W, dtype=np.int64) * sw).astype(F32), (np.arange(H, dtype=np.int64) * sh).astype(F32)
        shift = np.stack(np.broadcast_arrays(sx[None, :], sy[:, None], sx[None, :], sy[:, None]), axis=2).reshape(-1, 1, 4)
        out.append((shift + cell[None]).reshape(-1, 4).astype(F32))
    return np.concatenate(out)


def _check_head(objectness, bbox_deltas, cells):
    """shapes of the RPN head's outputs (numpy arrays or torch tensors): returns N and the grid sizes"""
    if len(objectness) != len(cells) or (bbox_deltas is not None and len(bbox_deltas) != len(cells)):
        raise ValueError(f"{len(objectness)} levels of objectness for {len(cells)} levels of sizes / aspect_ratios")
    N = int(objectness[0].shape[0]) if getattr(objectness[0], "ndim", 0) == 4 else -1
    for l, cell in enumerate(cells):
        o, A = objectness[l], int(cell.shape[0])
        if getattr(o, "ndim", 0) != 4 or int(o.shape[0]) != N or int(o.shape[1]) != A:
            raise ValueError(f"objectness of level {l} is [N, {A}, H, W], got {tuple(getattr(o, 'shape', ()))}")
        if bbox_deltas is not None and tuple(bbox_deltas[l].shape) != (N, 4 * A, int(o.shape[2]), int(o.shape[3])):
            raise ValueError(f"bbox_deltas of level {l} is {(N, 4 * A, int(o.shape[2]), int(o.shape[3]))}, got {tuple(bbox_deltas[l].shape)}")
    if not 0 < N <= 65535:
        raise ValueError(f"between 1 and 65535 images, got {N}")
    return N, [(int(o.shape[2]), int(o.shape[3])) for o in objectness]


def _check_top_n(pre_nms_top_n, post_nms_top_n=1):
    if int(pre_nms_top_n) <= 0 or int(post_nms_top_n) <= 0:
        raise ValueError(f"pre_nms_top_n and post_nms_top_n must be positive, got {pre_nms_top_n} and {post_nms_top_n}")
    if int(pre_nms_top_n) > RPN_MAX_PRE_NMS:
        raise ValueError(f"pre_nms_top_n is at most {RPN_MAX_PRE_NMS}, got {pre_nms_top_n}")
    return int(pre_nms_top_n), int(post_nms_top_n)


def select_reference(objectness, pre_nms_top_n: int = 1000) -> np.ndarray:
    """`_get_top_n_idx` without its offsets, THE RULE: for every image and level the min(pre_nms_top_n, H W A) elements with the greatest
    `boxes.score_keys` (every NaN one largest key, -0.0 and 0.0 one key), equal keys by ascending logical index i = (y W + x) A + a,
    in that order.  That is `torch.topk` wherever torch defines the order, and a fixed answer where it does not (among equal values
    and NaNs, see `cls` on ties).  ``objectness``: per level [N, A, H, W].  int32 [N, sum take_l] of level-local logical indices."""
    pre, _ = _check_top_n(pre_nms_top_n)
    out = []
    for o in _level_list(objectness):
        o = _host(o)
        flat = o.transpose(0, 2, 3, 1).reshape(o.shape[0], -1)
        out.append(np.stack([_boxes.rank_order_reference(row)[:min(pre, flat.shape[1])] for row in flat]))
    return np.concatenate(out, axis=1).astype(np.int32)


def sigmoid_reference(x, dtype=F32, exp=np.exp) -> np.ndarray:
    """1 / (1 + exp(-x)), each step rounded"""
    x = np.asarray(x, dtype=dtype)
    with np.errstate(over="ignore"):
        return (dtype(1) / (dtype(1) + exp(-x).astype(dtype))).astype(dtype)


def torch_exp(x) -> np.ndarray:
    """torch's CPU exp on a numpy array: the exponential the reference's own `BoxCoder.decode` runs.  Handed to the restatements as
    ``exp``, it makes them meet the reference's recorded boxes bit for bit; numpy's exp differs from it in the last bit for 39 % of
    unit-normal arguments, which moves a corner by an ulp or two."""
    import torch
    return torch.exp(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def candidates_reference(objectness, bbox_deltas, selected, image_sizes, padded_size, sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS,
                         pre_nms_top_n: int = 1000, score_thresh: float = 0.0, min_size: float = 1e-3,
                         bbox_xform_clip: float = BBOX_XFORM_CLIP, exp=np.exp):
    """What `filter_proposals` hands its NMS, per image [(boxes fp32 [m, 4], probs fp32 [m], levels int32 [m])].  For every element of
    ``selected`` (`select_reference`), in level order and then selection order:
      * the anchor of its logical index (`anchors_reference`);
      * `boxes.decode_reference` of its four deltas (channels 4 a + c at its cell) with weights (1, 1, 1, 1) and the log(1000 / 16) clamp;
      * prob = `sigmoid_reference` of its logit;
      * the corners clamped to [0, w] x [0, h] of that image's (h, w);
      * kept iff x2 - x1 >= min_size and y2 - y1 >= min_size and prob >= score_thresh (a NaN fails).
    ``exp``: the exponential of the decoding and the sigmoid, numpy's by default (`torch_exp`)."""
    objectness, bbox_deltas = [_host(o) for o in _level_list(objectness)], [_host(d) for d in _level_list(bbox_deltas)]
    cells = cell_anchors(sizes, aspect_ratios)
    N, grids = _check_head(objectness, bbox_deltas, cells)
    pre, _ = _check_top_n(pre_nms_top_n)
    table = level_table(grids, padded_size, cells)
    anchors = anchors_reference(grids, padded_size, sizes, aspect_ratios)
    selected = np.asarray(selected)
    takes = [min(pre, H * W * A) for H, W, A, _, _ in table]
    if selected.shape != (N, sum(takes)) or len(image_sizes) != N:
        raise ValueError(f"selected is [{N}, {sum(takes)}] and image_sizes has {N} entries, got {selected.shape} and {len(image_sizes)}")
    out = []
    for n in range(N):
        rows, logit, anc, lvl = [], [], [], []
        col = start = 0
        for l, ((H, W, A, _, _), take) in enumerate(zip(table, takes)):
            idx = selected[n, col:col + take].astype(np.int64)
            p, a = idx // A, idx % A
            d = bbox_deltas[l][n].reshape(A, 4, H * W)
            rows.append(d[a, :, p])
            logit.append(objectness[l][n].reshape(A, H * W)[a, p])
            anc.append(anchors[start + idx])
            lvl.append(np.full(take, l, dtype=np.int32))
            col, start = col + take, start + H * W * A
        rows, logit, anc, lvl = np.concatenate(rows), np.concatenate(logit), np.concatenate(anc), np.concatenate(lvl)
        b = _boxes.decode_reference(rows, anc, (1.0, 1.0, 1.0, 1.0), bbox_xform_clip, exp=exp)[:, 0]
        prob = sigmoid_reference(logit, exp=exp)
        h, w = F32(image_sizes[n][0]), F32(image_sizes[n][1])
        b = np.stack([_boxes._clamp(b[:, 0], w), _boxes._clamp(b[:, 1], h), _boxes._clamp(b[:, 2], w), _boxes._clamp(b[:, 3], h)], axis=1)
        with np.errstate(invalid="ignore"):
            flag = (b[:, 2] - b[:, 0] >= F32(min_size)) & (b[:, 3] - b[:, 1] >= F32(min_size)) & (prob >= F32(score_thresh))
        out.append((b[flag], prob[flag], lvl[flag]))
    return out


def nms_stage_reference(candidates, nms_thresh: float = 0.7, post_nms_top_n: int = 1000, probs=None):
    """The last step of `filter_proposals`: per image `boxes.batched_nms_reference` of the candidates by PROBABILITY with the level
    as the label (not by the logit: across levels the two orders differ where sigmoid saturates), the first ``post_nms_top_n`` kept.
    ``probs``: None, or per image the probabilities to rank by and return in place of the candidates' own (a test hands the device's
    in, so that one ulp of exp cannot flip an order).  [(boxes [k, 4], scores [k])]."""
    out = []
    for n, (b, p, lvl) in enumerate(candidates):
        p = p if probs is None else np.asarray(probs[n], dtype=F32)
        if p.shape != (b.shape[0],):
            raise ValueError(f"image {n}: {p.shape} probabilities for {b.shape[0]} candidates")
        keep = _boxes.batched_nms_reference(b, p, lvl, nms_thresh)[:int(post_nms_top_n)] if b.shape[0] else np.zeros(0, dtype=np.int64)
        out.append((b[keep], p[keep]))
    return out


def proposals_reference(objectness, bbox_deltas, image_sizes, padded_size, *, sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS,
                        pre_nms_top_n: int = 1000, post_nms_top_n: int = 1000, nms_thresh: float = 0.7, score_thresh: float = 0.0,
                        min_size: float = 1e-3, exp=np.exp):
    """`RegionProposalNetwork.forward` in eval mode from the head's outputs: `select_reference`, `candidates_reference`,
    `nms_stage_reference`.  [(boxes fp32 [k, 4], scores fp32 [k])] per image."""
    pre, post = _check_top_n(pre_nms_top_n, post_nms_top_n)
    selected = select_reference(objectness, pre)
    cand = candidates_reference(objectness, bbox_deltas, selected, image_sizes, padded_size, sizes, aspect_ratios, pre, score_thresh, min_size,
                               exp=exp)
    return nms_stage_reference(cand, nms_thresh, post)


def roi_levels_reference(rois, k_min: int, k_max: int, canonical_scale: float = 224.0, canonical_level: float = 4.0) -> np.ndarray:
    """`LevelMapper` in fp32: s = sqrt((x2 - x1) (y2 - y1)); t = floor((canonical_level + log2(s / canonical_scale)) + 1e-6), clamped to
    [k_min, k_max] (NaN: k_min); the level is t - k_min.  int64 [K].  log2 is the one step two implementations may round differently,
    so a level is certain only where canonical_level + log2(s / canonical_scale) is not within rounding of an integer."""
    r = np.asarray(rois, dtype=F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = np.sqrt((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]))
        t = np.floor((F32(canonical_level) + np.log2(s / F32(canonical_scale)).astype(F32)) + F32(LEVEL_EPS))
        t = np.where(~(t >= F32(k_min)), F32(k_min), np.where(t > F32(k_max), F32(k_max), t))
    return t.astype(np.int64) - int(k_min)


def _check_pool(output_size, sampling_ratio):
    P, S = int(output_size), int(sampling_ratio)
    if P <= 0 or S <= 0:
        raise ValueError(f"output_size and sampling_ratio must be positive (the adaptive ratio is not provided), got {output_size} and {sampling_ratio}")
    if P * S > ROI_MAX_TAPS:
        raise ValueError(f"output_size * sampling_ratio is at most {ROI_MAX_TAPS}, got {P} * {S}")
    return P, S


def _check_features(features, rois, image_sizes):
    feats = _level_list(features)
    if not 0 < len(feats) <= RPN_MAX_LEVELS:
        raise ValueError(f"between 1 and {RPN_MAX_LEVELS} feature levels, got {len(feats)}")
    if any(getattr(f, "ndim", 0) != 4 or tuple(f.shape[:2]) != tuple(feats[0].shape[:2]) for f in feats):
        raise ValueError("features are [N, C, H_l, W_l] per level with one N and one C")
    N = int(feats[0].shape[0])
    if len(rois) != N or len(image_sizes) != N or not 0 < N <= 65535:
        raise ValueError(f"{N} images in the features (1 to 65535), {len(rois)} lists of rois and {len(image_sizes)} image sizes")
    if any(getattr(r, "ndim", 0) != 2 or r.shape[1] != 4 for r in rois):
        raise ValueError("rois are [k_i, 4] per image")
    return feats, N


def _taps(start, bin_size, P: int, S: int, extent: int):
    """one axis of roi_align's sampling for [K] rois: (valid, low, high, l, h), each [K, P, S]"""
    ph, i = np.arange(P, dtype=F32)[None, :, None], np.arange(S, dtype=F32)[None, None, :]
    start, bin_size = start[:, None, None], bin_size[:, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((start + ph * bin_size) + ((i + F32(0.5)) * bin_size) / F32(S)).astype(F32)
        valid = (v >= F32(-1)) & (v <= F32(extent))
        v = np.where(valid, np.where(v <= 0, F32(0), v), F32(0))
    low = v.astype(np.int64)
    edge = low >= extent - 1
    low = np.where(edge, extent - 1, low)
    high = np.where(edge, extent - 1, low + 1)
    v = np.where(edge, low.astype(F32), v)
    l = (v - low.astype(F32)).astype(F32)
    return valid, low, high, l, (F32(1) - l).astype(F32)


def roi_align_reference(features, rois, image_sizes, output_size: int = 7, sampling_ratio: int = 2, canonical_scale: float = 224.0,
                        canonical_level: float = 4.0) -> np.ndarray:
    """`MultiScaleRoIAlign`, THE RULE.  ``features``: per level [N, C, H_l, W_l]; ``rois``: per image [k_i, 4] in image coordinates;
    fp32 [sum k_i, C, P, P] in roi order, the rois of image n reading features[..][n].
      * scales, k_min, k_max: `level_scales`; the level of a roi: `roi_levels_reference` (one level: no mapper);
      * roi_align with aligned=False, every step one fp32 operation: x1 .. y2 each times the level's scale; roi_w = max(x2 - x1, 1),
        roi_h alike; bin = roi / P;
      * for output (ph, pw) and iy, ix in [0, S): y = (y1 + ph bin_h) + ((iy + 0.5) bin_h) / S, x alike; a sample with y < -1, y > H,
        x < -1 or x > W (or a NaN coordinate) adds nothing; otherwise y = max(y, 0), y_low = int(y); y_low >= H - 1 gives y_low =
        y_high = H - 1 and y = y_low, otherwise y_high = y_low + 1; ly = y - y_low, hy = 1 - ly, x alike; the sample is
        (((hy hx) v11 + (hy lx) v12) + (ly hx) v21) + (ly lx) v22, added to the running sum with iy outer and ix inner;
      * the output is sum / (S S).  No product is contracted with a sum."""
    P, S = _check_pool(output_size, sampling_ratio)
    feats, N = _check_features(features, rois, image_sizes)
    feats = [_host(f) for f in feats]
    C = feats[0].shape[1]
    boxes = np.concatenate([np.asarray(_host(r), dtype=F32).reshape(-1, 4) for r in rois]) if len(rois) else np.zeros((0, 4), dtype=F32)
    batch = np.concatenate([np.full(int(r.shape[0]), n, dtype=np.int64) for n, r in enumerate(rois)])
    out = np.zeros((boxes.shape[0], C, P, P), dtype=F32)
    if not boxes.shape[0]:
        return out
    scales, k_min, k_max = level_scales([f.shape[-2:] for f in feats], image_sizes)
    levels = roi_levels_reference(boxes, k_min, k_max, canonical_scale, canonical_level) if len(feats) > 1 else np.zeros(boxes.shape[0], dtype=np.int64)
    for l, f in enumerate(feats):
        pick = np.nonzero(levels == l)[0]
        if not pick.size:
            continue
        H, W = f.shape[-2:]
        with np.errstate(invalid="ignore", over="ignore"):
            b = (boxes[pick] * F32(scales[l])).astype(F32)
            ew, eh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
            roi_w, roi_h = np.where(ew < 1, F32(1), ew), np.where(eh < 1, F32(1), eh)
            vy, y0, y1, ly, hy = _taps(b[:, 1], (roi_h / F32(P)).astype(F32), P, S, H)
            vx, x0, x1, lx, hx = _taps(b[:, 0], (roi_w / F32(P)).astype(F32), P, S, W)
        k = batch[pick][:, None, None, None]                                            # the image of each roi
        c = np.arange(C)[None, :, None, None]
        total = np.zeros((pick.size, C, P, P), dtype=F32)
        for iy in range(S):
            for ix in range(S):
                def at(yy, xx):
                    return f[k, c, yy[:, None, :, iy, None], xx[:, None, None, :, ix]]
                def wt(a, bb):
                    return (a[:, None, :, iy, None] * bb[:, None, None, :, ix]).astype(F32)
                with np.errstate(invalid="ignore", over="ignore"):
                    val = ((wt(hy, hx) * at(y0, x0) + wt(hy, lx) * at(y0, x1)) + wt(ly, hx) * at(y1, x0)) + wt(ly, lx) * at(y1, x1)
                    ok = (vy[:, None, :, iy, None] & vx[:, None, None, :, ix])
                    total = np.where(ok, (total + val).astype(F32), total)
        out[pick] = total / F32(S * S)
    return out


def _axis_weights(taps, extent: int) -> np.ndarray:
    """a[k][y][ph] of `roi_align_backward_reference` for one axis from its `_taps`: fp32 [K, extent, P]"""
    valid, low, high, l, h = taps
    K, P, S = valid.shape
    a = np.zeros((K, extent, P), dtype=F32)
    kk, pp = np.arange(K)[:, None], np.arange(P)[None, :]
    for i in range(S):                                                  # (k, ph) differ between the elements of one indexed sum
        ok = valid[:, :, i]
        a[kk, low[:, :, i], pp] = (a[kk, low[:, :, i], pp] + np.where(ok, h[:, :, i], F32(0))).astype(F32)
        a[kk, high[:, :, i], pp] = (a[kk, high[:, :, i], pp] + np.where(ok, l[:, :, i], F32(0))).astype(F32)
    return a


def roi_align_backward_reference(grad, feature_shapes, rois, image_sizes, output_size: int = 7, sampling_ratio: int = 2,
                                 canonical_scale: float = 224.0, canonical_level: float = 4.0, dtype: str = "float32") -> list:
    """The gradient of `roi_align_reference` with respect to its features, THE RULE of `roi_align_backward`.  ``grad``: fp32
    [sum k_i, C, P, P]; ``feature_shapes``: per level (N, C, H_l, W_l); returns one fp32 array of that shape per level.  The boxes get
    no gradient, as in torchvision.  For roi k the level, the image, the scaled box and the per-axis tap tables (valid, low, high, l, h
    of the P S positions) are the forward's, by `_taps`.  Every step is one rounded fp32 operation, nothing contracted:
      * g'[c][ph][pw] = grad[k][c][ph][pw] / (S S);
      * a[y][ph]: from +0, for iy = 0 .. S - 1 in order, if tap (ph, iy) is valid: + hy if y_low == y, then + ly if y_high == y (at
        the clamped edge low == high and both are added: l = 0 and h = 1 there); b[x][pw] alike on the other axis;
      * t[ph] = sum_pw b[x][pw] g'[c][ph][pw], pw ascending from +0; contrib_k[c][y][x] = sum_ph a[y][ph] t[ph], ph ascending from +0;
      * out_l[n][c][y][x] = sum_k contrib_k over the rois of image n on level l, k ascending from +0.0; ``dtype`` "float16" /
        "bfloat16" rounds that fp32 sum ONCE, to nearest even (and the array holds the rounded values, widened).
    This is the exact adjoint of `roi_align_reference` in real arithmetic: weights and validity are both separable there.  A term
    whose a or b is exactly zero may be skipped (the device does): a zero times a finite number is a zero, and no sum that starts at
    +0 changes by one, so for finite gradients not a bit differs.  A non-finite ``grad`` is unspecified.  A level, image or pixel that
    no roi touches is +0.0."""
    from . import labels
    P, S = _check_pool(output_size, sampling_ratio)
    shapes = [tuple(int(v) for v in s) for s in _level_list(feature_shapes)]
    if not 0 < len(shapes) <= RPN_MAX_LEVELS or any(len(s) != 4 or s[:2] != shapes[0][:2] for s in shapes):
        raise ValueError("feature_shapes are (N, C, H_l, W_l) per level with one N and one C, for 1 to 8 levels")
    N, C = shapes[0][:2]
    if len(rois) != N or len(image_sizes) != N or not 0 < N <= 65535:
        raise ValueError(f"{N} images in the features (1 to 65535), {len(rois)} lists of rois and {len(image_sizes)} image sizes")
    boxes = np.concatenate([np.asarray(_host(r), dtype=F32).reshape(-1, 4) for r in rois])
    batch = np.concatenate([np.full(int(np.asarray(_host(r)).reshape(-1, 4).shape[0]), n, dtype=np.int64) for n, r in enumerate(rois)])
    K = boxes.shape[0]
    grad = _host(grad)
    if grad.shape != (K, C, P, P):
        raise ValueError(f"grad is [{K}, {C}, {P}, {P}], got {grad.shape}")
    if dtype not in ("float32", "float16", "bfloat16"):
        raise ValueError(f"dtype is float32, float16 or bfloat16, got {dtype!r}")
    out = [np.zeros(s, dtype=F32) for s in shapes]
    if K:
        scales, k_min, k_max = level_scales([s[-2:] for s in shapes], image_sizes)
        levels = roi_levels_reference(boxes, k_min, k_max, canonical_scale, canonical_level) if len(shapes) > 1 else np.zeros(K, dtype=np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            gp = (grad / F32(S * S)).astype(F32)
    for l, (_, _, H, W) in enumerate(shapes):
        pick = np.nonzero(levels == l)[0] if K else np.zeros(0, dtype=np.int64)
        if not pick.size:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            b = (boxes[pick] * F32(scales[l])).astype(F32)
            ew, eh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
            roi_w, roi_h = np.where(ew < 1, F32(1), ew), np.where(eh < 1, F32(1), eh)
            ay = _axis_weights(_taps(b[:, 1], (roi_h / F32(P)).astype(F32), P, S, H), H)
            bx = _axis_weights(_taps(b[:, 0], (roi_w / F32(P)).astype(F32), P, S, W), W)
        for j, k in enumerate(pick):                                    # k ascending: the order of the sum over rois
            ys, xs = np.nonzero(ay[j].any(axis=1))[0], np.nonzero(bx[j].any(axis=1))[0]
            if not ys.size or not xs.size:
                continue
            ys, xs = np.arange(ys[0], ys[-1] + 1), np.arange(xs[0], xs[-1] + 1)    # zero rows inside add +0: no bit changes
            a, bb, g = ay[j][ys], bx[j][xs], gp[k]
            with np.errstate(invalid="ignore", over="ignore"):
                t = np.zeros((C, P, xs.size), dtype=F32)
                for pw in range(P):
                    t = (t + (bb[None, None, :, pw] * g[:, :, pw, None]).astype(F32)).astype(F32)
                contrib = np.zeros((C, ys.size, xs.size), dtype=F32)
                for ph in range(P):
                    contrib = (contrib + (a[None, :, ph, None] * t[:, ph, None, :]).astype(F32)).astype(F32)
                view = out[l][batch[k], :, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
                view[...] = (view + contrib).astype(F32)
    return [labels._round_to(o, dtype) for o in out]


def _np_image(v) -> np.ndarray:
    return v.detach().float().cpu().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=F32)


def _detector_options(kw: dict) -> dict:
    opts = dict(sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS, rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=1000, rpn_nms_thresh=0.7,
                rpn_score_thresh=0.0, rpn_min_size=1e-3, output_size=7, sampling_ratio=2, featmap_names=None, box_score_thresh=0.05,
                box_nms_thresh=0.5, box_detections_per_img=100)
    unknown = set(kw) - set(opts)
    if unknown:
        raise TypeError(f"assemble_detector takes no {sorted(unknown)}; its thresholds are {sorted(opts)}")
    opts.update(kw)
    return opts


def _pooled_levels(features, names):
    """the levels `MultiScaleRoIAlign` pools from: those named (all of them for None), in the features' order"""
    if names is None:
        return _level_list(features)
    return [v for k, v in features.items() if k in names]


def assemble_detector_reference(features_fn, rpn_head, box_head, box_predictor, replay: Optional[dict] = None, trace: Optional[dict] = None,
                                **thresholds):
    """`assemble_detector` through the restatements on the host.  The four learned parts are called with CPU torch tensors; with
    ``replay`` (the ``trace`` of a device run) they are not called at all: their recorded outputs — "features", "batch_shape",
    "image_sizes", "original_sizes", "objectness", "bbox_deltas", "class_logits", "box_regression" — and the device's candidate
    probabilities "probs" take their place, so that each non-learned step is restated from exactly what the device's step was given.
    ``trace``: a dict that receives this flow's own stages."""
    o = _detector_options(thresholds)

    def detnet(images):
        import torch
        tr = {} if trace is None else trace
        if replay is None:
            batch, image_sizes, original_sizes, features = features_fn(images)
            objectness, deltas = rpn_head(list(features.values()))
            batch_shape = tuple(batch.shape[-2:])
        else:
            batch_shape, image_sizes, original_sizes = replay["batch_shape"], replay["image_sizes"], replay["original_sizes"]
            features, objectness, deltas = replay["features"], replay["objectness"], replay["bbox_deltas"]
        features = OrderedDict((k, _host(v)) for k, v in features.items())
        selected = select_reference(objectness, o["rpn_pre_nms_top_n"])
        cand = candidates_reference(objectness, deltas, selected, image_sizes, batch_shape, o["sizes"], o["aspect_ratios"],
                                    o["rpn_pre_nms_top_n"], o["rpn_score_thresh"], o["rpn_min_size"])
        props = nms_stage_reference(cand, o["rpn_nms_thresh"], o["rpn_post_nms_top_n"], None if replay is None else replay.get("probs"))
        rois = [b for b, _ in props]
        pooled = roi_align_reference(_pooled_levels(features, o["featmap_names"]), rois, image_sizes, o["output_size"], o["sampling_ratio"])
        if replay is None:
            with torch.no_grad():
                logits, regression = box_predictor(box_head(torch.from_numpy(pooled)))
        else:
            logits, regression = replay["class_logits"], replay["box_regression"]
        logits, regression = _host(logits), _host(regression)
        tr.update(selected=selected, candidates=cand, proposals=props, pooled=pooled)
        out, start = [], 0
        for n, r in enumerate(rois):
            rows = slice(start, start + r.shape[0])
            start += r.shape[0]
            if not r.shape[0]:
                out.append({"boxes": np.zeros((0, 4), dtype=F32), "scores": np.zeros(0, dtype=F32), "labels": np.zeros(0, dtype=np.int64)})
                continue
            det = _boxes.detections_reference(logits[rows], regression[rows], r, image_sizes[n], o["box_score_thresh"], o["box_nms_thresh"],
                                              o["box_detections_per_img"])
            det["boxes"] = _boxes.resize_boxes_reference(det["boxes"], image_sizes[n], original_sizes[n])
            out.append(det)
        return out

    return detnet


LOSS_NAMES = ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")     # model/faster_rcnn.py:1295-1296, 2221-2226


def _training_options(kw: dict) -> dict:
    from .targets import ROI_WEIGHTS
    opts = dict(sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS, rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=2000, rpn_nms_thresh=0.7,
                rpn_score_thresh=0.0, rpn_min_size=1e-3, rpn_fg_iou_thresh=0.7, rpn_bg_iou_thresh=0.3, rpn_batch_size_per_image=256,
                rpn_positive_fraction=0.5, box_fg_iou_thresh=0.5, box_bg_iou_thresh=0.5, box_batch_size_per_image=512, box_positive_fraction=0.25,
                bbox_reg_weights=ROI_WEIGHTS, output_size=7, sampling_ratio=2, canonical_scale=224.0, canonical_level=4.0, featmap_names=None)
    unknown = set(kw) - set(opts)
    if unknown:
        raise TypeError(f"assemble_training_detector takes no {sorted(unknown)}; its thresholds are {sorted(opts)}")
    opts.update(kw)
    return opts


def flatten_head_outputs(objectness, bbox_deltas):
    """`concat_box_prediction_layers` (model/faster_rcnn.py:2231-2260) by permute / reshape: per level [N, A, H, W] and [N, 4 A, H, W]
    -> ([N sum H W A], [N sum H W A, 4]) in the anchors' order, level after level and (y, x, a) inside one.  Torch tensors, any
    device; autograd passes through."""
    import torch
    obj, deltas = [], []
    for o, d in zip(objectness, bbox_deltas):
        N, A, H, W = o.shape
        obj.append(o.permute(0, 2, 3, 1).reshape(N, -1))
        deltas.append(d.view(N, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, 4))
    return torch.cat(obj, dim=1).reshape(-1), torch.cat(deltas, dim=1).reshape(-1, 4)


def assemble_training_detector_reference(features_fn, rpn_head, box_head, box_predictor, source, replay: Optional[dict] = None,
                                         trace: Optional[dict] = None, loss_dtype=None, **thresholds):
    """`assemble_training_detector` through the restatements on the host, in the manner of `assemble_detector_reference`: returns
    ``train_step(images, targets, draw) -> (losses, features)``.  With ``replay`` (the ``trace`` of a device step) no learned part is
    called: their recorded outputs — "features", "objectness", "bbox_deltas", "class_logits", "box_regression" — the resized
    "targets", "batch_shape", "image_sizes" AND the device's "proposals" take their place (decoding uses exp, which numpy rounds
    differently, so the proposals must be the device's), and every non-learned training step — anchors, both matchings, both samples,
    both encodings, RoIAlign — is restated from exactly what the device's step was given.  Without ``replay`` the four parts are called
    with CPU tensors and the proposals are `proposals_reference`'s.  The losses are `targets.rpn_loss` and `targets.fastrcnn_loss` on
    the host in ``loss_dtype`` (default torch.float64).  ``trace`` receives "proposals", "rpn_targets", "roi_targets", "pooled"."""
    o = _training_options(thresholds)

    def train_step(images, targets, draw: int = 0):
        import torch
        from . import targets as _targets
        dt = torch.float64 if loss_dtype is None else loss_dtype
        tr = {} if trace is None else trace
        if replay is None:
            batch, image_sizes, _, features, resized = features_fn(images, targets)
            levels = list(features.values())
            objectness, deltas = rpn_head(levels)
            batch_shape = tuple(batch.shape[-2:])
            with torch.no_grad():
                props = proposals_reference([v.detach() for v in objectness], [v.detach() for v in deltas], image_sizes, batch_shape, sizes=o["sizes"],
                                            aspect_ratios=o["aspect_ratios"], pre_nms_top_n=o["rpn_pre_nms_top_n"],
                                            post_nms_top_n=o["rpn_post_nms_top_n"], nms_thresh=o["rpn_nms_thresh"],
                                            score_thresh=o["rpn_score_thresh"], min_size=o["rpn_min_size"])
        else:
            batch_shape, image_sizes, resized = replay["batch_shape"], replay["image_sizes"], replay["targets"]
            features, objectness, deltas = replay["features"], replay["objectness"], replay["bbox_deltas"]
            props = [(_host(b), _host(s)) for b, s in replay["proposals"]]
        grids = [tuple(int(v) for v in ob.shape[-2:]) for ob in objectness]
        anchors = anchors_reference(grids, batch_shape, o["sizes"], o["aspect_ratios"])
        rpn_t = _targets.rpn_targets_reference(anchors, resized, high=o["rpn_fg_iou_thresh"], low=o["rpn_bg_iou_thresh"], allow_low_quality=True,
                                               batch_size_per_image=o["rpn_batch_size_per_image"], positive_fraction=o["rpn_positive_fraction"],
                                               source=source, draw=draw, log=_targets.torch_log)
        roi_t = _targets.roi_targets_reference([b for b, _ in props], resized, high=o["box_fg_iou_thresh"], low=o["box_bg_iou_thresh"],
                                               allow_low_quality=False, batch_size_per_image=o["box_batch_size_per_image"],
                                               positive_fraction=o["box_positive_fraction"], weights=o["bbox_reg_weights"], source=source, draw=draw,
                                               log=_targets.torch_log)
        pooled_from = [_host(v) for v in _pooled_levels(features, o["featmap_names"])]
        pooled = roi_align_reference(pooled_from, list(roi_t["proposals"]), image_sizes, o["output_size"], o["sampling_ratio"], o["canonical_scale"],
                                     o["canonical_level"])
        if replay is None:
            logits, regression = box_predictor(box_head(torch.from_numpy(pooled)))
        else:
            logits, regression = replay["class_logits"], replay["box_regression"]

        def on_host(v):
            return v.detach().to("cpu", dt) if hasattr(v, "detach") else torch.from_numpy(np.asarray(v)).to(dt)
        as_t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rpn_t.items()}
        as_r = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in roi_t.items()}
        obj_flat, delta_flat = flatten_head_outputs([on_host(v) for v in objectness], [on_host(v) for v in deltas])
        loss_objectness, loss_rpn_box_reg = _targets.rpn_loss(obj_flat, delta_flat, as_t)
        loss_classifier, loss_box_reg = _targets.fastrcnn_loss(on_host(logits), on_host(regression), as_r)
        tr.update(proposals=props, rpn_targets=rpn_t, roi_targets=roi_t, pooled=pooled, anchors=anchors)
        losses = dict(zip(LOSS_NAMES, (loss_classifier, loss_box_reg, loss_objectness, loss_rpn_box_reg)))
        return losses, features

    return train_step


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _on_device(tensors, what: str, device=None):
    """a list of numpy arrays or torch tensors as contiguous device tensors of ONE of fp32 / fp16 / bf16 (a non-contiguous view is
    copied)"""
    import torch
    from .imageio import _device
    out = []
    for t in tensors:
        t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"{what} must be fp32, fp16 or bf16 arrays or tensors")
        dev = t.device if t.is_cuda and device is None else _device(device)
        device = dev
        out.append(t.to(dev).contiguous())
    if any(t.dtype != out[0].dtype for t in out):
        raise TypeError(f"{what} must share one dtype")
    return out


def _cells_on(cells, device):
    import torch
    return torch.from_numpy(np.concatenate(cells)).to(device)


def anchors(grid_sizes, image_size, sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS, device=None):
    """`anchors_reference` on the device, one launch: fp32 [sum H_l W_l A_l, 4].  For callers and tests; `proposals` forms its anchors
    from the index and reads no anchor tensor."""
    import torch
    from . import ops
    from .imageio import _device
    cells = cell_anchors(sizes, aspect_ratios)
    table = level_table(grid_sizes, image_size, cells)
    dev = _device(device)
    out = torch.empty((sum(H * W * A for H, W, A, _, _ in table), 4), dtype=torch.float32, device=dev)
    ops.launch(ops.make_rpn_anchors(levels=table, cells=_cells_on(cells, dev), anchors=out))
    return out


def rpn_select(objectness, pre_nms_top_n: int = 1000, device=None):
    """`select_reference` on the device, one launch (edtr_hip.h `edtr_rpn_select`), a 1024-lane workgroup per (level, image): a radix
    select on the 32-bit key, an ordered ballot compaction, a counting rank in LDS.  int32 [N, sum take_l]."""
    import torch
    from . import ops
    pre, _ = _check_top_n(pre_nms_top_n)
    obj = _on_device(_level_list(objectness), "objectness", device)
    if not 0 < len(obj) <= RPN_MAX_LEVELS:
        raise ValueError(f"between 1 and {RPN_MAX_LEVELS} levels, got {len(obj)}")
    if any(o.ndim != 4 or o.shape[0] != obj[0].shape[0] for o in obj) or not 0 < obj[0].shape[0] <= 65535:
        raise ValueError("objectness is [N, A, H, W] per level with one N between 1 and 65535")
    if any(o[0].numel() >= LIMIT or o.numel() == 0 for o in obj):
        raise ValueError("a level takes between 1 and 2^24 - 1 anchors")
    table = [(o.shape[2], o.shape[3], o.shape[1], 0, 0) for o in obj]
    selected = torch.empty((obj[0].shape[0], sum(min(pre, o[0].numel()) for o in obj)), dtype=torch.int32, device=obj[0].device)
    ops.launch(ops.make_rpn_select(objectness=obj, levels=table, pre_nms_top_n=pre, selected=selected))
    return selected


def rpn_candidates(objectness, bbox_deltas, selected, image_sizes, padded_size, sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS,
                   pre_nms_top_n: int = 1000, score_thresh: float = 0.0, min_size: float = 1e-3, bbox_xform_clip: float = BBOX_XFORM_CLIP,
                   device=None):
    """`candidates_reference` on the device, one launch (edtr_hip.h `edtr_rpn_candidates`) with no host sync: (boxes fp32 [N, M, 4],
    probs fp32 [N, M], levels int32 [N, M], counts int32 [N]); the first counts[n] rows of image n are its candidates."""
    import torch
    from . import ops
    pre, _ = _check_top_n(pre_nms_top_n)
    both = _on_device(_level_list(objectness) + _level_list(bbox_deltas), "objectness and bbox_deltas", device)
    obj, deltas = both[:len(both) // 2], both[len(both) // 2:]
    cells = cell_anchors(sizes, aspect_ratios)
    N, grids = _check_head(obj, deltas, cells)
    table = level_table(grids, padded_size, cells)
    dev = obj[0].device
    M = sum(min(pre, H * W * A) for H, W, A, _, _ in table)
    if not isinstance(selected, torch.Tensor) or selected.dtype != torch.int32 or tuple(selected.shape) != (N, M) or len(image_sizes) != N:
        raise ValueError(f"selected is int32 [{N}, {M}] and image_sizes has {N} entries")
    sizes_dev = torch.tensor([[float(s[0]), float(s[1])] for s in image_sizes], dtype=torch.float32).to(dev)
    out_boxes = torch.empty((N, M, 4), dtype=torch.float32, device=dev)
    probs = torch.empty((N, M), dtype=torch.float32, device=dev)
    level = torch.empty((N, M), dtype=torch.int32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    ops.launch(ops.make_rpn_candidates(objectness=obj, deltas=deltas, levels=table, pre_nms_top_n=pre, cells=_cells_on(cells, dev),
                                       selected=selected.to(dev).contiguous(), image_sizes=sizes_dev, xform_clip=bbox_xform_clip,
                                       min_size=min_size, score_thresh=score_thresh, boxes=out_boxes, probs=probs, level=level, counts=counts))
    return out_boxes, probs, level, counts


def proposals(objectness, bbox_deltas, image_sizes, padded_size, *, sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS,
              pre_nms_top_n: int = 1000, post_nms_top_n: int = 1000, nms_thresh: float = 0.7, score_thresh: float = 0.0,
              min_size: float = 1e-3, device=None, trace: Optional[dict] = None):
    """`proposals_reference` on the device: `RegionProposalNetwork.forward` in eval mode from the head's outputs as the head writes
    them (per level objectness [N, A, H, W] and bbox_deltas [N, 4 A, H, W], fp32 / fp16 / bf16), for images of ``image_sizes`` = [(h, w)]
    inside a padded batch of extent ``padded_size``.  `rpn_select` and `rpn_candidates` for the whole batch, then per image
    `boxes.batched_nms` by probability with the level as the label, its walk ending after ``post_nms_top_n`` kept boxes.  Device ->
    host copies: the candidate counts of the batch (4 N bytes, where the reference synchronises in `torch.where`) and per image the
    number kept (where it indexes with `keep`).  Beyond the bounds — ``pre_nms_top_n`` > 4096, more than 8 levels, a level of 2^24 or
    more anchors, more than 65 535 images — ValueError.  [(boxes fp32 [k, 4], scores fp32 [k])] on the device."""
    import torch
    pre, post = _check_top_n(pre_nms_top_n, post_nms_top_n)
    selected = rpn_select(objectness, pre, device)
    cand_boxes, probs, level, counts = rpn_candidates(objectness, bbox_deltas, selected, image_sizes, padded_size, sizes, aspect_ratios, pre,
                                                      score_thresh, min_size, device=selected.device)
    if trace is not None:
        trace.update(selected=selected, cand_boxes=cand_boxes, cand_probs=probs, cand_level=level, cand_counts=counts)
    out = []
    for n, m in enumerate(counts.cpu().tolist()):
        b, p, lvl = cand_boxes[n, :m], probs[n, :m], level[n, :m]
        if m:
            keep, count = _boxes.batched_nms(b, p, lvl, nms_thresh, max_out=post)
            keep = keep[:int(count.item())]
            b, p = b[keep], p[keep]
        out.append((b, p))
    return out


def roi_align(features, rois, image_sizes, output_size: int = 7, sampling_ratio: int = 2, canonical_scale: float = 224.0,
              canonical_level: float = 4.0, device=None):
    """`roi_align_reference` on the device, ONE launch for all rois and all levels (edtr_hip.h `edtr_roi_align`): ``features`` an
    ordered mapping or list of per-level [N, C, H_l, W_l] tensors (fp32 / fp16 / bf16; a non-contiguous view is copied), ``rois`` a
    list of per-image [k_i, 4] boxes, ``image_sizes`` = [(h, w)] for the scales.  The scales are worked out on the host, the level of
    each roi on the device.  fp32 [sum k_i, C, P, P] in roi order; no rois at all: the empty tensor, without a launch."""
    import torch
    from . import ops
    P, S = _check_pool(output_size, sampling_ratio)
    feats, N = _check_features(features, rois, image_sizes)
    feats = _on_device(feats, "features", device)
    dev = feats[0].device
    C = int(feats[0].shape[1])
    scales, k_min, k_max = level_scales([tuple(f.shape[-2:]) for f in feats], image_sizes)
    K = sum(int(r.shape[0]) for r in rois)
    out = torch.empty((K, C, P, P), dtype=torch.float32, device=dev)
    if K == 0 or C == 0:
        return out
    flat, batch = _flat_rois(rois, N, dev)

    def launch(levels):
        ops.launch(ops.make_roi_align(features=list(levels), scales=scales, rois=flat, batch_index=batch, out=out, sampling_ratio=S, k_min=k_min,
                                      k_max=k_max, canonical_scale=canonical_scale, canonical_level=canonical_level))
        return out

    if torch.is_grad_enabled() and any(f.requires_grad for f in feats):
        if P > ROI_BWD_MAX_P:
            raise ValueError(f"the backward of roi_align takes output_size up to {ROI_BWD_MAX_P}, got {P}")
        shapes, dtype = [tuple(f.shape) for f in feats], feats[0].dtype

        def backward(grad):
            return _roi_backward_launch(grad, shapes, dtype, flat, batch, scales, k_min, k_max, S, canonical_scale, canonical_level)

        return _differentiable_roi_align().apply(launch, backward, *feats)
    return launch(feats)


def _flat_rois(rois, N: int, dev):
    """the launches' form of per-image lists of rois: (fp32 [K, 4], 16-byte aligned; int32 [K], the image of each roi, not decreasing)"""
    import torch
    flat = torch.cat([_boxes._f32_on(r, dev, "rois").reshape(-1, 4) for r in rois]).contiguous()
    flat = flat.clone() if flat.data_ptr() % 16 else flat
    batch = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), torch.tensor([int(r.shape[0]) for r in rois])).to(dev)
    return flat, batch


_ROI_ALIGN_FUNCTION = None


def _differentiable_roi_align():
    """the autograd.Function behind a `roi_align` whose features require grad (made on first use: this module imports without torch)"""
    global _ROI_ALIGN_FUNCTION
    if _ROI_ALIGN_FUNCTION is None:
        import torch
        from torch.autograd.function import once_differentiable

        class RoiAlign(torch.autograd.Function):
            @staticmethod
            def forward(ctx, launch, backward, *levels):
                ctx.backward_launch = backward
                return launch(levels)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad):
                grads = ctx.backward_launch(grad.contiguous().float())
                return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))

        _ROI_ALIGN_FUNCTION = RoiAlign
    return _ROI_ALIGN_FUNCTION


def _roi_backward_launch(grad, shapes, dtype, flat, batch, scales, k_min, k_max, S, canonical_scale, canonical_level, out=None):
    import torch
    from . import ops
    N, K, P = shapes[0][0], int(grad.shape[0]), int(grad.shape[-1])
    dev = grad.device
    grads = [torch.empty(s, dtype=dtype, device=dev) for s in shapes] if out is None else list(out)
    workspace = torch.empty(ops.roi_align_backward_workspace(N, K, P, S), dtype=torch.uint8, device=dev)
    ops.launch(ops.make_roi_align_backward(grad=grad, grads_out=grads, scales=scales, rois=flat, batch_index=batch, workspace=workspace,
                                           sampling_ratio=S, k_min=k_min, k_max=k_max, canonical_scale=canonical_scale,
                                           canonical_level=canonical_level))
    return grads


def roi_align_backward(grad, feature_shapes, rois, image_sizes, output_size: int = 7, sampling_ratio: int = 2, canonical_scale: float = 224.0,
                       canonical_level: float = 4.0, dtype=None, device=None, out=None) -> list:
    """`roi_align_backward_reference` on the device, a launch pair for all rois and all levels (edtr_hip.h `edtr_roi_align_backward`): a
    pre-pass writes one record per roi (level, image, footprint, tap tables), then one workgroup per (image, level, 16 x 16 tile,
    32 channels) gathers the rois that reach it in k order.  No atomics and no memset: two calls give equal bits.  ``grad``: fp32
    [sum k_i, C, P, P]; ``feature_shapes``: per level (N, C, H_l, W_l); ``dtype``: torch.float32 (default), float16 or bfloat16, the
    type of the returned per-level list, each sum rounded once.  ``out``: per level a contiguous device tensor of that shape and type
    to write into (every word is written).  No rois at all, or no channels: zeros, without a launch.  output_size above 16: ValueError."""
    import torch
    from .imageio import _device
    P, S = _check_pool(output_size, sampling_ratio)
    if P > ROI_BWD_MAX_P:
        raise ValueError(f"the backward of roi_align takes output_size up to {ROI_BWD_MAX_P}, got {P}")
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"dtype is torch.float32, float16 or bfloat16, got {dtype}")
    shapes = [tuple(int(v) for v in s) for s in _level_list(feature_shapes)]
    if not 0 < len(shapes) <= RPN_MAX_LEVELS or any(len(s) != 4 or s[:2] != shapes[0][:2] for s in shapes):
        raise ValueError("feature_shapes are (N, C, H_l, W_l) per level with one N and one C, for 1 to 8 levels")
    N, C = shapes[0][:2]
    if len(rois) != N or len(image_sizes) != N or not 0 < N <= 65535:
        raise ValueError(f"{N} images in the features (1 to 65535), {len(rois)} lists of rois and {len(image_sizes)} image sizes")
    if any(getattr(r, "ndim", 0) != 2 or r.shape[1] != 4 for r in rois):
        raise ValueError("rois are [k_i, 4] per image")
    grad = torch.from_numpy(np.ascontiguousarray(grad)) if isinstance(grad, np.ndarray) else grad
    if not isinstance(grad, torch.Tensor) or grad.dtype != torch.float32:
        raise TypeError("grad must be an fp32 array or tensor")
    dev = grad.device if grad.is_cuda and device is None else _device(device)
    K = sum(int(r.shape[0]) for r in rois)
    if tuple(grad.shape) != (K, C, P, P):
        raise ValueError(f"grad is [{K}, {C}, {P}, {P}], got {tuple(grad.shape)}")
    if out is not None and (len(out) != len(shapes) or any(not isinstance(o, torch.Tensor) or tuple(o.shape) != s or o.dtype != dtype or
                                                            o.device != dev or not o.is_contiguous() for o, s in zip(out, shapes))):
        raise TypeError(f"out takes per level a contiguous {dtype} tensor of the level's shape on {dev}")
    scales, k_min, k_max = level_scales([s[-2:] for s in shapes], image_sizes)
    if K == 0 or C == 0:
        if out is None:
            return [torch.zeros(s, dtype=dtype, device=dev) for s in shapes]
        for o in out:
            o.zero_()
        return list(out)
    flat, batch = _flat_rois(rois, N, dev)
    return _roi_backward_launch(grad.detach().to(dev).contiguous(), shapes, dtype, flat, batch, scales, k_min, k_max, S, canonical_scale,
                                canonical_level, out)


def assemble_detector(features_fn, rpn_head, box_head, box_predictor, trace: Optional[dict] = None, **thresholds):
    """The reference's Faster R-CNN from its learned parts and this project's launches, with no compiled extension.
    ``features_fn(images) -> (batch [N, 3, Hp, Wp], image_sizes [(h, w)], original_sizes [(h, w)], OrderedDict of features)`` is the
    user's transform + backbone + FPN; ``rpn_head(list of features) -> (objectness, bbox_deltas)``, ``box_head`` and
    ``box_predictor(x) -> (class_logits, box_regression)`` are the reference's modules.  All four are plain torch and stay with the user.
    The returned callable runs rpn_head, `proposals`, `roi_align`, box_head, box_predictor, `boxes.detections` per image and
    `boxes.resize_boxes` back to the original sizes, and returns [{"boxes", "scores", "labels"}] on the device, the shape
    `boxes.detect` and `coco.evaluate` take.

    ``thresholds``: sizes, aspect_ratios (the anchor generator's; default fasterrcnn_resnet50_fpn_v2's), rpn_pre_nms_top_n = 1000,
    rpn_post_nms_top_n = 1000, rpn_nms_thresh = 0.7, rpn_score_thresh = 0.0, rpn_min_size = 1e-3, output_size = 7, sampling_ratio = 2,
    featmap_names (the levels that are pooled from, e.g. ("0", "1", "2", "3") to leave "pool" to the RPN; default all),
    box_score_thresh = 0.05, box_nms_thresh = 0.5, box_detections_per_img = 100.  ``trace``: a dict that receives every stage of a
    call (what `assemble_detector_reference` replays)."""
    o = _detector_options(thresholds)

    def detnet(images):
        import torch
        with torch.no_grad():
            batch, image_sizes, original_sizes, features = features_fn(images)
            objectness, deltas = rpn_head(list(features.values()))
            tr = {}
            props = proposals(objectness, deltas, image_sizes, tuple(batch.shape[-2:]), sizes=o["sizes"], aspect_ratios=o["aspect_ratios"],
                              pre_nms_top_n=o["rpn_pre_nms_top_n"], post_nms_top_n=o["rpn_post_nms_top_n"], nms_thresh=o["rpn_nms_thresh"],
                              score_thresh=o["rpn_score_thresh"], min_size=o["rpn_min_size"], trace=tr)
            rois = [b for b, _ in props]
            pooled = roi_align(_pooled_levels(features, o["featmap_names"]), rois, image_sizes, o["output_size"], o["sampling_ratio"])
            logits, regression = box_predictor(box_head(pooled))
            logits, regression = logits.float(), regression.float()
        if trace is not None:
            counts = tr["cand_counts"].cpu().tolist()
            trace.update(tr, batch_shape=tuple(batch.shape[-2:]), image_sizes=list(image_sizes), original_sizes=list(original_sizes),
                         features=features, objectness=objectness, bbox_deltas=deltas, proposals=props, pooled=pooled, class_logits=logits,
                         box_regression=regression, probs=[tr["cand_probs"][n, :m].cpu().numpy() for n, m in enumerate(counts)])
        out, start = [], 0
        for n, r in enumerate(rois):
            rows = slice(start, start + int(r.shape[0]))
            start += int(r.shape[0])
            if not r.shape[0]:
                out.append(_boxes._empty_detections(r.device))
                continue
            det = _boxes.detections(logits[rows], regression[rows], r, image_sizes[n], o["box_score_thresh"], o["box_nms_thresh"],
                                    o["box_detections_per_img"])
            det["boxes"] = _boxes.resize_boxes(det["boxes"], image_sizes[n], original_sizes[n])
            out.append(det)
        return out

    return detnet


def assemble_training_detector(features_fn, rpn_head, box_head, box_predictor, source, trace: Optional[dict] = None, **thresholds):
    """The reference's Faster R-CNN in TRAIN mode from its learned parts and this project's launches, with no compiled extension: what
    `detnet(res_list + gt_list[bs2:], annot_list)` computes in the "Train detnet" step (main/det/train_edtr.py:228-241).  Returns
    ``train_step(images, targets, draw) -> (losses, features)``: ``losses`` the four scalars "loss_classifier", "loss_box_reg",
    "loss_objectness", "loss_rpn_box_reg" with autograd through the box head, the RPN head and — by `roi_align`'s backward — the
    features; ``features`` the ordered mapping the reference returns with return_feat=True, for the feature-matching loss.

    ``features_fn(images, targets) -> (batch, image_sizes, original_sizes, features, resized targets)`` is
    `detinput.assemble_features(backbone, transform, grad=True)`; ``rpn_head``, ``box_head`` and ``box_predictor`` as in
    `assemble_detector`; ``source`` the batch's `rng.NoiseSource` and ``draw`` the training step: the two samples are functions of
    (seed, image id, draw), so a step repeats bit for bit.  ``targets``: per image {"boxes": [G, 4], "labels": [G]} in the images'
    own coordinates.  The step:
      1. features_fn, whose transform resizes the targets' boxes (`DetectorTransform.__call__`);
      2. rpn_head;
      3. `proposals` on the DETACHED head outputs under no_grad with the training counts (2000 / 2000);
      4. `targets.rpn_targets` and `targets.rpn_loss`, the head outputs flattened in `concat_box_prediction_layers`' order;
      5. `targets.roi_targets` (512 / 0.25; the ground truths join the proposals);
      6. the differentiable `roi_align` over all N x batch slots: an unfilled slot is the zero box with label -1, which no loss reads,
         so its gradient is zero;
      7. box_head, box_predictor, `targets.fastrcnn_loss`.
    Nothing is copied to the host but what `proposals` itself reads back (the candidate and kept counts); the targets, the pooling and
    the losses wait for nothing.

    ``thresholds``: sizes, aspect_ratios, rpn_pre_nms_top_n, rpn_post_nms_top_n, rpn_nms_thresh, rpn_score_thresh, rpn_min_size,
    rpn_fg_iou_thresh = 0.7, rpn_bg_iou_thresh = 0.3, rpn_batch_size_per_image = 256, rpn_positive_fraction = 0.5, box_fg_iou_thresh =
    box_bg_iou_thresh = 0.5, box_batch_size_per_image = 512, box_positive_fraction = 0.25, bbox_reg_weights = (10, 10, 5, 5),
    output_size, sampling_ratio, canonical_scale, canonical_level, featmap_names.  ``trace``: a dict that receives every stage of a
    step (what `assemble_training_detector_reference` replays)."""
    o = _training_options(thresholds)
    if source is None:
        raise ValueError("assemble_training_detector needs the NoiseSource of the batch: the samples are functions of (seed, image id, draw)")

    def train_step(images, targets, draw: int = 0):
        import torch
        from . import targets as _targets
        batch, image_sizes, original_sizes, features, resized = features_fn(images, targets)
        levels = list(features.values())
        objectness, deltas = rpn_head(levels)
        batch_shape = tuple(int(v) for v in batch.shape[-2:])
        tr = {}
        with torch.no_grad():
            props = proposals([v.detach() for v in objectness], [v.detach() for v in deltas], image_sizes, batch_shape, sizes=o["sizes"],
                              aspect_ratios=o["aspect_ratios"], pre_nms_top_n=o["rpn_pre_nms_top_n"], post_nms_top_n=o["rpn_post_nms_top_n"],
                              nms_thresh=o["rpn_nms_thresh"], score_thresh=o["rpn_score_thresh"], min_size=o["rpn_min_size"], trace=tr)
            grids = [tuple(int(v) for v in ob.shape[-2:]) for ob in objectness]
            rpn_t = _targets.rpn_targets(grids, batch_shape, resized, sizes=o["sizes"], aspect_ratios=o["aspect_ratios"], high=o["rpn_fg_iou_thresh"],
                                         low=o["rpn_bg_iou_thresh"], allow_low_quality=True, batch_size_per_image=o["rpn_batch_size_per_image"],
                                         positive_fraction=o["rpn_positive_fraction"], source=source, draw=draw, device=batch.device)
            roi_t = _targets.roi_targets([b for b, _ in props], resized, high=o["box_fg_iou_thresh"], low=o["box_bg_iou_thresh"],
                                         allow_low_quality=False, batch_size_per_image=o["box_batch_size_per_image"],
                                         positive_fraction=o["box_positive_fraction"], weights=o["bbox_reg_weights"], source=source, draw=draw)
        obj_flat, delta_flat = flatten_head_outputs(objectness, deltas)
        loss_objectness, loss_rpn_box_reg = _targets.rpn_loss(obj_flat.float(), delta_flat.float(), rpn_t)
        pooled = roi_align(_pooled_levels(features, o["featmap_names"]), list(roi_t.proposals), image_sizes, o["output_size"], o["sampling_ratio"],
                           o["canonical_scale"], o["canonical_level"])
        logits, regression = box_predictor(box_head(pooled))
        logits, regression = logits.float(), regression.float()
        loss_classifier, loss_box_reg = _targets.fastrcnn_loss(logits, regression, roi_t)
        losses = dict(zip(LOSS_NAMES, (loss_classifier, loss_box_reg, loss_objectness, loss_rpn_box_reg)))
        if trace is not None:
            trace.update(tr, batch_shape=batch_shape, image_sizes=list(image_sizes), original_sizes=list(original_sizes), targets=resized,
                         features=features, objectness=objectness, bbox_deltas=deltas, proposals=props, rpn_targets=rpn_t, roi_targets=roi_t,
                         pooled=pooled, class_logits=logits, box_regression=regression, losses=losses)
        return losses, features

    return train_step
