"""Detection boxes on the device: what sits between a detector and the boxes a user of the reference's demo sees.  The demo runs its
detector on the restored image in three modes (demo.py:126-160) and merges the tiled mode's windows with torchvision's `batched_nms`;
the detector's own head ends in `RoIHeads.postprocess_detections` (model/faster_rcnn.py:1187-1244).  Boxes are fp32 [n, 4] in xyxy,
scores fp32 [n], labels int64 [n]; the launches are include/edtr_hip.h "Detection boxes" (kernels in csrc/boxes.hip).  The task
networks stay outside: `detect` takes any callable as its detector, as `labels.evaluate` takes any `segnet`.

Three layers, as in `labels` and `degrade`:
  * `rank_order`, `nms`, `batched_nms`, `detections`, `box_transform`, `resize_boxes`, `bilinear_scale`, `detect`: thin wrappers over the launches
    (torch tensors on the device, the caller's stream);
  * `*_reference`: the numpy restatement of each.  They are the NORMATIVE definition: the kernels are tested against them — by
    equality wherever no `exp` enters — and they against the reference's own `BoxCoder.decode`, `sliding_windows`, `move_boxes`,
    `resize_boxes` and `postprocess_detections` (tests/golden/boxes.npz);
  * host-side parameter code in numpy: `det_windows`, `score_keys`, `drawable`.

NMS is pinned to the RULE written out under `batched_nms_reference`, not to torchvision's binary: torchvision is not a dependency of
this project and is not installed where its goldens are made, so the golden tool stands `torchvision.ops.boxes` in by a naive
per-pair loop over that same rule.  The rule is that of torchvision's CPU kernel, with labels compared as in its
`_batched_nms_vanilla`; its other path (`_batched_nms_coordinate_trick`, boxes offset by label * (max coordinate + 1)) differs from
it only where an IoU lies within fp32 rounding of the threshold, because the offset coordinates round differently.

`draw_box` itself (OpenCV's rectangle and Hershey text rasterisers) is not provided; `drawable` returns the boxes it would draw."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

F32 = np.float32
NMS_MAX_BOXES = 32768                   # EDTR_NMS_MAX_BOXES: at the cap the suppression mask is 128 MiB
BBOX_XFORM_CLIP = math.log(1000.0 / 16)
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)    # RoIHeads' bbox_reg_weights
TILE_SCORE_MIN = 0.6                    # demo.py:143
DET_MODES = ("resize", "tile", "direct")
VOC_TVMONITOR = 20                      # the label draw_box's corner rule names
# labels for which draw_box's table holds no class ("-"): the ids COCO never assigned
COCO_UNUSED = (12, 26, 29, 30, 45, 66, 68, 69, 71, 83, 91)


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative) and host-side parameters
# ----------------------------------------------------------------------------------------------------------------------------------
def _check_boxes(boxes, scores, labels, what: str):
    """shapes of an NMS input (numpy arrays or torch tensors): [n, 4], [n], None or [n]; returns n"""
    if getattr(boxes, "ndim", 0) != 2 or boxes.shape[1] != 4:
        raise ValueError(f"{what} takes boxes of shape [n, 4], got {tuple(getattr(boxes, 'shape', ()))}")
    n = int(boxes.shape[0])
    if getattr(scores, "ndim", 0) != 1 or int(scores.shape[0]) != n:
        raise ValueError(f"{what} takes one score per box, got {tuple(getattr(scores, 'shape', ()))} for {n} boxes")
    if labels is not None and (getattr(labels, "ndim", 0) != 1 or int(labels.shape[0]) != n):
        raise ValueError(f"{what} takes one label per box, got {tuple(getattr(labels, 'shape', ()))} for {n} boxes")
    if n > NMS_MAX_BOXES:
        raise ValueError(f"{what} takes at most {NMS_MAX_BOXES} boxes, got {n}")
    return n


def _check_max_out(max_out) -> Optional[int]:
    if max_out is None:
        return None
    if int(max_out) <= 0:
        raise ValueError(f"max_out must be positive, got {max_out}")
    return int(max_out)


def score_keys(scores) -> np.ndarray:
    """uint32 [n] whose unsigned order is the order torch sorts fp32 scores in: every NaN is one largest key, -0.0 and 0.0 one key"""
    s = np.ascontiguousarray(scores, dtype=F32)
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key = np.where(s == 0, np.uint32(0x80000000), key)
    return np.where(np.isnan(s), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def rank_order_reference(scores) -> np.ndarray:
    """int32 [n]: the candidates by descending `score_keys`, equal keys by ascending index — the permutation of the rank launch,
    whose rank of i is the number of greater keys plus the number of earlier equal ones"""
    key = score_keys(scores).astype(np.int64)
    return np.argsort(-key, kind="stable").astype(np.int32)


def iou_row_reference(box, others, dtype=F32) -> np.ndarray:
    """inter / ((area_box + area_other) - inter) of one box against [m, 4] others in ``dtype`` arithmetic, each step rounded, with
    max(a, b) = a if a > b else b, min alike, and a negative extent cut to 0; 0 / 0 is NaN"""
    a = np.asarray(box, dtype=dtype)
    b = np.asarray(others, dtype=dtype).reshape(-1, 4)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.where(a[2] < b[:, 2], a[2], b[:, 2]) - np.where(a[0] > b[:, 0], a[0], b[:, 0])
        h = np.where(a[3] < b[:, 3], a[3], b[:, 3]) - np.where(a[1] > b[:, 1], a[1], b[:, 1])
        inter = np.where(w > 0, w, dtype(0)) * np.where(h > 0, h, dtype(0))
        area_a = (a[2] - a[0]) * (a[3] - a[1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        return (inter / ((area_a + area_b) - inter)).astype(dtype)


def batched_nms_reference(boxes, scores, labels, iou_threshold: float, max_out: Optional[int] = None):
    """Non-maximum suppression per label, THE RULE:
      * order the candidates by score descending, equal scores by ascending index, NaN as the largest score (`rank_order_reference`);
      * walk that order: a candidate not yet suppressed is kept, and then suppresses every later candidate j of the same label with
        inter / (area_i + area_j - inter) > iou_threshold — strictly greater, in fp32 (`iou_row_reference`);
      * the result is the kept indices into the input, in that order.
    int64 [kept]; with ``max_out`` = K the walk ends after K kept candidates and the result is (keep int64 [K] padded with -1,
    count int32 [1]), the form the device returns without a host sync."""
    n = _check_boxes(boxes, scores, labels, "batched_nms_reference")
    K = _check_max_out(max_out)
    b = np.ascontiguousarray(boxes, dtype=F32)
    lab = np.zeros(n, dtype=np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    order = rank_order_reference(scores)
    ob, ol = b[order], lab[order]
    thr = F32(iou_threshold)
    removed = np.zeros(n, dtype=bool)
    kept = []
    for i in range(n):
        if removed[i]:
            continue
        kept.append(int(order[i]))
        if K is not None and len(kept) == K:
            break
        if i + 1 < n:
            hit = (iou_row_reference(ob[i], ob[i + 1:]) > thr) & (ol[i + 1:] == ol[i])
            removed[i + 1:] |= hit
    keep = np.asarray(kept, dtype=np.int64)
    if K is None:
        return keep
    return np.concatenate([keep, np.full(K - keep.size, -1, dtype=np.int64)]), np.asarray([keep.size], dtype=np.int32)


def nms_reference(boxes, scores, iou_threshold: float, max_out: Optional[int] = None):
    """`batched_nms_reference` with one label"""
    return batched_nms_reference(boxes, scores, None, iou_threshold, max_out)


def softmax_reference(logits, dtype=F32) -> np.ndarray:
    """softmax over the last axis: exp(x - max) / sum"""
    x = np.asarray(logits, dtype=dtype)
    e = np.exp(x - x.max(axis=-1, keepdims=True)).astype(dtype)
    return (e / e.sum(axis=-1, keepdims=True, dtype=dtype)).astype(dtype)


def decode_reference(rel_codes, proposals, weights=BOX_WEIGHTS, bbox_xform_clip: float = BBOX_XFORM_CLIP, dtype=F32, exp=np.exp) -> np.ndarray:
    """`BoxCoder.decode_single` (model/util.py:702-743) in its operation order: [P, 4 C] codes and [P, 4] proposals -> [P, C, 4].
    The deltas are divided by the weights, dw and dh cut at ``bbox_xform_clip``, and the only step that is not exact arithmetic is
    ``exp`` (numpy's unless another is handed in: two exponentials that are each within an ulp differ in the last bit for a good
    third of their arguments)."""
    r = np.asarray(rel_codes, dtype=dtype)
    p = np.asarray(proposals, dtype=dtype)
    if r.ndim != 2 or p.ndim != 2 or p.shape[1] != 4 or r.shape[0] != p.shape[0] or r.shape[1] % 4:
        raise ValueError(f"decode takes codes [P, 4 C] and proposals [P, 4], got {r.shape} and {p.shape}")
    wx, wy, ww, wh = (dtype(w) for w in weights)
    clip = dtype(bbox_xform_clip)
    widths, heights = (p[:, 2] - p[:, 0])[:, None], (p[:, 3] - p[:, 1])[:, None]
    ctr_x, ctr_y = p[:, 0:1] + dtype(0.5) * widths, p[:, 1:2] + dtype(0.5) * heights
    dx, dy, dw, dh = r[:, 0::4] / wx, r[:, 1::4] / wy, r[:, 2::4] / ww, r[:, 3::4] / wh
    dw, dh = np.where(dw > clip, clip, dw), np.where(dh > clip, clip, dh)
    with np.errstate(over="ignore", invalid="ignore"):
        pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
        half_w, half_h = dtype(0.5) * (exp(dw).astype(dtype) * widths), dtype(0.5) * (exp(dh).astype(dtype) * heights)
        return np.stack([pcx - half_w, pcy - half_h, pcx + half_w, pcy + half_h], axis=2).astype(dtype)


def _clamp(v, hi):
    return np.where(v < 0, v.dtype.type(0), np.where(v > hi, hi, v))


def _check_head(class_logits, box_regression, proposals):
    if getattr(class_logits, "ndim", 0) != 2 or getattr(box_regression, "ndim", 0) != 2 or getattr(proposals, "ndim", 0) != 2:
        raise ValueError("detections takes class_logits [P, C], box_regression [P, 4 C] and proposals [P, 4]")
    P, C = int(class_logits.shape[0]), int(class_logits.shape[1])
    if C < 2 or tuple(box_regression.shape) != (P, 4 * C) or tuple(proposals.shape) != (P, 4):
        raise ValueError(f"detections takes class_logits [P, C] with C >= 2, box_regression [P, 4 C] and proposals [P, 4], got "
                         f"{tuple(class_logits.shape)}, {tuple(box_regression.shape)} and {tuple(proposals.shape)}")
    return P, C


def candidates_reference(class_logits, box_regression, proposals, image_shape, score_thresh: float = 0.05, weights=BOX_WEIGHTS,
                         bbox_xform_clip: float = BBOX_XFORM_CLIP, min_size: float = 1e-2, dtype=F32):
    """The candidate stage of `postprocess_detections`: (boxes [m, 4], scores [m], labels int64 [m]) of the class predictions with
    score > score_thresh and both sides >= min_size after decoding and clipping, background column dropped, in candidate-index order
    p (C - 1) + (c - 1)."""
    P, C = _check_head(class_logits, box_regression, proposals)
    h, w = dtype(image_shape[0]), dtype(image_shape[1])
    scores = softmax_reference(class_logits, dtype)[:, 1:].reshape(-1)
    boxes = decode_reference(box_regression, proposals, weights, bbox_xform_clip, dtype)[:, 1:].reshape(-1, 4)
    boxes = np.stack([_clamp(boxes[:, 0], w), _clamp(boxes[:, 1], h), _clamp(boxes[:, 2], w), _clamp(boxes[:, 3], h)], axis=1)
    labels = np.tile(np.arange(1, C, dtype=np.int64), P)
    with np.errstate(invalid="ignore"):
        flag = (scores > dtype(score_thresh)) & (boxes[:, 2] - boxes[:, 0] >= dtype(min_size)) & (boxes[:, 3] - boxes[:, 1] >= dtype(min_size))
    return boxes[flag], scores[flag], labels[flag]


def cancellation_ratio(boxes, image_shape) -> float:
    """max of side / |coordinate| over the coordinates of decoded, clipped boxes that the clip did not pin to 0 or to the image's
    edge (those are exact).  A corner is centre -/+ half a side, and half a side carries exp's error: two exp implementations, each
    within an ulp, and the product's rounding put the half sides up to 3 * 2^-23 = 3.6e-7 relative apart, so two evaluations of one
    coordinate differ by up to 1.8e-7 * side.  Relative to the coordinate itself that stays below 1e-5 while side / |coordinate| <= 40
    (7.2e-6); a corner that lands within a fortieth of a side of the origin does not.  The golden tool and the device tests choose
    seeds whose REFERENCE output satisfies this, so that a relative bound of 1e-5 on every coordinate is a fair one."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    if b.size == 0:
        return 0.0
    h, w = float(image_shape[0]), float(image_shape[1])
    side = np.stack([b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]] * 2, axis=1)
    edge = np.array([w, h, w, h])
    free = (b != 0) & (b != edge)
    return float(np.max(np.where(free, side / np.where(free, np.abs(b), 1.0), 0.0)))


def detections_reference(class_logits, box_regression, proposals, image_shape, score_thresh: float = 0.05, nms_thresh: float = 0.5,
                         detections_per_img: int = 100, weights=BOX_WEIGHTS, bbox_xform_clip: float = BBOX_XFORM_CLIP,
                         min_size: float = 1e-2) -> dict:
    """`RoIHeads.postprocess_detections` for one image: `candidates_reference`, `batched_nms_reference`, the first
    ``detections_per_img``.  {"boxes": fp32 [k, 4], "scores": fp32 [k], "labels": int64 [k]}."""
    boxes, scores, labels = candidates_reference(class_logits, box_regression, proposals, image_shape, score_thresh, weights,
                                                 bbox_xform_clip, min_size)
    if boxes.shape[0] > NMS_MAX_BOXES:
        raise ValueError(f"{boxes.shape[0]} candidates pass the score threshold; NMS takes at most {NMS_MAX_BOXES}")
    keep = batched_nms_reference(boxes, scores, labels, nms_thresh)[:int(detections_per_img)]
    return {"boxes": boxes[keep], "scores": scores[keep], "labels": labels[keep]}


def det_windows(W: int, H: int, tile: int, stride: int):
    """[(x0, y0, x1, y1)]: the windows of the demo's tiled detection (utils/detection.py:671-684), rows first.  Not `tiling`'s rule: the
    starts are 0, stride, ... up to max(extent - tile, 0), a last window flush with the edge is added only where those leave a rest,
    and an image smaller than the tile gets one window that reaches past it (slicing cuts it)."""
    W, H, tile, stride = int(W), int(H), int(tile), int(stride)
    if W <= 0 or H <= 0 or tile <= 0 or stride <= 0:
        raise ValueError(f"extents, tile and stride must be positive, got {W} x {H}, {tile}, {stride}")
    xs = list(range(0, max(W - tile, 0) + 1, stride))
    ys = list(range(0, max(H - tile, 0) + 1, stride))
    if xs[-1] + tile < W:
        xs.append(W - tile)
    if ys[-1] + tile < H:
        ys.append(H - tile)
    return [(x, y, x + tile, y + tile) for y in ys for x in xs]


def _pair(v, what: str) -> Tuple[float, float]:
    x, y = (v, v) if isinstance(v, (int, float, np.floating, np.integer)) else (v[0], v[1])
    return float(x), float(y)


def box_transform_reference(boxes, shift=None, mul=None, div=None, clip=None) -> np.ndarray:
    """fp32 [n, 4], in this order and each only where given: + ``shift`` = (dx, dy); * ``mul`` = (fx, fy) or / ``div`` = (fx, fy);
    clamped to [0, w] x [0, h] for ``clip`` = (h, w), an image shape"""
    b = np.array(boxes, dtype=F32, copy=True)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"boxes are [n, 4], got {b.shape}")
    if mul is not None and div is not None:
        raise ValueError("give mul or div, not both")
    for pair, op in ((shift, np.add), (mul, np.multiply), (div, np.divide)):
        if pair is not None:
            fx, fy = _pair(pair, "factor")
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                b[:, 0::2] = op(b[:, 0::2], F32(fx))
                b[:, 1::2] = op(b[:, 1::2], F32(fy))
    if clip is not None:
        b[:, 0::2] = _clamp(b[:, 0::2], F32(clip[1]))
        b[:, 1::2] = _clamp(b[:, 1::2], F32(clip[0]))
    return b


def move_boxes_reference(boxes, dx, dy) -> np.ndarray:
    """`move_boxes` (utils/detection.py:687-692)"""
    return box_transform_reference(boxes, shift=(dx, dy))


def _ratios(original_size, new_size) -> Tuple[float, float]:
    """(ratio_w, ratio_h) of `resize_boxes`: fp32(new) / fp32(original) per axis of the (h, w) sizes"""
    rh, rw = (F32(n) / F32(o) for n, o in zip(new_size, original_size))
    return float(rw), float(rh)


def resize_boxes_reference(boxes, original_size, new_size) -> np.ndarray:
    """`resize_boxes` (model/faster_rcnn.py:2558-2571): x * fp32(new_w / orig_w), y * fp32(new_h / orig_h), sizes (h, w)"""
    return box_transform_reference(boxes, mul=_ratios(original_size, new_size))


def scaled_extent(n: int, scale: float) -> int:
    """floor(n * scale) in double: the output extent F.interpolate gives a scale factor"""
    return int(math.floor(float(n) * float(scale)))


def _index_lambda(rscale, n_in: int, n_out: int):
    # fma(rscale, o + 0.5, -0.5): the product of a 24-bit and a 25-bit number and the sum are exact in double for the extents and
    # factors of an image (extents below 2^24, factors between 1 / 32 and 32), so the one rounding to fp32 is the fma's
    src = np.maximum((np.float64(rscale) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(F32), F32(0))
    idx = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return idx, np.clip(src - idx.astype(F32), F32(0), F32(1)).astype(F32)


def bilinear_scale_reference(x, scale) -> np.ndarray:
    """`F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)` over the last two axes of fp32 ``x``: the output
    extent is floor(in * scale), and the source coordinate of output o is max(fma(fp32(1 / scale), o + 0.5, -0.5), 0) — torch's rule
    when a scale factor is given (`degrade.resize_reference` derives it from in / out, as torch does for ``size=``), with the product
    and the sum rounded ONCE, as torch's builds contract them: rounded twice, a weight lands up to 2e-6 from torch's.  ``scale``: one
    factor in [1 / 32, 32] or (scale_h, scale_w).  The weights and the four products are `degrade.resize_reference`'s, each rounded."""
    x = np.asarray(x, dtype=F32)
    if x.ndim < 2:
        raise ValueError(f"an image has at least two axes, got {x.shape}")
    sh, sw = (float(scale), float(scale)) if isinstance(scale, (int, float, np.floating, np.integer)) else (float(scale[0]), float(scale[1]))
    if not (1 / 32 <= sh <= 32 and 1 / 32 <= sw <= 32):
        raise ValueError(f"a scale factor must lie in [1 / 32, 32], got {scale}")
    ih, iw = x.shape[-2:]
    oh, ow = scaled_extent(ih, sh), scaled_extent(iw, sw)
    if oh <= 0 or ow <= 0:
        raise ValueError(f"scale {scale} leaves nothing of a {ih} x {iw} image")
    y0, ty = _index_lambda(F32(1.0 / sh), ih, oh)
    x0, tx = _index_lambda(F32(1.0 / sw), iw, ow)
    y1, x1 = y0 + (y0 < ih - 1), x0 + (x0 < iw - 1)
    wy0, wx0 = (F32(1) - ty)[:, None], F32(1) - tx
    ty = ty[:, None]
    top = wx0 * x[..., y0, :][..., x0] + tx * x[..., y0, :][..., x1]
    bot = wx0 * x[..., y1, :][..., x0] + tx * x[..., y1, :][..., x1]
    return (wy0 * top + ty * bot).astype(F32)


def drawable(target: dict, image_hw, score_threshold: float = 0.8, is_coco: bool = False) -> dict:
    """The boxes `draw_box` (utils/detection.py:100-138) would draw on an image of shape ``image_hw`` = (h, w), by its rules, in
    its order:
      * a box whose score is not > ``score_threshold`` is multiplied by 0 together with its label; the box (0, 0, 0, 0) with label 0
        then names the table's LAST entry — "tvmonitor" for VOC, which the corner rule drops, an unused id for COCO;
      * the corners are cut to integers toward zero;
      * a label without a class (`COCO_UNUSED`, and label 0 for COCO) is skipped;
      * a box with x1 < 0, y1 < 0, x2 > w or y2 > h is skipped, and so is a tvmonitor (VOC label 20, or the masked label 0) with
        x1 < 10 and y1 < 10.
    ``target``: {"boxes", "labels"} and optionally "scores", numpy arrays or tensors.  Returns {"index": int64 [k] into the input,
    "boxes": int64 [k, 4] the integer corners, "labels": int64 [k]} and "scores" fp32 [k] when given.  Host-side numpy; labels the
    reference's table cannot name (negative beyond its length, or past its end) raise ValueError where the reference raises IndexError."""
    def host(v, dtype):
        return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v).astype(dtype)
    boxes, labels = host(target["boxes"], F32).reshape(-1, 4), host(target["labels"], np.int64).reshape(-1)
    scores = host(target["scores"], F32).reshape(-1) if "scores" in target else None
    if labels.shape[0] != boxes.shape[0] or (scores is not None and scores.shape[0] != boxes.shape[0]):
        raise ValueError("drawable takes one label (and one score) per box")
    h, w = int(image_hw[0]), int(image_hw[1])
    n_names = 91 if is_coco else 20
    if labels.size and (labels.min() < 0 or labels.max() > n_names):
        raise ValueError(f"labels must lie in [0, {n_names}]")
    if scores is not None:
        shown = scores > F32(score_threshold)
        boxes, labels = boxes * shown[:, None].astype(F32), labels * shown
    corners = np.trunc(boxes).astype(np.int64)
    x1, y1, x2, y2 = corners.T if corners.size else (np.zeros(0, dtype=np.int64),) * 4
    if is_coco:
        named = ~np.isin(labels, COCO_UNUSED) & (labels != 0)
        tv = np.zeros(labels.shape, dtype=bool)
    else:
        named = np.ones(labels.shape, dtype=bool)
        tv = (labels == VOC_TVMONITOR) | (labels == 0)
    inside = ~((x1 < 0) | (x2 > w) | (y1 < 0) | (y2 > h))
    index = np.nonzero(named & inside & ~((x1 < 10) & (y1 < 10) & tv))[0].astype(np.int64)
    out = {"index": index, "boxes": corners[index], "labels": labels[index]}
    if scores is not None:
        out["scores"] = scores[index]
    return out


def _first(out) -> dict:
    """a detector returns [{boxes, scores, labels}], or ([...], extra) as the reference's does"""
    if isinstance(out, tuple):
        out = out[0]
    return out[0]


def detect_reference(image, detnet, mode: str = "resize", tile: int = 512, stride: int = 256, tile_nms_threshold: float = 0.3,
                     tile_score_min: float = TILE_SCORE_MIN, resize_to: int = 512) -> dict:
    """`detect` through the restatements: ``image`` a numpy fp32 [3, h, w], ``detnet`` a callable from a list of one numpy image to
    [{boxes, scores, labels}] of numpy arrays"""
    if mode not in DET_MODES:
        raise ValueError(f"mode must be one of {DET_MODES}, got {mode!r}")
    image = np.asarray(image, dtype=F32)
    h, w = image.shape[-2:]
    if mode == "direct":
        return dict(_first(detnet([image])))
    if mode == "resize":
        scale = resize_to / max(h, w)
        out = dict(_first(detnet([bilinear_scale_reference(image, scale)])))
        out["boxes"] = box_transform_reference(out["boxes"], div=(scale, scale))
        return out
    boxes, scores, labels = [np.zeros((0, 4), dtype=F32)], [np.zeros(0, dtype=F32)], [np.zeros(0, dtype=np.int64)]
    for x0, y0, x1, y1 in det_windows(w, h, tile, stride):
        out = _first(detnet([image[:, y0:y1, x0:x1]]))
        s = np.asarray(out["scores"], dtype=F32)
        keep = s >= F32(tile_score_min)
        boxes.append(move_boxes_reference(np.asarray(out["boxes"], dtype=F32).reshape(-1, 4)[keep], x0, y0))
        scores.append(s[keep])
        labels.append(np.asarray(out["labels"]).astype(np.int64)[keep])
    boxes, scores, labels = np.concatenate(boxes), np.concatenate(scores), np.concatenate(labels)
    keep = batched_nms_reference(boxes, scores, labels, tile_nms_threshold)
    return {"boxes": boxes[keep], "scores": scores[keep], "labels": labels[keep]}


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _f32_on(x, device, what: str):
    """``x`` (numpy array or torch tensor) as a contiguous fp32 device tensor whose base is 16-byte aligned"""
    import torch
    from .imageio import _device
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{what} must be an fp32 array or tensor")
    dev = t.device if t.is_cuda and device is None else _device(device)
    t = t.to(dev).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _labels_on(labels, device):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int64, torch.int32):
        raise TypeError("labels must be int64 (or int32)")
    t = t.to(device).contiguous()
    return t.clone() if t.data_ptr() % 8 else t


def rank_order(scores, device=None):
    """`rank_order_reference` on the device, one launch: int32 [n], the candidates by descending score, equal scores by ascending
    index, NaN first.  It is the first of `batched_nms`'s three launches; n is bounded as there."""
    import torch
    from . import ops
    if getattr(scores, "ndim", 0) != 1:
        raise ValueError(f"scores are [n], got {tuple(getattr(scores, 'shape', ()))}")
    if int(scores.shape[0]) > NMS_MAX_BOXES:
        raise ValueError(f"rank_order takes at most {NMS_MAX_BOXES} scores, got {int(scores.shape[0])}")
    s = _f32_on(scores, device, "scores")
    order = torch.empty(s.shape[0], dtype=torch.int32, device=s.device)
    if s.shape[0]:
        ops.launch(ops.make_boxes_rank(scores=s, order=order))
    return order


def batched_nms(boxes, scores, labels, iou_threshold: float, max_out: Optional[int] = None, device=None):
    """`batched_nms_reference` on the device, three launches (edtr_hip.h `edtr_boxes_nms`): a counting rank — O(n^2), chosen because it
    is deterministic, stable and needs no atomics —, the 64 x 64-blocked suppression mask, and a one-workgroup scan.  Labels are
    compared, as torchvision's `_batched_nms_vanilla` does; its coordinate-offset path differs from this only where an IoU lies
    within fp32 rounding of the threshold.

    Without ``max_out``: the kept indices, int64 [kept], after reading the count (one 4-byte device -> host copy).  With ``max_out`` =
    K: (keep int64 [K] padded with -1, count int32 [1]) with no host sync; the walk ends after K kept candidates.  n = 0 returns the
    empty result without a launch; more than `NMS_MAX_BOXES` candidates raise ValueError.  The workspaces are sized by n: 8 n ceil(n / 64)
    bytes of mask."""
    import torch
    from . import ops
    n = _check_boxes(boxes, scores, labels, "batched_nms")
    K = _check_max_out(max_out)
    b = _f32_on(boxes, device, "boxes")
    s = _f32_on(scores, b.device, "scores")
    lab = None if labels is None else _labels_on(labels, b.device)
    if n == 0:
        if K is None:
            return torch.empty(0, dtype=torch.int64, device=b.device)
        return torch.full((K,), -1, dtype=torch.int64, device=b.device), torch.zeros(1, dtype=torch.int32, device=b.device)
    order = torch.empty(n, dtype=torch.int32, device=b.device)
    mask = torch.empty(n * ((n + 63) // 64), dtype=torch.int64, device=b.device)
    keep = torch.empty(n if K is None else K, dtype=torch.int64, device=b.device)
    count = torch.empty(1, dtype=torch.int32, device=b.device)
    ops.launch(ops.make_boxes_nms(boxes=b, scores=s, labels=lab, iou_threshold=iou_threshold, order=order, mask=mask, keep=keep, count=count))
    if K is None:
        return keep[:int(count.item())]
    return keep, count


def nms(boxes, scores, iou_threshold: float, max_out: Optional[int] = None, device=None):
    """`batched_nms` with one label"""
    return batched_nms(boxes, scores, None, iou_threshold, max_out, device)


def _empty_detections(device) -> dict:
    import torch
    return {"boxes": torch.zeros((0, 4), dtype=torch.float32, device=device), "scores": torch.zeros(0, dtype=torch.float32, device=device),
            "labels": torch.zeros(0, dtype=torch.int64, device=device)}


def candidates(class_logits, box_regression, proposals, image_shape, score_thresh: float = 0.05, weights=BOX_WEIGHTS,
               bbox_xform_clip: float = BBOX_XFORM_CLIP, min_size: float = 1e-2, device=None):
    """`candidates_reference` on the device, three launches (edtr_hip.h `edtr_boxes_candidates`): (boxes [m, 4], scores [m], labels
    int32 [m]) after reading m (one 4-byte device -> host copy; the reference synchronises at the same point, in `torch.where`)."""
    import torch
    from . import ops
    P, C = _check_head(class_logits, box_regression, proposals)
    logits = _f32_on(class_logits, device, "class_logits")
    dev = logits.device
    if P == 0:
        e = _empty_detections(dev)
        return e["boxes"], e["scores"], e["labels"].to(torch.int32)
    reg, prop = _f32_on(box_regression, dev, "box_regression"), _f32_on(proposals, dev, "proposals")
    m = P * (C - 1)
    work = {"cand_boxes": torch.empty((m, 4), dtype=torch.float32, device=dev), "cand_scores": torch.empty(m, dtype=torch.float32, device=dev),
            "flags": torch.empty(m, dtype=torch.uint8, device=dev), "block_counts": torch.empty((P + 3) // 4, dtype=torch.int32, device=dev),
            "out_boxes": torch.empty((m, 4), dtype=torch.float32, device=dev), "out_scores": torch.empty(m, dtype=torch.float32, device=dev),
            "out_labels": torch.empty(m, dtype=torch.int32, device=dev), "count": torch.empty(1, dtype=torch.int32, device=dev)}
    ops.launch(ops.make_boxes_candidates(logits=logits, regression=reg, proposals=prop, image_hw=image_shape, score_thresh=score_thresh,
                                         min_size=min_size, weights=weights, xform_clip=bbox_xform_clip, **work))
    k = int(work["count"].item())
    return work["out_boxes"][:k], work["out_scores"][:k], work["out_labels"][:k]


def detections(class_logits, box_regression, proposals, image_shape, score_thresh: float = 0.05, nms_thresh: float = 0.5,
               detections_per_img: int = 100, weights=BOX_WEIGHTS, bbox_xform_clip: float = BBOX_XFORM_CLIP, min_size: float = 1e-2,
               device=None) -> dict:
    """`detections_reference` on the device: `RoIHeads.postprocess_detections` (model/faster_rcnn.py:1187-1244) for one image of shape
    ``image_shape`` = (h, w).  `candidates`, then `batched_nms` in its ``max_out`` form, whose walk ends after ``detections_per_img`` kept
    boxes.  Two 4-byte device -> host copies: the number of candidates (where the reference synchronises in `torch.where`) and the
    number kept (where it indexes with `keep`).  Since a row's scores sum to 1, at most 19 classes of a proposal pass 0.05: 19 000
    candidates for 1000 proposals, inside `NMS_MAX_BOXES`; more candidates than that raise ValueError.
    {"boxes": fp32 [k, 4], "scores": fp32 [k], "labels": int64 [k]} on the device."""
    import torch
    boxes, scores, labels = candidates(class_logits, box_regression, proposals, image_shape, score_thresh, weights, bbox_xform_clip,
                                       min_size, device)
    if boxes.shape[0] == 0:
        return _empty_detections(boxes.device)
    if boxes.shape[0] > NMS_MAX_BOXES:
        raise ValueError(f"{boxes.shape[0]} candidates pass the score threshold; NMS takes at most {NMS_MAX_BOXES}")
    keep, count = batched_nms(boxes, scores, labels, nms_thresh, max_out=int(detections_per_img))
    keep = keep[:int(count.item())]
    return {"boxes": boxes[keep], "scores": scores[keep], "labels": labels[keep].to(torch.int64)}


def box_transform(boxes, shift=None, mul=None, div=None, clip=None, out=None, device=None):
    """`box_transform_reference` on the device, one launch; ``out``: None or a contiguous fp32 [n, 4] tensor (it may be ``boxes``)"""
    import torch
    from . import lib as L, ops
    if getattr(boxes, "ndim", 0) != 2 or boxes.shape[1] != 4:
        raise ValueError(f"boxes are [n, 4], got {tuple(getattr(boxes, 'shape', ()))}")
    if mul is not None and div is not None:
        raise ValueError("give mul or div, not both")
    src = _f32_on(boxes, device, "boxes")
    dst = torch.empty_like(src) if out is None else out
    if dst.dtype != torch.float32 or tuple(dst.shape) != tuple(src.shape) or not dst.is_contiguous() or dst.device != src.device or dst.data_ptr() % 16:
        raise TypeError("out must be a contiguous, 16-byte aligned fp32 [n, 4] tensor on the boxes' device")
    if src.shape[0] == 0:
        return dst
    flags, kw = 0, {}
    if shift is not None:
        flags |= L.BOX_SHIFT
        kw["dx"], kw["dy"] = _pair(shift, "shift")
    if mul is not None or div is not None:
        flags |= L.BOX_MUL if mul is not None else L.BOX_DIV
        kw["fx"], kw["fy"] = _pair(mul if mul is not None else div, "factor")
    if clip is not None:
        flags |= L.BOX_CLIP
        kw["clip_h"], kw["clip_w"] = float(clip[0]), float(clip[1])
    ops.launch(ops.make_boxes_transform(src=src, dst=dst, flags=flags, **kw))
    return dst


def resize_boxes(boxes, original_size, new_size, device=None):
    """`resize_boxes_reference` on the device"""
    return box_transform(boxes, mul=_ratios(original_size, new_size), device=device)


def bilinear_scale(x, scale, device=None):
    """`bilinear_scale_reference` on the device, one launch: fp32 [..., h, w] -> [..., floor(h scale), floor(w scale)]"""
    import torch
    from . import ops
    if getattr(x, "ndim", 0) < 2:
        raise ValueError(f"an image has at least two axes, got {tuple(getattr(x, 'shape', ()))}")
    sh, sw = (float(scale), float(scale)) if isinstance(scale, (int, float, np.floating, np.integer)) else (float(scale[0]), float(scale[1]))
    if not (1 / 32 <= sh <= 32 and 1 / 32 <= sw <= 32):
        raise ValueError(f"a scale factor must lie in [1 / 32, 32], got {scale}")
    ih, iw = int(x.shape[-2]), int(x.shape[-1])
    oh, ow = scaled_extent(ih, sh), scaled_extent(iw, sw)
    if oh <= 0 or ow <= 0:
        raise ValueError(f"scale {scale} leaves nothing of a {ih} x {iw} image")
    src = _f32_on(x, device, "image")
    dst = torch.empty(tuple(src.shape[:-2]) + (oh, ow), dtype=torch.float32, device=src.device)
    ops.launch(ops.make_boxes_bilinear_scale(src=src.reshape(-1, ih, iw), dst=dst.view(-1, oh, ow), rscale_h=float(F32(1.0 / sh)),
                                             rscale_w=float(F32(1.0 / sw))))
    return dst


def detect(image, detnet, mode: str = "resize", tile: int = 512, stride: int = 256, tile_nms_threshold: float = 0.3,
           tile_score_min: float = TILE_SCORE_MIN, resize_to: int = 512) -> dict:
    """The detection step of the reference's demo (demo.py:126-160) in its three modes.  ``image``: fp32 [3, h, w] on the device;
    ``detnet``: any callable from a list of one image to [{"boxes", "scores", "labels"}] of device tensors, or to ([...], extra) as the
    reference's detector returns.  Returns that dictionary for the whole image, on the device.
      * "direct": one call of ``detnet``.
      * "resize": scale = ``resize_to`` / max(h, w); the image through `bilinear_scale`, one call, the boxes divided by the scale.
      * "tile": one call per window of `det_windows` (each a view of the image); one launch per window keeps score >=
        ``tile_score_min`` and shifts by the window's origin into shared tensors at a running offset that stays on the device; then
        one `batched_nms` at ``tile_nms_threshold``.  Two 4-byte device -> host copies at the end (the number gathered, the number
        kept); the reference moves every window's boxes to the host.  A window with nothing at or above the minimum contributes
        nothing: the reference instead appends the PREVIOUS window's boxes once more, shifted by this window's origin (its variables
        are stale, demo.py:144-147), or raises NameError when that happens in the first window.  That accident is not reproduced."""
    import torch
    from . import ops
    if mode not in DET_MODES:
        raise ValueError(f"mode must be one of {DET_MODES}, got {mode!r}")
    if not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype != torch.float32 or image.ndim != 3:
        raise TypeError("detect takes an fp32 [3, h, w] image on the device")
    h, w = int(image.shape[1]), int(image.shape[2])
    if mode == "direct":
        return dict(_first(detnet([image])))
    if mode == "resize":
        scale = int(resize_to) / max(h, w)
        out = dict(_first(detnet([bilinear_scale(image, scale)])))
        out["boxes"] = box_transform(out["boxes"], div=(scale, scale))
        return out
    outs = [(x0, y0, _first(detnet([image[:, y0:y1, x0:x1]]))) for x0, y0, x1, y1 in det_windows(w, h, tile, stride)]
    cap = sum(int(o["scores"].shape[0]) for _, _, o in outs)
    if cap == 0:
        return _empty_detections(image.device)
    dev = image.device
    boxes = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    scores = torch.empty(cap, dtype=torch.float32, device=dev)
    labels = torch.empty(cap, dtype=torch.int32, device=dev)
    offset = torch.zeros(1, dtype=torch.int32, device=dev)
    for x0, y0, o in outs:
        if int(o["scores"].shape[0]) == 0:
            continue
        _check_boxes(o["boxes"], o["scores"], o["labels"], "detect")
        ops.launch(ops.make_boxes_filter_shift(boxes=_f32_on(o["boxes"], dev, "boxes"), scores=_f32_on(o["scores"], dev, "scores"),
                                               labels=_labels_on(o["labels"].to(torch.int64), dev), score_min=tile_score_min, dx=x0, dy=y0,
                                               out_boxes=boxes, out_scores=scores, out_labels=labels, offset=offset))
    m = int(offset.item())
    if m == 0:
        return _empty_detections(dev)
    boxes, scores, labels = boxes[:m], scores[:m], labels[:m]
    keep = batched_nms(boxes, scores, labels, tile_nms_threshold)
    return {"boxes": boxes[keep], "scores": scores[keep], "labels": labels[keep].to(torch.int64)}
