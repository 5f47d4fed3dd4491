"""Detector training targets on the device: the non-learned half of the reference's Faster R-CNN in train mode.  The reference trains
its detector on restored images (main/det/train_edtr.py:205-240); between the learned parts that forward pass runs
`RegionProposalNetwork.assign_targets_to_anchors` (model/faster_rcnn.py:2030-2066), `Matcher`, `BoxCoder.encode` and
`BalancedPositiveNegativeSampler` (model/util.py:594-679, 746-920) and `RoIHeads.select_training_samples` (model/faster_rcnn.py:1087-1185).
No gradient flows through any of them, so each is a plain forward launch here, like everything in `rois`.  What the reference pays for
them: a dense [G, A] IoU matrix per image read three times, two `torch.randperm` per image that differ between devices and make no
run repeatable, and `torchvision.ops.boxes.box_iou`, a package this project runs without.

Three layers, as in `rois`, `boxes` and `coco`:
  * `match`, `encode`, `sample`, `rpn_targets`, `roi_targets`: thin wrappers over the launches of include/edtr_hip.h "Detector training
    targets" (kernels in csrc/targets.hip; torch tensors on the device, the caller's stream, no host sync: `Targets.to_host()` is the
    only copy); `rpn_loss` and `fastrcnn_loss` need autograd and are thin torch compositions over the masks and device counts;
  * `*_reference`: the numpy restatement of each.  They are the NORMATIVE definition: the kernels are tested against them by equality
    wherever `log` does not enter, and they against the reference's own classes (tests/golden/targets.npz);
  * host-side parameter code: `ragged_table`.

THE RULES.
  IoU      torchvision's `box_iou(gt, boxes)`, each step one rounded fp32 operation: area = (x2 - x1)(y2 - y1); w, h = max(min(rb) -
           max(lt), 0) with NaNs kept; inter = w h; iou = inter / ((area_g + area_p) - inter), IEEE division.  It is pinned to this
           written rule, not to torchvision's binary (as `boxes` pins NMS and `rois` RoIAlign).  No [G, P] matrix exists on the device.
  best     per box `match_quality_matrix.max(dim=0)` by torch's rule: the first maximal g wins and a NaN counts as the maximum.
  matched  -1 where best < low, -2 where low <= best < high; a NaN compares false both times and keeps its index.
  restore  with allow_low_quality, `set_low_quality_matches_` exactly: highest[g] = max_p iou[g, p] (a NaN propagates and then equals
           nothing); every p with iou[g, p] == highest[g] for some g gets back ITS OWN argmax, not g.  That includes the reference's
           quirk: a ground truth that overlaps nothing has highest = 0 and restores every box whose IoU with it is 0.  Reproduced,
           not repaired.
  labels   RPN form, fp32: 1 matched, 0 for -1, -1 for -2.  RoI form, int64: gt_labels[matched], 0 for -1, -1 for -2.  An image
           without ground truth gets labels 0 and matched 0 (the reference's background branch) and encodes against the zero box.
  encode   `encode_boxes` in its operation order: ew = px2 - px1, ecx = px1 + 0.5 ew (g alike); dx = (wx (gcx - ecx)) / ew, dw =
           ww log(gw / ew); y and h alike.  dx, dy are bit for bit; dw, dh are bit for bit once the `log` is handed in (`torch_log`),
           and within a measured tolerance of the device's logf.  RPN targets encode gt[max(matched, 0)] against EVERY anchor with
           weights (1, 1, 1, 1); RoI targets encode the sampled proposals only, with (10, 10, 5, 5).
  sample   `BalancedPositiveNegativeSampler` with its counts — num_pos = min(#(label >= 1), int(batch fraction)), num_neg = min(#(label
           == 0), batch - num_pos) — and, where it draws `torch.randperm`, the seeded stream: box i of an image has the 32-bit key
           `rng.uniform_words_reference(seed, [image_id], purpose, draw, .)[i]` with purpose `rng.PURPOSE_SAMPLE_RPN` or
           `rng.PURPOSE_SAMPLE_ROI` and draw = the training step.  The sampled positives are those with the num_pos smallest keys, equal
           keys going to the smaller index; the negatives follow the same rule over the same words.  The sample of an image depends on
           (seed, image id, draw) alone, not on the batch it travels in.
Limits (ValueError): at most 1024 ground truths and fewer than 2^24 boxes per image, at least one box per image, at most 65 535
images, batch_size_per_image at most 4096."""
from __future__ import annotations

import numpy as np

from . import rng as _rng
from .boxes import F32
from .rois import RPN_ASPECT_RATIOS, RPN_SIZES

MAX_GT = 1024                           # EDTR_TARGETS_MAX_GT
MAX_BATCH = 4096                        # EDTR_TARGETS_MAX_BATCH
TILE = 1024                             # EDTR_TARGETS_TILE
LIMIT = 1 << 24
FORM_RPN, FORM_ROI = 0, 1               # EDTR_TARGETS_RPN / EDTR_TARGETS_ROI
BELOW_LOW_THRESHOLD, BETWEEN_THRESHOLDS = -1, -2
RPN_WEIGHTS, ROI_WEIGHTS = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)
SMOOTH_L1_BETA = 1.0 / 9.0


# ----------------------------------------------------------------------------------------------------------------------------------
# host-side parameters
# ----------------------------------------------------------------------------------------------------------------------------------
def _np_boxes(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().float().cpu().numpy()
    return np.ascontiguousarray(v, dtype=F32).reshape(-1, 4)


def _form(form) -> int:
    if form in ("rpn", FORM_RPN):
        return FORM_RPN
    if form in ("roi", FORM_ROI):
        return FORM_ROI
    raise ValueError(f"form must be 'rpn' or 'roi', got {form!r}")


def ragged_table(box_counts, gt_counts) -> list:
    """[(box_start, gt_start)] with N + 1 rows for per-image counts of boxes and ground truths.  Checks the bounds of the launches."""
    box_counts, gt_counts = [int(v) for v in box_counts], [int(v) for v in gt_counts]
    if len(box_counts) != len(gt_counts):
        raise ValueError(f"{len(box_counts)} images of boxes for {len(gt_counts)} images of ground truth")
    if not 0 < len(box_counts) <= 65535:
        raise ValueError(f"between 1 and 65535 images, got {len(box_counts)}")
    rows, b, g = [(0, 0)], 0, 0
    for P, G in zip(box_counts, gt_counts):
        if P <= 0:
            raise ValueError("every image needs at least one box (the reference refuses an image without proposals)")
        if P >= LIMIT or G > MAX_GT or G < 0:
            raise ValueError(f"an image takes fewer than 2^24 boxes and at most {MAX_GT} ground truths, got {P} and {G}")
        b, g = b + P, g + G
        rows.append((b, g))
    if b >= 1 << 31:
        raise ValueError(f"a batch takes fewer than 2^31 boxes, got {b}")
    return rows


def _check_sampler(batch_size_per_image, positive_fraction):
    batch = int(batch_size_per_image)
    if not 0 < batch <= MAX_BATCH:
        raise ValueError(f"batch_size_per_image is between 1 and {MAX_BATCH}, got {batch_size_per_image}")
    max_pos = int(batch * positive_fraction)                # the reference's expression, in Python floats
    if not 0 <= max_pos <= batch:
        raise ValueError(f"positive_fraction must lie in [0, 1], got {positive_fraction}")
    return batch, max_pos


def _check_thresholds(high, low):
    if not float(low) <= float(high):
        raise ValueError(f"low_threshold should be <= high_threshold, got {low} and {high}")
    return F32(high), F32(low)


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative)
# ----------------------------------------------------------------------------------------------------------------------------------
def iou_reference(gt_boxes, boxes) -> np.ndarray:
    """`box_iou(gt, boxes)` by THE RULE: fp32 [G, P], every step one rounded fp32 operation, NaNs propagated as torch does."""
    g, p = _np_boxes(gt_boxes), _np_boxes(boxes)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        area_g, area_p = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]), (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
        w = np.minimum(g[:, None, 2], p[None, :, 2]) - np.maximum(g[:, None, 0], p[None, :, 0])
        h = np.minimum(g[:, None, 3], p[None, :, 3]) - np.maximum(g[:, None, 1], p[None, :, 1])
        inter = np.where(w < 0, F32(0), w) * np.where(h < 0, F32(0), h)
        return (inter / ((area_g[:, None] + area_p[None, :]) - inter)).astype(F32)


def best_reference(quality):
    """`quality.max(dim=0)` by torch's rule for a [G, P] matrix: (values, indices) with the first maximal g, a NaN counting as the
    maximum (the first NaN of a column wins)."""
    q = np.asarray(quality, dtype=F32)
    nan = np.isnan(q)
    idx = np.where(nan.any(axis=0), nan.argmax(axis=0), np.where(nan, -np.inf, q).argmax(axis=0))
    return q[idx, np.arange(q.shape[1])], idx.astype(np.int64)


def match_quality_reference(quality, high: float, low: float, allow_low_quality: bool) -> np.ndarray:
    """`Matcher.__call__` on a [G, P] quality matrix with G, P > 0, THE RULE of the module docstring: int32 [P]."""
    q = np.asarray(quality, dtype=F32)
    high, low = _check_thresholds(high, low)
    val, idx = best_reference(q)
    with np.errstate(invalid="ignore"):
        matched = np.where(val < low, BELOW_LOW_THRESHOLD, np.where((val >= low) & (val < high), BETWEEN_THRESHOLDS, idx))
        if allow_low_quality:
            nan = np.isnan(q)
            highest = np.where(nan.any(axis=1), F32(np.nan), np.where(nan, -np.inf, q).max(axis=1)).astype(F32)
            restore = (q == highest[:, None]).any(axis=0)
            matched = np.where(restore, idx, matched)
    return matched.astype(np.int32)


def match_reference(boxes, gt_boxes, high: float, low: float, allow_low_quality: bool) -> list:
    """Per image the int32 [P_i] result of `Matcher` over `iou_reference`; ``boxes``: a list of [P_i, 4], or one [P, 4] set shared by
    every image; ``gt_boxes``: a list of [G_i, 4].  An image without ground truth: zeros."""
    boxes = [boxes] * len(gt_boxes) if not isinstance(boxes, (list, tuple)) else list(boxes)
    ragged_table([_np_boxes(b).shape[0] for b in boxes], [_np_boxes(g).shape[0] for g in gt_boxes])
    out = []
    for b, g in zip(boxes, gt_boxes):
        b, g = _np_boxes(b), _np_boxes(g)
        out.append(match_quality_reference(iou_reference(g, b), high, low, allow_low_quality) if g.shape[0] else np.zeros(b.shape[0], np.int32))
    return out


def labels_reference(matched, form, gt_labels=None) -> np.ndarray:
    """The labels of one image from its ``matched``: fp32 1 / 0 / -1 (RPN form), or int64 gt_labels[matched] / 0 / -1 (RoI form;
    without ground truth: zeros)."""
    m = np.asarray(matched)
    if _form(form) == FORM_RPN:
        return np.where(m >= 0, F32(1), np.where(m == BELOW_LOW_THRESHOLD, F32(0), F32(-1))).astype(F32)
    gl = np.asarray(gt_labels, dtype=np.int64).reshape(-1)
    if not gl.size:
        return np.zeros(m.shape, dtype=np.int64)
    return np.where(m >= 0, gl[np.clip(m, 0, None)], np.where(m == BELOW_LOW_THRESHOLD, 0, -1)).astype(np.int64)


def torch_log(x) -> np.ndarray:
    """torch's CPU log on a numpy array: the logarithm the reference's own `BoxCoder.encode` runs (as `rois.torch_exp` for exp)."""
    import torch
    return torch.log(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def encode_reference(reference_boxes, proposals, weights=RPN_WEIGHTS, log=np.log) -> np.ndarray:
    """`encode_boxes` (model/util.py:594-638) in its operation order, fp32 [K, 4]: dx = (wx (gcx - ecx)) / ew, dw = ww log(gw / ew).
    ``log``: numpy's by default, `torch_log` to meet the reference bit for bit."""
    g, p = _np_boxes(reference_boxes), _np_boxes(proposals)
    if g.shape != p.shape:
        raise ValueError(f"one reference box per proposal, got {g.shape} and {p.shape}")
    wx, wy, ww, wh = (F32(v) for v in weights)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ew, eh = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
        ecx, ecy = p[:, 0] + F32(0.5) * ew, p[:, 1] + F32(0.5) * eh
        gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        gcx, gcy = g[:, 0] + F32(0.5) * gw, g[:, 1] + F32(0.5) * gh
        dx, dy = (wx * (gcx - ecx)) / ew, (wy * (gcy - ecy)) / eh
        dw, dh = ww * log((gw / ew).astype(F32)).astype(F32), wh * log((gh / eh).astype(F32)).astype(F32)
    return np.stack([dx, dy, dw, dh], axis=1).astype(F32)


def sample_keys_reference(source, count: int, draw: int, purpose: int, image: int) -> np.ndarray:
    """uint32 [count]: the keys of the boxes of image ``image`` of ``source`` (a `rng.NoiseSource`)"""
    if purpose not in _rng.SAMPLE_PURPOSES:
        raise ValueError(f"purpose must be one of {_rng.SAMPLE_PURPOSES}, got {purpose}")
    return _rng.uniform_words_reference(source.seed, [source.image_ids[image]], purpose, draw, (int(count) + 3) // 4 * 4)[0, :int(count)]


def sample_reference(labels, batch_size_per_image: int, positive_fraction: float, source=None, draw: int = 0,
                     purpose: int = _rng.PURPOSE_SAMPLE_RPN, keys=None):
    """`BalancedPositiveNegativeSampler.__call__` on the seeded stream, THE RULE.  ``labels``: per image [P_i] (any dtype); ``keys``:
    None, or per image the uint32 keys to use in place of the stream's.  Returns (mask_pos, mask_neg, sampled, counts): per image two
    uint8 [P_i] masks; int32 [N, batch] of the sampled indices in ascending order padded with -1; int32 [N, 2] = num_pos, num_neg."""
    batch, max_pos = _check_sampler(batch_size_per_image, positive_fraction)
    if keys is None:
        source.check_batch(len(labels), "sample_reference")
    mask_pos, mask_neg = [], []
    sampled, counts = np.full((len(labels), batch), -1, dtype=np.int32), np.zeros((len(labels), 2), dtype=np.int32)
    for n, lab in enumerate(labels):
        lab = np.asarray(lab.detach().cpu().numpy() if hasattr(lab, "detach") else lab).reshape(-1)
        key = sample_keys_reference(source, lab.size, draw, purpose, n) if keys is None else np.asarray(keys[n], dtype=np.uint32).reshape(-1)
        if key.shape != lab.shape:
            raise ValueError(f"image {n}: {key.size} keys for {lab.size} labels")
        positive, negative = np.nonzero(lab >= 1)[0], np.nonzero(lab == 0)[0]
        num_pos = min(positive.size, max_pos)
        num_neg = min(negative.size, batch - num_pos)
        mp, mn = np.zeros(lab.size, dtype=np.uint8), np.zeros(lab.size, dtype=np.uint8)
        mp[positive[np.argsort(key[positive], kind="stable")[:num_pos]]] = 1
        mn[negative[np.argsort(key[negative], kind="stable")[:num_neg]]] = 1
        pick = np.nonzero(mp | mn)[0]
        sampled[n, :pick.size], counts[n] = pick, (num_pos, num_neg)
        mask_pos.append(mp)
        mask_neg.append(mn)
    return mask_pos, mask_neg, sampled, counts


def _gt_lists(targets):
    boxes = [_np_boxes(t["boxes"]) for t in targets]
    labels = [np.asarray(t["labels"].detach().cpu().numpy() if hasattr(t["labels"], "detach") else t["labels"], dtype=np.int64).reshape(-1)
              if "labels" in t else np.ones(b.shape[0], dtype=np.int64) for t, b in zip(targets, boxes)]
    if any(l.shape[0] != b.shape[0] for l, b in zip(labels, boxes)):
        raise ValueError("every target has one label per box")
    return boxes, labels


def rpn_targets_reference(anchors, targets, *, high: float = 0.7, low: float = 0.3, allow_low_quality: bool = True,
                          batch_size_per_image: int = 256, positive_fraction: float = 0.5, source=None, draw: int = 0, log=np.log, keys=None) -> dict:
    """`rpn_targets` through the restatements from the anchors [A, 4] (`rois.anchors_reference`): `assign_targets_to_anchors`,
    `BoxCoder.encode` with weights 1 and the sampler of `compute_loss`.  {"matched" int32 [N, A], "labels" fp32 [N, A], "regression"
    fp32 [N, A, 4], "mask_pos" / "mask_neg" uint8 [N, A], "sampled" int32 [N, batch], "counts" int32 [N, 2]}."""
    anchors = _np_boxes(anchors)
    gt, _ = _gt_lists(targets)
    matched = match_reference(anchors, gt, high, low, allow_low_quality)
    labels = [labels_reference(m, FORM_RPN) if g.shape[0] else np.zeros(m.shape, dtype=F32) for m, g in zip(matched, gt)]
    regression = [encode_reference(g[np.clip(m, 0, None)] if g.shape[0] else np.zeros_like(anchors), anchors, RPN_WEIGHTS, log)
                  for m, g in zip(matched, gt)]
    mp, mn, sampled, counts = sample_reference(labels, batch_size_per_image, positive_fraction, source, draw, _rng.PURPOSE_SAMPLE_RPN, keys)
    return dict(matched=np.stack(matched), labels=np.stack(labels), regression=np.stack(regression), mask_pos=np.stack(mp), mask_neg=np.stack(mn),
                sampled=sampled, counts=counts)


def roi_targets_reference(proposals, targets, *, high: float = 0.5, low: float = 0.5, allow_low_quality: bool = False,
                          batch_size_per_image: int = 512, positive_fraction: float = 0.25, weights=ROI_WEIGHTS, source=None, draw: int = 0,
                          log=np.log, keys=None) -> dict:
    """`roi_targets` through the restatements: `select_training_samples`.  {"proposals" fp32 [N, batch, 4], "labels" / "matched" int64
    [N, batch], "regression_targets" fp32 [N, batch, 4], "sampled" int32 [N, batch], "counts" int32 [N, 2]}; the slots past an image's
    sampled count hold zeros and label -1."""
    gt, gt_labels = _gt_lists(targets)
    props = [np.concatenate([_np_boxes(p), g]) for p, g in zip(proposals, gt)]
    matched = match_reference(props, gt, high, low, allow_low_quality)
    labels = [labels_reference(m, FORM_ROI, gl) for m, gl in zip(matched, gt_labels)]
    _, _, sampled, counts = sample_reference(labels, batch_size_per_image, positive_fraction, source, draw, _rng.PURPOSE_SAMPLE_ROI, keys)
    N, batch = sampled.shape
    out = dict(proposals=np.zeros((N, batch, 4), dtype=F32), labels=np.full((N, batch), -1, dtype=np.int64), matched=np.zeros((N, batch), dtype=np.int64),
               regression_targets=np.zeros((N, batch, 4), dtype=F32), sampled=sampled, counts=counts)
    for n in range(N):
        k = int(counts[n].sum())
        idx = sampled[n, :k]
        m = np.clip(matched[n][idx], 0, None).astype(np.int64)
        g = gt[n] if gt[n].shape[0] else np.zeros((1, 4), dtype=F32)
        out["proposals"][n, :k], out["labels"][n, :k], out["matched"][n, :k] = props[n][idx], labels[n][idx], m
        out["regression_targets"][n, :k] = encode_reference(g[m], props[n][idx], weights, log)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
class Targets(dict):
    """The device tensors of a launch or a flow, by name and as attributes.  Nothing here synchronises with the host; `to_host` is the
    one copy."""
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def to_host(self) -> dict:
        return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in self.items()}


def _boxes_on(v, device):
    """(numpy array or torch tensor, any float dtype) as a contiguous fp32 [K, 4] device tensor; a non-contiguous view is copied"""
    import torch
    from .imageio import _device
    t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
    if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.numel() % 4 or (t.ndim and t.shape[-1] != 4):
        raise TypeError("boxes must be floating-point [K, 4] arrays or tensors")
    dev = t.device if t.is_cuda and device is None else _device(device)
    return t.to(dev, torch.float32).reshape(-1, 4).contiguous()


def _flat(parts, dev, dtype):
    """one 16-byte aligned tensor from per-image parts"""
    import torch
    parts = [p.to(dev, dtype) for p in parts]              # (parts may arrive on different devices: default labels are made on the host)
    t = (torch.cat(parts) if len(parts) > 1 else parts[0].clone()).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _table_on(table_host, dev):
    import torch
    return torch.tensor(table_host, dtype=torch.int32).to(dev)


def match(boxes, gt_boxes, high: float, low: float, allow_low_quality: bool, form="rpn", gt_labels=None, weights=None, device=None) -> Targets:
    """`match_reference` on the device, two launches for the whole ragged batch (edtr_hip.h `edtr_targets_match`).  ``boxes``: a list of
    per-image [P_i, 4], or ONE [P, 4] set that every image shares (the RPN's anchors); ``gt_boxes``: a list of per-image [G_i, 4];
    ``gt_labels``: a list of per-image int [G_i] for form "roi".  Returns flat tensors: "matched" int32 [sum P], "labels" (fp32 for
    "rpn", int64 for "roi"), "regression" fp32 [sum P, 4] when ``weights`` is given in the RPN form (every box encoded against
    gt[max(matched, 0)]), plus what the later launches need: "boxes", "gt_boxes", "table" (int32 [N + 1, 2] on the device) and
    "table_host"."""
    import torch
    from . import ops
    form = _form(form)
    _check_thresholds(high, low)
    shared = not isinstance(boxes, (list, tuple))
    N = len(gt_boxes)
    per_image = [_boxes_on(boxes, device)] if shared else [_boxes_on(b, device) for b in boxes]
    dev = per_image[0].device
    gts = [_boxes_on(g, dev) for g in gt_boxes]
    counts = [int(per_image[0].shape[0])] * N if shared else [int(b.shape[0]) for b in per_image]
    table_host = ragged_table(counts, [int(g.shape[0]) for g in gts])
    total, total_gt = table_host[-1]
    flat = _flat(per_image, dev, torch.float32)
    gt_flat = _flat(gts, dev, torch.float32) if total_gt else None
    gl_flat = None
    if form == FORM_ROI:
        if gt_labels is None or len(gt_labels) != N:
            raise ValueError("the RoI form takes one array of labels per image")
        gls = [torch.as_tensor(np.asarray(l) if not isinstance(l, torch.Tensor) else l).reshape(-1) for l in gt_labels]
        if any(l.shape[0] != g.shape[0] or l.is_floating_point() for l, g in zip(gls, gts)):
            raise ValueError("gt_labels are integers, one per ground-truth box")
        gl_flat = _flat(gls, dev, torch.int64) if total_gt else None
    table = _table_on(table_host, dev)
    matched = torch.empty(total, dtype=torch.int32, device=dev)
    labels = torch.empty(total, dtype=torch.float32 if form == FORM_RPN else torch.int64, device=dev)
    regression = torch.empty((total, 4), dtype=torch.float32, device=dev) if form == FORM_RPN and weights is not None else None
    best_val, best_idx = torch.empty(total, dtype=torch.float32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
    partial = torch.empty(ops.targets_partial_words(table_host), dtype=torch.int32, device=dev)
    ops.launch(ops.make_targets_match(boxes=flat, shared=shared, gt_boxes=gt_flat, gt_labels=gl_flat, table_host=table_host, table=table, high=high,
                                      low=low, allow_low_quality=allow_low_quality, form=form, weights=weights or RPN_WEIGHTS, best_val=best_val,
                                      best_idx=best_idx, partial=partial, matched=matched, labels=labels, regression=regression))
    return Targets(matched=matched, labels=labels, regression=regression, boxes=flat, gt_boxes=gt_flat, table=table, table_host=table_host)


def encode(reference_boxes, proposals, weights=RPN_WEIGHTS, device=None):
    """`encode_reference` on the device, one launch (edtr_hip.h `edtr_targets_encode`): fp32 [K, 4].  For callers and tests; the flows
    encode inside their match and gather launches."""
    import torch
    from . import ops
    ref = _boxes_on(reference_boxes, device)
    prop = _boxes_on(proposals, ref.device)
    if ref.shape != prop.shape:
        raise ValueError(f"one reference box per proposal, got {tuple(ref.shape)} and {tuple(prop.shape)}")
    ref, prop = (t.clone() if t.data_ptr() % 16 else t for t in (ref, prop))
    out = torch.empty_like(ref)
    if ref.shape[0]:
        ops.launch(ops.make_targets_encode(reference_boxes=ref, proposals=prop, weights=weights, out=out))
    return out


def sample(labels, batch_size_per_image: int, positive_fraction: float, source, draw: int = 0, purpose: int = _rng.PURPOSE_SAMPLE_RPN,
           table=None, table_host=None, device=None, keys=None) -> Targets:
    """`sample_reference` on the device, one launch with one workgroup per image (edtr_hip.h `edtr_targets_sample`).  ``labels``: a list
    of per-image [P_i] tensors (fp32: the RPN form, int64: the RoI form), or with ``table`` / ``table_host`` of `match` its flat labels.
    "mask_pos" / "mask_neg" uint8 [sum P], "sampled" int32 [N, batch] (ascending, then -1), "counts" int32 [N, 2] = num_pos, num_neg.
    ``keys``: None, or per image the uint32 keys that take the stream's place, as in `sample_reference` (``source`` may then be None);
    for tests: the stream practically never gives two boxes one key, and the rule for equal keys wants testing on the device too."""
    import torch
    from . import ops
    from .imageio import _device
    batch, max_pos = _check_sampler(batch_size_per_image, positive_fraction)
    if purpose not in _rng.SAMPLE_PURPOSES:
        raise ValueError(f"purpose must be one of {_rng.SAMPLE_PURPOSES}, got {purpose}")
    if table_host is None:
        parts = [torch.as_tensor(l).reshape(-1) for l in labels]
        dev = parts[0].device if parts[0].is_cuda and device is None else _device(device)
        table_host = ragged_table([int(p.shape[0]) for p in parts], [0] * len(parts))
        flat = _flat(parts, dev, torch.float32 if parts[0].is_floating_point() else torch.int64)
        table = _table_on(table_host, dev)
    else:
        flat = labels.contiguous()
    if flat.dtype not in (torch.float32, torch.int64) or flat.shape != (table_host[-1][0],):
        raise TypeError(f"labels are fp32 or int64 [{table_host[-1][0]}], got {flat.dtype} {tuple(flat.shape)}")
    N, dev = len(table_host) - 1, flat.device
    keys_dev = None
    if keys is None:
        source.check_batch(N, "sample")
    else:
        flat_keys = np.concatenate([np.asarray(k, dtype=np.uint32).reshape(-1) for k in keys])
        if len(keys) != N or any(np.asarray(k).size != b[0] - a[0] for k, a, b in zip(keys, table_host, table_host[1:])):
            raise ValueError("keys take one uint32 per box of every image")
        keys_dev = torch.from_numpy(flat_keys.view(np.int32)).to(dev)
    mask_pos, mask_neg = torch.empty(flat.shape[0], dtype=torch.uint8, device=dev), torch.empty(flat.shape[0], dtype=torch.uint8, device=dev)
    sampled, counts = torch.empty((N, batch), dtype=torch.int32, device=dev), torch.empty((N, 2), dtype=torch.int32, device=dev)
    ops.launch(ops.make_targets_sample(labels=flat, form=FORM_RPN if flat.dtype == torch.float32 else FORM_ROI, table_host=table_host, table=table,
                                       batch=batch, max_pos=max_pos, source=source, draw=draw, purpose=purpose, mask_pos=mask_pos, mask_neg=mask_neg,
                                       sampled=sampled, counts=counts, keys=keys_dev))
    return Targets(mask_pos=mask_pos, mask_neg=mask_neg, sampled=sampled, counts=counts)


def _gt_on(targets, device):
    import torch
    boxes = [_boxes_on(t["boxes"], device) for t in targets]
    labels = [torch.as_tensor(t["labels"]).reshape(-1) if "labels" in t else torch.ones(int(b.shape[0]), dtype=torch.int64) for t, b in zip(targets, boxes)]
    return boxes, labels


def rpn_targets(grid_sizes, padded_size, targets, *, sizes=RPN_SIZES, aspect_ratios=RPN_ASPECT_RATIOS, high: float = 0.7, low: float = 0.3,
                allow_low_quality: bool = True, batch_size_per_image: int = 256, positive_fraction: float = 0.5, source=None, draw: int = 0,
                device=None) -> Targets:
    """`rpn_targets_reference` on the device: the anchors of the padded batch (`rois.anchors`), `match` in the RPN form with every
    anchor encoded against its ground truth, and `sample` on purpose `rng.PURPOSE_SAMPLE_RPN` — four launches for the batch, no host
    sync.  ``targets``: per image {"boxes": [G, 4]}; ``source``: the `rng.NoiseSource` of the batch; ``draw``: the training step.
    Defaults: the v2 detector's 0.7 / 0.3 with low-quality matches, 256 / 0.5.  "labels" fp32 [N, A], "matched" int32 [N, A],
    "regression" fp32 [N, A, 4], "mask_pos" / "mask_neg" uint8 [N, A], "sampled" int32 [N, batch], "counts" int32 [N, 2], "anchors"."""
    from . import rois
    if source is None:
        raise ValueError("rpn_targets needs the NoiseSource of the batch: the sample is a function of (seed, image id, draw)")
    _check_sampler(batch_size_per_image, positive_fraction)
    anchors = rois.anchors(grid_sizes, padded_size, sizes, aspect_ratios, device)
    gt, _ = _gt_on(targets, anchors.device)
    m = match(anchors, gt, high, low, allow_low_quality, "rpn", weights=RPN_WEIGHTS)
    s = sample(m.labels, batch_size_per_image, positive_fraction, source, draw, _rng.PURPOSE_SAMPLE_RPN, m.table, m.table_host)
    N, A = len(gt), int(anchors.shape[0])
    return Targets(labels=m.labels.view(N, A), matched=m.matched.view(N, A), regression=m.regression.view(N, A, 4), mask_pos=s.mask_pos.view(N, A),
                   mask_neg=s.mask_neg.view(N, A), sampled=s.sampled, counts=s.counts, anchors=anchors)


def roi_targets(proposals, targets, *, high: float = 0.5, low: float = 0.5, allow_low_quality: bool = False, batch_size_per_image: int = 512,
                positive_fraction: float = 0.25, weights=ROI_WEIGHTS, source=None, draw: int = 0, device=None) -> Targets:
    """`roi_targets_reference` on the device, `RoIHeads.select_training_samples`: each image's ground-truth boxes appended to its
    proposals (torch.cat, plumbing), `match` in the RoI form, `sample` on purpose `rng.PURPOSE_SAMPLE_ROI`, and one launch that gathers
    the sampled proposals and encodes them (edtr_hip.h `edtr_targets_gather`).  No host sync: every image owns ``batch_size_per_image``
    slots, "counts" [N, 2] = num_pos, num_neg says how many are filled, and the rest hold zeros with label -1.  "proposals" fp32
    [N, batch, 4], "labels" / "matched" int64 [N, batch], "regression_targets" fp32 [N, batch, 4], "sampled" int32 [N, batch]."""
    import torch
    from . import ops
    if source is None:
        raise ValueError("roi_targets needs the NoiseSource of the batch: the sample is a function of (seed, image id, draw)")
    batch, _ = _check_sampler(batch_size_per_image, positive_fraction)
    if len(proposals) != len(targets):
        raise ValueError(f"{len(proposals)} images of proposals for {len(targets)} targets")
    props = [_boxes_on(p, device) for p in proposals]
    dev = props[0].device
    gt, gt_labels = _gt_on(targets, dev)
    m = match([torch.cat([p, g]) for p, g in zip(props, gt)], gt, high, low, allow_low_quality, "roi", gt_labels)
    s = sample(m.labels, batch, positive_fraction, source, draw, _rng.PURPOSE_SAMPLE_ROI, m.table, m.table_host)
    N = len(props)
    out = Targets(proposals=torch.empty((N, batch, 4), dtype=torch.float32, device=dev), labels=torch.empty((N, batch), dtype=torch.int64, device=dev),
                  matched=torch.empty((N, batch), dtype=torch.int64, device=dev),
                  regression_targets=torch.empty((N, batch, 4), dtype=torch.float32, device=dev), sampled=s.sampled, counts=s.counts)
    ops.launch(ops.make_targets_gather(boxes=m.boxes, gt_boxes=m.gt_boxes, matched=m.matched, labels=m.labels, table_host=m.table_host, table=m.table,
                                       sampled=s.sampled, weights=weights, out_boxes=out.proposals, out_labels=out.labels, out_matched=out.matched,
                                       out_targets=out.regression_targets))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# losses: thin torch compositions over the masks and the device counts (they need autograd, like the learned modules)
# ----------------------------------------------------------------------------------------------------------------------------------
def _masked_smooth_l1(pred, target, pos):
    """sum of smooth-L1 (beta 1/9) over the rows of ``pos``; the other rows' targets (some are infinite) never meet the prediction"""
    import torch.nn.functional as F
    keep = pos[:, None]
    loss = F.smooth_l1_loss(pred, target.masked_fill(~keep, 0.0), beta=SMOOTH_L1_BETA, reduction="none")
    return (loss * keep.to(loss.dtype)).sum()


def rpn_loss(objectness, pred_bbox_deltas, rpn_targets):
    """`RegionProposalNetwork.compute_loss` (model/faster_rcnn.py:2136-2171) over what `rpn_targets` returns: (objectness_loss,
    box_loss).  ``objectness`` [N A] or [N A, 1] and ``pred_bbox_deltas`` [N A, 4] in the order of `concat_box_prediction_layers`.
    Smooth-L1 with beta 1/9 summed over the sampled positives and divided by the sampled count; BCE-with-logits averaged over the
    sampled.  Masks and the device counts stand where the reference indexes: no `where`, no host sync."""
    import torch.nn.functional as F
    t = rpn_targets
    pos = t["mask_pos"].reshape(-1).bool()
    picked = pos | t["mask_neg"].reshape(-1).bool()
    count = t["counts"].sum().to(objectness.dtype)
    box_loss = _masked_smooth_l1(pred_bbox_deltas.reshape(-1, 4), t["regression"].reshape(-1, 4).to(pred_bbox_deltas.dtype), pos) / count
    bce = F.binary_cross_entropy_with_logits(objectness.reshape(-1), t["labels"].reshape(-1).clamp(min=0).to(objectness.dtype), reduction="none")
    return (bce * picked.to(bce.dtype)).sum() / count, box_loss


def fastrcnn_loss(class_logits, box_regression, roi_targets):
    """The reference's `fastrcnn_loss` (model/faster_rcnn.py:1402-1439) over what `roi_targets` returns: (classification_loss,
    box_loss).  ``class_logits`` [N batch, C] and ``box_regression`` [N batch, 4 C] are the box head's outputs for EVERY slot, the
    unfilled ones included: their label -1 is cross-entropy's ignore_index, and they are no positives.  No `where`, no host sync."""
    import torch.nn.functional as F
    t = roi_targets
    labels = t["labels"].reshape(-1)
    rows = labels.shape[0]
    classification_loss = F.cross_entropy(class_logits, labels, ignore_index=-1)
    pos = labels > 0
    pick = labels.clamp(min=0)[:, None, None].expand(rows, 1, 4)
    pred = box_regression.reshape(rows, -1, 4).gather(1, pick).squeeze(1)
    count = t["counts"].sum().to(box_regression.dtype)
    return classification_loss, _masked_smooth_l1(pred, t["regression_targets"].reshape(-1, 4).to(pred.dtype), pos) / count
