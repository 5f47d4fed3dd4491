"""Segmentation labels on the device: what sits between the restored image and the figure the reference's segmentation test reports
(main/seg/test_edtr.py:139-174), and the geometry its data sets apply to image and mask together (datasets/segmentation.py:82-114,
207-215).  A label map is uint8 [H, W] (255 = "ignore"), an image uint8 [h, w, 3]; the five launches are include/edtr_hip.h "Label
maps" (kernels in csrc/labels.hip).  The task networks stay outside: `evaluate` takes logits from any callable.

Three layers, as in `degrade`:
  * `resize_nearest`, `window`, `confusion`, `coarse_confusion`, `colorize`: thin wrappers over the launches (torch tensors on the device, the caller's
    stream).  With inputs already on the device nothing waits for the device; a numpy input is uploaded first (one host -> device
    copy), and `confusion`'s ``sizes`` travel in a pinned, non-blocking upload;
  * `*_reference`: the numpy restatement of each.  They are the NORMATIVE definition: the kernels are tested against them by
    equality, and they against Pillow and the reference's own functions (tests/golden/labels.npz);
  * host-side parameter code in numpy: `nearest_index` (Pillow's accumulating NEAREST rule), `voc_palette`, `compute_iou` (the
    reference's fp32 arithmetic), `SegGeometry` with the reference's YAML keys and `draw_geometry`, which draws one image's resize,
    crop and flip from ``numpy.random.default_rng([seed, image_id, GEOMETRY_WORD])`` — a stream of its own, so that
    `degrade.draw_params` / `draw_params2` return what they returned before.

`prepare_pair` / `paired_mask` are the data sets' `load_items`, `evaluate` the test loop's tail.  `coarse_confusion` takes the logits
at the network's stride and scores their bilinear upsample (model/deeplabv3.py:44-47) without storing it; `assemble_segmenter` puts
the reference's segmenter together from its learned parts so that it ends there (`CoarseLogits`).  `coarse_cross_entropy` is the
training loss on the same coarse logits (main/seg/train_edtr.py:213), forward and gathered backward without the upsample in either
direction, and `assemble_training_segmenter` the train-mode twin of `assemble_segmenter` that ends in it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

IGNORE = 255                            # the reference's "don't care" label; every target >= n is ignored
GEOMETRY_WORD = 0x47454F4D              # "GEOM": the purpose word of `draw_geometry`'s generator
CROP_TYPES = ("none", "center", "random")


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative) and host-side parameters
# ----------------------------------------------------------------------------------------------------------------------------------
def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """int32 [n_out]: the source index of every output position of `Image.resize(..., Image.NEAREST)` along one axis.  Pillow's
    ImagingScaleAffine accumulates in double — xo = 0.5 s; idx[x] = (int)xo; xo += s with s = n_in / n_out — which is NOT
    floor((x + 0.5) n_in / n_out): the two differ for many (n_in, n_out), 2 -> 7 and 500 -> 546 among them."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"sizes must be positive, got {n_in} -> {n_out}")
    s = n_in / n_out
    idx = np.empty(n_out, dtype=np.int32)
    xo = 0.5 * s
    for x in range(n_out):
        idx[x] = int(xo)
        xo += s
    return np.minimum(idx, n_in - 1)


def _u8(x, what: str) -> np.ndarray:
    x = np.ascontiguousarray(x)
    if x.dtype != np.uint8 or x.ndim not in (2, 3) or (x.ndim == 3 and x.shape[2] not in (1, 3)):
        raise TypeError(f"{what} takes a uint8 [h, w] label map or a uint8 [h, w, C] array with C of 1 or 3")
    return x


def _hw(size) -> Tuple[int, int]:
    H, W = (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))
    if H <= 0 or W <= 0:
        raise ValueError(f"an extent must be positive, got {H} x {W}")
    return H, W


def resize_nearest_reference(x, size) -> np.ndarray:
    """`Image.fromarray(x).resize((W, H), Image.NEAREST)` for ``size`` = (H, W): a gather through `nearest_index` of each axis"""
    x = _u8(x, "resize_nearest_reference")
    H, W = _hw(size)
    return np.ascontiguousarray(x[nearest_index(x.shape[0], H)][:, nearest_index(x.shape[1], W)])


def window_reference(x, out_hw, origin=(0, 0), hflip: bool = False, vflip: bool = False, fill: int = 0) -> np.ndarray:
    """out (y, x) = x (y0 + y', x0 + x'), y' = H - 1 - y under ``vflip``, x' = W - 1 - x under ``hflip``; ``fill`` outside the source:
    np.pad(constant), a crop at ``origin`` = (y0, x0) and the two flips of `augment` at once."""
    x = _u8(x, "window_reference")
    H, W = _hw(out_hw)
    y0, x0 = int(origin[0]), int(origin[1])
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"fill must be a byte, got {fill}")
    sy = y0 + (np.arange(H)[::-1] if vflip else np.arange(H))
    sx = x0 + (np.arange(W)[::-1] if hflip else np.arange(W))
    inside = ((sy >= 0) & (sy < x.shape[0]))[:, None] & ((sx >= 0) & (sx < x.shape[1]))[None, :]
    got = x[np.clip(sy, 0, x.shape[0] - 1)][:, np.clip(sx, 0, x.shape[1] - 1)]
    return np.ascontiguousarray(np.where(inside if x.ndim == 2 else inside[:, :, None], got, np.uint8(fill)).astype(np.uint8))


def argmax_reference(logits) -> np.ndarray:
    """uint8 argmax over axis 1 by torch's CPU rule, which is numpy's: the first NaN if there is one, else the first maximum
    (-0.0 == 0.0 is a tie)"""
    return np.argmax(np.asarray(logits), axis=1).astype(np.uint8)


def confusion_reference(logits, target, n: Optional[int] = None, sizes=None, return_pred: bool = False):
    """int64 [n, n]: `calculate_mat(target, argmax(logits), n)` as main/seg/test_edtr.py:159 calls it — a pixel counts iff its target is
    < n and then adds 1 to mat[target][argmax]; with ``sizes`` only the top-left (h, w) of image b counts.  ``logits`` [B, n, H, W]
    (any float type numpy holds; widen bf16 to fp32 first), ``target`` uint8 [B, H, W]."""
    logits = np.asarray(logits)
    target = np.asarray(target)
    if logits.ndim != 4 or target.shape != logits.shape[:1] + logits.shape[2:] or target.dtype != np.uint8:
        raise ValueError(f"expected logits [B, n, H, W] and a uint8 target [B, H, W], got {logits.shape} and {target.shape} {target.dtype}")
    n = logits.shape[1] if n is None else int(n)
    if n != logits.shape[1]:
        raise ValueError(f"{logits.shape[1]} logit planes for n = {n}")
    pred = argmax_reference(logits)
    keep = target < n
    if sizes is not None:
        B, H, W = target.shape
        for b, (h, w) in enumerate(sizes):
            if not (0 < int(h) <= H and 0 < int(w) <= W):
                raise ValueError(f"a {h} x {w} extent lies outside the {H} x {W} slot")
            keep[b, int(h):, :] = False
            keep[b, :, int(w):] = False
    inds = n * target[keep].astype(np.int64) + pred[keep]
    mat = np.bincount(inds, minlength=n * n).reshape(n, n).astype(np.int64)
    return (mat, pred) if return_pred else mat


LOGIT_TYPES = ("float32", "float16", "bfloat16")


def _round_to(v: np.ndarray, dtype: str) -> np.ndarray:
    """fp32 ``v`` rounded to nearest even to ``dtype`` and widened back to fp32 (bfloat16 in integer arithmetic on the bits; a NaN
    stays a NaN)"""
    if dtype == "float32":
        return v
    with np.errstate(over="ignore"):
        if dtype == "float16":
            return v.astype(np.float16).astype(np.float32)
    u = np.ascontiguousarray(v).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isnan(v), np.float32(np.nan), r)


def upsample_logits_reference(coarse, size, dtype: str = "float32") -> np.ndarray:
    """fp32 [B, n, H, W]: what `F.interpolate(coarse, size=size, mode="bilinear", align_corners=False)` hands to argmax, by the
    written rule of `degrade.resize_reference` (ATen's fp32 arithmetic, every product and sum rounded) for any number of planes.
    ``dtype`` is the type the logits are held in: "float16" / "bfloat16" values (given as fp16, or as fp32 that holds them — bf16
    travels widened) are widened exactly, blended in fp32, and the blend is rounded once to that type, which is what makes many more
    ties than fp32 has."""
    from . import degrade
    if dtype not in LOGIT_TYPES:
        raise ValueError(f"dtype must be one of {LOGIT_TYPES}, got {dtype!r}")
    x = np.asarray(coarse)
    if x.ndim != 4 or x.dtype not in (np.float32, np.float16) or 0 in x.shape:
        raise ValueError(f"expected fp32 / fp16 logits [B, n, ih, iw], got {x.dtype} {x.shape}")
    x = np.ascontiguousarray(x.astype(np.float32))
    if dtype != "float32" and not np.array_equal(_round_to(x, dtype), x, equal_nan=True):
        raise ValueError(f"the logits hold values that are not {dtype} values")
    H, W = _hw(size)
    with np.errstate(invalid="ignore", over="ignore"):
        return _round_to(degrade.bilinear_planes_reference(x, H, W), dtype)


def coarse_confusion_reference(coarse, target, size=None, n: Optional[int] = None, sizes=None, return_pred: bool = False,
                               dtype: str = "float32"):
    """`confusion_reference` of `upsample_logits_reference`: ``coarse`` [B, n, ih, iw] stands for its upsample to ``size`` (default:
    the extent of ``target`` uint8 [B, H, W]).  NORMATIVE for `coarse_confusion`: the launch equals it word for word, mat and pred."""
    target = np.asarray(target)
    if target.ndim != 3:
        raise ValueError(f"expected a uint8 target [B, H, W], got {target.shape}")
    return confusion_reference(upsample_logits_reference(coarse, target.shape[1:] if size is None else size, dtype), target, n, sizes,
                               return_pred)


SEG_CE_MAX_CLASSES = 256                # EDTR_SEG_CE_MAX_CLASSES
CE_TILE = (16, 64)                      # the output tile whose fp64 sum is one addend of the loss


def _ce_inputs(coarse, target, size, dtype):
    """(logits as fp32 [B, n, ih, iw], target uint8 [B, H, W]) of the two cross-entropy restatements, checked"""
    if dtype not in LOGIT_TYPES:
        raise ValueError(f"dtype must be one of {LOGIT_TYPES}, got {dtype!r}")
    x, target = np.asarray(coarse), np.asarray(target)
    if x.ndim != 4 or x.dtype not in (np.float32, np.float16) or 0 in x.shape:
        raise ValueError(f"expected fp32 / fp16 logits [B, n, ih, iw], got {x.dtype} {x.shape}")
    if x.shape[1] > SEG_CE_MAX_CLASSES:
        raise ValueError(f"at most {SEG_CE_MAX_CLASSES} classes, got {x.shape[1]}")
    if target.dtype != np.uint8 or target.ndim != 3 or target.shape[0] != x.shape[0] or 0 in target.shape:
        raise ValueError(f"target must be uint8 [B, H, W] with the logits' batch, got {target.dtype} {target.shape}")
    if size is not None and _hw(size) != tuple(target.shape[1:]):
        raise ValueError(f"size {_hw(size)} is not the target's extent {tuple(target.shape[1:])}")
    return np.ascontiguousarray(x.astype(np.float32)), target


def _tile_sum(tile: np.ndarray) -> float:
    """fp64 [16, 64] -> its sum in the order of the launch: a lane's four pixels left to right, then lane i += lane i + o for o = 128 ... 1"""
    lane = tile.reshape(16, 16, 4)
    v = (((lane[:, :, 0] + lane[:, :, 1]) + lane[:, :, 2]) + lane[:, :, 3]).reshape(256).copy()
    o = 128
    while o:
        v[:o] = v[:o] + v[o:2 * o]
        o >>= 1
    return float(v[0])


def coarse_cross_entropy_reference(coarse, target, size=None, ignore_index: int = 255, dtype: str = "float32"):
    """`F.cross_entropy(F.interpolate(coarse, size=, mode="bilinear", align_corners=False), target, ignore_index=)` by a written rule;
    NORMATIVE for `coarse_cross_entropy`.  Returns (loss fp32, lse fp32 [B, H, W], count, bad).
      z_c    `upsample_logits_reference`: seven rounded fp32 operations and, for 16-bit logits, the rounding to that type (what
             torch's interpolate returns under autocast; cross_entropy itself runs in fp32)
      lse    m + log(sum_c exp(z_c - m)), m the maximum over c, the sum over c ascending from 0, every step one rounded fp32 operation.
             (The launch takes the planes once with a running maximum and rescales its sum where the maximum moves: the same
             quantity with a few more roundings, inside the bound the tests derive.)
      count  pixels with target != ignore_index and target < n.  A target with n <= t != ignore_index makes torch RAISE; here it is
             IGNORED and counted in ``bad``, so that nothing has to wait for the device to find out.
      loss   float32(sum of float32(lse - z_target) over the counted pixels / count), the sum in fp64 in an order the shape alone
             decides: per 16 x 64 output tile (`_tile_sum`), then over the tiles ascending.  count == 0 gives NaN, torch's answer."""
    x, target = _ce_inputs(coarse, target, size, dtype)
    n = x.shape[1]
    B, H, W = target.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = upsample_logits_reference(x, (H, W), dtype)
        m = z.max(axis=1)
        s = np.zeros_like(m)
        for c in range(n):
            s = s + np.exp(z[:, c] - m)
        lse = (m + np.log(s)).astype(np.float32)
        t = target.astype(np.int64)
        keep = (t != int(ignore_index)) & (t < n)
        bad = int(np.count_nonzero((t >= n) & (t != int(ignore_index))))
        zt = np.take_along_axis(z, np.minimum(t, n - 1)[:, None], axis=1)[:, 0]
        ell = np.where(keep, (lse - zt).astype(np.float32), np.float32(0)).astype(np.float64)
    th, tw = CE_TILE
    padded = np.zeros((B, -(-H // th) * th, -(-W // tw) * tw), dtype=np.float64)
    padded[:, :H, :W] = ell
    total = 0.0
    for b in range(B):
        for y in range(0, padded.shape[1], th):
            for x0 in range(0, padded.shape[2], tw):
                total = total + _tile_sum(padded[b, y:y + th, x0:x0 + tw])
    count = int(np.count_nonzero(keep))
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float32(np.float64(total) / np.float64(count))
    return loss, lse, count, bad


def coarse_cross_entropy_backward_reference(coarse, target, lse, count, grad_loss=1.0, size=None, ignore_index: int = 255,
                                            dtype: str = "float32") -> np.ndarray:
    """The gradient of `coarse_cross_entropy_reference`'s loss in ``coarse``, times ``grad_loss``: fp32 [B, n, ih, iw] that holds values
    of ``dtype``.  NORMATIVE for the backward launch; ``lse`` and ``count`` are what the forward returned.  The exact adjoint of the
    forward's rule: element (b, c, i, j) is the sum, over the output pixels whose row taps and column taps land on (i, j), of
    row weight * column weight * (exp(z_c - lse) - [c == target]) * (grad_loss / count); ignored pixels contribute nothing.  In fp32,
    every product, sum and difference rounded on its own, in a fixed two-level order:
      g = float32(grad_loss) / float32(count);  per pixel e = (exp(z_c - lse) - [c == t]) * g
      per output row y:  r_j = 0; for x ascending: r_{j0(x)} += (1 - tx) * e, then r_{j1(x)} += tx * e
      acc_ij = 0; for y ascending: acc_{i0(y), j} += (1 - ty) * r_j, then acc_{i1(y), j} += ty * r_j
    with (i0, i1, t) of `upsample_logits_reference`.  Where an edge clamp puts both taps of an axis on one position (i0 == i1 at the last
    row or column, where t can be non-zero), both weights land there, 1 - t first.  A position no pixel reaches (down-sampling)
    gets +0.0, and with count == 0 every element is +0.0, torch's answer.  The fp32 sum is rounded ONCE to a 16-bit ``dtype``: a
    deliberate difference from torch, which rounds the upstream gradient to 16 bits before it is scattered."""
    from . import degrade
    x, target = _ce_inputs(coarse, target, size, dtype)
    B, n, ih, iw = x.shape
    _, H, W = target.shape
    lse = np.asarray(lse, dtype=np.float32)
    if lse.shape != target.shape:
        raise ValueError(f"lse must be fp32 [B, H, W] like the target, got {lse.shape}")
    out = np.zeros(x.shape, dtype=np.float32)
    if int(count) <= 0:
        return out
    g = np.float32(grad_loss) / np.float32(int(count))
    y0, ty = degrade._index_lambda(np.maximum(degrade._source_index(ih, H), np.float32(0)), ih)
    x0, tx = degrade._index_lambda(np.maximum(degrade._source_index(iw, W), np.float32(0)), iw)
    y1, x1 = y0 + (y0 < ih - 1), x0 + (x0 < iw - 1)
    wy0, wx0 = np.float32(1) - ty, np.float32(1) - tx
    t = target.astype(np.int64)
    keep = (t != int(ignore_index)) & (t < n)
    with np.errstate(invalid="ignore", over="ignore"):
        z = upsample_logits_reference(x, (H, W), dtype)
        hot = (np.arange(n)[None, :, None, None] == t[:, None]).astype(np.float32)
        e = ((np.exp(z - lse[:, None]) - hot) * g).astype(np.float32)
        e = np.where(keep[:, None], e, np.float32(0))
        r = np.zeros((B, n, H, iw), dtype=np.float32)
        for xx in range(W):
            r[:, :, :, x0[xx]] = r[:, :, :, x0[xx]] + wx0[xx] * e[:, :, :, xx]
            r[:, :, :, x1[xx]] = r[:, :, :, x1[xx]] + tx[xx] * e[:, :, :, xx]
        for yy in range(H):
            out[:, :, y0[yy], :] = out[:, :, y0[yy], :] + wy0[yy] * r[:, :, yy, :]
            out[:, :, y1[yy], :] = out[:, :, y1[yy], :] + ty[yy] * r[:, :, yy, :]
        return _round_to(out, dtype)


def compute_iou(mat) -> np.ndarray:
    """fp32 [n]: diag / (row sums + column sums - diag) on float32(mat), the reference's compute_iou (utils/segmentation.py:105-108).
    A class absent from truth and prediction alike is 0 / 0 = NaN, and a mean over it is NaN: the reference's behaviour, kept.
    Equal to the reference bit for bit while every row and column sum stays below 2^24 (all partial sums are then exact in fp32).
    Beyond that — a whole VOC validation set counts about 3.6e8 pixels — numpy and torch add the 21 terms in different orders (torch's
    is a detail of its CPU reduction kernels); each sum is then within 20 * 2^-24 relative of the exact one, the union
    rows + columns - diagonal has no cancellation (it is at least either sum), and an IoU can differ from the reference's by up to
    about 100 * 2^-24 = 6e-6 relative (tests/golden/labels.npz holds such a matrix; the CPU test asserts that bound)."""
    h = np.asarray(mat).astype(np.float32)
    if h.ndim != 2 or h.shape[0] != h.shape[1]:
        raise ValueError(f"a confusion matrix is square, got {h.shape}")
    d = np.diag(h)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (d / (h.sum(1, dtype=np.float32) + h.sum(0, dtype=np.float32) - d)).astype(np.float32)


def mean_iou(mat) -> float:
    """`compute_iou(confmat).mean().item() * 100` (main/seg/test_edtr.py:174)"""
    return float(np.mean(compute_iou(mat), dtype=np.float32)) * 100


def voc_palette() -> np.ndarray:
    """uint8 [256, 3]: the standard PASCAL-VOC colour map by its bit-reversal rule — bit j of channel c of label i is bit 3 j + c of i,
    placed at bit 7 - j"""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        c = i
        for j in range(8):
            for ch in range(3):
                pal[i, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    return pal


def _palette(palette) -> np.ndarray:
    if palette is None:
        return voc_palette()
    p = np.asarray(palette)
    if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= 256:
        raise TypeError("a palette is a uint8 [k, 3] array with k <= 256 (labels from k on come out black)")
    full = np.zeros((256, 3), dtype=np.uint8)
    full[:p.shape[0]] = p
    return full


def colorize_reference(labels, palette=None) -> np.ndarray:
    """uint8 [..., 3] = palette[labels]: the bytes save_image writes for convert2color's mask"""
    labels = np.asarray(labels)
    if labels.dtype != np.uint8:
        raise TypeError("colorize_reference takes uint8 labels")
    return _palette(palette)[labels]


# ----------------------------------------------------------------------------------------------------------------------------------
# geometry of the reference's segmentation data sets
# ----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class SegGeometry:
    """The geometry keys of DegradedSegmentationDataset (configs/seg/*/train/*.yaml, `dataset.train.params`).  ``resize_range`` None:
    r = 1; ``out_size`` None: no padding (and then no crop)."""
    gt_size: int = 560
    resize_range: Optional[Sequence[float]] = None
    out_size: Optional[int] = 512
    crop_type: str = "center"
    hflip: bool = False
    rotation: bool = False

    KEYS = ("gt_size", "resize_range", "out_size", "crop_type", "hflip", "rotation")

    def __post_init__(self):
        if self.rotation:
            # the reference's rot90 branch calls transpose(1, 0, 2) on the 2-D mask and cannot run; every seg config sets rotation: false
            raise NotImplementedError("rotation is not provided: the reference's own rotation cannot run on a mask")
        if int(self.gt_size) <= 0:
            raise ValueError(f"gt_size must be positive, got {self.gt_size}")
        if self.crop_type not in CROP_TYPES:
            raise ValueError(f"crop_type must be one of {CROP_TYPES}, got {self.crop_type!r}")
        if self.out_size is not None and int(self.out_size) <= 0:
            raise ValueError(f"out_size must be positive, got {self.out_size}")
        if self.crop_type != "none" and self.out_size is None:
            raise ValueError("a crop needs an out_size")
        if self.resize_range is not None and not (len(self.resize_range) == 2 and 0 < float(self.resize_range[0]) <= float(self.resize_range[1])):
            raise ValueError(f"resize_range must be [a, b] with 0 < a <= b, got {list(self.resize_range)}")

    @classmethod
    def from_dict(cls, d: dict) -> "SegGeometry":
        """From a mapping that holds the keys at its top level, under dataset.params or under dataset.train.params / dataset.val.params
        as the reference's configs do; other keys are ignored."""
        def find(node):
            if not isinstance(node, dict):
                return None
            if "gt_size" in node:
                return node
            for key in ("dataset", "train", "val", "params"):
                hit = find(node.get(key))
                if hit is not None:
                    return hit
            return None
        node = find(d)
        if node is None:
            raise ValueError("no gt_size key: not a geometry of the reference's segmentation data sets")
        return cls(**{k: node[k] for k in cls.KEYS if k in node})


def load_geometry(spec) -> SegGeometry:
    """A `SegGeometry`, a mapping with its keys, or the path of a YAML file that holds them"""
    if isinstance(spec, SegGeometry):
        return spec
    if isinstance(spec, dict):
        return SegGeometry.from_dict(spec)
    try:
        import yaml
    except ImportError as e:
        raise RuntimeError("reading a YAML geometry needs PyYAML (`import yaml` failed)") from e
    with open(spec) as fh:
        return SegGeometry.from_dict(yaml.safe_load(fh))


@dataclass
class GeometryParams:
    """What `draw_geometry` fixed for one image: resize to ``size``, pad by ``pad`` at the bottom / right, cut ``out_hw`` at ``origin``
    of the padded image, flip."""
    size: Tuple[int, int]               # (h, w) after the resize
    pad: Tuple[int, int]                # (rows, columns) added at the bottom / right
    origin: Tuple[int, int]             # (y0, x0) of the crop in the padded image
    out_hw: Tuple[int, int]
    hflip: bool


def resized_extent(gt_size: int, h: int, w: int, r: float = 1.0) -> Tuple[int, int]:
    """(h', w') of datasets/segmentation.py:86-92 with its order of operations: the shorter side to int(gt_size * r), the longer one
    to int(gt_size * long / short * r)"""
    if w >= h:
        ow, oh = int(gt_size * w / h * r), int(gt_size * r)
    else:
        ow, oh = int(gt_size * r), int(gt_size * h / w * r)
    if oh <= 0 or ow <= 0:
        raise ValueError(f"gt_size {gt_size} and r {r} leave nothing of a {h} x {w} image")
    return oh, ow


def draw_geometry(cfg: SegGeometry, seed: int, image_id: int, hw: Tuple[int, int]) -> GeometryParams:
    """One image's geometry from ``numpy.random.default_rng([seed, image_id, GEOMETRY_WORD])``: a function of the configuration, the
    seed, the image's data-set index and its extent.  Four uniform draws, made whether or not they are used: r, the crop's row, its
    column, the flip."""
    seed, image_id = int(seed), int(image_id)
    if not 0 <= seed < 1 << 64 or not 0 <= image_id < 1 << 32:
        raise ValueError(f"seed must be in [0, 2^64) and image_id in [0, 2^32), got {seed} and {image_id}")
    h, w = int(hw[0]), int(hw[1])
    if h <= 0 or w <= 0:
        raise ValueError(f"an image extent must be positive, got {h} x {w}")
    gen = np.random.default_rng([seed, image_id, GEOMETRY_WORD])
    u_r, u_y, u_x, u_flip = (float(gen.uniform()) for _ in range(4))
    r = 1.0
    if cfg.resize_range is not None:
        r = float(cfg.resize_range[0]) + u_r * (float(cfg.resize_range[1]) - float(cfg.resize_range[0]))
    rh, rw = resized_extent(int(cfg.gt_size), h, w, r)
    out = None if cfg.out_size is None else int(cfg.out_size)
    ph, pw = (0, 0) if out is None else (max(out - rh, 0), max(out - rw, 0))
    H, W = rh + ph, rw + pw
    if cfg.crop_type == "none":
        origin, out_hw = (0, 0), (H, W)
    elif cfg.crop_type == "center":
        origin, out_hw = ((H - out) // 2, (W - out) // 2), (out, out)
    else:
        origin, out_hw = (min(int(u_y * (H - out + 1)), H - out), min(int(u_x * (W - out + 1)), W - out)), (out, out)
    return GeometryParams((rh, rw), (ph, pw), origin, out_hw, bool(cfg.hflip and u_flip < 0.5))


def prepare_pair_reference(image_u8, mask_u8, geom: GeometryParams):
    """numpy restatement of `prepare_pair`: (gt uint8 [H, W, 3], mask uint8 [H, W])"""
    from .imageio import resize_u8_reference
    rh, rw = geom.size
    gt = window_reference(resize_u8_reference(np.asarray(image_u8), rw, rh), geom.out_hw, geom.origin, geom.hflip, False, 0)
    mask = window_reference(resize_nearest_reference(mask_u8, (rh, rw)), geom.out_hw, geom.origin, geom.hflip, False, IGNORE)
    return gt, mask


def _center_origin(hw, center_crop) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    c = _hw(center_crop)
    if hw[0] < c[0] or hw[1] < c[1]:
        raise ValueError(f"a {hw[0]} x {hw[1]} mask is smaller than the {c[0]} x {c[1]} centre crop")
    return ((hw[0] - c[0]) // 2, (hw[1] - c[1]) // 2), c


def paired_mask_reference(mask_u8, gt_hw, center_crop=None) -> np.ndarray:
    """numpy restatement of `paired_mask`"""
    m = resize_nearest_reference(mask_u8, gt_hw)
    if center_crop is None:
        return m
    origin, c = _center_origin(m.shape[:2], center_crop)
    return window_reference(m, c, origin, fill=IGNORE)


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
INDEX_TABLES_KEPT = 64


def _index_on(n_in: int, n_out: int, device):
    from .imageio import on_device
    return on_device(("nearest_index", n_in, n_out), device, lambda: nearest_index(n_in, n_out), kept=INDEX_TABLES_KEPT)


def _on_device(x, device, what: str):
    """``x`` (numpy array or torch tensor, uint8 [h, w] or [h, w, C]) as a contiguous uint8 [h, w, C] device tensor, and whether it was 2-D"""
    import torch
    from .imageio import _device
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.ndim not in (2, 3) or (t.ndim == 3 and t.shape[2] not in (1, 3)):
        raise TypeError(f"{what} takes a uint8 [h, w] label map or a uint8 [h, w, C] image with C of 1 or 3")
    dev = t.device if t.is_cuda and device is None else _device(device)
    flat = t.ndim == 2
    t = t.to(dev).contiguous()
    return (t[:, :, None] if flat else t), flat


def resize_nearest(x, size, device=None):
    """`resize_nearest_reference` on the device: ``size`` = (H, W)"""
    import torch
    from . import ops
    src, flat = _on_device(x, device, "resize_nearest")
    H, W = _hw(size)
    dst = torch.empty((H, W, src.shape[2]), dtype=torch.uint8, device=src.device)
    ops.launch(ops.make_label_resize_nearest(src=src, dst=dst, y_idx=_index_on(src.shape[0], H, src.device),
                                             x_idx=_index_on(src.shape[1], W, src.device)))
    return dst[:, :, 0] if flat else dst


def window(x, out_hw, origin=(0, 0), hflip: bool = False, vflip: bool = False, fill: int = 0, device=None):
    """`window_reference` on the device"""
    import torch
    from . import ops
    src, flat = _on_device(x, device, "window")
    H, W = _hw(out_hw)
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"fill must be a byte, got {fill}")
    dst = torch.empty((H, W, src.shape[2]), dtype=torch.uint8, device=src.device)
    ops.launch(ops.make_label_window(src=src, dst=dst, y0=int(origin[0]), x0=int(origin[1]), hflip=hflip, vflip=vflip, fill=int(fill)))
    return dst[:, :, 0] if flat else dst


def _logits_and_target(what: str, logits, target, full: bool):
    """What every launch on logits and a label map checks first: contiguous [B, n, H, W] logits on the device and a uint8 [B, H, W]
    target of their batch, which is returned on their device.  ``full``: its extent must be the logits' (else any [B, H, W] is taken)."""
    import torch
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.ndim != 4 or not logits.is_contiguous():
        raise TypeError(f"{what} takes a contiguous [B, n, H, W] logits tensor on the device")
    target = torch.as_tensor(target)
    fits = target.ndim == 3 and target.shape[0] == logits.shape[0] and (tuple(target.shape[1:]) == tuple(logits.shape[2:]) if full
                                                                         else 0 not in target.shape)
    if target.dtype != torch.uint8 or not fits:
        raise ValueError(f"target must be uint8 [B, H, W] matching the logits, got {target.dtype} {tuple(target.shape)}")
    return target.to(logits.device).contiguous()


def _confusion_args(what: str, logits, target, n, sizes, mat, return_pred: bool, full: bool):
    """The argument checks `confusion` and `coarse_confusion` share; returns (target on the device, sizes, mat, pred or None).
    ``full``: the target's extent must be the logits' (else any [B, H, W] is taken)."""
    import torch
    if isinstance(logits, torch.Tensor) and logits.ndim == 4 and logits.shape[1] != int(n):
        raise ValueError(f"{logits.shape[1]} logit planes for n = {n}")
    target = _logits_and_target(what, logits, target, full)
    if sizes is not None:
        sizes = [(int(h), int(w)) for h, w in sizes]
        if len(sizes) != logits.shape[0]:
            raise ValueError(f"{len(sizes)} sizes for a batch of {logits.shape[0]}")
    if mat is None:
        mat = torch.zeros((int(n), int(n)), dtype=torch.int64, device=logits.device)
    elif mat.dtype != torch.int64 or tuple(mat.shape) != (int(n), int(n)) or not mat.is_contiguous() or mat.device != logits.device:
        raise TypeError(f"mat must be a contiguous int64 [{n}, {n}] tensor on the logits' device")
    pred = torch.empty(target.shape, dtype=torch.uint8, device=logits.device) if return_pred else None
    return target, sizes, mat, pred


def confusion(logits, target, n: int = 21, sizes=None, mat=None, return_pred: bool = False, max_blocks: int = 0):
    """`confusion_reference` on the device, one launch: ``logits`` a contiguous fp32 / fp16 / bf16 [B, n, H, W] tensor, ``target`` uint8
    [B, H, W].  ``mat`` (int64 [n, n] on the device) is ADDED to and returned; without it a zeroed one is made.  ``max_blocks`` caps
    the grid (0: the default cap).  Returns mat, or (mat, pred uint8 [B, H, W]) with ``return_pred``; nothing is brought to the host,
    and with ``target`` on the device the call does not wait for it (a host ``target`` is uploaded first)."""
    from . import ops
    target, sizes, mat, pred = _confusion_args("confusion", logits, target, n, sizes, mat, return_pred, full=True)
    ops.launch(ops.make_seg_confusion(logits=logits, target=target, mat=mat, sizes=sizes, pred=pred, max_blocks=int(max_blocks)))
    return (mat, pred) if return_pred else mat


def coarse_confusion(coarse, target, n: int = 21, sizes=None, mat=None, return_pred: bool = False, max_blocks: int = 0):
    """`coarse_confusion_reference` on the device, one launch: `confusion` of the bilinear upsample of ``coarse`` (a contiguous fp32 /
    fp16 / bf16 [B, n, ih, iw] tensor at the network's stride) to the extent of ``target`` (uint8 [B, H, W]), without the [B, n, H, W]
    tensor ever being stored.  A 16-bit ``coarse`` is compared as `F.interpolate` would return it: blended in fp32, rounded to its
    type.  ``sizes``, ``mat``, ``return_pred``, ``max_blocks``, the return value and what does not wait for the device: as `confusion`."""
    from . import ops
    target, sizes, mat, pred = _confusion_args("coarse_confusion", coarse, target, n, sizes, mat, return_pred, full=False)
    ops.launch(ops.make_seg_confusion_coarse(coarse=coarse, target=target, mat=mat, sizes=sizes, pred=pred, max_blocks=int(max_blocks)))
    return (mat, pred) if return_pred else mat


def _palette_on(palette, device):
    import torch
    from .imageio import on_device
    if palette is not None:
        return torch.from_numpy(_palette(palette)).to(device)
    return on_device(("voc_palette",), device, voc_palette)


def colorize(labels, palette=None, device=None):
    """`colorize_reference` on the device: uint8 [H, W] or [B, H, W] labels -> uint8 [..., 3]; ``palette`` None (`voc_palette`) or a
    uint8 [k, 3] array"""
    import torch
    from . import ops
    from .imageio import _device
    t = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.ndim not in (2, 3):
        raise TypeError("colorize takes uint8 [H, W] or [B, H, W] labels")
    dev = t.device if t.is_cuda and device is None else _device(device)
    t = t.to(dev).contiguous()
    dst = torch.empty(tuple(t.shape) + (3,), dtype=torch.uint8, device=dev)
    ops.launch(ops.make_label_colorize(labels=t if t.ndim == 3 else t[None], palette=_palette_on(palette, dev), dst=dst))
    return dst


def prepare_pair(image_u8, mask_u8, geom: GeometryParams, device=None):
    """`load_items` of DegradedSegmentationDataset for one decoded pair under the geometry `draw_geometry` fixed: the image through the
    BICUBIC `imageio.resize_u8`, the mask through `resize_nearest`, then one `window` launch each (fill 0 against fill 255).
    Returns (gt uint8 [H, W, 3], mask uint8 [H, W]) on the device."""
    gt = prepare_image(image_u8, geom, device)
    return gt, prepare_mask(mask_u8, geom, gt.device)


def prepare_image(image_u8, geom: GeometryParams, device=None):
    """the image half of `prepare_pair`"""
    from . import imageio
    rh, rw = geom.size
    return window(imageio.resize_u8(image_u8, rw, rh, device=device), geom.out_hw, geom.origin, geom.hflip, False, 0)


def prepare_mask(mask_u8, geom: GeometryParams, device=None):
    """the mask half of `prepare_pair`"""
    if getattr(mask_u8, "ndim", 0) != 2:
        raise TypeError("a mask is a uint8 [h, w] label map")
    return window(resize_nearest(mask_u8, geom.size, device=device), geom.out_hw, geom.origin, geom.hflip, False, IGNORE)


def paired_mask(mask_u8, gt_hw, center_crop=None, device=None):
    """The mask of PairedSegmentationDataset.load_items: NEAREST to the ground-truth extent ``gt_hw`` = (h, w), then the centre crop of
    ``center_crop`` (the reference's is 512).  A mask smaller than the crop raises ValueError, where the reference would slice with a
    negative origin."""
    H, W = _hw(gt_hw)
    if center_crop is None:
        return resize_nearest(mask_u8, (H, W), device=device)
    origin, c = _center_origin((H, W), center_crop)
    return window(resize_nearest(mask_u8, (H, W), device=device), c, origin, fill=IGNORE)


@dataclass
class CoarseLogits:
    """Logits still at the network's stride: ``logits`` [B, n, ih, iw] on the device and the extent ``size`` = (H, W) their bilinear
    upsample (`F.interpolate(..., size=size, mode="bilinear", align_corners=False)`) would have.  `coarse_confusion` scores them
    without that upsample being stored; `evaluate` takes one wherever it takes logits."""
    logits: object
    size: Tuple[int, int]

    def __post_init__(self):
        self.size = _hw(self.size)
        if getattr(self.logits, "ndim", 0) != 4:
            raise TypeError("CoarseLogits holds a [B, n, ih, iw] tensor")


def assemble_segmenter(backbone, classifier, feature: str = "C5", normalize: bool = True):
    """The body of the reference's `_SimpleSegmentationModel.forward` (model/deeplabv3.py:36-47) from its learned parts, without the
    aux head and without the final upsample: a callable from a contiguous fp32 [1, 3, h, w] device tensor to `CoarseLogits` of
    extent (h, w).  ``normalize``: `cls.normalize` with the ImageNet constants first (the reference's segmenters normalise inside
    their forward; the input itself is not written); then ``backbone`` — a torch module that returns the feature tensor or a mapping
    that holds it under ``feature`` — and ``classifier``, both plain torch and the user's.  No [B, n, h, w] tensor is allocated: what
    `evaluate` does with the result is one `coarse_confusion` launch."""
    def segnet(x):
        import torch
        from . import cls
        with torch.no_grad():
            size = tuple(x.shape[-2:])
            feats = backbone(cls.normalize(x) if normalize else x)
            return CoarseLogits(classifier(feats[feature] if hasattr(feats, "keys") else feats), size)

    return segnet


def _ce_forward(coarse, target, ignore_index: int, max_blocks: int):
    """the forward launches: (loss fp32 [], counts int64 [2], lse fp32 [B, H, W]) on the device"""
    import torch
    from . import ops
    B, H, W = target.shape
    dev = coarse.device
    lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    workspace = torch.empty((ops.seg_ce_workspace(B, H, W),), dtype=torch.uint8, device=dev)
    ops.launch(ops.make_seg_ce_forward(coarse=coarse, target=target, lse=lse, workspace=workspace, loss=loss, counts=counts,
                                       ignore_index=ignore_index, max_blocks=max_blocks))
    return loss, counts, lse


def coarse_cross_entropy_backward(coarse, target, lse, counts, grad_loss, ignore_index: int = 255, max_blocks: int = 0):
    """`coarse_cross_entropy_backward_reference` on the device, one launch: the gradient [B, n, ih, iw] in the type of ``coarse`` from
    the ``lse`` and ``counts`` of the forward (`coarse_cross_entropy(..., return_saved=True)`) and the upstream gradient ``grad_loss``, a
    number or an fp32 device scalar.  A gather with a fixed order: two calls give the same bits, and every element is written."""
    import torch
    from . import ops
    target = _logits_and_target("coarse_cross_entropy_backward", coarse, target, full=False)
    if not (isinstance(lse, torch.Tensor) and lse.dtype == torch.float32 and lse.shape == target.shape and lse.is_contiguous()
            and lse.device == coarse.device):
        raise TypeError("lse must be the contiguous fp32 [B, H, W] tensor the forward wrote")
    if not (isinstance(counts, torch.Tensor) and counts.dtype == torch.int64 and counts.numel() == 2 and counts.device == coarse.device):
        raise TypeError("counts must be the int64 [2] tensor the forward wrote")
    g = grad_loss if isinstance(grad_loss, torch.Tensor) else torch.tensor(float(grad_loss), dtype=torch.float32)
    if g.numel() != 1:
        raise ValueError("grad_loss is one number")
    g = g.to(device=coarse.device, dtype=torch.float32).contiguous()
    grad = torch.empty_like(coarse)
    ops.launch(ops.make_seg_ce_backward(coarse=coarse, target=target, lse=lse, counts=counts, grad_loss=g, grad=grad,
                                        ignore_index=int(ignore_index), max_blocks=int(max_blocks)))
    return grad


_CE_FUNCTION = None


def _ce_function():
    """the autograd.Function behind a `coarse_cross_entropy` whose logits require grad (made on first use: this module imports without torch)"""
    global _CE_FUNCTION
    if _CE_FUNCTION is None:
        import torch
        from torch.autograd.function import once_differentiable

        class CoarseCrossEntropy(torch.autograd.Function):
            @staticmethod
            def forward(ctx, coarse, target, ignore_index, max_blocks):
                loss, counts, lse = _ce_forward(coarse.detach(), target, ignore_index, max_blocks)
                ctx.save_for_backward(coarse, target, lse, counts)
                ctx.ignore_index, ctx.max_blocks = ignore_index, max_blocks
                ctx.mark_non_differentiable(counts)
                return loss, counts

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_loss, _):
                coarse, target, lse, counts = ctx.saved_tensors
                return coarse_cross_entropy_backward(coarse.detach(), target, lse, counts, grad_loss, ctx.ignore_index, ctx.max_blocks), None, None, None

        _CE_FUNCTION = CoarseCrossEntropy
    return _CE_FUNCTION


def coarse_cross_entropy(coarse, target, size=None, ignore_index: int = 255, return_counts: bool = False, max_blocks: int = 0,
                         return_saved: bool = False):
    """`coarse_cross_entropy_reference` on the device: `F.cross_entropy(F.interpolate(coarse, size, mode="bilinear"), target,
    ignore_index=)` of ``coarse`` (a contiguous fp32 / fp16 / bf16 [B, n, ih, iw] device tensor, n <= 256, or a `CoarseLogits` in place
    of (coarse, size)) against ``target`` uint8 [B, H, W], without the [B, n, H, W] logits, their log-softmax or a gradient of that
    extent ever being stored.  ``size`` (default: the target's extent) must be the target's extent.  Returns the loss, an fp32 scalar on
    the device; with ``return_counts`` also the int64 [2] device tensor (count, bad): a label n <= t != ignore_index is ignored and
    counted in bad, where torch raises.  No counted pixel: NaN.  Nothing waits for the device.
    With grad mode on and a ``coarse`` that requires grad the loss is differentiable (once) in ``coarse``: its backward is one gather
    launch that takes the upstream gradient as a device scalar and gives the same bits on every run.  In every other case only the
    forward launches run.  ``max_blocks`` caps the grids (0: the default cap); no result depends on it.  ``return_saved`` (forward
    only): returns (loss, counts, lse), what `coarse_cross_entropy_backward` takes."""
    import torch
    if isinstance(coarse, CoarseLogits):
        if size is not None and _hw(size) != coarse.size:
            raise ValueError(f"size {_hw(size)} against CoarseLogits that stand for {coarse.size}")
        coarse, size = coarse.logits, coarse.size
    target = _logits_and_target("coarse_cross_entropy", coarse, target, full=False)
    if coarse.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {coarse.dtype}")
    if coarse.shape[1] > SEG_CE_MAX_CLASSES:
        raise ValueError(f"at most {SEG_CE_MAX_CLASSES} classes, got {coarse.shape[1]}")
    if size is not None and _hw(size) != tuple(target.shape[1:]):
        raise ValueError(f"size {_hw(size)} is not the target's extent {tuple(target.shape[1:])}")
    ignore_index, max_blocks = int(ignore_index), int(max_blocks)
    if max_blocks < 0:
        raise ValueError(f"max_blocks must not be negative, got {max_blocks}")
    if return_saved:
        return _ce_forward(coarse.detach(), target, ignore_index, max_blocks)
    if torch.is_grad_enabled() and coarse.requires_grad:
        loss, counts = _ce_function().apply(coarse, target, ignore_index, max_blocks)
    else:
        loss, counts, _ = _ce_forward(coarse, target, ignore_index, max_blocks)
    return (loss, counts) if return_counts else loss


def assemble_training_segmenter(backbone, classifier, feature: str = "C5", normalize: bool = True):
    """The train-mode twin of `assemble_segmenter`: the "Train segnet" step of the reference (main/seg/train_edtr.py:208-213) from its
    learned parts.  Returns ``train_step(images, masks) -> (loss_ce, features)``: ``images`` a contiguous fp32 [B, 3, h, w] device
    tensor, ``masks`` uint8 [B, h, w]; Normalize (``normalize``), ``backbone`` and ``classifier`` run with grad on, and ``loss_ce`` is
    `coarse_cross_entropy` of the classifier's logits at the network's stride against the masks, differentiable in every learned
    part.  ``features`` is what the backbone returned, so that the caller can form the feature-matching L1 of train_edtr.py:218 with
    `losses.feature_matching(features, teacher_features, keys=("C5",))`.  Without the aux head (the reference has it commented out), class weights or label smoothing (it uses neither)."""
    def train_step(images, masks):
        import torch
        from . import cls
        with torch.enable_grad():
            feats = backbone(cls.normalize(images) if normalize else images)
            logits = classifier(feats[feature] if hasattr(feats, "keys") else feats)
            loss = coarse_cross_entropy(CoarseLogits(logits.contiguous(), tuple(images.shape[-2:])), masks)
        return loss, feats

    return train_step


def evaluate(images, masks, segnet, n_classes: int = 21, return_preds: bool = False, palette=None):
    """The tail of the reference's segmentation test: for every image (fp32 [3, h, w] or [1, 3, h, w] on the device, as
    `evalutil.restore_dataset` returns them) one call of ``segnet`` — any callable from [1, 3, h, w] fp32 to logits [1, n, h, w], or to
    a mapping with key "out" as torchvision's models return — and one `confusion` launch into a shared matrix against the uint8
    [h, w] mask; with ``return_preds`` also the argmax and its colour map.  Where ``segnet`` returns `CoarseLogits` (itself or
    under "out"; `assemble_segmenter` does), the launch is `coarse_confusion` against the mask, whose extent must be the one the
    coarse logits stand for.  One device -> host copy at the end; masks that are not on
    the device yet cost one upload each, so hand device tensors in where the loop must not touch the host.  Returns
    {"mat": int64 [n, n], "iou": fp32 [n], "miou": float (in percent)} (and "preds", "colors": lists of device tensors)."""
    import torch
    images, masks = list(images), list(masks)
    if not images or len(images) != len(masks):
        raise ValueError(f"evaluate needs as many masks as images, got {len(masks)} for {len(images)}")
    mat, preds, colors = None, [], []
    for img, mask in zip(images, masks):
        x = img if img.ndim == 4 else img[None]
        out = segnet(x)
        out = out["out"] if hasattr(out, "keys") else out
        coarse = isinstance(out, CoarseLogits)
        logits = (out.logits if coarse else out).contiguous()
        m = torch.as_tensor(mask)
        if m.ndim != 2:
            raise ValueError(f"a mask is a uint8 [h, w] label map, got {tuple(m.shape)}")
        if coarse and tuple(m.shape) != out.size:
            raise ValueError(f"coarse logits that stand for {out.size[0]} x {out.size[1]} against a {m.shape[0]} x {m.shape[1]} mask")
        if mat is None:
            mat = torch.zeros((int(n_classes), int(n_classes)), dtype=torch.int64, device=logits.device)
        res = (coarse_confusion if coarse else confusion)(logits, m[None], n_classes, mat=mat, return_pred=return_preds)
        if return_preds:
            preds.append(res[1][0])
            colors.append(colorize(res[1][0], palette))
    host = mat.cpu().numpy()
    result = {"mat": host, "iou": compute_iou(host), "miou": mean_iou(host)}
    if return_preds:
        result["preds"], result["colors"] = preds, colors
    return result
