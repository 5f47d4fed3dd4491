"""Classification on the device: what the reference's classification test does after `wavelet_reconstruction`
(main/cls/test_edtr.py:127-162) — the classifier's input normalisation, `calculate_accuracy(pred, label, topk=(1, 5))` and, with
--calc-fd, `F.l1_loss(feat_res, feat_gt, reduction='none').mean(dim=(1, 2, 3))` — and the geometry its data set applies to the ground
truth (datasets/classification.py:65-96: shorter side to gt_size, crop, `augment`'s flips and rot90).  The five launches are
include/edtr_hip.h "Classification" (kernels in csrc/cls.hip).  The task networks stay outside, as in `labels` and `boxes`: `evaluate`
takes any callable, and `assemble_training_classifier` puts the reference's "Train clsnet" step (main/cls/train_edtr.py:207-213)
together from the classifier, its teacher and the loss launches of `losses`.

Three layers, as in `labels` and `coco`:
  * `rank`, `fdist`, `normalize`, `window`, `Scores`: thin wrappers over the launches (torch tensors on the device, the caller's
    stream).  With inputs already on the device nothing waits for the device; a numpy input is uploaded first;
  * `*_reference`: the numpy restatement of each.  They are the NORMATIVE definition: the kernels are tested against them by
    equality, and they against the reference's own functions and plain torch (tests/golden/cls.npz);
  * host-side parameter code: `ClsGeometry` with the reference's YAML keys, `draw_cls_geometry` (a generator stream of its own, so
    that `labels.draw_geometry` and `degrade.draw_params*` return what they returned before), `image_folder`, `summarize`.

THE ORDER RULE.  With key = `boxes.score_keys` (every NaN is one largest key, -0.0 and 0.0 are one key), class j PRECEDES class i iff
key(v_j) > key(v_i), or the keys are equal and j < i.  rank[b] is the number of classes that precede the label's class (C for a label
outside [0, C): `pred.eq(target)` can never hold there), top[b, m] the class with exactly m predecessors, and an image is CORRECT AT k
iff rank < k.  On a row without equal keys this is `torch.topk(maxk, 1, True, True)`, NaN first included.  Where keys are equal torch
itself is unspecified — its CPU topk returns tied values in arbitrary index order (a row of equal values gave [135, 132, 133, 134,
131]), so whether a label tied at the k-th place counts is an accident of the reference; this rule fixes it: the lower index first.
For 2-D targets `target.max(dim=1)[1]` is top[:, 0] of the target rows: torch's CPU max returns the first NaN, else the first maximum,
and so does the rule.

THE FEATURE DISTANCE.  fd[b] = mean |a - b| over the n = C h w elements of image b.  Each difference is formed in fp32 (widen,
subtract, absolute value): for fp32 inputs these are torch's own elements; for fp16 / bf16 inputs this is deliberately MORE accurate
than torch, which rounds the difference to the half type.  The sum is fp64 in an order that depends on n alone: chunks of `FD_CHUNK`
elements; within a chunk, lane l of 256 adds its elements l, l + 256, ... in that order; the tree s = 128, 64, ..., 1 with
sum[l] += sum[l + s] adds the 256 lane sums; the chunk sums are added in chunk order, divided by n in fp64, rounded once to fp32.

THE ACCURACY.  Per batch acc_k = float32(correct_k) * float32(100.0 / n): one fp32 product, the scalar rounded first — what
`correct_k * (100.0 / batch_size)` does to torch's fp32 count.  "acc1" / "acc5" are the reference's figure, the mean over images of
their batch's value (`val_acc1 += [acc] * bs`, then `.mean()`), as an fp64 mean rounded to fp32; "acc1_exact" / "acc5_exact" are
100 * sum(correct) / sum(n)."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import boxes as _boxes
from . import labels as _labels

F32, F64 = np.float32, np.float64
MAX_CLASSES, MAX_KEEP, MAX_TOPK = 65536, 8, 4           # EDTR_CLS_MAX_*
FD_CHUNK, FD_MAX_ELEMS = 4096, 1 << 28                  # EDTR_CLS_FD_*
FD_LANES = 256
CLS_GEOMETRY_WORD = 0x434C5347                          # "CLSG": the purpose word of `draw_cls_geometry`'s generator
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=F32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=F32)
# the reference's inverse pair (model/resnet.py:22-27): Normalize with these undoes Normalize with the two above
IMAGENET_INV_MEAN = np.array([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225], dtype=F32)
IMAGENET_INV_STD = np.array([1 / 0.229, 1 / 0.224, 1 / 0.225], dtype=F32)
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")      # torchvision's
IMAGE_FIELDS = (("label", np.int32), ("rank", np.int32), ("top", np.int32), ("fd", F32), ("batch", np.int32))
BATCH_FIELDS = (("n", np.int32), ("correct", np.int32))


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative)
# ----------------------------------------------------------------------------------------------------------------------------------
def _widen(v) -> np.ndarray:
    """fp32 / fp16 / bf16 values (numpy array or tensor) widened exactly to an fp32 numpy array"""
    if hasattr(v, "detach"):
        v = v.detach().cpu().float().numpy()
    v = np.asarray(v)
    if v.dtype not in (np.float32, np.float16):
        raise TypeError(f"expected float32, float16 or bfloat16 values, got {v.dtype}")
    return np.ascontiguousarray(v.astype(F32))


def _check_topk(topk) -> Tuple[int, ...]:
    topk = tuple(int(k) for k in topk)
    if not 1 <= len(topk) <= MAX_TOPK or any(not 1 <= k <= MAX_KEEP for k in topk):
        raise ValueError(f"topk takes 1 to {MAX_TOPK} entries in [1, {MAX_KEEP}], got {topk}")
    return topk


def _check_rows(B: int, C: int, keep: int) -> None:
    if not 1 <= B <= 65535 or not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"logits are [B, C] with 1 <= B <= 65535 and 1 <= C <= {MAX_CLASSES}, got [{B}, {C}]")
    if not 0 <= int(keep) <= MAX_KEEP:
        raise ValueError(f"keep must lie in [0, {MAX_KEEP}], got {keep}")


def rank_reference(logits, labels=None, keep: int = 5):
    """THE ORDER RULE of this module's docstring for ``logits`` [B, C]: (rank int32 [B], or None without ``labels``; top int32
    [B, keep], -1 from place C on)."""
    v = _widen(logits)
    if v.ndim != 2:
        raise ValueError(f"logits are [B, C], got {v.shape}")
    B, C = v.shape
    _check_rows(B, C, keep)
    keys = _boxes.score_keys(v.reshape(-1)).astype(np.int64).reshape(B, C)
    order = np.argsort(-keys, axis=1, kind="stable")
    top = np.full((B, int(keep)), -1, dtype=np.int32)
    top[:, :min(int(keep), C)] = order[:, :int(keep)]
    if labels is None:
        return None, top
    lab = np.asarray(labels.detach().cpu().numpy() if hasattr(labels, "detach") else labels).astype(np.int64).reshape(-1)
    if lab.shape[0] != B:
        raise ValueError(f"{lab.shape[0]} labels for {B} rows")
    place = np.empty((B, C), dtype=np.int64)
    np.put_along_axis(place, order, np.broadcast_to(np.arange(C), (B, C)), axis=1)
    inside = (lab >= 0) & (lab < C)
    rank = np.where(inside, place[np.arange(B), np.clip(lab, 0, C - 1)], C).astype(np.int32)
    return rank, top


def target_labels_reference(target) -> np.ndarray:
    """int32 [B]: `target.max(dim=1)[1]` of 2-D targets — the first place of the order rule"""
    return rank_reference(target, None, 1)[1][:, 0].copy()


def fdist_reference(a, b) -> np.ndarray:
    """THE FEATURE DISTANCE of this module's docstring: fp32 [B] from ``a``, ``b`` [B, ...] (fp32 / fp16 / bf16), in the launches'
    order — written with explicit loops and reshapes; `np.sum`'s pairwise order is not it."""
    a, b = _widen(a), _widen(b)
    if a.shape != b.shape or a.ndim < 2:
        raise ValueError(f"two feature arrays of one shape [B, ...], got {a.shape} and {b.shape}")
    B = a.shape[0]
    a, b = a.reshape(B, -1), b.reshape(B, -1)
    n = a.shape[1]
    if not 1 <= n <= FD_MAX_ELEMS:
        raise ValueError(f"an image takes 1 to {FD_MAX_ELEMS} feature elements, got {n}")
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(a - b).astype(F32).astype(F64)                   # the difference and its absolute value in fp32
        chunks = (n + FD_CHUNK - 1) // FD_CHUNK
        per_lane = FD_CHUNK // FD_LANES
        # (a padding zero is added to a sum that is >= +0 or NaN, and changes neither)
        padded = np.zeros((B, chunks * FD_CHUNK), dtype=F64)
        padded[:, :n] = d
        grid = padded.reshape(B, chunks, per_lane, FD_LANES)        # element l + 256 i of a chunk is [i, l]
        lanes = np.zeros((B, chunks, FD_LANES), dtype=F64)
        for i in range(per_lane):                                   # lane l adds its elements in order
            lanes = lanes + grid[:, :, i, :]
        step = FD_LANES // 2
        while step:                                                 # the fixed-pairing tree
            lanes = lanes[:, :, :step] + lanes[:, :, step:2 * step]
            step //= 2
        total = np.zeros(B, dtype=F64)
        for c in range(chunks):                                     # the partials in chunk order
            total = total + lanes[:, c, 0]
        return (total / F64(n)).astype(F32)


def _constants(mean, std):
    m, s = np.asarray(mean, dtype=F32).reshape(-1), np.asarray(std, dtype=F32).reshape(-1)
    if m.shape != (3,) or s.shape != (3,) or np.isnan(m).any() or np.isnan(s).any() or (s == 0).any():
        raise ValueError("mean and std take three numbers each, and no std is zero")
    return m, s


def normalize_reference(x, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
    """(x - mean_c) / std_c on fp32 [B, 3, H, W] with fp32 constants, each operation rounded: torchvision's Normalize (`sub_` then
    `div_`)"""
    x = np.asarray(x, dtype=F32)
    if x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"normalize takes fp32 [B, 3, H, W], got {x.shape}")
    m, s = _constants(mean, std)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((x - m[None, :, None, None]).astype(F32) / s[None, :, None, None]).astype(F32)


def window_reference(x, out_hw, origin=(0, 0), hflip: bool = False, vflip: bool = False, rot90: bool = False, fill: int = 0) -> np.ndarray:
    """`labels.window_reference` — the ``out_hw`` = (H, W) crop at ``origin``, ``fill`` outside, both flips — and then, under
    ``rot90``, `augment`'s `img.transpose(1, 0, 2)`: the result is [W, H(, C)] and out (y, x) = flipped crop (x, y)."""
    out = _labels.window_reference(x, out_hw, origin, hflip, vflip, fill)
    if rot90:
        out = out.transpose(1, 0) if out.ndim == 2 else out.transpose(1, 0, 2)
    return np.ascontiguousarray(out)


def prepare_reference(x, size=None, upsample=1, normalize: bool = True) -> np.ndarray:
    """numpy restatement of `prepare`"""
    from . import degrade
    x = np.asarray(x, dtype=F32)
    if size is not None:
        x = degrade.resize_reference(x, size, "bilinear")
    if upsample > 1:
        x = _boxes.bilinear_scale_reference(x, upsample)
    return normalize_reference(x) if normalize else x


def batch_accuracy(correct, n) -> np.ndarray:
    """fp32: float32(correct) * float32(100.0 / n), `correct_k * (100.0 / batch_size)` of utils/classification.py:59-60"""
    correct, n = np.asarray(correct), np.asarray(n)
    scale = (100.0 / n.astype(F64)).astype(F32)
    return (correct.astype(F32) * (scale[:, None] if correct.ndim == 2 else scale)).astype(F32)


def _empty_records(topk, keep: int) -> dict:
    out = {name: np.zeros((0, keep) if name == "top" else 0, dtype=dt) for name, dt in IMAGE_FIELDS}
    out.update(n=np.zeros(0, dtype=np.int32), correct=np.zeros((0, len(topk)), dtype=np.int32), topk=np.array(topk, dtype=np.int32))
    return out


def records_reference(batches, topk=(1, 5), keep: int = 5) -> dict:
    """The records `Scores` holds after one `update` per entry of ``batches`` — (logits, labels), or (logits, labels, feat, feat_gt) —
    by the restatements: the loop the device path is tested against."""
    topk = _check_topk(topk)
    parts = [_empty_records(topk, int(keep))]
    for i, batch in enumerate(batches):
        logits, lab = batch[0], batch[1]
        lab = np.asarray(lab.detach().cpu().numpy() if hasattr(lab, "detach") else lab)
        if lab.ndim == 2:
            lab = target_labels_reference(lab)
        rank, top = rank_reference(logits, lab, keep)
        B = rank.shape[0]
        fd = fdist_reference(batch[2], batch[3]) if len(batch) > 2 and batch[2] is not None else np.full(B, np.nan, dtype=F32)
        parts.append(dict(label=lab.astype(np.int32), rank=rank, top=top, fd=fd, batch=np.full(B, i, dtype=np.int32), n=np.array([B], dtype=np.int32),
                          correct=np.array([[int((rank < k).sum()) for k in topk]], dtype=np.int32)))
    out = {name: np.concatenate([p[name] for p in parts]) for name, _ in IMAGE_FIELDS + BATCH_FIELDS}
    out["topk"] = np.array(topk, dtype=np.int32)
    return out


def merge_records(shards: Sequence[dict]) -> dict:
    """The shards' records concatenated in the order given, the batches renumbered to follow on: `gather_for_metrics` for records"""
    shards = list(shards)
    if not shards:
        raise ValueError("merge_records needs at least one shard")
    topk = np.asarray(shards[0]["topk"])
    out = {name: [] for name, _ in IMAGE_FIELDS + BATCH_FIELDS}
    batches = 0
    for s in shards:
        if not np.array_equal(np.asarray(s["topk"]), topk) or s["top"].shape[1] != shards[0]["top"].shape[1]:
            raise ValueError("the shards were recorded with different topk or keep")
        for name, _ in IMAGE_FIELDS + BATCH_FIELDS:
            out[name].append(np.asarray(s[name]) + (np.int32(batches) if name == "batch" else 0))
        batches += int(np.asarray(s["n"]).shape[0])
    merged = {name: np.concatenate(out[name]).astype(dt) for name, dt in IMAGE_FIELDS + BATCH_FIELDS}
    merged["topk"] = topk.astype(np.int32)
    return merged


def summarize(records: dict) -> dict:
    """THE ACCURACY of this module's docstring from the records of a data set: for every k of the records' topk "acc<k>" (the
    reference's figure) and "acc<k>_exact"; "fd", the fp64 mean of the per-image fp32 values rounded to fp32 (NaN if an image was
    recorded without features); "batch_acc" fp32 [batches, len(topk)]; "images"."""
    n, correct, topk = np.asarray(records["n"]), np.asarray(records["correct"]), [int(k) for k in np.asarray(records["topk"])]
    total = int(n.sum())
    if total == 0:
        raise ValueError("no image was recorded")
    if total != int(np.asarray(records["rank"]).shape[0]):
        raise ValueError(f"the batch rows count {total} images, the image rows {np.asarray(records['rank']).shape[0]}")
    acc = batch_accuracy(correct, n)
    out = {"batch_acc": acc, "images": total}
    for t, k in enumerate(topk):
        out[f"acc{k}"] = float(F32(np.mean(np.repeat(acc[:, t], n).astype(F64))))
        out[f"acc{k}_exact"] = 100.0 * int(correct[:, t].sum()) / total
    with np.errstate(invalid="ignore"):
        out["fd"] = float(F32(np.mean(np.asarray(records["fd"]).astype(F64))))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# geometry of the reference's classification data set
# ----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class ClsGeometry:
    """The geometry keys of DegradedClassificationDataset (configs/cls/*/train/*.yaml, `dataset.train.params`)"""
    gt_size: int = 256
    out_size: int = 224
    crop_type: str = "center"
    hflip: bool = False
    rotation: bool = False

    KEYS = ("gt_size", "out_size", "crop_type", "hflip", "rotation")

    def __post_init__(self):
        if int(self.gt_size) <= 0 or int(self.out_size) <= 0:
            raise ValueError(f"gt_size and out_size must be positive, got {self.gt_size} and {self.out_size}")
        if self.crop_type not in _labels.CROP_TYPES:
            raise ValueError(f"crop_type must be one of {_labels.CROP_TYPES}, got {self.crop_type!r}")

    @classmethod
    def from_dict(cls, d: dict) -> "ClsGeometry":
        """From a mapping that holds the keys at its top level, under dataset.params or under dataset.train.params /
        dataset.val.params as the reference's configs do; other keys (the degradation's) are ignored."""
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
            raise ValueError("no gt_size key: not a geometry of the reference's classification data set")
        return cls(**{k: node[k] for k in cls.KEYS if k in node})


def load_cls_geometry(spec) -> ClsGeometry:
    """A `ClsGeometry`, a mapping with its keys, or the path of a YAML file that holds them"""
    if isinstance(spec, ClsGeometry):
        return spec
    if isinstance(spec, dict):
        return ClsGeometry.from_dict(spec)
    try:
        import yaml
    except ImportError as e:
        raise RuntimeError("reading a YAML geometry needs PyYAML (`import yaml` failed)") from e
    with open(spec) as fh:
        return ClsGeometry.from_dict(yaml.safe_load(fh))


@dataclass
class ClsGeometryParams:
    """What `draw_cls_geometry` fixed for one image: resize to ``size``, cut ``out_hw`` at ``origin``, flip, transpose"""
    size: Tuple[int, int]               # (h, w) after the resize
    origin: Tuple[int, int]             # (y0, x0) of the crop in the resized image
    out_hw: Tuple[int, int]             # the crop's extent (before the transpose)
    hflip: bool
    vflip: bool
    rot90: bool


def cls_resized_extent(gt_size: int, h: int, w: int) -> Tuple[int, int]:
    """(w', h') of datasets/classification.py:76-80 in Python's double arithmetic: the shorter side to gt_size, the longer one to
    int(gt_size * long / short) — the pair `Image.resize` takes"""
    gt_size, h, w = int(gt_size), int(h), int(w)
    if gt_size <= 0 or h <= 0 or w <= 0:
        raise ValueError(f"extents must be positive, got gt_size {gt_size} for a {h} x {w} image")
    return (int(gt_size * w / h), gt_size) if w >= h else (gt_size, int(gt_size * h / w))


def draw_cls_geometry(cfg: ClsGeometry, seed: int, image_id: int, hw: Tuple[int, int]) -> ClsGeometryParams:
    """One image's geometry from ``numpy.random.default_rng([seed, image_id, CLS_GEOMETRY_WORD])``: a function of the configuration,
    the seed, the image's data-set index and its extent.  Five uniform draws, made whether or not they are used: the crop's row, its
    column, hflip, vflip, rot90 (`augment` draws the three flags in that order; the two rotation flags only under ``rotation``)."""
    seed, image_id = int(seed), int(image_id)
    if not 0 <= seed < 1 << 64 or not 0 <= image_id < 1 << 32:
        raise ValueError(f"seed must be in [0, 2^64) and image_id in [0, 2^32), got {seed} and {image_id}")
    gen = np.random.default_rng([seed, image_id, CLS_GEOMETRY_WORD])
    u_y, u_x, u_h, u_v, u_r = (float(gen.uniform()) for _ in range(5))
    rw, rh = cls_resized_extent(cfg.gt_size, hw[0], hw[1])
    out = int(cfg.out_size)
    if cfg.crop_type == "none" or (rh == out and rw == out):
        if rh != out or rw != out:
            raise ValueError(f"crop_type 'none' needs a {out} x {out} image after the resize, got {rh} x {rw}")
        origin = (0, 0)
    else:
        if rh < out or rw < out:
            raise ValueError(f"a {rh} x {rw} image is smaller than the {out} x {out} crop")
        if cfg.crop_type == "center":
            origin = ((rh - out) // 2, (rw - out) // 2)
        else:
            origin = (min(int(u_y * (rh - out + 1)), rh - out), min(int(u_x * (rw - out + 1)), rw - out))
    rotation = bool(cfg.rotation)
    return ClsGeometryParams((rh, rw), origin, (out, out), bool(cfg.hflip and u_h < 0.5), rotation and u_v < 0.5, rotation and u_r < 0.5)


def prepare_image_reference(image_u8, geom: ClsGeometryParams) -> np.ndarray:
    """numpy restatement of `prepare_image`"""
    from .imageio import resize_u8_reference
    rh, rw = geom.size
    return window_reference(resize_u8_reference(np.asarray(image_u8), rw, rh), geom.out_hw, geom.origin, geom.hflip, geom.vflip, geom.rot90, 0)


def image_folder(root: str):
    """torchvision `ImageFolder`'s listing of ``root``: (samples, classes) with classes = the sorted names of root's directories,
    samples = [(path, class index)] over the classes in that order, each walked with sorted directories and sorted file names
    (links followed), a file counting iff its lower-cased name ends in one of `IMG_EXTENSIONS`.  FileNotFoundError without class
    directories or for a class without a file, as torchvision raises."""
    root = os.path.expanduser(str(root))
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"couldn't find any class folder in {root}")
    samples, empty = [], []
    for index, name in enumerate(classes):
        before = len(samples)
        for folder, _, files in sorted(os.walk(os.path.join(root, name), followlinks=True)):
            samples.extend((os.path.join(folder, f), index) for f in sorted(files) if f.lower().endswith(IMG_EXTENSIONS))
        if len(samples) == before:
            empty.append(name)
    if empty:
        raise FileNotFoundError(f"found no valid file for the classes {', '.join(empty)}; supported extensions are {', '.join(IMG_EXTENSIONS)}")
    return samples, classes


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _float_on(x, device, what: str, ndim_min: int = 2):
    """``x`` (numpy fp32 / fp16 array or torch tensor) as a contiguous fp32 / fp16 / bf16 device tensor"""
    import torch
    from .imageio import _device
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float16, torch.bfloat16) or t.ndim < ndim_min:
        raise TypeError(f"{what} must be a float32, float16 or bfloat16 array or tensor of at least {ndim_min} axes")
    dev = t.device if t.is_cuda and device is None else _device(device)
    return t.to(dev).contiguous()


def _labels_i32(labels, B: int, device):
    """1-D integer labels narrowed to int32 on the device (a device tensor is narrowed there: no host wait)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else torch.as_tensor(labels)
    if t.ndim != 1 or t.shape[0] != B or t.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
        raise TypeError(f"labels are one integer per row, got {t.dtype} {tuple(t.shape)} for {B} rows")
    return t.to(device).to(torch.int32).contiguous()


def target_labels(target, device=None):
    """`target.max(dim=1)[1]` of 2-D targets as int32 [B] on the device: one `rank` launch with keep = 1 and no labels"""
    import torch
    from . import ops
    t = _float_on(target, device, "targets")
    if t.ndim != 2:
        raise ValueError(f"targets are [B, C], got {tuple(t.shape)}")
    _check_rows(t.shape[0], t.shape[1], 1)
    top = torch.empty((t.shape[0], 1), dtype=torch.int32, device=t.device)
    ops.launch(ops.make_cls_rank(logits=t, labels=None, keep=1, rec_label=None, rec_rank=None, rec_top=top, offset=None, capacity=t.shape[0]))
    return top.view(-1)


def rank(logits, labels=None, keep: int = 5, device=None):
    """`rank_reference` on the device, one launch (two for 2-D targets): (rank int32 [B] or None, top int32 [B, keep])"""
    import torch
    from . import ops
    x = _float_on(logits, device, "logits")
    if x.ndim != 2:
        raise ValueError(f"logits are [B, C], got {tuple(x.shape)}")
    B, C = x.shape
    _check_rows(B, C, keep)
    lab = out_rank = None
    if labels is not None:
        lab = target_labels(labels, x.device) if getattr(labels, "ndim", 1) == 2 else _labels_i32(labels, B, x.device)
        out_rank = torch.empty(B, dtype=torch.int32, device=x.device)
    top = torch.empty((B, int(keep)), dtype=torch.int32, device=x.device)
    if lab is not None or keep > 0:
        ops.launch(ops.make_cls_rank(logits=x, labels=lab, keep=int(keep), rec_label=None, rec_rank=out_rank, rec_top=top, offset=None, capacity=B))
    return out_rank, top


def _fd_partials(a, b):
    import torch
    from . import ops
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError(f"the two feature tensors must agree in shape and type, got {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
    B = a.shape[0]
    n = a.numel() // max(B, 1)
    if not 1 <= B <= 65535 or not 1 <= n <= FD_MAX_ELEMS:
        raise ValueError(f"features are [B, ...] with 1 <= B <= 65535 and 1 to {FD_MAX_ELEMS} elements per image, got {tuple(a.shape)}")
    partials = torch.empty(B * ((n + FD_CHUNK - 1) // FD_CHUNK), dtype=torch.float64, device=a.device)
    ops.launch(ops.make_cls_fdist(a=a, b=b, partials=partials))
    return partials, n


def fdist(a, b, device=None):
    """`fdist_reference` on the device: fp32 [B].  Two launches (the chunk sums, the finalisation); nothing is read back."""
    import torch
    from . import ops
    a = _float_on(a, device, "features")
    b = _float_on(b, a.device, "features")
    partials, n = _fd_partials(a, b)
    B = a.shape[0]
    fd = torch.empty(B, dtype=torch.float32, device=a.device)
    scratch = torch.zeros(B + 3, dtype=torch.int32, device=a.device)        # batch [B], batch_n [1], the two offsets
    ops.launch(ops.make_cls_commit(rec_rank=None, rec_fd=fd, rec_batch=scratch[:B], B=B, partials=partials, n=n, topk=(), batch_n=scratch[B:B + 1],
                                   batch_correct=None, offsets=scratch[B + 1:], capacity=B, batch_capacity=1))
    return fd


def normalize(x, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=None):
    """`normalize_reference` on the device, one launch: ``x`` a contiguous fp32 [B, 3, H, W] device tensor; ``out`` may be ``x``"""
    import torch
    from . import degrade, ops
    degrade._check_device_batch(x, "normalize")
    m, s = _constants(mean, std)
    if out is None:
        out = torch.empty_like(x)
    elif not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise TypeError("out must be a contiguous tensor of x's shape, type and device")
    ops.launch(ops.make_cls_normalize(x=x, out=out, mean=m.tolist(), std=s.tolist()))
    return out


_normalize = normalize          # (`prepare` has a flag of that name)


def prepare(x, size=None, upsample=1, normalize: bool = True):
    """The head of the reference classifier's `forward` (model/resnet.py:285-294) on a contiguous fp32 [B, 3, H, W] device tensor:
    `F.interpolate(size=, mode='bilinear')` by `degrade.resize` (``size`` None: skipped; the reference's ImageNet models take (224,
    224)), `F.interpolate(scale_factor=upsample, mode='bilinear')` by `boxes.bilinear_scale` (1: skipped), then Normalize with the
    ImageNet constants by this module's launch (in place on an intermediate).  ``x`` itself is never written."""
    from . import degrade
    degrade._check_device_batch(x, "prepare")
    y = x
    if size is not None:
        y = degrade.resize(y, size, "bilinear")
    if upsample > 1:
        y = _boxes.bilinear_scale(y, upsample)
    if normalize:
        y = _normalize(y, out=None if y is x else y)
    return y


def window(x, out_hw, origin=(0, 0), hflip: bool = False, vflip: bool = False, rot90: bool = False, fill: int = 0, device=None):
    """`window_reference` on the device, one launch"""
    import torch
    from . import ops
    src, flat = _labels._on_device(x, device, "window")
    H, W = _labels._hw(out_hw)
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"fill must be a byte, got {fill}")
    dst = torch.empty(((W, H) if rot90 else (H, W)) + (src.shape[2],), dtype=torch.uint8, device=src.device)
    ops.launch(ops.make_cls_window(src=src, dst=dst, out_hw=(H, W), y0=int(origin[0]), x0=int(origin[1]), hflip=hflip, vflip=vflip,
                                   transpose=rot90, fill=int(fill)))
    return dst[:, :, 0] if flat else dst


def prepare_image(image_u8, geom: ClsGeometryParams, device=None):
    """`load_gt_image` of DegradedClassificationDataset for one decoded image under the geometry `draw_cls_geometry` fixed: the
    BICUBIC `imageio.resize_u8`, then one `window` launch.  Returns uint8 [H, W, 3] on the device."""
    from . import imageio
    rh, rw = geom.size
    return window(imageio.resize_u8(image_u8, rw, rh, device=device), geom.out_hw, geom.origin, geom.hflip, geom.vflip, geom.rot90, 0)


class Scores:
    """The running record of a data set's classification scores on the device: `update` appends one batch (two launches, three with
    features, one more for 2-D targets; no host sync: both offsets stay on the device), `to_host` makes the single copy and returns
    the records `summarize` takes.  ``capacity`` image rows and ``batch_capacity`` batch rows (default: as many).  Per image: `label`,
    `rank`, `top` [keep] (int32), `fd` (fp32, NaN without features), `batch` (the row of its batch); per batch: `n` and `correct`
    [len(topk)].  Every field lives in ONE device buffer, each with a guard row behind it that no launch may write; rows that do not
    fit are dropped on the device, the offsets move on all the same, and `to_host` then raises."""
    GUARD = 0x5A

    def __init__(self, capacity: int, topk=(1, 5), keep: int = 5, device=None, batch_capacity: Optional[int] = None):
        import torch
        from .imageio import _device
        self.capacity, self.batch_capacity = int(capacity), int(capacity if batch_capacity is None else batch_capacity)
        if self.capacity <= 0 or self.batch_capacity <= 0 or max(self.capacity, self.batch_capacity) > 1 << 27:
            raise ValueError(f"capacities must lie in [1, 2^27], got {capacity} and {batch_capacity}")
        self.topk, self.keep = _check_topk(topk), int(keep)
        if not 1 <= self.keep <= MAX_KEEP:
            raise ValueError(f"keep must lie in [1, {MAX_KEEP}], got {keep}")
        self.device = _device(device)
        self._layout, at = {}, 8                                # bytes 0 .. 7: the two offsets
        for name, dtype in IMAGE_FIELDS + BATCH_FIELDS:
            rows = (self.capacity if (name, dtype) in IMAGE_FIELDS else self.batch_capacity) + 1
            width = {"top": self.keep, "correct": len(self.topk)}.get(name, 1)
            self._layout[name] = (at, rows, width, np.dtype(dtype))
            at += rows * width * 4
        host = np.full(at, self.GUARD, dtype=np.uint8)
        host[:8] = 0
        self.buffer = torch.from_numpy(host).to(self.device)
        self.fields = {name: self.buffer[at:at + rows * width * 4].view(torch.float32 if dt == F32 else torch.int32)
                       for name, (at, rows, width, dt) in self._layout.items()}
        self.offsets = self.buffer[:8].view(torch.int32)

    def update(self, logits, labels, feat=None, feat_gt=None) -> None:
        """Append one batch: ``logits`` [B, C] (fp32 / fp16 / bf16), ``labels`` integers [B] (int64 is narrowed) or 2-D targets
        [B, C'], and optionally the two feature tensors [B, ...] of one shape and type.  Host arrays cost one upload each; nothing is
        read back."""
        from . import ops
        dev = self.device
        x = _float_on(logits, dev, "logits")
        if x.ndim != 2:
            raise ValueError(f"logits are [B, C], got {tuple(x.shape)}")
        B, C = x.shape
        _check_rows(B, C, self.keep)
        lab = target_labels(labels, dev) if getattr(labels, "ndim", 1) == 2 else _labels_i32(labels, B, dev)
        if lab.shape[0] != B:
            raise ValueError(f"{lab.shape[0]} targets for {B} rows")
        if (feat is None) != (feat_gt is None):
            raise ValueError("the feature distance takes both feature tensors or neither")
        partials, n = None, 0
        f = self.fields
        ops.launch(ops.make_cls_rank(logits=x, labels=lab, keep=self.keep, rec_label=f["label"], rec_rank=f["rank"], rec_top=f["top"],
                                     offset=self.offsets[0:1], capacity=self.capacity))
        if feat is not None:
            a = _float_on(feat, dev, "features")
            b = _float_on(feat_gt, dev, "features")
            if a.shape[0] != B:
                raise ValueError(f"features of {a.shape[0]} images for {B} rows")
            partials, n = _fd_partials(a, b)
        ops.launch(ops.make_cls_commit(rec_rank=f["rank"], rec_fd=f["fd"], rec_batch=f["batch"], B=B, partials=partials, n=n, topk=self.topk,
                                       batch_n=f["n"], batch_correct=f["correct"], offsets=self.offsets, capacity=self.capacity,
                                       batch_capacity=self.batch_capacity))

    def to_host(self) -> dict:
        """The single device -> host copy: the records as a dict of numpy arrays (`IMAGE_FIELDS`, `BATCH_FIELDS`, "topk").  Raises
        RuntimeError if more rows were appended than the capacity holds, or if a guard row was written."""
        raw = self.buffer.cpu().numpy()
        images, batches = (int(v) for v in raw[:8].view(np.int32))
        out = {}
        for name, (at, rows, width, dt) in self._layout.items():
            col = raw[at:at + rows * width * 4]
            if not np.all(col[(rows - 1) * width * 4:] == self.GUARD):
                raise RuntimeError(f"the guard row behind '{name}' was written")
            count = images if name in dict(IMAGE_FIELDS) else batches
            col = col.view(dt)[:min(max(count, 0), rows - 1) * width].copy()
            out[name] = col.reshape(-1, width) if name in ("top", "correct") else col
        if not 0 <= images <= self.capacity or not 0 <= batches <= self.batch_capacity:
            raise RuntimeError(f"{images} images in {batches} batches were appended to records of {self.capacity} image rows and "
                               f"{self.batch_capacity} batch rows: pass a larger capacity")
        out["topk"] = np.array(self.topk, dtype=np.int32)
        return out


def evaluate(images, labels, clsnet, teacher=None, gts=None, batch_size: int = 8, topk=(1, 5)) -> dict:
    """The tail of the reference's classification test (main/cls/test_edtr.py:127-162): the restored ``images`` (fp32 [N, 3, h, w] on
    the device, or a sequence of [3, h, w] / [1, 3, h, w] tensors of one extent, as `evalutil.restore_dataset` returns them) go
    through ``clsnet`` — any callable from [b, 3, h, w] fp32 to logits [b, C]; the reference's normalisation is `prepare` — in batches
    of ``batch_size``, one `Scores.update` each against ``labels`` (N integers; uploaded once).  With ``teacher`` — a callable to a
    feature tensor — it is called on the restored batch and on the same rows of ``gts``, for the feature distance.  No host sync in
    the loop and ONE device -> host copy at the end.
    Returns `summarize`'s keys ("fd" is the data set's mean, the reference's val/fd) plus, per image, "pred" (top-1), "rank" and
    "fd_image", and "records"."""
    import torch
    topk = _check_topk(topk)
    if int(batch_size) <= 0:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    if (teacher is None) != (gts is None):
        raise ValueError("the feature distance takes a teacher and the ground-truth images, or neither")

    def stacked(v):
        return v if isinstance(v, torch.Tensor) and v.ndim == 4 else torch.stack([t[0] if t.ndim == 4 else t for t in v])

    def rows(v, lo, hi):
        return v[lo:hi].contiguous() if isinstance(v, torch.Tensor) and v.ndim == 4 else stacked(list(v)[lo:hi]).contiguous()

    N = len(images)
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
    if N == 0 or lab.shape[0] != N or (gts is not None and len(gts) != N):
        raise ValueError(f"evaluate needs one label (and one ground truth) per image, got {lab.shape[0]} for {N}")
    scores = None
    for lo in range(0, N, int(batch_size)):
        hi = min(lo + int(batch_size), N)
        x = rows(images, lo, hi)
        logits = clsnet(x).contiguous()
        if scores is None:
            scores = Scores(N, topk, max(topk), logits.device, batch_capacity=(N + int(batch_size) - 1) // int(batch_size))
            lab = lab.to(logits.device)
        feats = (teacher(x).contiguous(), teacher(rows(gts, lo, hi)).contiguous()) if teacher is not None else (None, None)
        scores.update(logits, lab[lo:hi], *feats)
    records = scores.to_host()
    return {**summarize(records), "pred": records["top"][:, 0].copy(), "rank": records["rank"], "fd_image": records["fd"], "records": records}


def assemble_training_classifier(clsnet, teacher=None, weight_ce: float = 1.0, weight_fm: float = 1.0):
    """The "Train clsnet" step of the reference (main/cls/train_edtr.py:207-213) from its learned parts, the train-mode twin of
    `evaluate`'s use of ``clsnet``.  Returns ``train_step(images, labels, gts=None) -> (losses, (pred, feat_student))``: ``images`` an
    fp32 [B, 3, h, w] device tensor (the restored half and the clean half already concatenated, normalised as the classifier expects:
    `prepare`), ``labels`` B integers.  ``clsnet(images, return_feat=True)`` runs with grad on and returns (logits [B, C], features);
    ``losses["ce"]`` is ``weight_ce`` * `losses.cross_entropy` of the logits, differentiable in every learned part.  With ``teacher``,
    ``teacher(gts, return_feat=True)`` runs under no_grad (``gts`` defaults to ``images``) and ``losses["fm"]`` is `losses.l1_mean` of
    (student features, teacher features) with weight ``weight_fm``; without a teacher there is no "fm".  Both are fp32 device
    scalars: ``sum(losses.values()).backward()`` is the reference's `accelerator.backward(loss_ce + loss_fm)`.  No label smoothing
    (the reference passes 0.0)."""
    def train_step(images, labels, gts=None):
        import torch
        from . import losses
        with torch.enable_grad():
            pred, feat_student = clsnet(images, return_feat=True)
            out = {"ce": losses.cross_entropy(pred, labels) * float(weight_ce)}
            if teacher is not None:
                with torch.no_grad():
                    _, feat_teacher = teacher(images if gts is None else gts, return_feat=True)
                out["fm"] = losses.l1_mean([(feat_student, feat_teacher)], [float(weight_fm)])
        return out, (pred, feat_student)

    return train_step
