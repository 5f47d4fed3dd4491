"""The detector's input transform on the device: `GeneralizedRCNNTransform.forward` in eval mode (model/faster_rcnn.py:2266-2435), the
first non-learned step of the reference's Faster R-CNN and the one `rois.assemble_detector` still left to the caller.  For every image
the reference runs `(x - mean) / std`, `F.interpolate(scale_factor=, mode="bilinear", recompute_scale_factor=True)`, and then copies
the results into one zero batch whose extent is rounded up to `size_divisible`: four launches and two full-size intermediates per
image.  `transform` does all of it, for the whole ragged list, in ONE launch (include/edtr_hip.h "Detector input", the kernel in
csrc/det_transform.hip) and with no device -> host copy: every extent comes from shapes.

THE EXTENT RULE.  The reference takes `min(im_shape)` of a `torch.tensor`, so `self_min_size / min_size` is `Tensor.__rtruediv__`: the
fp32 reciprocal times the scalar, not a division; `interpolate` then truncates the fp32 product `size * scale`.  With F = float32:

    a = F(F(1) / F(min(h, w))) * F(min_size)
    b = F(F(1) / F(max(h, w))) * F(max_size)
    s = b if b < a else a
    oh, ow = int(F(h) * s), int(F(w) * s)               # each an fp32 product, truncated

`resized_extent` is that rule, and tests/golden/det_transform.npz holds what the reference's own `_resize_image_and_masks` gave for
2000 seeded shapes.  The obvious `floor(h * min(min_size / min(h, w), max_size / max(h, w)))` in Python floats differs on about one
shape in eight: a 375 x 500 image at 800 / 1333 becomes 799 x 1066, not 800 x 1066, and one row moves every anchor, every
`image_sizes` clip and every box ratio of `postprocess`.  ``fixed_size`` = (fw, fh) gives (fh, fw) for every image.  The batch extent
is `int(math.ceil(float(m) / size_divisible) * size_divisible)` of the per-axis maxima (`batch_extent`).

THE VALUES.  `recompute_scale_factor=True` makes `interpolate` work from the output extent alone, so the resize is
`F.interpolate(size=(oh, ow))`: `degrade.bilinear_planes_reference`, with the source coordinate F(h) / F(oh) * (y + 0.5) - 0.5 clamped
at 0 and every step rounded.  `transform_reference` composes `cls.normalize_reference` (an fp32 subtraction, then an IEEE division),
that resize, and the copy into a +0.0 batch; a 16-bit batch holds the fp32 result rounded once to nearest even.  It is the NORMATIVE
definition: the launch is tested against it bit for bit, and it against the reference's own `forward` within four times the
reference's own distance from an fp64 evaluation (CPU ATen's bilinear kernel is not bit-reproducible from its written rule; an image
whose scale is exactly 1 is).

Three layers, as in `rois`, `boxes` and `cls`: `transform` (`transform_record` builds its launch), `DetectorTransform`,
`assemble_features` over the launch;
`transform_reference` in numpy; `resized_extent` and `batch_extent` on the host.  Eval mode only: no `torch_choice` over several
`min_size`, no `_skip_resize`, no masks, no keypoints."""
from __future__ import annotations

import math
from collections import OrderedDict, namedtuple
from typing import Optional, Tuple

import numpy as np

from . import boxes as _boxes
from . import cls as _cls
from .cls import IMAGENET_MEAN, IMAGENET_STD

F32 = np.float32
MAX_CHANNELS = 4                        # EDTR_DET_MAX_CHANNELS
MAX_EXTENT = 32768                      # EDTR_DET_MAX_EXTENT
TILE_W, TILE_H = 256, 16                # EDTR_DET_TILE_W / _H: the tile of a slot one workgroup writes
DTYPES = ("float32", "float16", "bfloat16")

ImageBatch = namedtuple("ImageBatch", ("tensors", "image_sizes"))       # the reference's ImageList


# ----------------------------------------------------------------------------------------------------------------------------------
# host side
# ----------------------------------------------------------------------------------------------------------------------------------
def _last(min_size) -> int:
    return int(min_size[-1]) if isinstance(min_size, (list, tuple)) else int(min_size)


def resized_extent(h: int, w: int, min_size=800, max_size: int = 1333, fixed_size: Optional[Tuple[int, int]] = None) -> Tuple[int, int]:
    """(oh, ow) of an h x w image under the module's extent rule; a tuple ``min_size`` counts by its last entry (the eval branch)"""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"an image has positive extents, got {h} x {w}")
    if fixed_size is not None:
        oh, ow = int(fixed_size[1]), int(fixed_size[0])
    else:
        a = F32(F32(1) / F32(min(h, w))) * F32(_last(min_size))
        b = F32(F32(1) / F32(max(h, w))) * F32(int(max_size))
        s = b if b < a else a
        oh, ow = int(F32(h) * s), int(F32(w) * s)
    if oh < 1 or ow < 1:
        raise ValueError(f"nothing is left of a {h} x {w} image at min_size {min_size}, max_size {max_size}, fixed_size {fixed_size}")
    return oh, ow


def batch_extent(extents, size_divisible: int = 32) -> Tuple[int, int]:
    """(H, W) of the padded batch that holds images of ``extents`` = [(oh, ow)]: each maximum rounded up to ``size_divisible``"""
    extents = [(int(e[0]), int(e[1])) for e in extents]
    if not extents or int(size_divisible) < 1:
        raise ValueError("at least one extent and a positive size_divisible")
    stride = float(size_divisible)
    return tuple(int(math.ceil(float(max(e[axis] for e in extents)) / stride) * stride) for axis in (0, 1))


def _constants(image_mean, image_std, C: int):
    m, s = np.asarray(image_mean, dtype=F32).reshape(-1), np.asarray(image_std, dtype=F32).reshape(-1)
    if m.shape != s.shape or not 1 <= m.shape[0] <= MAX_CHANNELS or np.isnan(m).any() or np.isnan(s).any() or (s == 0).any():
        raise ValueError(f"image_mean and image_std take 1 to {MAX_CHANNELS} numbers each, as many as each other, and no std is zero")
    if C != m.shape[0]:
        raise ValueError(f"an image of {C} channels for {m.shape[0]} means")
    return m, s


def _is_floating(v) -> bool:
    return v.is_floating_point() if hasattr(v, "is_floating_point") else np.issubdtype(np.asarray(v).dtype, np.floating)


def _image_list(images) -> list:
    """a list of [C, h, w] images from a list, or from one [N, C, h, w] array or tensor; the reference's two complaints"""
    if hasattr(images, "ndim") and images.ndim == 4:
        images = [images[i] for i in range(images.shape[0])]
    images = list(images)
    if not 1 <= len(images) <= 65535:
        raise ValueError(f"between 1 and 65535 images, got {len(images)}")
    for img in images:
        if not _is_floating(img):
            raise TypeError(f"Expected input images to be of floating type (in range [0, 1]), but found type {img.dtype} instead")
        if img.ndim != 3:
            raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {tuple(img.shape)}")
        if any(n > MAX_EXTENT for n in img.shape[1:]) or any(n < 1 for n in img.shape):
            raise ValueError(f"an image is [C, h, w] with extents between 1 and {MAX_EXTENT}, got {tuple(img.shape)}")
    return images


def _plan(shapes, min_size, max_size, size_divisible, fixed_size):
    """(resized extents, (H, W)) for images of ``shapes`` = [(h, w)]"""
    extents = [resized_extent(h, w, min_size, max_size, fixed_size) for h, w in shapes]
    H, W = batch_extent(extents, size_divisible)
    if H > MAX_EXTENT or W > MAX_EXTENT:
        raise ValueError(f"the batch would be {H} x {W}; extents end at {MAX_EXTENT}")
    return extents, (H, W)


def _normalize_planes(x: np.ndarray, m: np.ndarray, s: np.ndarray) -> np.ndarray:
    """`cls.normalize_reference` on [C, h, w] for any C: it takes three planes, so another count goes through it a plane at a time"""
    if x.shape[0] == 3:
        return _cls.normalize_reference(x[None], m, s)[0]
    return np.concatenate([_cls.normalize_reference(np.repeat(x[None, c:c + 1], 3, axis=1), [m[c]] * 3, [s[c]] * 3)[0, :1]
                           for c in range(x.shape[0])])


def transform_reference(images, min_size=800, max_size: int = 1333, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD,
                        size_divisible: int = 32, fixed_size=None, dtype: str = "float32"):
    """The normative numpy form of `transform`: (batch fp32 [N, C, H, W], image_sizes [(oh, ow)], original_sizes [(h, w)]).  For
    ``dtype`` "float16" / "bfloat16" the batch holds, in fp32, the values rounded once to that type."""
    from . import degrade, labels
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {DTYPES}, got {dtype!r}")
    imgs = [np.ascontiguousarray(_host_image(v)) for v in _image_list(images)]
    m, s = _constants(image_mean, image_std, imgs[0].shape[0])
    if any(v.shape[0] != imgs[0].shape[0] for v in imgs):
        raise ValueError("the images of a batch have one number of channels")
    original = [tuple(int(n) for n in v.shape[1:]) for v in imgs]
    extents, (H, W) = _plan(original, min_size, max_size, size_divisible, fixed_size)
    batch = np.zeros((len(imgs), imgs[0].shape[0], H, W), dtype=F32)
    for i, (v, (oh, ow)) in enumerate(zip(imgs, extents)):
        batch[i, :, :oh, :ow] = labels._round_to(degrade.bilinear_planes_reference(_normalize_planes(v, m, s)[None], oh, ow)[0], dtype)
    return batch, extents, original


def _host_image(v) -> np.ndarray:
    """an fp32 image on the host (a tensor of any device; other float types are refused as `transform` refuses them)"""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    v = np.asarray(v)
    if v.dtype != F32:
        raise TypeError(f"images are float32, got {v.dtype}")
    return v


def _resize_targets(targets, original, extents, device=None):
    """the reference's copy of ``targets`` with every "boxes" through `boxes.resize_boxes`; what is not provided is refused by name"""
    if targets is None:
        return None
    if len(targets) != len(original):
        raise ValueError(f"{len(targets)} targets for {len(original)} images")
    out = []
    for t, o, e in zip(targets, original, extents):
        t = dict(t)
        for missing in ("masks", "keypoints"):
            if missing in t:
                raise ValueError(f"target {missing!r} are not provided: DetectorTransform resizes \"boxes\" only")
        if "boxes" in t:
            t["boxes"] = _boxes.resize_boxes(t["boxes"], o, e, device=device)
        out.append(t)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def transform_record(images, min_size=800, max_size: int = 1333, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD, size_divisible: int = 32,
                     fixed_size=None, dtype: str = "float32", out=None, device=None):
    """Everything of `transform` but the launch: (the `ops.Rec` that `ops.launch` replays, batch, image_sizes, original_sizes).  The
    record keeps the sources and the descriptors alive (tools/bench_det_transform.py times the kernel alone with it)."""
    import torch
    from . import lib as L, ops
    from .imageio import _device
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {DTYPES}, got {dtype!r}")
    imgs = [torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v for v in _image_list(images)]
    if any(not isinstance(t, torch.Tensor) or t.dtype != torch.float32 for t in imgs):
        raise TypeError(f"images are float32 arrays or tensors, got {[getattr(t, 'dtype', type(t)) for t in imgs]}")
    C = int(imgs[0].shape[0])
    m, s = _constants(image_mean, image_std, C)
    if any(int(t.shape[0]) != C for t in imgs):
        raise ValueError("the images of a batch have one number of channels")
    original = [(int(t.shape[1]), int(t.shape[2])) for t in imgs]
    extents, (H, W) = _plan(original, min_size, max_size, size_divisible, fixed_size)
    dev = next((t.device for t in imgs if t.is_cuda), None) if device is None else None
    dev = dev if dev is not None else _device(device)
    srcs = [t.detach().to(dev).contiguous() for t in imgs]
    shape, tdtype = (len(srcs), C, H, W), getattr(torch, dtype)
    if out is None:
        out = torch.empty(shape, dtype=tdtype, device=srcs[0].device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != tdtype or out.device != srcs[0].device or not out.is_contiguous():
        raise TypeError(f"out must be a contiguous {dtype} tensor of shape {shape} on {srcs[0].device}")
    descs = (L.DetImage * len(srcs))()
    for d, t, (h, w), (oh, ow) in zip(descs, srcs, original, extents):
        d.src, d.h, d.w, d.oh, d.ow = t.data_ptr(), h, w, oh, ow
    ddescs = torch.frombuffer(descs, dtype=torch.uint8).pin_memory().to(srcs[0].device, non_blocking=True)
    rec = ops.make_det_transform(descs_host=descs, descs=ddescs, mean=m.tolist(), std=s.tolist(), batch=out, keep=srcs)
    return rec, out, extents, original


def transform(images, min_size=800, max_size: int = 1333, image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD, size_divisible: int = 32,
              fixed_size=None, dtype: str = "float32", out=None, device=None):
    """`transform_reference` on the device, one launch (edtr_hip.h `edtr_det_transform`): ``images`` a list of fp32 [C, h, w] tensors or
    arrays, or one [N, C, h, w]; host images are uploaded and a non-contiguous view is copied.  Returns (batch [N, C, H, W] of
    ``dtype`` on the device, image_sizes, original_sizes).  ``out``: a contiguous device tensor of that shape and type to write into
    (every element is written, whatever it held).  Nothing is read back and nothing waits for the device: the extents come from
    shapes, and the 24-byte descriptors travel from pinned memory on the caller's stream."""
    from . import ops
    rec, out, extents, original = transform_record(images, min_size, max_size, image_mean, image_std, size_divisible, fixed_size, dtype, out, device)
    ops.launch(rec)
    return out, extents, original


class DetectorTransform:
    """`GeneralizedRCNNTransform` with the reference's constructor arguments, in eval mode: `__call__(images, targets=None)` ->
    (ImageBatch(tensors, image_sizes), targets) with every target's "boxes" through `boxes.resize_boxes` ("masks" and "keypoints" raise
    ValueError), and `postprocess(result, image_sizes, original_sizes)`, `boxes.resize_boxes` back on every "boxes".  `batch(images)`
    is `transform` under the constructor's arguments, original sizes included."""

    def __init__(self, min_size, max_size: int, image_mean, image_std, size_divisible: int = 32, fixed_size: Optional[Tuple[int, int]] = None):
        self.min_size = tuple(min_size) if isinstance(min_size, (list, tuple)) else (min_size,)
        self.max_size, self.size_divisible, self.fixed_size = max_size, size_divisible, fixed_size
        self.image_mean, self.image_std = list(image_mean), list(image_std)
        _constants(self.image_mean, self.image_std, len(self.image_mean))

    def batch(self, images, dtype: str = "float32", out=None, device=None):
        return transform(images, self.min_size, self.max_size, self.image_mean, self.image_std, self.size_divisible, self.fixed_size,
                         dtype=dtype, out=out, device=device)

    def __call__(self, images, targets=None):
        tensors, image_sizes, original = self.batch(images)
        return ImageBatch(tensors, image_sizes), _resize_targets(targets, original, image_sizes, device=tensors.device)

    def postprocess(self, result, image_sizes, original_sizes):
        for pred, size, original in zip(result, image_sizes, original_sizes):
            pred["boxes"] = _boxes.resize_boxes(pred["boxes"], size, original)
        return result


def assemble_features(backbone, transform: Optional[DetectorTransform] = None, autocast_dtype=None, grad: bool = False):
    """The ``features_fn`` that `rois.assemble_detector` takes, from the learned ``backbone`` (backbone + FPN: a torch module from the
    batch to an ordered mapping of feature levels, or to one tensor) alone: `DetectorTransform.batch`, then the backbone under
    no_grad (and under `torch.autocast` of ``autocast_dtype``, if given).  ``transform``: default the reference detector's 800 / 1333
    with the ImageNet constants.  Returns (batch, image_sizes, original_sizes, features).

    ``grad`` = True is the form `rois.assemble_training_detector` takes: the backbone runs in the caller's grad mode, so a loss can
    reach it, and ``features_fn(images, targets)`` sends the targets' boxes through `DetectorTransform.__call__` and returns them,
    resized to the batch, as a fifth value."""
    prepare = transform if transform is not None else DetectorTransform(800, 1333, IMAGENET_MEAN, IMAGENET_STD)

    def features_fn(images, targets=None):
        import contextlib
        import torch
        if targets is not None and not grad:
            raise TypeError("features_fn takes targets only when it was assembled with grad=True")
        resized = None
        if targets is None:
            batch, image_sizes, original_sizes = prepare.batch(images)
        else:
            original_sizes = [(int(v.shape[-2]), int(v.shape[-1])) for v in _image_list(images)]
            (batch, image_sizes), resized = prepare(images, targets)
        cast = torch.autocast("cuda", dtype=autocast_dtype) if autocast_dtype is not None else contextlib.nullcontext()
        with contextlib.nullcontext() if grad else torch.no_grad(), cast:
            features = backbone(batch)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([("0", features)])
        if resized is None:
            return batch, image_sizes, original_sizes, features
        return batch, image_sizes, original_sizes, features, resized

    return features_fn
