"""The 8-bit image boundary around the fp32 NCHW batches (include/edtr_hip.h "Images in, images out"; kernels in csrc/imageio.hip):
what the reference's callers do around the restoration path with Pillow, numpy and torchvision — `Image.resize(size, BICUBIC)`
(demo.py:80-84), `np.array(img) / 255.0` -> CHW -> `pad_if_smaller` -> `pad_to_multiples_of` (demo.py:85-90), replicate padding
(main/seg/test_edtr.py:113-115), the crop and `save_image` (demo.py:165) and `calculate_psnr_pt` — as four launches on uint8 HWC
images.  Three rules make the device results a bit-exact function of the bytes, and each is restated here in numpy for the tests:

  resize   Pillow's algorithm: per output position a window (xmin, n) and n coefficients, built in float64 (`resize_coeffs`), turned
           into 22-bit fixed point; int32 accumulation from 1 << 21, clamp(acc >> 22, 0, 255); a horizontal pass, then a vertical
           pass over its uint8 result; a pass whose axis keeps its size is skipped (`resize_u8_reference`)
  ingest   a byte v becomes float32(float64(v) / 255.0) — `INGEST_TABLE`, read by the kernel: no device division, no double rounding
  emit     trunc(clamp(x * 255 + 0.5, 0, 255)), the product and the sum each rounded to fp32 (never an FMA); NaN gives 0
           (`emit_reference`)

A whole ragged batch crosses the boundary in a fixed number of launches (`ingest_resized`: at most two, `emit_packed`: one; the same bits
as `resize_u8` -> `ingest` and `emit` per image), and `plan_buckets` groups images of one padded extent so that such batches exist.

Host side: numpy.  Device side: torch owns the buffers; every computation is a libedtr_hip launch (a missing library is an error)."""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import numpy as np

PRECISION_BITS = 22                     # Pillow: 32 - 8 - 2
BICUBIC_SUPPORT = 2.0
# demo.py:85 computes np.array(img) / 255.0 in float64 and rounds once to float32
INGEST_TABLE = np.array([np.float32(float(v) / 255.0) for v in range(256)], dtype=np.float32)


def _bicubic(x: np.ndarray) -> np.ndarray:
    """Pillow's bicubic_filter (Keys, a = -0.5), with its order of operations."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resize_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out_size, 2] = (xmin, n), coefs int32 [out_size, ksize]) of one axis of `Image.resize(..., BICUBIC)`:
    Pillow's precompute_coeffs + normalize_coeffs_8bpc in float64.  Entries past n are zero."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = BICUBIC_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coefs = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)              # int() truncates toward zero, as the C cast does
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = _bicubic((np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w:                                             # summed in index order
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        fixed = w * float(1 << PRECISION_BITS)
        coefs[xx, :n] = np.where(w < 0.0, fixed - 0.5, fixed + 0.5).astype(np.int64)       # (astype truncates toward zero)
        bounds[xx] = (xmin, n)
    return bounds, coefs


def _resample_axis0(img: np.ndarray, bounds: np.ndarray, coefs: np.ndarray) -> np.ndarray:
    """One pass along axis 0 of a uint8 array: int32 accumulation from 1 << 21, clamp(acc >> 22, 0, 255)."""
    out = np.empty((bounds.shape[0],) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int32)
    for i, (lo, n) in enumerate(bounds):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        acc = acc + np.tensordot(coefs[i, :n], src[lo:lo + n], axes=(0, 0)).astype(np.int32)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8_reference(img: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
    """numpy restatement of `Image.fromarray(img).resize((out_w, out_h), Image.BICUBIC)` on uint8 [h, w, c]."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise TypeError("resize_u8_reference takes a uint8 [h, w, c] array")
    h, w, _ = img.shape
    if out_w != w:
        img = _resample_axis0(img.transpose(1, 0, 2), *resize_coeffs(w, out_w)).transpose(1, 0, 2)
    if out_h != h:
        img = _resample_axis0(img, *resize_coeffs(h, out_h))
    return np.ascontiguousarray(img)


def demo_size(w: int, h: int, scale: float = -1.0) -> Tuple[int, int]:
    """(out_w, out_h) of demo.py:80-84: the longer side to 512 with `int(round(...))` when scale == -1.0, else `int(x * scale)`."""
    if scale == -1.0:
        s = 512 / max(w, h)
        return int(round(w * s)), int(round(h * s))
    return int(w * scale), int(h * scale)


def emit_reference(x: np.ndarray) -> np.ndarray:
    """numpy statement of the emit rule on a float32 array: x * 255 rounded to fp32, + 0.5 rounded to fp32, clamped, truncated; NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    t = (x * np.float32(255.0)).astype(np.float32) + np.float32(0.5)
    t = np.where(np.isnan(t), np.float32(0.0), np.clip(t, np.float32(0.0), np.float32(255.0)))
    return t.astype(np.uint8)


def _packed_offsets(sizes: Sequence[Tuple[int, int]]) -> Tuple[List[int], int]:
    """(byte offset of every [h, w, 3] crop in the packed buffer, total bytes): back to back, each start raised to a multiple of 4."""
    offs, at = [], 0
    for h, w in sizes:
        offs.append(at)
        at = _round_up(at + int(h) * int(w) * 3, 4)
    return offs, at


def ingest_resized_reference(images, out_sizes, size=None, pad: str = "zero", multiple: Optional[int] = None, min_size: Optional[int] = None):
    """numpy restatement of `ingest_resized`: `resize_u8_reference` -> `INGEST_TABLE` (v / 255) -> CHW -> padding, per image.
    Returns (float32 [B, 3, H, W], [(h, w), ...])."""
    if pad not in ("zero", "replicate"):
        raise ValueError(f"pad must be 'zero' or 'replicate', got {pad!r}")
    small = [resize_u8_reference(np.asarray(im), int(ow), int(oh)) for im, (ow, oh) in zip(images, out_sizes)]
    sizes = [(a.shape[0], a.shape[1]) for a in small]
    H, W = batch_extent(sizes, size, multiple, min_size)
    batch = np.empty((len(small), 3, H, W), dtype=np.float32)
    for b, a in enumerate(small):
        chw = INGEST_TABLE[a].transpose(2, 0, 1)
        batch[b] = np.pad(chw, ((0, 0), (0, H - a.shape[0]), (0, W - a.shape[1])), mode="edge" if pad == "replicate" else "constant")
    return batch, sizes


def emit_packed_reference(batch: np.ndarray, sizes: Sequence[Tuple[int, int]]):
    """numpy restatement of `emit_packed`: (packed uint8 buffer, byte offsets); crop i = `emit_reference` of batch[i, :, :h, :w] as HWC at
    offsets[i].  Bytes between the crops are zero here (the device leaves them as they were)."""
    offs, total = _packed_offsets(sizes)
    out = np.zeros(total, dtype=np.uint8)
    for i, ((h, w), o) in enumerate(zip(sizes, offs)):
        out[o:o + h * w * 3] = emit_reference(np.asarray(batch[i])[:, :h, :w].transpose(1, 2, 0)).reshape(-1)
    return out, offs


def plan_buckets(sizes: Sequence[Tuple[int, int]], batch_size: int, min_size: Optional[int] = None,
                 multiple: Optional[int] = None) -> List[Tuple[Tuple[int, int], List[int]]]:
    """Group images by padded extent: ``sizes`` are the images' (h, w) after any resize; image k belongs to the bucket
    `batch_extent([sizes[k]], multiple=multiple, min_size=min_size)`.  Buckets are opened in the order their first image appears, the
    indices of a bucket keep data-set order, and a bucket is cut into chunks of at most ``batch_size``.  Returns the chunks as
    [((H, W), [indices]), ...]: a partition of range(len(sizes)) that depends on nothing but the arguments.  Pure Python."""
    batch_size = int(batch_size)
    if batch_size <= 0:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    buckets: dict = {}                          # (dicts keep insertion order)
    for k, (h, w) in enumerate(sizes):
        buckets.setdefault(batch_extent([(int(h), int(w))], multiple=multiple, min_size=min_size), []).append(k)
    return [(hw, idx[i:i + batch_size]) for hw, idx in buckets.items() for i in range(0, len(idx), batch_size)]


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
_ON_DEVICE: dict = {}                   # family -> {key + device: tensor(s)}: what `on_device` keeps
_RESIZE_TABLES: OrderedDict = OrderedDict()     # (in, out, device) -> (bounds, coefficients): the RESIZE_TABLES_KEPT most recently used
RESIZE_TABLES_KEPT = 64


def _device(device=None):
    import torch
    return torch.device(device if device is not None else "cuda")


def _device_key(device) -> Tuple[str, int]:
    """("cuda", index), with the current device's index for a bare "cuda": one cache entry per physical device."""
    import torch
    d = torch.device(device)
    return d.type, d.index if d.index is not None else (torch.cuda.current_device() if d.type == "cuda" else 0)


def on_device(key: tuple, device, build, kept: int = 0):
    """The device copy of ``build()`` (a numpy array, or a tuple of them -> a tuple of tensors): built once and uploaded once per
    ``key`` and physical device.  ``key[0]`` names the family of tables; ``kept`` > 0 bounds the family, oldest entry out first.
    (A table that a queued launch still reads stays valid as long as that launch was queued on the stream the table was allocated
    on: torch's allocator hands a freed block out again on that stream only, behind the launch.)"""
    import torch
    cache = _ON_DEVICE.setdefault(key[0], {})
    key = key + _device_key(device)
    if key not in cache:
        while kept and len(cache) >= kept:
            cache.pop(next(iter(cache)))
        made = build()
        cache[key] = tuple(torch.from_numpy(a).to(device) for a in made) if isinstance(made, tuple) else torch.from_numpy(made).to(device)
    return cache[key]


def _ingest_table(device):
    return on_device(("ingest",), device, INGEST_TABLE.copy)      # one 1 KB table per device: kept for good


def _resize_tables(in_size: int, out_size: int, device):
    import torch
    key = (in_size, out_size) + _device_key(device)
    if key in _RESIZE_TABLES:
        _RESIZE_TABLES.move_to_end(key)
        return _RESIZE_TABLES[key]
    while len(_RESIZE_TABLES) >= RESIZE_TABLES_KEPT:
        _RESIZE_TABLES.popitem(last=False)          # (a table a queued launch still reads stays valid: frees are stream-ordered)
    _RESIZE_TABLES[key] = tuple(torch.from_numpy(t).to(device) for t in resize_coeffs(in_size, out_size))
    return _RESIZE_TABLES[key]


def is_u8_image(x) -> bool:
    """A uint8 [h, w, 3] torch tensor or numpy array (what Pillow decodes to)?"""
    import torch
    dt = getattr(x, "dtype", None)
    return (dt == torch.uint8 or dt == np.uint8) and getattr(x, "ndim", 0) == 3 and x.shape[-1] == 3


def _hwc_on(img, device):
    """``img`` (torch tensor or numpy array, uint8 or floating, [h, w, 3]) as a contiguous uint8 / fp32 tensor on ``device``."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    if t.ndim != 3 or t.shape[-1] != 3:
        raise ValueError(f"expected an [h, w, 3] image, got {tuple(t.shape)}")
    if t.dtype != torch.uint8:
        t = t.float()
    return t.to(device).contiguous()


def resize_u8(img, out_w: int, out_h: int, device=None):
    """`Image.resize((out_w, out_h), Image.BICUBIC)` of a uint8 [h, w, 3] image on the device -> uint8 [out_h, out_w, 3] tensor."""
    import torch
    from . import ops
    dev = img.device if isinstance(img, torch.Tensor) and img.is_cuda and device is None else _device(device)
    src = _hwc_on(img, dev)
    if src.dtype != torch.uint8:
        raise TypeError("resize_u8 takes a uint8 image")
    h, w, _ = src.shape
    out_w, out_h = int(out_w), int(out_h)
    if out_w <= 0 or out_h <= 0:
        raise ValueError(f"output size must be positive, got {out_w} x {out_h}")
    dst = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=dev)
    h_tab = _resize_tables(w, out_w, dev) if out_w != w else None
    v_tab = _resize_tables(h, out_h, dev) if out_h != h else None
    tmp = torch.empty((h, out_w, 3), dtype=torch.uint8, device=dev) if h_tab is not None and v_tab is not None else None
    ops.launch(ops.make_image_resize_u8(src=src, dst=dst, h_tab=h_tab, v_tab=v_tab, tmp=tmp))
    return dst


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def batch_extent(sizes: Sequence[Tuple[int, int]], size=None, multiple: Optional[int] = None, min_size: Optional[int] = None) -> Tuple[int, int]:
    """(H, W) of the batch `ingest` builds: ``size`` when given, else the largest image, raised to ``min_size`` (pad_if_smaller) and
    then to the next multiple of ``multiple`` (pad_to_multiples_of)."""
    if size is not None:
        H, W = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    else:
        H, W = max(h for h, _ in sizes), max(w for _, w in sizes)
    if min_size is not None:
        H, W = max(H, int(min_size)), max(W, int(min_size))
    if multiple is not None:
        H, W = _round_up(H, int(multiple)), _round_up(W, int(multiple))
    for h, w in sizes:
        if h > H or w > W:
            raise ValueError(f"a {h} x {w} image does not fit the {H} x {W} batch")
    return H, W


def ingest(images, size=None, pad: str = "zero", multiple: Optional[int] = None, min_size: Optional[int] = None, device=None):
    """uint8 (or floating, copied as fp32) [h, w, 3] images -> (fp32 [B, 3, H, W] batch on the device, [(h, w), ...]): every image
    top-left in its slot, the rest of the slot zero (``pad="zero"``: F.pad 'constant') or the last row / column repeated
    (``"replicate"``).  (H, W): see `batch_extent`."""
    import torch
    from . import ops
    if pad not in ("zero", "replicate"):
        raise ValueError(f"pad must be 'zero' or 'replicate', got {pad!r}")
    images = list(images)
    if not images:
        raise ValueError("ingest needs at least one image")
    first = images[0]
    dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda and device is None else _device(device)
    srcs = [_hwc_on(im, dev) for im in images]
    sizes = [(int(s.shape[0]), int(s.shape[1])) for s in srcs]
    H, W = batch_extent(sizes, size, multiple, min_size)
    batch = torch.empty((len(srcs), 3, H, W), dtype=torch.float32, device=dev)
    table = _ingest_table(dev)
    for b, s in enumerate(srcs):
        ops.launch(ops.make_image_ingest(src=s, batch=batch, b=b, replicate=pad == "replicate", table=table))
    return batch, sizes


def emit(batch, sizes: Sequence[Tuple[int, int]]) -> List:
    """fp32 [B, 3, H, W] -> one uint8 [h, w, 3] tensor per image: the top-left (h, w) crop with save_image's quantisation."""
    import torch
    from . import ops
    if batch.ndim != 4 or batch.dtype != torch.float32 or not batch.is_contiguous():
        raise TypeError("emit takes a contiguous fp32 [B, 3, H, W] batch")
    if len(sizes) != batch.shape[0]:
        raise ValueError(f"{len(sizes)} sizes for a batch of {batch.shape[0]}")
    outs = []
    for b, (h, w) in enumerate(sizes):
        dst = torch.empty((int(h), int(w), 3), dtype=torch.uint8, device=batch.device)
        ops.launch(ops.make_image_emit(batch=batch, b=b, dst=dst))
        outs.append(dst)
    return outs


def ingest_resized(images, out_sizes, size=None, pad: str = "zero", multiple: Optional[int] = None, min_size: Optional[int] = None, device=None):
    """`resize_u8` of every uint8 [h, w, 3] image to its (out_w, out_h) of ``out_sizes`` and `ingest` of the results, for the whole
    list in at most two launches (edtr_image_resize_h_batch, edtr_image_resize_ingest_batch): host images travel in one upload, the
    horizontal results share one scratch allocation, the resized uint8 images are never written.  Returns (batch, sizes) like
    `ingest`, bit for bit what `ingest([resize_u8(im, ow, oh) for ...], size, pad, multiple, min_size)` returns."""
    import torch
    from . import lib as L
    from . import ops
    if pad not in ("zero", "replicate"):
        raise ValueError(f"pad must be 'zero' or 'replicate', got {pad!r}")
    images, out_sizes = list(images), [(int(ow), int(oh)) for ow, oh in out_sizes]
    if not images or len(images) != len(out_sizes):
        raise ValueError(f"ingest_resized needs as many output sizes as images, got {len(out_sizes)} for {len(images)}")
    first = images[0]
    dev = first.device if isinstance(first, torch.Tensor) and first.is_cuda and device is None else _device(device)
    hosts = []                                  # (index, contiguous uint8 host tensor): packed into one upload
    srcs: list = [None] * len(images)
    for i, im in enumerate(images):
        t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
        if t.dtype != torch.uint8 or t.ndim != 3 or t.shape[-1] != 3:
            raise TypeError("ingest_resized takes uint8 [h, w, 3] images")
        if t.is_cuda:
            srcs[i] = t.to(dev).contiguous()
        else:
            hosts.append((i, t.contiguous()))
    if hosts:
        offs, total = _packed_offsets([(t.shape[0], t.shape[1]) for _, t in hosts])
        stage = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
        for (_, t), o in zip(hosts, offs):
            stage[o:o + t.numel()].copy_(t.reshape(-1))
        up = stage.to(dev, non_blocking=True)
        for (i, t), o in zip(hosts, offs):
            srcs[i] = up[o:o + t.numel()].view(t.shape)
    for ow, oh in out_sizes:
        if ow <= 0 or oh <= 0:
            raise ValueError(f"output size must be positive, got {ow} x {oh}")
    sizes = [(oh, ow) for ow, oh in out_sizes]
    H, W = batch_extent(sizes, size, multiple, min_size)
    descs = (L.ImageDesc * len(srcs))()
    keep, tmp_bytes = [], 0
    for b, (s, (ow, oh)) in enumerate(zip(srcs, out_sizes)):
        h, w = int(s.shape[0]), int(s.shape[1])
        d = descs[b]
        d.src, d.in_h, d.in_w, d.out_h, d.out_w, d.b = s.data_ptr(), h, w, oh, ow, b
        if ow != w:
            hb, hc = _resize_tables(w, ow, dev)
            d.h_bounds, d.h_coefs, d.h_ksize, d.tmp_offset = hb.data_ptr(), hc.data_ptr(), hc.shape[1], tmp_bytes
            tmp_bytes = _round_up(tmp_bytes + h * ow * 3, 4)
            keep += [hb, hc]
        if oh != h:
            vb, vc = _resize_tables(h, oh, dev)
            d.v_bounds, d.v_coefs, d.v_ksize = vb.data_ptr(), vc.data_ptr(), vc.shape[1]
            keep += [vb, vc]
    keep += srcs
    ddescs = torch.frombuffer(descs, dtype=torch.uint8).to(dev)
    tmp = torch.empty((tmp_bytes,), dtype=torch.uint8, device=dev) if tmp_bytes else None
    batch = torch.empty((len(srcs), 3, H, W), dtype=torch.float32, device=dev)
    if tmp is not None:
        ops.launch(ops.make_image_resize_h_batch(descs_host=descs, descs=ddescs, tmp=tmp, keep=keep))
    ops.launch(ops.make_image_resize_ingest_batch(descs_host=descs, descs=ddescs, tmp=tmp, batch=batch, replicate=pad == "replicate",
                                                  table=_ingest_table(dev), keep=keep))
    return batch, sizes


def emit_packed(batch, sizes: Sequence[Tuple[int, int]]):
    """`emit` of a whole batch in one launch (edtr_image_emit_batch) into ONE uint8 device buffer: returns (packed, views), views[i] the
    uint8 [h, w, 3] view of image i's bytes at its 4-byte aligned offset (`_packed_offsets`) — the bytes `emit` gives.  A caller
    brings the batch to the host with one copy of ``packed``."""
    import ctypes
    import torch
    from . import ops
    if batch.ndim != 4 or batch.dtype != torch.float32 or not batch.is_contiguous():
        raise TypeError("emit_packed takes a contiguous fp32 [B, 3, H, W] batch")
    if len(sizes) != batch.shape[0]:
        raise ValueError(f"{len(sizes)} sizes for a batch of {batch.shape[0]}")
    sizes = [(int(h), int(w)) for h, w in sizes]
    offs, total = _packed_offsets(sizes)
    rows = [v for b, ((h, w), o) in enumerate(zip(sizes, offs)) for v in (b, h, w, o)]
    table_host = (ctypes.c_int64 * len(rows))(*rows)
    table = torch.tensor(rows, dtype=torch.int64).to(batch.device)
    packed = torch.empty((total,), dtype=torch.uint8, device=batch.device)
    ops.launch(ops.make_image_emit_batch(batch=batch, table_host=table_host, table=table, dst=packed))
    return packed, [packed[o:o + h * w * 3].view(h, w, 3) for (h, w), o in zip(sizes, offs)]


def sqdiff(a, b, sizes=None, crop_border: int = 0, test_y_channel: bool = False):
    """(fp64 [B] sums of squared differences on the device, fp64 [B] element counts) of two fp32 [B, 3, H, W] batches over each
    image's valid (h, w) extent less ``crop_border`` on every side.  Fixed summation order: equal bits on every run."""
    import torch
    from . import lib as L
    from . import ops
    if a.shape != b.shape or a.ndim != 4:
        raise ValueError(f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError("sqdiff takes fp32 batches")
    a, b = a.contiguous(), b.contiguous()
    B, _, H, W = a.shape
    hw = [(H, W)] * B if sizes is None else [(int(h), int(w)) for h, w in sizes]
    if len(hw) != B:
        raise ValueError(f"{len(hw)} sizes for a batch of {B}")
    cb = int(crop_border)
    counts = []
    for h, w in hw:
        if not (0 < h <= H and 0 < w <= W) or cb < 0 or h - 2 * cb <= 0 or w - 2 * cb <= 0:
            raise ValueError(f"nothing left of a {h} x {w} image in a {H} x {W} batch with crop_border {cb}")
        counts.append((1 if test_y_channel else 3) * (h - 2 * cb) * (w - 2 * cb))
    dsizes = None if sizes is None else torch.tensor(hw, dtype=torch.int32).to(a.device)
    partials = torch.empty((B, L.SQDIFF_BLOCKS), dtype=torch.float64, device=a.device)
    out = torch.empty((B,), dtype=torch.float64, device=a.device)
    ops.launch(ops.make_image_sqdiff(a=a, b=b, sizes=dsizes, crop_border=cb, y_channel=test_y_channel, partials=partials, out=out))
    return out, torch.tensor(counts, dtype=torch.float64).to(a.device)


def psnr(a, b, sizes=None, crop_border: int = 0, test_y_channel: bool = False):
    """Per-image PSNR in dB (fp64 [B] on the device) of fp32 [B, 3, H, W] batches in [0, 1]: `calculate_psnr_pt` (utils/common.py:219-247)
    with the reduction done by edtr_image_sqdiff; ``sizes`` gives every image of a padded batch the PSNR it gets alone.  The Y form
    is the BT.601 luma in fp64 (the reference rounds it to fp32 first: equal to ~1e-6 dB, not bit for bit)."""
    import torch
    s, n = sqdiff(a, b, sizes, crop_border, test_y_channel)
    return 10.0 * torch.log10(1.0 / (s / n + 1e-8))
