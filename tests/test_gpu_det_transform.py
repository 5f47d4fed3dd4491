"""The launch of edtr_amd/detinput.py (csrc/det_transform.hip) against its numpy restatement `transform_reference`: bit for bit, by
uint32 / uint16 views, the padding included.  The restatement itself is held to the reference's own transform in
tests/test_det_transform_cpu.py."""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

from edtr_amd import boxes, detinput, rois

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
TILE_W, TILE_H = 256, 16                # the tile of a slot one workgroup writes (EDTR_DET_TILE_W / _H)
RAGGED = ((53, 47), (40, 167), (61, 163), (64, 64))
SMALL = dict(min_size=64, max_size=100, size_divisible=32)
MEANS = {1: ([0.45], [0.225]), 3: (detinput.IMAGENET_MEAN, detinput.IMAGENET_STD), 4: ([0.485, 0.456, 0.406, 0.5], [0.229, 0.224, 0.225, 0.25])}


@functools.lru_cache(maxsize=None)
def images_of(shapes, C=3, seed=11):
    rng = np.random.default_rng([seed, C, len(shapes)])
    return tuple(rng.uniform(0, 1, (C, h, w)).astype(F32) for h, w in shapes)


@functools.lru_cache(maxsize=None)
def reference(shapes, C=3, dtype="float32", **kw):
    mean, std = MEANS[C]
    return detinput.transform_reference(list(images_of(shapes, C)), image_mean=mean, image_std=std, dtype=dtype, **kw)


def bits(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def want_bits(ref: np.ndarray, dtype: str) -> np.ndarray:
    """the bits of the restatement's batch, which holds 16-bit values widened to fp32"""
    if dtype == "float32":
        return ref.view(np.uint32)
    return ref.astype(np.float16).view(np.uint16) if dtype == "float16" else (ref.view(np.uint32) >> 16).astype(np.uint16)


def check(shapes, C=3, dtype="float32", prefill=False, **kw):
    mean, std = MEANS[C]
    want, sizes, original = reference(shapes, C, dtype, **kw)
    out = None
    if prefill:
        out = torch.full(want.shape, float("nan"), dtype=getattr(torch, dtype), device=DEV)
    got, got_sizes, got_original = detinput.transform([torch.from_numpy(v).to(DEV) for v in images_of(shapes, C)], image_mean=mean, image_std=std,
                                                       dtype=dtype, out=out, **kw)
    assert got.dtype == getattr(torch, dtype) and tuple(got.shape) == want.shape and got_sizes == sizes and got_original == original
    assert out is None or got is out
    g, w = bits(got), want_bits(want, dtype)
    assert np.array_equal(g, w), f"{int((g != w).sum())} of {g.size} words differ"
    for i, (oh, ow) in enumerate(sizes):                 # the padding is +0.0 in bits
        pad = np.ones(want.shape[2:], dtype=bool)
        pad[:oh, :ow] = False
        assert not g[i][:, pad].any()
    return got, sizes


# ---- the ragged set ------------------------------------------------------------------------------------------------------------------------
def test_the_ragged_sets_extents_are_torchs_and_not_the_naive_rules():
    import math
    want = [(72, 63), (23, 100), (37, 99), (64, 64)]
    differ = 0
    for (h, w), e in zip(RAGGED, want):
        shape = torch.tensor([h, w])
        scale = min(64 / min(shape), 100 / max(shape))                  # the reference's lines, on the CPU
        out = torch.nn.functional.interpolate(torch.zeros(1, 1, h, w), scale_factor=scale, mode="bilinear", recompute_scale_factor=True, align_corners=False)
        assert tuple(out.shape[-2:]) == e == detinput.resized_extent(h, w, 64, 100)
        s = min(64 / min(h, w), 100 / max(h, w))
        differ += (math.floor(h * s), math.floor(w * s)) != e
    assert differ == 3 and detinput.batch_extent(want, 32) == (96, 128)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_the_ragged_set_into_a_nan_buffer(dtype):
    """an upscale, a max_size-bound downscale, a downscale and an identity; 4 x 3 x 96 x 128, rows stored 16 (8) bytes per lane"""
    got, sizes = check(RAGGED, dtype=dtype, prefill=True, **SMALL)
    assert tuple(got.shape) == (4, 3, 96, 128) and sizes == [(72, 63), (23, 100), (37, 99), (64, 64)]


# ---- the element-wise store path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_an_odd_pitch_takes_the_element_wise_stores(dtype):
    got, sizes = check(((61, 163),), dtype=dtype, prefill=True, min_size=64, max_size=100, size_divisible=1)
    assert tuple(got.shape) == (1, 3, 37, 99) and sizes == [(37, 99)]


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_a_six_fold_upscale(dtype):
    got, sizes = check(((17, 9),), dtype=dtype, prefill=True, min_size=64, max_size=100, size_divisible=1)
    assert tuple(got.shape) == (1, 3, 100, 52) and sizes == [(100, 52)]
    check(((17, 9), (61, 163)), dtype=dtype, prefill=True, min_size=64, max_size=100, size_divisible=1)         # 100 x 99: both, odd pitch


def test_a_misaligned_out_buffer_takes_the_element_wise_stores():
    """W % 4 == 0 but the buffer starts 4 bytes past a 16-byte boundary"""
    want, sizes, _ = reference(RAGGED, **SMALL)
    flat = torch.full((want.size + 1,), float("nan"), device=DEV)
    out = flat[1:].view(want.shape)
    assert out.data_ptr() % 16 == 4
    got, _, _ = detinput.transform([torch.from_numpy(v).to(DEV) for v in images_of(RAGGED)], out=out, **SMALL)
    assert np.array_equal(bits(got), want.view(np.uint32)) and torch.isnan(flat[0])


# ---- fixed_size and other channel counts ---------------------------------------------------------------------------------------------------
def test_fixed_size():
    got, sizes = check(((53, 47), (30, 70)), prefill=True, min_size=64, max_size=100, size_divisible=32, fixed_size=(48, 40))
    assert sizes == [(40, 48), (40, 48)] and tuple(got.shape) == (2, 3, 64, 64)


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("size_divisible", [32, 1])
def test_one_and_four_channels(C, size_divisible):
    got, _ = check(((53, 47), (61, 163)), C=C, prefill=True, min_size=64, max_size=100, size_divisible=size_divisible)
    assert got.shape[1] == C and got.shape[3] == (128 if size_divisible == 32 else 99)


# ---- tile boundaries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size_divisible", [8, 1])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_three_tiles_in_each_axis_with_a_partial_last_tile(size_divisible, dtype):
    """A slot of two tiles and a part in each axis, derived from the tile: a TILE_H-row image scaled by (2 TILE_H + 6) / TILE_H = 2.375
    (exact in fp32) to 38 x 551, and a second image that ends inside the second column of tiles; 21 k outputs per plane.  With
    size_divisible = 8 the pitch is 552 (vector stores), with 1 it is 551 (element-wise)."""
    assert (TILE_W, TILE_H) == (detinput.TILE_W, detinput.TILE_H)
    oh = 2 * TILE_H + 6
    shapes = ((TILE_H, 232), (12, 100))
    got, sizes = check(shapes, dtype=dtype, prefill=True, min_size=oh, max_size=1000, size_divisible=size_divisible)
    H, W = got.shape[-2:]
    assert sizes[0] == (oh, 551) and 2 * TILE_W < sizes[0][1] < 3 * TILE_W and TILE_W < sizes[1][1] < 2 * TILE_W
    assert -(-H // TILE_H) == 3 and -(-W // TILE_W) == 3 and H % TILE_H and W % TILE_W and (W % 4 == 0) == (size_divisible == 8)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def test_a_non_contiguous_view_a_host_array_and_one_batched_tensor():
    want, sizes, _ = reference(RAGGED, **SMALL)
    imgs = images_of(RAGGED)
    wide = torch.from_numpy(np.concatenate([imgs[0], imgs[0]], axis=2)).to(DEV)
    view = wide[:, :, :imgs[0].shape[2]]
    assert not view.is_contiguous()
    mixed = [view, imgs[1], torch.from_numpy(imgs[2]), torch.from_numpy(imgs[3]).to(DEV)]             # a view, an array, a host and a device tensor
    got, got_sizes, _ = detinput.transform(mixed, **SMALL)
    assert got.is_cuda and got_sizes == sizes and np.array_equal(bits(got), want.view(np.uint32))
    stack = np.stack([imgs[3], imgs[3][:, ::-1].copy()])
    one, _, _ = detinput.transform(torch.from_numpy(stack).to(DEV), **SMALL)
    two, _, _ = detinput.transform(stack, **SMALL)
    ref = detinput.transform_reference(stack, **SMALL)[0]
    assert np.array_equal(bits(one), ref.view(np.uint32)) and np.array_equal(bits(two), ref.view(np.uint32))


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_two_calls_give_the_same_bits_and_nothing_waits_for_the_device():
    """the means of the other no-sync tests: under torch's sync debug mode a device -> host copy, or any other synchronising call,
    inside `transform` raises"""
    want, _, _ = reference(RAGGED, **SMALL)
    resident = [torch.from_numpy(v).to(DEV) for v in images_of(RAGGED)]
    first, _, _ = detinput.transform(resident, **SMALL)                                         # (loads the library, pins the first page)
    out = torch.full(want.shape, float("nan"), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second, sizes, original = detinput.transform(resident, out=out, **SMALL)
        third, _, _ = detinput.transform(resident, dtype="bfloat16", **SMALL)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sizes == [(72, 63), (23, 100), (37, 99), (64, 64)] and original == list(RAGGED)
    assert np.array_equal(bits(first), bits(second)) and np.array_equal(bits(second), want.view(np.uint32))
    assert np.array_equal(bits(third), want_bits(reference(RAGGED, dtype="bfloat16", **SMALL)[0], "bfloat16"))


def test_refusals_on_the_device():
    x = torch.rand(3, 20, 30, device=DEV)
    with pytest.raises(TypeError, match="floating type"):
        detinput.transform([(x * 255).to(torch.uint8)])
    with pytest.raises(ValueError, match="3d tensors"):
        detinput.transform([x[0]])
    with pytest.raises(TypeError):
        detinput.transform([x.double()])
    with pytest.raises(TypeError):
        detinput.transform([x], out=torch.empty(1, 3, 32, 32, device=DEV), **SMALL)             # not the batch's shape
    with pytest.raises(ValueError):
        detinput.transform([x, x[:1]], **SMALL)


# ---- DetectorTransform and the composed detector -------------------------------------------------------------------------------------------
def test_detector_transform_resizes_targets_and_postprocess_undoes_it():
    imgs = images_of(RAGGED)
    t = detinput.DetectorTransform((480, 64), 100, detinput.IMAGENET_MEAN, detinput.IMAGENET_STD)
    rng = np.random.default_rng(3)
    raw = [np.sort(rng.uniform(0, 40, (4, 2, 2)), axis=1).reshape(4, 4).astype(F32) for _ in imgs]
    batch, targets = t([torch.from_numpy(v).to(DEV) for v in imgs], [{"boxes": torch.from_numpy(b).to(DEV), "labels": i} for i, b in enumerate(raw)])
    want, sizes, original = reference(RAGGED, **SMALL)
    assert isinstance(batch, detinput.ImageBatch) and batch.image_sizes == sizes and np.array_equal(bits(batch.tensors), want.view(np.uint32))
    for i, (tg, b) in enumerate(zip(targets, raw)):
        assert tg["labels"] == i
        assert np.array_equal(tg["boxes"].cpu().numpy(), boxes.resize_boxes_reference(b, original[i], sizes[i]))
    back = t.postprocess([{"boxes": tg["boxes"]} for tg in targets], sizes, original)
    for i, r in enumerate(back):
        want_back = boxes.resize_boxes_reference(boxes.resize_boxes_reference(raw[i], original[i], sizes[i]), sizes[i], original[i])
        assert np.array_equal(r["boxes"].cpu().numpy(), want_back)
    with pytest.raises(ValueError, match="masks"):
        t([torch.from_numpy(imgs[3]).to(DEV)], [{"boxes": torch.zeros(1, 4, device=DEV), "masks": None}])


class RpnHead(torch.nn.Module):
    def __init__(self, C, A):
        super().__init__()
        self.conv, self.cls, self.box = torch.nn.Conv2d(C, C, 3, padding=1), torch.nn.Conv2d(C, A, 1), torch.nn.Conv2d(C, 4 * A, 1)

    def forward(self, feats):
        hidden = [torch.relu(self.conv(f)) for f in feats]
        return [self.cls(h) * 4 for h in hidden], [self.box(h) for h in hidden]


class Predictor(torch.nn.Module):
    def __init__(self, D, classes):
        super().__init__()
        self.cls, self.box = torch.nn.Linear(D, classes), torch.nn.Linear(D, 4 * classes)

    def forward(self, x):
        return self.cls(x) * 6, self.box(x)


class Backbone(torch.nn.Module):
    def __init__(self, C):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, C, 3, padding=1)

    def forward(self, batch):
        x = torch.relu(self.stem(batch))
        return OrderedDict((str(l), torch.nn.functional.avg_pool2d(x, 4 * 2 ** l).contiguous()) for l in range(3))


def test_assemble_features_feeds_assemble_detector_with_nothing_but_the_learned_parts():
    """The flow test of tests/test_gpu_rois.py with `detinput.assemble_features(backbone)` for its hand-written features_fn: a 40 x 60
    image (-> 64 x 96) next to a 25 x 40 one (-> 62 x 100) in a 64 x 128 batch, 3 levels.  The result equals
    `rois.assemble_detector_reference` replayed from the trace (the bound of that test: labels equal, boxes and scores 1e-5)."""
    torch.manual_seed(7)
    C, A, classes = 8, 3, 5
    backbone, rpn_head = Backbone(C).to(DEV), RpnHead(C, A).to(DEV)
    box_head = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(C * 49, 32), torch.nn.ReLU()).to(DEV)
    predictor = Predictor(32, classes).to(DEV)
    shapes = ((40, 60), (25, 40))
    t = detinput.DetectorTransform(**{k: v for k, v in SMALL.items()}, image_mean=detinput.IMAGENET_MEAN, image_std=detinput.IMAGENET_STD)
    features_fn = detinput.assemble_features(backbone, t)
    kw = dict(sizes=((8,), (16,), (32,)), aspect_ratios=((0.5, 1.0, 2.0),) * 3, rpn_pre_nms_top_n=100, rpn_post_nms_top_n=40, box_score_thresh=0.05,
              box_detections_per_img=20)
    images = [torch.from_numpy(v).to(DEV) for v in images_of(shapes)]
    want_batch, sizes, original = reference(shapes, **SMALL)
    assert sizes == [(64, 96), (62, 100)] and want_batch.shape == (2, 3, 64, 128)

    batch, got_sizes, got_original, feats = features_fn(images)
    assert np.array_equal(bits(batch), want_batch.view(np.uint32)) and got_sizes == sizes and got_original == original == list(shapes)
    assert list(feats) == ["0", "1", "2"] and tuple(feats["0"].shape) == (2, C, 16, 32)

    trace = {}
    out = rois.assemble_detector(features_fn, rpn_head, box_head, predictor, trace=trace, **kw)(images)
    want = rois.assemble_detector_reference(None, None, None, None, replay=trace, **kw)(images)
    assert trace["image_sizes"] == sizes and trace["original_sizes"] == original and trace["batch_shape"] == want_batch.shape[-2:]
    assert len(out) == len(want) == 2 and sum(len(w["labels"]) for w in want) > 0
    for o, w in zip(out, want):
        assert o["labels"].dtype == torch.int64 and o["labels"].cpu().numpy().tolist() == w["labels"].tolist()
        np.testing.assert_allclose(o["boxes"].cpu().numpy(), w["boxes"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(o["scores"].cpu().numpy(), w["scores"], rtol=1e-5, atol=0)
    for o, (h, w_) in zip(out, original):                                # back in the original image's coordinates
        b = o["boxes"].cpu().numpy()
        assert b.size == 0 or (b.min() >= 0 and b[:, 2].max() <= w_ * (1 + 1e-6) and b[:, 3].max() <= h * (1 + 1e-6))


def test_assemble_features_defaults_and_autocast():
    features_fn = detinput.assemble_features(torch.nn.Conv2d(3, 4, 3, padding=1).to(DEV), autocast_dtype=torch.bfloat16)
    batch, sizes, original, feats = features_fn([torch.rand(3, 30, 40, device=DEV)])                 # 800 / 1333: 30 x 40 -> 800 x 1066
    assert sizes == [detinput.resized_extent(30, 40)] == [(800, 1066)] and tuple(batch.shape) == (1, 3, 800, 1088) and original == [(30, 40)]
    assert list(feats) == ["0"] and feats["0"].dtype == torch.bfloat16 and batch.dtype == torch.float32
    assert not batch[0, :, :, 1066:].any() and not batch.isnan().any()
