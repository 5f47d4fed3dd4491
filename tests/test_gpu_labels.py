"""The label-map launches on the device (csrc/labels.hip, include/edtr_hip.h "Label maps") against their numpy restatements
(edtr_amd/labels.py), by EQUALITY: each is an integer or gather function of its inputs.  Shapes are the smallest at which a launch
can still go wrong: widths that are and are not multiples of 4 (the dword / float4 forms and the element-by-element ones), a base one
element into a buffer, more than one workgroup, a capped grid that has to stride, and every output inside a guarded buffer at an
aligned and at an odd offset whose guards must come back untouched."""
import os

import numpy as np
import pytest
import torch

from edtr_amd import labels, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GUARD = 0xA5
NEAREST_CASES = [(2, 2, 7, 15), (3, 2, 21, 7), (1, 5, 1, 1), (5, 1, 3, 9), (2, 64, 23, 33), (9, 9, 9, 9), (281, 500, 307, 546)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "labels.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what=""):
    """bit equality of two arrays (device tensors are copied); what differs is printed before the assertion"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    if bad.any():
        print(f"\n[{what}] {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}: "
              f"{got[tuple(np.argwhere(bad)[0])]} for {want[tuple(np.argwhere(bad)[0])]}")
    return not bad.any()


def guarded(shape, offset):
    """a uint8 output of ``shape`` at byte ``offset`` of a buffer of GUARD bytes (64: 4-byte aligned; 61: not)"""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + 67,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[offset:offset + n].view(shape)


def guards_ok(buf, shape, offset):
    n = int(np.prod(shape))
    return bool((buf[:offset] == GUARD).all()) and bool((buf[offset + n:] == GUARD).all())


def targets(shape, n, seed):
    """uint8 targets that hold every class below ``n``, the ignore label, n itself and 200 (all three are ignored)"""
    t = np.random.default_rng(seed).integers(0, n, size=shape).astype(np.uint8)
    flat = t.reshape(-1)
    flat[:n] = np.arange(n)
    flat[n:n + 3] = (255, n, 200)
    return t


def check_confusion(logits_t, target, n, sizes=None, max_blocks=0):
    """mat and pred of one launch against the restatement on the values the device holds; returns the matrix"""
    host = logits_t.float().cpu().numpy()            # (16-bit logits widen exactly)
    want_mat, want_pred = labels.confusion_reference(host, target, n, sizes=sizes, return_pred=True)
    mat, pred = labels.confusion(logits_t, dev(target), n, sizes=sizes, return_pred=True, max_blocks=max_blocks)
    assert mat.dtype == torch.int64 and same(mat, want_mat, "mat")
    assert same(pred, want_pred, "pred")                      # every pixel, ignored ones and those outside sizes included
    assert same(pred, logits_t.cpu().argmax(1).to(torch.uint8), "pred against torch's CPU argmax")
    alone = labels.confusion(logits_t, dev(target), n, sizes=sizes, max_blocks=max_blocks)          # the form without pred
    assert same(alone, want_mat, "mat without pred")
    counted = target < n
    if sizes is not None:
        for b, (h, w) in enumerate(sizes):
            counted[b, h:, :] = False
            counted[b, :, w:] = False
    assert int(mat.sum()) == int(counted.sum())
    return want_mat


# ---- confusion -------------------------------------------------------------------------------------------------------------------------
def test_confusion_planted_argmax_cases():
    """n = 21 at (2, 21, 5, 7), fp32, W % 4 != 0 (the element-by-element path): the pixels where torch's CPU rule is not the obvious one"""
    nan, inf = float("nan"), float("inf")
    rng = np.random.default_rng(1)
    logits = rng.standard_normal((2, 21, 5, 7)).astype(np.float32)
    planted = {}

    def plant(b, y, x, base, values, want):
        logits[b, :, y, x] = base
        for c, v in values.items():
            logits[b, c, y, x] = v
        planted[(b, y, x)] = want

    plant(0, 0, 0, 0.0, {3: 5.0, 9: 5.0}, 3)                       # a tie: the lower index
    plant(0, 1, 6, -1.0, {0: 7.0, 4: 7.0, 11: 7.0}, 0)             # a three-way tie that includes channel 0
    plant(0, 2, 3, -1.0, {2: -0.0, 5: 0.0}, 2)                     # -0.0 against 0.0 is a tie
    plant(0, 2, 4, -1.0, {2: 0.0, 5: -0.0}, 2)
    plant(1, 0, 5, 0.0, {6: inf, 13: inf}, 6)                      # +inf twice
    plant(1, 3, 2, 0.0, {1: 100.0, 8: nan}, 8)                     # a NaN behind a larger value
    plant(1, 4, 6, 0.0, {3: 50.0, 9: nan, 17: nan}, 9)             # two NaNs: the first
    plant(1, 4, 0, 0.0, {0: nan, 20: inf}, 0)                      # a NaN in channel 0 is never displaced
    plant(1, 2, 2, -inf, {}, 0)                                    # every channel -inf
    target = targets((2, 5, 7), 21, 2)
    for (b, y, x) in list(planted)[:4]:
        target[b, y, x] = 255                                      # some planted pixels are ignored ones: pred is written all the same
    check_confusion(dev(logits), target, 21)
    _, pred = labels.confusion(dev(logits), dev(target), 21, return_pred=True)
    pred = pred.cpu().numpy()
    for (b, y, x), want in planted.items():
        assert pred[b, y, x] == want, ((b, y, x), int(pred[b, y, x]), want)


def test_confusion_vector_path_and_a_misaligned_base():
    rng = np.random.default_rng(3)
    logits = np.round(rng.standard_normal((1, 21, 8, 16)) * 2).astype(np.float32) / 2          # coarse values: many ties
    target = targets((1, 8, 16), 21, 4)
    want = check_confusion(dev(logits), target, 21)
    buf = torch.zeros(logits.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(logits.shape)
    view.copy_(dev(logits))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert np.array_equal(check_confusion(view, target, 21), want)
    # a target and a pred one byte into their buffers: the same matrix through the element-by-element kernel, guards untouched
    tbuf = torch.zeros(target.size + 1, dtype=torch.uint8, device=DEV)
    tview = tbuf[1:].view(target.shape)
    tview.copy_(dev(target))
    for offset in (64, 61):
        pbuf, pred = guarded(target.shape, offset)
        mat = torch.zeros((21, 21), dtype=torch.int64, device=DEV)
        ops.launch(ops.make_seg_confusion(logits=dev(logits), target=tview, mat=mat, pred=pred))
        assert same(mat, want) and same(pred, labels.argmax_reference(logits)) and guards_ok(pbuf, target.shape, offset)


@pytest.mark.parametrize("n", [1, 2, 32])
def test_confusion_class_counts(n):
    rng = np.random.default_rng(10 + n)
    for shape in ((2, n, 6, 8), (1, n, 5, 7)):
        logits = np.round(rng.standard_normal(shape) * 2).astype(np.float32) / 2
        t = rng.integers(0, n, size=(shape[0],) + shape[2:]).astype(np.uint8)
        t.reshape(-1)[:3] = (255, n, 200)
        t.reshape(-1)[3:3 + min(n, 32)] = np.arange(min(n, 32))
        check_confusion(dev(logits), t, n)


def test_confusion_refuses_more_than_32_classes():
    logits = torch.zeros((1, 33, 4, 4), device=DEV)
    with pytest.raises(RuntimeError, match="-5"):
        labels.confusion(logits, torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV), 33)
    with pytest.raises(ValueError):
        labels.confusion(logits, torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV), 21)
    with pytest.raises(RuntimeError, match="-2"):          # a sizes entry outside the slot: refused by the entry point, nothing launched
        labels.confusion(logits[:, :21].contiguous(), torch.zeros((1, 4, 4), dtype=torch.uint8, device=DEV), 21, sizes=[(5, 4)])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 21, 8, 16), (2, 21, 5, 7)])
def test_confusion_16_bit_logits(dtype, shape):
    gen = torch.Generator().manual_seed(5)
    logits = (torch.randn(shape, generator=gen) * 3).to(dtype)
    logits[:, 7] = logits[:, 3]                    # a tie wherever plane 3 holds the maximum
    logits[0, 4, 1, 2] = float("nan")
    logits[1, 0, 0, 0] = float("inf")
    logits[1, 20, 0, 0] = float("inf")
    host = logits.float().numpy()
    assert (np.sort(host, axis=1)[:, -1] == np.sort(host, axis=1)[:, -2]).any(), "the 16-bit case needs ties among its maxima"
    check_confusion(logits.to(DEV), targets((shape[0],) + shape[2:], 21, 6), 21)
    buf = torch.zeros(logits.numel() + 1, dtype=dtype, device=DEV)         # 2 bytes off an 8-byte boundary
    buf[1:].view(shape).copy_(logits)
    check_confusion(buf[1:].view(shape), targets((shape[0],) + shape[2:], 21, 6), 21)


@pytest.mark.parametrize("shape", [(3, 21, 8, 16), (3, 21, 6, 11)])
def test_confusion_sizes(shape):
    rng = np.random.default_rng(7)
    logits = rng.standard_normal(shape).astype(np.float32)
    B, _, H, W = shape
    target = targets((B, H, W), 21, 8)
    check_confusion(dev(logits), target, 21, sizes=[(1, 1), (H, W), (H - 3, W - 5)])
    check_confusion(dev(logits), target, 21, sizes=[(H, 2), (3, W), (H, W)])


def test_confusion_capped_grid_strides_and_accumulates(gold):
    rng = np.random.default_rng(9)
    logits = np.round(rng.standard_normal((1, 21, 40, 64)) * 4).astype(np.float32) / 4
    target = targets((1, 40, 64), 21, 10)
    want = check_confusion(dev(logits), target, 21)                           # 640 groups: three workgroups by default
    assert np.array_equal(check_confusion(dev(logits), target, 21, max_blocks=2), want)       # two workgroups stride over them
    assert np.array_equal(check_confusion(dev(logits), target, 21, max_blocks=1), want)
    # two calls into one matrix = the sum of two matrices; nothing is zeroed in between
    other = check_confusion(dev(gold["conf_logits"]), gold["conf_target"], 21)
    mat = labels.confusion(dev(logits), dev(target), 21)
    again = labels.confusion(dev(gold["conf_logits"]), dev(gold["conf_target"]), 21, mat=mat)
    assert again is mat and same(mat, want + other)


def test_confusion_equals_the_references_calculate_mat(gold):
    mat = labels.confusion(dev(gold["conf_logits"]), dev(gold["conf_target"]), 21)
    assert same(mat, gold["conf_mat"])
    assert np.array_equal(labels.compute_iou(mat.cpu().numpy()), gold["conf_iou"], equal_nan=True)


# ---- resize_nearest, window, colorize --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(NEAREST_CASES)))
@pytest.mark.parametrize("channels", [1, 3])
def test_resize_nearest_equals_pillow(gold, case, channels):
    h, w, oh, ow = NEAREST_CASES[case]
    src, want = gold[f"nearest{case}_c{channels}_in"], gold[f"nearest{case}_c{channels}_out"]
    assert same(labels.resize_nearest(src, (oh, ow)), want)
    assert same(labels.resize_nearest(dev(src), (oh, ow)), labels.resize_nearest_reference(src, (oh, ow)))
    src3 = dev(src.reshape(h, w, channels))
    for offset in (64, 61):
        buf, dst = guarded((oh, ow, channels), offset)
        ops.launch(ops.make_label_resize_nearest(src=src3, dst=dst, y_idx=dev(labels.nearest_index(h, oh)), x_idx=dev(labels.nearest_index(w, ow))))
        assert same(dst, want.reshape(oh, ow, channels)) and guards_ok(buf, dst.shape, offset)


def test_resize_nearest_forces_a_wrong_table_inside_the_source():
    src = np.arange(12, dtype=np.uint8).reshape(3, 4)
    dst = torch.empty((2, 4, 1), dtype=torch.uint8, device=DEV)
    ops.launch(ops.make_label_resize_nearest(src=dev(src[:, :, None]), dst=dst, y_idx=dev(np.array([-5, 99], np.int32)),
                                             x_idx=dev(np.array([0, 1, 7, -1], np.int32))))
    assert same(dst[:, :, 0], src[[0, 2]][:, [0, 1, 3, 0]])


# (source extent, window extent, origin, hflip, vflip)
WINDOWS = [((5, 7), (9, 12), (0, 0), False, False),            # pad only
           ((9, 13), (4, 8), (3, 5), False, False),            # crop only, at an odd origin
           ((6, 10), (8, 8), (1, 3), False, False),            # pad and crop
           ((6, 10), (8, 8), (1, 3), True, False),
           ((6, 10), (8, 8), (1, 3), False, True),
           ((6, 10), (8, 8), (1, 3), True, True),
           ((6, 10), (5, 7), (2, 1), True, False),             # W not a multiple of 4
           ((3, 3), (1, 1), (1, 2), False, False),             # 1 x 1
           ((4, 4), (3, 8), (-10, 40), True, True),            # the whole window outside the source: all fill
           ((4, 6), (6, 8), (-1, -2), False, False)]           # rows and columns before the source


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("fill", [0, 255])
def test_window_pad_crop_flip(channels, fill):
    rng = np.random.default_rng(12)
    for (hw, out_hw, origin, hf, vf) in WINDOWS:
        x = rng.integers(1, 255, size=hw + (channels,), dtype=np.uint8)
        want = labels.window_reference(x, out_hw, origin, hf, vf, fill)
        assert same(labels.window(x, out_hw, origin, hf, vf, fill), want, str((hw, out_hw, origin, hf, vf)))
        if channels == 1:
            assert same(labels.window(dev(x[:, :, 0]), out_hw, origin, hf, vf, fill), want[:, :, 0])
        for offset in (64, 61):
            buf, dst = guarded(out_hw + (channels,), offset)
            ops.launch(ops.make_label_window(src=dev(x), dst=dst, y0=origin[0], x0=origin[1], hflip=hf, vflip=vf, fill=fill))
            assert same(dst, want) and guards_ok(buf, dst.shape, offset)
    assert (labels.window_reference(x, (3, 8), (-10, 40), True, True, fill) == fill).all()


def test_colorize(gold):
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    small = np.array([[0, 1, 20, 21, 255], [7, 7, 7, 200, 3], [15, 0, 255, 255, 19]], dtype=np.uint8)
    batch = np.stack([small, small[::-1], small[:, ::-1]])
    for pal in (None, gold["ref_palette"], gold["ref_palette"][:21]):
        for lab in (every, small, batch):
            want = labels.colorize_reference(lab, pal)
            assert same(labels.colorize(lab, pal), want)
            for offset in (64, 61):
                buf, dst = guarded(lab.shape + (3,), offset)
                src = dev(lab if lab.ndim == 3 else lab[None])
                ops.launch(ops.make_label_colorize(labels=src, palette=dev(labels._palette(pal)), dst=dst))
                assert same(dst, want) and guards_ok(buf, dst.shape, offset)
    assert same(labels.colorize(gold["color_labels"], gold["ref_palette"]), gold["color_out"])         # convert2color -> save_image
    assert same(labels.colorize(every)[15, 15], np.array([224, 224, 192], dtype=np.uint8))
    odd = torch.zeros(16, dtype=torch.uint8, device=DEV)[1:].view(3, 5)                                  # labels one byte off a dword
    odd.copy_(dev(small))
    assert same(labels.colorize(odd), labels.colorize_reference(small))


# ---- the data sets' geometry and the test loop's tail ----------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size,crop_type", [(24, "center"), (12, "center"), (12, "random"), (24, "none")])
def test_prepare_pair_equals_the_restatement(out_size, crop_type):
    rng = np.random.default_rng(14)
    img = rng.integers(0, 256, size=(37, 23, 3), dtype=np.uint8)
    mask = rng.integers(0, 21, size=(37, 23), dtype=np.uint8)
    cfg = labels.SegGeometry(16, None, out_size, crop_type, True)
    seen = set()
    for k in range(6):
        geom = labels.draw_geometry(cfg, 4, k, (37, 23))
        assert geom.size == (25, 16)
        seen.add(geom.hflip)
        gt, m = labels.prepare_pair(img, mask, geom)
        want_gt, want_m = labels.prepare_pair_reference(img, mask, geom)
        assert gt.is_cuda and tuple(gt.shape) == geom.out_hw + (3,) and tuple(m.shape) == geom.out_hw
        assert same(gt, want_gt) and same(m, want_m)
        # against plain numpy slicing of the resized arrays
        from edtr_amd import imageio
        big = np.pad(imageio.resize_u8_reference(img, 16, 25), ((0, geom.pad[0]), (0, geom.pad[1]), (0, 0)))
        bigm = np.pad(labels.resize_nearest_reference(mask, (25, 16)), ((0, geom.pad[0]), (0, geom.pad[1])), constant_values=255)
        (y0, x0), (H, W) = geom.origin, geom.out_hw
        cut, cutm = big[y0:y0 + H, x0:x0 + W], bigm[y0:y0 + H, x0:x0 + W]
        assert same(gt, cut[:, ::-1] if geom.hflip else cut) and same(m, cutm[:, ::-1] if geom.hflip else cutm)
    assert seen == {False, True}


def test_paired_mask():
    mask = np.random.default_rng(15).integers(0, 21, size=(37, 23), dtype=np.uint8)
    assert same(labels.paired_mask(mask, (40, 30)), labels.resize_nearest_reference(mask, (40, 30)))
    assert same(labels.paired_mask(mask, (40, 30), center_crop=24), labels.resize_nearest_reference(mask, (40, 30))[8:32, 3:27])
    assert same(labels.paired_mask(mask, (40, 30), center_crop=24), labels.paired_mask_reference(mask, (40, 30), 24))
    with pytest.raises(ValueError):
        labels.paired_mask(mask, (20, 30), center_crop=24)


def test_evaluate_accumulates_over_images_of_different_extents(gold):
    weight = torch.randn((21, 3), generator=torch.Generator().manual_seed(21)).to(DEV)
    seen = []

    def segnet(x):          # a fixed 1 x 1 convolution, returned the way torchvision's segmentation models return logits
        assert x.ndim == 4 and x.shape[:2] == (1, 3) and x.dtype == torch.float32
        out = (weight[None, :, :, None, None] * x[:, None]).sum(2)
        seen.append(out)
        return {"out": out}

    rng = np.random.default_rng(16)
    extents = [(9, 12), (16, 8), (5, 7)]
    images = [dev(rng.random((3, h, w), dtype=np.float32)) for h, w in extents]
    masks = [targets((h, w), 21, 30 + i) for i, (h, w) in enumerate(extents)]
    res = labels.evaluate(images, [dev(m) for m in masks], segnet, return_preds=True, palette=gold["ref_palette"])
    assert len(seen) == 3
    want = np.zeros((21, 21), dtype=np.int64)
    for logits, m, pred, color in zip(seen, masks, res["preds"], res["colors"]):
        mat, p = labels.confusion_reference(logits.cpu().numpy(), m[None], 21, return_pred=True)
        want += mat
        assert same(pred, p[0]) and same(color, labels.colorize_reference(p[0], gold["ref_palette"]))
    assert isinstance(res["mat"], np.ndarray) and same(res["mat"], want)
    assert np.array_equal(res["iou"], labels.compute_iou(want), equal_nan=True)
    assert res["miou"] == labels.mean_iou(want) or (np.isnan(res["miou"]) and np.isnan(labels.mean_iou(want)))
    plain = labels.evaluate([im[None] for im in images], masks, lambda x: (weight[None, :, :, None, None] * x[:, None]).sum(2))
    assert set(plain) == {"mat", "iou", "miou"} and same(plain["mat"], want)
