"""edtr_seg_confusion_coarse on the device (csrc/labels.hip) against its numpy restatement `labels.coarse_confusion_reference`, by
EQUALITY of the matrix and of the label map.  A tile of the launch is 16 x 64 output pixels and its coarse patch is staged in LDS
while npad * rows * columns of it (npad: n rounded up to 4) fit 4096 floats, so the shapes are the smallest that reach: every index clamped, the dword and the
byte-by-byte form of the rows, up- and down-scaling at integer and non-integer ratios, both ways of reading the taps, several tiles
along each axis with ragged last ones, a grid that has to stride, and outputs inside guarded buffers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from edtr_amd import degrade, labels, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GUARD = 0xA5
NAMES = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
# (ih, iw) -> (H, W)
SHAPES = [((1, 1), (5, 7)),             # every index clamps
          ((2, 3), (16, 24)),           # integer x 8, W % 4 == 0
          ((7, 5), (50, 37)),           # non-integer ratio, unaligned rows, four tiles down
          ((9, 9), (4, 5)),             # down-scale
          ((40, 40), (8, 8)),           # a 37 x 37 patch: its taps come from memory at every n
          ((12, 12), (8, 8)),           # a 12 x 12 patch: staged up to n = 28 (down-scaling from LDS), from memory at n = 32
          ((9, 13), (37, 150)),         # 3 x 3 tiles, ragged last ones (5 rows, 22 columns), rows byte by byte
          ((9, 13), (40, 136))]         # 3 x 3 tiles, ragged last ones (8 rows, 8 columns), rows as dwords


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "coarse.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what=""):
    """bit equality of two arrays (device tensors are copied); what differs is printed before the assertion"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    if bad.any():
        first = tuple(np.argwhere(bad)[0])
        print(f"\n[{what}] {int(bad.sum())} of {bad.size} elements differ, first at {first}: {got[first]} for {want[first]}")
    return not bad.any()


def targets(shape, n, seed):
    """uint8 targets that hold every class below ``n``, the ignore label, n itself and 200 (all three are ignored)"""
    t = np.random.default_rng(seed).integers(0, n, size=shape).astype(np.uint8)
    flat = t.reshape(-1)
    k = min(n, flat.size)
    flat[:k] = np.arange(k)
    flat[k:k + 3] = (255, n, 200)[:max(0, min(3, flat.size - k))]
    return t


def logits_for(shape, seed, dtype=torch.float32, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def check(coarse_t, target, n, sizes=None, max_blocks=0, what=""):
    """mat and pred of one launch against the restatement on the values the device holds; returns (mat, pred) of the restatement"""
    coarse_t = coarse_t.to(DEV)
    host = coarse_t.float().cpu().numpy()             # (16-bit logits widen exactly)
    want_mat, want_pred = labels.coarse_confusion_reference(host, target, n=n, sizes=sizes, return_pred=True, dtype=NAMES[coarse_t.dtype])
    mat, pred = labels.coarse_confusion(coarse_t, dev(target), n, sizes=sizes, return_pred=True, max_blocks=max_blocks)
    assert mat.dtype == torch.int64 and same(mat, want_mat, what + " mat")
    assert same(pred, want_pred, what + " pred")                # every pixel, ignored ones and those outside sizes included
    alone = labels.coarse_confusion(coarse_t, dev(target), n, sizes=sizes, max_blocks=max_blocks)             # the form without pred
    assert same(alone, want_mat, what + " mat without pred")
    return want_mat, want_pred


# ---- shapes, classes, batch, types -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SHAPES)))
@pytest.mark.parametrize("B", [1, 3])
def test_shapes_at_21_classes(case, B):
    (ih, iw), (H, W) = SHAPES[case]
    check(logits_for((B, 21, ih, iw), 10 + case), targets((B, H, W), 21, 20 + case), 21, what=str(SHAPES[case]))


@pytest.mark.parametrize("n", [1, 2, 32])
def test_class_counts_on_both_tap_paths(n):
    for case in (2, 4, 5, 7):           # at (12, 12) -> (8, 8), n = 1 and 2 stage the patch that n = 32 reads from memory
        (ih, iw), (H, W) = SHAPES[case]
        coarse = torch.round(logits_for((2, n, ih, iw), 30 + n) * 2) / 2               # coarse values: many ties
        check(coarse, targets((2, H, W), n, 40 + n), n, what=f"n = {n} {SHAPES[case]}")


def test_more_than_32_classes_and_the_other_refusals():
    t = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    mat = torch.full((33, 33), 7, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="-5"):           # EDTR_E_UNSUPPORTED, nothing launched: mat is as it was
        labels.coarse_confusion(torch.zeros((1, 33, 2, 2), device=DEV), t, 33, mat=mat)
    assert bool((mat == 7).all())
    coarse = torch.zeros((1, 21, 2, 2), device=DEV)
    with pytest.raises(ValueError):
        labels.coarse_confusion(torch.zeros((1, 33, 2, 2), device=DEV), t, 21)
    with pytest.raises(RuntimeError, match="-2"):           # a sizes entry outside the slot
        labels.coarse_confusion(coarse, t, 21, sizes=[(9, 8)])
    with pytest.raises(ValueError):
        labels.coarse_confusion(coarse, t, 21, sizes=[(8, 8), (8, 8)])
    with pytest.raises(ValueError):                         # a batch of two targets for one image, an int32 target
        labels.coarse_confusion(coarse, torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV), 21)
    with pytest.raises(ValueError):
        labels.coarse_confusion(coarse, t.int(), 21)
    with pytest.raises(TypeError):                          # mat of another type, logits that are a view
        labels.coarse_confusion(coarse, t, 21, mat=torch.zeros((21, 21), dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        labels.coarse_confusion(torch.zeros((1, 21, 2, 4), device=DEV)[:, :, :, ::2], t, 21)
    with pytest.raises(TypeError):
        labels.coarse_confusion(torch.zeros((1, 21, 2, 2), dtype=torch.float64, device=DEV), t, 21)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", [1, 2, 4, 5, 6])
def test_16_bit_logits(dtype, case):
    (ih, iw), (H, W) = SHAPES[case]
    coarse = logits_for((2, 21, ih, iw), 50 + case, dtype, 3.0)
    coarse[:, 7] = coarse[:, 3]                      # a tie wherever plane 3 holds the maximum
    check(coarse, targets((2, H, W), 21, 60 + case), 21, what=f"{dtype} {SHAPES[case]}")
    buf = torch.zeros(coarse.numel() + 1, dtype=dtype, device=DEV)          # a base 2 bytes off a dword
    view = buf[1:].view(coarse.shape)
    view.copy_(coarse)
    assert view.data_ptr() % 4 == 2
    check(view, targets((2, H, W), 21, 60 + case), 21, what=f"{dtype} {SHAPES[case]} at an odd element")


def test_bf16_rounding_creates_ties():
    """two planes whose fp32 blends differ by less than a bf16 step: only the rounding of the blend to bf16 makes them equal, and
    the lower plane must then win where the higher one leads in fp32"""
    coarse = logits_for((1, 4, 5, 6), 70, torch.bfloat16, 0.25) - 4.0
    coarse[:, 2] = coarse[:, 1].roll(1, 2)
    coarse[:, 3] = 3.0
    coarse[:, 0] = coarse[:, 3] + logits_for((1, 5, 6), 71, torch.bfloat16, 0.0078125)            # within half a step of 3 (a step is 2^-6)
    host = coarse.float().numpy()
    exact = labels.upsample_logits_reference(host, (37, 51))
    held = labels.upsample_logits_reference(host, (37, 51), "bfloat16")
    flips = (labels.argmax_reference(exact) == 3) & (labels.argmax_reference(held) == 0)
    assert flips.mean() > 0.05, "the case needs pixels where plane 3 leads in fp32 and ties with plane 0 in bf16"
    _, pred = check(coarse, targets((1, 37, 51), 4, 72), 4, what="bf16 ties")
    assert (pred[flips] == 0).all()


# ---- values ----------------------------------------------------------------------------------------------------------------------------
def test_nan_inf_and_signed_zero_in_the_coarse_logits():
    nan, inf = float("nan"), float("inf")
    coarse = logits_for((2, 21, 6, 7), 80)
    coarse[0, 8, 2, 3] = nan                    # spreads over the pixels whose taps touch it; a NaN beats every number
    coarse[0, 4, 2, 3] = 100.0
    coarse[0, 5, 4, 1] = inf                    # inf under a zero weight is a NaN too (0 * inf), as in ATen
    coarse[0, 12, 4, 1] = inf
    coarse[1, 3, 1, 5] = -inf
    coarse[1, :, 3:, :] = -1.0
    coarse[1, 6, 3:, :] = -0.0                  # -0.0 against 0.0 is a tie: the lower plane
    coarse[1, 9, 3:, :] = 0.0
    for size in ((29, 45), (6, 7), (3, 4)):
        _, pred = check(coarse, targets((2,) + size, 21, 81), 21, what=f"special values at {size}")
    up = labels.upsample_logits_reference(coarse.numpy(), (29, 45))
    assert np.isnan(up).any() and np.isinf(up).any()
    _, pred = check(coarse, targets((2, 29, 45), 21, 81), 21)
    assert (pred[1, 22:] == 6).all() and (pred[0][np.isnan(up[0, 8]) & ~np.isnan(up[0, :8]).any(0)] == 8).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_constant_planes_are_all_ties(dtype):
    coarse = torch.full((2, 21, 5, 9), 0.3).to(dtype)
    target = targets((2, 33, 70), 21, 90)
    mat, pred = check(coarse, target, 21)
    assert (pred == 0).all() and mat[:, 1:].sum() == 0 and mat.sum() == (target < 21).sum()


# ---- behaviour -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [6, 7])
def test_sizes_smaller_than_the_slot_still_write_every_label(case):
    (ih, iw), (H, W) = SHAPES[case]
    coarse = logits_for((3, 21, ih, iw), 100)
    target = targets((3, H, W), 21, 101)
    for sizes in ([(1, 1), (H, W), (H - 3, W - 5)], [(H, 2), (17, W), (16, 64)]):
        mat, pred = check(coarse, target, 21, sizes=sizes)
        assert np.array_equal(pred, labels.argmax_reference(labels.upsample_logits_reference(coarse.numpy(), (H, W))))
        counted = target < 21
        for b, (h, w) in enumerate(sizes):
            counted[b, h:, :] = False
            counted[b, :, w:] = False
        assert int(mat.sum()) == int(counted.sum())


def test_ignored_targets():
    coarse = logits_for((1, 5, 4, 6), 110)
    target = np.random.default_rng(111).integers(0, 256, size=(1, 30, 44)).astype(np.uint8)         # most values lie in [5, 255]
    assert ((target >= 5) & (target < 255)).any() and (target == 255).any() and (target < 5).any()
    mat, _ = check(coarse, target, 5)
    assert int(mat.sum()) == int((target < 5).sum())
    check(coarse, np.full((1, 30, 44), 255, np.uint8), 5)


def test_capped_grid_strides_and_two_calls_add_up(gold):
    coarse = torch.round(logits_for((2, 21, 9, 13), 120) * 4) / 4
    target = targets((2, 40, 136), 21, 121)                  # 18 tiles
    want, _ = check(coarse, target, 21)
    for cap in (1, 2, 5):
        assert np.array_equal(check(coarse, target, 21, max_blocks=cap)[0], want)
    other, _ = check(torch.from_numpy(gold["a0_coarse"]), gold["a0_target"], 21)
    mat = labels.coarse_confusion(coarse.to(DEV), dev(target), 21)
    again = labels.coarse_confusion(dev(gold["a0_coarse"]), dev(gold["a0_target"]), 21, mat=mat)       # nothing is zeroed in between
    assert again is mat and same(mat, want + other)


def test_guarded_outputs_and_a_target_off_a_dword():
    """pred at an aligned and at an odd offset of a guarded buffer, the target one byte into its buffer: the same words through the
    byte-by-byte form, and the guards untouched"""
    (ih, iw), (H, W) = SHAPES[7]
    coarse = logits_for((2, 21, ih, iw), 130).to(DEV)
    target = targets((2, H, W), 21, 131)
    want_mat, want_pred = labels.coarse_confusion_reference(coarse.cpu().numpy(), target, return_pred=True)
    tbuf = torch.zeros(target.size + 1, dtype=torch.uint8, device=DEV)
    tview = tbuf[1:].view(target.shape)
    tview.copy_(dev(target))
    n = target.size
    for tgt in (dev(target), tview):
        for offset in (64, 61):
            buf = torch.full((offset + n + 67,), GUARD, dtype=torch.uint8, device=DEV)
            pred = buf[offset:offset + n].view(target.shape)
            mat = torch.zeros((21, 21), dtype=torch.int64, device=DEV)
            ops.launch(ops.make_seg_confusion_coarse(coarse=coarse, target=tgt, mat=mat, pred=pred))
            assert same(mat, want_mat) and same(pred, want_pred)
            assert bool((buf[:offset] == GUARD).all()) and bool((buf[offset + n:] == GUARD).all())


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_the_wrapper_does_not_wait_for_the_device():
    coarse = logits_for((3, 21, 9, 13), 140).to(DEV)
    target = targets((3, 40, 136), 21, 141)
    tgt = dev(target)
    mat = torch.zeros((21, 21), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")         # a synchronising call inside the block raises
    try:
        labels.coarse_confusion(coarse, tgt, 21, mat=mat)
        _, pred = labels.coarse_confusion(coarse, tgt, 21, sizes=[(40, 136), (7, 9), (16, 64)], mat=mat, return_pred=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    host = coarse.cpu().numpy()
    want = labels.coarse_confusion_reference(host, target) + labels.coarse_confusion_reference(host, target, sizes=[(40, 136), (7, 9), (16, 64)])
    assert same(mat, want) and same(pred, labels.argmax_reference(labels.upsample_logits_reference(host, (40, 136))))


# ---- the reference's answer, the parent path, the neighbours ---------------------------------------------------------------------------
def test_set_a_equals_the_references_matrices_and_the_full_logits_path(gold):
    for i, (ih, iw, H, W) in enumerate(gold["a_cases"]):
        coarse, target = dev(gold[f"a{i}_coarse"]), dev(gold[f"a{i}_target"])
        mat, pred = labels.coarse_confusion(coarse, target, 21, return_pred=True)
        assert same(mat, gold[f"a{i}_mat"]) and same(pred, gold[f"a{i}_pred"])            # torch on the CPU -> the reference's calculate_mat
        full = F.interpolate(coarse, size=(int(H), int(W)), mode="bilinear", align_corners=False)
        fmat, fpred = labels.confusion(full, target, 21, return_pred=True)                # what this launch replaces
        assert same(fmat, mat) and same(fpred, pred)


def test_tie_prone_set_equals_the_restatement(gold):
    check(torch.from_numpy(gold["b_coarse"]), gold["b_target"], 21, what="set (b)")


@pytest.mark.parametrize("ihw,size", [((5, 7), (37, 51)), ((33, 33), (257, 260)), ((40, 40), (8, 8)), ((9, 13), (9, 13))])
def test_degrade_resize_keeps_its_bits(ihw, size):
    x = np.random.default_rng(150).standard_normal((2, 3) + ihw).astype(np.float32)
    got = degrade.resize(dev(x), size, "bilinear").cpu().numpy()
    assert np.array_equal(got.view(np.uint32), degrade.resize_reference(x, size, "bilinear").view(np.uint32))
    assert np.array_equal(got.view(np.uint32), labels.upsample_logits_reference(x, size).view(np.uint32))


def test_assemble_segmenter_and_evaluate_on_the_device():
    """a strided convolution and a 1 x 1 convolution as the learned parts: `evaluate` scores the `CoarseLogits` in one launch per image,
    and the matrix is the restatement's on the logits the modules returned"""
    torch.manual_seed(3)
    backbone = torch.nn.Conv2d(3, 8, 3, stride=4, padding=1).to(DEV)
    classifier = torch.nn.Conv2d(8, 21, 1).to(DEV)
    seen = []

    def keep(x):
        out = classifier(x)
        seen.append(out)
        return out

    segnet = labels.assemble_segmenter(lambda x: {"C5": backbone(x)}, keep)
    rng = np.random.default_rng(160)
    extents = [(33, 70), (18, 27)]
    images = [dev(rng.random((3, h, w), dtype=np.float32)) for h, w in extents]
    masks = [targets(hw, 21, 161 + i) for i, hw in enumerate(extents)]
    res = labels.evaluate(images, [dev(m) for m in masks], segnet, return_preds=True)
    want = np.zeros((21, 21), dtype=np.int64)
    for logits, m, pred in zip(seen, masks, res["preds"]):
        assert tuple(logits.shape[2:]) != m.shape
        mat, p = labels.coarse_confusion_reference(logits.cpu().numpy(), m[None], return_pred=True)
        want += mat
        assert same(pred, p[0])
    assert same(res["mat"], want)
    assert res["miou"] == labels.mean_iou(want) or (np.isnan(res["miou"]) and np.isnan(labels.mean_iou(want)))
