"""Scoring segmentation from coarse logits, on the host: the numpy restatements of edtr_seg_confusion_coarse (edtr_amd/labels.py:
`upsample_logits_reference`, `coarse_confusion_reference`) against `degrade.resize_reference` and against plain torch on the CPU
(tests/golden/coarse.npz, written by tools/make_coarse_goldens.py with the reference's own `calculate_mat`), the entry point's
declaration and its argument checks, and `assemble_segmenter` / `evaluate` with stub modules.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from edtr_amd import cls, degrade, labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DIFFERING = 1e-3        # share of the pixels whose label may differ from torch's on the tie-prone and the 16-bit inputs


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "coarse.npz"))


def torch_labels(coarse_t, size):
    with torch.no_grad():
        return F.interpolate(coarse_t, size=size, mode="bilinear", align_corners=False).argmax(1).to(torch.uint8).numpy()


def blend_fp64(coarse, size):
    """the bilinear rule in exact terms, evaluated in fp64: [B, n, H, W]"""
    x = np.asarray(coarse, dtype=np.float64)

    def axis(n_in, n_out):
        src = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), np.clip(src - i0, 0.0, 1.0)

    (y0, y1, ty), (x0, x1, tx) = axis(x.shape[2], size[0]), axis(x.shape[3], size[1])
    ty = ty[:, None]
    top = (1 - tx) * x[:, :, y0][:, :, :, x0] + tx * x[:, :, y0][:, :, :, x1]
    bot = (1 - tx) * x[:, :, y1][:, :, :, x0] + tx * x[:, :, y1][:, :, :, x1]
    return (1 - ty) * top + ty * bot


def assert_labels_meet_torch(ours, theirs, coarse, size, d, what):
    """at most MAX_DIFFERING of the labels differ, and only where the two best planes lie within 2 d of each other under the fp64
    blend (each plane's value may move by d between the two evaluations)"""
    differ = ours != theirs
    share = differ.mean()
    top2 = np.sort(blend_fp64(coarse, size), axis=1)[:, -2:]
    gap = (top2[:, 1] - top2[:, 0])[differ]
    print(f"\n[{what}] {int(differ.sum())} of {differ.size} labels differ ({share:.2e}); d = {d:.3e}, largest gap of the two best planes "
          f"at a differing pixel {gap.max() if gap.size else 0.0:.3e}")
    assert share <= MAX_DIFFERING
    assert (gap <= 2 * d).all()


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ihw,size", [((5, 7), (37, 51)), ((8, 8), (64, 64)), ((9, 13), (4, 5)), ((1, 1), (5, 7)), ((33, 33), (257, 260)),
                                      ((40, 40), (8, 8)), ((6, 10), (6, 10))])
def test_upsample_logits_reference_is_resize_reference_on_three_planes(ihw, size):
    x = np.random.default_rng(1).standard_normal((2, 3) + ihw).astype(np.float32)
    got = labels.upsample_logits_reference(x, size)
    want = degrade.resize_reference(x, size, "bilinear")
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_set_a_gives_the_golden_matrices_and_label_maps(gold):
    for i, (ih, iw, H, W) in enumerate(gold["a_cases"]):
        coarse, target = gold[f"a{i}_coarse"], gold[f"a{i}_target"]
        assert coarse.shape == (2, 21, ih, iw) and target.shape == (2, H, W)
        mat, pred = labels.coarse_confusion_reference(coarse, target, return_pred=True)
        assert mat.dtype == np.int64 and np.array_equal(mat, gold[f"a{i}_mat"])
        assert pred.dtype == np.uint8 and np.array_equal(pred, gold[f"a{i}_pred"])
        assert np.array_equal(labels.coarse_confusion_reference(coarse, target, size=(H, W), n=21), gold[f"a{i}_mat"])
        assert np.array_equal(torch_labels(torch.from_numpy(coarse), (H, W)), gold[f"a{i}_pred"])           # torch alone: zero differing pixels


def test_tie_prone_set_meets_torch_at_the_level_of_labels(gold):
    coarse, target, d = gold["b_coarse"], gold["b_target"], float(gold["b_d"])
    size = tuple(int(v) for v in gold["tie_case"][2:])
    assert np.array_equal(coarse, np.round(coarse * 2) / 2) and 0 < d < 1e-4
    up = labels.upsample_logits_reference(coarse, size)
    top2 = np.sort(up, axis=1)[:, -2:]
    assert (top2[:, 0] == top2[:, 1]).mean() > 0.01, "the tie-prone set needs ties among its maxima"
    mat, pred = labels.coarse_confusion_reference(coarse, target, return_pred=True)
    assert int(mat.sum()) == int((target < 21).sum())
    assert_labels_meet_torch(pred, gold["b_pred"], coarse, size, d, "set (b) against the recorded labels")
    assert_labels_meet_torch(pred, torch_labels(torch.from_numpy(coarse), size), coarse, size, d, "set (b) against this torch")


@pytest.mark.parametrize("key,dtype,tdtype", [("h", "float16", torch.float16), ("bf", "bfloat16", torch.bfloat16)])
def test_16_bit_logits_meet_torch_at_the_level_of_labels(gold, key, dtype, tdtype):
    held, d = gold[f"{key}_coarse"], float(gold[f"{key}_d"])
    size = tuple(int(v) for v in gold["tie_case"][2:])
    assert held.dtype == (np.float16 if dtype == "float16" else np.float32)
    up = labels.upsample_logits_reference(held, size, dtype)
    assert up.dtype == np.float32 and np.array_equal(labels._round_to(up, dtype), up)              # every value is one of the type
    assert not np.array_equal(up, labels.upsample_logits_reference(held.astype(np.float32), size))  # (the rounding is not a no-op)
    pred = labels.argmax_reference(up)
    widened = held.astype(np.float32)
    assert_labels_meet_torch(pred, gold[f"{key}_pred"], widened, size, d, f"{dtype} against the recorded labels")
    assert_labels_meet_torch(pred, torch_labels(torch.from_numpy(widened).to(tdtype), size), widened, size, d, f"{dtype} against this torch")
    mat, again = labels.coarse_confusion_reference(held, gold["h_target"], return_pred=True, dtype=dtype)
    assert np.array_equal(again, pred) and np.array_equal(mat, labels.confusion_reference(up, gold["h_target"]))


def test_round_to_is_round_to_nearest_even():
    v = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895314e38, np.inf, -np.inf, np.nan, 65520.0, 0.0, -0.0], dtype=np.float32)
    bf = labels._round_to(v, "bfloat16")
    want = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    assert np.array_equal(bf, want, equal_nan=True) and np.signbit(bf[-1])
    assert bf[1] == 1.0 and bf[2] == np.float32(1.015625)              # ties go to the even neighbour, both ways
    h = labels._round_to(v, "float16")
    assert np.array_equal(h, torch.from_numpy(v).to(torch.float16).float().numpy(), equal_nan=True) and np.isinf(h[8])
    assert labels._round_to(v, "float32") is v


def test_reference_argument_errors():
    x = np.zeros((1, 21, 4, 4), np.float32)
    with pytest.raises(ValueError):
        labels.upsample_logits_reference(x, (8, 8), "float64")
    with pytest.raises(ValueError):
        labels.upsample_logits_reference(x[0], (8, 8))
    with pytest.raises(ValueError):
        labels.upsample_logits_reference(x.astype(np.float64), (8, 8))
    with pytest.raises(ValueError):
        labels.upsample_logits_reference(x, (0, 8))
    with pytest.raises(ValueError):                                     # 1 + 2^-12 is no bf16 value
        labels.upsample_logits_reference(x + np.float32(1.000244140625), (8, 8), "bfloat16")
    with pytest.raises(ValueError):
        labels.coarse_confusion_reference(x, np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError):                                     # the target's extent and `size` disagree
        labels.coarse_confusion_reference(x, np.zeros((1, 8, 8), np.uint8), size=(8, 9))
    with pytest.raises(ValueError):
        labels.coarse_confusion_reference(x, np.zeros((1, 8, 8), np.uint8), n=20)
    with pytest.raises(ValueError):
        labels.coarse_confusion_reference(x, np.zeros((1, 8, 8), np.uint8), sizes=[(9, 8)])


# ---- the C ABI's rules for the new entry point -----------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_bound():
    from edtr_amd import build, lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "edtr_hip.h")).read(), flags=re.S)
    assert "edtr_seg_confusion_coarse" in lib.DECLARED_SYMBOLS
    assert re.search(r"int edtr_seg_confusion_coarse\(int logits_dtype, const void\* coarse, int B, int n, int ih, int iw,\s*const uint8_t\* target, "
                     r"int H, int W,\s*const int32_t\* sizes_host, const int32_t\* sizes, int64_t\* mat, uint8_t\* pred, int max_blocks,\s*"
                     r"edtr_stream_t stream\);", text)
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == lib.ABI_VERSION == 10 and hasattr(handle, "edtr_seg_confusion_coarse")


def test_entry_point_rejects_bad_arguments_in_the_order_of_edtr_seg_confusion():
    """refused on the host before any launch (no device is touched): each call below breaks one rule, or two to show which is
    looked at first"""
    import ctypes
    from edtr_amd import build, lib
    build.build_library()
    f = lib.load().edtr_seg_confusion_coarse
    p = 4096            # a non-NULL, aligned stand-in: every call fails its checks before the pointer is used

    def call(dt=0, coarse=p, B=1, n=21, ih=2, iw=3, target=p, H=4, W=4, sizes_host=None, sizes=None, mat=p, pred=None, max_blocks=0):
        return f(dt, coarse, B, n, ih, iw, target, H, W, sizes_host, sizes, mat, pred, max_blocks, None)

    assert call(coarse=None) == -1 and call(target=None) == -1 and call(mat=None) == -1
    assert call(sizes_host=(ctypes.c_int32 * 2)(4, 4)) == -1 and call(sizes=p) == -1
    assert call(coarse=None, dt=3) == -1                    # NULL before the type
    assert call(dt=3) == -4 and call(dt=-1) == -4
    assert call(dt=3, n=0) == -4                            # the type before the shape
    for bad in (dict(B=0), dict(n=0), dict(ih=0), dict(iw=-1), dict(H=0), dict(W=0), dict(max_blocks=-1)):
        assert call(**bad) == -2, bad
    assert call(n=33) == -5 and call(n=33, H=0) == -2       # the shape before the class limit
    assert call(ih=(1 << 24) + 1) == -5 and call(W=(1 << 24) + 1) == -5
    for bad in ((5, 4), (4, 5), (0, 4), (4, -1)):
        assert call(sizes_host=(ctypes.c_int32 * 2)(*bad), sizes=p) == -2
    assert call(n=33, sizes_host=(ctypes.c_int32 * 2)(5, 4), sizes=p) == -5                 # the class limit before the sizes
    assert call(coarse=p + 2) == -3 and call(dt=1, coarse=p + 1) == -3 and call(mat=p + 4) == -3
    assert call(sizes_host=(ctypes.c_int32 * 2)(4, 4), sizes=p + 2) == -3
    assert call(coarse=p + 2, sizes_host=(ctypes.c_int32 * 2)(5, 4), sizes=p) == -2        # the sizes before the alignment


def test_wrapper_argument_errors():
    t = torch.zeros((1, 4, 4), dtype=torch.uint8)
    with pytest.raises(TypeError):                          # logits on the host: there is no path without the launch
        labels.coarse_confusion(torch.zeros((1, 21, 2, 2)), t, 21)
    with pytest.raises(TypeError):
        labels.coarse_confusion(np.zeros((1, 21, 2, 2), np.float32), t, 21)
    with pytest.raises(TypeError):
        labels.CoarseLogits(torch.zeros((21, 2, 2)), (4, 4))
    with pytest.raises(ValueError):
        labels.CoarseLogits(torch.zeros((1, 21, 2, 2)), (0, 4))
    assert labels.CoarseLogits(torch.zeros((1, 21, 2, 2)), [4, 6]).size == (4, 6)


# ---- assemble_segmenter and evaluate ---------------------------------------------------------------------------------------------------
class Backbone(torch.nn.Module):
    def __init__(self, calls, as_dict):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3, stride=4, padding=1)
        self.calls, self.as_dict = calls, as_dict

    def forward(self, x):
        self.calls.append(("backbone", x))
        y = self.conv(x)
        return {"C2": y * 0, "C5": y} if self.as_dict else y


class Classifier(torch.nn.Module):
    def __init__(self, calls):
        super().__init__()
        self.conv = torch.nn.Conv2d(8, 21, 1)
        self.calls = calls

    def forward(self, x):
        self.calls.append(("classifier", x))
        return self.conv(x)


@pytest.mark.parametrize("as_dict", [True, False])
def test_assemble_segmenter_runs_normalize_backbone_classifier_in_order(monkeypatch, as_dict):
    calls = []
    torch.manual_seed(0)
    backbone, classifier = Backbone(calls, as_dict), Classifier(calls)

    def normalize(x):
        calls.append(("normalize", x))
        return torch.from_numpy(cls.normalize_reference(x.numpy()))

    monkeypatch.setattr(cls, "normalize", normalize)
    x = torch.rand((1, 3, 18, 27))
    kept = x.clone()
    out = labels.assemble_segmenter(backbone, classifier)(x)
    assert [c[0] for c in calls] == ["normalize", "backbone", "classifier"]
    assert calls[0][1] is x and torch.equal(x, kept)
    assert isinstance(out, labels.CoarseLogits) and out.size == (18, 27) and tuple(out.logits.shape) == (1, 21, 5, 7)
    assert not out.logits.requires_grad
    with torch.no_grad():
        want = classifier.conv(backbone.conv(torch.from_numpy(cls.normalize_reference(x.numpy()))))
    assert torch.equal(out.logits, want)
    del calls[:]
    plain = labels.assemble_segmenter(backbone, classifier, normalize=False)(x)
    assert [c[0] for c in calls] == ["backbone", "classifier"] and calls[0][1] is x
    with torch.no_grad():
        assert torch.equal(plain.logits, classifier.conv(backbone.conv(x)))
    if as_dict:
        with pytest.raises(KeyError):
            labels.assemble_segmenter(backbone, classifier, feature="C4", normalize=False)(x)


def test_evaluate_routes_coarse_logits_and_leaves_full_logits_alone(monkeypatch):
    """with the two launches replaced by their restatements: `CoarseLogits` (plain or under "out") goes to coarse_confusion, a tensor to
    confusion, and the accumulated matrix is the sum of the restatements'"""
    routed = []

    def fake(name, reference):
        def launch(logits, target, n=21, sizes=None, mat=None, return_pred=False, max_blocks=0):
            routed.append(name)
            m, p = reference(logits.numpy(), target.numpy(), n=n, return_pred=True)
            mat += torch.from_numpy(m)
            return (mat, torch.from_numpy(p)) if return_pred else mat
        return launch

    monkeypatch.setattr(labels, "coarse_confusion", fake("coarse", labels.coarse_confusion_reference))
    monkeypatch.setattr(labels, "confusion", fake("full", labels.confusion_reference))
    rng = np.random.default_rng(5)
    weight = torch.from_numpy(rng.standard_normal((21, 3)).astype(np.float32))
    images = [torch.from_numpy(rng.random((3, h, w), dtype=np.float32)) for h, w in ((12, 16), (9, 7))]
    masks = [rng.integers(0, 21, size=tuple(im.shape[1:])).astype(np.uint8) for im in images]

    def full_logits(x):
        return (weight[None, :, :, None, None] * x[:, None]).sum(2)

    def coarse_net(x):
        return labels.CoarseLogits(full_logits(x)[:, :, ::3, ::3].contiguous(), tuple(x.shape[-2:]))

    res = labels.evaluate(images, masks, coarse_net)
    assert routed == ["coarse", "coarse"]
    want = sum(labels.coarse_confusion_reference(coarse_net(im[None]).logits.numpy(), m[None]) for im, m in zip(images, masks))
    assert np.array_equal(res["mat"], want) and res["miou"] == labels.mean_iou(want)
    del routed[:]
    assert np.array_equal(labels.evaluate(images, masks, lambda x: {"out": coarse_net(x), "aux": None})["mat"], want)
    assert routed == ["coarse", "coarse"]
    del routed[:]
    full = labels.evaluate(images, masks, lambda x: {"out": full_logits(x)})
    assert routed == ["full", "full"]
    assert np.array_equal(full["mat"], sum(labels.confusion_reference(full_logits(im[None]).numpy(), m[None]) for im, m in zip(images, masks)))
    with pytest.raises(ValueError, match="stand for"):       # coarse logits that stand for another extent than the mask's
        labels.evaluate(images[:1], masks[:1], lambda x: labels.CoarseLogits(coarse_net(x).logits, (12, 17)))
