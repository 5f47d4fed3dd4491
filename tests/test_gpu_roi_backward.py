"""RoIAlign's backward on the device (-m gpu): `rois.roi_align_backward` equals `rois.roi_align_backward_reference` bit for bit at the
cases of tests/roi_backward_cases.py, into NaN-filled destinations between guard bands; two calls agree; `rois.roi_align` is
differentiable where its features ask for it and unchanged where they do not; the entry point rejects by return code; and the
training detector assembled from a tiny torch model matches the host flow stage by stage."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import roi_backward_cases as RC
from swin_cases import bits, untouched, window

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _rois():
    from edtr_amd import rois
    return rois


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F32).view(np.uint32), np.ascontiguousarray(b, dtype=F32).view(np.uint32))


def reference(case, dtype="float32", grad=None):
    return _rois().roi_align_backward_reference(case["grad"] if grad is None else grad, case["shapes"], case["rois"], case["image_sizes"],
                                                case["P"], case["S"], case["canonical_scale"], case["canonical_level"], dtype=dtype)


def launch(case, dtype="float32", out=None, grad=None):
    return _rois().roi_align_backward(dev(case["grad"]) if grad is None else grad, case["shapes"], [dev(r) for r in case["rois"]],
                                      case["image_sizes"], case["P"], case["S"], case["canonical_scale"], case["canonical_level"],
                                      dtype=TORCH[dtype], out=out)


@pytest.fixture(scope="module")
def wanted():
    cache = {}

    def get(i, dtype):
        if (i, dtype) not in cache:
            cache[i, dtype] = reference(RC.CASES[i], dtype)
        return cache[i, dtype]
    return get


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=RC.CASE_IDS)
def test_backward_equals_the_restatement_bit_for_bit_inside_guards(i, dtype, wanted):
    case = RC.CASES[i]
    guarded = [window(N * C * H, W, TORCH[dtype], DEV, "nan", extra_rows=0) for N, C, H, W in case["shapes"]]
    out = [view.view(shape) for (_, view, _), shape in zip(guarded, case["shapes"])]
    got = launch(case, dtype, out=out)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    for l, (g, w, (buf, view, before)) in enumerate(zip(got, wanted(i, dtype), guarded)):
        assert not torch.isnan(g).any(), f"level {l}: {int(torch.isnan(g).sum())} words were never written"
        assert same_bits(host(g), w), f"level {l}: {int((host(g) != w).sum())} elements differ from the restatement"
        untouched(buf, before, torch.ones(view.shape, dtype=torch.bool))


def test_two_calls_give_equal_bits_and_fresh_buffers():
    case = RC.CASES[2]
    first, second = launch(case), launch(case)
    assert all(a.data_ptr() != b.data_ptr() and torch.equal(bits(a), bits(b)) for a, b in zip(first, second))


def test_no_rois_and_host_inputs():
    rois = _rois()
    case = RC.CASES[0]
    none = [torch.zeros((0, 4), device=DEV)] * 2
    out = rois.roi_align_backward(torch.zeros((0, 70, 7, 7), device=DEV), case["shapes"], none, case["image_sizes"], dtype=torch.bfloat16)
    assert [tuple(o.shape) for o in out] == [tuple(s) for s in case["shapes"]] and all(o.dtype == torch.bfloat16 and not o.any() for o in out)
    got = rois.roi_align_backward(case["grad"], case["shapes"], case["rois"], case["image_sizes"], 7, 2, case["canonical_scale"], case["canonical_level"])
    assert all(g.is_cuda and same_bits(host(g), w) for g, w in zip(got, reference(case)))
    with pytest.raises(ValueError):
        rois.roi_align_backward(torch.zeros((1, 2, 17, 17), device=DEV), [(1, 2, 8, 8)], [torch.zeros((1, 4), device=DEV)], [(32, 32)], 17, 1)
    with pytest.raises(TypeError):
        launch(case, out=[torch.empty(s, device=DEV).half() for s in case["shapes"]])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_roi_align_is_differentiable_where_asked_and_unchanged_where_not(dtype):
    rois = _rois()
    case = RC.CASES[2]
    rng = np.random.default_rng(11)
    feats = [dev(rng.standard_normal(s).astype(F32)).to(TORCH[dtype]) for s in case["shapes"]]
    boxes = [dev(r) for r in case["rois"]]
    args = (boxes, case["image_sizes"], case["P"], case["S"], case["canonical_scale"], case["canonical_level"])
    plain = rois.roi_align(OrderedDict((str(l), f) for l, f in enumerate(feats)), *args)
    assert plain.grad_fn is None and not plain.requires_grad
    assert same_bits(host(plain), rois.roi_align_reference([host(f) for f in feats], case["rois"], *args[1:]))

    leaves = [f.clone().requires_grad_() for f in feats]
    pooled = rois.roi_align(leaves, *args)
    assert pooled.grad_fn is not None and torch.equal(bits(pooled), bits(plain))
    g = dev(case["grad"])
    pooled.backward(g)
    for leaf, want, again in zip(leaves, reference(case, dtype), launch(case, dtype)):
        assert leaf.grad.dtype == TORCH[dtype] and same_bits(host(leaf.grad), want) and torch.equal(bits(leaf.grad), bits(again))

    with torch.no_grad():
        quiet = rois.roi_align(leaves, *args)
    assert quiet.grad_fn is None and torch.equal(bits(quiet), bits(plain))
    # one level asking is enough, and only it receives a gradient
    mixed = [feats[0].clone().requires_grad_(), feats[1].clone()]
    rois.roi_align(mixed, *args).backward(g)
    assert mixed[1].grad is None and same_bits(host(mixed[0].grad), reference(case, dtype)[0])
    # a non-contiguous incoming gradient is made contiguous first
    leaves2 = [f.clone().requires_grad_() for f in feats]
    (rois.roi_align(leaves2, *args).transpose(2, 3) * g.transpose(2, 3)).sum().backward()
    assert all(same_bits(host(a.grad), w) for a, w in zip(leaves2, reference(case, dtype)))
    with pytest.raises(ValueError):
        rois.roi_align([f.clone().requires_grad_() for f in feats], boxes, case["image_sizes"], 17, 1, case["canonical_scale"], case["canonical_level"])


def test_backward_rejects_bad_arguments_by_return_code():
    from edtr_amd import lib
    RC.check_rejections(lib.load())


# ---- the training detector ---------------------------------------------------------------------------------------------------------------
class RpnHead(torch.nn.Module):
    def __init__(self, C, A):
        super().__init__()
        self.conv, self.cls, self.box = torch.nn.Conv2d(C, C, 3, padding=1), torch.nn.Conv2d(C, A, 1), torch.nn.Conv2d(C, 4 * A, 1)

    def forward(self, feats):
        hidden = [torch.relu(self.conv(f)) for f in feats]
        return [self.cls(h) * 4 for h in hidden], [self.box(h) for h in hidden]


class Backbone(torch.nn.Module):
    """two convolutions, two levels of 8 channels at strides 4 and 8"""
    def __init__(self, C):
        super().__init__()
        self.c1, self.c2 = torch.nn.Conv2d(3, C, 4, stride=4), torch.nn.Conv2d(C, C, 2, stride=2)

    def forward(self, x):
        a = torch.tanh(self.c1(x))
        return OrderedDict([("0", a), ("1", torch.tanh(self.c2(a)))])


class Predictor(torch.nn.Module):
    def __init__(self, D, classes):
        super().__init__()
        self.cls, self.box = torch.nn.Linear(D, classes), torch.nn.Linear(D, 4 * classes)

    def forward(self, x):
        return self.cls(x) * 3, self.box(x)


KW = dict(sizes=((16,), (32,)), aspect_ratios=((0.5, 1.0, 2.0),) * 2, rpn_pre_nms_top_n=64, rpn_post_nms_top_n=64, rpn_batch_size_per_image=32,
          box_batch_size_per_image=32, box_positive_fraction=0.25, canonical_scale=40.0)
SLOTS = 32


def close_encoding(got, want, tol):
    """tests/test_gpu_targets.py's: dx, dy equal; dw, dh (through logf) finite in the same places and within the recorded tolerance"""
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    ok = np.isfinite(want[:, 2:])
    worst = float(np.abs(got[:, 2:][ok] - want[:, 2:][ok]).max()) if ok.any() else 0.0
    return (np.array_equal(got[:, :2], want[:, :2], equal_nan=True) and np.array_equal(np.isfinite(got[:, 2:]), ok) and worst <= float(tol)
            and np.array_equal(got[:, 2:][~ok], want[:, 2:][~ok], equal_nan=True))


@pytest.fixture(scope="module")
def detector(golden_dir):
    """the tiny model, one traced training step, the host flow replayed from it in fp64 and in fp32, and the gradients of that step"""
    import os
    from edtr_amd import detinput, rng
    rois = _rois()
    # the learned parts are torch's: its convolutions choose repeatable weight-gradient algorithms only when asked to
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    torch.manual_seed(3)
    C, A, classes = 8, 3, 4
    backbone, rpn_head = Backbone(C).to(DEV), RpnHead(C, A).to(DEV)
    box_head = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(C * 49, 16), torch.nn.ReLU()).to(DEV)
    predictor = Predictor(16, classes).to(DEV)
    modules = torch.nn.ModuleList([backbone, rpn_head, box_head, predictor])
    gen = np.random.default_rng(21)
    images = [dev(gen.random((3, h, w), dtype=F32)) for h, w in ((96, 128), (80, 112))]
    # three ground truths per image in the image's own coordinates; the last lies outside every anchor (the quirk `targets` reproduces)
    annots = [{"boxes": dev(np.array([[10, 12, 60, 70], [70, 30, 118, 64], [400, 400, 440, 450]], dtype=F32)), "labels": torch.tensor([1, 3, 2])},
              {"boxes": dev(np.array([[5, 8, 37, 30], [48, 20, 100, 75], [300, 500, 330, 560]], dtype=F32)), "labels": torch.tensor([2, 1, 3])}]
    transform = detinput.DetectorTransform(80, 128, detinput.IMAGENET_MEAN, detinput.IMAGENET_STD)
    features_fn = detinput.assemble_features(backbone, transform, grad=True)
    source = rng.NoiseSource(5, [11, 12])
    trace = {}
    step = rois.assemble_training_detector(features_fn, rpn_head, box_head, predictor, source, trace=trace, **KW)

    def grads_of(draw, tr=None):
        if tr is not None:
            trace.clear()
        modules.zero_grad(set_to_none=True)
        losses, features = step(images, annots, draw)
        sum(losses.values()).backward()
        return losses, features, {n: p.grad.clone() for n, p in modules.named_parameters()}

    losses, features, grads = grads_of(7)
    first = dict(trace)
    ref = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        ref[name + "_trace"] = {}
        ref[name], _ = rois.assemble_training_detector_reference(None, None, None, None, source, replay=first, trace=ref[name + "_trace"],
                                                                 loss_dtype=dt, **KW)(images, annots, 7)
    gold = np.load(os.path.join(golden_dir, "targets.npz"))
    yield dict(step=step, grads_of=grads_of, losses=losses, features=features, grads=grads, trace=first, ref=ref, modules=modules,
               images=images, annots=annots, source=source, parts=(features_fn, rpn_head, box_head, predictor),
               tol=(float(gold["tol_rpn_dwdh"]), float(gold["tol_roi_dwdh"])))
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before


def test_training_step_returns_the_four_losses_and_the_features(detector):
    rois = _rois()
    assert tuple(detector["losses"]) == rois.LOSS_NAMES == ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")
    assert all(v.ndim == 0 and v.grad_fn is not None and bool(torch.isfinite(v)) for v in detector["losses"].values())
    assert list(detector["features"]) == ["0", "1"] and [tuple(f.shape) for f in detector["features"].values()] == [(2, 8, 24, 32), (2, 8, 12, 16)]
    tr = detector["trace"]
    assert tr["batch_shape"] == (96, 128) and tr["image_sizes"] == [(80, 106), (80, 112)] and tr["original_sizes"] == [(96, 128), (80, 112)]
    assert {"selected", "cand_counts", "proposals", "rpn_targets", "roi_targets", "pooled", "objectness", "bbox_deltas", "class_logits",
            "box_regression", "features", "targets", "losses"} <= set(tr)
    assert tuple(tr["pooled"].shape) == (2 * SLOTS, 8, 7, 7) and tr["pooled"].grad_fn is not None
    with pytest.raises(TypeError):
        rois.assemble_training_detector(*detector["parts"], detector["source"], box_score_thresh=0.5)
    with pytest.raises(ValueError):
        rois.assemble_training_detector(*detector["parts"], None)


def test_both_targets_match_the_host_flow_word_for_word_and_pooled_bit_for_bit(detector):
    """every integer, mask, label, box and dx / dy word equal; dw / dh pass through logf, which the host cannot repeat, and are held to
    the tolerance recorded for them in tests/golden/targets.npz, as tests/test_gpu_targets.py holds them"""
    tr, ref = detector["trace"], detector["ref"]["f64_trace"]
    got, want = tr["rpn_targets"].to_host(), ref["rpn_targets"]
    for key in ("matched", "labels", "mask_pos", "mask_neg", "sampled", "counts"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert close_encoding(got["regression"], want["regression"], detector["tol"][0])
    assert np.array_equal(got["anchors"], ref["anchors"])
    # the ground truth that overlaps nothing restores every anchor whose IoU with it is 0: nearly every anchor is a positive, so the
    # sample holds its 16 positives and whatever negatives are left
    assert (want["counts"][:, 0] == 16).all() and (want["counts"].sum(axis=1) <= 32).all() and (want["labels"] == 1).sum() > 1000
    got, want = tr["roi_targets"].to_host(), ref["roi_targets"]
    for key in ("proposals", "labels", "matched", "sampled", "counts"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert close_encoding(got["regression_targets"], want["regression_targets"], detector["tol"][1])
    filled = want["counts"].sum(axis=1)
    assert (want["counts"][:, 0] > 0).all() and (filled <= SLOTS).all()
    for n in range(2):
        assert (want["labels"][n, filled[n]:] == -1).all() and not want["proposals"][n, filled[n]:].any()
    # no proposal sits on a level boundary, so the level of every slot is certain
    d = want["proposals"].reshape(-1, 4).astype(np.float64)
    s = np.sqrt((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]))
    value = 4.0 + np.log2(np.where(s > 0, s, 1.0) / KW["canonical_scale"])
    assert (np.abs(value - np.round(value))[s > 0] >= 1e-3).all()
    levels = _rois().roi_levels_reference(want["proposals"].reshape(-1, 4), 2, 3, KW["canonical_scale"], 4.0)
    assert set(levels.tolist()) == {0, 1}
    assert same_bits(host(tr["pooled"]), ref["pooled"])


def test_losses_lie_within_the_margin_of_the_fp64_composition(detector):
    """margin: 4 x the distance between the fp64 value and its fp32 evaluation on the host, floored at 1e-6 relative; both sides of it
    are the host flow's, measured in this run"""
    for name, got in detector["losses"].items():
        f64, f32 = float(detector["ref"]["f64"][name]), float(detector["ref"]["f32"][name])
        margin = max(4.0 * abs(f64 - f32), 1e-6 * abs(f64))
        print(f"{name}: device {float(got.detach())!r}, fp64 {f64!r}, fp32 on the host {f32!r}, |device - fp64| "
              f"{abs(float(got.detach()) - f64):.3e}, margin {margin:.3e}")
        assert f64 > 0 and abs(float(got.detach()) - f64) <= margin, name


def test_feature_gradient_is_the_restated_backward_of_pooled_grad(detector):
    rois = _rois()
    features_fn, rpn_head, box_head, predictor = detector["parts"]

    def leaves_fn(images, targets):
        batch, image_sizes, original_sizes, features, resized = features_fn(images, targets)
        return batch, image_sizes, original_sizes, OrderedDict((k, v.detach().requires_grad_()) for k, v in features.items()), resized
    tr = {}
    losses, features = rois.assemble_training_detector(leaves_fn, rpn_head, box_head, predictor, detector["source"], trace=tr, **KW)(
        detector["images"], detector["annots"], 7)
    tr["pooled"].retain_grad()
    (losses["loss_classifier"] + losses["loss_box_reg"]).backward()
    assert torch.equal(bits(tr["pooled"]), bits(detector["trace"]["pooled"]))
    pooled_grad = host(tr["pooled"].grad)
    labels = host(tr["roi_targets"].labels).reshape(-1)
    assert not pooled_grad[labels < 0].any() and pooled_grad[labels >= 0].any()         # an unfilled slot receives a zero gradient
    want = rois.roi_align_backward_reference(pooled_grad, [tuple(f.shape) for f in features.values()], list(host(tr["roi_targets"].proposals)),
                                             tr["image_sizes"], 7, 2, KW["canonical_scale"], 4.0)
    for f, w in zip(features.values(), want):
        assert f.grad is not None and w.any() and same_bits(host(f.grad), w)


def test_every_parameter_receives_a_gradient_and_a_step_repeats_bit_for_bit(detector):
    grads = detector["grads"]
    assert len(grads) == 16
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()) and bool(g.any()), name
    losses, _, again = detector["grads_of"](7)
    for name in detector["losses"]:
        assert torch.equal(bits(losses[name]), bits(detector["losses"][name])), name
    differ = [name for name, g in grads.items() if not torch.equal(bits(again[name]), bits(g))]
    assert not differ, differ
    tr = {}
    rois = _rois()
    rois.assemble_training_detector(*detector["parts"], detector["source"], trace=tr, **KW)(detector["images"], detector["annots"], 8)
    first = detector["trace"]
    assert not torch.equal(tr["rpn_targets"].sampled, first["rpn_targets"].sampled)
    assert not torch.equal(tr["roi_targets"].sampled, first["roi_targets"].sampled)
