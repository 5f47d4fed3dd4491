"""RoIAlign's backward on the host (-m "not gpu"): the numpy restatement `rois.roi_align_backward_reference`, which the kernel is held to
bit for bit, against fp64 autograd through a forward written here from `rois._taps` (tests/roi_backward_cases.py), within a bound
that is derived and not measured; the adjoint identity; seeded defects that the bound must reject; the header; the Python surface."""
import os

import numpy as np
import pytest
import torch

import roi_backward_cases as RC
from edtr_amd import detinput, rois

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference(case, dtype="float32", grad=None):
    return rois.roi_align_backward_reference(case["grad"] if grad is None else grad, case["shapes"], case["rois"], case["image_sizes"], case["P"],
                                             case["S"], case["canonical_scale"], case["canonical_level"], dtype=dtype)


def worst_ratio(got, want, bound):
    return max(float((np.abs(g.astype(np.float64) - w) / np.maximum(b, 1e-300)).max()) for g, w, b in zip(got, want, bound))


@pytest.fixture(scope="module")
def fp64():
    """(want, bound) per case and output type, computed once"""
    cache = {}

    def get(i, dtype="float32"):
        if (i, dtype) not in cache:
            cache[i, dtype] = RC.bounds(RC.CASES[i], dtype)
        return cache[i, dtype]
    return get


def test_the_case_table_keeps_its_promises():
    RC.self_check()


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=RC.CASE_IDS)
def test_restatement_against_fp64_autograd(i, dtype, fp64):
    case = RC.CASES[i]
    got = reference(case, dtype)
    want, bound = fp64(i, dtype)
    assert [g.shape for g in got] == [tuple(s) for s in case["shapes"]] and all(g.dtype == F32 for g in got)
    ratio = worst_ratio(got, want, bound)
    print(f"{case['name']} {dtype}: worst |got - fp64| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # what no roi touches is +0.0, sign included
    for g, w in zip(got, want):
        assert not np.signbit(g[w == 0]).any() and not g[w == 0].any()


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=RC.CASE_IDS)
def test_restatement_equals_its_scalar_copy_bit_for_bit(i):
    """the copy visits every pixel and skips no zero term: skipping them changes no bit"""
    case = RC.CASES[i]
    for dtype in ("float32", "bfloat16"):
        for g, c in zip(reference(case, dtype), RC.backward_copy(case, dtype=dtype)):
            assert np.array_equal(g.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("i", range(len(RC.CASES)), ids=RC.CASE_IDS)
def test_adjoint_identity(i, fp64):
    """<roi_align_reference(f), g> = <f, backward_reference(g)>, both accumulated in fp64.  The left side carries the forward's own fp32
    rounding, the right side the backward's; each is bounded by the element bound summed against |f| (the forward's operations are
    the same products and sums, transposed), so the two differ by at most twice that."""
    case = RC.CASES[i]
    rng = np.random.default_rng(100 + i)
    feats = [rng.standard_normal(s).astype(F32) for s in case["shapes"]]
    pooled = rois.roi_align_reference(feats, case["rois"], case["image_sizes"], case["P"], case["S"], case["canonical_scale"], case["canonical_level"])
    left = float((pooled.astype(np.float64) * case["grad"].astype(np.float64)).sum())
    right = sum(float((f.astype(np.float64) * g.astype(np.float64)).sum()) for f, g in zip(feats, reference(case)))
    _, bound = fp64(i)
    slack = 2.0 * sum(float((np.abs(f).astype(np.float64) * b).sum()) for f, b in zip(feats, bound))
    print(f"{case['name']}: <Af, g> = {left!r}, <f, A'g> = {right!r}, |difference| = {abs(left - right):.3e}, bound {slack:.3e}")
    assert abs(left - right) <= slack


@pytest.mark.parametrize("defect", RC.DEFECTS)
def test_each_seeded_defect_is_rejected(defect, fp64):
    """the copy with a defect exceeds the bound the restatement meets, on the first two cases (both have invalid and clamped taps)"""
    for i in (0, 1):
        want, bound = fp64(i)
        assert worst_ratio(RC.backward_copy(RC.CASES[i]), want, bound) <= 1.0
        ratio = worst_ratio(RC.backward_copy(RC.CASES[i], defect), want, bound)
        assert ratio > 1e3, (defect, RC.CASES[i]["name"], ratio)


def test_the_one_element_gradient_lands_on_the_pixels_of_its_bin():
    case = RC.CASES[3]
    k, c = 1, case["C"] - 1
    got = reference(case)
    _, n, lvl, H, W, ty, tx = RC.per_roi(case)[k]
    ph, pw = case["P"] - 1, case["P"] // 2
    rows = {int(v) for t, ok in ((ty[1], ty[0]), (ty[2], ty[0])) for v in t[ph][ok[ph]]}
    cols = {int(v) for t, ok in ((tx[1], tx[0]), (tx[2], tx[0])) for v in t[pw][ok[pw]]}
    for l, g in enumerate(got):
        nz = np.argwhere(g != 0)
        if l != lvl:
            assert not nz.size
            continue
        assert nz.size and set(nz[:, 0]) == {n} and set(nz[:, 1]) == {c}
        assert set(nz[:, 2]) <= rows and set(nz[:, 3]) <= cols


def test_restatement_checks_its_arguments_and_the_empty_forms():
    case = RC.CASES[0]
    with pytest.raises(ValueError):
        reference(case, grad=case["grad"][:, :, :6])
    with pytest.raises(ValueError):
        reference(case, dtype="float64")
    with pytest.raises(ValueError):
        rois.roi_align_backward_reference(case["grad"], case["shapes"], case["rois"][:1], case["image_sizes"], 7, 2)
    none = [np.zeros((0, 4), dtype=F32)] * 2
    out = rois.roi_align_backward_reference(np.zeros((0, 70, 7, 7), dtype=F32), case["shapes"], none, case["image_sizes"])
    assert [o.shape for o in out] == [tuple(s) for s in case["shapes"]] and not any(o.any() or np.signbit(o).any() for o in out)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_backward_and_the_abi_is_still_10():
    from edtr_amd import build, lib
    assert {"edtr_roi_align_backward", "edtr_roi_align_backward_workspace"} <= set(lib.DECLARED_SYMBOLS)
    assert lib.ABI_VERSION == 10 and (lib.ROI_BWD_MAX_P, lib.ROI_BWD_CHUNK) == (rois.ROI_BWD_MAX_P, 32)
    ret, params = lib.HEADER.functions["edtr_roi_align_backward"]
    forward = [n for n, _ in lib.HEADER.functions["edtr_roi_align"][1]]
    names = [n for n, _ in params]
    assert names[:1] + names[2:16] == forward[:1] + forward[2:16]            # the forward's list, the pointer table renamed
    assert names[16:] == ["grad", "workspace", "workspace_bytes", "stream"] and names[1] == "grads_out_host"
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == 10 and hasattr(handle, "edtr_roi_align_backward") and hasattr(handle, "edtr_roi_align_backward_workspace")


def test_the_backward_rejects_bad_arguments_before_any_launch():
    from edtr_amd import build, lib
    build.build_library()
    RC.check_rejections(lib.load())


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------
def test_roi_align_on_cpu_tensors_raises_as_before():
    """the argument checks come before any device; and where there is no device the launch wrapper, which has no host path, raises
    what it raised before, with or without requires_grad"""
    with pytest.raises(ValueError):
        rois.roi_align_backward(torch.zeros(1, 2, 17, 17), [(1, 2, 8, 8)], [torch.zeros(1, 4)], [(32, 32)], 17, 1, device="cpu")
    with pytest.raises(TypeError):
        rois.roi_align_backward(torch.zeros(1, 2, 7, 7).double(), [(1, 2, 8, 8)], [torch.zeros(1, 4)], [(32, 32)], device="cpu")
    with pytest.raises(ValueError):
        rois.roi_align_backward(torch.zeros(1, 2, 7, 7), [(1, 2, 8, 8), (1, 3, 4, 4)], [torch.zeros(1, 4)], [(32, 32)], device="cpu")
    if torch.cuda.is_available():
        return                  # with a device the wrapper uploads host tensors: tests/test_gpu_roi_backward.py
    kinds = []
    for needs in (False, True):
        with pytest.raises(Exception) as e:
            rois.roi_align([torch.zeros(1, 2, 8, 8).requires_grad_(needs)], [torch.tensor([[1.0, 1.0, 9.0, 9.0]])], [(32, 32)])
        kinds.append(type(e.value))
    assert kinds[0] is kinds[1] and not issubclass(kinds[0], (TypeError, ValueError, AttributeError, NameError))


def test_assemble_features_without_grad_is_the_old_behaviour(monkeypatch):
    """grad=False (the default) runs the backbone under no_grad and returns the four values; grad=True runs it with grad enabled and,
    given targets, returns the resized targets as a fifth value."""
    seen = {}

    class Prepare:
        def batch(self, images):
            return torch.ones(1, 3, 8, 8), [(8, 8)], [(16, 16)]

        def __call__(self, images, targets=None):
            seen["targets"] = targets
            return detinput.ImageBatch(torch.ones(1, 3, 8, 8), [(8, 8)]), [dict(t, resized=True) for t in targets]

    weight = torch.nn.Parameter(torch.tensor(2.0))
    images = [torch.zeros(3, 16, 16)]

    def backbone(x):
        seen["grad_mode"] = torch.is_grad_enabled()
        return x * weight

    for kw in ({}, {"grad": False}):
        out = detinput.assemble_features(backbone, Prepare(), **kw)(images)
        assert len(out) == 4 and seen["grad_mode"] is False
        assert list(out[3]) == ["0"] and out[3]["0"].grad_fn is None and not out[3]["0"].requires_grad
    fn = detinput.assemble_features(backbone, Prepare(), grad=True)
    out = fn(images)
    assert len(out) == 4 and seen["grad_mode"] is True and out[3]["0"].grad_fn is not None
    with torch.no_grad():
        assert fn(images)[3]["0"].grad_fn is None                                   # (the caller's no_grad still holds)
    out = fn(images, [{"boxes": torch.zeros(1, 4)}])
    assert len(out) == 5 and out[4][0]["resized"] and out[1] == [(8, 8)] and out[2] == [(16, 16)]
    with pytest.raises(TypeError):
        detinput.assemble_features(backbone, Prepare())(images, [{"boxes": torch.zeros(1, 4)}])
