"""The segmentation loss from coarse logits on the host (-m "not gpu"): the numpy restatements `labels.coarse_cross_entropy_reference` /
`coarse_cross_entropy_backward_reference`, which the launches are held to, against torch's fp64 chain within the bound that
tests/seg_loss_cases.py derives; the items that are exact; the bound against six seeded defects; the C entry points' refusals."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_loss_cases as K
from edtr_amd import labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(case):
    x, t = K.inputs(case)
    loss, lse, count, bad = labels.coarse_cross_entropy_reference(x, t, dtype=case["dtype"])
    grad = labels.coarse_cross_entropy_backward_reference(x, t, lse, count, K.GRAD_LOSS, dtype=case["dtype"])
    return loss, lse, count, bad, grad


@pytest.mark.parametrize("case", K.CASES, ids=K.CASE_IDS)
def test_restatements_stay_within_the_bound_of_the_fp64_chain(case):
    x, t = K.inputs(case)
    loss, lse, count, bad, grad = restated(case)
    ref = K.reference(case["name"])
    keep = K.keep_mask(case, t)
    assert count == ref["count"] == int(keep.sum()) and bad == int(((t >= case["n"]) & (t != 255)).sum())
    assert (bad > 0) == case["planted_bad"]
    r = K.ratios(case["name"], loss, lse, grad)
    line = f"{case['name']}: restatement error / bound  loss {r[0]:.3g}  lse {r[1]:.3g}  grad {r[2]:.3g}"
    if case["dtype"] == "float32" and count:
        xt = torch.tensor(x, requires_grad=True)
        z = F.interpolate(xt, size=(case["H"], case["W"]), mode="bilinear", align_corners=False)
        lt = F.cross_entropy(z, torch.tensor(np.where(keep, t, 255).astype(np.int64)), ignore_index=255)
        (K.GRAD_LOSS * lt).backward()
        q = K.ratios(case["name"], lt.item(), torch.logsumexp(z, 1).detach().numpy(), xt.grad.numpy())
        line += f";  torch fp32 error / bound  loss {q[0]:.3g}  lse {q[1]:.3g}  grad {q[2]:.3g}"
    print(line)
    if count == 0:
        assert np.isnan(loss) and np.isnan(ref["loss"]) and not grad.any() and not np.signbit(grad).any()
    assert max(r) <= 1.0, line


def test_exact_items():
    # (e): one class, so lse == z and the softmax is 1: loss exactly 0, gradient exactly +0.0
    loss, lse, count, bad, grad = restated(K.BY_NAME["e_one_class"])
    assert loss == 0.0 and count > 0 and not grad.any() and not np.signbit(grad).any()
    # strong down-sampling leaves coarse positions no pixel reaches: +0.0 there
    case = K.BY_NAME["c_down_far"]
    _, _, _, _, grad = restated(case)
    (Ay, _), (Ax, _) = K._axis(case["ih"], case["H"]), K._axis(case["iw"], case["W"])
    reached = (Ay.sum(0) > 0)[:, None] & (Ax.sum(0) > 0)[None, :]
    assert np.flatnonzero(~(Ay.sum(0) > 0)).tolist() == [0, 3, 4, 5, 8]
    assert not reached.all() and reached.any()
    assert not grad[:, :, ~reached].any() and not np.signbit(grad[:, :, ~reached]).any() and np.all(grad[:, :, reached] != 0)
    # (g): every t is 0, the upsample is the identity: plain cross-entropy of the logits
    case = K.BY_NAME["g_identity"]
    x, t = K.inputs(case)
    assert np.array_equal(labels.upsample_logits_reference(x, (6, 6)), x)
    # image 1 of (f) is entirely 255: its gradient is zero
    _, _, _, _, grad = restated(K.BY_NAME["f_tiles"])
    assert not grad[1].any() and grad[0].any() and grad[2].any()


def test_a_16_bit_gradient_holds_values_of_its_type_and_the_arguments_are_checked():
    case = K.BY_NAME["b_fractional_bf16"]
    x, t = K.inputs(case)
    _, _, _, _, grad = restated(case)
    assert np.array_equal(labels._round_to(grad, "bfloat16"), grad)
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy_reference(x, t, size=(37, 51))
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy_reference(x, t[:1])
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy_reference(x, t.astype(np.int64))
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy_reference(np.zeros((1, 257, 2, 2), dtype=np.float32), np.zeros((1, 4, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy_reference((x + np.float32(1e-3)).astype(np.float32), t, dtype="bfloat16")


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_the_bound_rejects_a_seeded_defect(defect):
    """Each defect at the case the issue names for it.  "The maximum not subtracted" (at logits of +-80) is planted as the one omission
    that makes the value wrong: exp(z_c) in place of exp(z_c - m) inside lse = m + log(sum), which is off by m."""
    case = K.BY_NAME[K.DEFECT_CASE[defect]]
    good, bad = K.ratios(case["name"], *K.restatement_copy(case)), K.ratios(case["name"], *K.restatement_copy(case, defect))
    print(f"{defect} at {case['name']}: error / bound (loss, lse, grad) without {tuple(f'{v:.3g}' for v in good)}, with {tuple(f'{v:.3g}' for v in bad)}")
    assert max(good) <= 1.0
    assert max(bad) > 1.0


def test_a_sum_without_the_maximum_is_rejected_where_fp32_cannot_hold_it():
    """log(sum_c exp(z_c)) with the maximum neither subtracted nor added back is the rule's value written another way.  At logits of
    +-80 fp32 holds every exp(z_c), the two forms are equally accurate and the bound accepts both (error / bound of (loss, lse, grad)
    measured at (0.00056, 0.012, 0.060) for either); at +-100 exp overflows, lse is inf and the bound rejects it."""
    at80, at100 = K.BY_NAME["a_8x_pm80"], K.BY_NAME["a_8x_pm100"]
    held = K.ratios(at80["name"], *K.restatement_copy(at80, "plain_sum"))
    lost = K.ratios(at100["name"], *K.restatement_copy(at100, "plain_sum"))
    print(f"plain_sum: error / bound (loss, lse, grad) at +-80 {tuple(f'{v:.3g}' for v in held)}, at +-100 {tuple(f'{v:.3g}' for v in lost)}")
    assert max(held) <= 1.0 and max(K.ratios(at100["name"], *K.restatement_copy(at100))) <= 1.0
    assert max(lost) > 1.0


def test_the_ulp_figures_are_twice_the_measured_ones():
    with open(os.path.join(ROOT, "profiles", "seg_loss_timing.json")) as fh:
        ulp = json.load(fh)["ulp"]
    assert K.ULP_EXP == 2.0 * ulp["expf"]["worst_ulp"] and K.ULP_LOG == 2.0 * ulp["logf"]["worst_ulp"]


def test_abi_is_additive_and_the_entry_points_refuse_bad_arguments():
    from edtr_amd import build, lib, ops
    assert "seg_loss.hip" in build.GLUE_SOURCES and lib.ABI_VERSION == 10
    assert {"edtr_seg_ce_forward", "edtr_seg_ce_backward", "edtr_seg_ce_workspace"} <= set(lib.DECLARED_SYMBOLS)
    assert lib.SEG_CE_MAX_CLASSES == labels.SEG_CE_MAX_CLASSES == 256
    assert callable(ops.make_seg_ce_forward) and callable(ops.make_seg_ce_backward)
    with open(os.path.join(ROOT, "edtr_amd", "csrc", "seg_loss.hip")) as fh:
        src = fh.read()
    assert not re.search(r"atomic|hipMemset|__expf|__logf", re.sub(r"//.*", "", src))
    build.build_library()
    K.check_rejections(lib.load())


def test_the_device_wrapper_refuses_before_it_launches():
    """no device is needed: every one of these is refused on its arguments"""
    x, t = torch.zeros(1, 3, 2, 2), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(TypeError):
        labels.coarse_cross_entropy(x, t)                                       # not on the device
    with pytest.raises(ValueError):
        labels.coarse_cross_entropy(labels.CoarseLogits(x, (4, 4)), t, size=(4, 5))
