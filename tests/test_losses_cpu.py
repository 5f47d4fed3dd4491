"""The training losses on the host (-m "not gpu"): the numpy restatements of `edtr_amd.losses`, which the launches are held to, against
torch's fp64 chains within the bounds that tests/losses_cases.py derives; the items that are exact; the bounds against the seeded
defects; the ulp constants; the C entry points' and the wrappers' refusals."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import losses_cases as K
from edtr_amd import labels, losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def l1_restated(case):
    pairs, dts = K.l1_inputs(case["name"]), K.l1_dtypes(case)
    loss, terms = losses.l1_mean_reference(pairs, case["weights"], dts)
    ga, gb = losses.l1_mean_backward_reference(pairs, case["weights"], K.GRAD_LOSS, dts)
    return loss, terms, ga, gb


@pytest.mark.parametrize("case", K.L1_CASES, ids=K.L1_IDS)
def test_l1_restatement_stays_within_the_bound_and_its_gradients_are_the_rules(case):
    name = case["name"]
    loss, terms, ga, gb = l1_restated(case)
    ref = K.l1_reference(name)
    r = K.l1_ratio(name, loss, terms)
    print(f"{name}: restatement error / bound  loss {r[0]:.3g}  terms {r[1]:.3g}")
    assert max(r) <= 1.0
    want_a, want_b = K.l1_expected_grads(name)
    for k, (p, w) in enumerate(zip(case["pairs"], case["weights"])):
        assert K.same_bits(ga[k], want_a[k]) and K.same_bits(gb[k], want_b[k]), k
        assert np.array_equal(labels._round_to(ga[k], p["dtype"]), ga[k])            # a 16-bit gradient holds values of its type
        # against torch's fp64 gradient: c_k lies within u (and half a 16-bit ulp) relative of the fp64 value, the sign is exact
        tol = (K.U + K.U16[p["dtype"]]) * np.abs(ref["grad_a"][k])
        assert np.all(np.abs(ga[k] - ref["grad_a"][k]) <= tol) and np.all(np.abs(gb[k] - ref["grad_b"][k]) <= tol)
        c = abs(float(K.F32(K.GRAD_LOSS)) * float(K.F32(w)) / p["n"])
        nonzero = ga[k][ga[k] != 0]
        assert nonzero.size == 0 or np.all(np.abs(np.abs(nonzero) - c) <= (K.U + K.U16[p["dtype"]]) * c)


def test_l1_exact_items():
    # equal elements: +0.0 in grad_a and -0.0 in grad_b, as torch's fp32 chain writes them
    case = K.L1_BY_NAME["equal"]
    _, _, ga, gb = l1_restated(case)
    for k, ((a, b), p) in enumerate(zip(K.l1_inputs("equal"), case["pairs"])):
        ta, tb = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
        (K.GRAD_LOSS * F.l1_loss(ta, tb)).backward()
        zero = a == b
        assert int(zero.sum()) == p["equal"]
        assert not ga[k][zero].any() and not np.signbit(ga[k][zero]).any() and not gb[k][zero].any() and np.signbit(gb[k][zero]).all()
        assert np.array_equal(np.signbit(ta.grad.numpy()), np.signbit(ga[k])) and np.array_equal(np.signbit(tb.grad.numpy()), np.signbit(gb[k]))
        assert np.all(ga[k][~zero] != 0)
    # one NaN: NaN loss, +0.0 / -0.0 gradient at it (torch's sign), every other element as without it
    loss, terms, ga, gb = l1_restated(K.L1_BY_NAME["nan"])
    (a, b), = K.l1_inputs("nan")
    at = np.flatnonzero(np.isnan(a))
    assert np.isnan(loss) and np.isnan(terms[0]) and at.size == 1
    assert ga[0][at[0]] == 0 and not np.signbit(ga[0][at[0]]) and gb[0][at[0]] == 0 and np.signbit(gb[0][at[0]])
    ta, tb = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
    lt = F.l1_loss(ta, tb)
    (K.GRAD_LOSS * lt).backward()
    assert torch.isnan(lt) and np.array_equal(np.signbit(ta.grad.numpy()), np.signbit(ga[0])) and np.array_equal(np.signbit(tb.grad.numpy()), np.signbit(gb[0]))
    # for fp32 operands the terms are torch's own fp32 l1_loss to within the bound, and a zero weight adds exactly nothing
    case = K.L1_BY_NAME["mixed5"]
    loss, terms, _, _ = l1_restated(case)
    pairs, dts = K.l1_inputs("mixed5"), K.l1_dtypes(case)
    keep = [k for k, w in enumerate(case["weights"]) if w != 0]
    loss_kept, _ = losses.l1_mean_reference([pairs[k] for k in keep], [case["weights"][k] for k in keep], [dts[k] for k in keep])
    assert loss == loss_kept and len(keep) == 4


def test_l1_sum_order_depends_on_n_alone():
    """the same elements as fp32 and as fp16 (held exactly by both) give the same bits, and a pair's place in the list does not move its term"""
    (a, b), = K.l1_inputs("f16_odd")
    l32, t32 = losses.l1_mean_reference([(a, b)], [1.0], ["float32"])
    l16, t16 = losses.l1_mean_reference([(a.astype(np.float16), b.astype(np.float16))], [1.0], ["float16"])
    assert K.same_bits(l32, l16) and K.same_bits(t32, t16)
    pairs, dts = K.l1_inputs("mixed5"), K.l1_dtypes(K.L1_BY_NAME["mixed5"])
    _, terms = losses.l1_mean_reference(pairs, None, dts)
    _, rev = losses.l1_mean_reference(pairs[::-1], None, dts[::-1])
    assert K.same_bits(terms, rev[::-1])
    # the chunk partials by the stated lane ownership, written out element by element for one chunk
    d = np.abs(a.astype(np.float64) - b)[:4096]
    lane = np.zeros(256)
    for l in range(256):
        for q in range(4):
            for j in range(4):
                lane[l] += d[q * 1024 + 4 * l + j]
    s = 128
    while s:
        lane[:s] += lane[s:2 * s]
        s //= 2
    assert losses.l1_chunk_partials(d)[0] == lane[0]


@pytest.mark.parametrize("defect", K.L1_DEFECTS)
def test_the_l1_bound_rejects_a_seeded_defect(defect):
    name = K.L1_DEFECT_CASE[defect]
    good, bad = K.l1_ratio(name, *K.l1_copy(name)), K.l1_ratio(name, *K.l1_copy(name, defect))
    print(f"{defect} at {name}: error / bound (loss, terms) without {tuple(f'{v:.3g}' for v in good)}, with {tuple(f'{v:.3g}' for v in bad)}")
    assert max(good) <= 1.0
    assert max(bad) > 1.0


def ce_restated(case):
    x, t = K.ce_inputs(case["name"])
    loss, lse, count, bad = losses.cross_entropy_reference(x, t, K.IGNORE, case["dtype"])
    grad = losses.cross_entropy_backward_reference(x, t, lse, count, K.GRAD_LOSS, K.IGNORE, case["dtype"])
    return loss, lse, count, bad, grad


@pytest.mark.parametrize("case", K.CE_CASES, ids=K.CE_IDS)
def test_ce_restatement_stays_within_the_bound_of_the_fp64_chain(case):
    x, t = K.ce_inputs(case["name"])
    loss, lse, count, bad, grad = ce_restated(case)
    ref = K.ce_reference(case["name"])
    keep = K.ce_keep(case, t)
    assert count == ref["count"] == int(keep.sum()) and bad == int((~keep & (t != K.IGNORE)).sum()) and (bad > 0) == case["bad"]
    r = K.ce_ratios(case["name"], loss, lse, grad)
    print(f"{case['name']}: restatement error / bound  loss {r[0]:.3g}  lse {r[1]:.3g}  grad {r[2]:.3g}")
    if count == 0:
        assert np.isnan(loss) and np.isnan(ref["loss"]) and not grad.any() and not np.signbit(grad).any()
    assert not grad[~keep].any() and not np.signbit(grad[~keep]).any()
    assert np.array_equal(labels._round_to(grad, case["dtype"]), grad)
    assert max(r) <= 1.0


def test_ce_exact_items():
    loss, lse, count, bad, grad = ce_restated(K.CE_BY_NAME["one_class"])
    assert loss == 0.0 and count == 1 and not grad.any() and not np.signbit(grad).any()
    # a row of equal logits: lse = z + log(C) and every probability 1 / C to within the bound; the label's element negative
    case = K.CE_BY_NAME["ties"]
    x, t = K.ce_inputs("ties")
    _, lse, _, _, grad = ce_restated(case)
    assert np.all(x[1] == x[1, 0]) and abs(float(lse[1]) - (float(x[1, 0]) + np.log(case["C"]))) <= K.ce_bounds("ties")["lse"][1]
    assert grad[1, t[1]] < 0 and np.all(np.delete(grad[1], t[1]) > 0) and np.unique(np.delete(grad[1], t[1])).size == 1


@pytest.mark.parametrize("defect", K.CE_DEFECTS)
def test_the_ce_bound_rejects_a_seeded_defect(defect):
    name = K.CE_DEFECT_CASE[defect]
    good, bad = K.ce_ratios(name, *K.ce_copy(name)), K.ce_ratios(name, *K.ce_copy(name, defect))
    print(f"{defect} at {name}: error / bound (loss, lse, grad) without {tuple(f'{v:.3g}' for v in good)}, with {tuple(f'{v:.3g}' for v in bad)}")
    assert max(good) <= 1.0
    assert max(bad) > 1.0


def test_the_ulp_figures_are_twice_the_measured_ones():
    with open(os.path.join(ROOT, "profiles", "seg_loss_timing.json")) as fh:
        expf = json.load(fh)["ulp"]["expf"]
    with open(os.path.join(ROOT, "profiles", "losses_timing.json")) as fh:
        logf = json.load(fh)["ulp"]["logf"]
    assert expf["interval"] == [-90.0, 0.0] and logf["interval"] == [1.0, 65536.0]
    assert K.ULP_EXP == 2.0 * expf["worst_ulp"] and K.ULP_LOG == 2.0 * logf["worst_ulp"]


def test_abi_is_additive_and_the_entry_points_refuse_bad_arguments():
    from edtr_amd import build, lib, ops
    assert lib.ABI_VERSION == 10 and "losses.hip" in build.GLUE_SOURCES and "losses.hip" not in build.SOURCES
    assert len(lib.HEADER.structs) == 12
    assert {"edtr_l1_workspace", "edtr_l1_forward", "edtr_l1_backward", "edtr_cls_ce_forward", "edtr_cls_ce_backward"} <= set(lib.DECLARED_SYMBOLS)
    assert lib.L1_MAX_PAIRS == losses.L1_MAX_PAIRS == 8 and lib.L1_CHUNK == losses.L1_CHUNK == 4096 and lib.L1_MAX_ELEMS == losses.L1_MAX_ELEMS == 1 << 30
    assert lib.CLS_MAX_CLASSES == losses.CE_MAX_CLASSES
    for fn in ("edtr_l1_forward", "edtr_l1_backward", "edtr_cls_ce_forward", "edtr_cls_ce_backward"):      # no parameter is a pointer to a struct
        assert not any(t.base in lib.HEADER.structs for _, t in lib.HEADER.functions[fn][1])
    assert all(callable(getattr(ops, n)) for n in ("make_l1_forward", "make_l1_backward", "make_cls_ce_forward", "make_cls_ce_backward", "l1_workspace"))
    with open(os.path.join(ROOT, "edtr_amd", "csrc", "losses.hip")) as fh:
        src = re.sub(r"//.*", "", fh.read())
    assert not re.search(r"atomic|hipMemset|__expf|__logf|\basm\b|wave_prims", src) and '#include "glue.h"' in src
    build.build_library()
    h = lib.load()
    K.check_l1_rejections(h)
    K.check_ce_rejections(h)


def test_the_wrappers_refuse_before_they_launch():
    """no device is needed: every one of these is refused on its arguments"""
    a, b = torch.zeros(2, 3), torch.zeros(2, 3)
    with pytest.raises(TypeError):
        losses.l1_mean([(a.double(), b.double())])                               # a dtype
    with pytest.raises(TypeError):
        losses.l1_mean([(a, b.half())])
    with pytest.raises(ValueError):
        losses.l1_mean([(a, torch.zeros(3, 2))])                                 # a shape mismatch within a pair
    with pytest.raises(ValueError):
        losses.l1_mean([(a, b)] * 9)                                             # more than 8 pairs
    with pytest.raises(ValueError):
        losses.l1_mean([])
    with pytest.raises(ValueError):
        losses.l1_mean([(a, b)], weights=[1.0, 2.0])
    with pytest.raises(TypeError):
        losses.l1_mean([(a, b)])                                                 # not on the device
    with pytest.raises(ValueError):
        losses.feature_matching({"C5": a}, {"C5": b}, keys=("C5",), weights=(0.5, 0.5))
    with pytest.raises(TypeError):
        losses.feature_matching({"C5": a}, b)
    with pytest.raises(ValueError):
        losses.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), label_smoothing=0.1)
    with pytest.raises(TypeError):
        losses.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))   # not on the device
    with pytest.raises(ValueError):
        losses.l1_mean_reference([(np.zeros(3, np.float32), np.zeros(4, np.float32))])
    with pytest.raises(ValueError):
        losses.l1_mean_reference([(np.full(3, 1e-3, np.float32), np.zeros(3, np.float32))], dtypes=["bfloat16"])
    with pytest.raises(ValueError):
        losses.cross_entropy_reference(np.zeros((2, 3), np.float32), np.zeros(3, np.int64))


def test_the_module_imports_without_torch():
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None; import numpy as np; from edtr_amd import losses; "
            "print(losses.l1_mean_reference([(np.ones(5, np.float32), np.zeros(5, np.float32))])[0])")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "1.0", out.stderr
