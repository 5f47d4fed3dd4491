"""The launches of edtr_amd/targets.py (csrc/targets.hip) against their numpy restatements, word for word wherever log does not enter:
matched indices, labels, masks, sampled indices, counts and the dx, dy of every encoding.  dw and dh go through the device's logf and
stay within the tolerance tools/make_targets_goldens.py measured (tests/golden/targets.npz) of the restatement with numpy's log."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from edtr_amd import lib, ops, rng, targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32 = np.float32
N = 3


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "targets.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def source_of(gold):
    return rng.NoiseSource(int(gold["seed"]), gold["image_ids"].tolist())


def targets_of(gold):
    return [{"boxes": gold[f"gt_boxes{n}"], "labels": gold[f"gt_labels{n}"]} for n in range(N)]


def geometry(gold):
    return dict(sizes=tuple(map(tuple, gold["sizes"])), aspect_ratios=tuple(map(tuple, gold["ratios"])))


def close_encoding(got, want, tol):
    """dx, dy equal; dw, dh finite in the same places and within tol there, equal elsewhere (the infinities of a zero box)"""
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    ok = np.isfinite(want[:, 2:])
    worst = float(np.abs(got[:, 2:][ok] - want[:, 2:][ok]).max()) if ok.any() else 0.0
    print(f"\n[encode] {got.shape[0]} boxes, max |dw, dh - restatement| {worst:.3e}, tolerance {float(tol):.3e}")
    return (np.array_equal(got[:, :2], want[:, :2], equal_nan=True) and np.array_equal(np.isfinite(got[:, 2:]), ok) and worst <= float(tol)
            and np.array_equal(got[:, 2:][~ok], want[:, 2:][~ok], equal_nan=True))


@pytest.fixture(scope="module")
def random_case():
    """three images of 2500, 1 and 1025 boxes (three tiles, one box, one box past a tile) with 7, 3 and 0 ground truths: boxes on a
    quarter-pixel grid so that equal IoUs are common, some ground truths copied from boxes, one far away; left unchanged"""
    rs = np.random.default_rng(20282)

    def boxes(n, span):
        x1, y1 = rs.integers(0, 4 * span, n) / 4, rs.integers(0, 4 * span, n) / 4
        return np.stack([x1, y1, x1 + rs.integers(4, 160, n) / 4, y1 + rs.integers(4, 160, n) / 4], axis=1).astype(F32)
    b = [boxes(2500, 100), boxes(1, 100), boxes(1025, 60)]
    g = [np.concatenate([boxes(4, 100), b[0][[17, 17, 2400]]]).astype(F32), np.concatenate([b[1], boxes(1, 100), [[900, 900, 910, 910]]]).astype(F32),
         np.zeros((0, 4), dtype=F32)]
    labels = [rs.integers(1, 6, len(x)) for x in g]
    return b, g, labels


# ---- match -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("allow", [True, False])
def test_match_on_the_shared_anchors_equals_the_restatement(gold, allow):
    gt = [gold[f"gt_boxes{n}"] for n in range(N)]
    got = targets.match(gold["anchors"], gt, 0.7, 0.3, allow, "rpn", weights=targets.RPN_WEIGHTS)
    want = targets.match_reference(gold["anchors"], gt, 0.7, 0.3, allow)
    assert got.matched.dtype == torch.int32 and got.labels.dtype == torch.float32 and got.matched.is_cuda
    assert np.array_equal(host(got.matched), np.concatenate(want))
    if allow:
        assert np.array_equal(host(got.matched).reshape(N, -1), gold["rpn_matched"]) and np.array_equal(host(got.labels).reshape(N, -1), gold["rpn_labels"])
    assert np.array_equal(host(got.labels), np.concatenate([targets.labels_reference(m, "rpn") if len(g) else np.zeros(len(m), F32) for m, g in zip(want, gt)]))
    ref = np.concatenate([targets.encode_reference(g[np.clip(m, 0, None)] if len(g) else np.zeros_like(gold["anchors"]), gold["anchors"])
                          for m, g in zip(want, gt)])
    assert close_encoding(host(got.regression), ref, gold["tol_rpn_dwdh"])


def test_match_reproduces_the_quirk_beside_real_matches(gold):
    got = targets.match(gold["anchors"], [gold["gt6"]], 0.7, 0.3, True)
    assert np.array_equal(host(got.matched), gold["quirk6_matched"]) and got.regression is None
    q = dev(np.zeros((5, 4), dtype=F32))            # degenerate boxes: every IoU is 0 / 0, every best a NaN that keeps index 0
    nan = targets.match([q], [gold["gt6"][:2] * 0], 0.7, 0.3, True)
    assert np.array_equal(host(nan.matched), targets.match_reference([np.zeros((5, 4), F32)], [np.zeros((2, 4), F32)], 0.7, 0.3, True)[0])


@pytest.mark.parametrize("allow", [True, False])
def test_ragged_match_in_the_roi_form_equals_the_restatement(random_case, allow):
    b, g, labels = random_case
    got = targets.match(b, g, 0.5, 0.25, allow, "roi", gt_labels=labels)
    want = targets.match_reference(b, g, 0.5, 0.25, allow)
    assert np.array_equal(host(got.matched), np.concatenate(want)) and got.labels.dtype == torch.int64
    assert np.array_equal(host(got.labels), np.concatenate([targets.labels_reference(m, "roi", l) for m, l in zip(want, labels)]))
    assert got.table_host == [(0, 0), (2500, 7), (2501, 10), (3526, 10)]
    assert all({-1, -2} <= set(m.tolist()) for m in want[:1]) and (want[2] == 0).all()


def test_match_propagates_nan_coordinates_as_torch_does():
    b = np.array([[0, 0, 4, 4], [np.nan, 0, 4, 4], [1, 1, 3, 3], [0, 0, 4, np.nan], [10, 10, 12, 12]], dtype=F32)
    g = np.array([[0, 0, 4, 4], [1, 1, 3, 3], [0, 0, 4, 4]], dtype=F32)
    for allow in (True, False):
        got = targets.match([b], [g], 0.7, 0.3, allow)
        assert np.array_equal(host(got.matched), targets.match_reference([b], [g], 0.7, 0.3, allow)[0])
    g[1, 2] = np.nan                                # a NaN ground truth: its highest is NaN and restores nothing
    got = targets.match([b], [g], 0.7, 0.3, True)
    assert np.array_equal(host(got.matched), targets.match_reference([b], [g], 0.7, 0.3, True)[0])


def test_a_non_contiguous_view_is_copied(gold):
    wide = dev(np.repeat(gold["anchors"], 2, axis=1))
    view = wide[:, ::2]
    assert not view.is_contiguous()
    gt = [dev(np.repeat(gold["gt_boxes0"], 2, axis=0))[::2]]
    got = targets.match(view, gt, 0.7, 0.3, True)
    assert np.array_equal(host(got.matched), gold["rpn_matched"][0])
    enc = targets.encode(view[:5], dev(np.repeat(gold["gt_boxes0"], 2, axis=1))[:, ::2])
    assert np.array_equal(host(enc)[:, :2], targets.encode_reference(gold["anchors"][:5], gold["gt_boxes0"])[:, :2])


# ---- encode ------------------------------------------------------------------------------------------------------------------------------
def test_encode_launch_equals_the_restatement(gold):
    ref = np.concatenate([gold[f"roi_proposals{n}"] for n in range(N)])
    rs = np.random.default_rng(3)
    g = (ref + rs.normal(0, 3, ref.shape)).astype(F32)
    g[:, 2:] = np.maximum(g[:, 2:], g[:, :2] + 1)
    for w in (targets.RPN_WEIGHTS, targets.ROI_WEIGHTS):
        got = targets.encode(g, ref, w)
        assert got.dtype == torch.float32 and close_encoding(host(got), targets.encode_reference(g, ref, w), gold["tol_roi_dwdh"])
    assert targets.encode(np.zeros((0, 4), F32), np.zeros((0, 4), F32)).shape == (0, 4)


# ---- sample ------------------------------------------------------------------------------------------------------------------------------
def check_sample(labels, batch, fraction, src, draw, purpose):
    got = targets.sample([dev(l) for l in labels], batch, fraction, src, draw, purpose).to_host()
    mp, mn, sampled, counts = targets.sample_reference(labels, batch, fraction, src, draw, purpose)
    assert got["mask_pos"].dtype == np.uint8 and np.array_equal(got["mask_pos"], np.concatenate(mp)) and np.array_equal(got["mask_neg"], np.concatenate(mn))
    assert np.array_equal(got["sampled"], sampled) and np.array_equal(got["counts"], counts)
    return counts


def test_sample_on_the_fixture_labels_equals_the_restatement(gold):
    counts = check_sample(list(gold["rpn_labels"]), 256, 0.5, source_of(gold), int(gold["draw"]), rng.PURPOSE_SAMPLE_RPN)
    assert counts.tolist() == gold["rpn_counts"].tolist()
    got = targets.sample([dev(l) for l in gold["rpn_labels"]], 256, 0.5, source_of(gold), int(gold["draw"]))
    assert np.array_equal(host(got.mask_pos).reshape(N, -1), gold["rpn_mask_pos"]) and np.array_equal(host(got.mask_neg).reshape(N, -1), gold["rpn_mask_neg"])
    roi = [gold[f"roi_all_labels{n}"] for n in range(N)]
    assert check_sample(roi, 64, 0.25, source_of(gold), int(gold["draw"]), rng.PURPOSE_SAMPLE_ROI).tolist() == [[16, 48], [16, 48], [0, 64]]


@pytest.mark.parametrize("sizes", [(1, 63, 64), (65, 1023, 1024), (1025, 4099, 2)])
def test_sample_sizes_around_the_wave_and_the_workgroup(sizes):
    rs = np.random.default_rng(sum(sizes))
    labels = [rs.choice(np.array([-1, 0, 0, 1, 3], dtype=np.int64), n) for n in sizes]
    src = rng.NoiseSource(99, [5, 1 << 31, 77])
    for batch, fraction in ((1, 1.0), (8, 0.5), (512, 0.25), (4096, 0.0)):
        check_sample(labels, batch, fraction, src, 2, rng.PURPOSE_SAMPLE_ROI)
    check_sample([l.astype(F32) for l in labels], 16, 0.75, src, 0, rng.PURPOSE_SAMPLE_RPN)


@pytest.mark.parametrize("dtype", [np.int64, F32])
def test_equal_keys_go_to_the_smaller_index(gold, dtype):
    """keys handed in, as to `sample_reference`: the stream practically never gives two boxes one key.  The fixture's twelve boxes; then
    three images whose keys take a handful of values (one value only in the last), so that the threshold key is shared by boxes of
    several lanes, waves and rounds and only some of them are taken"""
    batch, fraction = gold["eq_params"]
    got = targets.sample([dev(gold["eq_labels"].astype(dtype))], int(batch), fraction, None, keys=[gold["eq_keys"]]).to_host()
    assert np.array_equal(got["mask_pos"], gold["eq_mask_pos"]) and np.array_equal(got["mask_neg"], gold["eq_mask_neg"])
    assert got["sampled"].tolist() == [[0, 1, 2, 4, 6, 8]] and got["counts"].tolist() == [[3, 3]]
    rs = np.random.default_rng(7)
    sizes = (9001, 4097, 300)
    labels = [rs.choice(np.array([-1, 0, 0, 1, 2]), n).astype(dtype) for n in sizes]
    keys = [rs.choice(np.array([0, 3, 3, 1 << 21, (1 << 21) + 1, 0xffffffff, 0xfffffc00], dtype=np.uint32), sizes[0]),
            rs.integers(0, 5, sizes[1]).astype(np.uint32) << np.uint32(10), np.full(sizes[2], 77, dtype=np.uint32)]
    for b, f in ((512, 0.25), (4096, 0.5), (7, 0.5)):
        got = targets.sample([dev(l) for l in labels], b, f, None, keys=keys).to_host()
        mp, mn, sampled, counts = targets.sample_reference(labels, b, f, keys=keys)
        assert np.array_equal(got["mask_pos"], np.concatenate(mp)) and np.array_equal(got["mask_neg"], np.concatenate(mn))
        assert np.array_equal(got["sampled"], sampled) and np.array_equal(got["counts"], counts)


def test_the_sample_of_an_image_does_not_depend_on_its_batch(gold):
    labels = list(gold["rpn_labels"])
    ids = gold["image_ids"].tolist()
    seed, draw = int(gold["seed"]), int(gold["draw"])
    whole = targets.sample([dev(l) for l in labels], 256, 0.5, rng.NoiseSource(seed, ids), draw).to_host()
    other = targets.sample([dev(labels[2]), dev(labels[0])], 256, 0.5, rng.NoiseSource(seed, [ids[2], ids[0]]), draw).to_host()
    alone = targets.sample([dev(labels[0])], 256, 0.5, rng.NoiseSource(seed, [ids[0]]), draw).to_host()
    A = labels[0].shape[0]
    assert np.array_equal(whole["sampled"][0], other["sampled"][1]) and np.array_equal(whole["sampled"][0], alone["sampled"][0])
    assert np.array_equal(whole["mask_neg"][:A], other["mask_neg"][A:]) and np.array_equal(whole["sampled"][2], other["sampled"][0])
    again = targets.sample([dev(labels[0])], 256, 0.5, rng.NoiseSource(seed, [ids[0]]), draw + 1).to_host()
    assert not np.array_equal(again["sampled"], alone["sampled"]) and np.array_equal(again["counts"], alone["counts"])


# ---- the two flows -----------------------------------------------------------------------------------------------------------------------
def test_rpn_targets_equals_the_flow_through_the_restatements(gold):
    high, low, batch, fraction = gold["rpn_params"]
    kw = dict(high=high, low=low, batch_size_per_image=int(batch), positive_fraction=fraction, source=source_of(gold), draw=int(gold["draw"]))
    got = targets.rpn_targets(gold["grids"], gold["padded"], targets_of(gold), **geometry(gold), **kw).to_host()
    want = targets.rpn_targets_reference(gold["anchors"], targets_of(gold), **kw)
    assert np.array_equal(got["anchors"], gold["anchors"])
    for k in ("matched", "labels", "mask_pos", "mask_neg", "sampled", "counts"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["labels"], gold["rpn_labels"]) and np.array_equal(got["mask_pos"], gold["rpn_mask_pos"])
    assert got["regression"].shape == (N, 1512, 4) and close_encoding(got["regression"], want["regression"], gold["tol_rpn_dwdh"])


def test_roi_targets_equals_the_flow_through_the_restatements(gold):
    high, low, batch, fraction = gold["roi_params"]
    kw = dict(high=high, low=low, batch_size_per_image=int(batch), positive_fraction=fraction, weights=tuple(gold["roi_weights"]),
              source=source_of(gold), draw=int(gold["draw"]))
    props = [gold[f"roi_input{n}"] for n in range(N)]
    got = targets.roi_targets(props, targets_of(gold), **kw).to_host()
    want = targets.roi_targets_reference(props, targets_of(gold), **kw)
    for k in ("proposals", "labels", "matched", "sampled", "counts"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert close_encoding(got["regression_targets"], want["regression_targets"], gold["tol_roi_dwdh"])
    for n in range(N):
        k = int(got["counts"][n].sum())
        assert np.array_equal(got["proposals"][n, :k], gold[f"roi_proposals{n}"]) and np.array_equal(got["labels"][n, :k], gold[f"roi_labels{n}"])
        assert np.array_equal(got["matched"][n, :k], gold[f"roi_matched{n}"])
    # the defaults: 512 / 0.25 at 0.5 / 0.5, more slots than some image fills
    d = targets.roi_targets(props, targets_of(gold), source=source_of(gold), draw=1).to_host()
    w = targets.roi_targets_reference(props, targets_of(gold), source=source_of(gold), draw=1)
    assert d["labels"].shape == (N, 512) and all(np.array_equal(d[k], w[k]) for k in ("proposals", "labels", "matched", "sampled", "counts"))


def test_rpn_loss_on_the_device_meets_compute_loss(gold):
    """the device's targets (logf in dw, dh) and torch's device reductions against the reference's recorded losses, within the
    tolerance the golden tool measured for another summation order or another log"""
    t = targets.rpn_targets(gold["grids"], gold["padded"], targets_of(gold), **geometry(gold), source=source_of(gold), draw=int(gold["draw"]))
    obj, deltas = dev(gold["rpn_objectness"]).requires_grad_(), dev(gold["rpn_deltas"]).requires_grad_()
    got = targets.rpn_loss(obj, deltas, t)
    (got[0] + got[1]).backward()
    assert got[0].is_cuda and torch.isfinite(obj.grad).all() and torch.isfinite(deltas.grad).all()
    for g, want, tol in zip(got, gold["rpn_loss"], gold["tol_rpn_loss"]):
        print(f"\n[rpn_loss on the device] got {float(g.detach()):.9f} want {want:.9f} tol {tol:.2e}")
        assert abs(float(g.detach()) - want) <= tol


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_limits_raise_value_error_and_the_entry_points_answer_their_codes(gold):
    box = dev(gold["anchors"][:8])
    src = rng.NoiseSource(1, [0])
    with pytest.raises(ValueError):
        targets.match([box], [np.zeros((targets.MAX_GT + 1, 4), F32)], 0.7, 0.3, True)
    with pytest.raises(ValueError):
        targets.match([box], [box], 0.3, 0.7, True)
    with pytest.raises(ValueError):
        targets.match([box[:0]], [box], 0.7, 0.3, True)
    with pytest.raises(ValueError):
        targets.sample([torch.zeros(8, device=DEV)], targets.MAX_BATCH + 1, 0.5, src)
    with pytest.raises(ValueError):
        targets.sample([torch.zeros(8, device=DEV)], 8, 0.5, src, purpose=rng.PURPOSE_STEP)
    with pytest.raises(ValueError):
        targets.sample([torch.zeros(8, device=DEV)] * 2, 8, 0.5, src)
    with pytest.raises(ValueError):
        targets.roi_targets([box], [{"boxes": box[:1], "labels": np.array([1])}])
    import ctypes as C
    h, s = lib.load(), ops.stream_ptr()
    tab = (C.c_int32 * 4)(0, 0, 8, 1)
    w = (C.c_float * 4)(1, 1, 1, 1)
    table, out = torch.tensor([0, 0, 8, 1], dtype=torch.int32, device=DEV), torch.full((64,), -7, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()  # noqa: E731

    def match(**kw):
        a = dict(boxes=P(box), shared=0, gt=P(box), gl=None, th=tab, t=P(table), N=1, high=0.7, low=0.3, allow=1, form=0, w=w, bv=P(out), bi=P(out),
                 part=P(out), words=1, m=P(out), lab=P(out), reg=None)
        a.update(kw)
        return h.edtr_targets_match(*a.values(), s)
    assert match(boxes=None) == -1 and match(N=0) == -2 and match(words=0) == -2 and match(form=5) == -4 and match(boxes=P(box) + 4) == -3
    assert match(th=(C.c_int32 * 4)(0, 0, 8, 1025)) == -5
    assert h.edtr_targets_sample(P(out), 0, tab, P(table), 1, 4097, 0, 1, None, 0, 0, 8, None, P(out), P(out), P(out), P(out), s) == -5
    assert h.edtr_targets_sample(P(out), 0, tab, P(table), 1, 8, 4, 1, None, 0, 0, 3, None, P(out), P(out), P(out), P(out), s) == -4
    assert h.edtr_targets_gather(P(box), P(box), P(out), P(out), tab, P(table), 1, None, 8, w, P(out), P(out), P(out), P(out), s) == -1
    assert h.edtr_targets_encode(P(box), P(box), 0, w, P(out), s) == -2
    torch.cuda.synchronize()
    assert (out == -7).all()                        # nothing was launched
