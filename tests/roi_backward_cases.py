"""The cases RoIAlign's backward is tested at, shared by tests/test_roi_backward_cpu.py and tests/test_gpu_roi_backward.py, and the
two independent restatements the CPU test holds `rois.roi_align_backward_reference` against:
  * `backward_copy`: the rule of that restatement once more, pixel row by pixel row in scalar fp32 steps, with a switch per seeded defect;
  * `forward_fp64`: a differentiable fp64 torch forward written from `rois._taps` (index gathers and weights, no grid_sample), whose
    autograd gives the gradient in real arithmetic up to fp64 rounding, and the derived element bound.

Shapes: the smallest at which the gather can still go wrong.  Two levels of 20 x 23 and 10 x 12 (no extent a multiple of the 16-pixel
tile: the first level has four tiles with ragged edges, the second one ragged tile), strides 4 and 8 from the larger image of 80 x 92,
N = 2, C = 70 (two 32-channel chunks and a tail of 6; 64 + 6 for a 64-channel chunk), (P, S) = (7, 2) and (2, 3); one single-level
case with C = 3, P = S = 1.  The canonical scale is 56, so that boxes of this size fall on both levels."""
import numpy as np
import torch

from edtr_amd import rois

F32 = np.float32
CANONICAL = (56.0, 4.0)
LEVELS = ((20, 23), (10, 12))
IMAGE_SIZES = [(80, 92), (72, 88)]          # the scales come from the larger extent: 1 / 4 and 1 / 8

# x1, y1, x2, y2 in image coordinates.  sqrt(area) < 28 pools from level 0 (scale 1 / 4), the others from level 1 (scale 1 / 8).
BOXES = np.array([
    [55.0, 52.0, 75.0, 74.0],               # overlaps the next one across the corner (16, 16) of level 0's four tiles
    [58.5, 57.25, 79.5, 76.0],
    [-14.0, -10.0, 6.0, 5.0],               # level 0, partly outside above and left: samples below -1 are invalid
    [80.0, 70.0, 99.0, 86.0],               # level 0, partly outside below and right: invalid past the extent, rows 19 / columns 22 clamped (low == high)
    [33.0, 41.0, 34.5, 42.0],               # smaller than a pixel of level 0: every bin falls on the same pixels
    [0.0, 0.0, 92.0, 80.0],                 # the whole map, level 1
    [0.0, 0.0, 0.0, 0.0],                   # an unfilled slot of roi_targets: sqrt(area) = 0, level 0
    [10.0, 8.0, 50.0, 44.0],                # level 1, inside
    [-30.0, -25.0, 20.0, 12.0],             # level 1, partly outside above and left
    [60.0, 50.0, 120.0, 95.0],              # level 1, partly outside below and right, clamped rows and columns
], dtype=F32)
BOX_LEVEL = [0, 0, 0, 0, 0, 1, 0, 1, 1, 1]


def _case(name, levels, image_sizes, C, P, S, per_image, canonical, seed, single=False):
    K = sum(r.shape[0] for r in per_image)
    rng = np.random.default_rng(seed)
    grad = rng.standard_normal((K, C, P, P)).astype(F32)
    if single:                              # one non-zero element: a misplaced tap shows as a misplaced pixel
        value = grad[1, C - 1, P - 1, P // 2]
        grad = np.zeros_like(grad)
        grad[1, C - 1, P - 1, P // 2] = value
    shapes = [(len(image_sizes), C, H, W) for H, W in levels]
    return dict(name=name, shapes=shapes, image_sizes=list(image_sizes), C=C, P=P, S=S, rois=[np.ascontiguousarray(r, dtype=F32) for r in per_image],
                canonical_scale=canonical[0], canonical_level=canonical[1], grad=grad)


NONE = np.zeros((0, 4), dtype=F32)
SINGLE_BOXES = np.array([[3.0, 2.0, 30.0, 29.0], [0.0, 0.0, 0.0, 0.0], [-9.0, 20.0, 12.0, 41.0], [40.0, 30.0, 47.0, 36.0], [17.0, 9.0, 17.5, 9.25]], dtype=F32)
CASES = [
    _case("p7s2_image1_empty", LEVELS, IMAGE_SIZES, 70, 7, 2, [BOXES, NONE], CANONICAL, 1),
    _case("p2s3_image0_empty", LEVELS, IMAGE_SIZES, 70, 2, 3, [NONE, BOXES], CANONICAL, 2),
    _case("p7s2_both_images", LEVELS, IMAGE_SIZES, 70, 7, 2, [BOXES[[0, 5, 2, 1]], BOXES[[7, 0, 1, 3, 6, 9]]], CANONICAL, 3),
    _case("p7s2_one_element", LEVELS, IMAGE_SIZES, 70, 7, 2, [BOXES[[0, 1, 5]], BOXES[[1, 0, 8]]], CANONICAL, 4, single=True),
    _case("one_level_p1s1", ((9, 11),), [(36, 44)], 3, 1, 1, [SINGLE_BOXES], (224.0, 4.0), 5),
]
CASE_IDS = [c["name"] for c in CASES]


def self_check():
    """what the table promises: every level is certain (`roi_levels_reference` warns of log2 next to an integer), both levels are
    used, an image is empty, invalid samples and clamped edges occur"""
    for case in CASES:
        flat = np.concatenate(case["rois"]).astype(np.float64)
        if len(case["shapes"]) > 1:
            s = np.sqrt((flat[:, 2] - flat[:, 0]) * (flat[:, 3] - flat[:, 1]))
            with np.errstate(divide="ignore"):
                v = case["canonical_level"] + np.log2(s / case["canonical_scale"])
            finite = np.isfinite(v)
            assert np.all(np.abs(v[finite] - np.round(v[finite])) >= 1e-3), case["name"]
    lv = rois.roi_levels_reference(BOXES, 2, 3, *CANONICAL)
    assert lv.tolist() == BOX_LEVEL
    assert any(r.shape[0] == 0 for r in CASES[0]["rois"]) and any(r.shape[0] == 0 for r in CASES[1]["rois"])
    seen = set()
    for _, _, _, H, W, ty, tx in per_roi(CASES[0]):
        for (valid, low, high, l, h), extent in ((ty, H), (tx, W)):
            seen |= {"invalid"} if (~valid).any() else set()
            seen |= {"clamped"} if (valid & (low == high) & (low == extent - 1)).any() else set()
    assert seen == {"invalid", "clamped"}


def per_roi(case):
    """(k, image, level, H, W, taps_y, taps_x) of every roi as `roi_align_reference` works them out; each tap table is (valid, low, high,
    l, h) of shape [P, S]"""
    shapes, P, S = case["shapes"], case["P"], case["S"]
    boxes = np.concatenate(case["rois"])
    batch = np.concatenate([np.full(r.shape[0], n) for n, r in enumerate(case["rois"])]).astype(np.int64)
    scales, k_min, k_max = rois.level_scales([s[-2:] for s in shapes], case["image_sizes"])
    levels = rois.roi_levels_reference(boxes, k_min, k_max, case["canonical_scale"], case["canonical_level"]) if len(shapes) > 1 \
        else np.zeros(boxes.shape[0], dtype=np.int64)
    out = []
    for k in range(boxes.shape[0]):
        lvl = int(levels[k])
        H, W = shapes[lvl][-2:]
        with np.errstate(invalid="ignore", over="ignore"):
            b = (boxes[k:k + 1] * F32(scales[lvl])).astype(F32)
            ew, eh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
            roi_w, roi_h = np.where(ew < 1, F32(1), ew), np.where(eh < 1, F32(1), eh)
            ty = tuple(v[0] for v in rois._taps(b[:, 1], (roi_h / F32(P)).astype(F32), P, S, H))
            tx = tuple(v[0] for v in rois._taps(b[:, 0], (roi_w / F32(P)).astype(F32), P, S, W))
        out.append((k, int(batch[k]), lvl, H, W, ty, tx))
    return out


DEFECTS = ("swap", "no_division", "invalid_counted", "edge_once")


def _weights_copy(taps, extent, P, S, defect):
    """a[y][ph], scalar step by scalar step.  Defects: "swap" adds l at low and h at high; "invalid_counted" forgets the validity;
    "edge_once" adds, where low == high at the clamped edge, only the high tap's l = 0 and so loses the weight 1 of that row."""
    valid, low, high, l, h = taps
    a = np.zeros((extent, P), dtype=F32)
    for ph in range(P):
        for i in range(S):
            if not valid[ph, i] and defect != "invalid_counted":
                continue
            wl, wh = (h[ph, i], l[ph, i]) if defect == "swap" else (l[ph, i], h[ph, i])
            if not (defect == "edge_once" and low[ph, i] == high[ph, i]):
                a[low[ph, i], ph] = F32(a[low[ph, i], ph] + wh)
            a[high[ph, i], ph] = F32(a[high[ph, i], ph] + wl)
    return a


def backward_copy(case, defect=None, dtype="float32"):
    """`rois.roi_align_backward_reference` written a second time: every zero term included, every pixel of the map visited"""
    from edtr_amd import labels
    P, S, C = case["P"], case["S"], case["C"]
    out = [np.zeros(s, dtype=F32) for s in case["shapes"]]
    for k, n, lvl, H, W, ty, tx in per_roi(case):
        a, b = _weights_copy(ty, H, P, S, defect), _weights_copy(tx, W, P, S, defect)
        g = case["grad"][k] if defect == "no_division" else (case["grad"][k] / F32(S * S)).astype(F32)
        t = np.zeros((C, P, W), dtype=F32)
        for pw in range(P):
            t = (t + (b[None, None, :, pw] * g[:, :, pw, None]).astype(F32)).astype(F32)
        contrib = np.zeros((C, H, W), dtype=F32)
        for ph in range(P):
            contrib = (contrib + (a[None, :, ph, None] * t[:, ph, None, :]).astype(F32)).astype(F32)
        out[lvl][n] = (out[lvl][n] + contrib).astype(F32)
    return [labels._round_to(o, dtype) for o in out]


def forward_fp64(case, features):
    """The forward of `roi_align_reference` in fp64 torch from the fp32 tap tables of `_taps`: differentiable in ``features`` (per
    level fp64 [N, C, H, W]).  [K, C, P, P]."""
    P, S = case["P"], case["S"]
    rows = []
    for k, n, lvl, H, W, ty, tx in per_roi(case):
        f = features[lvl][n]                                               # [C, H, W]
        vy, y0, y1, ly, hy = (torch.from_numpy(np.ascontiguousarray(v)) for v in ty)
        vx, x0, x1, lx, hx = (torch.from_numpy(np.ascontiguousarray(v)) for v in tx)
        ly, hy, lx, hx = ly.double() * vy, hy.double() * vy, lx.double() * vx, hx.double() * vx      # [P, S]; an invalid tap weighs nothing
        def at(yy, xx):                                                     # [C, P, S, P, S]
            return f[:, yy[:, :, None, None], xx[None, None, :, :]]
        def wt(wy, wx):
            return wy[:, :, None, None] * wx[None, None, :, :]
        val = wt(hy, hx) * at(y0, x0) + wt(hy, lx) * at(y0, x1) + wt(ly, hx) * at(y1, x0) + wt(ly, lx) * at(y1, x1)
        rows.append(val.sum(dim=(2, 4)) / float(S * S))
    return torch.stack(rows)


def backward_fp64(case, grad):
    """the gradient of <forward_fp64(f), grad> in f by fp64 autograd: per level fp64 [N, C, H, W]"""
    feats = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in case["shapes"]]
    (forward_fp64(case, feats) * torch.as_tensor(grad).double()).sum().backward()
    return [f.grad.numpy() if f.grad is not None else np.zeros(tuple(f.shape)) for f in feats]


def bounds(case, dtype="float32"):
    """(want, bound) per level.  want: `backward_fp64` of the case's gradient.  bound, per element: n_ops 2^-24 B, with B the same
    backward of |grad| — the weights are non-negative, so that is the sum of the absolute terms — and n_ops = (rois of that image) +
    2 P + 2 S + 8: one rounding per roi summed, per bin summed on each axis (2 P), per sample summed into a weight on each axis
    (2 S), and the division, the two products, and the roundings of the weights' own l and h (8 covers them).  A 16-bit output adds half
    an ulp of the output type at the value that is rounded, the fp32 sum: at most u (|want| + the fp32 bound) with u = 2^-8 for
    bfloat16 and 2^-11 for float16 (+ 2^-25, half the spacing of its subnormals)."""
    want = backward_fp64(case, case["grad"])
    B = backward_fp64(case, np.abs(case["grad"]))
    per_image = np.array([r.shape[0] for r in case["rois"]], dtype=np.float64)
    n_ops = per_image + 2 * case["P"] + 2 * case["S"] + 8
    u = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}[dtype]
    floor = 2.0 ** -25 if dtype == "float16" else 0.0
    fp32 = [n_ops[:, None, None, None] * 2.0 ** -24 * b for b in B]
    return want, [e + u * (np.abs(w) + e) + floor for w, e in zip(want, fp32)]


def check_rejections(h):
    """`edtr_roi_align_backward` by return code only: the checks of `edtr_roi_align` in its order, then the new ones.  Every call fails
    before its stand-in pointers are used, so nothing is launched."""
    import ctypes as C
    p = 4096
    NULL, SHAPE, ALIGN, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -5
    from edtr_amd import lib

    def ptrs(*v):
        return (C.c_void_p * len(v))(*v)
    hw, sc = (C.c_int32 * 2)(4, 4), (C.c_float * 1)(0.25)
    need = h.edtr_roi_align_backward_workspace(1, 5, 7, 2)
    assert need == 4 * (4 + 5 * (8 + 8 * 14)) and h.edtr_roi_align_backward_workspace(1, 0, 7, 2) == 0

    def back(**kw):
        a = dict(dt=0, outs=ptrs(p), hw=hw, scales=sc, L=1, N=1, C=8, rois=p, batch=p, K=5, P=7, S=2, k_min=2, k_max=2, s0=224.0, k0=4.0, grad=p,
                 ws=p, ws_bytes=need)
        a.update(kw)
        return h.edtr_roi_align_backward(*a.values(), None)
    assert back(outs=None) == NULL and back(rois=None) == NULL and back(batch=None) == NULL and back(grad=None) == NULL and back(ws=None) == NULL
    assert back(outs=ptrs(None)) == NULL and back(hw=None) == NULL and back(scales=None) == NULL
    assert back(K=0) == SHAPE and back(C=0) == SHAPE and back(P=0) == SHAPE and back(S=0) == SHAPE and back(hw=(C.c_int32 * 2)(0, 4)) == SHAPE
    assert back(scales=(C.c_float * 1)(0.0)) == SHAPE and back(s0=0.0) == SHAPE and back(k_max=1) == SHAPE
    assert back(L=9) == UNSUPPORTED and back(N=65536) == UNSUPPORTED and back(P=9, S=8) == UNSUPPORTED
    assert back(dt=5) == DTYPE and back(rois=p + 8) == ALIGN and back(outs=ptrs(p + 2)) == ALIGN and back(dt=2, outs=ptrs(p + 1)) == ALIGN
    # the order of the forward's checks: a NULL before a bad shape before a cap before the dtype before an alignment
    assert back(rois=None, K=0) == NULL and back(K=0, L=9) == SHAPE and back(L=9, dt=5) == UNSUPPORTED and back(dt=5, rois=p + 8) == DTYPE
    # the new ones: the cap on P, the gradient's and the workspace's alignment, the workspace's size
    # (P at the cap itself is accepted; it is not tried here, where a call that passes every check would launch on the stand-ins)
    assert lib.ROI_BWD_MAX_P == 16
    assert back(P=lib.ROI_BWD_MAX_P + 1, S=1, ws_bytes=1 << 20) == UNSUPPORTED and back(P=17, S=3) == UNSUPPORTED
    assert back(grad=p + 2) == ALIGN and back(ws=p + 8) == ALIGN and back(ws_bytes=need - 1) == SHAPE and back(ws_bytes=0) == SHAPE
