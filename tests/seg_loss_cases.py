"""The cases the segmentation loss from coarse logits is tested at, shared by tests/test_seg_loss_cpu.py and tests/test_gpu_seg_loss.py:
the case table, the independent fp64 reference, the derived element bound and a second restatement with a switch per seeded defect.

The reference is torch on the CPU in fp64: `F.interpolate(mode="bilinear", align_corners=False)` -> `F.cross_entropy(ignore_index=255)`
-> `backward()`.  For 16-bit logits the rule ROUNDS the blend to the logits' type, which is no continuous function: there the reference
takes the blend's value from `labels.upsample_logits_reference` (normative and tested bit for bit elsewhere) and its derivative from the
fp64 interpolate (straight through the rounding, as torch's own 16-bit chain differentiates), so that a rounding left out shows as an
error and a blend that lands next to a rounding boundary does not.

Shapes: the smallest at which the kernels can still go wrong (the table's comments).  The forward stages a tile's coarse patch while
n (padded to 4) x patch rows x patch columns <= 4096 floats; the backward stages a tile's footprint while it has at most 6144 pixels
and 160 rows and columns: (d) is past the first threshold, (h) past the second, every other case below both."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from edtr_amd import degrade, labels

F32 = np.float32
U = 2.0 ** -24
GRAD_LOSS = 0.37
# Worst error of the device's expf on [-90, 0] and logf on [1, 256] against fp64, in ulps, TWICE what tools/bench_seg_loss.py measured
# on an MI355X (profiles/seg_loss_timing.json "ulp": expf 0.89 -> 1, logf 1.88 -> 2 — the HIP math documentation is not part of the ROCm installation
# this was written on; twice, because not every argument was sampled).  tests/test_seg_loss_cpu.py holds the constants to that file.
ULP_EXP = 2.0
ULP_LOG = 4.0


def _case(name, B, n, ih, iw, H, W, dtype="float32", scale=None, ignore_rows=0, dead_images=(), planted_bad=False, seed=0):
    return dict(name=name, B=B, n=n, ih=ih, iw=iw, H=H, W=W, dtype=dtype, scale=scale, ignore_rows=ignore_rows, dead_images=tuple(dead_images),
                planted_bad=planted_bad, seed=seed)


CASES = [
    _case("a_8x", 2, 21, 8, 8, 64, 64, seed=1),                                       # an integer 8x scale
    _case("a_8x_pm80", 2, 21, 8, 8, 64, 64, scale=80.0, seed=1),                      # ... with logits scaled to +-80
    _case("a_8x_pm100", 2, 21, 8, 8, 64, 64, scale=100.0, seed=1),                    # ... and to +-100, past the 88.7 above which fp32 cannot hold exp(z)
    _case("a_8x_f16", 2, 21, 8, 8, 64, 64, dtype="float16", seed=1),
    _case("a_8x_bf16", 2, 21, 8, 8, 64, 64, dtype="bfloat16", seed=1),
    _case("b_fractional", 2, 21, 5, 7, 37, 50, ignore_rows=3, seed=2),               # partial tiles on both axes, a row pitch that is no multiple of 4
    _case("b_fractional_f16", 2, 21, 5, 7, 37, 50, dtype="float16", ignore_rows=3, seed=2),
    _case("b_fractional_bf16", 2, 21, 5, 7, 37, 50, dtype="bfloat16", ignore_rows=3, seed=2),
    _case("b_fractional_bad", 2, 21, 5, 7, 37, 50, ignore_rows=3, planted_bad=True, seed=2),      # labels in [n, 254]: counted in bad, ignored
    _case("c_down", 1, 3, 9, 9, 5, 6, seed=3),                                        # down-sampling: unreached positions, n padded to 4
    _case("c_down_far", 1, 3, 9, 9, 2, 3, seed=9),                                    # 9 x 9 -> 2 x 3: coarse rows 0, 3, 4, 5, 8 are reached by no pixel ((c)'s own are all reached)
    _case("d_memory", 1, 150, 12, 12, 16, 16, seed=4),                                # a patch that does not fit the stage
    _case("e_one_class", 1, 1, 2, 2, 4, 4, seed=5),                                   # loss exactly 0, gradient exactly 0
    _case("f_tiles", 3, 21, 4, 4, 20, 68, dead_images=(1,), seed=6),                  # two tiles on each axis, image 1 entirely 255
    _case("f_tiles_all_dead", 3, 21, 4, 4, 20, 68, dead_images=(0, 1, 2), seed=6),    # the whole batch at 255: NaN loss, zero gradient
    _case("g_identity", 1, 21, 6, 6, 6, 6, seed=7),                                   # every t is 0: plain cross-entropy
    _case("h_footprint", 1, 5, 3, 3, 81, 80, seed=8),                                 # a footprint of 81 x 80 > 6144 pixels: the backward's memory path
]
CASE_IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def inputs(case):
    """(coarse as fp32 that holds values of the case's type, target uint8): logits 4 N(0, 1), scaled to +-``scale`` where that is set"""
    if "given" in case:                    # (`given`: a case made from tensors a test computed)
        return case["given"]
    rng = np.random.default_rng(case["seed"])
    x = (4.0 * rng.standard_normal((case["B"], case["n"], case["ih"], case["iw"]))).astype(F32)
    if case["scale"]:
        x = (x * F32(case["scale"] / np.abs(x).max())).astype(F32)
    x = labels._round_to(x, case["dtype"])
    t = rng.integers(0, case["n"], (case["B"], case["H"], case["W"])).astype(np.uint8)
    t[rng.random(t.shape) < 0.05] = 255
    if case["planted_bad"]:
        where = rng.random(t.shape) < 0.1
        t[where] = rng.integers(case["n"], 255, int(where.sum())).astype(np.uint8)
    if case["ignore_rows"]:
        t[0, :case["ignore_rows"]] = 255
    for b in case["dead_images"]:
        t[b] = 255
    return x, t


def given(name, coarse, target, dtype="float32"):
    """registers (and returns) a case whose inputs are these arrays, so that `reference` and `bounds` serve it too"""
    coarse, target = np.ascontiguousarray(coarse, dtype=F32), np.ascontiguousarray(target, dtype=np.uint8)
    B, n, ih, iw = coarse.shape
    BY_NAME[name] = dict(_case(name, B, n, ih, iw, target.shape[1], target.shape[2], dtype=dtype), given=(coarse, target))
    return BY_NAME[name]


def keep_mask(case, target):
    return (target != 255) & (target < case["n"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64: dict(loss, lse [B, H, W], grad [B, n, ih, iw] for the upstream gradient GRAD_LOSS, z [B, n, H, W], count)"""
    case = BY_NAME[name]
    x, t = inputs(case)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    z = F.interpolate(xt, size=(case["H"], case["W"]), mode="bilinear", align_corners=False)
    if case["dtype"] != "float32":
        ruled = torch.tensor(labels.upsample_logits_reference(x, (case["H"], case["W"]), case["dtype"]), dtype=torch.float64)
        z = z + (ruled - z).detach()
    tt = torch.tensor(np.where(keep_mask(case, t), t, 255).astype(np.int64))
    count = int((tt != 255).sum())
    loss = F.cross_entropy(z, tt, ignore_index=255)
    if count:
        (GRAD_LOSS * loss).backward()
    grad = xt.grad.numpy() if xt.grad is not None else np.zeros(x.shape)
    return dict(loss=loss.item(), lse=torch.logsumexp(z, dim=1).detach().numpy(), grad=grad, z=z.detach().numpy(), count=count)


def _axis(n_in, n_out):
    """(A, I) fp64 [n_out, n_in] of one axis by the rule's fp32 taps: the blend's weights, and 1 at both taps of every output index"""
    i0, t = degrade._index_lambda(np.maximum(degrade._source_index(n_in, n_out), F32(0)), n_in)
    i1 = i0 + (i0 < n_in - 1)
    A, I = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    for y in range(n_out):
        A[y, i0[y]] += 1.0 - float(t[y])
        A[y, i1[y]] += float(t[y])
        I[y, i0[y]] = I[y, i1[y]] = 1.0
    return A, I


@functools.lru_cache(maxsize=None)
def bounds(name):
    """dict(loss, lse [B, H, W], grad [B, n, ih, iw]): what a correct fp32 evaluation of the rule may differ from `reference` by.  Each is
    (a count of rounded operations on the path) x 2^-24 x (the same forward or backward applied to absolute values).  With M the largest
    |logit| and u = 2^-24:
      z     7 u A|x| for the blend's seven operations (A: the blend) + 16 u max(ih, iw) M for the source index, which the rule forms in fp32
            and torch's fp64 chain in fp64: three rounded steps move a lambda by at most 4 u (extent), on each axis, between two logits
            that differ by at most 2 M.  Zero for 16-bit logits, whose reference takes the rule's own rounded blend.
      lse   max_c E_z + u [4 M + n (2 ULP_EXP + 3)] + 2 u ULP_LOG ln n + u (|lse| + 1): every addend exp(z_c - m) carries the rounding of its
            argument (<= 2 M u) and, in the launch's running form, the roundings of the rescales' arguments, which telescope to
            m_last - m_first <= 2 M; per plane at most one rescale (a product, an expf) and one sum; logf of a value in [1, n]; the last sum.
      loss  the mean over the counted pixels of E_lse + E_z[target] + u |lse - z_t|, + 2 u |loss| (the fp64 sums are exact to 2^-53)
      grad  the adjoint applied to E_e, the error of e = (p - [c == t]) g with p = exp(z_c - lse): g p (E_z + E_lse + u |z_c - lse| + 2 u ULP_EXP)
            + 4 u |e|;  + u (rows that reach i + columns that reach j + 6) x the adjoint of |e| for the two-level sum and the products;
            + 4 u (iw + ih) x the adjoint of |e| with the weights of one axis replaced by 1 at both taps, for the lambdas (as under z).
            A 16-bit gradient adds half an ulp of its type at the value that is rounded: u16 (|want| + bound), u16 = 2^-8 / 2^-11 (+ 2^-25
            for float16's subnormals)."""
    case = BY_NAME[name]
    ref = reference(name)
    x, t = inputs(case)
    n, ih, iw = case["n"], case["ih"], case["iw"]
    keep = keep_mask(case, t)
    M = float(np.abs(x).max())
    (Ay, Iy), (Ax, Ix) = _axis(ih, case["H"]), _axis(iw, case["W"])
    def adj(ay, v, ax):
        return np.einsum("yi,bnyx,xj->bnij", ay, v, ax)
    Ez = np.zeros(ref["z"].shape)
    if case["dtype"] == "float32":
        Ez = U * (7.0 * np.einsum("yi,bnij,xj->bnyx", Ay, np.abs(x).astype(np.float64), Ax) + 16.0 * max(ih, iw) * M)
    Else = Ez.max(axis=1) + U * (4.0 * M + n * (2.0 * ULP_EXP + 3.0)) + 2.0 * U * ULP_LOG * np.log(n) + U * (np.abs(ref["lse"]) + 1.0)
    tt = np.minimum(t, n - 1).astype(np.int64)
    zt = np.take_along_axis(ref["z"], tt[:, None], axis=1)[:, 0]
    Ezt = np.take_along_axis(Ez, tt[:, None], axis=1)[:, 0]
    Eell = Else + Ezt + U * np.abs(ref["lse"] - zt)
    out = dict(lse=Else, loss=float("nan"), grad=np.zeros(x.shape))
    if ref["count"]:
        out["loss"] = float(Eell[keep].mean() + 2.0 * U * abs(ref["loss"]))
        g = GRAD_LOSS / ref["count"]
        p = np.exp(ref["z"] - ref["lse"][:, None])
        e = np.abs(p - (np.arange(n)[None, :, None, None] == tt[:, None])) * g * keep[:, None]
        Ee = (g * p * (Ez + Else[:, None] + U * np.abs(ref["z"] - ref["lse"][:, None]) + 2.0 * U * ULP_EXP)) * keep[:, None] + 4.0 * U * e
        K = Iy.sum(0)[:, None] + Ix.sum(0)[None, :] + 6.0
        Eg = adj(Ay, Ee, Ax) + U * K * adj(Ay, e, Ax) + 4.0 * U * (iw * adj(Ay, e, Ix) + ih * adj(Iy, e, Ax))
        u16 = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}[case["dtype"]]
        out["grad"] = Eg + u16 * (np.abs(ref["grad"]) + Eg) + (2.0 ** -25 if case["dtype"] == "float16" else 0.0)
    return out


def ratios(name, loss, lse, grad):
    """(loss, lse, grad) error / bound against `reference`, the worst element of each (0 where both are 0; inf where only the bound is)"""
    ref, bnd = reference(name), bounds(name)
    def worst(err, b):
        err, b = np.asarray(err, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / b)
        return float(np.max(q)) if q.size else 0.0
    r_loss = 0.0 if not ref["count"] else worst(abs(float(loss) - ref["loss"]), bnd["loss"])
    return r_loss, worst(np.abs(np.asarray(lse, dtype=np.float64) - ref["lse"]), bnd["lse"]), worst(np.abs(np.asarray(grad, dtype=np.float64) - ref["grad"]), bnd["grad"])


DEFECTS = ("edge_once", "swap", "count_ignored", "no_max", "no_round", "skip_column")
DEFECT_CASE = {"edge_once": "a_8x", "swap": "b_fractional", "count_ignored": "b_fractional", "no_max": "a_8x_pm80", "no_round": "b_fractional_bf16",
               "skip_column": "a_8x"}           # ("plain_sum" is no defect of these six: see `restatement_copy` and the CPU test)


def _axis_copy(n_in, n_out, defect):
    """fp32 [n_out, n_in] weights of one axis.  "edge_once": where the clamp puts both taps on the last position only 1 - t lands there;
    "swap": t at the first tap and 1 - t at the second"""
    i0, t = degrade._index_lambda(np.maximum(degrade._source_index(n_in, n_out), F32(0)), n_in)
    i1 = i0 + (i0 < n_in - 1)
    A = np.zeros((n_out, n_in), dtype=F32)
    for y in range(n_out):
        w0, w1 = (t[y], F32(1) - t[y]) if defect == "swap" else (F32(1) - t[y], t[y])
        A[y, i0[y]] += w0
        if not (defect == "edge_once" and i0[y] == i1[y]):
            A[y, i1[y]] += w1
    return A


def restatement_copy(case, defect=None):
    """The rule of the two restatements once more, through dense per-axis weight matrices in fp32 (its sums in another order: inside the
    bound, not equal in bits), with a switch per seeded defect ("swap" acts on the columns only).  Returns (loss, lse, grad for GRAD_LOSS)."""
    x, t = inputs(case)
    n = case["n"]
    Ay, Ax = _axis_copy(case["ih"], case["H"], None if defect == "swap" else defect), _axis_copy(case["iw"], case["W"], defect)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        # (16-bit logits: the blend by the rule itself unless the defect is in the weights — a blend that differs in its last fp32 bit can
        # round to the other 16-bit neighbour, which is a whole 16-bit ulp and no rounding error of this copy's)
        z = np.einsum("yi,bnij,xj->bnyx", Ay, x, Ax).astype(F32) if defect in ("edge_once", "swap") or case["dtype"] == "float32" \
            else labels.upsample_logits_reference(x, (case["H"], case["W"]), "float32")
        if defect != "no_round":
            z = labels._round_to(z, case["dtype"])
        # "no_max": the subtraction inside exp is left out of lse = m + log(sum_c exp(z_c - m)), the one omission that makes the value
        # wrong (by m).  "plain_sum" leaves out the addition of m as well: log(sum_c exp(z_c)), the SAME value on paper and, while fp32
        # holds every exp(z_c) (-87.3 < z < 88.7), as accurate as the rule, so no defect there and none that a bound could reject; past
        # that range it overflows.
        m = np.zeros(z[:, 0].shape, dtype=F32) if defect == "plain_sum" else z.max(axis=1)
        inside = np.zeros_like(m) if defect == "no_max" else m
        s = np.zeros_like(m)
        for c in range(n):
            s = s + np.exp(z[:, c] - inside)
        lse = (m + np.log(s)).astype(F32)
        keep = keep_mask(case, t)
        seen = np.ones_like(keep)
        if defect == "skip_column":
            seen[:, :, 63::64] = False
            lse = np.where(seen, lse, F32(0))
        counted = keep & seen
        tt = np.minimum(t, n - 1).astype(np.int64)
        ell = (lse - np.take_along_axis(z, tt[:, None], axis=1)[:, 0]).astype(F32)
        count = int(seen.sum()) if defect == "count_ignored" else int(counted.sum())
        loss = F32(ell[counted].astype(np.float64).sum() / count) if count else F32(np.nan)
        g = F32(GRAD_LOSS) / F32(max(count, 1))
        e = ((np.exp(z - lse[:, None]) - (np.arange(n)[None, :, None, None] == tt[:, None]).astype(F32)) * g).astype(F32) * counted[:, None]
        grad = labels._round_to(np.einsum("yi,bnyx,xj->bnij", Ay, e, Ax).astype(F32), case["dtype"])
    return loss, lse, grad


def check_rejections(h):
    """`edtr_seg_ce_forward` / `edtr_seg_ce_backward` by return code only.  Every call fails before its stand-in pointers are used, so
    nothing is launched."""
    p = 4096
    NULL, SHAPE, ALIGN, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -5
    need = h.edtr_seg_ce_workspace(2, 37, 50)
    assert need == 16 * 2 * 3 * 1 and h.edtr_seg_ce_workspace(0, 4, 4) == 0 and h.edtr_seg_ce_workspace(1, 16, 65) == 32

    def fwd(**kw):
        a = dict(dt=0, coarse=p, B=2, n=21, ih=5, iw=7, target=p, H=37, W=50, ignore=255, lse=p, ws=p, ws_bytes=need, loss=p, counts=p, max_blocks=0)
        a.update(kw)
        return h.edtr_seg_ce_forward(*a.values(), None)

    def bwd(**kw):
        a = dict(dt=0, coarse=p, B=2, n=21, ih=5, iw=7, target=p, H=37, W=50, ignore=255, lse=p, counts=p, grad_loss=p, grad=p, max_blocks=0)
        a.update(kw)
        return h.edtr_seg_ce_backward(*a.values(), None)
    for name in ("coarse", "target", "lse", "ws", "loss", "counts"):
        assert fwd(**{name: None}) == NULL, name
    for name in ("coarse", "target", "lse", "counts", "grad_loss", "grad"):
        assert bwd(**{name: None}) == NULL, name
    for f in (fwd, bwd):
        assert f(dt=3) == DTYPE and f(n=257) == UNSUPPORTED and f(H=(1 << 24) + 1) == UNSUPPORTED
        for name in ("B", "n", "ih", "iw", "H", "W"):
            assert f(**{name: 0}) == SHAPE, name
        assert f(max_blocks=-1) == SHAPE and f(coarse=p + 2) == ALIGN and f(dt=2, coarse=p + 1) == ALIGN and f(lse=p + 2) == ALIGN and f(counts=p + 4) == ALIGN
        # a NULL before the dtype before a shape before a cap before an alignment
        assert f(coarse=None, dt=3) == NULL and f(dt=3, n=0) == DTYPE and f(n=0, H=(1 << 24) + 1) == SHAPE and f(n=257, coarse=p + 2) == UNSUPPORTED
    assert fwd(ws_bytes=need - 1) == SHAPE and fwd(ws=p + 4) == ALIGN and fwd(loss=p + 2) == ALIGN
    assert bwd(grad=p + 2) == ALIGN and bwd(grad_loss=p + 2) == ALIGN and bwd(dt=1, grad=p + 1) == ALIGN
