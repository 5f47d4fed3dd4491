"""The cases the training losses are tested at, shared by tests/test_losses_cpu.py and tests/test_gpu_losses.py: the case tables, the
independent fp64 references, the derived bounds and a second restatement of each loss with a switch per seeded defect.

The references are torch on the CPU in fp64: `F.l1_loss(reduction="mean") * w` summed over the pairs, and `F.cross_entropy(reduction=
"mean", ignore_index=)`, each followed by `backward()` with the upstream gradient GRAD_LOSS.  16-bit inputs are widened exactly.

Shapes: the smallest at which the kernels can still go wrong (the tables' comments).  The L1 launch sums chunks of 4096 elements, a lane
owning four consecutive elements of each 1024-element quarter, and folds a pair's chunk partials 256 at a time; the cross-entropy
launch gives a row to one wave of 64 lanes."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from edtr_amd import labels, losses

F32 = np.float32
U = 2.0 ** -24
GRAD_LOSS = 0.37
IGNORE = -100
# Worst error of the device's expf on [-90, 0] and logf on [1, 65536] against fp64, in ulps, TWICE what was measured on an MI355X:
# expf from profiles/seg_loss_timing.json (0.89 -> 1), logf from profiles/losses_timing.json (tools/bench_losses.py; the sum of a row of up
# to 65536 terms lies in [1, 65536], and seg_loss_timing.json covers [1, 256] only).  Twice, because not every argument was sampled.
# tests/test_losses_cpu.py holds the constants to those files.
ULP_EXP = 2.0
ULP_LOG = 4.0
U16 = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}      # half an ulp of the type, relative


# ---- the weighted mean-L1 ----------------------------------------------------------------------------------------------------------
def _pair(n, dtype="float32", offset=0, equal=0, nan=False, need_a=True, need_b=False):
    return dict(n=n, dtype=dtype, offset=offset, equal=equal, nan=nan, need_a=need_a, need_b=need_b)


def _l1(name, pairs, weights=None, seed=0):
    return dict(name=name, pairs=pairs, weights=[1.0] * len(pairs) if weights is None else list(weights), seed=seed)


L1_CASES = [
    _l1("n1", [_pair(1)], seed=1),                                                   # below one vector
    _l1("n3", [_pair(3)], [0.75], seed=2),
    _l1("n4095", [_pair(4095)], seed=3),                                             # the chunk edge
    _l1("n4096", [_pair(4096)], seed=4),
    _l1("n4097", [_pair(4097)], seed=5),
    _l1("tail", [_pair(3 * 4096 + 5)], [0.5], seed=6),                               # a tail that is no multiple of 4
    _l1("fold", [_pair(300 * 4096 + 7)], seed=7),                                    # more than 256 chunks: the fold's lane stride, grid rounds under max_blocks = 2
    _l1("f16_odd", [_pair(5003, "float16")], seed=8),                                # 16-bit tails
    _l1("bf16_odd", [_pair(4101, "bfloat16")], [2.0], seed=9),
    _l1("views", [_pair(4100, offset=1), _pair(4099, "float16", offset=1)], seed=10),    # operands one element into their buffers: element loads
    _l1("mixed5", [_pair(9001), _pair(4096 + 130, "bfloat16"), _pair(17), _pair(2 * 4096, "float16"), _pair(4097 + 2)],
        [0.5, 0.25, 1.0, 0.0, 2.0], seed=11),                                        # the multi-pair launch, a zero weight among them
    _l1("equal", [_pair(4200, equal=37, need_b=True), _pair(515, "bfloat16", equal=9, need_b=True)], seed=12),   # zeros in both gradients
    _l1("nan", [_pair(4200, nan=True, need_b=True)], seed=13),                       # NaN loss, +0.0 / -0.0 gradient there
    _l1("optional", [_pair(4500, need_a=True, need_b=True), _pair(700, need_a=False, need_b=True), _pair(33, need_a=False, need_b=False)],
        [1.0, 0.5, 3.0], seed=14),                                                   # grad_b too, grad_b only, a pair that is skipped
]
L1_IDS = [c["name"] for c in L1_CASES]
L1_BY_NAME = {c["name"]: c for c in L1_CASES}


@functools.lru_cache(maxsize=None)
def l1_inputs(name):
    """[(a, b)] as fp32 arrays that hold values of each pair's type: N(0, 1), with the planted equal elements and NaN"""
    case = L1_BY_NAME[name]
    if "given" in case:                    # (`l1_given`: a case made from tensors a test computed)
        return case["given"]
    rng = np.random.default_rng(case["seed"])
    out = []
    for p in case["pairs"]:
        a = labels._round_to(rng.standard_normal(p["n"]).astype(F32), p["dtype"])
        b = labels._round_to(rng.standard_normal(p["n"]).astype(F32), p["dtype"])
        if p["equal"]:
            at = rng.choice(p["n"], p["equal"], replace=False)
            b[at] = a[at]
            a[at[0]] = b[at[0]] = F32(0.0)                  # 0 - 0 among them
        if p["nan"]:
            a[p["n"] // 2] = np.nan
        a.setflags(write=False), b.setflags(write=False)
        out.append((a, b))
    return out


def l1_given(name, pairs, weights, dtypes):
    """registers (and returns) a case whose inputs are these arrays, so that `l1_reference` and `l1_bounds` serve it too"""
    pairs = [(np.ascontiguousarray(a, dtype=F32).reshape(-1), np.ascontiguousarray(b, dtype=F32).reshape(-1)) for a, b in pairs]
    L1_BY_NAME[name] = dict(_l1(name, [_pair(a.size, dt) for (a, _), dt in zip(pairs, dtypes)], weights), given=pairs)
    return L1_BY_NAME[name]


def l1_dtypes(case):
    return [p["dtype"] for p in case["pairs"]]


@functools.lru_cache(maxsize=None)
def l1_reference(name):
    """fp64: dict(loss, terms [pairs], grad_a, grad_b: lists of fp64 arrays for the upstream gradient GRAD_LOSS, mean_abs [pairs])"""
    case = L1_BY_NAME[name]
    ts = [(torch.tensor(a, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True)) for a, b in l1_inputs(name)]
    terms = [F.l1_loss(a, b, reduction="mean") for a, b in ts]
    loss = sum(t * w for t, w in zip(terms, case["weights"]))
    (GRAD_LOSS * loss).backward()
    return dict(loss=loss.item(), terms=np.array([t.item() for t in terms]), grad_a=[a.grad.numpy() for a, _ in ts], grad_b=[b.grad.numpy() for _, b in ts])


def l1_depth(n, pairs):
    """the number of fp64 additions an element's difference passes through in the stated order: 16 in its lane and 8 in the tree of its
    chunk, ceil(chunks / 256) in the fold's lane and 8 in its tree, and the sum over the pairs"""
    chunks = -(-n // losses.L1_CHUNK)
    return 16 + 8 + -(-chunks // 256) + 8 + pairs


def l1_bounds(name):
    """dict(loss, terms [pairs]): what a correct evaluation of the rule may differ from `l1_reference` by, u = 2^-24.
    The operands hold fp32 (or narrower) values, so the exact difference of a pair of elements is a real number whose fp32 rounding,
    the rule's ONE rounded subtraction, is off by at most u |d|; |.| and the widening to fp64 are exact.  Every |d| then passes through
    D = `l1_depth` fp64 additions, each off by at most 2^-53 of its result, and all addends are non-negative, so the sum is off by at
    most (u + D 2^-53) sum |d| to first order.  The division by n and the product with w are two more fp64 roundings, below the
    first-order terms dropped.  Per pair that is |w| mean|d| (u + D 2^-53); the loss adds u |loss| for its rounding to fp32, a term
    u |term| for its own."""
    case, ref = L1_BY_NAME[name], l1_reference(name)
    k = len(case["pairs"])
    rel = np.array([U + l1_depth(p["n"], k) * 2.0 ** -53 for p in case["pairs"]])
    per_pair = np.abs(ref["terms"]) * rel
    return dict(loss=float(np.sum(np.abs(case["weights"]) * per_pair) + U * abs(ref["loss"])), terms=per_pair + U * np.abs(ref["terms"]))


def l1_ratio(name, loss, terms):
    """(loss, worst term) error / bound against `l1_reference` (0 where both are 0; a NaN reference wants a NaN)"""
    ref, bnd = l1_reference(name), l1_bounds(name)
    def one(got, want, b):
        if np.isnan(want):
            return 0.0 if np.isnan(got) else float("inf")
        err = abs(float(got) - want)
        return 0.0 if err == 0 else (err / b if b > 0 else float("inf"))
    return one(loss, ref["loss"], bnd["loss"]), max(one(t, w, b) for t, w, b in zip(terms, ref["terms"], bnd["terms"]))


def l1_expected_grads(name):
    """([grad_a], [grad_b]) as fp32 arrays by the rule, from the fp64 reference's signs and an independent c_k: the sign of an fp32
    difference of two fp32 numbers is the sign of their exact difference (it is zero only where they are equal), so torch's fp64
    gradient has the rule's sign pattern; c_k = fp32(fp64(fp32 GRAD_LOSS) fp64(fp32 w_k) / n_k) in Python's doubles, rounded once to a
    16-bit type.  A NaN difference: +0.0 in a, -0.0 in b."""
    case, ref = L1_BY_NAME[name], l1_reference(name)
    ga, gb = [], []
    for p, w, ra in zip(case["pairs"], case["weights"], ref["grad_a"]):
        c = labels._round_to(np.array([F32(float(F32(GRAD_LOSS)) * float(F32(w)) / p["n"])], dtype=F32), p["dtype"])[0]
        with np.errstate(invalid="ignore"):
            s = np.sign(np.nan_to_num(ra, nan=0.0)) * np.sign(w if w != 0 else 1.0)      # (a negative weight flips torch's gradient, not the difference's sign)
            if w == 0:                                                                   # torch's gradient is all zero: take the sign from the operands
                a, b = l1_inputs(name)[len(ga)]
                s = np.sign(np.nan_to_num(a.astype(np.float64) - b.astype(np.float64), nan=0.0))
        g = np.where(s > 0, c, np.where(s < 0, -c, F32(0.0))).astype(F32)
        ga.append(g)
        gb.append(-g)
    return ga, gb


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(y, dtype=F32)
    return x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))


L1_DEFECTS = ("fp32_sum", "drop_last", "padded_mean", "round_difference", "one_weight")
L1_DEFECT_CASE = {"fp32_sum": "fold", "drop_last": "n4097", "padded_mean": "tail", "round_difference": "bf16_odd", "one_weight": "mixed5"}


def l1_copy(name, defect=None):
    """The L1 rule once more in plain numpy sums (another order: inside the bound, not equal in bits), with a switch per seeded defect:
    "fp32_sum" the sum kept in fp32 (a running fp32 sum, element by element), "drop_last" the last element dropped, "padded_mean" the
    mean over the padded chunk length, "round_difference" the difference rounded to the 16-bit type, "one_weight" w applied to the
    first pair only.  Returns (loss, terms)."""
    case = L1_BY_NAME[name]
    total, terms = 0.0, []
    for k, ((a, b), p, w) in enumerate(zip(l1_inputs(name), case["pairs"], case["weights"])):
        d = np.abs((a - b).astype(F32))
        if defect == "round_difference":
            d = labels._round_to(d, p["dtype"])
        if defect == "drop_last":
            d = d[:-1]
        if defect == "fp32_sum":
            s = float(np.cumsum(d, dtype=F32)[-1])
        else:
            s = float(np.sum(d.astype(np.float64)))
        n = -(-p["n"] // losses.L1_CHUNK) * losses.L1_CHUNK if defect == "padded_mean" else p["n"]
        term = s / n
        terms.append(F32(term))
        total += (float(F32(w)) if (defect != "one_weight" or k == 0) else 1.0) * term
    return F32(total), np.array(terms, dtype=F32)


def check_l1_rejections(h):
    """`edtr_l1_workspace` / `edtr_l1_forward` / `edtr_l1_backward` by return code only.  Every call fails before its stand-in pointers
    are used, so nothing is launched."""
    import ctypes as ct
    p = 4096
    NULL, SHAPE, ALIGN, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -5
    i64 = lambda *v: (ct.c_int64 * len(v))(*v)
    assert h.edtr_l1_workspace(i64(1, 4096, 4097), 3) == 8 * 4 and h.edtr_l1_workspace(i64(300 * 4096 + 7), 1) == 8 * 301
    assert h.edtr_l1_workspace(None, 1) == 0 and h.edtr_l1_workspace(i64(1), 0) == 0 and h.edtr_l1_workspace(i64(*[1] * 9), 9) == 0
    assert h.edtr_l1_workspace(i64(0), 1) == 0 and h.edtr_l1_workspace(i64((1 << 30) + 1), 1) == 0 and h.edtr_l1_workspace(i64(1 << 30), 1) == 8 << 18

    def tables(k=2, dt=(0, 2), a=(p, p), b=(p, p), n=(4097, 5), w=(1.0, 0.5), ga=(p, None), gb=(None, p)):
        vp = lambda v: (ct.c_void_p * max(len(v), 1))(*v)
        return dict(dt=(ct.c_int32 * len(dt))(*dt), a=vp(a), b=vp(b), n=i64(*n), w=(ct.c_float * len(w))(*w), pairs=k, ga=vp(ga), gb=vp(gb))

    def fwd(ws=p, ws_bytes=24, loss=p, terms=p, max_blocks=0, drop=(), **kw):
        t = tables(**kw)
        for name in drop:
            t[name] = None
        return h.edtr_l1_forward(t["dt"], t["a"], t["b"], t["n"], t["w"], t["pairs"], ws, ws_bytes, loss, terms, max_blocks, None)

    def bwd(grad_loss=p, max_blocks=0, drop=(), **kw):
        t = tables(**kw)
        for name in drop:
            t[name] = None
        return h.edtr_l1_backward(t["dt"], t["a"], t["b"], t["n"], t["w"], t["pairs"], grad_loss, t["ga"], t["gb"], max_blocks, None)

    for name in ("dt", "a", "b", "n", "w"):
        assert fwd(drop=(name,)) == NULL and bwd(drop=(name,)) == NULL, name
    assert bwd(drop=("ga",)) == NULL and bwd(drop=("gb",)) == NULL and bwd(grad_loss=None) == NULL
    assert fwd(ws=None) == NULL and fwd(loss=None) == NULL and fwd(terms=None, ws_bytes=0) == SHAPE       # terms is optional
    assert bwd(ga=(None, None), gb=(None, None)) == NULL                                 # every gradient NULL
    for f in (fwd, bwd):
        assert f(a=(p, None)) == NULL and f(b=(None, p)) == NULL
        assert f(k=0) == SHAPE and f(k=9) == SHAPE and f(max_blocks=-1) == SHAPE and f(n=(4097, 0)) == SHAPE and f(n=(-1, 5)) == SHAPE
        assert f(n=(4097, (1 << 30) + 1)) == UNSUPPORTED and f(dt=(0, 3)) == DTYPE and f(dt=(-1, 0)) == DTYPE
        assert f(a=(p + 2, p)) == ALIGN and f(b=(p, p + 1)) == ALIGN
        # a NULL before the dtype before a count before the cap before an alignment
        assert f(a=(None, p), dt=(0, 3)) == NULL and f(dt=(0, 3), n=(0, 5)) == DTYPE and f(n=(0, (1 << 30) + 1)) == SHAPE
        assert f(n=(4097, (1 << 30) + 1), a=(p + 2, p)) == UNSUPPORTED
    assert fwd(ws_bytes=23) == SHAPE and fwd(ws=p + 4) == ALIGN and fwd(loss=p + 2) == ALIGN and fwd(terms=p + 2) == ALIGN
    assert bwd(grad_loss=p + 2) == ALIGN and bwd(ga=(p + 2, None)) == ALIGN and bwd(gb=(None, p + 1)) == ALIGN


# ---- the classifier's cross-entropy ----------------------------------------------------------------------------------------------------
def _ce(name, B, C, dtype="float32", scale=None, ignored=(), bad=False, ties=False, seed=0):
    return dict(name=name, B=B, C=C, dtype=dtype, scale=scale, ignored=ignored, bad=bad, ties=ties, seed=seed)


CE_CASES = [
    _ce("one_class", 1, 1, seed=1),                                  # loss and gradient exactly 0
    _ce("c63", 3, 63, seed=2), _ce("c64", 3, 64, seed=3), _ce("c65", 3, 65, seed=4),      # the wave edge
    _ce("typical_1000", 5, 1000, seed=5), _ce("typical_200", 32, 200, seed=6),
    _ce("pm100", 5, 1000, scale=100.0, seed=5),                      # logits scaled to +-100, past where fp32 holds exp(z)
    _ce("f16", 5, 200, dtype="float16", seed=7), _ce("bf16", 5, 200, dtype="bfloat16", seed=7),
    _ce("ignored_rows", 32, 200, ignored=(0, 5, 31), seed=8),
    _ce("all_ignored", 4, 65, ignored=(0, 1, 2, 3), seed=9),         # NaN loss, zero gradient
    _ce("bad_labels", 6, 65, ignored=(2,), bad=True, seed=10),       # labels >= C and negative ones other than ignore_index: counted as bad
    _ce("ties", 3, 130, ties=True, seed=11),                         # a row of equal logits
]
CE_IDS = [c["name"] for c in CE_CASES]
CE_BY_NAME = {c["name"]: c for c in CE_CASES}


@functools.lru_cache(maxsize=None)
def ce_inputs(name):
    """(logits as fp32 that hold values of the case's type, labels int64): logits 4 N(0, 1), scaled to +-``scale`` where that is set"""
    case = CE_BY_NAME[name]
    if "given" in case:                    # (`ce_given`: a case made from tensors a test computed)
        return case["given"]
    rng = np.random.default_rng(case["seed"])
    x = (4.0 * rng.standard_normal((case["B"], case["C"]))).astype(F32)
    if case["scale"]:
        x = (x * F32(case["scale"] / np.abs(x).max())).astype(F32)
    if case["ties"]:
        x[1] = x[1, 0]
    x = labels._round_to(x, case["dtype"])
    t = rng.integers(0, case["C"], case["B"]).astype(np.int64)
    for b in case["ignored"]:
        t[b] = IGNORE
    if case["bad"]:
        t[0], t[1], t[4] = case["C"], -1, 1 << 20
    x.setflags(write=False), t.setflags(write=False)
    return x, t


def ce_given(name, logits, labels, dtype="float32"):
    """registers (and returns) a case whose inputs are these arrays, so that `ce_reference` and `ce_bounds` serve it too"""
    x, t = np.ascontiguousarray(logits, dtype=F32), np.ascontiguousarray(labels, dtype=np.int64)
    CE_BY_NAME[name] = dict(_ce(name, x.shape[0], x.shape[1], dtype=dtype), given=(x, t))
    return CE_BY_NAME[name]


def ce_keep(case, t):
    return (t != IGNORE) & (t >= 0) & (t < case["C"])


@functools.lru_cache(maxsize=None)
def ce_reference(name):
    """fp64: dict(loss, lse [B], grad [B, C] for the upstream gradient GRAD_LOSS, count)"""
    case = CE_BY_NAME[name]
    x, t = ce_inputs(name)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(np.where(ce_keep(case, t), t, IGNORE))
    count = int((tt != IGNORE).sum())
    loss = F.cross_entropy(xt, tt, reduction="mean", ignore_index=IGNORE)
    if count:
        (GRAD_LOSS * loss).backward()
    grad = xt.grad.numpy() if xt.grad is not None else np.zeros(x.shape)
    return dict(loss=loss.item(), lse=torch.logsumexp(xt, dim=1).detach().numpy(), grad=grad, count=count)


@functools.lru_cache(maxsize=None)
def ce_bounds(name):
    """dict(loss, lse [B], grad [B, C]): tests/seg_loss_cases.py's per-element bound taken on rows, where the logits are given and carry
    no error of their own (its E_z = 0).  With M the largest |logit|, n = C and u = 2^-24:
      lse   u [4 M + n (2 ULP_EXP + 3)] + 2 u ULP_LOG ln n + u (|lse| + 1): every addend exp(z_c - m) carries the rounding of its argument
            (<= 2 M u) and expf's own error, every sum one rounding (the lane-and-tree order has fewer on any path than the n counted
            here); logf of a value in [1, n]; the last sum
      loss  the mean over the counted rows of E_lse + u |lse - z_t|, + 2 u |loss| (the fp64 sums are exact to 2^-53)
      grad  e = (p - [c == t]) g with p = exp(z_c - lse): g p (E_lse + u |z_c - lse| + 2 u ULP_EXP) + 4 u |e|; a 16-bit gradient adds half
            an ulp of its type at the value that is rounded: u16 (|want| + bound) (+ 2^-25 for float16's subnormals).
            On rows the bound of an element is no longer a sum over many pixels, so fp32's underflow shows: with logits of +-100 a
            probability is as small as exp(-200) = 1e-87, which no fp32 holds.  Below the smallest normal 2^-126 an fp32 value is
            rounded on a grid of 2^-149 or, where subnormal results are flushed, replaced by 0: an absolute error of at most 2^-126 in
            p and again in the product with g, (g + 1) 2^-126 in all (1e-38: it hides nothing a relative bound shows)."""
    case, ref = CE_BY_NAME[name], ce_reference(name)
    x, t = ce_inputs(name)
    n = case["C"]
    keep = ce_keep(case, t)
    M = float(np.abs(x).max())
    Else = U * (4.0 * M + n * (2.0 * ULP_EXP + 3.0)) + 2.0 * U * ULP_LOG * np.log(n) + U * (np.abs(ref["lse"]) + 1.0)
    tt = np.clip(t, 0, n - 1)
    zt = x.astype(np.float64)[np.arange(case["B"]), tt]
    Eell = Else + U * np.abs(ref["lse"] - zt)
    out = dict(lse=Else, loss=float("nan"), grad=np.zeros(x.shape))
    if ref["count"]:
        out["loss"] = float(Eell[keep].mean() + 2.0 * U * abs(ref["loss"]))
        g = GRAD_LOSS / ref["count"]
        z = x.astype(np.float64)
        p = np.exp(z - ref["lse"][:, None])
        e = np.abs(p - (np.arange(n)[None, :] == tt[:, None])) * g * keep[:, None]
        Eg = (g * p * (Else[:, None] + U * np.abs(z - ref["lse"][:, None]) + 2.0 * U * ULP_EXP) + (g + 1.0) * 2.0 ** -126) * keep[:, None] + 4.0 * U * e
        out["grad"] = Eg + U16[case["dtype"]] * (np.abs(ref["grad"]) + Eg) + (2.0 ** -25 if case["dtype"] == "float16" else 0.0)
    return out


def ce_ratios(name, loss, lse, grad, scale=1.0):
    """(loss, lse, grad) error / (``scale`` x bound) against `ce_reference`, the worst element of each (0 where both are 0; inf where
    only the bound is)"""
    ref, bnd = ce_reference(name), ce_bounds(name)
    def worst(err, b):
        err, b = np.asarray(err, dtype=np.float64), np.asarray(b, dtype=np.float64) * scale
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / b)
        return float(np.max(q)) if q.size else 0.0
    r_loss = 0.0 if not ref["count"] else worst(abs(float(loss) - ref["loss"]), bnd["loss"])
    return r_loss, worst(np.abs(np.asarray(lse, dtype=np.float64) - ref["lse"]), bnd["lse"]), worst(np.abs(np.asarray(grad, dtype=np.float64) - ref["grad"]), bnd["grad"])


CE_DEFECTS = ("no_max", "count_ignored", "divide_by_B")
CE_DEFECT_CASE = {"no_max": "pm100", "count_ignored": "ignored_rows", "divide_by_B": "ignored_rows"}


def ce_copy(name, defect=None):
    """The cross-entropy rule once more with plain numpy row sums (another order: inside the bound), with a switch per seeded defect:
    "no_max" the maximum left out of the exponent, "count_ignored" an ignored row counted (as class 0), "divide_by_B" the division by
    B in place of the count.  Returns (loss, lse, grad for GRAD_LOSS)."""
    case = CE_BY_NAME[name]
    x, t = ce_inputs(name)
    B, C = x.shape
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = x.max(axis=1)
        inside = np.zeros_like(m) if defect == "no_max" else m
        s = np.exp((x - inside[:, None]).astype(F32)).sum(axis=1, dtype=F32)
        lse = (m + np.log(s)).astype(F32)
        keep = ce_keep(case, t)
        counted = np.ones_like(keep) if defect == "count_ignored" else keep
        tt = np.where(keep, t, 0)
        ell = (lse - x[np.arange(B), tt]).astype(F32)
        count = B if defect == "divide_by_B" else int(counted.sum())
        loss = F32(ell[counted].astype(np.float64).sum() / count) if count else F32(np.nan)
        g = F32(GRAD_LOSS) / F32(max(count, 1))
        hot = (np.arange(C)[None, :] == tt[:, None]).astype(F32)
        grad = labels._round_to((((np.exp((x - lse[:, None]).astype(F32)) - hot) * g).astype(F32) * counted[:, None]).astype(F32), case["dtype"])
    return loss, lse, grad


def check_ce_rejections(h):
    """`edtr_cls_ce_forward` / `edtr_cls_ce_backward` by return code only; nothing is launched"""
    p = 4096
    NULL, SHAPE, ALIGN, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -5

    def fwd(**kw):
        a = dict(dt=0, logits=p, labels=p, B=5, C=1000, ignore=IGNORE, lse=p, ws=p, ws_bytes=40, loss=p, counts=p)
        a.update(kw)
        return h.edtr_cls_ce_forward(*a.values(), None)

    def bwd(**kw):
        a = dict(dt=0, logits=p, labels=p, B=5, C=1000, ignore=IGNORE, lse=p, counts=p, grad_loss=p, grad=p)
        a.update(kw)
        return h.edtr_cls_ce_backward(*a.values(), None)
    for name in ("logits", "labels", "lse", "ws", "loss", "counts"):
        assert fwd(**{name: None}) == NULL, name
    for name in ("logits", "labels", "lse", "counts", "grad_loss", "grad"):
        assert bwd(**{name: None}) == NULL, name
    for f in (fwd, bwd):
        assert f(dt=3) == DTYPE and f(B=0) == SHAPE and f(C=0) == SHAPE and f(B=65536) == UNSUPPORTED and f(C=65537) == UNSUPPORTED
        assert f(logits=p + 2) == ALIGN and f(dt=2, logits=p + 1) == ALIGN and f(labels=p + 2) == ALIGN and f(lse=p + 2) == ALIGN and f(counts=p + 4) == ALIGN
        assert f(logits=None, dt=3) == NULL and f(dt=3, B=0) == DTYPE and f(B=0, C=65537) == SHAPE and f(C=65537, logits=p + 2) == UNSUPPORTED
    assert fwd(ws_bytes=39) == SHAPE and fwd(ws=p + 4) == ALIGN and fwd(loss=p + 2) == ALIGN
    assert bwd(grad=p + 2) == ALIGN and bwd(grad_loss=p + 2) == ALIGN and bwd(dt=1, grad=p + 1) == ALIGN
