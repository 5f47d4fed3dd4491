"""Training losses on the device: the two loss terms every training script of the reference shares.

  * THE FEATURE-MATCHING L1.  `F.l1_loss(feat_a, feat_b, reduction="mean") * w` is the feature-matching term loss_fm and the
    feature-distance term loss_hlf of all three tasks (main/cls/train_edtr.py:175-176, 213; main/seg/train_edtr.py:180-181, 218;
    main/det/train_edtr.py:194-197, 236-237) and the val_fd of the segmentation and detection test loops.  `l1_mean` takes the whole
    list of pairs of such a term — up to `L1_MAX_PAIRS`, of mixed types and sizes — in one forward launch pair and one backward launch;
    `feature_matching` is the same call on tensors or on the mappings the task networks return.
  * THE CLASSIFIER'S CROSS-ENTROPY.  `F.cross_entropy(pred, label, reduction="mean", label_smoothing=0.0)`
    (main/cls/train_edtr.py:208): `cross_entropy`, the rule of `labels.coarse_cross_entropy` on rows of logits.

The launches are include/edtr_hip.h "Training losses" (kernels in csrc/losses.hip, launch records in `ops`).  Layers as in `labels`:
thin wrappers over the launches (torch tensors on the device, the caller's stream, nothing waits for the device), and the numpy
restatements `*_reference`, which are the NORMATIVE definition.  This module imports without torch.

THE L1 RULE.  loss = sum_k w_k mean_i |a_k[i] - b_k[i]|.  Each difference is formed in fp32 — both operands widened exactly, ONE
rounded subtraction, the absolute value — and added in fp64.  For fp16 / bf16 inputs that is what torch computes under autocast
(l1_loss runs in fp32 there) and a deliberate difference from a plain 16-bit l1_loss, which rounds each difference to 16 bits.  The
order of the fp64 sum is a function of n alone (the same for the three element types), never of the grid, a pointer's alignment or
the pair's place in the list: a chunk is `L1_CHUNK` = 4096 elements; lane l of 256 owns elements 4 l ... 4 l + 3 of each of the
chunk's four 1024-element quarters and adds them in ascending order; the tree s = 128, 64, ..., 1 with sum[l] += sum[l + s] gives the
chunk's partial.  Per pair, lane l then adds partials l, l + 256, ... ascending, the same tree follows, term_k = sum / float64(n_k),
total = sum over k ascending of float64(w_k) term_k, loss = float32(total); terms[k] = float32(term_k).  A NaN difference makes the loss
NaN, as in torch.  There is no transcendental: the launches equal the restatements bit for bit, gradients included.

THE L1 GRADIENT.  c_k = float32(float64(grad_loss) float64(w_k) / float64(n_k)); grad_a[i] is +c_k where the fp32 difference is
positive, -c_k where it is negative and +0.0 where it is zero or NaN (torch's sign); grad_b = -grad_a by a flip of the sign bit, so
-0.0 where grad_a is +0.0.  A 16-bit gradient takes c_k rounded once.

THE CROSS-ENTROPY RULE.  Per row: m the maximum; s = sum_c exp(z_c - m) in fp32, lane l of 64 adding c = l, l + 64, ... ascending,
then the tree o = 32, ..., 1 with s[l] += s[l + o]; lse = m + log(s).  A row counts iff label != ignore_index and 0 <= label < C; any
other label that is not ignore_index makes torch RAISE and is here IGNORED and counted in ``bad``.  loss = float32(sum of
float64(float32(lse - z_label)) over the counted rows in row order / count); no counted row: NaN.  The gradient is
fmul(fadd(exp(fadd(z_c, -lse)), -[c == label]), g), g = float32(grad_loss) / float32(count), +0.0 on rows that do not count, rounded
once to a 16-bit type.  The launches differ from the restatements only in expf / logf."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

F32, F64 = np.float32, np.float64
L1_MAX_PAIRS = 8                        # EDTR_L1_MAX_PAIRS
L1_CHUNK = 4096                         # EDTR_L1_CHUNK
L1_MAX_ELEMS = 1 << 30                  # EDTR_L1_MAX_ELEMS
L1_LANES = 256
CE_MAX_CLASSES = 65536                  # EDTR_CLS_MAX_CLASSES
CE_MAX_ROWS = 65535
CE_LANES = 64
LOGIT_TYPES = ("float32", "float16", "bfloat16")


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative)
# ----------------------------------------------------------------------------------------------------------------------------------
def _round_to(v: np.ndarray, dtype: str) -> np.ndarray:
    from . import labels
    return labels._round_to(np.asarray(v, dtype=F32), dtype)


def _tree(v: np.ndarray) -> np.ndarray:
    """[..., L] (L a power of two) -> [...]: the tree s = L / 2, ..., 1 with v[l] += v[l + s]"""
    v = v.copy()
    s = v.shape[-1] // 2
    while s:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s //= 2
    return v[..., 0]


def _pair_arrays(pairs, weights, dtypes):
    """[(a, b, dtype)] with a, b flat fp32 arrays that hold values of the pair's type, and fp32 weights, checked"""
    pairs = [tuple(p) for p in pairs]
    if not 1 <= len(pairs) <= L1_MAX_PAIRS:
        raise ValueError(f"1 to {L1_MAX_PAIRS} pairs, got {len(pairs)}")
    weights = [1.0] * len(pairs) if weights is None else list(weights)
    dtypes = [None] * len(pairs) if dtypes is None else list(dtypes)
    if len(weights) != len(pairs) or len(dtypes) != len(pairs):
        raise ValueError(f"{len(weights)} weights and {len(dtypes)} types for {len(pairs)} pairs")
    out = []
    for (a, b), dt in zip(pairs, dtypes):
        a, b = np.asarray(a), np.asarray(b)
        if dt is None:
            dt = "float16" if a.dtype == np.float16 else "float32"
        if dt not in LOGIT_TYPES:
            raise ValueError(f"a pair's type is one of {LOGIT_TYPES}, got {dt!r}")
        if a.dtype not in (np.float32, np.float16) or b.dtype != a.dtype:
            raise TypeError(f"a pair is two fp32 / fp16 arrays of one type (bf16 travels widened), got {a.dtype} and {b.dtype}")
        if a.shape != b.shape or a.size == 0:
            raise ValueError(f"the arrays of a pair have one non-empty shape, got {a.shape} and {b.shape}")
        if a.size > L1_MAX_ELEMS:
            raise ValueError(f"at most {L1_MAX_ELEMS} elements a pair, got {a.size}")
        a, b = a.astype(F32).reshape(-1), b.astype(F32).reshape(-1)
        if not (np.array_equal(_round_to(a, dt), a, equal_nan=True) and np.array_equal(_round_to(b, dt), b, equal_nan=True)):
            raise ValueError(f"the arrays do not hold {dt} values")
        out.append((a, b, dt))
    return out, np.asarray(weights, dtype=F32)


def l1_chunk_partials(absdiff: np.ndarray) -> np.ndarray:
    """fp64 [ceil(n / L1_CHUNK)]: the chunk sums of fp64 ``absdiff`` [n] in the launch's order (the elements past n add nothing)"""
    n = absdiff.size
    chunks = -(-n // L1_CHUNK)
    x = np.zeros(chunks * L1_CHUNK, dtype=F64)
    x[:n] = absdiff
    x = x.reshape(chunks, 4, L1_LANES, 4)
    lane = np.zeros((chunks, L1_LANES), dtype=F64)
    for q in range(4):
        for j in range(4):
            lane = lane + x[:, q, :, j]
    return _tree(lane)


def l1_fold(partials: np.ndarray) -> float:
    """the fp64 sum of a pair's chunk partials in the finalize launch's order: lane l adds partials l, l + 256, ... ascending, then the tree"""
    rounds = -(-partials.size // L1_LANES)
    p = np.zeros(rounds * L1_LANES, dtype=F64)
    p[:partials.size] = partials
    lane = np.zeros(L1_LANES, dtype=F64)
    for row in p.reshape(rounds, L1_LANES):
        lane = lane + row
    return _tree(lane)


def l1_mean_reference(pairs, weights=None, dtypes=None):
    """sum_k w_k mean |a_k - b_k| by THE L1 RULE (module docstring); NORMATIVE for `l1_mean`.  ``pairs``: [(a, b)] of fp32 / fp16 arrays
    (bf16 values travel as fp32; name them in ``dtypes``, one of `LOGIT_TYPES` per pair).  Returns (loss fp32, terms fp32 [pairs])."""
    arrays, w = _pair_arrays(pairs, weights, dtypes)
    total, terms = F64(0.0), np.zeros(len(arrays), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (a, b, _) in enumerate(arrays):
            d = np.abs((a - b).astype(F32)).astype(F64)
            term = F64(l1_fold(l1_chunk_partials(d))) / F64(a.size)
            total = total + F64(w[k]) * term
            terms[k] = F32(term)
        return F32(total), terms


def l1_mean_backward_reference(pairs, weights=None, grad_loss=1.0, dtypes=None):
    """The gradients of `l1_mean_reference`'s loss times ``grad_loss`` by THE L1 GRADIENT (module docstring); NORMATIVE for the backward
    launch.  Returns ([grad_a_k], [grad_b_k]): fp32 arrays of each pair's shape that hold values of its type."""
    shapes = [np.asarray(p[0]).shape for p in pairs]
    arrays, w = _pair_arrays(pairs, weights, dtypes)
    ga, gb = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for (a, b, dt), wk, shape in zip(arrays, w, shapes):
            c = _round_to(np.array([F32(F64(F32(grad_loss)) * F64(wk) / F64(a.size))], dtype=F32), dt)[0]
            d = (a - b).astype(F32)
            g = np.where(d > 0, c, np.where(d < 0, -c, F32(0.0))).astype(F32).reshape(shape)
            ga.append(g)
            gb.append(-g)
    return ga, gb


def _ce_inputs(logits, labels, dtype):
    if dtype not in LOGIT_TYPES:
        raise ValueError(f"dtype must be one of {LOGIT_TYPES}, got {dtype!r}")
    x, t = np.asarray(logits), np.asarray(labels)
    if x.ndim != 2 or x.dtype not in (np.float32, np.float16) or 0 in x.shape:
        raise ValueError(f"expected fp32 / fp16 logits [B, C], got {x.dtype} {x.shape}")
    if x.shape[0] > CE_MAX_ROWS or x.shape[1] > CE_MAX_CLASSES:
        raise ValueError(f"at most {CE_MAX_ROWS} rows of {CE_MAX_CLASSES} classes, got {x.shape}")
    if t.ndim != 1 or t.shape[0] != x.shape[0] or t.dtype.kind not in "iu":
        raise ValueError(f"labels are one integer per row, got {t.dtype} {t.shape}")
    x = np.ascontiguousarray(x.astype(F32))
    if not np.array_equal(_round_to(x, dtype), x, equal_nan=True):
        raise ValueError(f"the logits do not hold {dtype} values")
    return x, t.astype(np.int64)


def cross_entropy_reference(logits, labels, ignore_index: int = -100, dtype: str = "float32"):
    """`F.cross_entropy(logits, labels, reduction="mean", ignore_index=)` by THE CROSS-ENTROPY RULE (module docstring); NORMATIVE for
    `cross_entropy`.  Returns (loss fp32, lse fp32 [B], count, bad)."""
    z, t = _ce_inputs(logits, labels, dtype)
    B, C = z.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = z.max(axis=1)
        rounds = -(-C // CE_LANES)
        e = np.zeros((B, rounds * CE_LANES), dtype=F32)
        e[:, :C] = np.exp((z - m[:, None]).astype(F32))
        s = np.zeros((B, CE_LANES), dtype=F32)
        for r in range(rounds):
            s = s + e[:, r * CE_LANES:(r + 1) * CE_LANES]
        lse = (m + np.log(_tree(s))).astype(F32)
        keep = (t != int(ignore_index)) & (t >= 0) & (t < C)
        bad = int(np.count_nonzero(~keep & (t != int(ignore_index))))
        zt = z[np.arange(B), np.clip(t, 0, C - 1)]
        ell = (lse - zt).astype(F32).astype(F64)
        total, count = F64(0.0), 0
        for b in range(B):
            if keep[b]:
                total, count = total + ell[b], count + 1
        loss = F32(total / F64(count))
    return loss, lse, count, bad


def cross_entropy_backward_reference(logits, labels, lse, count, grad_loss=1.0, ignore_index: int = -100, dtype: str = "float32") -> np.ndarray:
    """The gradient of `cross_entropy_reference`'s loss in the logits times ``grad_loss``: fp32 [B, C] that holds values of ``dtype``.
    NORMATIVE for the backward launch; ``lse`` and ``count`` are what the forward returned."""
    z, t = _ce_inputs(logits, labels, dtype)
    B, C = z.shape
    lse = np.asarray(lse, dtype=F32)
    if lse.shape != (B,):
        raise ValueError(f"lse must be fp32 [B], got {lse.shape}")
    out = np.zeros((B, C), dtype=F32)
    if int(count) <= 0:
        return out
    g = F32(grad_loss) / F32(int(count))
    keep = (t != int(ignore_index)) & (t >= 0) & (t < C)
    with np.errstate(invalid="ignore", over="ignore"):
        hot = (np.arange(C)[None, :] == t[:, None]).astype(F32)
        e = ((np.exp((z - lse[:, None]).astype(F32)) - hot).astype(F32) * g).astype(F32)
        return _round_to(np.where(keep[:, None], e, F32(0.0)).astype(F32), dtype)


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _device_pairs(pairs, weights):
    """([(a, b)] contiguous device tensors, [float weights]) of `l1_mean`, checked before anything is launched"""
    import torch
    pairs = [tuple(p) for p in pairs]
    if not 1 <= len(pairs) <= L1_MAX_PAIRS:
        raise ValueError(f"1 to {L1_MAX_PAIRS} pairs, got {len(pairs)}")
    weights = [1.0] * len(pairs) if weights is None else [float(w) for w in weights]
    if len(weights) != len(pairs):
        raise ValueError(f"{len(weights)} weights for {len(pairs)} pairs")
    out = []
    for p in pairs:
        if len(p) != 2 or not all(isinstance(v, torch.Tensor) for v in p):
            raise TypeError("a pair is two tensors")
        a, b = p
        if a.dtype not in (torch.float32, torch.float16, torch.bfloat16) or b.dtype != a.dtype:
            raise TypeError(f"both tensors of a pair must be float32, float16 or bfloat16 alike, got {a.dtype} and {b.dtype}")
        if a.shape != b.shape or a.numel() == 0:
            raise ValueError(f"the tensors of a pair have one non-empty shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        if a.numel() > L1_MAX_ELEMS:
            raise ValueError(f"at most {L1_MAX_ELEMS} elements a pair, got {a.numel()}")
        if not (a.is_cuda and b.is_cuda and a.device == b.device == pairs[0][0].device):
            raise TypeError("l1_mean takes tensors on one device")
        out.append((a.contiguous(), b.contiguous()))
    return out, weights


def _l1_forward(pairs, weights, max_blocks: int):
    """the forward launches on checked pairs: (loss fp32 [], terms fp32 [pairs]) on the device"""
    import torch
    from . import ops
    dev = pairs[0][0].device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    terms = torch.empty((len(pairs),), dtype=torch.float32, device=dev)
    workspace = torch.empty((ops.l1_workspace([a.numel() for a, _ in pairs]),), dtype=torch.uint8, device=dev)
    ops.launch(ops.make_l1_forward(pairs=pairs, weights=weights, workspace=workspace, loss=loss, terms=terms, max_blocks=max_blocks))
    return loss, terms


def _grad_scalar(grad_loss, device):
    import torch
    g = grad_loss if isinstance(grad_loss, torch.Tensor) else torch.tensor(float(grad_loss), dtype=torch.float32)
    if g.numel() != 1:
        raise ValueError("grad_loss is one number")
    return g.detach().to(device=device, dtype=torch.float32).contiguous()


def l1_mean_backward(pairs, weights=None, grad_loss=1.0, need_a: Optional[Sequence[bool]] = None, need_b: Optional[Sequence[bool]] = None,
                     max_blocks: int = 0):
    """`l1_mean_backward_reference` on the device, ONE launch for all pairs: ([grad_a_k or None], [grad_b_k or None]) in each pair's
    shape and type for the upstream gradient ``grad_loss``, a number or an fp32 device scalar.  ``need_a`` / ``need_b`` (default: every
    a, no b): which gradients are allocated and written; the others come back as None.  Every element is written; two calls give the
    same bits."""
    import torch
    from . import ops
    pairs, weights = _device_pairs([(a.detach(), b.detach()) for a, b in pairs], weights)
    need_a = [True] * len(pairs) if need_a is None else [bool(v) for v in need_a]
    need_b = [False] * len(pairs) if need_b is None else [bool(v) for v in need_b]
    if len(need_a) != len(pairs) or len(need_b) != len(pairs) or not any(need_a + need_b):
        raise ValueError("one flag per pair and side, at least one of them set")
    if int(max_blocks) < 0:
        raise ValueError(f"max_blocks must not be negative, got {max_blocks}")
    grads_a = [torch.empty_like(a) if need else None for (a, _), need in zip(pairs, need_a)]
    grads_b = [torch.empty_like(b) if need else None for (_, b), need in zip(pairs, need_b)]
    ops.launch(ops.make_l1_backward(pairs=pairs, weights=weights, grad_loss=_grad_scalar(grad_loss, pairs[0][0].device), grads_a=grads_a,
                                    grads_b=grads_b, max_blocks=int(max_blocks)))
    return grads_a, grads_b


_L1_FUNCTION = None


def _l1_function():
    """the autograd.Function behind an `l1_mean` with an operand that requires grad (made on first use: this module imports without torch)"""
    global _L1_FUNCTION
    if _L1_FUNCTION is None:
        import torch
        from torch.autograd.function import once_differentiable

        class L1Mean(torch.autograd.Function):
            @staticmethod
            def forward(ctx, weights, max_blocks, *flat):
                pairs = [(flat[i].detach(), flat[i + 1].detach()) for i in range(0, len(flat), 2)]
                loss, terms = _l1_forward(pairs, weights, max_blocks)
                ctx.save_for_backward(*flat)
                ctx.weights, ctx.max_blocks = weights, max_blocks
                ctx.mark_non_differentiable(terms)
                return loss, terms

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_loss, _):
                flat = ctx.saved_tensors
                need = ctx.needs_input_grad[2:]
                pairs = [(flat[i], flat[i + 1]) for i in range(0, len(flat), 2)]
                ga, gb = l1_mean_backward(pairs, ctx.weights, grad_loss, need[0::2], need[1::2], ctx.max_blocks)
                return (None, None) + tuple(g for ab in zip(ga, gb) for g in ab)

        _L1_FUNCTION = L1Mean
    return _L1_FUNCTION


def l1_mean(pairs, weights=None, return_terms: bool = False, max_blocks: int = 0):
    """`l1_mean_reference` on the device: sum_k weights[k] * `F.l1_loss(a_k, b_k, reduction="mean")` over ``pairs`` = [(a, b)], up to
    `L1_MAX_PAIRS` pairs of device tensors, each pair of one shape and one of float32 / float16 / bfloat16 (the pairs may differ;
    16-bit differences are formed in fp32, as under autocast).  They are made contiguous.  Returns the loss, an fp32 scalar on the
    device; with ``return_terms`` also fp32 [pairs], the unweighted means (what the test loops log as val_fd).  Each operand is read
    once; no full-size intermediate is stored.  Nothing waits for the device, and the bits depend on the shapes alone.
    With grad mode on and any operand that requires grad the loss is differentiable (once): the backward is one launch for all pairs
    that allocates and writes gradients only for the operands that require them.  In every other case only the forward launches run.
    ``max_blocks`` caps the grids (0: the default cap); no result depends on it."""
    import torch
    checked, weights = _device_pairs(pairs, weights)
    max_blocks = int(max_blocks)
    if max_blocks < 0:
        raise ValueError(f"max_blocks must not be negative, got {max_blocks}")
    if torch.is_grad_enabled() and any(t.requires_grad for p in checked for t in p):
        loss, terms = _l1_function().apply(tuple(weights), max_blocks, *[t for p in checked for t in p])
    else:
        loss, terms = _l1_forward(checked, weights, max_blocks)
    return (loss, terms) if return_terms else loss


def feature_matching(student, teacher, keys=None, weights=None, weight: float = 1.0):
    """The feature-matching term of the reference's training scripts as one `l1_mean`: ``weight`` * sum over ``keys`` of weights[key] *
    `F.l1_loss(student[key], teacher[key])`.  ``student`` / ``teacher``: two tensors, or two mappings as the task networks return them
    under return_feat (``keys``: which entries, default every key of ``student``).  keys=("C5",) is the segmenter's form
    (main/seg/train_edtr.py:218), keys=("0", "1"), weights=(0.5, 0.5) the detector's (main/det/train_edtr.py:236-237), two tensors the
    classifier's (main/cls/train_edtr.py:213).  The teacher's features take no gradient unless they require one."""
    if hasattr(student, "keys") != hasattr(teacher, "keys"):
        raise TypeError("student and teacher are two tensors or two mappings")
    if hasattr(student, "keys"):
        keys = list(student.keys()) if keys is None else list(keys)
        pairs = [(student[k], teacher[k]) for k in keys]
    else:
        if keys is not None:
            raise ValueError("keys select from mappings")
        pairs = [(student, teacher)]
    weights = [1.0] * len(pairs) if weights is None else [float(w) for w in weights]
    if len(weights) != len(pairs):
        raise ValueError(f"{len(weights)} weights for {len(pairs)} pairs")
    return l1_mean(pairs, [float(weight) * w for w in weights])


def _ce_checked(what: str, logits, labels):
    """contiguous [B, C] logits on the device and their int32 labels there, checked"""
    import torch
    from . import cls
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.ndim != 2:
        raise TypeError(f"{what} takes a [B, C] logits tensor on the device")
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {logits.dtype}")
    B, C = logits.shape
    if not 1 <= B <= CE_MAX_ROWS or not 1 <= C <= CE_MAX_CLASSES:
        raise ValueError(f"1 to {CE_MAX_ROWS} rows of 1 to {CE_MAX_CLASSES} classes, got {tuple(logits.shape)}")
    return logits.contiguous(), cls._labels_i32(labels, B, logits.device)


def _ce_forward(logits, labels, ignore_index: int):
    """the forward launches: (loss fp32 [], counts int64 [2], lse fp32 [B]) on the device"""
    import torch
    from . import ops
    B, dev = logits.shape[0], logits.device
    lse = torch.empty((B,), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty((2,), dtype=torch.int64, device=dev)
    workspace = torch.empty((8 * B,), dtype=torch.uint8, device=dev)
    ops.launch(ops.make_cls_ce_forward(logits=logits, labels=labels, lse=lse, workspace=workspace, loss=loss, counts=counts,
                                       ignore_index=ignore_index))
    return loss, counts, lse


def cross_entropy_backward(logits, labels, lse, counts, grad_loss, ignore_index: int = -100):
    """`cross_entropy_backward_reference` on the device, one launch: the gradient [B, C] in the type of ``logits`` from the ``lse`` and
    ``counts`` of the forward (`cross_entropy(..., return_saved=True)`) and the upstream gradient ``grad_loss``, a number or an fp32
    device scalar.  Every element is written."""
    import torch
    from . import ops
    logits, labels = _ce_checked("cross_entropy_backward", logits, labels)
    if not (isinstance(lse, torch.Tensor) and lse.dtype == torch.float32 and tuple(lse.shape) == (logits.shape[0],) and lse.is_contiguous()
            and lse.device == logits.device):
        raise TypeError("lse must be the contiguous fp32 [B] tensor the forward wrote")
    if not (isinstance(counts, torch.Tensor) and counts.dtype == torch.int64 and counts.numel() == 2 and counts.device == logits.device):
        raise TypeError("counts must be the int64 [2] tensor the forward wrote")
    grad = torch.empty_like(logits)
    ops.launch(ops.make_cls_ce_backward(logits=logits, labels=labels, lse=lse, counts=counts, grad_loss=_grad_scalar(grad_loss, logits.device),
                                        grad=grad, ignore_index=int(ignore_index)))
    return grad


_CE_FUNCTION = None


def _ce_function():
    """the autograd.Function behind a `cross_entropy` whose logits require grad (made on first use)"""
    global _CE_FUNCTION
    if _CE_FUNCTION is None:
        import torch
        from torch.autograd.function import once_differentiable

        class CrossEntropy(torch.autograd.Function):
            @staticmethod
            def forward(ctx, logits, labels, ignore_index):
                loss, counts, lse = _ce_forward(logits.detach(), labels, ignore_index)
                ctx.save_for_backward(logits, labels, lse, counts)
                ctx.ignore_index = ignore_index
                ctx.mark_non_differentiable(counts)
                return loss, counts

            @staticmethod
            @once_differentiable
            def backward(ctx, grad_loss, _):
                logits, labels, lse, counts = ctx.saved_tensors
                return cross_entropy_backward(logits.detach(), labels, lse, counts, grad_loss, ctx.ignore_index), None, None

        _CE_FUNCTION = CrossEntropy
    return _CE_FUNCTION


def cross_entropy(logits, labels, ignore_index: int = -100, label_smoothing: float = 0.0, return_counts: bool = False,
                  return_saved: bool = False):
    """`cross_entropy_reference` on the device: `F.cross_entropy(logits, labels, reduction="mean", ignore_index=)` of ``logits`` (a
    float32 / float16 / bfloat16 [B, C] device tensor) against ``labels`` (B integers).  Returns the loss, an fp32 scalar on the device;
    with ``return_counts`` also the int64 [2] device tensor (count, bad): a label outside [0, C) that is not ``ignore_index`` is ignored
    and counted in bad, where torch raises.  No counted row: NaN.  Nothing waits for the device.  ``label_smoothing`` must be 0.0 (the
    reference passes nothing else).
    With grad mode on and ``logits`` that require grad the loss is differentiable (once) in ``logits``: its backward is one launch
    that takes the upstream gradient as a device scalar.  In every other case only the forward launches run.  ``return_saved``
    (forward only): returns (loss, counts, lse), what `cross_entropy_backward` takes."""
    import torch
    if float(label_smoothing) != 0.0:
        raise ValueError(f"label_smoothing must be 0.0, got {label_smoothing}")
    checked, labels = _ce_checked("cross_entropy", logits, labels)
    ignore_index = int(ignore_index)
    if return_saved:
        return _ce_forward(checked.detach(), labels, ignore_index)
    if torch.is_grad_enabled() and checked.requires_grad:
        loss, counts = _ce_function().apply(checked, labels, ignore_index)
    else:
        loss, counts, _ = _ce_forward(checked, labels, ignore_index)
    return (loss, counts) if return_counts else loss
