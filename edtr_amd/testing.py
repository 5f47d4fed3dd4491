"""Helpers shared by tests / smoke / bench: build a ControlLDM with the synthetic weights of edtr_amd.synth.
Nothing here touches the CPU oracle (oracle/ is imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline only)."""
from __future__ import annotations

import bisect
import contextlib
import math
from typing import Dict, Iterable, Set, Tuple

import torch

from . import arch, synth
from .model import ControlLDM


_SD_CACHE: Dict[str, Dict[str, Dict[str, torch.Tensor]]] = {}


def synthetic_state_dicts(cfg: dict, device=None, weights: str = "smooth") -> Dict[str, Dict[str, torch.Tensor]]:
    """{'unet': sd, 'controlnet': sd, 'vae': sd} with reference key names; hash keys carry the part prefix, exactly
    as tools/make_goldens.py did on the reference model (`cldm.state_dict()` keys).  Cached per configuration (hashing the
    1.3 G parameters of the SD-2.1 size takes about a minute of CPU; consumers copy the values, never mutate them)."""
    import json
    key = json.dumps({k: cfg[k] for k in ("unet_cfg", "controlnet_cfg", "vae_cfg")}, sort_keys=True, default=str) + str(device) + weights
    if key in _SD_CACHE:
        return _SD_CACHE[key]
    _SD_CACHE[key] = _synthetic_state_dicts(cfg, device, weights)
    return _SD_CACHE[key]


def _synthetic_state_dicts(cfg: dict, device=None, weights: str = "smooth") -> Dict[str, Dict[str, torch.Tensor]]:
    gen = synth.WEIGHT_SETS[weights]
    specs = {
        "unet": arch.unet_param_spec(arch.unet_arch(cfg["unet_cfg"])),
        "controlnet": arch.unet_param_spec(arch.unet_arch(cfg["controlnet_cfg"], controlnet=True)),
        "vae": arch.vae_param_spec(cfg["vae_cfg"]),
    }
    return {part: {k: gen(f"{part}.{k}", shp, device=device) for k, shp in spec} for part, spec in specs.items()}


def build_synthetic_cldm(cfg: dict, device, dtype=None, sds=None, precision=None, weights: str = "smooth") -> ControlLDM:
    from .model.params import skip_init
    on_gpu = torch.device(device).type == "cuda"
    with skip_init(), torch.device(device if on_gpu else "cpu"):      # parameters are born on the device: no 5 GB host round trip
        model = ControlLDM(**cfg)
    sds = sds or synthetic_state_dicts(cfg, device if on_gpu else None, weights)   # hashed on the device: bit-identical to the host
    model.unet.load_state_dict(sds["unet"], strict=True)
    model.load_controlnet_from_ckpt(sds["controlnet"])
    model.vae.load_state_dict(sds["vae"], strict=True)
    if dtype is not None:
        model.compute_dtype = dtype
    if precision is not None:
        model.precision = model.controlnet.precision = model.unet.precision = precision
    return model.eval().to(device)


@contextlib.contextmanager
def injected_noise(noises: Iterable[torch.Tensor]):
    """Replace torch.randn_like by a fixed list (the sampler draws one per step, reference utils/sampler.py:199)."""
    it = iter(noises)
    orig = torch.randn_like
    torch.randn_like = lambda x, *a, **k: next(it).to(device=x.device, dtype=x.dtype)
    try:
        yield
    finally:
        torch.randn_like = orig


# ---------------------------------------------------------------------------------------------------------------------
# Buffer discipline of a launch program (tests/test_lanes_cpu.py) and the captured forms of the engines (tests/test_gpu_graphs.py)
# ---------------------------------------------------------------------------------------------------------------------
def tensor_range(t: torch.Tensor) -> Tuple[int, int]:
    """(first byte, end byte) of ``t``: from data_ptr() to its last element inclusive, sum((size - 1) * stride) + 1 elements — so
    two interleaved column slices of one buffer overlap (deliberately conservative)."""
    span = sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + span * t.element_size()


def rec_ranges(rec) -> Set[Tuple[int, int]]:
    """The (first byte, end byte) ranges of every non-empty tensor reachable from ``rec.keep`` (tuples and lists nest:
    ops.make_swin_layer keeps ``(attn.keep, mlp.keep)``; parameter structs, scalars and None are passed over)."""
    out: Set[Tuple[int, int]] = set()
    todo = [rec.keep]
    while todo:
        v = todo.pop()
        if isinstance(v, torch.Tensor):
            if v.numel():
                out.add(tensor_range(v))
        elif isinstance(v, (tuple, list)):
            todo.extend(v)
    return out


def ranges_overlap(A, B) -> Set[Tuple[int, int]]:
    """The members of ``A`` that intersect any member of ``B`` (half-open byte ranges).  B sorted by first byte with a running
    maximum of the end bytes: a range of A is hit iff one of the B ranges that begin before its end reaches past its start."""
    b = sorted(B)
    starts = [s for s, _ in b]
    reach, hi = [], 0
    for _, e in b:
        hi = max(hi, e)
        reach.append(hi)
    out = set()
    for s, e in A:
        n = bisect.bisect_left(starts, e)          # the B ranges with first byte < e
        if n and reach[n - 1] > s:
            out.add((s, e))
    return out


def capture_engines(cldm: ControlLDM, parallel_lanes: bool = True) -> None:
    """What bench.py's capture_all() does: every cached engine program that is not a hipGraph yet becomes one (the denoise step
    with its two lanes as two graph branches unless ``parallel_lanes`` is False; the context programs stay launch lists)."""
    for e in cldm._cldm_engines.values():
        if e.step_prog.graph is None:
            e.step_prog.capture(parallel_lanes=parallel_lanes)
    for e in cldm._vae_engines.values():
        if e.prog.graph is None:
            e.prog.capture()


def release_graphs(cldm: ControlLDM) -> None:
    """Back to eager replay: drop the hipGraph of every cached engine (the engines, their buffers and programs stay)."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()                   # a replay of one of these graphs may still be queued
    for e in cldm._cldm_engines.values():
        e.step_prog.release_graph()
        e.ctx_prog.release_graph()
    for e in cldm._vae_engines.values():
        e.prog.release_graph()


def program_signature(recs, arenas) -> list:
    """One line per launch record of a program: name, tag, flops, bytes, then every scalar argument and every field of every
    parameter struct verbatim — except pointers, which would differ from run to run and are written as ``0``, as
    ``A<arena>.<chunk>+<byte offset>`` inside a chunk of one of ``arenas`` (so allocation order and buffer reuse are part of the
    signature) or as ``X<k>``, k = order of first appearance in the program (weights and static buffers: cache sharing is part
    of it too).  Which arguments are pointers is read off the C prototypes (edtr_amd/lib.py).  tests/golden/program_signatures.json
    holds the hashes of these listings as recorded from the commit before a change (tools/make_program_signatures.py)."""
    import ctypes as ct
    chunks = sorted((c.data_ptr(), c.data_ptr() + c.numel(), f"A{ai}.{ci}") for ai, a in enumerate(arenas) for ci, c in enumerate(a.chunks))
    starts = [c[0] for c in chunks]
    foreign: Dict[int, int] = {}

    def pointer(v) -> str:
        if not v:
            return "0"
        i = bisect.bisect_right(starts, v) - 1
        if i >= 0 and v < chunks[i][1]:
            return f"{chunks[i][2]}+{v - chunks[i][0]}"
        return f"X{foreign.setdefault(v, len(foreign))}"

    def struct(s) -> str:
        return "{" + " ".join(f"{f}={pointer(getattr(s, f)) if t is ct.c_void_p else repr(getattr(s, f))}" for f, t in s._fields_) + "}"

    lines = []
    for r in recs:
        out = [r.name, r.tag, repr(float(r.flops)), repr(float(r.bytes))]
        for a, t in zip(r.args, r.fn.argtypes):
            if isinstance(getattr(a, "_obj", None), ct.Structure):      # byref(parameter struct)
                out.append(struct(a._obj))
            elif t is ct.c_void_p and (a is None or isinstance(a, int)):
                out.append(pointer(a))
            elif isinstance(a, (bool, int, float)):
                out.append(repr(a))
            else:
                raise TypeError(f"{r.name}: no canonical form for argument {a!r}")
        lines.append(" | ".join(out))
    return lines


def signature_summary(lines) -> Dict[str, object]:
    """What the golden table keeps of a listing: record count, SHA-256, launches per name (the counts make a mismatch legible) and
    six hex digits of every record's own SHA-256, in order (they name the first record that differs)."""
    import collections
    import hashlib
    names = collections.Counter(ln.split(" | ", 1)[0] for ln in lines)
    return {"records": len(lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(), "launches": dict(sorted(names.items())),
            "record_hashes": "".join(hashlib.sha256(ln.encode()).hexdigest()[:6] for ln in lines)}


def rel_err(a, b) -> float:
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def err_stats(a, b) -> Dict[str, float]:
    """Error of ``a`` against the reference ``b`` in the three norms the parity gates quote (BASELINE.md §3 asks for the "max
    relative error"; the relative L2 norm alone would hide a localised defect — one wrong halo column, one bad tile seam):
      l2     ||a - b||_2 / ||b||_2
      max    max|a - b| / max|b|                      (the worst element, relative to the signal's peak)
      p9999  99.99th percentile of |a - b| / max|b|   (the worst element outside 1e-4 of the tensor)"""
    a = torch.as_tensor(a).double().cpu().reshape(-1)
    b = torch.as_tensor(b).double().cpu().reshape(-1)
    d = (a - b).abs()
    peak = float(b.abs().max().clamp_min(1e-30))
    k = max(1, int(round(d.numel() * 1e-4)))
    p9999 = float(torch.topk(d, k).values[-1]) if d.numel() > 1 else float(d.max())
    return {"l2": float(d.norm() / b.norm().clamp_min(1e-30)), "max": float(d.max()) / peak, "p9999": p9999 / peak}


# ---------------------------------------------------------------------------------------------------------------------
# Rounding-aware element bound (the per-kernel parity tests).  A kernel that reads 16-bit operands, accumulates in fp32 and
# rounds its output once satisfies, element by element,
#     |got - ref| <= 2 u |ref| + k 2^-22 absref + extra + floor
# with ref in fp64 from exactly the 16-bit values the kernel reads, absref the same expression on absolute values
# (|alpha| |A| @ |W|^T + |bias| + |residual|, conv2d(|x|, |w|), ...), k the reduction length and u the unit roundoff of the
# stored output (2u = one ulp).  k 2^-22 absref bounds fp32 accumulation in any order generously (fp32 MFMA chains measure
# ~1e-7 sum|a b|); `extra` names the roundings a kernel performs on purpose (a 16-bit P before P V, a 16-bit hidden tensor);
# `floor` covers fp16 subnormals.  A correct kernel stays near 0.5; one wrong tile, seam, tail or column exceeds 1 even
# where the relative L2 norm of the whole tensor does not move.
# ---------------------------------------------------------------------------------------------------------------------
ACC_F32 = 2.0 ** -22                      # per-term fp32 accumulation slack (k 2^-22 absref)
LIPSCHITZ = {"none": 1.0, "silu": 1.1, "gelu": 1.13, "leaky": 1.0}
GELU_APPROX = 2.0e-7                      # csrc/common.h gelu_erf_f: A&S 7.1.26 erf (|err| <= 1.5e-7) + rcp / exp ulps, times 0.5 |x|


def unit_roundoff(dtype) -> float:
    """u of the stored output: 2^-8 bf16, 2^-11 fp16, 2^-24 fp32 (round to nearest: |fl(x) - x| <= u |x|)."""
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}[dtype]


def _floor(dtype) -> float:
    return 2.0 ** -24 if dtype == torch.float16 else 1e-300


def elem_bound(ref, absref, out_dtype, k, extra=None) -> torch.Tensor:
    """The bound above as an fp64 tensor of ref's shape (extra: {name: tensor or float}, every term added)."""
    ref = torch.as_tensor(ref).double().cpu()
    b = 2.0 * unit_roundoff(out_dtype) * ref.abs() + _floor(out_dtype)
    if absref is not None and k:
        b = b + float(k) * ACC_F32 * torch.as_tensor(absref).double().cpu()
    for term in (extra or {}).values():
        b = b + (torch.as_tensor(term).double().cpu() if torch.is_tensor(term) else float(term))
    return b


def elem_ratio(got, ref, absref, out_dtype, k, extra=None):
    """Worst |got - ref| / bound and where it occurs: (ratio, {"index", "got", "ref", "bound"}).  A non-finite `got` is inf."""
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    b = elem_bound(ref, absref, out_dtype, k, extra).expand(ref.shape)
    r = (got - ref).abs() / b
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    if r.numel() == 0:
        return 0.0, {}
    flat = int(torch.argmax(torch.nan_to_num(r, nan=float("inf"))))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), r.shape))
    info = {"index": idx, "got": float(got[idx]), "ref": float(ref[idx]), "bound": float(b[idx])}
    return float(r[idx]), info


def attn_elem_ratio(got, q, k, v, scale, dtype, out_dtype=None, causal=False, on_block=None) -> float:
    """Worst element ratio of softmax(scale q k^T) v against the kernel's [.., N, D] heads (q / k / v: the 16-bit values it reads).
    Two named terms besides the output rounding: the kernel packs P to 16 bits before P V (attention.hip, attn512.hip: pack2 of
    the fp32 probabilities) -> 2 u_in P|V|; the fp32 logits carry D 2^-22 |scale| |q||k|^T each, which moves the output by at
    most (P o delta)|V| + rowsum(P o delta) P|V|.  on_block(ratio, where) is called per 1024-query block (the tests record and
    assert there)."""
    kd, vd = torch.as_tensor(k).double().cpu(), torch.as_tensor(v).double().cpu()
    got = torch.as_tensor(got).double().cpu()
    worst = 0.0
    for r0 in range(0, q.shape[-2], 1024):           # query blocks: the fp64 score matrices stay small
        qd = q[..., r0:r0 + 1024, :].double().cpu()
        logits = (qd @ kd.transpose(-1, -2)) * scale
        delta = qd.shape[-1] * 2.0 ** -22 * abs(scale) * (qd.abs() @ kd.abs().transpose(-1, -2))
        if causal:
            rows = torch.arange(r0, r0 + qd.shape[-2])[:, None]
            logits = logits.masked_fill(torch.arange(kd.shape[-2])[None, :] > rows, float("-inf"))
        p = torch.softmax(logits, dim=-1)
        pv = p @ vd.abs()
        pd = p * delta
        extra = {"16-bit P before P V": 2.0 * unit_roundoff(dtype) * pv, "fp32 logits": pd @ vd.abs() + pd.sum(-1, keepdim=True) * pv}
        r, where = elem_ratio(got[..., r0:r0 + 1024, :], p @ vd, pv, out_dtype or dtype, kd.shape[-2], extra)
        if on_block is not None:
            on_block(r, where)
        worst = max(worst, r)
    return worst


def geglu_err(val, gate, ev, eg):
    """Absolute error bound of val * gelu(gate) when val / gate are off by at most ev / eg: the product rule with GELU's
    Lipschitz constant and the epilogue's erf approximation."""
    val, gate = torch.as_tensor(val).double(), torch.as_tensor(gate).double()
    eg = LIPSCHITZ["gelu"] * torch.as_tensor(eg).double() + GELU_APPROX * gate.abs()
    ev = torch.as_tensor(ev).double()
    return ev * torch.nn.functional.gelu(gate).abs() + val.abs() * eg + ev * eg


def geglu_slack(val, gate, abs_val, abs_gate, k):
    """geglu_err for val / gate that carry the fp32 accumulation error k 2^-22 abs_* (pass it as an `extra` term with k = 0)."""
    return geglu_err(val, gate, float(k) * ACC_F32 * torch.as_tensor(abs_val).double(), float(k) * ACC_F32 * torch.as_tensor(abs_gate).double())


def rounded_operand(v, dv, dtype):
    """A kernel rounds an fp32 intermediate to 16 bits on purpose (a normalised row, a hidden tensor) before multiplying it; the
    reference mirrors that rounding on its fp64 value v.  Where the kernel's fp32 value may differ from v by dv, it rounds to
    the same 16-bit value unless a rounding boundary lies within dv of v; there it may land one spacing away.  Returns
    (v rounded to dtype, in fp64; that spacing where a boundary lies within dv, else 0) — the second is the operand error
    to propagate, instead of assuming every operand is one ulp off."""
    v = torch.as_tensor(v).double()
    v16 = v.to(dtype).double()
    p = {torch.bfloat16: 8, torch.float16: 11}[dtype]
    emin = {torch.bfloat16: -126, torch.float16: -14}[dtype]
    e = torch.floor(torch.log2(v16.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    ulp = torch.pow(2.0, e - (p - 1))                                  # spacing above |v16|
    pow2 = (v16.abs() == torch.pow(2.0, e)) & (e > emin)
    below = torch.where(pow2, ulp / 2, ulp)                            # spacing below |v16| (half at a power of two)
    dist = torch.minimum(ulp, below) / 2 - (v - v16).abs()             # distance from v to the nearest rounding boundary
    dv = torch.as_tensor(dv).double() + 2.0 ** -23 * v.abs()          # (+ the fp32 representation of v itself, a tie at the boundary)
    return v16, torch.where(dist <= dv, ulp, torch.zeros_like(ulp))


def block_rel(got, ref, cols, block=32) -> float:
    """Worst relative L2 error over the block x block tiles of the [rows, cols] view, each tile's reference norm floored at
    the tensor's RMS (a tile of near-zero values does not turn rounding noise into a large ratio)."""
    got = torch.as_tensor(got).double().cpu().reshape(-1, cols)
    ref = torch.as_tensor(ref).double().cpu().reshape(-1, cols)
    rms = float(ref.pow(2).mean().sqrt())
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    rows = ref.shape[0]
    pr, pc = -rows % block, -cols % block
    d2 = torch.nn.functional.pad((got - ref) ** 2, (0, pc, 0, pr))
    f2 = torch.nn.functional.pad(ref ** 2, (0, pc, 0, pr))
    n = torch.nn.functional.pad(torch.ones_like(ref), (0, pc, 0, pr))

    def tiles(t):
        return t.reshape(t.shape[0] // block, block, t.shape[1] // block, block).sum((1, 3))
    den = torch.maximum(tiles(f2), rms * rms * tiles(n)).sqrt().clamp_min(1e-300)
    return float((tiles(d2).sqrt() / den).max())
