"""Thin torch-tensor front end over the C ABI (edtr_amd/lib.py).  torch is plumbing here: it owns the
device buffers and the stream; every computation is a libedtr_hip launch on torch's current stream.

Launch records: each ``make_*`` returns a ``(c_function, params_struct, keepalive)`` tuple that can
be replayed any number of times with ``launch(rec)`` — the engine (edtr_amd/engine.py) pre-builds
them once per shape so the steady-state host cost per kernel is one ctypes call.
"""
from __future__ import annotations

import ctypes as ct
import os
from typing import Optional, Sequence, Tuple

import torch

from . import lib as L

F32S = "f32_split"     # high-precision mode: fp32 activation stream, bf16 split-3 GEMM operands (edtr_hip.h EDTR_F32_SPLIT)
# mixed-precision mode: fp32 activation stream, fp16 GEMM operands of 1 / 2 / 3 parts (edtr_hip.h EDTR_F32_H1 / H2 / H3)
F32H = {1: "f32_h1", 2: "f32_h2", 3: "f32_h3"}
MIXED = "f32_mixed"    # WeightStore dtype of the mixed mode: fp16 matrices packed per requested part count
PARTS_2W = 4           # precision-policy code of the WEIGHTS-EXACT two-part product: x16 . [Wh | Wl] with the A columns read twice
_DT = {torch.bfloat16: L.BF16, torch.float16: L.F16, F32S: L.F32_SPLIT, F32H[1]: L.F32_H1, F32H[2]: L.F32_H2, F32H[3]: L.F32_H3}


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"libedtr_hip stores activations as bfloat16 or float16, got {dtype}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> Optional[int]:      # the address of a tensor; None and integer addresses pass through
    return t if t is None or isinstance(t, int) else t.data_ptr()


class Rec:
    """One pre-built kernel launch."""
    __slots__ = ("fn", "args", "keep", "name", "flops", "bytes", "tag")

    def __init__(self, fn, args, keep, name, flops=0.0, nbytes=0.0):
        self.fn, self.args, self.keep, self.name, self.flops, self.bytes = fn, args, keep, name, flops, nbytes
        self.tag = ""           # shape tag for the per-shape bench breakdown

    def launch(self, stream: int) -> None:
        code = self.fn(*self.args, stream)
        if code != 0:
            L.check(code, self.name)


def launch(rec: Rec) -> None:
    rec.launch(stream_ptr())


# --------------------------------------------------------------------------------------------
# igemm
# --------------------------------------------------------------------------------------------
IGEMM_POINTERS = ("a1", "a2", "w", "out", "bias_n", "bias_m", "rowvec", "residual", "workspace", "gn_partial", "vt_out", "row_stats",
                  "ln_stats", "ln_c1", "ln_c2", "out16", "a_gn", "a3")       # igemm_params' pointer keywords, in the order a record keeps them alive
PLAN_ADDR = 0x1000      # a 16-byte-aligned placeholder for the shape-only queries: the planner looks at addresses, never through them


def igemm_params(*, dtype: torch.dtype, a1, w, out, M: int, N: int, C1: int, ld1: int, ldw: int, ldc: int, taps: int = 1, a2=None,
                 C2: int = 0, ld2: int = 0, spatial: Optional[Tuple[int, int, int, int, int, int, int, int]] = None, Z: int = 1,
                 zdiv: int = 1, a_zs=(0, 0), w_zs=(0, 0), o_zs=(0, 0), alpha: float = 1.0, bias_n=None, bias_m=None, rowvec=None,
                 rowvec_ld: int = 0, rows_per_image: int = 0, act: int = 0, residual=None, ldr: int = 0, out_f32: bool = False,
                 n_valid: int = 0, tile: int = 0, splitk: int = 1, workspace=None, workspace_bytes: int = 0, gn_partial=None,
                 act_slope: float = 0.0, residual_f32: bool = False, vt_out=None, vt_col0: int = 0, vt_ld: int = 0, vt_alpha: float = 1.0,
                 row_stats=None, ln_stats=None, ln_C: int = 0, ln_valid: int = 0, ln_eps: float = 1e-5, ln_c1=None, ln_c2=None,
                 w_phase_stride: int = 0, out16=None, ld16: int = 0, a_wrap: int = 0, a_gn=None, a_gn_silu: bool = True,
                 gn_slot_rows: int = 0, gn_ld: int = 0, a3=None, C3: int = 0, ld3: int = 0, raw: Optional[dict] = None) -> L.IgemmParams:
    """edtr_igemm_params from keyword arguments: the one place that fills the struct.  Every pointer keyword (IGEMM_POINTERS) takes a
    tensor, an integer address or None; ``ld3``, ``ld16`` and ``workspace_bytes`` describe an a3 / out16 / workspace that is given as an
    address (a tensor says them itself).  ``raw``: struct fields set after everything else."""
    p, C3 = L.IgemmParams(), C3 if a3 is not None else 0
    p.dtype, p.taps, p.M, p.N, p.K = dt_code(dtype), taps, M, N, taps * (C1 + C2) + C3
    if a3 is not None:                    # K tail of a 3x3 convolution: C3 more columns read at the output pixel itself (the 1x1 skip)
        p.a3, p.C3, p.ld3 = ptr(a3), C3, ld3 or a3.stride(0)
    p.n_valid, p.Z, p.zdiv = n_valid, Z, zdiv
    p.a1, p.a2, p.C1, p.C2, p.ld1, p.ld2 = ptr(a1), ptr(a2), C1, C2, ld1, ld2
    p.a_zs_outer, p.a_zs_inner = a_zs
    if spatial is not None:
        p.IH, p.IW, p.OH, p.OW, p.stride, p.pad_t, p.pad_l, p.upsample2x = spatial
    p.w, p.ldw = ptr(w), ldw
    p.w_phase_stride = w_phase_stride     # sub-pixel upsample convolution (spatial[7] == 2): four pre-summed phase matrices
    if out16 is not None:                 # fp16 mirror of an fp32 stream output (mixed mode)
        p.out16, p.ld16 = ptr(out16), ld16 or out16.stride(0)
    p.a_wrap = a_wrap                     # weights-exact two-part product: A columns read twice against [Wh | Wl]
    p.a_gn, p.a_gn_silu = ptr(a_gn), int(a_gn_silu)     # GroupNorm apply (+ SiLU) of the input fused into the halo tile's staging
    p.gn_slot_rows, p.gn_ld = int(gn_slot_rows), int(gn_ld)
    p.w_zs_outer, p.w_zs_inner = w_zs
    p.alpha, p.bias_n, p.bias_m, p.rowvec = alpha, ptr(bias_n), ptr(bias_m), ptr(rowvec)
    p.rowvec_ld, p.rows_per_image, p.act = rowvec_ld, rows_per_image, act
    p.residual, p.ldr = ptr(residual), ldr
    p.out, p.ldc, p.out_f32 = ptr(out), ldc, int(out_f32)
    p.o_zs_outer, p.o_zs_inner = o_zs
    p.tile, p.splitk = tile, splitk
    if splitk > 1:
        p.workspace, p.workspace_bytes = ptr(workspace), workspace_bytes or workspace.numel() * workspace.element_size()
    p.gn_partial, p.act_slope, p.residual_f32 = ptr(gn_partial), act_slope, int(residual_f32)
    if vt_out is not None:
        p.vt_out, p.vt_col0, p.vt_ld, p.vt_alpha = ptr(vt_out), vt_col0, vt_ld, vt_alpha
    p.row_stats = ptr(row_stats)
    if ln_stats is not None:
        p.ln_stats, p.ln_slots, p.ln_C, p.ln_eps, p.ln_c1, p.ln_c2 = ptr(ln_stats), ln_C // 32, ln_valid or ln_C, ln_eps, ptr(ln_c1), ptr(ln_c2)
    for k, v in (raw or {}).items():
        setattr(p, k, v)
    return p


def make_igemm(*, name: str = "igemm", **kw) -> Rec:
    """The launch record of one edtr_igemm call.  The keywords are igemm_params', with tensors for the pointers."""
    p = igemm_params(**kw)
    has = {k: kw.get(k) is not None for k in IGEMM_POINTERS}
    M, N, Z, C1, C2, taps, act, splitk, spatial = p.M, p.N, p.Z, p.C1, p.C2, p.taps, p.act, p.splitk, kw.get("spatial")
    flops = 2.0 * M * N * p.K * Z
    # algorithmic HBM bytes: every operand once (a conv reads its input image once, not once per tap)
    a_rows = (M // (p.OH * p.OW)) * p.IH * p.IW if spatial else M
    n_out = N // 2 if act == L.ACT_GEGLU else N
    nbytes = Z * (2.0 * a_rows * (C1 + C2) + 2.0 * M * p.C3 + 2.0 * N * p.K + (4.0 if p.out_f32 else 2.0) * M * n_out
                  + ((4.0 if p.residual_f32 else 2.0) * M * n_out if has["residual"] else 0.0))
    rec = Rec(L.load().edtr_igemm, (ct.byref(p),), (p,) + tuple(kw.get(k) for k in IGEMM_POINTERS), name, flops, nbytes)
    rec.tag = (f"taps{taps} M{M} N{N} K{p.K} Z{Z}" + (f" C2={C2}" if C2 else "") + (f" s{p.stride}" if spatial and p.stride != 1 else "")
               + ((" up2" if p.upsample2x == 1 else " up2sp") if spatial and p.upsample2x else "") + (f" sk{splitk}" if splitk > 1 else "") + (f" act{act}" if act else "")
               + (" f32" if p.out_f32 else "") + (" gnp" if has["gn_partial"] else "") + (" vT" if has["vt_out"] else "") + (" ln" if has["ln_stats"] else "")
               + (" rs" if has["row_stats"] else "") + (" m16" if has["out16"] else "") + (" 2w" if p.a_wrap else "") + (" gnin" if has["a_gn"] else "")
               + (" kt" if has["a3"] else ""))
    return rec


def igemm_plan(*, raw: Optional[dict] = None, **kw) -> int:
    """edtr_igemm_plan for igemm_params' keywords, from shapes alone: the tile that would run, or the negative error.  PLAN_ADDR stands
    in for a1, w and out, for a split-K workspace (of splitk * M * N * 4 bytes) and for every pointer keyword given as True.  No
    launch, no device.  ``raw``: struct fields set after everything else (a K that does not count its tail ...)."""
    slabs = dict(workspace=PLAN_ADDR, workspace_bytes=kw["splitk"] * kw["M"] * kw["N"] * 4) if kw.get("splitk", 1) > 1 else {}
    kw = {"a1": PLAN_ADDR, "w": PLAN_ADDR, "out": PLAN_ADDR, **slabs,
          **{k: (PLAN_ADDR if v else None) if k in IGEMM_POINTERS and isinstance(v, bool) else v for k, v in kw.items()}}
    return int(L.load().edtr_igemm_plan(ct.byref(igemm_params(raw=raw, **kw))))


def conv3x3_plan(B: int, H: int, W: int, C: int, N: int, *, dtype: torch.dtype = torch.bfloat16, ld: int = 0, splitk: int = 1,
                 tail: Optional[Tuple[int, int]] = None, subpixel: bool = False, raw: Optional[dict] = None, **kw) -> int:
    """igemm_plan for the 3x3 / stride 1 / pad 1 convolution of a [B, H, W, C] activation (row stride ``ld`` or C) into N channels.
    ``tail`` = (C3, ld3): with a K tail of C3 columns; ``subpixel``: the sub-pixel form of the nearest-2x upsample convolution (four
    phase matrices of [N][4 C]).  Further keywords (a_gn=True, tile, residual ...) are igemm_plan's."""
    up, (C3, ld3) = 2 if subpixel else 1, tail or (0, 0)
    weights = dict(ldw=4 * C, w_phase_stride=N * 4 * C) if subpixel else dict(ldw=9 * C + C3)
    return igemm_plan(dtype=dtype, taps=9, M=B * up * H * up * W, N=N, C1=C, ld1=ld or C, ldc=N, splitk=splitk,
                      spatial=(H, W, up * H, up * W, 1, 1, 1, 2 if subpixel else 0), a3=bool(tail), C3=C3, ld3=ld3, raw=raw, **weights, **kw)


def ktail_plan(dtype: torch.dtype, B: int, H: int, W: int, C1: int, ld1: int, N: int, C3: int, ld3: int, splitk: int = 1, a_gn: bool = False) -> int:
    """conv3x3_plan with a K tail of C3 columns: the tile that would run (16 / 17 / 20), or < 0 where no tile takes the tail at that shape."""
    return conv3x3_plan(B, H, W, C1, N, dtype=dtype, ld=ld1, splitk=splitk, a_gn=a_gn, tail=(C3, ld3))


def ktail_enabled() -> bool:
    """EDTR_KTAIL=0 keeps the 1x1 skip convolutions of the width-changing ResBlocks as launches of their own (A/B runs); the default
    folds them into conv2 as a K tail (edtr_hip.h: a3) wherever the halo tile of that shape takes one."""
    return os.environ.get("EDTR_KTAIL", "1") != "0"


LN_FOLD_MAX_BATCH = 4     # UNet / ControlNet LayerNorm fold: on by default up to this batch size (engine.Emitter.ln_fold_ok has the measurements)


def batch_invariant() -> bool:
    """EDTR_AMD_BATCH_INVARIANT=1: launch choices must not depend on the batch size (engine.Emitter)."""
    return os.environ.get("EDTR_AMD_BATCH_INVARIANT", "0") == "1"


def invariant_tile(C1: int, C2: int) -> int:
    """The one tile geometry of the batch-invariant mode: the 128x128 LDS-DMA loop where the operand layout allows it
    (Cin % 64 == 0, no fused concat), the 128x128 register-staged loop otherwise — never chosen from M."""
    return 3 if (C1 % 64 == 0 and not C2) else 1


def choose_splitk(M: int, N: int, K: int, Z: int = 1, act: int = 0, img8: bool = False) -> Tuple[int, int]:
    """(tile, splitk) heuristic for the 256-CU MI355X: when the 128x128 tile grid cannot fill the chip, cut K so
    that ~480 workgroups exist — but only while every split keeps enough K-tiles (of 64) to amortise the fp32 slab
    round trip of the reducer: >= 20 per split (>= 12 when fewer than 64 tiles exist at all).  Measured with
    tools/bench_kernels.py gsplitk / splitk: M=2048 N=1280 K=1280 runs 18.5 us unsplit vs 24.8 us at 3 splits, while
    K=5120 gains (53.5 -> 42.3 us) and the 8x8-level convolutions (M=512, K=11520) gain 3.4x at 6 splits."""
    if Z != 1 or act == L.ACT_GEGLU:
        return 0, 1
    if img8 and M % 256 == 0 and N % 128 == 0 and K % (9 * 64) == 0 and K // (9 * 64) >= 10 and (M // 256) * (N // 128) <= 64:
        # 3x3 convolutions of the 8x8 latent level on the halo kernel's 4-images-per-workgroup geometry: split over the
        # 64-channel chunks so that every workgroup multiplies 2 (K = 11520) .. 4 (K = 23040) chunks.  Measured
        # (profiles/r03/ab_tiles_3_vs_16_smallm.log, one device): 31.1 us at 10 splits against 36.7 us for the 128x128 loop at its
        # 6 splits (K = 11520), 42.2 against 59.3 us (K = 23040); batch 4: 27.1 against 33.1 us
        return 0, 10
    nkt = (K + 63) // 64
    b128 = ((M + 127) // 128) * ((N + 127) // 128)
    if b128 >= 200 or nkt < 24:
        return 0, 1
    want = max(1, round(480 / b128))
    per_split = 12 if b128 <= 64 else 20
    s = max(1, min(want, nkt // per_split, 6))
    return 0, s      # tile 0 = library default (LDS-DMA 128x128 main loop whenever Cin % 64 == 0)


# --------------------------------------------------------------------------------------------
# attention
# --------------------------------------------------------------------------------------------
def make_flash_attn(*, dtype, q, k, vt, out, B, H, Nq, Nk, q_bs, q_ld, k_bs, k_ld, vt_bs, vt_ld, o_bs, o_ld,
                    scale: float, causal: bool = False, prescaled: bool = False, q_lo=None, k_lo=None, vt_lo=None,
                    out_f32: bool = False, name: str = "flash_attn64") -> Rec:
    """``q_lo`` / ``k_lo`` (/ ``vt_lo``): low halves of hi + lo operand pairs, same strides as q / k / vt (edtr_hip.h: split operands)."""
    p = L.AttnParams()
    p.dtype, p.B, p.H, p.Nq, p.Nk = dt_code(dtype), B, H, Nq, Nk
    p.q, p.q_bs, p.q_ld = ptr(q), q_bs, q_ld
    p.k, p.k_bs, p.k_ld = ptr(k), k_bs, k_ld
    p.vt, p.vt_bs, p.vt_ld = ptr(vt), vt_bs, vt_ld
    p.out, p.o_bs, p.o_ld = ptr(out), o_bs, o_ld
    p.scale = scale
    p.causal = int(causal)
    p.q_prescaled = int(prescaled)
    p.q_lo, p.k_lo, p.vt_lo, p.out_f32 = ptr(q_lo), ptr(k_lo), ptr(vt_lo), int(out_f32)
    flops = 4.0 * B * H * Nq * Nk * 64
    # algorithmic HBM bytes: Q and O once, K and V^T once per (image, head)
    nbytes = 2.0 * B * H * 64 * (2 * Nq + 2 * Nk)
    rec = Rec(L.load().edtr_flash_attn64, (ct.byref(p),), (p, q, k, vt, out, q_lo, k_lo, vt_lo), name, flops, nbytes)
    rec.tag = f"attn B{B} H{H} Nq{Nq} Nk{Nk}" + (" causal" if causal else "") + (" split" if q_lo is not None else "") + (" pv" if vt_lo is not None else "")
    return rec


ATTN_GENERIC, ATTN_SPLIT_QK, ATTN_SPLIT_QKPV, ATTN_SMALLK, ATTN_V3 = 1, 2, 3, 4, 5       # edtr_hip.h: enum edtr_attn_kernel


def flash_attn_plan(rec: Rec) -> Tuple[int, int]:
    """edtr_flash_attn64_plan of a make_flash_attn record: (kernel id or negative error code, the small-Nk kernel's 32-query blocks
    per workgroup or 0).  The launch dispatches on the same function; no HIP call, no device."""
    bpw = ct.c_int32(0)
    code = int(L.load().edtr_flash_attn64_plan(rec.args[0], ct.byref(bpw)))
    return code, int(bpw.value)


def flash_attn_plan_shape(dtype, B: int, H: int, Nq: int, Nk: int, *, causal: bool = False, prescaled: bool = False, split: int = 0,
                          out_f32: bool = False, q_ld: int = 0, k_ld: int = 0, vt_ld: int = 0, o_ld: int = 0) -> Tuple[int, int]:
    """flash_attn_plan from shapes alone (the pointers are placeholders; dense strides unless given).  split: 0 = one part,
    1 = q_lo / k_lo, 2 = and vt_lo."""
    p = L.AttnParams()
    C, fake = H * 64, 0x1000
    q_ld, k_ld, vt_ld, o_ld = q_ld or C, k_ld or C, vt_ld or round_up(Nk, 8), o_ld or C
    p.dtype, p.B, p.H, p.Nq, p.Nk = dt_code(dtype), B, H, Nq, Nk
    p.q, p.q_bs, p.q_ld = fake, Nq * q_ld, q_ld
    p.k, p.k_bs, p.k_ld = fake, Nk * k_ld, k_ld
    p.vt, p.vt_bs, p.vt_ld = fake, C * vt_ld, vt_ld
    p.out, p.o_bs, p.o_ld = fake, Nq * o_ld, o_ld
    p.scale, p.causal, p.q_prescaled, p.out_f32 = 0.125, int(causal), int(prescaled), int(out_f32)
    if split:
        p.q_lo = p.k_lo = fake
    if split > 1:
        p.vt_lo = fake
    bpw = ct.c_int32(0)
    code = int(L.load().edtr_flash_attn64_plan(ct.byref(p), ct.byref(bpw)))
    return code, int(bpw.value)


def flash_attn512_ok(N: int, C: int) -> bool:
    """Does edtr_flash_attn512 take the VAE's single-head attention over N positions of C channels?  (head width 512, whole 32-key
    tiles; EDTR_ATTN512=0 keeps the GEMM -> softmax -> GEMM form for A/B runs)"""
    return os.environ.get("EDTR_ATTN512", "1") != "0" and C == 512 and N % 32 == 0


def make_flash_attn512(*, dtype, q, k, vt, out, B, N, q_bs, q_ld, k_bs, k_ld, vt_bs, vt_ld, o_bs, o_ld, scale: float, out_f32: bool = False,
                       name: str = "flash_attn512") -> Rec:
    """The VAE AttnBlock's softmax(q k^T scale) v in one launch (edtr_hip.h: edtr_flash_attn512): q / k rows of 512 channels, vt = V^T."""
    p = L.AttnParams()
    p.dtype, p.B, p.H, p.Nq, p.Nk = dt_code(dtype), B, 1, N, N
    p.q, p.q_bs, p.q_ld = ptr(q), q_bs, q_ld
    p.k, p.k_bs, p.k_ld = ptr(k), k_bs, k_ld
    p.vt, p.vt_bs, p.vt_ld = ptr(vt), vt_bs, vt_ld
    p.out, p.o_bs, p.o_ld = ptr(out), o_bs, o_ld
    p.scale, p.out_f32 = scale, int(out_f32)
    flops = 4.0 * B * N * N * 512
    nbytes = 2.0 * B * 512 * (3 * N) + (4.0 if out_f32 else 2.0) * B * N * 512
    rec = Rec(L.load().edtr_flash_attn512, (ct.byref(p),), (p, q, k, vt, out), name, flops, nbytes)
    rec.tag = f"attn512 B{B} N{N}" + (" f32" if out_f32 else "")
    return rec


def make_window_attn(*, dtype, qkv, ld_qkv, out, ld_out, B, H, W, heads, head_dim, c_pad, shift, bias, labels, scale,
                     name: str = "window_attn") -> Rec:
    """SwinIR shifted-window attention (edtr_hip.h: edtr_window_attn): qkv [B*H*W, 3*heads*32] -> out [B*H*W, c_pad]."""
    p = L.WindowAttnParams()
    p.dtype, p.B, p.H, p.W, p.heads, p.head_dim, p.shift = dt_code(dtype), B, H, W, heads, head_dim, shift
    p.qkv, p.ld_qkv, p.out, p.ld_out, p.c_pad = ptr(qkv), ld_qkv, ptr(out), ld_out, c_pad
    p.bias, p.labels, p.scale = ptr(bias), ptr(labels), scale
    tokens = B * H * W
    flops = 4.0 * tokens * 64 * heads * head_dim
    nbytes = 2.0 * tokens * (3 * heads * 32 + heads * head_dim)
    return Rec(L.load().edtr_window_attn, (ct.byref(p),), (p, qkv, out, bias, labels), name, flops, nbytes)


SWIN_MLP_C, SWIN_MLP_HIDDEN = 192, 384          # the one shape edtr_swin_mlp is built for (include/edtr_hip.h)


def _swin_image_rows(w: torch.Tensor) -> torch.Tensor:
    """16-bit [32 t, 192] -> t LDS images of a 32-row tile: chunk c of row r in slot c ^ ((r >> 1) & 7) (edtr_hip.h: edtr_swin_mlp w1)."""
    T, C = w.shape[0] // 32, w.shape[1]
    a = w.reshape(T, 32, C // 8, 8)
    r = torch.arange(32, device=w.device)[:, None]
    c = torch.arange(C // 8, device=w.device)[None, :]
    img = torch.empty_like(a)
    img[:, r, c ^ ((r >> 1) & 7)] = a[:, r, c]
    return img.reshape(-1).contiguous()


def _swin_image_slices(w: torch.Tensor) -> torch.Tensor:
    """16-bit [192, 32 t] -> t LDS images of a 32-column slice: chunk c of row r in slot c ^ ((r >> 2) & 3) (edtr_swin_mlp w2)."""
    C, T = w.shape[0], w.shape[1] // 32
    b = w.reshape(C, T, 4, 8).permute(1, 0, 2, 3)
    r = torch.arange(C, device=w.device)[:, None]
    c = torch.arange(4, device=w.device)[None, :]
    img = torch.empty((T, C, 4, 8), dtype=w.dtype, device=w.device)
    img[:, r, c ^ ((r >> 2) & 3)] = b[:, r, c]
    return img.reshape(-1).contiguous()


def pack_swin_mlp_weights(w1g: torch.Tensor, w2: torch.Tensor, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 [384, 192] (gamma-scaled fc1) and [192, 384] (fc2), both already zero-padded -> the two LDS-image tensors
    edtr_swin_mlp copies by LDS-DMA (layout: include/edtr_hip.h, edtr_swin_mlp_params.w1 / .w2)."""
    assert tuple(w1g.shape) == (SWIN_MLP_HIDDEN, SWIN_MLP_C) and tuple(w2.shape) == (SWIN_MLP_C, SWIN_MLP_HIDDEN)
    return _swin_image_rows(w1g.to(dtype)), _swin_image_slices(w2.to(dtype))


SWIN_ATTN_HEADS = 6          # the one structure edtr_swin_attn is built for: 6 heads of <= 32 columns, 192 token columns, window 8


def pack_swin_attn_weights(wqkv: torch.Tensor, wproj: torch.Tensor, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 [3 * heads * 32, 192] (the head-padded, gamma- and q-scaled qkv matrix, rows (s, h, e) as model.swinir.pack_qkv orders
    them) and [192, heads * 32] (proj with head-padded input columns) -> the LDS images of edtr_swin_attn (edtr_hip.h)."""
    H = SWIN_ATTN_HEADS
    assert tuple(wqkv.shape) == (3 * H * 32, SWIN_MLP_C) and tuple(wproj.shape) == (SWIN_MLP_C, H * 32)
    by_head = wqkv.reshape(3, H, 32, SWIN_MLP_C).permute(1, 0, 2, 3).reshape(3 * H * 32, SWIN_MLP_C)        # image 3 h + s
    return _swin_image_rows(by_head.to(dtype)), _swin_image_slices(wproj.to(dtype))


def swin_attn_bias(bias: torch.Tensor) -> torch.Tensor:
    """[heads, 64 queries, 64 keys] (model.swinir.expand_bias) -> [heads, 16 key groups, 64 queries, 4] for edtr_swin_attn."""
    h = bias.shape[0]
    return bias.reshape(h, 64, 16, 4).permute(0, 2, 1, 3).contiguous()


def make_swin_attn(*, dtype, x, ldx, out, ldo, B, H, W, head_dim, shift, c_valid, eps, wqkv, wproj, c1, c2b, bproj, bias, labels,
                   name="swin.attn") -> Rec:
    """One Swin layer's x + proj(WindowAttention(LayerNorm(x))) (edtr_hip.h: edtr_swin_attn)."""
    p = L.SwinAttnParams()
    p.dtype, p.B, p.H, p.W, p.heads, p.head_dim, p.shift = dt_code(dtype), B, H, W, SWIN_ATTN_HEADS, head_dim, shift
    p.C, p.c_valid, p.eps = SWIN_MLP_C, c_valid, eps
    p.x, p.ldx, p.out, p.ldo = ptr(x), ldx, ptr(out), ldo
    p.wqkv, p.wproj, p.c1, p.c2b, p.bproj, p.bias, p.labels = ptr(wqkv), ptr(wproj), ptr(c1), ptr(c2b), ptr(bproj), ptr(bias), ptr(labels)
    tokens = B * H * W
    flops = 2.0 * tokens * SWIN_MLP_C * 4 * SWIN_ATTN_HEADS * 32 + 4.0 * tokens * 64 * SWIN_ATTN_HEADS * head_dim
    nbytes = 2.0 * tokens * 2 * SWIN_MLP_C + 2.0 * 4 * SWIN_ATTN_HEADS * 32 * SWIN_MLP_C
    return Rec(L.load().edtr_swin_attn, (ct.byref(p),), (p, x, out, wqkv, wproj, c1, c2b, bproj, bias, labels), name, flops, nbytes)


def make_swin_mlp(*, dtype, x, ldx, rows, c_valid, eps, w1, w2, c1, c2b, b2, out, ldo, row_stats=None, name="swin.mlp") -> Rec:
    """One Swin layer's x + fc2(GELU(fc1(LayerNorm(x)))) (edtr_hip.h: edtr_swin_mlp)."""
    p = L.SwinMlpParams()
    p.dtype, p.rows, p.C, p.hidden, p.c_valid, p.eps = dt_code(dtype), rows, SWIN_MLP_C, SWIN_MLP_HIDDEN, c_valid, eps
    p.x, p.ldx, p.w1, p.w2 = ptr(x), ldx, ptr(w1), ptr(w2)
    p.c1, p.c2b, p.b2 = ptr(c1), ptr(c2b), ptr(b2)
    p.out, p.ldo, p.row_stats = ptr(out), ldo, ptr(row_stats)
    flops = 4.0 * rows * SWIN_MLP_C * SWIN_MLP_HIDDEN
    nbytes = 2.0 * rows * 2 * SWIN_MLP_C + 4.0 * SWIN_MLP_C * SWIN_MLP_HIDDEN
    return Rec(L.load().edtr_swin_mlp, (ct.byref(p),), (p, x, w1, w2, c1, c2b, b2, out, row_stats), name, flops, nbytes)


FFN_D, FFN_H, FFN_ROWS = 320, 1280, 128       # what edtr_ffn is built for (include/edtr_hip.h)
FFN_PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def ffn_ok(M: int, D: int, H: int) -> bool:
    """Does edtr_ffn (the feed-forward half of a transformer block in one launch) take this shape — and is it the faster form?  A
    workgroup owns 128 tokens for the WHOLE hidden dimension, so the launch lasts ~95 us however few rows there are: it pays where the
    rows fill at least half the chip (batch 8: 256 workgroups, + 1.4 % on the whole path; batch 4: 128 workgroups beside the other lane's
    launches, + 0.7 %), not on the 4096 rows of a latent tile of the tiled sampler (32 workgroups against two ~20-us GEMMs).
    EDTR_FFN=0 keeps the two-GEMM form everywhere (A/B runs); EDTR_FFN_MIN_ROWS overrides the threshold."""
    if os.environ.get("EDTR_FFN", "1") == "0" or D != FFN_D or H != FFN_H or M <= 0 or M % FFN_ROWS:
        return False
    return M >= int(os.environ.get("EDTR_FFN_MIN_ROWS", "16384"))


def pack_ffn_w2(w2: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[D, H] fp32 -> 16-bit with the columns permuted inside every aligned group of 16 (edtr_hip.h: edtr_ffn_params.w2)."""
    d, hid = w2.shape
    assert hid % 16 == 0
    perm = (torch.arange(hid // 16, device=w2.device)[:, None] * 16 + torch.tensor(FFN_PERM16, device=w2.device)[None, :]).reshape(-1)
    return w2[:, perm].to(dtype).contiguous()


def pack_ffn_constants(c2b: torch.Tensor) -> torch.Tensor:
    """The per-unit constants W1 beta + b1 in edtr_ffn's per-chunk order (edtr_hip.h: edtr_ffn_params.cst).  ``c2b`` is indexed by the
    PACKED (value / gate interleaved) w1 row; gate entries are stored halved."""
    n = c2b.numel()
    assert n % 128 == 0
    dev = c2b.device
    c, hh, q, vg, lh, e = torch.meshgrid(torch.arange(n // 128, device=dev), torch.arange(2, device=dev), torch.arange(4, device=dev),
                                         torch.arange(2, device=dev), torch.arange(2, device=dev), torch.arange(4, device=dev), indexing="ij")
    R = 128 * c + 64 * hh + 32 * vg + e + 8 * q + 4 * lh
    out = c2b.float()[R] * torch.where(vg == 1, 0.5, 1.0)
    return out.reshape(-1).contiguous()                      # [chunk][half][q][vg][lh][e]


def make_ffn(*, dtype, x, ldx, M, w1, w2, cst, b2, out, ldo, eps=1e-5, name="ff.fused") -> Rec:
    """x + ff(LayerNorm(x)) in one launch (edtr_hip.h: edtr_ffn)."""
    p = L.FfnParams()
    p.dtype, p.M, p.D, p.H, p.eps = dt_code(dtype), M, FFN_D, FFN_H, eps
    p.x, p.ldx, p.w1, p.w2, p.cst, p.b2 = ptr(x), ldx, ptr(w1), ptr(w2), ptr(cst), ptr(b2)
    p.out, p.ldo = ptr(out), ldo
    flops = 2.0 * M * FFN_D * 3 * FFN_H
    nbytes = 2.0 * M * 2 * FFN_D + 2.0 * 3 * FFN_D * FFN_H
    rec = Rec(L.load().edtr_ffn, (ct.byref(p),), (p, x, w1, w2, cst, b2, out), name, flops, nbytes)
    rec.tag = f"ffn M{M} D{FFN_D} H{FFN_H}"
    return rec


LIN320_K, LIN320_ROWS = 320, 128              # what edtr_lin320 is built for (include/edtr_hip.h)


def lin320_ok(M: int, N: int, K: int, ln: bool = False) -> bool:
    """Does edtr_lin320 (a K = 320 linear layer as a row-resident product, optionally behind its LayerNorm) take this shape — and is it
    the faster form?  Measured against the launches it replaces (profiles/r06/lin320_time.log): with a LayerNorm in front and N = 320 it
    wins from half a chip of 128-row workgroups (16384 rows: 15 against 20 us), everything else from a full one (32768 rows; at 16384 the
    plain forms and the N = 960 projection are 4 - 17 % slower than edtr_igemm's tiles).  EDTR_LIN320=0 keeps the edtr_igemm form
    everywhere (A/B runs); EDTR_LIN320_MIN_ROWS overrides the thresholds."""
    if os.environ.get("EDTR_LIN320", "1") == "0" or K != LIN320_K or M <= 0 or M % LIN320_ROWS or N % 64 or N > 1024:
        return False
    env = os.environ.get("EDTR_LIN320_MIN_ROWS")
    return M >= (int(env) if env else (16384 if (ln and N <= 320) else 32768))


def pack_lin320_w(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[N, 320] fp32 -> 16-bit in edtr_lin320's fragment order (edtr_hip.h: edtr_lin320_params.w): 16 bytes per (chunk of 32 rows, k-step of
    16, lane) = w[32 c + (lane & 31)][16 s + 8 (lane >> 5) .. + 7]."""
    n, k = w.shape
    assert k == LIN320_K and n % 32 == 0
    w16 = w.to(dtype).reshape(n // 32, 32, k // 16, 2, 8)            # [c][l31][s][lh][8]
    return w16.permute(0, 2, 3, 1, 4).contiguous().reshape(-1)         # [c][s][lh][l31][8]: lane = 32 lh + l31


def make_lin320(*, dtype, x, ldx, M, N, w, cvec=None, alpha=1.0, ln=False, eps=1e-5, residual=None, ldr=0, out, ldo, vt_out=None, vt_col0=0,
                vt_ld=0, vt_alpha=1.0, rows_per_image=0, gn_table=None, name="lin320") -> Rec:
    """out = alpha * (LayerNorm?)(x) w^T + cvec (+ residual) in one launch; the columns from ``vt_col0`` on transposed into ``vt_out`` (the V^T
    operand of a fused [Wq; Wk; Wv] projection) where given (edtr_hip.h: edtr_lin320)."""
    p = L.Lin320Params()
    p.dtype, p.M, p.N, p.K, p.ln, p.eps, p.alpha = dt_code(dtype), M, N, LIN320_K, int(ln), eps, alpha
    p.x, p.ldx, p.w, p.cvec = ptr(x), ldx, ptr(w), ptr(cvec)
    p.residual, p.ldr, p.out, p.ldo = ptr(residual), ldr, ptr(out), ldo
    p.vt_out, p.vt_col0, p.vt_ld, p.vt_alpha, p.rows_per_image = ptr(vt_out), vt_col0, vt_ld, vt_alpha, rows_per_image
    p.gn_table = ptr(gn_table)
    flops = 2.0 * M * N * LIN320_K
    nbytes = 2.0 * M * (LIN320_K + N * (2 if residual is not None else 1)) + 2.0 * N * LIN320_K
    rec = Rec(L.load().edtr_lin320, (ct.byref(p),), (p, x, w, cvec, residual, out, vt_out, gn_table), name, flops, nbytes)
    rec.tag = (f"lin320 M{M} N{N}" + (" ln" if ln else "") + (" gnin" if gn_table is not None else "") + (" res" if residual is not None else "")
               + (" vT" if vt_out is not None else ""))
    return rec


def make_swin_layer(attn: Rec, mlp: Rec, name="swin.layer") -> Rec:
    """A whole Swin layer in one launch from the two half-layer records (edtr_hip.h: edtr_swin_layer): the attention record's x / out
    are the layer's input / output, the MLP record contributes its weights and constants."""
    pa, pm = attn.keep[0], mlp.keep[0]
    return Rec(L.load().edtr_swin_layer, (ct.byref(pa), ct.byref(pm)), (attn.keep, mlp.keep), name, attn.flops + mlp.flops,
               attn.bytes + mlp.bytes - 4.0 * pa.B * pa.H * pa.W * SWIN_MLP_C)


def pack_conv64_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[Cout <= 64, 64 (or fewer, zero padded), 3, 3] fp32 -> the nine 8-KiB LDS images of edtr_conv64 (edtr_hip.h)."""
    co, ci, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and co <= 64 and ci <= 64
    full = torch.zeros((9, 64, 8, 8), dtype=torch.float32, device=w.device)                   # [tap][n][chunk][j]
    full.reshape(9, 64, 64)[:, :co, :ci] = w.permute(2, 3, 0, 1).reshape(9, co, ci)
    n = torch.arange(64, device=w.device)[:, None]
    c = torch.arange(8, device=w.device)[None, :]
    img = torch.empty_like(full)
    img[:, n, c ^ ((n >> 1) & 7)] = full[:, n, c]
    return img.to(dtype).reshape(-1).contiguous()


def pack_conv128_out_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[Cout <= 32, 128, 3, 3] fp32 -> the nine 8-KiB LDS images of edtr_conv128_out (edtr_hip.h)."""
    co, ci, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and co <= 32 and ci == 128
    full = torch.zeros((9, 32, 16, 8), dtype=torch.float32, device=w.device)                  # [tap][n][chunk][j]
    full.reshape(9, 32, 128)[:, :co] = w.permute(2, 3, 0, 1).reshape(9, co, ci)
    n = torch.arange(32, device=w.device)[:, None]
    c = torch.arange(16, device=w.device)[None, :]
    img = torch.empty_like(full)
    img[:, n, c ^ (n & 15)] = full[:, n, c]
    return img.to(dtype).reshape(-1).contiguous()


def conv128_out_ok(H: int, W: int, cin: int, cout: int) -> bool:
    """Does edtr_conv128_out take this convolution (the VAE decoder's conv_out)?  EDTR_CONV128_OUT=0 keeps the three launches."""
    return os.environ.get("EDTR_CONV128_OUT", "1") != "0" and cin == 128 and cout <= 4 and H % 16 == 0 and W % 16 == 0


def make_conv128_out(*, dtype, x, ldx, w, bias, out, B, H, W, n_valid, gn_table=None, alpha=1.0, name="vae.conv_out") -> Rec:
    p = L.Conv128OutParams()
    p.dtype, p.B, p.H, p.W = dt_code(dtype), B, H, W
    p.x, p.ldx, p.gn_table, p.w, p.bias = ptr(x), ldx, ptr(gn_table), ptr(w), ptr(bias)
    p.alpha, p.out, p.n_valid = alpha, ptr(out), n_valid
    flops = 2.0 * B * H * W * 128 * 9 * n_valid
    nbytes = 2.0 * B * H * W * 128 + 4.0 * B * H * W * n_valid
    return Rec(L.load().edtr_conv128_out, (ct.byref(p),), (p, x, w, bias, out, gn_table), name, flops, nbytes)


def conv64_ok(H: int, W: int, cin: int, cout: int) -> bool:
    """Does edtr_conv64 take this 3x3 convolution (output H x W)?  EDTR_CONV64=0 keeps edtr_igemm (A/B runs)."""
    return os.environ.get("EDTR_CONV64", "1") != "0" and cin == 64 and cout <= 64 and H % 16 == 0 and W % 16 == 0


def make_conv64(*, dtype, x, ldx, w, bias, out, B, H, W, upsample2x=False, act=0, act_slope=0.0, alpha=1.0, ldo=0, out_nchw_f32=False,
                n_valid=0, name="conv64") -> Rec:
    p = L.Conv64Params()
    p.dtype, p.B, p.H, p.W, p.upsample2x = dt_code(dtype), B, H, W, int(upsample2x)
    p.x, p.ldx, p.w, p.bias = ptr(x), ldx, ptr(w), ptr(bias)
    p.act, p.act_slope, p.alpha = act, act_slope, alpha
    p.out, p.ldo, p.out_nchw_f32, p.n_valid = ptr(out), ldo, int(out_nchw_f32), n_valid
    flops = 2.0 * B * H * W * 64 * 9 * (n_valid if out_nchw_f32 else 64)
    src = B * H * W * 64 * 2 / (4 if upsample2x else 1)
    nbytes = src + (B * H * W * n_valid * 4 if out_nchw_f32 else B * H * W * 64 * 2)
    return Rec(L.load().edtr_conv64, (ct.byref(p),), (p, x, w, bias, out), name, flops, nbytes)


# --------------------------------------------------------------------------------------------
# norms
# --------------------------------------------------------------------------------------------
def make_embed_tokens(*, dtype, tokens, table, pos, rows, L_ctx, D, out, ld, name="embed_tokens") -> Rec:
    args = (dt_code(dtype), ptr(tokens), ptr(table), ptr(pos), rows, L_ctx, D, table.shape[0], ptr(out), ld)
    return Rec(L.load().edtr_embed_tokens, args, (tokens, table, pos, out), name, 0.0, 10.0 * rows * D)


def make_zero(t: torch.Tensor, name: str = "zero") -> Rec:
    nbytes = t.numel() * t.element_size()
    return Rec(L.load().edtr_zero_bytes, (ptr(t), nbytes), (t,), name, 0.0, float(nbytes))


# edtr_gn_apply folds the producer's per-tile partials itself up to this many 128-row tiles per image (the kernel accepts 64).
# Every one of the apply launch's ~2000 workgroups repeats the fold for its channels, so it only pays while tiles x channels is
# small next to a workgroup's own slab: the 16x16 and 32x32 latent levels (2 / 8 tiles); at 64x64 (32 tiles) the whole path
# lost 6 % (profiles/r03/experiments_gn_fold.log) and the separate edtr_gn_finalize launch stays.
GN_FOLD_MAX_TILES = int(__import__("os").environ.get("EDTR_GN_FOLD_MAX", "8"))


def gn_foldable(HW: int, C: int, groups: int = 32, tiles: int = 0) -> bool:
    """Can edtr_gn_apply fold the producing igemm's partials itself (no edtr_gn_finalize launch)?  ``tiles``: slots per image of the
    partials (0 = HW / 128: the main-loop epilogues' 128-row slots)."""
    if tiles <= 0:
        if HW % 128:
            return False
        tiles = HW // 128
    return tiles <= GN_FOLD_MAX_TILES and C // groups <= 64


def make_gn(*, dtype, x, ldx, B, HW, C, sums, gamma, beta, eps, silu, y, ldy, groups: int = 32, name="gn",
            sums_zeroed: bool = False, partial=None, tiles_per_image: int = 0):
    """Returns (stats_rec, apply_rec).  ``partial``: the producing igemm's gn_partial tensor — the apply launch folds it
    itself (gn_foldable) and ``sums`` may be None."""
    p = L.GnParams()
    p.dtype, p.B, p.HW, p.C, p.groups = dt_code(dtype), B, HW, C, groups
    p.x, p.ldx, p.sums = ptr(x), ldx, ptr(sums)
    p.gamma, p.beta, p.eps, p.silu = ptr(gamma), ptr(beta), eps, int(silu)
    p.y, p.ldy = ptr(y), ldy
    p.sums_zeroed = int(sums_zeroed)
    if partial is not None:
        p.partial, p.tiles_per_image = ptr(partial), tiles_per_image or HW // 128
    keep = (p, x, sums, gamma, beta, y, partial)
    lib = L.load()
    nb = 2.0 * B * HW * C
    return (Rec(lib.edtr_gn_stats, (ct.byref(p),), keep, name + ".stats", 0.0, nb),
            Rec(lib.edtr_gn_apply, (ct.byref(p),), keep, name + ".apply", 0.0, 2 * nb))


def make_gn_finalize(*, partial, tiles_per_image, B, C, sums, groups: int = 32, name="gn.finalize") -> Rec:
    return Rec(L.load().edtr_gn_finalize, (ptr(partial), tiles_per_image, B, C, groups, ptr(sums)), (partial, sums), name)


def make_gn_table(*, partial, tiles_per_image, sums, B, C, HW, gamma, beta, eps, table, groups: int = 32, name="gn.table") -> Rec:
    """(scale, shift) per image and channel for a consumer that normalises the tensor itself (edtr_hip.h: edtr_gn_table, a_gn)."""
    return Rec(L.load().edtr_gn_table, (ptr(partial), tiles_per_image, ptr(sums), B, C, groups, HW, ptr(gamma), ptr(beta), eps, ptr(table)),
               (partial, sums, gamma, beta, table), name)


def gn_in_conv_ok(B: int, H: int, W: int, C: int, N: int, splitk: int = 1, ld: int = 0) -> bool:
    """Should this 3x3 / stride 1 / pad 1 convolution run with the GroupNorm of its input fused into a halo tile's patch staging
    (edtr_hip.h: a_gn)?  Measured policy first: the thresholds of edtr_igemm's automatic halo choice, 128-column tiles without padding
    and >= 48 units — and N <= EDTR_GN_IN_CONV_MAXN (default 128): measured on the MI355X (profiles/r04/gn_in_conv_ab.log),
    the fused form wins where ONE 128-column tile covers the output channels (the VAE's 512 x 512 level: headline +1.4 %) and loses
    beyond (N = 256: -0.5 % against that, N = 512 / 640 / 1280: the whole path -1 .. -2 %), because every column tile of a patch
    normalises the patch again.  EDTR_GN_IN_CONV=0 keeps the edtr_gn_apply launch everywhere (A/B runs).  Whether a tile takes the
    launch is the planner's word (conv3x3_plan): its geometry, split-K and addressability rules are stated in csrc/igemm_plan.h only."""
    if os.environ.get("EDTR_GN_IN_CONV", "1") == "0" or os.environ.get("EDTR_IGEMM_HALO", "1") == "0":
        return False
    if N % 128 or N > int(os.environ.get("EDTR_GN_IN_CONV_MAXN", "128")) or (B * H * W // 256) * (N // 128) * max(splitk, 1) < 48:
        return False         # (every 128-column tile of the convolution normalises the whole patch again: N / 128 times the arithmetic of edtr_gn_apply)
    return conv3x3_plan(B, H, W, C, N, ld=ld, splitk=splitk, a_gn=True) > 0


def gn_slot_rows(hw: int) -> int:
    """Rows per slot of the fused GroupNorm partials for images of ``hw`` pixels (0 = no fused statistics): 128-row slots wherever an
    image is whole slots; 64-row slots for the 8 x 8 images of the deepest latent level (the split-K reducer writes those)."""
    if hw > 0 and hw % 128 == 0:
        return 128
    return 64 if hw == 64 else 0


def gn_fusable(M: int, N: int, C1: int, hw: int, C2: int = 0, splitk: int = 1, invariant: bool = False) -> bool:
    """Can the producing edtr_igemm also emit GroupNorm partials?  Without split-K: whole 128-row tiles inside one image on the
    128x128 kernels.  With split-K (round 6) the REDUCER writes them: any slot size gn_slot_rows() knows, N % 32 == 0.
    EDTR_GN_SPLITK_STATS=0 keeps the edtr_gn_stats launch behind split-K producers (A/B runs)."""
    if C2 or N % 32:
        return False
    if splitk > 1:
        sr = gn_slot_rows(hw)
        return os.environ.get("EDTR_GN_SPLITK_STATS", "1") != "0" and sr > 0 and M % sr == 0
    if hw % 128 or M % 128:
        return False
    dma_ok = C1 % 64 == 0
    big = ((M + 127) // 128) * ((N + 127) // 128)
    return dma_ok or invariant or big >= 200      # (register-staged shapes: the 128x128 tile 1, which the invariant mode always takes)


def gn_tiles(hw: int, splitk: int = 1) -> int:
    """Slots per image of a fused-partials buffer written by a producer with this split-K count."""
    return hw // (gn_slot_rows(hw) if splitk > 1 else 128)


def make_layernorm(*, dtype, x, rows, C, ldx, gamma, beta, eps, y, ldy, c_valid: int = 0, name="layernorm") -> Rec:
    """c_valid (0 = C): statistics over the first c_valid columns only; the remaining columns of y are written as zeros."""
    args = (dt_code(dtype), ptr(x), rows, C, c_valid, ldx, ptr(gamma), ptr(beta), eps, ptr(y), ldy)
    return Rec(L.load().edtr_layernorm, args, (x, gamma, beta, y), name, 0.0, 4.0 * rows * C)


def make_softmax_rows(*, dtype, s, rows, cols, ld_s, p, ld_p, cols_pad=0, name="softmax_rows") -> Rec:
    args = (dt_code(dtype), ptr(s), rows, cols, ld_s, ptr(p), ld_p, cols_pad)
    return Rec(L.load().edtr_softmax_rows, args, (s, p), name, 0.0, 10.0 * rows * cols)


# --------------------------------------------------------------------------------------------
# layout / elementwise
# --------------------------------------------------------------------------------------------
def make_nchw_to_nhwc(*, dtype, src, B, C, HW, dst, ld, coff=0, zero_pad_to=0, scale=1.0, shift=0.0,
                      name="nchw_to_nhwc") -> Rec:
    args = (dt_code(dtype), ptr(src), B, C, HW, ptr(dst), ld, coff, zero_pad_to, scale, shift)
    return Rec(L.load().edtr_nchw_to_nhwc, args, (src, dst), name, 0.0, 6.0 * B * C * HW)


def make_pixel_unshuffle(*, dtype, src, B, C, H, W, r, dst, ld, sub=None, scale=1.0, zero_pad_to=0,
                         name="pixel_unshuffle") -> Rec:
    args = (dt_code(dtype), ptr(src), B, C, H, W, r, ptr(sub), scale, ptr(dst), ld, zero_pad_to)
    return Rec(L.load().edtr_pixel_unshuffle, args, (src, sub, dst), name, 0.0, 6.0 * B * C * H * W)


def make_nhwc_to_nchw(*, dtype, src, src_f32, B, C, HW, ld, dst, scale=1.0, name="nhwc_to_nchw") -> Rec:
    args = (dt_code(dtype), ptr(src), int(src_f32), B, C, HW, ld, ptr(dst), scale)
    return Rec(L.load().edtr_nhwc_to_nchw, args, (src, dst), name, 0.0, 6.0 * B * C * HW)


def make_add(*, dtype, a, lda, b, ldb, out, ldo, rows, C, name="add") -> Rec:
    args = (dt_code(dtype), ptr(a), lda, ptr(b), ldb, ptr(out), ldo, rows, C)
    return Rec(L.load().edtr_add, args, (a, b, out), name, 0.0, (6.0 if b is not None else 4.0) * rows * C)


def make_add_stats(*, dtype, a, lda, b, ldb, out, ldo, rows, C, gn_partial, gn_ld, slot_rows, name="add") -> Rec:
    """a (+ b) -> out and the result's per-slot column statistics in edtr_igemm's gn_partial format (edtr_hip.h: edtr_add_stats);
    ``gn_partial`` is a 1-D view that starts at this tensor's first column inside slot 0."""
    args = (dt_code(dtype), ptr(a), lda, ptr(b), ldb, ptr(out), ldo, rows, C, ptr(gn_partial), gn_ld, slot_rows)
    return Rec(L.load().edtr_add_stats, args, (a, b, out, gn_partial), name, 0.0, (6.0 if b is not None else 4.0) * rows * C)


def make_add_mirror(*, a, lda, b, ldb, out, ldo, out16, rows, C, name="add") -> Rec:
    """fp32 a (+ b) -> fp32 out and its fp16 mirror (edtr_hip.h: edtr_add_mirror)."""
    args = (ptr(a), lda, ptr(b), ldb, ptr(out), ldo, ptr(out16), out16.stride(0), rows, C)
    return Rec(L.load().edtr_add_mirror, args, (a, b, out, out16), name, 0.0, (14.0 if b is not None else 10.0) * rows * C)


def make_timestep_embedding(*, dtype, t, B, dim, out, ld, name="timestep_embedding") -> Rec:
    return Rec(L.load().edtr_timestep_embedding, (dt_code(dtype), ptr(t), B, dim, ptr(out), ld), (t, out), name)


def make_sampler_update(*, x, eps, noise, coefs: Sequence[float], x_prev, pred_x0, n, name="sampler_update") -> Rec:
    a, b, c1, c2, sigma = (float(v) for v in coefs)
    args = (ptr(x), ptr(eps), ptr(noise), a, b, c1, c2, sigma, ptr(x_prev), ptr(pred_x0), n)
    return Rec(L.load().edtr_sampler_update, args, (x, eps, noise, x_prev, pred_x0), name, 0.0, 20.0 * n)


def make_axpby(*, x, y, a, b, out, n, name="axpby") -> Rec:
    return Rec(L.load().edtr_axpby, (ptr(x), ptr(y), float(a), float(b), ptr(out), n), (x, y, out), name, 0.0, 12.0 * n)


def make_q_sample(*, x, noise, t, tab_a, tab_b, out, name="q_sample") -> Rec:
    B = x.shape[0]
    per = x.numel() // B
    args = (ptr(x), ptr(noise), ptr(t), ptr(tab_a), ptr(tab_b), tab_a.numel(), ptr(out), B, per)
    return Rec(L.load().edtr_q_sample, args, (x, noise, t, tab_a, tab_b, out), name, 0.0, 12.0 * x.numel())


def make_split3(*, src: torch.Tensor, rows: int, C: int, dst: torch.Tensor, pattern: int = 0, name="split3") -> Rec:
    code = L.F32_SPLIT if src.dtype == torch.float32 else dt_code(src.dtype)
    args = (code, ptr(src), rows, C, src.stride(0), pattern, ptr(dst), dst.stride(0))
    return Rec(L.load().edtr_split3, args, (src, dst), name, 0.0, (src.element_size() + 6.0) * rows * C)


def make_split_operand(*, src: torch.Tensor, rows: int, C: int, dst: torch.Tensor, fmt, name="split_operand") -> Rec:
    """[rows, C] fp32 / 16-bit -> GEMM operand in format ``fmt`` (F32S: bf16 [hi|lo|hi]; F32H[p]: fp16, p parts)."""
    code = L.F32_SPLIT if src.dtype == torch.float32 else dt_code(src.dtype)
    parts = 3 if fmt == F32S else {v: k for k, v in F32H.items()}[fmt]
    args = (code, ptr(src), rows, C, src.stride(0), dt_code(fmt), ptr(dst), dst.stride(0))
    return Rec(L.load().edtr_split_operand, args, (src, dst), name, 0.0, (src.element_size() + 2.0 * parts) * rows * C)


def make_sampler_update_indexed(*, x, eps, noise, index, coefs, x_prev, pred_x0, name="sampler_update") -> Rec:
    B = x.shape[0]
    per = x.numel() // B
    args = (ptr(x), ptr(eps), ptr(noise), ptr(index), ptr(coefs), coefs.shape[0], ptr(x_prev), ptr(pred_x0), B, per)
    return Rec(L.load().edtr_sampler_update_indexed, args, (x, eps, noise, index, coefs, x_prev, pred_x0), name, 0.0, 20.0 * x.numel())


def make_gaussian_sample(*, moments, ld, noise, out, B, C, HW, scale, name="gaussian_sample") -> Rec:
    args = (ptr(moments), ld, ptr(noise), ptr(out), B, C, HW, float(scale))
    return Rec(L.load().edtr_gaussian_sample, args, (moments, noise, out), name, 0.0, 16.0 * B * C * HW)


# -- seeded noise (edtr_hip.h "Reproducible noise"): the records of the tensor-noise launches above with the noise operand replaced by
#    a `rng.NoiseSource` (seed by value, the batch's global image ids read from its device copy) --------------------------------------
def _noise_args(source, B: int, device, what: str):
    """(seed, image_ids pointer, image_id_base, keepalive) of a NoiseSource checked against the batch size"""
    ids = source.check_batch(B, what).ids_on(device)
    return source.seed, ptr(ids), 0, ids


def make_normal_fill(*, out, source, purpose: int, draw: int = 0, name="normal_fill") -> Rec:
    """out [B, ...] fp32 = the stream of ``source``'s images for (purpose, draw)."""
    B = out.shape[0]
    per = out.numel() // B
    seed, ids_p, base, ids = _noise_args(source, B, out.device, name)
    args = (ptr(out), B, per, seed, ids_p, base, int(purpose), int(draw))
    return Rec(L.load().edtr_normal_fill, args, (out, ids), name, 0.0, 4.0 * out.numel())


def make_q_sample_rng(*, x, source, t, tab_a, tab_b, out, name="q_sample_rng") -> Rec:
    B = x.shape[0]
    per = x.numel() // B
    seed, ids_p, base, ids = _noise_args(source, B, x.device, name)
    args = (ptr(x), ptr(t), ptr(tab_a), ptr(tab_b), tab_a.numel(), ptr(out), B, per, seed, ids_p, base)
    return Rec(L.load().edtr_q_sample_rng, args, (x, t, tab_a, tab_b, out, ids), name, 0.0, 8.0 * x.numel())


def make_sampler_update_rng(*, x, eps, source, draw: int, coefs: Sequence[float], x_prev, pred_x0, name="sampler_update_rng") -> Rec:
    a, b, c1, c2, sigma = (float(v) for v in coefs)
    B = x.shape[0]
    per = x.numel() // B
    seed, ids_p, base, ids = _noise_args(source, B, x.device, name)
    args = (ptr(x), ptr(eps), a, b, c1, c2, sigma, ptr(x_prev), ptr(pred_x0), B, per, seed, ids_p, base, int(draw))
    return Rec(L.load().edtr_sampler_update_rng, args, (x, eps, x_prev, pred_x0, ids), name, 0.0, 16.0 * x.numel())


def make_sampler_update_indexed_rng(*, x, eps, source, index, coefs, x_prev, pred_x0, name="sampler_update_rng") -> Rec:
    B = x.shape[0]
    per = x.numel() // B
    seed, ids_p, base, ids = _noise_args(source, B, x.device, name)
    args = (ptr(x), ptr(eps), ptr(index), ptr(coefs), coefs.shape[0], ptr(x_prev), ptr(pred_x0), B, per, seed, ids_p, base)
    return Rec(L.load().edtr_sampler_update_indexed_rng, args, (x, eps, index, coefs, x_prev, pred_x0, ids), name, 0.0, 16.0 * x.numel())


def make_gaussian_sample_rng(*, moments, ld, source, out, B, C, HW, scale, name="gaussian_sample_rng") -> Rec:
    seed, ids_p, base, ids = _noise_args(source, B, out.device, name)
    args = (ptr(moments), ld, ptr(out), B, C, HW, float(scale), seed, ids_p, base)
    return Rec(L.load().edtr_gaussian_sample_rng, args, (moments, out, ids), name, 0.0, 12.0 * B * C * HW)


# -- the 8-bit image boundary (edtr_hip.h "Images in, images out"; the callers and the host restatements are edtr_amd/imageio.py) -----
def make_image_resize_u8(*, src, dst, h_tab=None, v_tab=None, tmp=None, name="image.resize_u8") -> Rec:
    """uint8 [in_h, in_w, 3] -> uint8 [out_h, out_w, 3]; ``h_tab`` / ``v_tab`` = (bounds int32 [out, 2], coefs int32 [out, k]) device
    tensors of the pass (None for an axis that keeps its size); ``tmp`` uint8 [in_h, out_w, 3] when both passes run."""
    (in_h, in_w, ch), (out_h, out_w, _) = src.shape, dst.shape
    hb, hc = h_tab if h_tab is not None else (None, None)
    vb, vc = v_tab if v_tab is not None else (None, None)
    args = (ptr(src), in_h, in_w, ch, ptr(dst), out_h, out_w, ptr(hb), ptr(hc), hc.shape[1] if hc is not None else 0,
            ptr(vb), ptr(vc), vc.shape[1] if vc is not None else 0, ptr(tmp))
    return Rec(L.load().edtr_image_resize_u8, args, (src, dst, hb, hc, vb, vc, tmp), name, 0.0, 3.0 * (in_h * in_w + 2 * in_h * out_w + out_h * out_w))


def make_image_ingest(*, src, batch, b: int, replicate: bool, table, name="image.ingest") -> Rec:
    """``src`` uint8 or fp32 [h, w, 3] -> slot ``b`` of fp32 ``batch`` [B, 3, H, W], zero- or replicate-padded."""
    h, w, ch = src.shape
    B, _, H, W = batch.shape
    args = (int(src.dtype == torch.float32), ptr(src), h, w, ch, ptr(batch), b, B, H, W, int(replicate), ptr(table))
    return Rec(L.load().edtr_image_ingest, args, (src, batch, table), name, 0.0, float(src.element_size() * 3 * h * w + 12 * H * W))


def make_image_emit(*, batch, b: int, dst, name="image.emit") -> Rec:
    """the top-left [h, w] crop of image ``b`` of fp32 ``batch`` [B, 3, H, W] -> uint8 ``dst`` [h, w, 3]."""
    B, ch, H, W = batch.shape
    h, w, _ = dst.shape
    return Rec(L.load().edtr_image_emit, (ptr(batch), b, B, ch, H, W, ptr(dst), h, w), (batch, dst), name, 0.0, 15.0 * h * w)


def make_image_resize_h_batch(*, descs_host, descs, tmp, keep=(), name="image.resize_h_batch") -> Rec:
    """the horizontal pass of every image of a ragged batch in one launch: ``descs_host`` a ctypes array of `lib.ImageDesc`, ``descs`` its
    copy on the device (a uint8 tensor), ``tmp`` the shared uint8 scratch buffer; ``keep``: the tensors the descriptors point at."""
    B = len(descs_host)
    args = (descs_host, ptr(descs), B, 3, ptr(tmp), 0 if tmp is None else tmp.numel())
    nbytes = sum(3.0 * d.in_h * (d.in_w + d.out_w) for d in descs_host if d.in_w != d.out_w)
    return Rec(L.load().edtr_image_resize_h_batch, args, (descs_host, descs, tmp) + tuple(keep), name, 0.0, nbytes)


def make_image_resize_ingest_batch(*, descs_host, descs, tmp, batch, replicate: bool, table, keep=(), name="image.resize_ingest_batch") -> Rec:
    """every image's vertical pass -> v / 255 -> its padded slot of fp32 ``batch`` [slots, 3, H, W], in one launch."""
    B = len(descs_host)
    slots, _, H, W = batch.shape
    args = (descs_host, ptr(descs), B, 3, ptr(tmp), 0 if tmp is None else tmp.numel(), ptr(batch), slots, H, W, int(replicate), ptr(table))
    nbytes = sum(3.0 * d.in_h * d.out_w for d in descs_host) + 12.0 * B * H * W
    return Rec(L.load().edtr_image_resize_ingest_batch, args, (descs_host, descs, tmp, batch, table) + tuple(keep), name, 0.0, nbytes)


def make_image_emit_batch(*, batch, table_host, table, dst, name="image.emit_batch") -> Rec:
    """crop i = the top-left [h, w] of image b of fp32 ``batch`` -> uint8 HWC at byte ``offset`` of ``dst``, (b, h, w, offset) = row i of the
    int64 [n, 4] table (``table_host``: a ctypes int64 array, ``table``: its device copy), in one launch."""
    B, ch, H, W = batch.shape
    n = len(table_host) // 4
    args = (ptr(batch), B, ch, H, W, table_host, ptr(table), n, ptr(dst), dst.numel())
    nbytes = sum(15.0 * table_host[4 * i + 1] * table_host[4 * i + 2] for i in range(n))
    return Rec(L.load().edtr_image_emit_batch, args, (batch, table_host, table, dst), name, 0.0, nbytes)


def make_image_sqdiff(*, a, b, sizes, crop_border: int, y_channel: bool, partials, out, name="image.sqdiff") -> Rec:
    """fp64 ``out`` [B] = per-image sums of squared differences of fp32 [B, 3, H, W] batches (``sizes``: int32 [B, 2] device or None)."""
    B, ch, H, W = a.shape
    args = (ptr(a), ptr(b), B, ch, H, W, ptr(sizes), int(crop_border), int(y_channel), ptr(partials), ptr(out))
    return Rec(L.load().edtr_image_sqdiff, args, (a, b, sizes, partials, out), name, 0.0, 24.0 * B * H * W)


# -- the degradation stage (edtr_hip.h "Low-quality inputs"; the callers and the host restatements are edtr_amd/degrade.py) -----------
def make_degrade_filter2d(*, x, kernels, out, name="degrade.filter2d") -> Rec:
    """fp32 ``x`` [B, 3, H, W] blurred with fp32 ``kernels`` [B or 1, k, k] (correlation, reflect borders) -> ``out``."""
    B, ch, H, W = x.shape
    n, k, _ = kernels.shape
    args = (ptr(x), ptr(out), B, ch, H, W, ptr(kernels), n, k)
    return Rec(L.load().edtr_degrade_filter2d, args, (x, kernels, out), name, 2.0 * x.numel() * k * k, 8.0 * x.numel())


def make_degrade_resize(*, x, out, mode: int, name="degrade.resize") -> Rec:
    """fp32 ``x`` [B, 3, ih, iw] -> ``out`` [B, 3, oh, ow] as F.interpolate(size=, mode=lib.RESIZE_*)."""
    B, ch, ih, iw = x.shape
    args = (ptr(x), ptr(out), B, ch, ih, iw, out.shape[2], out.shape[3], int(mode))
    return Rec(L.load().edtr_degrade_resize, args, (x, out), name, 0.0, 4.0 * (x.numel() + out.numel()))


def _host_and_device(values, B: int, ctype, device):
    """one value per image as the ctypes array an entry point checks and as its copy on ``device`` (the values as the C type holds them)"""
    host = (ctype * B)(*values)
    return host, torch.tensor(list(host), dtype=torch.float32 if ctype is ct.c_float else torch.int32).to(device)


def make_degrade_gaussian_noise(*, x, out, noise_out, sigma, gray, source, draw: int, rounds: bool, name="degrade.gaussian_noise") -> Rec:
    """``out`` = clamp(``x`` + n * sigma[b] / 255) with n from ``source``'s stream; ``sigma`` / ``gray``: one Python value per image
    (uploaded here, and handed to the entry point as host arrays as well); ``noise_out``: None or a tensor that receives n."""
    B, ch, H, W = x.shape
    (sig_host, sig), (gray_host, gry) = _host_and_device(sigma, B, ct.c_float, x.device), _host_and_device(gray, B, ct.c_int32, x.device)
    seed, ids_p, base, ids = _noise_args(source, B, x.device, name)
    args = (ptr(x), ptr(out), ptr(noise_out), B, ch, H, W, sig_host, ptr(sig), gray_host, ptr(gry), seed, ids_p, base, int(draw), int(rounds))
    return Rec(L.load().edtr_degrade_gaussian_noise, args, (x, out, noise_out, sig_host, sig, gray_host, gry, ids), name, 0.0, 8.0 * x.numel())


def make_degrade_jpeg(*, x, out, quality, factor, dct, coefs=None, name="degrade.jpeg") -> Rec:
    """DiffJPEG of ``x`` -> ``out``; ``quality``: one Python float per image (checked by the entry point), ``factor``: fp32 [B] device
    tensor of their quality_to_factor, ``dct``: the fp32 [64, 64] table on the device, ``coefs``: None or fp32 [B, 6 mcus, 64]."""
    B, ch, H, W = x.shape
    q_host = (ct.c_float * B)(*quality)
    args = (ptr(x), ptr(out), B, ch, H, W, q_host, ptr(factor), ptr(dct), ptr(coefs))
    mcus = ((H + 15) // 16) * ((W + 15) // 16)
    return Rec(L.load().edtr_degrade_jpeg, args, (x, out, q_host, factor, dct, coefs), name, 4.0 * B * mcus * 6 * 4096, 8.0 * x.numel())


def make_degrade_poisson_noise(*, x, out, noise_out, scale, gray, tables, lows, levels, counts_out, source, draw: int, rounds: bool,
                               name="degrade.poisson_noise") -> Rec:
    """``out`` = clamp(``x`` + noise * scale[b]) with the Poisson noise of edtr_hip.h drawn from ``source``'s stream; ``scale`` / ``gray``:
    one Python value per image; ``tables`` uint32 [9, 256, 256] / ``lows`` int32 [9, 256]: `degrade.poisson_tables_on(device)`;
    ``levels``: int32 [B, 16] workspace; ``counts_out``: None or int32 [B, 2]; ``noise_out``: None or a tensor that receives the noise."""
    B, ch, H, W = x.shape
    (sc_host, sc), (gray_host, gry) = _host_and_device(scale, B, ct.c_float, x.device), _host_and_device(gray, B, ct.c_int32, x.device)
    seed, ids_p, base, ids = _noise_args(source, B, x.device, name)
    args = (ptr(x), ptr(out), ptr(noise_out), B, ch, H, W, sc_host, ptr(sc), gray_host, ptr(gry), ptr(tables), ptr(lows), ptr(levels),
            ptr(counts_out), seed, ids_p, base, int(draw), int(rounds))
    keep = (x, out, noise_out, sc_host, sc, gray_host, gry, tables, lows, levels, counts_out, ids)
    return Rec(L.load().edtr_degrade_poisson_noise, args, keep, name, 0.0, 24.0 * x.numel())


def make_degrade_sepblur(*, x, taps, out, mask_out=None, threshold: float = 0.0, name="degrade.sepblur") -> Rec:
    """fp32 ``x`` [B, 3, H, W] blurred with the fp32 tap vector ``taps`` [k] along rows, then columns (reflect borders) -> ``out``;
    ``mask_out``: None or a tensor that receives |x - out| * 255 > ``threshold`` as 0 / 1."""
    B, ch, H, W = x.shape
    k = taps.numel()
    args = (ptr(x), ptr(out), ptr(mask_out), B, ch, H, W, ptr(taps), k, float(threshold))
    return Rec(L.load().edtr_degrade_sepblur, args, (x, taps, out, mask_out), name, 4.0 * x.numel() * k, 8.0 * x.numel())


def make_degrade_usm_apply(*, x, blur, soft, out, weight: float, name="degrade.usm_apply") -> Rec:
    """``out`` = soft * clamp(x + weight (x - blur), 0, 1) + (1 - soft) * x, all fp32 [B, 3, H, W]."""
    B, ch, H, W = x.shape
    args = (ptr(x), ptr(blur), ptr(soft), ptr(out), B, ch, H, W, float(weight))
    return Rec(L.load().edtr_degrade_usm_apply, args, (x, blur, soft, out), name, 0.0, 16.0 * x.numel())


# -- label maps (edtr_hip.h "Label maps"; the callers and the host restatements are edtr_amd/labels.py) -------------------------------
_LOGITS_DT = {torch.float32: L.LOGITS_F32, torch.float16: L.LOGITS_F16, torch.bfloat16: L.LOGITS_BF16}


def _seg_sizes(sizes, device):
    """``sizes`` (None or one (h, w) per image) as the pair the confusion entry points take: a ctypes int32 host array and its device
    copy, uploaded from pinned memory without waiting"""
    if sizes is None:
        return None, None
    flat = [int(v) for hw in sizes for v in hw]
    return (ct.c_int32 * len(flat))(*flat), torch.tensor(flat, dtype=torch.int32).pin_memory().to(device, non_blocking=True)


def make_seg_confusion(*, logits, target, mat, sizes=None, pred=None, max_blocks: int = 0, name="labels.confusion") -> Rec:
    """int64 ``mat`` [n, n] += the confusion matrix of argmax(``logits`` [B, n, H, W], fp32 / fp16 / bf16) against uint8 ``target``
    [B, H, W]; ``sizes``: None or one (h, w) per image (uploaded here from pinned memory without waiting, and handed to the entry point as a host
    array as well);
    ``pred``: None or a uint8 [B, H, W] tensor that receives the argmax."""
    B, n, H, W = logits.shape
    if logits.dtype not in _LOGITS_DT:
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {logits.dtype}")
    sizes_host, dsizes = _seg_sizes(sizes, logits.device)
    args = (_LOGITS_DT[logits.dtype], ptr(logits), ptr(target), B, n, H, W, sizes_host, ptr(dsizes), ptr(mat), ptr(pred), int(max_blocks))
    nbytes = float(logits.element_size() * logits.numel() + target.numel() * (2 if pred is not None else 1))
    return Rec(L.load().edtr_seg_confusion, args, (logits, target, sizes_host, dsizes, mat, pred), name, 0.0, nbytes)


def make_seg_confusion_coarse(*, coarse, target, mat, sizes=None, pred=None, max_blocks: int = 0, name="labels.coarse_confusion") -> Rec:
    """`make_seg_confusion` on ``coarse`` [B, n, ih, iw] logits (fp32 / fp16 / bf16) that stand for their bilinear upsample to the
    extent of uint8 ``target`` [B, H, W]; ``sizes``, ``pred`` and ``max_blocks`` as there."""
    B, n, ih, iw = coarse.shape
    _, H, W = target.shape
    if coarse.dtype not in _LOGITS_DT:
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {coarse.dtype}")
    sizes_host, dsizes = _seg_sizes(sizes, coarse.device)
    args = (_LOGITS_DT[coarse.dtype], ptr(coarse), B, n, ih, iw, ptr(target), H, W, sizes_host, ptr(dsizes), ptr(mat), ptr(pred), int(max_blocks))
    nbytes = float(coarse.element_size() * coarse.numel() + target.numel() * (2 if pred is not None else 1))
    return Rec(L.load().edtr_seg_confusion_coarse, args, (coarse, target, sizes_host, dsizes, mat, pred), name, 0.0, nbytes)


def seg_ce_workspace(B: int, H: int, W: int) -> int:
    """bytes of the workspace `make_seg_ce_forward` takes (edtr_hip.h `edtr_seg_ce_workspace`: 16 per 16 x 64 output tile)"""
    return int(L.load().edtr_seg_ce_workspace(int(B), int(H), int(W)))


def make_seg_ce_forward(*, coarse, target, lse, workspace, loss, counts, ignore_index: int = 255, max_blocks: int = 0,
                        name="labels.coarse_cross_entropy") -> Rec:
    """`F.cross_entropy` of the bilinear upsample of ``coarse`` [B, n, ih, iw] (fp32 / fp16 / bf16) to the extent of uint8 ``target``
    [B, H, W], which is never stored: fp32 ``lse`` [B, H, W], fp32 ``loss`` [1] and int64 ``counts`` [2] (count, bad) are written;
    ``workspace``: a uint8 device tensor of `seg_ce_workspace` bytes.  The launch pair of edtr_hip.h `edtr_seg_ce_forward`."""
    B, n, ih, iw = coarse.shape
    _, H, W = target.shape
    if coarse.dtype not in _LOGITS_DT:
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {coarse.dtype}")
    args = (_LOGITS_DT[coarse.dtype], ptr(coarse), B, n, ih, iw, ptr(target), H, W, int(ignore_index), ptr(lse), ptr(workspace),
            workspace.numel() if workspace is not None else 0, ptr(loss), ptr(counts), int(max_blocks))
    nbytes = float(coarse.element_size() * coarse.numel() + 5 * target.numel())
    return Rec(L.load().edtr_seg_ce_forward, args, (coarse, target, lse, workspace, loss, counts), name, 0.0, nbytes)


def make_seg_ce_backward(*, coarse, target, lse, counts, grad_loss, grad, ignore_index: int = 255, max_blocks: int = 0,
                         name="labels.coarse_cross_entropy_backward") -> Rec:
    """``grad`` [B, n, ih, iw] (the type of ``coarse``) = the gradient of `make_seg_ce_forward`'s loss in ``coarse``, scaled by the fp32
    device scalar ``grad_loss``, from the ``lse`` and ``counts`` that launch wrote: a gather, every element written (edtr_hip.h
    `edtr_seg_ce_backward`)."""
    B, n, ih, iw = coarse.shape
    _, H, W = target.shape
    if coarse.dtype not in _LOGITS_DT:
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {coarse.dtype}")
    args = (_LOGITS_DT[coarse.dtype], ptr(coarse), B, n, ih, iw, ptr(target), H, W, int(ignore_index), ptr(lse), ptr(counts), ptr(grad_loss),
            ptr(grad), int(max_blocks))
    nbytes = float(2 * coarse.element_size() * coarse.numel() + 5 * target.numel())
    return Rec(L.load().edtr_seg_ce_backward, args, (coarse, target, lse, counts, grad_loss, grad), name, 0.0, nbytes)


def make_label_resize_nearest(*, src, dst, y_idx, x_idx, name="labels.resize_nearest") -> Rec:
    """uint8 ``src`` [in_h, in_w, C] -> ``dst`` [out_h, out_w, C] (C 1 or 3) through the int32 device tables ``y_idx`` [out_h] /
    ``x_idx`` [out_w] of `labels.nearest_index`."""
    (in_h, in_w, ch), (out_h, out_w, _) = src.shape, dst.shape
    args = (ptr(src), in_h, in_w, ch, ptr(dst), out_h, out_w, ptr(y_idx), ptr(x_idx))
    return Rec(L.load().edtr_label_resize_nearest, args, (src, dst, y_idx, x_idx), name, 0.0, 2.0 * dst.numel())


def make_label_window(*, src, dst, y0: int, x0: int, hflip: bool, vflip: bool, fill: int, name="labels.window") -> Rec:
    """uint8 ``src`` [h, w, C] -> ``dst`` [H, W, C]: the window at (y0, x0), flipped, ``fill`` outside the source."""
    (h, w, ch), (H, W, _) = src.shape, dst.shape
    args = (ptr(src), h, w, ch, ptr(dst), H, W, int(y0), int(x0), int(bool(hflip)), int(bool(vflip)), int(fill))
    return Rec(L.load().edtr_label_window, args, (src, dst), name, 0.0, 2.0 * dst.numel())


def make_label_colorize(*, labels, palette, dst, name="labels.colorize") -> Rec:
    """uint8 ``labels`` [B, H, W] -> ``dst`` [B, H, W, 3] through the uint8 [256, 3] device ``palette``."""
    B, H, W = labels.shape
    return Rec(L.load().edtr_label_colorize, (ptr(labels), B, H, W, ptr(palette), ptr(dst)), (labels, palette, dst), name, 0.0, 4.0 * labels.numel())


# -- detection boxes (edtr_hip.h "Detection boxes"; the callers and the host restatements are edtr_amd/boxes.py) ---------------------
def make_boxes_rank(*, scores, order, name="boxes.rank") -> Rec:
    """int32 ``order`` [n] = the stable descending argsort of fp32 ``scores`` [n] (NaN first), by counting"""
    return Rec(L.load().edtr_boxes_rank, (ptr(scores), scores.numel(), ptr(order)), (scores, order), name, 0.0, 8.0 * scores.numel())


def make_boxes_nms(*, boxes, scores, labels, iou_threshold: float, order, mask, keep, count, name="boxes.nms") -> Rec:
    """``keep`` int64 [max_out] / ``count`` int32 [1] = the per-label NMS of fp32 ``boxes`` [n, 4] / ``scores`` [n]; ``labels``: None,
    int32 [n] or int64 [n]; ``order`` int32 [n] and ``mask`` int64 [n * ceil(n / 64)]: workspaces."""
    n = boxes.shape[0]
    i64 = int(labels is not None and labels.dtype == torch.int64)
    args = (ptr(boxes), ptr(scores), ptr(labels), i64, n, float(iou_threshold), ptr(order), ptr(mask), ptr(keep), keep.numel(), ptr(count))
    return Rec(L.load().edtr_boxes_nms, args, (boxes, scores, labels, order, mask, keep, count), name, 0.0, 8.0 * mask.numel())


def make_boxes_candidates(*, logits, regression, proposals, image_hw, score_thresh, min_size, weights, xform_clip, cand_boxes, cand_scores,
                          flags, block_counts, out_boxes, out_scores, out_labels, count, name="boxes.candidates") -> Rec:
    """The candidate stage of the detector head's post-processing: fp32 ``logits`` [P, C], ``regression`` [P, 4 C], ``proposals`` [P, 4]
    -> the flagged candidates in ``out_boxes`` / ``out_scores`` / ``out_labels`` (int32) and their number in ``count`` (int32 [1])."""
    P, C = logits.shape
    w_host = (ct.c_float * 4)(*[float(w) for w in weights])
    args = (ptr(logits), ptr(regression), ptr(proposals), P, C, float(image_hw[0]), float(image_hw[1]), float(score_thresh), float(min_size),
            w_host, float(xform_clip), ptr(cand_boxes), ptr(cand_scores), ptr(flags), ptr(block_counts), ptr(out_boxes), ptr(out_scores),
            ptr(out_labels), ptr(count))
    keep = (logits, regression, proposals, w_host, cand_boxes, cand_scores, flags, block_counts, out_boxes, out_scores, out_labels, count)
    return Rec(L.load().edtr_boxes_candidates, args, keep, name, 0.0, 4.0 * (logits.numel() + regression.numel()) + 42.0 * P * (C - 1))


def make_boxes_filter_shift(*, boxes, scores, labels, score_min: float, dx: float, dy: float, out_boxes, out_scores, out_labels, offset,
                            name="boxes.filter_shift") -> Rec:
    """the boxes with score >= ``score_min``, shifted by (dx, dy), appended to the ``out_*`` tensors at the device counter ``offset``"""
    n = boxes.shape[0]
    args = (ptr(boxes), ptr(scores), ptr(labels), n, float(score_min), float(dx), float(dy), ptr(out_boxes), ptr(out_scores), ptr(out_labels),
            ptr(offset), out_scores.numel())
    return Rec(L.load().edtr_boxes_filter_shift, args, (boxes, scores, labels, out_boxes, out_scores, out_labels, offset), name, 0.0, 56.0 * n)


def make_boxes_transform(*, src, dst, flags: int, dx=0.0, dy=0.0, fx=1.0, fy=1.0, clip_w=0.0, clip_h=0.0, name="boxes.transform") -> Rec:
    """``dst`` = ``src`` (fp32 [n, 4]) shifted, multiplied or divided, clipped: each under its lib.BOX_* flag, in that order"""
    args = (ptr(src), ptr(dst), src.shape[0], int(flags), float(dx), float(dy), float(fx), float(fy), float(clip_w), float(clip_h))
    return Rec(L.load().edtr_boxes_transform, args, (src, dst), name, 0.0, 32.0 * src.shape[0])


def make_boxes_bilinear_scale(*, src, dst, rscale_h: float, rscale_w: float, name="boxes.bilinear_scale") -> Rec:
    """fp32 ``src`` [planes, ih, iw] -> ``dst`` [planes, oh, ow] as F.interpolate(scale_factor=, mode="bilinear"): source coordinates from
    ``rscale_*`` = fp32(1 / scale_factor)."""
    planes, ih, iw = src.shape
    args = (ptr(src), ptr(dst), planes, ih, iw, dst.shape[1], dst.shape[2], float(rscale_h), float(rscale_w))
    return Rec(L.load().edtr_boxes_bilinear_scale, args, (src, dst), name, 0.0, 4.0 * (src.numel() + dst.numel()))


# -- detection scores (edtr_hip.h "Detection scores"; the caller and the host restatement are edtr_amd/coco.py) -----------------------
def make_coco_match(*, det_boxes, det_scores, det_labels, count, gt_boxes, gt_labels, gt_area, gt_crowd, n_labels: int, image_id: int,
                    thresholds, areas, rec: dict, det_offset, capacity: int, gt_offset, gt_capacity: int, name="coco.match") -> Rec:
    """One image's detections (fp32 ``det_boxes`` [n, 4], ``det_scores`` [n], ``det_labels`` [n], of which the int32 [1] device ``count``
    exist, or all for None) matched against its ground truth (``gt_boxes`` [g, 4], ``gt_labels``, fp32 ``gt_area``, uint8 ``gt_crowd``) and
    appended to the record arrays ``rec`` (`coco.Records`; at least ``capacity`` / ``gt_capacity`` rows) at the device offsets, which are
    moved on.  Labels: both int64 or both int32."""
    n, g = det_scores.shape[0], gt_area.shape[0]
    if capacity > rec["match"].numel() or gt_capacity > rec["gt_ignore"].numel():
        raise ValueError("the record arrays are shorter than the capacities")
    if det_labels.dtype != gt_labels.dtype or det_labels.dtype not in (torch.int64, torch.int32):
        raise TypeError("labels must be int64 or int32, the same for detections and ground truth")
    args = (ptr(det_boxes), ptr(det_scores), ptr(det_labels), n, ptr(count), ptr(gt_boxes), ptr(gt_labels), ptr(gt_area), ptr(gt_crowd), g,
            int(det_labels.dtype == torch.int64), int(n_labels), int(image_id), ptr(thresholds), thresholds.numel(), ptr(areas),
            ptr(rec["image"]), ptr(rec["label"]), ptr(rec["score"]), ptr(rec["rank"]), ptr(rec["match"]), ptr(rec["ignore"]), ptr(det_offset),
            int(capacity), ptr(rec["gt_image"]), ptr(rec["gt_label"]), ptr(rec["gt_ignore"]), ptr(gt_offset), int(gt_capacity))
    keep = (det_boxes, det_scores, det_labels, count, gt_boxes, gt_labels, gt_area, gt_crowd, thresholds, areas, rec, det_offset, gt_offset)
    return Rec(L.load().edtr_coco_match, args, keep, name, 0.0, 28.0 * n + 26.0 * g)


def _coco_workspace(workspace, capacity: int, n_labels: int) -> int:
    need = int(L.load().edtr_coco_accumulate_workspace(int(capacity), int(n_labels)))
    if need <= 0 or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"the workspace holds {workspace.numel() * workspace.element_size()} bytes, {capacity} rows of {n_labels} labels take {need}")
    return workspace.numel() * workspace.element_size()


def make_coco_order(*, rec: dict, det_offset, capacity: int, n_labels: int, workspace, order, seg_start, n_kept, status, name="coco.order") -> Rec:
    """The rows of the record arrays ``rec`` below the device counter ``det_offset`` in the order of `coco.accumulate_order_reference`:
    row indices into int32 ``order`` [capacity], each label's segment into int32 ``seg_start`` [n_labels + 1], their number into
    ``n_kept`` and bit 0 of ``status`` for a counter past ``capacity`` (int32 [1] each).  ``workspace``: `edtr_coco_accumulate_workspace`
    bytes."""
    if capacity > rec["rank"].numel() or order.numel() < capacity or seg_start.numel() < n_labels + 1:
        raise ValueError("the record arrays or the outputs are shorter than the capacity")
    nbytes = _coco_workspace(workspace, capacity, n_labels)
    args = (ptr(rec["image"]), ptr(rec["label"]), ptr(rec["score"]), ptr(rec["rank"]), ptr(det_offset), int(capacity), int(n_labels),
            ptr(workspace), nbytes, ptr(order), ptr(seg_start), ptr(n_kept), ptr(status))
    return Rec(L.load().edtr_coco_order, args, (rec, det_offset, workspace, order, seg_start, n_kept, status), name, 0.0, 52.0 * capacity)


def make_coco_accumulate(*, order, seg_start, rec: dict, capacity: int, gt_offset, gt_capacity: int, n_labels: int, recall_thresholds, workspace,
                         precision, recall, status, name="coco.accumulate") -> Rec:
    """`coco.accumulate` from ``order`` / ``seg_start`` (`make_coco_order`) and the record arrays: fp64 ``precision`` [10, 101, n_labels, 4, 3]
    and ``recall`` [10, n_labels, 4, 3], every element written; bit 1 of ``status`` for a ground-truth counter past ``gt_capacity``."""
    if precision.numel() != 10 * 101 * n_labels * 12 or recall.numel() != 10 * n_labels * 12 or recall_thresholds.numel() != 101:
        raise ValueError("precision is [10, 101, n_labels, 4, 3], recall [10, n_labels, 4, 3] and the recall thresholds are 101")
    if capacity > rec["match"].numel() or gt_capacity > rec["gt_ignore"].numel() or order.numel() < capacity or seg_start.numel() < n_labels + 1:
        raise ValueError("the record arrays or the order are shorter than the capacities")
    nbytes = _coco_workspace(workspace, capacity, n_labels)
    args = (ptr(order), ptr(seg_start), ptr(rec["match"]), ptr(rec["ignore"]), ptr(rec["rank"]), int(capacity), ptr(rec["gt_label"]),
            ptr(rec["gt_ignore"]), ptr(gt_offset), int(gt_capacity), int(n_labels), ptr(recall_thresholds), ptr(workspace), nbytes,
            ptr(precision), ptr(recall), ptr(status))
    keep = (order, seg_start, rec, gt_offset, recall_thresholds, workspace, precision, recall, status)
    return Rec(L.load().edtr_coco_accumulate, args, keep, name, 0.0, 8.0 * (precision.numel() + recall.numel()) + 40.0 * 24.0 * capacity)


def make_coco_summarize(*, precision, recall, n_labels: int, status, out, name="coco.summarize") -> Rec:
    """the 12 statistics of `coco.summarize_ordered_reference` into fp64 ``out`` [13]; out[12] takes ``status`` as an int64"""
    if out.numel() != 13 or out.dtype != torch.float64 or precision.numel() != 10 * 101 * n_labels * 12 or recall.numel() != 10 * n_labels * 12:
        raise ValueError("out is fp64 [13], precision [10, 101, n_labels, 4, 3] and recall [10, n_labels, 4, 3]")
    args = (ptr(precision), ptr(recall), int(n_labels), ptr(status), ptr(out))
    return Rec(L.load().edtr_coco_summarize, args, (precision, recall, status, out), name, 0.0, 8.0 * (precision.numel() + recall.numel()))


# -- classification (edtr_hip.h "Classification"; the callers and the host restatements are edtr_amd/cls.py) ---------------------------
def make_cls_rank(*, logits, labels, keep: int, rec_label, rec_rank, rec_top, offset, capacity: int, name="cls.rank") -> Rec:
    """The order behind topk for ``logits`` [B, C] (fp32 / fp16 / bf16): the rank of int32 ``labels`` [B] (or None) into ``rec_rank``,
    the first ``keep`` classes into ``rec_top`` [capacity, keep], the labels into ``rec_label`` (or None), at the rows from the int32
    [1] device ``offset`` (None: 0) and below ``capacity``."""
    B, C = logits.shape
    if logits.dtype not in _LOGITS_DT:
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {logits.dtype}")
    if labels is not None and (labels.dtype != torch.int32 or labels.numel() != B):
        raise TypeError("labels must be int32, one per row")
    if (rec_rank is not None and capacity > rec_rank.numel()) or (keep > 0 and capacity * keep > rec_top.numel()):
        raise ValueError("the record arrays are shorter than the capacity")
    args = (_LOGITS_DT[logits.dtype], ptr(logits), ptr(labels), B, C, int(keep), ptr(rec_label), ptr(rec_rank), ptr(rec_top), ptr(offset),
            int(capacity))
    return Rec(L.load().edtr_cls_rank, args, (logits, labels, rec_label, rec_rank, rec_top, offset), name, 0.0,
               float(logits.element_size() * logits.numel() * (1 + int(keep))))


def make_cls_fdist(*, a, b, partials, name="cls.fdist") -> Rec:
    """fp64 ``partials`` [B, ceil(n / lib.CLS_FD_CHUNK)] = the chunk sums of |a - b| over the n elements of every image of ``a``, ``b``
    [B, ...] (fp32 / fp16 / bf16, the same for both)"""
    B = a.shape[0]
    n = a.numel() // B
    if a.dtype not in _LOGITS_DT or b.dtype != a.dtype or a.shape != b.shape:
        raise TypeError("the two feature tensors must have one shape and one of float32, float16 and bfloat16")
    if partials.dtype != torch.float64 or partials.numel() < B * ((n + L.CLS_FD_CHUNK - 1) // L.CLS_FD_CHUNK):
        raise ValueError("partials takes one fp64 word per image and chunk")
    args = (_LOGITS_DT[a.dtype], ptr(a), ptr(b), B, n, ptr(partials))
    return Rec(L.load().edtr_cls_fdist, args, (a, b, partials), name, 0.0, 2.0 * a.element_size() * a.numel())


def make_cls_commit(*, rec_rank, rec_fd, rec_batch, B: int, partials, n: int, topk: Sequence[int], batch_n, batch_correct, offsets,
                    capacity: int, batch_capacity: int, name="cls.commit") -> Rec:
    """Closes a batch of ``B`` images: counts rank < k for every k of ``topk`` into the batch row, finalises the feature distances from
    ``partials`` (None: NaN), and moves the int32 [2] device ``offsets`` (images, batches) on."""
    topk_host = (ct.c_int32 * max(len(topk), 1))(*[int(k) for k in topk])
    if capacity > rec_fd.numel() or capacity > rec_batch.numel() or batch_capacity > batch_n.numel():
        raise ValueError("the record arrays are shorter than the capacities")
    args = (ptr(rec_rank), ptr(rec_fd), ptr(rec_batch), int(B), ptr(partials), int(n), topk_host, len(topk), ptr(batch_n), ptr(batch_correct),
            ptr(offsets), int(capacity), int(batch_capacity))
    return Rec(L.load().edtr_cls_commit, args, (rec_rank, rec_fd, rec_batch, partials, topk_host, batch_n, batch_correct, offsets), name, 0.0, 16.0 * B)


def make_cls_normalize(*, x, out, mean: Sequence[float], std: Sequence[float], name="cls.normalize") -> Rec:
    """``out`` = (``x`` - mean_c) / std_c on fp32 [B, 3, H, W], each operation rounded; ``out`` may be ``x``"""
    B, ch, H, W = x.shape
    m_host, s_host = (ct.c_float * 3)(*[float(v) for v in mean]), (ct.c_float * 3)(*[float(v) for v in std])
    args = (ptr(x), ptr(out), B, ch, H, W, m_host, s_host)
    return Rec(L.load().edtr_cls_normalize, args, (x, out, m_host, s_host), name, 0.0, 8.0 * x.numel())


def make_cls_window(*, src, dst, out_hw, y0: int, x0: int, hflip: bool, vflip: bool, transpose: bool, fill: int, name="cls.window") -> Rec:
    """uint8 ``src`` [h, w, C] -> ``dst``: the ``out_hw`` = (H, W) crop at (y0, x0), flipped, ``fill`` outside the source; ``dst`` is
    [H, W, C], or [W, H, C] under ``transpose``."""
    (h, w, ch), (H, W) = src.shape, out_hw
    if tuple(dst.shape) != ((W, H, ch) if transpose else (H, W, ch)):
        raise ValueError(f"dst is {tuple(dst.shape)} for a {H} x {W} crop with transpose = {bool(transpose)}")
    args = (ptr(src), h, w, ch, ptr(dst), int(H), int(W), int(y0), int(x0), int(bool(hflip)), int(bool(vflip)), int(bool(transpose)), int(fill))
    return Rec(L.load().edtr_cls_window, args, (src, dst), name, 0.0, 2.0 * dst.numel())


# -- training losses (edtr_hip.h "Training losses"; the callers and the host restatements are edtr_amd/losses.py) ----------------------
def _l1_tables(pairs, weights):
    """the host arrays of the L1 entry points for ``pairs`` = [(a, b)] of device tensors and one host float per pair, checked"""
    pairs = [tuple(p) for p in pairs]
    if not 1 <= len(pairs) <= L.L1_MAX_PAIRS:
        raise ValueError(f"1 to {L.L1_MAX_PAIRS} pairs, got {len(pairs)}")
    if len(weights) != len(pairs):
        raise ValueError(f"{len(weights)} weights for {len(pairs)} pairs")
    for a, b in pairs:
        if a.dtype not in _LOGITS_DT or b.dtype != a.dtype:
            raise TypeError(f"both tensors of a pair must be float32, float16 or bfloat16 alike, got {a.dtype} and {b.dtype}")
        if a.shape != b.shape or a.numel() == 0:
            raise ValueError(f"the tensors of a pair have one non-empty shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        if a.numel() > L.L1_MAX_ELEMS:
            raise ValueError(f"at most {L.L1_MAX_ELEMS} elements a pair, got {a.numel()}")
        if not (a.is_contiguous() and b.is_contiguous()):
            raise ValueError("the tensors of a pair must be contiguous")
    k = len(pairs)
    return (pairs, (ct.c_int32 * k)(*[_LOGITS_DT[a.dtype] for a, _ in pairs]), _pointer_table([a for a, _ in pairs]),
            _pointer_table([b for _, b in pairs]), (ct.c_int64 * k)(*[a.numel() for a, _ in pairs]), (ct.c_float * k)(*[float(w) for w in weights]))


def l1_workspace(counts: Sequence[int]) -> int:
    """bytes of the workspace `make_l1_forward` takes for pairs of these element counts (edtr_hip.h `edtr_l1_workspace`: 8 per chunk)"""
    n_host = (ct.c_int64 * max(len(counts), 1))(*[int(n) for n in counts])
    return int(L.load().edtr_l1_workspace(n_host, len(counts)))


def make_l1_forward(*, pairs, weights, workspace, loss, terms=None, max_blocks: int = 0, name="losses.l1_mean") -> Rec:
    """fp32 ``loss`` [1] = sum_k weights[k] * mean |a_k - b_k| over ``pairs`` = [(a, b)] (contiguous device tensors, fp32 / fp16 / bf16 per
    pair) and, where given, fp32 ``terms`` [len(pairs)] = the unweighted means; ``workspace``: a uint8 device tensor of `l1_workspace`
    bytes.  The launch pair of edtr_hip.h `edtr_l1_forward`."""
    pairs, dt, pa, pb, n_host, w_host = _l1_tables(pairs, weights)
    if terms is not None and terms.numel() < len(pairs):
        raise ValueError("terms takes one fp32 word per pair")
    args = (dt, pa, pb, n_host, w_host, len(pairs), ptr(workspace), workspace.numel() if workspace is not None else 0, ptr(loss), ptr(terms),
            int(max_blocks))
    nbytes = float(sum(2 * a.element_size() * a.numel() for a, _ in pairs))
    return Rec(L.load().edtr_l1_forward, args, (dt, pa, pb, n_host, w_host, pairs, workspace, loss, terms), name, 0.0, nbytes)


def make_l1_backward(*, pairs, weights, grad_loss, grads_a, grads_b, max_blocks: int = 0, name="losses.l1_mean_backward") -> Rec:
    """``grads_a[k]`` / ``grads_b[k]`` (a tensor like the pair's, or None) = the gradient of `make_l1_forward`'s loss in a_k / b_k scaled
    by the fp32 device scalar ``grad_loss``: one launch for all pairs, every element written (edtr_hip.h `edtr_l1_backward`)."""
    pairs, dt, pa, pb, n_host, w_host = _l1_tables(pairs, weights)
    grads_a, grads_b = list(grads_a), list(grads_b)
    if len(grads_a) != len(pairs) or len(grads_b) != len(pairs):
        raise ValueError("one gradient slot (a tensor or None) per pair and side")
    for (a, _), ga, gb in zip(pairs, grads_a, grads_b):
        for g in (ga, gb):
            if g is not None and (g.dtype != a.dtype or g.shape != a.shape or not g.is_contiguous()):
                raise TypeError("a gradient is a contiguous tensor of its pair's shape and type")
    pga, pgb = _pointer_table(grads_a), _pointer_table(grads_b)
    args = (dt, pa, pb, n_host, w_host, len(pairs), ptr(grad_loss), pga, pgb, int(max_blocks))
    nbytes = float(sum(a.element_size() * a.numel() * (2 + (ga is not None) + (gb is not None))
                       for (a, _), ga, gb in zip(pairs, grads_a, grads_b) if ga is not None or gb is not None))
    return Rec(L.load().edtr_l1_backward, args, (dt, pa, pb, n_host, w_host, pga, pgb, pairs, grad_loss, grads_a, grads_b), name, 0.0, nbytes)


def make_cls_ce_forward(*, logits, labels, lse, workspace, loss, counts, ignore_index: int = -100, name="losses.cross_entropy") -> Rec:
    """`F.cross_entropy` of ``logits`` [B, C] (fp32 / fp16 / bf16) against int32 ``labels`` [B]: fp32 ``lse`` [B], fp32 ``loss`` [1] and
    int64 ``counts`` [2] (count, bad) are written; ``workspace``: a uint8 device tensor of 8 B bytes.  The launch pair of edtr_hip.h
    `edtr_cls_ce_forward`."""
    B, C = logits.shape
    if logits.dtype not in _LOGITS_DT:
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {logits.dtype}")
    args = (_LOGITS_DT[logits.dtype], ptr(logits), ptr(labels), B, C, int(ignore_index), ptr(lse), ptr(workspace),
            workspace.numel() if workspace is not None else 0, ptr(loss), ptr(counts))
    return Rec(L.load().edtr_cls_ce_forward, args, (logits, labels, lse, workspace, loss, counts), name, 0.0,
               float(2 * logits.element_size() * logits.numel()))


def make_cls_ce_backward(*, logits, labels, lse, counts, grad_loss, grad, ignore_index: int = -100, name="losses.cross_entropy_backward") -> Rec:
    """``grad`` [B, C] (the type of ``logits``) = the gradient of `make_cls_ce_forward`'s loss in ``logits`` scaled by the fp32 device
    scalar ``grad_loss``, from the ``lse`` and ``counts`` that launch wrote; every element written (edtr_hip.h `edtr_cls_ce_backward`)."""
    B, C = logits.shape
    if logits.dtype not in _LOGITS_DT:
        raise TypeError(f"logits must be float32, float16 or bfloat16, got {logits.dtype}")
    args = (_LOGITS_DT[logits.dtype], ptr(logits), ptr(labels), B, C, int(ignore_index), ptr(lse), ptr(counts), ptr(grad_loss), ptr(grad))
    return Rec(L.load().edtr_cls_ce_backward, args, (logits, labels, lse, counts, grad_loss, grad), name, 0.0,
               float(2 * logits.element_size() * logits.numel()))


# -- region proposals and RoI pooling (edtr_hip.h; the callers and the host restatements are edtr_amd/rois.py) -----------------------
def _level_table(levels):
    """int32 [L][5] on the host from [(H, W, A, stride_h, stride_w)]"""
    flat = [int(v) for row in levels for v in row]
    return (ct.c_int32 * max(len(flat), 1))(*flat)


def _pointer_table(tensors):
    return (ct.c_void_p * max(len(tensors), 1))(*[ptr(t) for t in tensors])


def _one_dtype(tensors, what: str) -> int:
    if not tensors or tensors[0].dtype not in _LOGITS_DT or any(t.dtype != tensors[0].dtype for t in tensors):
        raise TypeError(f"{what} must all be float32, all float16 or all bfloat16")
    return _LOGITS_DT[tensors[0].dtype]


def make_rpn_anchors(*, levels, cells, anchors, name="rois.anchors") -> Rec:
    """fp32 ``anchors`` [sum H W A, 4] from ``levels`` = [(H, W, A, stride_h, stride_w)] and the fp32 device ``cells`` [sum A, 4]"""
    table = _level_table(levels)
    return Rec(L.load().edtr_rpn_anchors, (table, len(levels), ptr(cells), ptr(anchors)), (table, cells, anchors), name, 0.0, 16.0 * anchors.shape[0])


def make_rpn_select(*, objectness, levels, pre_nms_top_n: int, selected, name="rois.select") -> Rec:
    """int32 ``selected`` [N, sum min(pre_nms_top_n, H W A)]: per image and level the logical indices of the greatest ``objectness``
    (a list of contiguous [N, A, H, W] tensors of one dtype), in topk order"""
    dt, table, ptrs = _one_dtype(objectness, "objectness"), _level_table(levels), _pointer_table(objectness)
    N = objectness[0].shape[0]
    args = (dt, ptrs, table, len(levels), N, int(pre_nms_top_n), ptr(selected))
    nbytes = 5.0 * sum(o.element_size() * o.numel() for o in objectness)
    return Rec(L.load().edtr_rpn_select, args, (ptrs, table, tuple(objectness), selected), name, 0.0, nbytes)


def make_rpn_candidates(*, objectness, deltas, levels, pre_nms_top_n: int, cells, selected, image_sizes, xform_clip: float, min_size: float,
                        score_thresh: float, boxes, probs, level, counts, name="rois.candidates") -> Rec:
    """The selected elements of ``objectness`` / ``deltas`` (lists of [N, A, H, W] / [N, 4 A, H, W]) decoded against their anchors,
    clipped to the fp32 device ``image_sizes`` [N, 2] and filtered, compacted per image into ``boxes`` [N, M, 4], ``probs`` and ``level``
    (int32) [N, M]; ``counts`` int32 [N]."""
    dt, table = _one_dtype(list(objectness) + list(deltas), "objectness and bbox_deltas"), _level_table(levels)
    po, pd = _pointer_table(objectness), _pointer_table(deltas)
    N = objectness[0].shape[0]
    args = (dt, po, pd, table, len(levels), N, int(pre_nms_top_n), ptr(cells), ptr(selected), ptr(image_sizes), float(xform_clip),
            float(min_size), float(score_thresh), ptr(boxes), ptr(probs), ptr(level), ptr(counts))
    keep = (po, pd, table, tuple(objectness), tuple(deltas), cells, selected, image_sizes, boxes, probs, level, counts)
    return Rec(L.load().edtr_rpn_candidates, args, keep, name, 0.0, 48.0 * selected.numel())


def make_roi_align(*, features, scales, rois, batch_index, out, sampling_ratio: int, k_min: int, k_max: int, canonical_scale: float,
                   canonical_level: float, name="rois.roi_align") -> Rec:
    """fp32 ``out`` [K, C, P, P] = MultiScaleRoIAlign of ``features`` (a list of contiguous [N, C, H, W] tensors of one dtype) at the fp32
    ``rois`` [K, 4] of the images ``batch_index`` (int32 [K]); ``scales``: one host float per level"""
    dt, ptrs = _one_dtype(features, "features"), _pointer_table(features)
    hw = [int(v) for f in features for v in f.shape[-2:]]
    hw_host, sc_host = (ct.c_int32 * len(hw))(*hw), (ct.c_float * len(features))(*[float(v) for v in scales])
    N, C = features[0].shape[:2]
    K, P = out.shape[0], out.shape[-1]
    args = (dt, ptrs, hw_host, sc_host, len(features), N, C, ptr(rois), ptr(batch_index), K, P, int(sampling_ratio), int(k_min), int(k_max),
            float(canonical_scale), float(canonical_level), ptr(out))
    keep = (ptrs, hw_host, sc_host, tuple(features), rois, batch_index, out)
    nbytes = 4.0 * out.numel() * (1 + 4 * int(sampling_ratio) ** 2)
    return Rec(L.load().edtr_roi_align, args, keep, name, 9.0 * out.numel() * int(sampling_ratio) ** 2, nbytes)


def roi_align_backward_workspace(N: int, K: int, P: int, S: int) -> int:
    """bytes of the workspace `make_roi_align_backward` takes (edtr_hip.h `edtr_roi_align_backward_workspace`)"""
    return int(L.load().edtr_roi_align_backward_workspace(int(N), int(K), int(P), int(S)))


def make_roi_align_backward(*, grad, grads_out, scales, rois, batch_index, workspace, sampling_ratio: int, k_min: int, k_max: int,
                            canonical_scale: float, canonical_level: float, name="rois.roi_align_backward") -> Rec:
    """``grads_out`` (a list of contiguous [N, C, H, W] tensors of one dtype, every word written) = the gradient of `make_roi_align`
    with respect to its features for the fp32 ``grad`` [K, C, P, P]: the launch pair of edtr_hip.h `edtr_roi_align_backward`.
    ``workspace``: a uint8 device tensor of `roi_align_backward_workspace` bytes; ``batch_index`` must not decrease."""
    dt, ptrs = _one_dtype(grads_out, "grads_out"), _pointer_table(grads_out)
    hw = [int(v) for f in grads_out for v in f.shape[-2:]]
    hw_host, sc_host = (ct.c_int32 * len(hw))(*hw), (ct.c_float * len(grads_out))(*[float(v) for v in scales])
    N, C = grads_out[0].shape[:2]
    K, P = grad.shape[0], grad.shape[-1]
    if grad.dtype != torch.float32 or tuple(grad.shape) != (K, C, P, P):
        raise TypeError(f"grad is fp32 [K, {C}, P, P], got {grad.dtype} {tuple(grad.shape)}")
    args = (dt, ptrs, hw_host, sc_host, len(grads_out), N, C, ptr(rois), ptr(batch_index), K, P, int(sampling_ratio), int(k_min), int(k_max),
            float(canonical_scale), float(canonical_level), ptr(grad), ptr(workspace), int(workspace.numel()))
    keep = (ptrs, hw_host, sc_host, tuple(grads_out), rois, batch_index, grad, workspace)
    nbytes = 4.0 * grad.numel() + sum(float(f.element_size() * f.numel()) for f in grads_out)
    return Rec(L.load().edtr_roi_align_backward, args, keep, name, 4.0 * grad.numel() * P * P, nbytes)


# -- the detector's input transform (edtr_hip.h "Detector input"; the caller and the host restatement are edtr_amd/detinput.py) ---------
def make_det_transform(*, descs_host, descs, mean: Sequence[float], std: Sequence[float], batch, keep=(), name="detinput.transform") -> Rec:
    """Every image of a ragged list normalised, resized and padded into its slot of ``batch`` [N, C, H, W] (fp32 / fp16 / bf16) in one
    launch: ``descs_host`` a ctypes array of `lib.DetImage`, ``descs`` its copy on the device (a uint8 tensor), ``mean`` / ``std`` C host
    floats each; ``keep``: the source tensors the descriptors point at."""
    if batch.dtype not in _LOGITS_DT:
        raise TypeError(f"batch must be float32, float16 or bfloat16, got {batch.dtype}")
    N, C, H, W = batch.shape
    if len(descs_host) != N or len(mean) != C or len(std) != C:
        raise ValueError(f"batch is {tuple(batch.shape)} for {len(descs_host)} images and {len(mean)} / {len(std)} constants")
    m_host, s_host = (ct.c_float * C)(*[float(v) for v in mean]), (ct.c_float * C)(*[float(v) for v in std])
    args = (descs_host, ptr(descs), N, C, m_host, s_host, _LOGITS_DT[batch.dtype], ptr(batch), H, W)
    nbytes = 4.0 * C * sum(d.h * d.w for d in descs_host) + float(batch.element_size() * batch.numel())
    return Rec(L.load().edtr_det_transform, args, (descs_host, descs, m_host, s_host, batch) + tuple(keep), name, 0.0, nbytes)


# -- detector training targets (edtr_hip.h "Detector training targets"; the callers and the host restatements are edtr_amd/targets.py) --
def _targets_table(table_host):
    """the ctypes int32 [N + 1][2] table of box and ground-truth starts from a list of rows"""
    flat = [int(v) for row in table_host for v in row]
    return (ct.c_int32 * len(flat))(*flat), len(flat) // 2 - 1


def targets_partial_words(table_host) -> int:
    """words of `make_targets_match`'s ``partial``: N x tiles of the longest image x the largest ground-truth count (at least 1)"""
    rows = [tuple(int(v) for v in r) for r in table_host]
    pmax = max([b[0] - a[0] for a, b in zip(rows, rows[1:])] + [1])
    gmax = max([b[1] - a[1] for a, b in zip(rows, rows[1:])] + [1])
    return (len(rows) - 1) * ((pmax + L.TARGETS_TILE - 1) // L.TARGETS_TILE) * gmax


def make_targets_match(*, boxes, shared: bool, gt_boxes, gt_labels, table_host, table, high: float, low: float, allow_low_quality: bool, form: int,
                       weights, best_val, best_idx, partial, matched, labels, regression=None, name="targets.match") -> Rec:
    """Matcher over box_iou per image of a ragged batch (two launches): int32 ``matched`` and ``labels`` (fp32 for `lib.TARGETS_RPN`,
    int64 for `lib.TARGETS_ROI`) [sum P]; with ``regression`` fp32 [sum P, 4] (RPN form) the encoding of every box against its
    ground truth under ``weights``.  ``table_host``: rows (box_start, gt_start), N + 1 of them; ``table`` its int32 copy on the device;
    ``best_val`` / ``best_idx`` [sum P] and ``partial`` (`targets_partial_words` uint32 words, an int32 tensor) are the scan's workspace."""
    tab, N = _targets_table(table_host)
    w_host = (ct.c_float * 4)(*[float(v) for v in weights])
    args = (ptr(boxes), int(bool(shared)), ptr(gt_boxes), ptr(gt_labels), tab, ptr(table), N, float(high), float(low), int(bool(allow_low_quality)),
            int(form), w_host, ptr(best_val), ptr(best_idx), ptr(partial), int(partial.numel()), ptr(matched), ptr(labels), ptr(regression))
    keep = (tab, w_host, boxes, gt_boxes, gt_labels, table, best_val, best_idx, partial, matched, labels, regression)
    G = max(int(gt_boxes.shape[0]) // max(N, 1), 1) if gt_boxes is not None else 1
    return Rec(L.load().edtr_targets_match, args, keep, name, 30.0 * matched.numel() * G, 64.0 * matched.numel())


def make_targets_encode(*, reference_boxes, proposals, weights, out, name="targets.encode") -> Rec:
    """fp32 ``out`` [K, 4] = encode_boxes(``reference_boxes``, ``proposals``, ``weights``), all fp32 [K, 4] on the device"""
    w_host = (ct.c_float * 4)(*[float(v) for v in weights])
    args = (ptr(reference_boxes), ptr(proposals), int(out.shape[0]), w_host, ptr(out))
    return Rec(L.load().edtr_targets_encode, args, (w_host, reference_boxes, proposals, out), name, 0.0, 48.0 * out.shape[0])


def make_targets_sample(*, labels, form: int, table_host, table, batch: int, max_pos: int, source, draw: int, purpose: int, mask_pos, mask_neg,
                        sampled, counts, keys=None, name="targets.sample") -> Rec:
    """The balanced sample of every image on ``source``'s stream: uint8 ``mask_pos`` / ``mask_neg`` [sum P], int32 ``sampled`` [N, batch]
    (ascending, then -1) and ``counts`` [N, 2] = num_pos, num_neg.  ``keys``: None, or int32 / uint32 words [sum P] on the device that take the
    stream's place (``source`` may then be None)"""
    tab, N = _targets_table(table_host)
    seed, ids_p, base, ids = (0, None, 0, None) if source is None and keys is not None else _noise_args(source, N, labels.device, name)
    args = (ptr(labels), int(form), tab, ptr(table), N, int(batch), int(max_pos), seed, ids_p, base, int(draw), int(purpose), ptr(keys), ptr(mask_pos),
            ptr(mask_neg), ptr(sampled), ptr(counts))
    keep = (tab, ids, labels, keys, table, mask_pos, mask_neg, sampled, counts)
    return Rec(L.load().edtr_targets_sample, args, keep, name, 0.0, 5.0 * labels.element_size() * labels.numel())


def make_targets_gather(*, boxes, gt_boxes, matched, labels, table_host, table, sampled, weights, out_boxes, out_labels, out_matched, out_targets,
                        name="targets.gather") -> Rec:
    """The sampled boxes of every image with their labels, clamped matches and regression targets: ``out_boxes`` / ``out_targets`` fp32
    [N, batch, 4], ``out_labels`` / ``out_matched`` int64 [N, batch]"""
    tab, N = _targets_table(table_host)
    w_host = (ct.c_float * 4)(*[float(v) for v in weights])
    args = (ptr(boxes), ptr(gt_boxes), ptr(matched), ptr(labels), tab, ptr(table), N, ptr(sampled), int(sampled.shape[1]), w_host, ptr(out_boxes),
            ptr(out_labels), ptr(out_matched), ptr(out_targets))
    keep = (tab, w_host, boxes, gt_boxes, matched, labels, table, sampled, out_boxes, out_labels, out_matched, out_targets)
    return Rec(L.load().edtr_targets_gather, args, keep, name, 0.0, 80.0 * sampled.numel())


def make_cast16(*, dtype, src: torch.Tensor, rows: int, C: int, dst: torch.Tensor, name="cast16") -> Rec:
    args = (dt_code(dtype), ptr(src), rows, C, src.stride(0), ptr(dst), dst.stride(0))
    return Rec(L.load().edtr_cast16, args, (src, dst), name, 0.0, 6.0 * rows * C)


def make_tile_accumulate(*, tile, wts, out, count, B, C, H, W, th, tw, hi, wi, name="tile_accumulate") -> Rec:
    args = (ptr(tile), ptr(wts), ptr(out), ptr(count), B, C, H, W, th, tw, hi, wi)
    return Rec(L.load().edtr_tile_accumulate, args, (tile, wts, out, count), name)


def make_divide(*, num, den, out, n, name="divide") -> Rec:
    return Rec(L.load().edtr_divide, (ptr(num), ptr(den), ptr(out), n), (num, den, out), name)


def make_tile_gather(*, src, table_host, table, th, tw, dst, name="tile_gather") -> Rec:
    """every th x tw window of fp32 ``src`` [B, C, H, W] -> ``dst`` [n B, C, th, tw], window-major, in one launch; ``table_host``: a ctypes
    int32 array of n (hi, wi) pairs, ``table``: its device copy (an int32 tensor)."""
    B, C, H, W = src.shape
    n = len(table_host) // 2
    args = (ptr(src), B, C, H, W, table_host, ptr(table), n, th, tw, ptr(dst))
    return Rec(L.load().edtr_tile_gather, args, (src, table_host, table, dst), name, 0.0, 8.0 * n * B * C * th * tw)


def make_tile_blend(*, tiles, wts, table_host, table, th, tw, out, name="tile_blend") -> Rec:
    """``out`` [B, C, H, W] = the ``wts``-weighted mean of the window-major ``tiles`` [n B, C, th, tw] over the windows covering each pixel,
    in one launch (the bits of zeroed planes -> make_tile_accumulate per window in table order -> make_divide)."""
    B, C, H, W = out.shape
    n = len(table_host) // 2
    args = (ptr(tiles), ptr(wts), table_host, ptr(table), n, th, tw, ptr(out), B, C, H, W)
    return Rec(L.load().edtr_tile_blend, args, (tiles, wts, table_host, table, out), name, 0.0, 4.0 * B * C * (n * th * tw + H * W))


def make_gn_pool(*, sums, weights, counts, T, BG, name="gn_pool") -> Rec:
    return Rec(L.load().edtr_gn_pool, (ptr(sums), ptr(weights), ptr(counts), T, BG), (sums, weights, counts), name)


def make_copy3d(*, src, src_plane, src_row, dst, dst_plane, dst_row, planes, rows, cols, name="copy3d") -> Rec:
    args = (ptr(src), src_plane, src_row, ptr(dst), dst_plane, dst_row, planes, rows, cols)
    return Rec(L.load().edtr_copy3d_f32, args, (src, dst), name, 0.0, 8.0 * planes * rows * cols)


def make_wavelet_level(*, src, low, high, planes, H, W, radius, name="wavelet_level") -> Rec:
    args = (ptr(src), ptr(low), ptr(high), planes, H, W, radius)
    return Rec(L.load().edtr_wavelet_level, args, (src, low, high), name, 0.0, 12.0 * planes * H * W)


# --------------------------------------------------------------------------------------------
# weight packing (host side, torch CPU or GPU tensors)
# --------------------------------------------------------------------------------------------
def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def split3_weight(w: torch.Tensor, dtype: torch.dtype = torch.bfloat16, parts: int = 3) -> torch.Tensor:
    """fp32 [..., C] -> 16-bit [..., parts*C] along the last axis, the weight side of a multi-part product:
    parts 3 = [hi | hi | lo] against the activation operand [hi | lo | hi] (xh*wh + xl*wh + xh*wl), parts 2 = [hi | hi] against
    [hi | lo] (the activation exact, the weight rounded once), parts 1 = [hi]."""
    hi = w.to(dtype)
    if parts == 1:
        return hi.contiguous()
    if parts == 2:
        return torch.cat([hi, hi], dim=-1).contiguous()
    lo = (w - hi.float()).to(dtype)
    if parts == PARTS_2W:       # [hi | lo] against the activation's one part read twice (edtr_hip.h: a_wrap): x16 . (Wh + Wl)
        return torch.cat([hi, lo], dim=-1).contiguous()
    return torch.cat([hi, hi, lo], dim=-1).contiguous()


def op_parts(parts: int) -> int:
    """Parts the ACTIVATION operand of a `parts`-policy product has (the weights-exact form reads one part twice)."""
    return 1 if parts == PARTS_2W else parts


def k_mult(parts: int) -> int:
    """K of a `parts`-policy product in units of the logical K."""
    return 2 if parts == PARTS_2W else parts


def _weight_format(dtype, parts: int):
    """(16-bit storage dtype, part count) of a packed matrix for a WeightStore dtype."""
    if dtype == F32S:
        return torch.bfloat16, 3
    if dtype == MIXED:
        if parts not in (1, 2, 3, PARTS_2W):
            raise ValueError(f"mixed-precision weights have 1..3 parts (or {PARTS_2W} = weights-exact two-part), got {parts}")
        return torch.float16, parts
    return dtype, 1


def pack_conv_weight(w: torch.Tensor, dtype, cin_pad: Optional[int] = None,
                     cout_pad: Optional[int] = None, parts: int = 1) -> torch.Tensor:
    """[Cout, Cin, kh, kw] fp32 -> [Cout_pad][kh][kw][Cin_pad] 16-bit, flattened to [N][K] (K contiguous).
    dtype == F32S / MIXED: [Cout_pad][kh][kw][parts*Cin_pad] with the channel axis split (split3_weight)."""
    co, ci, kh, kw = w.shape
    cip = cin_pad or round_up(ci, 8)
    cop = cout_pad or round_up(co, 8)
    out = torch.zeros((cop, kh, kw, cip), dtype=torch.float32, device=w.device)
    out[:co, :, :, :ci] = w.permute(0, 2, 3, 1)
    dt16, parts = _weight_format(dtype, parts)
    return split3_weight(out, dt16, parts).reshape(cop, -1)


# sub-pixel form of nearest-2x upsample + 3x3 conv: which 3x3 taps add up on source offset d (0 / 1) of output parity p
SUBPIXEL_TAPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}


def pack_conv_weight_subpixel(w: torch.Tensor, dtype, cin_pad: Optional[int] = None, parts: int = 1) -> torch.Tensor:
    """[Cout, Cin, 3, 3] fp32 -> four phase matrices [4 * Cout_pad][2 * 2 * parts * Cin_pad] of the sub-pixel form of
    `interpolate(nearest, x2) -> conv3x3` (include/edtr_hip.h: w_phase_stride; reference model/unet.py:70-79, model/vae.py:35-39):
    output pixel (2s + py, 2r + px) = sum over (dy, dx) in {0, 1}^2 of W[py, px][dy][dx] . src[s + py - 1 + dy, r + px - 1 + dx] with
    W[py, px][dy][dx] = sum of w[ky][kx] over ky in SUBPIXEL_TAPS[py][dy], kx in SUBPIXEL_TAPS[px][dx].  The sums are taken in
    fp32 BEFORE the 16-bit (or multi-part) rounding, so the packed operand is at least as close to the fp32 kernel as nine
    separately rounded taps."""
    co, ci, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise ValueError("the sub-pixel form is for 3x3 kernels")
    cip = cin_pad or round_up(ci, 8)
    cop = round_up(co, 8)
    wf = w.float()
    out = torch.zeros((4, cop, 2, 2, cip), dtype=torch.float32, device=w.device)
    for py in (0, 1):
        for px in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    acc = torch.zeros((co, ci), dtype=torch.float32, device=w.device)
                    for ky in SUBPIXEL_TAPS[py][dy]:
                        for kx in SUBPIXEL_TAPS[px][dx]:
                            acc = acc + wf[:, :, ky, kx]
                    out[2 * py + px, :co, dy, dx, :ci] = acc
    dt16, parts = _weight_format(dtype, parts)
    return split3_weight(out, dt16, parts).reshape(4 * cop, -1)


def subpixel_ok(H: int, W: int, Ce: int, N: int, B: int, ld: int = 0) -> bool:
    """Should this nearest-2x upsample convolution (source H x W, Ce operand channels incl. parts, N output channels) run in its
    sub-pixel form?  Policy: 128-column tiles and enough units to be worth a 146-KiB workgroup (the halo tile's own threshold);
    whether the halo kernel's sub-pixel geometry takes the launch is the planner's word (conv3x3_plan answers 16).  EDTR_SUBPIXEL=0
    keeps the 9-tap gather (A/B runs)."""
    units = B * (H // 16) * (W // 16) * 4 * ((N + 127) // 128)
    if os.environ.get("EDTR_SUBPIXEL", "1") == "0" or N % 128 or units < 48:
        return False
    return conv3x3_plan(B, H, W, Ce, N, ld=ld, subpixel=True) == 16


def pack_linear_weight(w: torch.Tensor, dtype, n_pad: Optional[int] = None, parts: int = 1) -> torch.Tensor:
    n, k = w.shape
    npad = n_pad or round_up(n, 8)
    out = torch.zeros((npad, round_up(k, 8)), dtype=torch.float32, device=w.device)
    out[:n, :k] = w
    dt16, parts = _weight_format(dtype, parts)
    return split3_weight(out, dt16, parts)


def geglu_perm(inner: int) -> torch.Tensor:
    """Row permutation that interleaves 32-row value / gate blocks (see edtr_hip.h, GEGLU epilogue)."""
    assert inner % 32 == 0
    j = torch.arange(inner // 32)
    val = (j[:, None] * 32 + torch.arange(32)[None, :])            # [J, 32]
    gate = val + inner
    return torch.cat([val, gate], dim=1).reshape(-1)               # [J * 64]


def pad_bias(b: Optional[torch.Tensor], n_pad: int) -> Optional[torch.Tensor]:
    if b is None:
        return None
    out = torch.zeros(n_pad, dtype=torch.float32, device=b.device)
    out[: b.numel()] = b.float()
    return out
