"""The cells of edtr_igemm's planner table (edtr_amd/csrc/igemm_plan.h) that production reaches or an explicit `tile` admits and no
other test launches: z-batched launches of every GEMM template, the 64-bit-address form of tile 3, tile 14 away from its one
comparison with tile 3, split-K on tiles 8 / 14 and with empty trailing splits.  One table for the device-free checks
(tests/test_igemm_cells_cpu.py: the plan, the automatic tile, the references) and the launches (tests/test_gpu_igemm_cells.py).

A Cell names its shape (`s`), the explicit tile, the options (`o`), what edtr_igemm_plan must answer (`expect`: the tile, or
E_UNSUPPORTED for a refusal cell) and the kernel it is meant to reach (`path`).  Three builders turn it into a launch:
  operands(cell, dtype)   dense CPU tensors of 16-bit values (fp32 for the bias vectors), seeded by the cell's name
  reference(cell, d, dt)  (ref, absref) of edtr_hip.h's epilogue order in `dt` (fp64 for the gates), [Z, M, n] each: the two parts
                          edtr_amd.testing.elem_ratio takes
  layout(cell, code)      the edtr_igemm_params fields and where every operand lives inside its poisoned buffer: ld = width + 8, two
                          guard rows behind every slice, z slices NOT in z order (outer / inner strides that differ per operand).
tests/stream_cells.py (the fp32-stream forms of the parity modes) uses the same three builders with further option keys, none of which
an older cell sets: res_f32 (an fp32 residual of that scale, ldr = N + 4 floats), out16 (the 16-bit mirror, ld16 = N + 16), a_wrap
(A read twice against [Wh | Wl]), gnp / slot (GroupNorm partials of the output, the reducer's slot rows), a_gn (GroupNorm + SiLU of the
input in the staging), split (A written as the real hi / lo parts of an fp32 tensor), ups = 2 (the sub-pixel form: four phase
matrices, guard rows between them), act = GEGLU."""
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from edtr_amd.testing import ACC_F32, LIPSCHITZ, geglu_slack

E_UNSUPPORTED = -5
PTR = 0x10000               # a 16-byte aligned placeholder: the planner looks at addresses, never through them
PLAN_CUS = 256              # the CU count edtr_igemm_plan assumes without a device (igemm.hip: igemm_plan::plan(pp, 256)); the three
                            # automatic rules asserted here (tiles 1 / 2, 6, 8) count tiles only and do not depend on it
GEGLU, SILU, LRELU = 1, 2, 4
TILE_BM_BN = {1: (128, 128), 2: (64, 64), 3: (128, 128), 6: (256, 256), 8: (128, 160), 14: (256, 32)}      # igemm_plan.h kTiles + the launches
GEMM_TILES = (1, 2, 3, 6, 8, 14)
WIDE_LD1, WIDE_LDW = 1 << 22, 1 << 24      # row strides (elements) that put 520 A rows / 136 W rows past 0xF0000000 bytes (kBufferLimit)

Cell = namedtuple("Cell", "name group kind tile expect path s o auto")

PATHS = {1: "igemm_kernel<2,2>", 2: "igemm_kernel<1,1>", 3: "igemm_dma_kernel<FAST=1>", 6: "igemm_256_kernel", 8: "igemm_n160_kernel<4,5>",
         14: "igemm_n160_kernel<8,1>"}


def _cell(name, group, kind, tile, s, o, expect=None, path=None, auto=None):
    return Cell(name, group, kind, tile, tile if expect is None else expect, path or PATHS.get(tile, "refused"), s, o, auto or [])


def _gemm(name, group, tile, M, N, K, Z=1, zdiv=1, **kw):
    meta = {k: kw.pop(k) for k in ("expect", "path", "auto") if k in kw}
    return _cell(name, group, "gemm", tile, dict(M=M, N=N, K=K, Z=Z, zdiv=zdiv), kw, **meta)


def _conv(name, group, tile, B, H, W, cin, cout, stride=1, pad=1, ups=0, Z=1, **kw):
    meta = {k: kw.pop(k) for k in ("expect", "path", "auto") if k in kw}
    return _cell(name, group, "conv", tile, dict(B=B, H=H, W=W, cin=cin, cout=cout, stride=stride, pad=pad, ups=ups, Z=Z, zdiv=1), kw, **meta)


def _cells():
    out = []
    # ---- a. z-batches: Z = 6 with zdiv = 3 (quotient and remainder both take more than one value), M = 2 BM + 1, N = BN + 8
    for t in GEMM_TILES:
        bm, bn = TILE_BM_BN[t]
        M, N = 2 * bm + 1, 40 if t == 14 else bn + 8
        f32, b16 = dict(out_f32=True, alpha=0.125), dict(bias_m=True, n_valid=N - 3)
        out += [_gemm(f"z6-t{t}-f32alpha", "z", t, M, N, 192, 6, 3, **f32), _gemm(f"z6-t{t}-biasm-nvalid", "z", t, M, N, 192, 6, 3, **b16),
                _gemm(f"z6-t{t}-sharedA", "z", t, M, N, 192, 6, 3, shared_a=True, **b16), _gemm(f"z6-t{t}-zdiv1", "z", t, M, N, 192, 6, 1, **f32)]
        if t <= 2:      # the register-staged K tail: K = 200 is no multiple of the 64-wide K-tile
            out += [_gemm(f"z6-t{t}-k200-f32alpha", "z", t, M, N, 200, 6, 3, **f32), _gemm(f"z6-t{t}-k200-biasm-nvalid", "z", t, M, N, 200, 6, 3, **b16)]
    for t in (3, 1):    # validation admits a z-batched convolution: the spatial offsets add to the z offset
        out.append(_conv(f"z2-conv3x3-t{t}", "z", t, 2, 12, 20, 64, 72, Z=2, bias_n=True))
    # the three production shapes at their smallest faithful size (M shrunk; `auto`: the full-size shape and the tile it must choose)
    for t in (1, 2):    # nets.py _g_vae_attn's fallback P V product of a 66 x 66 latent: K = 4360 is no multiple of 64
        out.append(_gemm(f"prod-pv-k4360-t{t}", "z", t, 129, 512, 4360, 2,
                         auto=[(dict(M=4356, Z=2), 1), (dict(M=4356, Z=1), 2)] if t == 1 else []))
    # engine.py Emitter.vt_gemm at 1600 tokens, batch 5: N % 160 == 0, N % 128 != 0, 4 * 10 * 5 = 200 tiles of 128 x 160
    out.append(_gemm("prod-vt-1600-t8", "z", 8, 129, 1600, 512, 5, shared_a=True, bias_m=True, n_valid=1600,
                     auto=[(dict(M=512, Z=5), 8), (dict(M=512, Z=4), 3)]))
    # the 4096-token P V product at batch 4: ksel >= 1024 and 16 * 2 * 4 = 128 tiles of 256 x 256
    out.append(_gemm("prod-pv-4096-t6", "z", 6, 257, 512, 1024, 4, auto=[(dict(M=4096, K=4096, Z=4), 6), (dict(M=4096, K=4096, Z=3), 3)]))

    # ---- b. the 64-bit-address form of tile 3 (bf16 only).  Small route: a nearest-2x source at stride 2
    full = dict(bias_n=True, rowvec=True, residual=True)
    for t in (3, 1, 2):
        out.append(_conv(f"up2-s2-t{t}", "wide", t, 2, 12, 20, 64, 72, stride=2, ups=1, path="igemm_dma_kernel<SPATIAL=1,FAST=0>" if t == 3 else None, **full))
    out += [_conv(f"up2-s2-refuse-t{t}", "refuse", t, 2, 12, 20, 64, 72, stride=2, ups=1, expect=E_UNSUPPORTED, **full) for t in (6, 8, 14)]
    # ... and the register-staged tiles on a nearest-2x source at stride 1 (test_conv3x3's `up` resolves to tile 3)
    out += [_conv(f"up2-s1-t{t}", "wide", t, 2, 12, 20, 64, 72, ups=1, **full) for t in (1, 2)]
    # wide operands: a row stride, not a shape, carries the last rows past a 4 GiB byte offset
    # (521 rows of 2^22 elements: rows 512.. start past 2^32 bytes; the 17 x 16 images likewise; 136 W rows of 2^24 elements)
    wide = [(lambda t, g, **kw: _gemm(f"wideA-gemm-t{t}", g, t, 521, 136, 192, ld1=WIDE_LD1, bias_n=True, **kw), "igemm_dma_kernel<SPATIAL=0,FAST=0>"),
            (lambda t, g, **kw: _conv(f"wideA-conv3x3-t{t}", g, t, 2, 17, 16, 192, 72, ld1=WIDE_LD1, bias_n=True, residual=True, **kw), "igemm_dma_kernel<SPATIAL=1,FAST=0>"),
            (lambda t, g, **kw: _gemm(f"wideW-gemm-t{t}", g, t, 129, 136, 192, ldw=WIDE_LDW, bias_n=True, **kw), "igemm_dma_kernel<SPATIAL=0,FAST=0>")]
    for mk, path in wide:
        out += [mk(t, "wide", expect=3, path=path) for t in (0, 3)]
        out += [mk(t, "refuse", expect=E_UNSUPPORTED) for t in (6, 8, 14, 16, 17)]

    # ---- c. tile 14 on its own: ragged M, N = 8 / 24 / 32 / 40, both stores, every epilogue, every form
    lre = dict(act=LRELU, slope=0.2, bias_n=True)
    out += [_gemm("t14-gemm-m513-n8-full", "t14", 14, 513, 8, 128, **full), _gemm("t14-gemm-m300-n24-f32-silu", "t14", 14, 300, 24, 128, out_f32=True, act=SILU, bias_n=True),
            _gemm("t14-gemm-m513-n32-lrelu", "t14", 14, 513, 32, 128, **lre), _gemm("t14-gemm-m300-n40-full", "t14", 14, 300, 40, 192, **full),
            _gemm("t14-gemm-m513-n40-f32", "t14", 14, 513, 40, 128, out_f32=True, bias_n=True),
            _conv("t14-conv-s1-n24-full", "t14", 14, 2, 12, 20, 64, 24, **full), _conv("t14-conv-s1-n40-f32-lrelu", "t14", 14, 2, 12, 20, 64, 40, out_f32=True, **lre),
            _conv("t14-conv-s2-pad0-n8-silu", "t14", 14, 2, 24, 40, 64, 8, stride=2, pad=0, act=SILU, bias_n=True),
            _conv("t14-conv-s2-pad0-n32-f32-full", "t14", 14, 2, 24, 40, 64, 32, stride=2, pad=0, out_f32=True, **full),
            _conv("t14-conv-up2-n32-f32-lrelu", "t14", 14, 2, 12, 20, 64, 32, ups=1, out_f32=True, **lre), _conv("t14-conv-up2-n40-full", "t14", 14, 2, 12, 20, 64, 40, ups=1, **full)]

    # ---- d. split-K: tiles 8 and 14 at test_gemm_splitk's shapes, then trailing splits that own no K-tile (per = ceil(10 / S) = 2)
    out += [_gemm("sk-t8-m512-n320-k1152-s4", "splitk", 8, 512, 320, 1152, splitk=4, **full), _gemm("sk-t8-m100-n168-k640-s10", "splitk", 8, 100, 168, 640, splitk=10, **full),
            _gemm("sk-t8-m64-n320-k2880-s7", "splitk", 8, 64, 320, 2880, splitk=7, **full), _gemm("sk-t14-m512-n32-k1152-s4", "splitk", 14, 512, 32, 1152, splitk=4, **full),
            _gemm("sk-t14-m100-n32-k640-s10", "splitk", 14, 100, 32, 640, splitk=10, **full)]
    for t in (1, 2, 3, 8, 14):
        out += [_gemm(f"sk-empty-t{t}-k640-s{S}", "splitk", t, 100, 32 if t == 14 else 72, 640, splitk=S, **full) for S in (7, 8)]
    out += [_conv(f"sk-empty-conv3x3-t{t}-s7", "splitk", t, 2, 8, 8, 128, 136, splitk=7, **full) for t in (1, 2, 3)]      # 9 * 128 / 64 = 18 K-tiles, per = 3
    out.append(_gemm("sk-refuse-t6", "refuse", 6, 100, 72, 640, splitk=7, expect=E_UNSUPPORTED, **full))      # (kTiles: tile 6 has no split-K; the workspace stays as it was)
    return out


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)


def cells(group):
    return [c for c in CELLS if c.group == group]


def ids(cs):
    return [c.name for c in cs]


# ---- shape arithmetic ----------------------------------------------------------------------------------------------------------------
def out_hw(s):
    """Output height / width of a convolution cell: pad = 1 is conv2d(padding=1); pad = 0 the VAE's F.pad(x, (0, 1, 0, 1)) + padding 0."""
    up = 2 if s["ups"] else 1

    def one(L):
        L *= up
        return (L - 1) // s["stride"] + 1 if s["pad"] else (L - 2) // s["stride"] + 1
    return one(s["H"]), one(s["W"])


def dims(c):
    """(M, N, K) of a cell."""
    s = c.s
    if c.kind == "gemm":
        return s["M"], s["N"], s["K"]
    oh, ow = out_hw(s)
    return s["B"] * oh * ow, s["cout"], 9 * s["cin"]


def a_shape(c):
    """(rows, columns) of one z slice of the A operand: the matrix, or the NHWC image."""
    s = c.s
    if c.kind == "gemm":
        return s["M"], s["K"] // 2 if c.o.get("a_wrap") else s["K"]      # a_wrap: the columns are read twice
    return s["B"] * s["H"] * s["W"], s["cin"]


def n_out(c):
    """Stored columns: GEGLU folds the value / gate pairs."""
    N = dims(c)[1]
    return N // 2 if c.o.get("act") == GEGLU else N


def phases(c):
    """Weight matrices per launch: 4 in the sub-pixel form of the upsample convolution (edtr_hip.h: w_phase_stride), each [N][2][2][C1]."""
    return 4 if c.kind == "conv" and c.s["ups"] == 2 else 1


def images(c):
    """(rowvec rows, rows_per_image): a GEMM's rows are dealt to three `images` whose last one is short, so a row tile straddles two."""
    M = dims(c)[0]
    if c.kind == "conv":
        oh, ow = out_hw(c.s)
        return c.s["B"], oh * ow
    return 3, (M + 2) // 3


# ---- operands and references ------------------------------------------------------------------------------------------------------------
def operands(c, dtype):
    M, N, K = dims(c)
    Z, o = c.s["Z"], c.o
    rows, C1 = a_shape(c)
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))

    def r(*shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale
    # W keeps n_valid rows per slice: the rows at and beyond n_valid "read as zero" (edtr_hip.h) and belong to the next slice in memory
    if o.get("split"):      # the real parts of an fp32 tensor: [hi | lo | hi][:parts] (edtr_split_operand's formats), C1 = parts * C
        x = r(Z, rows, C1 // o["split"])
        hi = x.to(dtype)
        a = torch.cat([hi, (x - hi.float()).to(dtype), hi][:o["split"]], dim=2)
    else:
        a = r(1 if o.get("shared_a") else Z, rows, C1).to(dtype)
    if phases(c) == 4:
        d = {"a": a, "w": r(4, N, 4 * C1, scale=1 / math.sqrt(4 * C1)).to(dtype)}
    else:
        d = {"a": a, "w": r(Z, o.get("n_valid") or N, K, scale=1 / math.sqrt(K)).to(dtype)}
    if o.get("bias_n"):
        d["bias_n"] = r(N)
    if o.get("bias_m"):
        d["bias_m"] = r(M)
    if o.get("rowvec"):
        d["rowvec"] = r(images(c)[0], N)
    if o.get("residual"):
        d["res"] = r(M, n_out(c), scale=o["res_f32"]) if o.get("res_f32") else r(M, N).to(dtype)
    if o.get("a_gn"):       # the (scale, shift) table edtr_gn_table would derive: [B][C1][2] fp32
        d["gn_table"] = torch.stack([1 + 0.2 * r(c.s["B"], C1), 0.2 * r(c.s["B"], C1)], dim=-1)
    return d


def _product(c, a, w):
    """[Z, M, N] = A(z) W(z)^T in the dtype of a / w; a convolution through conv2d on the NCHW image and the [N][ky][kx][cin] weights."""
    if c.kind == "gemm":
        return a @ w.transpose(1, 2)
    s = c.s
    if phases(c) == 4:      # output pixel (2 sy + py, 2 sx + px) = a 2 x 2 convolution of source rows sy + py - 1 .. sy + py with phase 2 py + px
        x = F.pad(a[0].reshape(s["B"], s["H"], s["W"], s["cin"]).permute(0, 3, 1, 2), (1, 1, 1, 1))
        y = x.new_zeros((s["B"], w.shape[1], 2 * s["H"], 2 * s["W"]))
        for py in (0, 1):
            for px in (0, 1):
                wp = w[2 * py + px].reshape(-1, 2, 2, s["cin"]).permute(0, 3, 1, 2)
                y[:, :, py::2, px::2] = F.conv2d(x[:, :, py:py + s["H"] + 1, px:px + s["W"] + 1], wp)
        return y.permute(0, 2, 3, 1).reshape(1, -1, y.shape[1])
    outs = []
    for z in range(w.shape[0]):
        x = a[z].reshape(s["B"], s["H"], s["W"], s["cin"]).permute(0, 3, 1, 2)
        wz = w[z].reshape(-1, 3, 3, s["cin"]).permute(0, 3, 1, 2)
        if s["ups"]:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        if not s["pad"]:
            x = F.pad(x, (0, 1, 0, 1))
        y = F.conv2d(x, wz, stride=s["stride"], padding=1 if s["pad"] else 0)
        outs.append(y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]))
    return torch.stack(outs)


def reference(c, d, dt=torch.float64):
    """(ref, absref), [Z, M, N] in `dt`, from the 16-bit values the kernel reads, in edtr_hip.h's epilogue order: alpha, bias_n, bias_m,
    rowvec, activation, residual; absref the same on absolute values (the activation by its Lipschitz constant)."""
    M, N, _ = dims(c)
    Z, o = c.s["Z"], c.o
    a, w = d["a"].to(dt), d["w"].to(dt)
    if "gn_table" in d:     # a_gn: silu(a * scale + shift) rounded to 16 bits as edtr_gn_apply stores it (stream_cells adds the flip term)
        from swin_cases import gn_apply16
        t = d["gn_table"]
        a = gn_apply16(d["a"].float().reshape(c.s["B"], -1, a.shape[2]), t[:, None, :, 0], t[:, None, :, 1], d["a"].dtype)[0].reshape(a.shape).to(dt)
    if o.get("a_wrap"):
        a = torch.cat([a, a], dim=2)
    if phases(c) == 1:
        a = a.expand(Z, -1, -1)
    w = F.pad(w, (0, 0, 0, N - w.shape[1]))
    alpha = o.get("alpha", 1.0)
    ref, ab = alpha * _product(c, a, w), abs(alpha) * _product(c, a.abs(), w.abs())
    if "bias_n" in d:
        t = d["bias_n"].to(dt)
        ref, ab = ref + t, ab + t.abs()
    if "bias_m" in d:
        t = d["bias_m"].to(dt)[:, None]
        ref, ab = ref + t, ab + t.abs()
    if "rowvec" in d:
        t = d["rowvec"].to(dt).repeat_interleave(images(c)[1], dim=0)[:M]
        ref, ab = ref + t, ab + t.abs()
    if o.get("act") == GEGLU:      # value / gate blocks of 32 columns interleaved by the weight packer (ops.geglu_perm)
        from edtr_amd.ops import geglu_perm
        perm, K = geglu_perm(N // 2), dims(c)[2]
        h, hab = torch.empty_like(ref), torch.empty_like(ab)
        h[..., perm], hab[..., perm] = ref, ab
        val, gate = h[..., :N // 2], h[..., N // 2:]
        ref = val * F.gelu(gate)
        # the product rule's slack stands in for absref: the caller's k 2^-22 absref is then geglu_slack exactly
        ab = geglu_slack(val, gate, hab[..., :N // 2], hab[..., N // 2:], K).to(dt) / (K * ACC_F32)
    elif o.get("act") == SILU:
        ref, ab = F.silu(ref), LIPSCHITZ["silu"] * ab
    elif o.get("act") == LRELU:
        ref, ab = torch.where(ref > 0, ref, o["slope"] * ref), LIPSCHITZ["leaky"] * ab
    if "res" in d:
        t = d["res"].to(dt)
        ref, ab = ref + t, ab + t.abs()
    return ref, ab


# ---- layout: parameters and the place of every slice ------------------------------------------------------------------------------------
Slab = namedtuple("Slab", "numel offs rows cols ld")      # a poisoned buffer of `numel` elements; slice z = [rows, cols] at element offs[z], row stride ld


def layout(c, dtype_code=0, shape=None, tile=None):
    """-> (fields, pointer field names, {"a", "w", "out"[, "res", "out16", "gnp"]: Slab}).  `shape` overrides entries of the cell's shape
    (the full-size production shape of an `auto` check), `tile` the explicit tile.  The row strides all differ: ldc = n + 8, ldr = n + 4
    floats for an fp32 residual, ld16 = n + 16; the "gnp" slab is [slots][2 N] floats with one guard slot behind it."""
    c = c._replace(s=dict(c.s, **(shape or {})))
    s, o = c.s, c.o
    M, N, K = dims(c)
    Z, zdiv = s["Z"], s["zdiv"]
    rows, C1 = a_shape(c)
    No, P = n_out(c), phases(c)
    ld1, ldw, ldc = o.get("ld1", C1 + 8), o.get("ldw", (4 * C1 if P == 4 else K) + 8), No + 8
    nv = o.get("n_valid", 0)
    SA, SO = (rows + 2) * ld1, (M + 3) * ldc
    SW = nv * ldw if nv else (N + 2) * ldw      # n_valid: the next slice's live rows follow at once, so reading a row >= n_valid shows

    def strides(S, P, Q, step1=2):      # zdiv > 1: slot zo P + zi Q (injective for the patterns used below); zdiv = 1: every step1-th slot
        if Z == 1:
            return 0, 0
        return (P * S, Q * S) if zdiv > 1 else (step1 * S, S)      # (zdiv = 1: the inner stride is set and must not be used)

    def offsets(st):
        offs = [(z // zdiv) * st[0] + (z % zdiv) * st[1] for z in range(Z)]
        assert len(set(offs)) == Z or st == (0, 0)
        return offs
    a_zs = (0, 0) if o.get("shared_a") else strides(SA, 1, 2)
    w_zs, o_zs = strides(SW, 3, 2, 1 if nv else 2), strides(SO, 1, 3)
    ao, wo, oo = offsets(a_zs), offsets(w_zs), offsets(o_zs)
    if P == 4:      # the four phase matrices, w_phase_stride apart: two guard rows behind each
        wo = [i * SW for i in range(4)]
    slabs = {"a": Slab(max(ao) + SA, ao, rows, C1, ld1), "w": Slab(max(wo) + SW + 2 * ldw, wo, nv or N, 4 * C1 if P == 4 else K, ldw),
             "out": Slab(max(oo) + SO, oo, M, No, ldc)}
    f = dict(dtype=dtype_code, taps=9 if c.kind == "conv" else 1, M=M, N=N, K=K, n_valid=nv, Z=Z, zdiv=zdiv, C1=K if o.get("a_wrap") else C1, ld1=ld1, ldw=ldw,
             a_zs_outer=a_zs[0], a_zs_inner=a_zs[1], w_zs_outer=w_zs[0], w_zs_inner=w_zs[1], o_zs_outer=o_zs[0], o_zs_inner=o_zs[1],
             alpha=o.get("alpha", 1.0), ldc=ldc, out_f32=int(bool(o.get("out_f32"))), act=o.get("act", 0), act_slope=o.get("slope", 0.0),
             tile=c.tile if tile is None else tile, splitk=o.get("splitk", 0))
    ptrs = ["a1", "w", "out"]
    if c.kind == "conv":
        oh, ow = out_hw(s)
        f.update(IH=s["H"], IW=s["W"], OH=oh, OW=ow, stride=s["stride"], pad_t=s["pad"], pad_l=s["pad"], upsample2x=s["ups"])
    for name in ("bias_n", "bias_m"):
        if o.get(name):
            ptrs.append(name)
    if o.get("rowvec"):
        f.update(rowvec_ld=N, rows_per_image=images(c)[1])
        ptrs.append("rowvec")
    if P == 4:
        f.update(w_phase_stride=SW)
    if o.get("a_wrap"):
        f.update(a_wrap=K // 2)
    if o.get("residual"):
        ldr = No + 4 if o.get("res_f32") else N + 8
        f.update(ldr=ldr, residual_f32=int(bool(o.get("res_f32"))))
        ptrs.append("residual")
        slabs["res"] = Slab((M + 2) * ldr, [0], M, No, ldr)
    if o.get("out16"):
        f.update(ld16=No + 16)
        ptrs.append("out16")
        slabs["out16"] = Slab((M + 2) * (No + 16), [0], M, No, No + 16)
    if o.get("gnp"):
        slots = M // (o.get("slot") or 128)
        f.update(gn_slot_rows=o.get("slot", 0))
        ptrs.append("gn_partial")
        slabs["gnp"] = Slab((slots + 1) * 2 * N, [0], slots, 2 * N, 2 * N)
    if o.get("a_gn"):
        f.update(a_gn_silu=1, rows_per_image=images(c)[1])
        ptrs.append("a_gn")
    if o.get("splitk", 0) > 1:
        f.update(workspace_bytes=o["splitk"] * M * N * 4)
        ptrs.append("workspace")
    return f, ptrs, slabs


def to_params(fields, ptrs=(), addr=None):
    """edtr_igemm_params from a dict of fields (layout()'s); the pointer fields `ptrs` from `addr` (name -> address), placeholders without."""
    from edtr_amd import lib as L
    p = L.IgemmParams()
    for k, v in fields.items():
        setattr(p, k, v)
    for k in ptrs:
        setattr(p, k, PTR if addr is None else addr[k])
    return p


def plan_of(p):
    import ctypes
    from edtr_amd import lib as L
    return int(L.load().edtr_igemm_plan(ctypes.byref(p)))
