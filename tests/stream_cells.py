"""The edtr_igemm forms that the parity modes (mixed / hybrid / robust / high) emit and the 16-bit fast mode never reaches: an fp32 output,
an fp32 residual, the 16-bit mirror out16, the weights-exact product a_wrap, GroupNorm partials of an fp32 output, the split-K reducer
doing all of these, operands two or three parts wide per tap.  One table for the device-free checks (tests/test_stream_cells_cpu.py: the
plans, the census of what production emits, the defects the checks reject) and the launches (tests/test_gpu_stream_cells.py).

The CENSUS reduces every edtr_igemm record of the sd21 programs (census(): CldmEngine(8, 64, 64, 77) context + step, VAE encode
8 x 512 x 512, VAE decode 8 x 64 x 64) that sets out_f32, residual_f32, out16 or a_wrap to form_key(): the planned tile and the options that
pick a kernel path.  Every emitted key is some cell's `covers`; every cell's `covers` is emitted unless the cell is `extra`.

A cell is an igemm_cells.Cell (shape, explicit tile, options, the tile edtr_igemm_plan must answer) plus `covers`, the production
`launch` it stands for and the dtypes it runs in (fp16 always, bf16 where the `high` mode emits the form).  igemm_cells' builders make
the operands, the fp64 reference and the layout.  Shapes are the smallest that keep the geometry: one 48 x 48 image for tile 16's
patches (corner, edge and interior), eight 8 x 8 images for its image form (two workgroups), 2 x 2 units of 32 x 16 for tile 17, two
16 x 16 units side by side for tile 20, M = 2 BM + 1 for the GEMM tiles where the form admits a ragged M and M = 256 (512 for tile 6)
with two or more images or slots where the statistics need whole slots.  Operands `parts` wide (C1 = parts * C) hold independent O(1)
values in every part: the kernel sees plain columns, so a dropped or misaddressed part is an O(1) error; three `split` cells write the
real hi / lo parts of an fp32 tensor instead, one per format.

Every operand and output lives in a NaN-filled buffer, ld = width + 8 (+ 4 floats for the fp32 residual, + 16 for the mirror: ldr != ldc
!= ld16), two guard rows behind every slice, the split-K workspace and the gn_partial buffer poisoned with a guard behind them.  Case
makes the buffers on the host, judge() is every check of a finished launch (it only reads host tensors), simulate() is a perfect kernel
on the host (the fp64 reference rounded once) with the named DEFECTS: the CPU file shows that judge() accepts the former and rejects the
latter, the GPU file hands judge() what the device wrote.

No tolerance of its own: the output is held to edtr_amd.testing.elem_bound (k = the reduction length, fp32 or 16-bit output), the mirror
to bit equality with the cast of the stored output, every statistics slot to the same bound form against fp64 sums of the STORED output
over that slot's rows with k = the rows.

The fp32 residual is drawn at RES_SCALE = 32: rounding it to the operand type is then an error of 2^-12.5 |res| (fp16; 2^-9.5 bf16) at the
median against a bound of K 2^-22 |res|, a ratio of 724 / K (5792 / K).  res16_visible(): where that is >= 8 the CPU file asserts that the
rounding exceeds the bound 4 x on half the elements; for a longer K the element bound cannot see a residual rounded to 16 bits, and no
derivable bound can (k 2^-22 absref is the project's accumulation term) — there the mirror's bit equality and the statistics still
hold the epilogue, the rounding itself is only seen by the short-K cells of the same tile.

Worst element ratios measured on the MI355X stand beside the cells."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import igemm_cells as IC
from edtr_amd.testing import elem_ratio

NAN = float("nan")
RES_SCALE = 32.0
E_UNSUPPORTED = IC.E_UNSUPPORTED
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
HALO_UNIT = {16: (16, 16), 17: (16, 32), 20: (16, 16)}      # rows x columns of output pixels per workgroup (igemm.hip / halo512.hip)
HALO_SLOTS = {16: 2, 17: 4, 20: 2}                          # 128-row gn_partial slots per unit: the first takes the sums, the others zeros


# ---- the census' reduction ------------------------------------------------------------------------------------------------------------------
def form_key(tile, p):
    """One edtr_igemm launch reduced to the planned tile and the options that select a kernel path, nothing about sizes.  `p` is anything
    with edtr_igemm_params' fields.  gn_slot_rows counts only where it is read (gn_partial behind split-K: the reducer's slots);
    `ldc>N` is a row stride wider than the stored columns."""
    n_out = p.N // 2 if p.act == 1 else p.N
    t = [f"t{tile}", f"taps{p.taps}"]
    if p.OH > 0 and p.stride != 1:
        t.append(f"s{p.stride}")
    if p.upsample2x:
        t.append({1: "up2", 2: "up2sp"}[p.upsample2x])
    t.append("f32" if p.out_f32 else "o16")
    if p.residual:
        t.append("r32" if p.residual_f32 else "r16")
    for name, on in (("m16", p.out16), ("2w", p.a_wrap), ("gnp", p.gn_partial)):
        if on:
            t.append(name)
    if p.gn_partial and p.splitk > 1:
        t.append(f"slot{p.gn_slot_rows or 128}")
    for name, on in (("gnin", p.a_gn), ("sk", p.splitk > 1), (f"act{p.act}", p.act), ("rv", p.rowvec), ("vT", p.vt_out), ("Z", p.Z > 1),
                     ("ldc>N", p.ldc > n_out)):
        if on:
            t.append(name)
    return " ".join(t)


def in_census(p):
    return bool(p.out_f32 or p.residual_f32 or p.out16 or p.a_wrap)


def census(mode):
    """{key: {"launch": the first record that reduces to it, "n": how many do, "bf16": any of them in bf16}} of the sd21 programs of one
    precision mode, built on the CPU."""
    from edtr_amd import lib, synth
    from edtr_amd.model import ControlLDM
    from edtr_amd.model.cldm import CldmEngine, VaeEngine
    from edtr_amd.model.params import skip_init
    with skip_init():
        model = ControlLDM(**synth.sd21_config()).eval()
    model.compute_dtype = torch.bfloat16
    model.precision = model.controlnet.precision = model.unet.precision = mode
    model.release_engines()
    eng = CldmEngine(model, 8, 64, 64, 77)
    progs = [eng.ctx_prog.recs, eng.step_prog.recs] + [VaeEngine(model, *a).prog.recs for a in (("encode", 8, 512, 512), ("decode", 8, 64, 64))]
    out = {}
    for recs in progs:
        for r in recs:
            if getattr(r.fn, "__name__", "") != "edtr_igemm":
                continue
            p = r.args[0]._obj
            if not in_census(p):
                continue
            e = out.setdefault(form_key(int(lib.load().edtr_igemm_plan(r.args[0])), p), {"launch": f"{mode}: {r.name} {r.tag}", "n": 0, "bf16": False})
            e["n"] += 1
            e["bf16"] = e["bf16"] or p.dtype == lib.BF16
    return out


class _Fields:
    """layout()'s fields and pointer names behind edtr_igemm_params' attribute names (an unset field is 0, a named pointer is set)."""

    def __init__(self, f, ptrs):
        self.f, self.ptrs = f, set(ptrs)

    def __getattr__(self, k):
        return 1 if k in self.ptrs else self.f.get(k, 0)


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
SCell = namedtuple("SCell", "name cell covers launch dtypes extra")
F32 = dict(out_f32=True, bias_n=True)
R32 = dict(residual=True, res_f32=RES_SCALE)
GNP, M16, RV = dict(gnp=True), dict(out16=True), dict(rowvec=True)


def _mk(cell, launch, bf16=False, ldcN=(0,), extra=None, dtypes=None):
    """`ldcN`: the `ldc>N` flags of the production keys the cell stands for (the cell itself always launches with ldc = N + 8)."""
    f, ptrs, _ = IC.layout(cell)
    covers = ()
    if cell.expect > 0:
        f = dict(f, ldc=0)
        base = form_key(cell.expect, _Fields(f, ptrs))
        covers = tuple(base + (" ldc>N" if flag else "") for flag in ldcN)
    return SCell(cell.name, cell, covers, launch, tuple(dtypes or (("fp16", "bf16") if bf16 else ("fp16",))), extra)


def _opts(*bundles, **kw):
    o = {}
    for b in bundles:
        o.update(b)
    o.update(kw)
    return o


def _cells():
    # Trailing comments: the worst ratios measured on the MI355X, output / statistics slots / split-K against the unsplit launch, fp16 first,
    # bf16 in brackets.  A residual rounded to 16 bits is a defect the element bound sees at K <= 90 in fp16 and K <= 724 in bf16
    # (res16_visible): the K = 64 GEMM cells of tiles 3 / 6 / 8 in both dtypes, the K = 576 halo cells (t16-r32-gnp, t17-r32-gnp, t20-r32-gnp-*)
    # and the K = 320 split-K GEMM cells in bf16; NOT the fp16 runs of those, the three-part halo cells (K >= 1728), t17-r32-gnp-gnin (fp16 only)
    # or the 16-bit outputs.
    g, cv = IC._gemm, IC._conv
    out = []

    def add(cell, launch, **kw):
        out.append(_mk(cell, launch, **kw))

    # ---- tile 16, 16 x 16 patches of one 48 x 48 image: 9 patches (4 corners, 4 edges, 1 interior), 3 parts of 64 channels per tap
    P = (1, 48, 48)
    add(cv("t16-rv-gnp", "t16", 16, *P, 192, 128, parts=3, **_opts(F32, GNP, RV)), "robust res.conv1 M8192 N640 K8640", bf16=True)      # 0.00014 / 0.0027 (0.00013 / 0.0028)
    add(cv("t16-rv-gnp-sk128", "t16", 16, *P, 192, 128, parts=3, splitk=3, **_opts(F32, GNP, RV)), "robust res.conv1 M2048 N1280 K17280 sk3", bf16=True)      # 7.3e-05 / 0.013 / 0.00016 (7.3e-05 / 0.014 / 0.00013)
    add(cv("t16-r32-gnp", "t16", 16, *P, 64, 128, **_opts(F32, R32, GNP)), "mixed res.conv2 M8192 N640 K5760", bf16=True)      # 0.00041 / 0.003 (0.00038 / 0.0025)
    add(cv("t16-r32-gnp-sk128", "t16", 16, *P, 192, 128, parts=3, splitk=3, **_opts(F32, R32, GNP)), "mixed res.conv2 M2048 N1280 K11520 sk3", bf16=True)      # 0.00012 / 0.012 / 0.00022 (0.00012 / 0.014 / 0.00023)
    # ---- tile 16, four whole 8 x 8 images per workgroup: 8 images = two workgroups, two column tiles, 6 chunks dealt 1 / 2 / 1 / 2 to four
    # splits (the halo kernel deals chunks by floor((y + 1) n / S) - floor(y n / S): the short splits are not the trailing ones)
    I8 = (8, 8, 8, 384, 256)
    i8 = dict(parts=3, splitk=4)
    add(cv("t16-img8-rv-gnp-sk64", "t16", 16, *I8, slot=64, **_opts(F32, GNP, RV, i8)), "robust res.conv1 M512 N1280 K34560 sk10", bf16=True)      # 3.2e-05 / 0.029 / 6.8e-05 (3.1e-05 / 0.029 / 6.3e-05)
    add(cv("t16-img8-r32-gnp-sk64", "t16", 16, *I8, slot=64, **_opts(F32, R32, GNP, i8)), "mixed res.conv2 M512 N1280 K11520 sk10", bf16=True)      # 5.8e-05 / 0.03 / 0.00011 (5.6e-05 / 0.03 / 0.00011)
    add(cv("t16-img8-r32-m16-gnp-sk64", "t16", 16, *I8, slot=64, **_opts(F32, R32, GNP, M16, i8)), "mixed res.conv2 M512 N1280 K11520 sk10 m16")      # 5.8e-05 / 0.029 / 0.00011
    add(cv("t16-img8-r32-m16-sk", "t16", 16, *I8, **_opts(F32, R32, M16, i8)), "mixed res.conv2 M512 N1280 K11520 sk10 m16, ldc > N", ldcN=(1,))      # 5.5e-05 / 0.00011
    add(cv("t16-img8-r32-sk", "t16", 16, *I8, **_opts(F32, R32, i8)), "high res.conv2 M512 N1280 K34560 sk10, ldc > N", bf16=True, ldcN=(1,))      # 5.8e-05 / 0.00011 (5.8e-05 / 0.00012)
    # ---- tile 16 on an upsampled source: the nearest-2x gather (16 x 16 -> 32 x 32) behind split-K, the sub-pixel form (16 x 32 -> 32 x 64)
    add(cv("t16-up2-m16-sk", "t16", 16, 1, 16, 16, 192, 128, ups=1, parts=3, splitk=3, **_opts(F32, M16)), "mixed upsample.conv M2048 N1280 K11520 up2 sk3 m16", ldcN=(1,))      # 7.7e-05 / 0.00015
    add(cv("t16-up2-sk", "t16", 16, 1, 16, 16, 192, 128, ups=1, parts=3, splitk=3, **F32), "high upsample.conv M2048 N1280 K34560 up2 sk3", bf16=True, ldcN=(1,))      # 6.3e-05 / 0.00015 (7.7e-05 / 0.00013)
    add(cv("t16-up2sp-gnp", "t16", 16, 1, 16, 32, 64, 128, ups=2, **_opts(F32, GNP)), "mixed vae.upsample.conv M131072 N512 K13824 up2sp", bf16=True)      # 0.0012 / 0.0036 (0.0011 / 0.0028)
    add(cv("t16-up2sp", "t16", 16, 1, 16, 32, 192, 128, ups=2, parts=3, **F32), "high upsample.conv M8192 N1280 K34560 up2sp", bf16=True, ldcN=(1,))      # 0.00036 (0.00031)
    add(cv("t16-up2sp-m16", "t16", 16, 1, 16, 32, 64, 128, ups=2, **_opts(F32, M16)), "mixed upsample.conv M8192 N1280 K11520 up2sp m16", ldcN=(1,))      # 0.0011
    # ---- tile 17: 2 x 2 units of 32 x 16 pixels (every unit has two image borders)
    U = (1, 32, 64)
    add(cv("t17-gnp", "t17", 17, *U, 96, 128, parts=3, **_opts(F32, GNP)), "high vae.conv1 M2097152 N128 K3456", bf16=True)      # 0.00054 / 0.00093 (0.00049 / 0.0011)
    add(cv("t17-r32-gnp", "t17", 17, *U, 64, 128, **_opts(F32, R32, GNP)), "mixed vae.conv2 M524288 N256 K2304", bf16=True)      # 0.00056 / 0.0011 (0.00051 / 0.0012)
    add(cv("t17-r32-gnp-gnin", "t17", 17, *U, 64, 128, a_gn=True, **_opts(F32, R32, GNP)), "mixed vae.conv2 M2097152 N128 K1152 with GroupNorm + SiLU of the input in the staging")      # 0.18 / 0.0012
    # ---- tile 20: two 16 x 16 units side by side, one and two 160-column tiles
    # rv-gnp n160: 0.00022 / 0.0023 (0.00021 / 0.0024), n320: 0.00024 / 0.0028 (0.00029 / 0.0024)
    # r32-gnp n160: 0.00048 / 0.003 (0.00054 / 0.0024), n320: 0.00083 / 0.0021 (0.00048 / 0.0023)
    for n in (160, 320):
        add(cv(f"t20-rv-gnp-n{n}", "t20", 20, 1, 16, 32, 192, n, parts=3, **_opts(F32, GNP, RV)), "robust res.conv1 M32768 N320 K8640", bf16=True,
            extra=None if n == 160 else "the second column tile of tile 20")
        add(cv(f"t20-r32-gnp-n{n}", "t20", 20, 1, 16, 32, 64, n, **_opts(F32, R32, GNP)), "mixed res.conv2 M32768 N320 K2880", bf16=True,
            extra=None if n == 160 else "the second column tile of tile 20")
    # ---- tile 3, GEMMs: M = 2 BM + 1 and N = BN + 8; K = 64 where an fp32 residual is added (its 16-bit rounding is then visible);
    # split-K over 5 K-tiles in 4 splits of 2 / 2 / 1 / 0 (an empty trailing split)
    add(g("t3-f32", "t3", 3, 257, 136, 128, **F32), "mixed zero_conv M8192 N320 K320", bf16=True)      # 0.0035 (0.0026)
    add(g("t3-2w", "t3", 3, 257, 136, 256, a_wrap=True, **F32), "mixed res.skip1x1 M2048 N1280 K1280 2w")      # 0.0016
    add(g("t3-2w-sk", "t3", 3, 257, 136, 256, a_wrap=True, splitk=3, **F32), "mixed res.skip1x1 M512 N1280 K5120 sk6 2w (4 K-tiles in 3 splits: 2 / 2 / 0)")      # 0.001 / 0.0018
    add(g("t3-z", "t3", 3, 257, 136, 128, Z=2, **F32), "high ctx_vT(all) M5760 N80 K3072 Z8", bf16=True)      # 0.0026 (0.0025)
    add(g("t3-geglu", "t3", 3, 257, 192, 128, act=IC.GEGLU, **F32), "robust ff.geglu M32768 N2560 K960 act1", bf16=True)      # 0.0015 (0.0012)
    add(g("t3-silu", "t3", 3, 257, 136, 128, act=IC.SILU, **F32), "mixed time_embed.0 M8 N1280 K960 act2", bf16=True)      # 0.003 (0.0029)
    add(g("t3-sk", "t3", 3, 257, 136, 320, splitk=4, **F32), "mixed emb_layers(all) M8 N9600 K3840 sk3", bf16=True)      # 0.00063 / 0.0013 (0.00066 / 0.00099)
    add(g("t3-sk-silu", "t3", 3, 257, 136, 320, splitk=4, act=IC.SILU, **F32), "mixed time_embed.2 M8 N1280 K3840 sk5 act2", bf16=True)      # 0.0007 / 0.0011 (0.00074 / 0.0012)
    add(g("t3-r32", "t3", 3, 257, 136, 64, **_opts(F32, R32)), "mixed attn.out M2048 N1280 K1280")      # 0.0043
    add(g("t3-r32-sk", "t3", 3, 257, 136, 320, splitk=4, **_opts(F32, R32)), "robust ff.out M2048 N1280 K15360 sk3; high st.proj_out sk3, ldc > N", bf16=True, ldcN=(0, 1))      # 0.00072 / 0.0013 (0.00072 / 0.0013)
    add(g("t3-r32-gnp", "t3", 3, 256, 136, 64, **_opts(F32, R32, GNP)), "mixed st.proj_out M2048 N1280 K1280 gnp")      # 0.0042 / 0.0036
    add(g("t3-r32-gnp-sk128", "t3", 3, 256, 160, 320, splitk=4, **_opts(F32, R32, GNP)), "robust st.proj_out M2048 N1280 K3840 sk3 gnp", bf16=True)      # 0.00071 / 0.01 / 0.0015 (0.00069 / 0.01 / 0.0013)
    add(g("t3-r32-gnp-sk64", "t3", 3, 256, 160, 320, splitk=4, slot=64, **_opts(F32, R32, GNP)), "robust st.proj_out M512 N1280 K3840 sk5 gnp", bf16=True)      # 0.00068 / 0.022 / 0.0013 (0.00069 / 0.023 / 0.0013)
    add(g("t3-r32-m16-gnp", "t3", 3, 256, 136, 64, **_opts(F32, R32, GNP, M16)), "mixed st.proj_out M2048 N1280 K1280 gnp m16")      # 0.0039 / 0.0037
    add(g("t3-r32-m16", "t3", 3, 257, 136, 64, **_opts(F32, R32, M16)), "mixed st.proj_out M2048 N1280 K1280 m16, ldc > N", ldcN=(1,))      # 0.0044
    add(g("t3-r32-m16-sk", "t3", 3, 257, 136, 320, splitk=4, **_opts(F32, R32, M16)), "robust st.proj_out M2048 N1280 K3840 sk3 m16, ldc > N", ldcN=(1,))      # 0.00071 / 0.0013
    add(g("t3-o16-r32-sk", "t3", 3, 257, 136, 320, splitk=4, bias_n=True, **R32), "mixed ff.out M2048 N1280 K5120 sk3 (16-bit output, fp32 residual)")      # 0.45 / 0.26
    # ---- tile 3, convolutions: N = 8, and stride 2 on an odd-sized source (17 x 17 with the VAE's pad (0, 1, 0, 1), 15 x 15 with pad 1:
    # 8 x 8 outputs, four images = 256 rows = four 64-row slots); 9 K-tiles in 2 splits of 5 / 4 and in 6 of 2 / 2 / 2 / 2 / 1 / 0
    add(cv("t3-conv-n8", "t3", 3, 2, 12, 20, 64, 8, **F32), "mixed unet.out_conv M32768 N8 K8640", bf16=True)      # 0.0005 (0.00048)
    add(cv("t3-s2-gnp", "t3", 3, 4, 17, 17, 64, 136, stride=2, pad=0, **_opts(F32, GNP)), "mixed vae.downsample M524288 N128 K3456 s2", bf16=True)      # 0.00068 / 0.004 (0.00063 / 0.0038)
    add(cv("t3-s2-gnp-sk128", "t3", 3, 4, 15, 15, 64, 160, stride=2, splitk=2, **_opts(F32, GNP)), "high downsample M8192 N320 K8640 s2 sk2", bf16=True)      # 0.00045 / 0.011 / 0.00092 (0.00038 / 0.013 / 0.00069)
    add(cv("t3-s2-gnp-sk64", "t3", 3, 4, 15, 15, 64, 160, stride=2, splitk=6, slot=64, **_opts(F32, GNP)), "mixed downsample M512 N1280 K11520 s2 sk6", bf16=True)      # 0.00033 / 0.023 / 0.00062 (0.00027 / 0.036 / 0.00062)
    add(cv("t3-s2-m16-gnp-sk128", "t3", 3, 4, 15, 15, 64, 160, stride=2, splitk=2, **_opts(F32, GNP, M16)), "mixed downsample M8192 N320 K2880 s2 sk2 m16")      # 0.00045 / 0.012 / 0.0007
    add(cv("t3-s2-m16-gnp-sk64", "t3", 3, 4, 15, 15, 64, 160, stride=2, splitk=6, slot=64, **_opts(F32, GNP, M16)), "mixed downsample M512 N1280 K11520 s2 sk6 m16")      # 0.00032 / 0.03 / 0.00071
    # ---- tile 6: 256 x 256 tiles
    add(g("t6-f32", "t6", 6, 513, 264, 128, **F32), "mixed vae.nin_shortcut M524288 N256 K1536", bf16=True)      # 0.0028 (0.0033)
    add(g("t6-z", "t6", 6, 513, 264, 128, Z=2, **F32), "high vae.attn.vT M512 N4096 K1536 Z8", bf16=True)      # 0.0033 (0.0032)
    add(g("t6-r32-gnp", "t6", 6, 512, 264, 64, **_opts(F32, R32, GNP)), "high vae.attn.proj_out M32768 N512 K1536 gnp", bf16=True)      # 0.0049 / 0.0053 (0.0043 / 0.0053)
    add(cv("t6-s2-gnp", "t6", 6, 8, 17, 17, 64, 264, stride=2, pad=0, **_opts(F32, GNP)), "mixed vae.downsample M131072 N256 K6912 s2", bf16=True)      # 0.0008 / 0.005 (0.00071 / 0.0051)
    # ---- tile 8: 128 x 160 tiles
    add(g("t8-f32", "t8", 8, 257, 168, 128, **F32), "mixed zero_conv M32768 N320 K320", bf16=True)      # 0.0032 (0.0029)
    add(g("t8-2w", "t8", 8, 257, 168, 256, a_wrap=True, **F32), "mixed res.skip1x1 M8192 N640 K640 2w")      # 0.0014
    add(g("t8-r32", "t8", 8, 257, 168, 64, **_opts(F32, R32)), "mixed attn.out M32768 N320 K320; high st.proj_out M8192 N640, ldc > N", bf16=True, ldcN=(0, 1))      # 0.0049 (0.0042)
    add(g("t8-r32-gnp", "t8", 8, 256, 168, 64, **_opts(F32, R32, GNP)), "mixed st.proj_out M32768 N320 K320 gnp", bf16=True)      # 0.0042 / 0.0057 (0.0041 / 0.0064)
    add(g("t8-r32-m16-gnp", "t8", 8, 256, 168, 64, **_opts(F32, R32, GNP, M16)), "mixed st.proj_out M32768 N320 K320 gnp m16")      # 0.005 / 0.0052
    add(g("t8-r32-m16", "t8", 8, 257, 168, 64, **_opts(F32, R32, M16)), "mixed st.proj_out M8192 N640 K640 m16, ldc > N", ldcN=(1,))      # 0.004
    add(g("t8-o16-r32", "t8", 8, 257, 168, 64, bias_n=True, **R32), "mixed ff.out M32768 N320 K1280 (16-bit output, fp32 residual)")      # 0.48
    # ---- tiles 1 and 14: the narrow ends of the VAE and conv_in's 24 (3 x 8) input channels
    add(g("t1-f32-n8-k24", "t1", 1, 257, 8, 24, **F32), "mixed vae.quant_conv M32768 N8 K24", bf16=True)      # 0.016 (0.012)
    add(cv("t1-conv-gnp", "t1", 1, 2, 16, 16, 24, 136, **_opts(F32, GNP)), "mixed conv_in M32768 N320 K216 gnp", bf16=True)      # 0.0019 / 0.0043 (0.0023 / 0.0044)
    add(cv("t1-conv-m16-gnp", "t1", 1, 2, 16, 16, 24, 136, **_opts(F32, GNP, M16)), "mixed conv_in M32768 N320 K216 gnp m16")      # 0.0018 / 0.004
    add(cv("t14-conv-n8", "t14", 14, 2, 12, 20, 64, 8, **F32), "mixed vae.conv_out M2097152 N8 K3456", bf16=True)      # 0.00052 (0.00065)
    # ---- real parts of an fp32 tensor, one cell per format: bf16 [hi | lo | hi], fp16 [hi | lo], fp16 [hi | lo | hi]
    add(g("split-bf16x3", "split", 3, 257, 136, 192, split=3, **F32), "F32S operand (edtr_split_operand)", dtypes=("bf16",), extra="a real hi / lo split, bf16 x 3")      # (0.0019)
    add(g("split-fp16x2", "split", 3, 257, 136, 128, split=2, **F32), "F32H[2] operand", dtypes=("fp16",), extra="a real hi / lo split, fp16 x 2")      # 0.0053
    add(g("split-fp16x3", "split", 3, 257, 136, 192, split=3, **F32), "F32H[3] operand", dtypes=("fp16",), extra="a real hi / lo split, fp16 x 3")      # 0.0021
    # ---- what the planner must refuse (no launch)
    ref = dict(expect=E_UNSUPPORTED)
    add(g("refuse-2w-t6", "refuse", 6, 257, 264, 256, a_wrap=True, **F32, **ref), "a_wrap on the 256 x 256 tile")
    add(g("refuse-slot64-unsplit", "refuse", 3, 256, 160, 320, slot=64, **_opts(F32, GNP), **ref), "64-row slots without split-K")
    add(g("refuse-gnp-ragged-m", "refuse", 3, 257, 136, 64, **_opts(F32, GNP), **ref), "statistics of a ragged M")
    add(g("refuse-gnp-sk-n-not-32", "refuse", 3, 256, 136, 320, splitk=4, **_opts(F32, GNP), **ref), "the reducer's statistics need N % 32 == 0")
    add(g("refuse-m16-of-16-bit-out", "refuse", 3, 257, 136, 64, bias_n=True, **M16, **ref), "a mirror of a 16-bit output")
    add(cv("refuse-t17-sk", "refuse", 17, *U, 128, 128, splitk=2, **F32, **ref), "split-K on tile 17")
    add(cv("refuse-t20-gnin", "refuse", 20, 1, 16, 32, 64, 160, a_gn=True, **F32, **ref), "a_gn on tile 20")
    add(cv("refuse-t16-gnin-img8", "refuse", 16, 8, 8, 8, 128, 128, a_gn=True, **F32, **ref), "a_gn on the 8 x 8-image form")
    add(cv("refuse-t16-sk-above-chunks", "refuse", 16, *P, 64, 128, splitk=2, **F32, **ref), "more splits than 64-channel chunks")
    add(cv("refuse-t14-gnp-sk", "refuse", 14, 4, 15, 15, 64, 32, stride=2, splitk=2, **_opts(F32, GNP), **ref), "the reducer's statistics behind tile 14")
    return out


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)
LAUNCHED = [c for c in CELLS if c.cell.expect > 0]
RUNS = [(c, dt) for c in LAUNCHED for dt in c.dtypes]
RUN_IDS = [f"{c.name}-{dt}" for c, dt in RUNS]


# ---- buffers ------------------------------------------------------------------------------------------------------------------------------------
def _view(buf, sl, z=0):
    return buf.as_strided((sl.rows, sl.cols), (sl.ld, 1), sl.offs[z])


def kred(c):
    """The reduction length of one output element: 4 C1 in the sub-pixel form (four 2 x 2 convolutions), K otherwise."""
    return 4 * c.s["cin"] if IC.phases(c) == 4 else IC.dims(c)[2]


class Case:
    """One cell in one dtype on the host: layout, operands, the poisoned input buffers, the reference."""

    def __init__(self, sc, dtype):
        c = self.c = sc.cell
        self.sc, self.dtype = sc, dtype
        self.f, self.ptrs, self.slabs = IC.layout(c, {torch.bfloat16: 0, torch.float16: 1}[dtype])
        self.ops = IC.operands(c, dtype)
        self.out_dtype = torch.float32 if c.o.get("out_f32") else dtype
        self.M, self.N, self.K = IC.dims(c)
        self.No = IC.n_out(c)
        self.types = {"a": dtype, "w": dtype, "res": torch.float32 if c.o.get("res_f32") else dtype, "out": self.out_dtype, "out16": dtype,
                      "gnp": torch.float32}
        self.inputs = {}
        dense = {"a": self.ops["a"], "w": self.ops["w"]}
        if "res" in self.ops:
            dense["res"] = self.ops["res"][None]
        for k, t in dense.items():
            buf = torch.full((self.slabs[k].numel,), NAN, dtype=self.types[k])
            for z in range(t.shape[0]):
                _view(buf, self.slabs[k], z).copy_(t[z])
            self.inputs[k] = buf
        self.vecs = {k: self.ops[v] for k, v in (("bias_n", "bias_n"), ("bias_m", "bias_m"), ("rowvec", "rowvec"), ("a_gn", "gn_table")) if v in self.ops}
        self.splitk = c.o.get("splitk", 0)
        self.ws_guard = 8 * self.N      # floats behind the [splitk][M][N] slabs

    def new_outputs(self, splitk=True):
        outs = {k: torch.full((self.slabs[k].numel,), NAN, dtype=self.types[k]) for k in ("out", "out16", "gnp") if k in self.slabs}
        if splitk and self.splitk > 1:
            outs["ws"] = torch.full((self.splitk * self.M * self.N + self.ws_guard,), NAN, dtype=torch.float32)
        return outs

    @functools.cached_property
    def reference(self):
        """(ref, absref, extra) in fp64, [Z, M, n]."""
        return reference_of(self)

    @functools.cached_property
    def slot_rows(self):
        return slot_rows(self.c)


@functools.lru_cache(maxsize=None)
def case(name, dt):
    return Case(BY_NAME[name], DT[dt])


def reference_of(cs, d=None):
    d = cs.ops if d is None else d
    ref, ab = IC.reference(cs.c, d)
    extra = None
    if "gn_table" in d:      # a normalised value within the fp32 arithmetic's reach of a 16-bit rounding boundary may land one spacing away
        from swin_cases import gn_apply16
        s, t = cs.c.s, d["gn_table"]
        flip = gn_apply16(d["a"].float().reshape(s["B"], -1, s["cin"]), t[:, None, :, 0], t[:, None, :, 1], cs.dtype)[1]
        flip = flip.reshape(s["B"], s["H"], s["W"], s["cin"]).permute(0, 3, 1, 2)
        w = d["w"][0].double().reshape(-1, 3, 3, s["cin"]).permute(0, 3, 1, 2).abs()
        extra = {"16-bit normalised operand, boundary values": F.conv2d(flip, w, padding=1).permute(0, 2, 3, 1).reshape(1, cs.M, cs.N)}
    return ref, ab, extra


def slot_rows(c):
    """The output rows behind every gn_partial slot, as the kernels fill them (include/edtr_hip.h: `which rows a slot covers is the kernel's
    business`): the split-K reducer and the row-major tiles take consecutive rows; a halo tile puts a whole unit (a 16 x 16 patch, four 8 x 8
    images, a 32 x 16 or 16 x 16 unit; in the sub-pixel form the 16 x 16 pixels of one phase of a 32 x 32 block) into the unit's first slot
    and zeros into its others (an empty list here)."""
    M, o, s = IC.dims(c)[0], c.o, c.s
    sk = o.get("splitk", 0) > 1
    sr = (o.get("slot") or 128) if sk else 128
    t = c.expect
    if sk or t not in HALO_UNIT:
        return [torch.arange(i * sr, (i + 1) * sr) for i in range(M // sr)]
    per, rows = HALO_SLOTS[t], []
    empty = [torch.empty(0, dtype=torch.long)] * (per - 1)
    oh, ow = IC.out_hw(s)
    if t == 16 and oh == 8 and ow == 8:
        for u in range(M // 256):
            rows += [torch.arange(u * 256, (u + 1) * 256)] + empty
        return rows
    uh, uw = HALO_UNIT[t]
    i, j = torch.meshgrid(torch.arange(uh), torch.arange(uw), indexing="ij")
    for img in range(s["B"]):
        if s["ups"] == 2:
            for ty in range(s["H"] // 16):
                for tx in range(s["W"] // 16):
                    for ph in range(4):
                        r = (img * oh + 32 * ty + (ph >> 1) + 2 * i) * ow + 32 * tx + (ph & 1) + 2 * j
                        rows += [r.reshape(-1)] + empty
        else:
            for ty in range(oh // uh):
                for tx in range(ow // uw):
                    rows += [((img * oh + ty * uh + i) * ow + tx * uw + j).reshape(-1)] + empty
    assert len(rows) == M // 128
    return rows


# ---- the checks of a finished launch ------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def read_guarded(buf, sl, what):
    """[Z, rows, cols] of the slab's slices: every slice finite, every other element of the buffer still NaN."""
    host = buf.clone()
    got = torch.stack([_view(host, sl, z).clone() for z in range(len(sl.offs))])
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values in the valid region (a poisoned row, column or slot was read, or an element never written)"
    for z in range(len(sl.offs)):
        _view(host, sl, z).fill_(NAN)
    assert bool(torch.isnan(host).all()), f"{what}: a store landed outside the views (guard rows, guard columns or the guard slot)"
    return got


def judge(cs, outs, inputs=None):
    """Every check of one finished launch, on host tensors: `outs` = {"out"[, "out16", "gnp", "ws"]: the flat buffers after the launch},
    `inputs` = the operand buffers after it.  Returns {"out": worst element ratio[, "stats": worst slot ratio]}; raises AssertionError."""
    c, fig = cs.c, {}
    for k, buf in (inputs or {}).items():
        assert torch.equal(_bits(buf), _bits(cs.inputs[k])), f"operand {k} (or its guards) changed"
    got = read_guarded(outs["out"], cs.slabs["out"], "out")
    ref, ab, extra = cs.reference
    r, where = elem_ratio(got, ref, ab, cs.out_dtype, kred(c), extra)
    fig["out"] = r
    assert r <= 1.0, f"{cs.sc.name}: element bound exceeded: ratio {r:.3g} at {where}"
    if "out16" in cs.slabs:
        mir = read_guarded(outs["out16"], cs.slabs["out16"], "out16")
        assert torch.equal(_bits(mir), _bits(got.to(cs.dtype))), "the mirror is not the stored fp32 output rounded once"
    if "gnp" in cs.slabs:
        assert cs.out_dtype == torch.float32 and got.shape[0] == 1
        st = read_guarded(outs["gnp"], cs.slabs["gnp"], "gn_partial")[0].reshape(-1, cs.N, 2).double()
        o64, worst = got[0].double(), 0.0
        assert len(cs.slot_rows) == st.shape[0]
        for i, rows in enumerate(cs.slot_rows):
            if rows.numel() == 0:
                assert bool((st[i] == 0).all()), f"slot {i} of a halo unit holds something: the unit's first slot takes the sums, the others zeros"
                continue
            v = o64[rows]
            for j, (want, absw) in enumerate(((v.sum(0), v.abs().sum(0)), ((v * v).sum(0), (v * v).sum(0)))):
                rr, wh = elem_ratio(st[i, :, j], want, absw, torch.float32, rows.numel())
                worst = max(worst, rr)
                assert rr <= 1.0, f"{cs.sc.name}: statistics slot {i} ({('sum', 'sum of squares')[j]}): ratio {rr:.3g} at {wh}"
        fig["stats"] = worst
    if "ws" in outs:
        n = cs.splitk * cs.M * cs.N
        assert bool(torch.isnan(outs["ws"][n:]).all()), "a store landed behind the split-K workspace"
        assert bool(torch.isfinite(outs["ws"][:n]).all()), "a slab element was not written (an empty split writes zeros)"
    return fig


def same_as_unsplit(cs, out_split, out_plain):
    """The split-K result against the unsplit launch of the same cell, within the element bound (the unsplit output as `ref`)."""
    a = read_guarded(out_split, cs.slabs["out"], "out")
    b = read_guarded(out_plain, cs.slabs["out"], "unsplit out")
    r, where = elem_ratio(a, b, cs.reference[1], cs.out_dtype, kred(cs.c), cs.reference[2])
    assert r <= 1.0, f"{cs.sc.name}: split-K differs from the unsplit launch: ratio {r:.3g} at {where}"
    return r


# ---- a perfect kernel on the host, and the defects ----------------------------------------------------------------------------------------------
DEFECTS = {
    "res16": "the residual rounded to 16 bits before the add",
    "res_ldc": "the residual indexed with ldc instead of ldr",
    "mirror_pre": "the mirror rounded from the value before the residual",
    "slot_unwritten": "one statistics slot left unwritten",
    "slot128": "statistics summed over 128 rows where the slot is 64",
    "ring_part": "one part's columns read as zero in the outermost halo ring only",
    "out_ld16": "out stored with ld16",
}


def res16_visible(sc, dt):
    """Whether the element bound can see the residual rounded to the operand type: median rounding error 2^-12.5 |res| (fp16; 2^-9.5 bf16)
    against K 2^-22 |res| — a ratio of 724 / K (5792 / K) in the limit of a large residual; asserted where that is >= 8."""
    return bool(sc.cell.o.get("out_f32")) and (724.0 if dt == "fp16" else 5792.0) / kred(sc.cell) >= 8.0


def applies(sc, defect):
    c, o = sc.cell, sc.cell.o
    if c.expect <= 0:
        return False
    return {"res16": bool(o.get("res_f32")), "res_ldc": bool(o.get("res_f32")), "mirror_pre": bool(o.get("out16") and o.get("res_f32")),
            "slot_unwritten": bool(o.get("gnp")), "slot128": bool(o.get("gnp") and o.get("slot") == 64),
            "ring_part": bool(o.get("parts") and c.expect in HALO_UNIT and not c.s["ups"] and IC.out_hw(c.s) != (8, 8)),
            "out_ld16": bool(o.get("out16"))}[defect]


def _ring_delta(cs, part=1):
    """What part `part`'s columns of the pixels OUTSIDE a unit (its halo ring) add to the unit's outputs: the full convolution of those
    columns minus the convolution of every unit on its own with zeros around it."""
    c, s = cs.c, cs.c.s
    assert not c.o.get("act") and c.o.get("alpha", 1.0) == 1.0
    width = s["cin"] // c.o["parts"]
    a = torch.zeros_like(cs.ops["a"], dtype=torch.float64)
    a[..., part * width:(part + 1) * width] = cs.ops["a"][..., part * width:(part + 1) * width].double()
    w = cs.ops["w"][0].double().reshape(-1, 3, 3, s["cin"]).permute(0, 3, 1, 2)
    x = a[0].reshape(s["B"], s["H"], s["W"], s["cin"]).permute(0, 3, 1, 2)
    full = F.conv2d(x, w, padding=1)
    uh, uw = HALO_UNIT[c.expect]
    B, C, H, W = x.shape
    xu = x.reshape(B, C, H // uh, uh, W // uw, uw).permute(0, 2, 4, 1, 3, 5).reshape(-1, C, uh, uw)
    own = F.conv2d(xu, w, padding=1).reshape(B, H // uh, W // uw, -1, uh, uw).permute(0, 3, 1, 4, 2, 5).reshape(B, -1, H, W)
    return (full - own).permute(0, 2, 3, 1).reshape(1, cs.M, cs.N)


def _scatter(buf, values, ld, off=0):
    """values[m][n] -> buf[off + m ld + n]; what falls behind the buffer is dropped."""
    M, N = values.shape
    idx = off + torch.arange(M)[:, None] * ld + torch.arange(N)[None, :]
    ok = idx < buf.numel()
    buf[idx[ok]] = values[ok]


def simulate(cs, defect=None):
    """What a kernel that computes the fp64 reference and rounds once would leave in the output buffers; with a defect, that kernel's bug."""
    c, o = cs.c, cs.c.o
    ref = cs.reference[0]
    res = cs.ops.get("res")
    if defect == "res16":
        ref = ref - res.double() + res.to(cs.dtype).double()
    elif defect == "res_ldc":
        idx = torch.arange(cs.M)[:, None] * cs.f["ldc"] + torch.arange(cs.No)[None, :]
        buf = cs.inputs["res"]
        wrong = torch.where(idx < buf.numel(), buf[idx.clamp(max=buf.numel() - 1)], torch.full((), NAN))
        ref = ref - res.double() + wrong.double()
    elif defect == "ring_part":
        ref = ref - _ring_delta(cs)
    outs = cs.new_outputs()
    got = ref.to(cs.out_dtype)
    sl = cs.slabs["out"]
    for z in range(got.shape[0]):
        _scatter(outs["out"], got[z], cs.f["ld16"] if defect == "out_ld16" else sl.ld, sl.offs[z])
    if "out16" in outs:
        pre = (ref - res.double()).to(cs.out_dtype) if defect == "mirror_pre" else got
        _view(outs["out16"], cs.slabs["out16"]).copy_(pre[0].to(cs.dtype))
    if "gnp" in outs:
        st = _view(outs["gnp"], cs.slabs["gnp"]).reshape(-1, cs.N, 2)
        o64 = got[0].double()
        last = max(i for i, rows in enumerate(cs.slot_rows) if rows.numel())
        for i, rows in enumerate(cs.slot_rows):
            if defect == "slot128":
                rows = torch.arange(128 * (i // 2), 128 * (i // 2) + 128)
            if defect == "slot_unwritten" and i == last:
                continue
            v = o64[rows]
            st[i, :, 0], st[i, :, 1] = v.sum(0).float(), (v * v).sum(0).float()
    if "ws" in outs:
        outs["ws"][:cs.splitk * cs.M * cs.N] = 0.0
    return outs
