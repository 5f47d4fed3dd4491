"""Per-kernel tests of the 16-bit layout, elementwise and normalisation kernels that every network launches between its GEMMs (run on
the MI355X box: pytest -m gpu): nchw_to_nhwc / nhwc_to_nchw, add (16-bit and fp32 stream), add_stats, split3 / split_operand,
timestep_embedding, embed_tokens, zero_bytes (csrc/elementwise.hip) and softmax_rows, layernorm, gn_stats + gn_apply (csrc/norm.hip).
Conventions of tests/test_gpu_glue.py: every call goes through edtr_amd.ops.make_* and ops.launch; a kernel that only moves, adds once
in fp32 or rounds is compared bit for bit with that statement in torch, every other output element with an fp64 reference of the exact
values the kernel reads (tests/glue16_reference.py) through edtr_amd.testing.elem_ratio.  The bounds follow from the arithmetic, they
are not measured.  Every destination is a view inside a larger buffer — NaN around pure stores, a finite pattern around partial writes
— and everything outside the written region must stay bit-unchanged; every source pad column that must not be read holds NaN.  Each
grid-stride loop has one case above its span (4096 x 256 units; 1024 x 256 for zero_bytes).  The shapes are the smallest that reach the
line in question: the second channel pass of the transposes (C > 64), the flat-cast form (B = C = ld = 1), LayerNorm's fourth vector
slot (C = 2048) and single live lane (C = 8), the generic loop of gn_apply (C = 96, 960), gn_stats' unrolled loop followed by its tail
(C = 128, HW = 5000), softmax with cols_pad = ld as the VAE attention passes it.  Emitter.add never passes `out` aliasing `a` (nets.py,
model/cldm.py: always a fresh tensor or a slice of another buffer), so no in-place add is tested.  tests/test_glue16_bound.py shows on
the CPU which defects these checks reject."""
import os

import pytest
import torch

import glue16_reference as R
from edtr_amd.testing import block_rel, elem_ratio, unit_roundoff

pytestmark = pytest.mark.gpu

F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
PAD = 64                        # guard elements in front of and behind every destination
PATTERN = 0x5A3C                # bit pattern of a pre-filled 16-bit destination (a finite value in both formats)
SENTINEL = 12345.678            # pre-filled fp32 / fp64 destinations
GRID_SPAN = R.GRID_SPAN
NAN = float("nan")


def _ops():
    from edtr_amd import ops
    return ops


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


ELEM = {}          # kernel -> worst element ratio measured in this file (0 = bit-exact comparisons only; printed by the last test; EDTR_GLUE16_ERRLOG=path dumps it)


def elem(kernel, got, ref, absref, k, out_dtype, extra=None):
    """Assert the rounding-aware element bound (edtr_amd/testing.py): |got - ref| <= 2u|ref| + k 2^-22 absref + extra everywhere."""
    r, where = elem_ratio(got, ref, absref, out_dtype, k, extra)
    ELEM[kernel] = max(ELEM.get(kernel, 0.0), r)
    print(f"[{kernel}] worst element ratio {r:.3f}")
    assert r <= 1.0, f"{kernel}: element bound exceeded: ratio {r:.3g} at {where}"
    return r


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def exact(kernel, got, want):
    """Bit-exact comparison (recorded as ratio 0 / inf so that the summary lists the kernel)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got), bits(want)
    ok = torch.equal(g, w)
    ELEM[kernel] = max(ELEM.get(kernel, 0.0), 0.0 if ok else float("inf"))
    if not ok:
        bad = (g != w).nonzero()
        raise AssertionError(f"{kernel}: {len(bad)} elements differ bitwise, first at {bad[0].tolist()}: "
                             f"{got.cpu()[tuple(bad[0])]} vs {want.cpu()[tuple(bad[0])]}")


def filled(n, dtype, fill):
    """Host tensor of n elements: NaN (fill "nan": around pure stores) or a finite pattern (fill "pattern": around partial writes)."""
    if fill == "nan":
        return torch.full((n,), NAN, dtype=dtype)
    if dtype in DTYPES:
        return torch.full((n,), PATTERN, dtype=torch.int16).view(dtype)
    return torch.full((n,), SENTINEL, dtype=dtype)


def window(rows, ld, dtype, d, fill, extra_rows=2):
    """A [rows + extra_rows, ld] view PAD elements inside a flat pre-filled buffer.  Returns (buffer, view, host copy before)."""
    n = (rows + extra_rows) * ld
    host = filled(n + 2 * PAD, dtype, fill)
    buf = host.to(d)
    return buf, buf[PAD:PAD + n].view(rows + extra_rows, ld), host


def untouched(buf, before, written):
    """Everything of `buf` outside the written region equals `before` bit for bit.  `written`: bool mask over the view's elements."""
    a, b = bits(buf), bits(before)
    mask = torch.ones(a.shape, dtype=torch.bool)
    mask[PAD:PAD + written.numel()] = ~written.reshape(-1)
    assert torch.equal(a[mask], b[mask]), f"{int((a[mask] != b[mask]).sum())} elements outside the written region changed"


def region(view, rows, c0, c1):
    m = torch.zeros(view.shape, dtype=torch.bool)
    m[:rows, c0:c1] = True
    return m


def in_nan_columns(x, ld, d, col0=0):
    """x [rows, C] as the column slice [col0, col0 + C) of a [rows, ld] device buffer whose other columns hold NaN."""
    host = torch.full((x.shape[0], ld), NAN, dtype=x.dtype)
    host[:, col0:col0 + x.shape[1]] = x
    return host.to(d)[:, col0:col0 + x.shape[1]]


# =====================================================================================================================================
# 1. nchw_to_nhwc
# =====================================================================================================================================
def _to_nhwc(dtype, out_dtype, src, ld, coff, pad_to, scale, shift, d):
    """Launch into a pattern-filled [B HW + 2, ld] window; checks the zeroed pad columns and everything outside
    [coff, coff + cpad); returns the [B, HW, C] result on the host."""
    ops = _ops()
    B, C, HW = src.shape
    cpad = max(C, pad_to)
    buf, win, before = window(B * HW, ld, out_dtype, d, "pattern")
    ops.launch(ops.make_nchw_to_nhwc(dtype=dtype, src=src.to(d), B=B, C=C, HW=HW, dst=win, ld=ld, coff=coff, zero_pad_to=pad_to,
                                     scale=scale, shift=shift))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, B * HW, coff, coff + cpad))
    got = win[:B * HW].cpu()
    if cpad > C:
        assert torch.equal(bits(got[:, coff + C:coff + cpad]), torch.zeros((B * HW, cpad - C), dtype=bits(got).dtype)), "pad columns are not +0"
    return got[:, coff:coff + C].reshape(B, HW, C)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nchw_to_nhwc_second_channel_pass_and_zeroed_pad(dtype):
    """C = 70 > 64: the c0 loop's second pass with a ragged tail of 6 channels; pad columns 70-71 zeroed; columns 72-79 of ld = 80
    and the rows beyond keep the pattern.  HW = 130: three pixel tiles, the last of 2.  k = 2: one product and one sum (or one fma)."""
    d = dev()
    src = rnd((2, 70, 130), 1000)
    got = _to_nhwc(dtype, dtype, src, 80, 0, 72, 0.7, -0.3, d)
    ref, absref = R.nchw_to_nhwc_ref(src, 0.7, -0.3)
    elem("nchw_to_nhwc", got, ref, absref, 2, dtype)
    got = _to_nhwc(dtype, dtype, src, 80, 0, 72, 1.0, 0.0, d)           # identity: a transposed rounding
    exact("nchw_to_nhwc", got, src.permute(0, 2, 1).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW", [1, 63, 64, 65])
def test_nchw_to_nhwc_pixel_tile_edges(dtype, HW):
    """C = 3 into columns 3-5 (+ a zeroed column 6) of ld = 8: one pixel, one short of a tile, a whole tile, one more."""
    d = dev()
    src = rnd((2, 3, HW), 1010 + HW)
    got = _to_nhwc(dtype, dtype, src, 8, 3, 4, 1.0, 0.0, d)
    exact("nchw_to_nhwc", got, src.permute(0, 2, 1).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nchw_to_nhwc_flat_cast_form(dtype):
    """What Emitter.cast_flat launches: B = 1, C = 1, ld = 1, HW = n — an fp32 -> 16-bit cast of n = 4099 contiguous elements."""
    d = dev()
    src = rnd((1, 1, 4099), 1020) * 3
    got = _to_nhwc(dtype, dtype, src, 1, 0, 0, 1.0, 0.0, d)
    exact("nchw_to_nhwc", got, src.permute(0, 2, 1).to(dtype))


@pytest.mark.parametrize("code", ["f32_split", "f32_h2"])
def test_nchw_to_nhwc_fp32_destination(code):
    """The fp32-stream codes keep the NHWC activation fp32: same geometry as the 16-bit case, columns 4-75 of ld = 80."""
    ops, d = _ops(), dev()
    assert code in (ops.F32S, ops.F32H[2])
    src = rnd((2, 70, 130), 1030)
    got = _to_nhwc(code, F32, src, 80, 4, 72, 0.7, -0.3, d)
    ref, absref = R.nchw_to_nhwc_ref(src, 0.7, -0.3)
    elem("nchw_to_nhwc[f32]", got, ref, absref, 2, F32)
    got = _to_nhwc(code, F32, src, 80, 4, 72, 1.0, 0.0, d)
    exact("nchw_to_nhwc[f32]", got, src.permute(0, 2, 1).contiguous())


# =====================================================================================================================================
# 2. nhwc_to_nchw
# =====================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src_f32", [False, True])
@pytest.mark.parametrize("B,C,ld,HW", [(2, 70, 72, 130), (1, 1, 1, 4099)])      # second channel pass; the flat form of model/clip.py
def test_nhwc_to_nchw(dtype, src_f32, B, C, ld, HW):
    """Source columns >= C hold NaN; the dense fp32 destination sits between NaN guards.  One fp32 product per element."""
    ops, d = _ops(), dev()
    scale = 0.3
    x = rnd((B * HW, C), 1100 + C)
    x = x if src_f32 else x.to(dtype)
    src = in_nan_columns(x, ld, d)
    buf, win, before = window(B * C, HW, F32, d, "nan", extra_rows=0)
    ops.launch(ops.make_nhwc_to_nchw(dtype=dtype, src=src, src_f32=src_f32, B=B, C=C, HW=HW, ld=ld, dst=win, scale=scale))
    torch.cuda.synchronize()
    exact("nhwc_to_nchw", win.cpu().reshape(B, C, HW), R.nhwc_to_nchw_exact(x.reshape(B, HW, C), C, scale))
    untouched(buf, before, region(win, B * C, 0, HW))


# =====================================================================================================================================
# 3. add (16-bit, fp32 stream), add_stats
# =====================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_b", [True, False])
def test_add16_grid_stride_with_three_row_strides(dtype, with_b):
    """rows = 4100, C = 2056: 1 053 700 eight-wide vectors (> 4096 x 256) with lda = 2064, ldb = 2072, ldo = 2080."""
    ops, d = _ops(), dev()
    rows, C, lda, ldb, ldo = 4100, 2056, 2064, 2072, 2080
    assert rows * C // 8 > GRID_SPAN
    a, b = rnd((rows, C), 1200).to(dtype), (rnd((rows, C), 1201).to(dtype) if with_b else None)
    buf, win, before = window(rows, ldo, dtype, d, "pattern", extra_rows=1)
    ops.launch(ops.make_add(dtype=dtype, a=in_nan_columns(a, lda, d), lda=lda, b=in_nan_columns(b, ldb, d) if with_b else None,
                            ldb=ldb if with_b else 0, out=win[:, 16:], ldo=ldo, rows=rows, C=C))
    torch.cuda.synchronize()
    exact("add", win[:rows, 16:16 + C].cpu(), R.add16_exact(a, b, dtype))
    untouched(buf, before, region(win, rows, 16, 16 + C))


@pytest.mark.parametrize("with_b", [True, False])
def test_add_f32_stream_grid_stride(with_b):
    """C = 12 (a multiple of 4, not of 8): the four-wide fp32 kernel; rows x 3 = 1 048 800 vectors (> 4096 x 256)."""
    ops, d = _ops(), dev()
    rows, C, lda, ldb, ldo = 349600, 12, 16, 20, 24
    assert rows * C // 4 > GRID_SPAN and C & 3 == 0 and C & 7
    a, b = rnd((rows, C), 1210), (rnd((rows, C), 1211) if with_b else None)
    buf, win, before = window(rows, ldo, F32, d, "pattern", extra_rows=1)
    ops.launch(ops.make_add(dtype=ops.F32S, a=in_nan_columns(a, lda, d), lda=lda, b=in_nan_columns(b, ldb, d, 4) if with_b else None,
                            ldb=ldb if with_b else 0, out=win[:, 8:], ldo=ldo, rows=rows, C=C))
    torch.cuda.synchronize()
    exact("add[f32]", win[:rows, 8:8 + C].cpu(), a + b if with_b else a)
    untouched(buf, before, region(win, rows, 8, 8 + C))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slot_rows", [64, 128])
@pytest.mark.parametrize("C", [32, 96])
@pytest.mark.parametrize("with_b", [True, False])
def test_add_stats_partials_against_their_own_reference(dtype, slot_rows, C, with_b):
    """Three slots; gn_partial is the column slice [32, 32 + C) of a slot buffer with gn_ld = C + 64 and a fourth slot, sentinels
    everywhere else.  Partials: fp64 column sums / sums of squares of the fp32 value a + b; k = slot_rows additions (and products)."""
    ops, d = _ops(), dev()
    slots, gn_ld, col = 3, C + 64, 32
    rows = slots * slot_rows
    a = (rnd((rows, C), 1300) + 0.5).to(dtype)
    b = (rnd((rows, C), 1301) * 0.5 - 0.2).to(dtype) if with_b else None
    obuf, owin, o_before = window(rows, C + 24, dtype, d, "pattern")
    gbuf, gwin, g_before = window(slots, gn_ld * 2, F32, d, "pattern", extra_rows=1)
    ops.launch(ops.make_add_stats(dtype=dtype, a=in_nan_columns(a, C + 8, d), lda=C + 8, b=in_nan_columns(b, C + 16, d, 8) if with_b else None,
                                  ldb=C + 16 if with_b else 0, out=owin[:, 8:], ldo=C + 24, rows=rows, C=C,
                                  gn_partial=gwin.reshape(-1)[2 * col:], gn_ld=gn_ld, slot_rows=slot_rows))
    torch.cuda.synchronize()
    exact("add_stats", owin[:rows, 8:8 + C].cpu(), R.add16_exact(a, b, dtype))
    untouched(obuf, o_before, region(owin, rows, 8, 8 + C))
    sums, absr = R.add_stats_ref(a, b, slot_rows)
    elem("add_stats", gwin[:slots, 2 * col:2 * (col + C)].cpu().reshape(slots, C, 2), sums, absr, slot_rows, F32)
    untouched(gbuf, g_before, region(gwin, slots, 2 * col, 2 * (col + C)))


# =====================================================================================================================================
# 4. split3 / split_operand (bit-exact against the torch restatement of tests/test_gpu_mixed.py)
# =====================================================================================================================================
SRC_DTYPES = {"f32": F32, "f16": torch.float16, "bf16": torch.bfloat16}


def _split(kernel, x, ld_src, dt, order, d, launch):
    """x [rows, C] as a NaN-padded slice with row stride ld_src; the operand lands in a pattern-filled window of ld = parts C + 8."""
    rows, C = x.shape
    parts = len(order)
    buf, win, before = window(rows, parts * C + 8, dt, d, "pattern", extra_rows=1)
    launch(in_nan_columns(x, ld_src, d), win[:, :parts * C])
    torch.cuda.synchronize()
    exact(kernel, win[:rows, :parts * C].cpu(), R.parts_exact(x, dt, order))
    untouched(buf, before, region(win, rows, 0, parts * C))


@pytest.mark.parametrize("src", ["f32", "f16", "bf16"])
def test_split_strided_source(src):
    """ld_src = C + 8 > C (NaN in the source's pad columns): both split-3 patterns and every operand format."""
    ops, d = _ops(), dev()
    x = (rnd((301, 200), 1400) * 3).to(SRC_DTYPES[src])
    for pattern, order in ((0, "hlh"), (1, "hhl")):
        _split("split3", x, 208, torch.bfloat16, order, d,
               lambda s, o: ops.launch(ops.make_split3(src=s, rows=301, C=200, dst=o, pattern=pattern)))
    for fmt, dt, order in ((ops.F32S, torch.bfloat16, "hlh"), (ops.F32H[1], torch.float16, "h"), (ops.F32H[2], torch.float16, "hl"),
                           (ops.F32H[3], torch.float16, "hlh")):
        _split("split_operand", x, 208, dt, order, d,
               lambda s, o: ops.launch(ops.make_split_operand(src=s, rows=301, C=200, dst=o, fmt=fmt)))


@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_split3_grid_stride(src):
    """rows = 4100, C = 2048: 1 049 600 eight-wide vectors (> 4096 x 256)."""
    ops, d = _ops(), dev()
    rows, C = 4100, 2048
    assert rows * C // 8 > GRID_SPAN
    x = rnd((rows, C), 1410).to(SRC_DTYPES[src])
    pattern = 1 if src == "f32" else 0
    _split("split3", x, C, torch.bfloat16, "hhl" if pattern else "hlh", d,
           lambda s, o: ops.launch(ops.make_split3(src=s, rows=rows, C=C, dst=o, pattern=pattern)))


@pytest.mark.parametrize("src", ["f32", "f16"])
def test_split_operand_grid_stride(src):
    ops, d = _ops(), dev()
    rows, C = 4100, 2048
    assert rows * C // 8 > GRID_SPAN
    x = rnd((rows, C), 1420).to(SRC_DTYPES[src])
    parts = 1 if src == "f32" else 2
    _split("split_operand", x, C, torch.float16, "hl"[:parts], d,
           lambda s, o: ops.launch(ops.make_split_operand(src=s, rows=rows, C=C, dst=o, fmt=ops.F32H[parts])))


# =====================================================================================================================================
# 5. timestep embedding, token embedding, zero_bytes
# =====================================================================================================================================
def _temb(dtype, out_dtype, t, dim, d):
    ops = _ops()
    B, ld = t.numel(), dim + 8
    buf, win, before = window(B, ld, out_dtype, d, "pattern")
    ops.launch(ops.make_timestep_embedding(dtype=dtype, t=t.to(d), B=B, dim=dim, out=win, ld=ld))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, B, 0, dim))
    return win[:B, :dim].cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [2, 64, 1280])                  # 1280: half = 640 > 256 threads, the loop's second and third trips
def test_timestep_embedding(dtype, dim):
    """t = 0, 1, 999 into rows of ld = dim + 8.  t = 0: cos exactly 1, sin exactly 0."""
    d = dev()
    t = torch.tensor([0, 1, 999], dtype=torch.int64)
    got = _temb(dtype, dtype, t, dim, d)
    ref, arg_err = R.temb_ref(t, dim)
    elem("timestep_embedding", got, ref, None, 0, dtype, extra={"fp32 argument": arg_err})
    exact("timestep_embedding", got[0], torch.cat([torch.ones(dim // 2), torch.zeros(dim // 2)]).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_timestep_embedding_single_image(dtype):
    d = dev()
    t = torch.tensor([437], dtype=torch.int64)
    ref, arg_err = R.temb_ref(t, 64)
    elem("timestep_embedding", _temb(dtype, dtype, t, 64, d), ref, None, 0, dtype, extra={"fp32 argument": arg_err})


def test_timestep_embedding_fp32_output():
    ops, d = _ops(), dev()
    t = torch.tensor([0, 1, 999], dtype=torch.int64)
    got = _temb(ops.F32S, F32, t, 1280, d)
    ref, arg_err = R.temb_ref(t, 1280)
    elem("timestep_embedding[f32]", got, ref, None, 0, F32, extra={"fp32 argument": arg_err})
    exact("timestep_embedding[f32]", got[0], torch.cat([torch.ones(640), torch.zeros(640)]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_tokens_grid_stride_and_clamped_ids(dtype):
    """rows = 108 x 77, D = 1024: 1 064 448 eight-wide vectors (> 4096 x 256); ids from -5 to 69 against a vocabulary of 64."""
    ops, d = _ops(), dev()
    B, L, D, vocab, ld = 108, 77, 1024, 64, 1032
    rows = B * L
    assert rows * D // 8 > GRID_SPAN
    table, pos = rnd((vocab, D), 1500), rnd((L, D), 1501)
    tokens = torch.randint(-5, vocab + 6, (rows,), generator=torch.Generator().manual_seed(1502))
    tokens[:4] = torch.tensor([-1, vocab, 0, vocab - 1])
    buf, win, before = window(rows, ld, dtype, d, "pattern", extra_rows=1)
    ops.launch(ops.make_embed_tokens(dtype=dtype, tokens=tokens.to(d), table=table.to(d), pos=pos.to(d), rows=rows, L_ctx=L, D=D, out=win, ld=ld))
    torch.cuda.synchronize()
    exact("embed_tokens", win[:rows, :D].cpu(), R.embed_tokens_exact(tokens, table, pos, dtype))
    untouched(buf, before, region(win, rows, 0, D))


@pytest.mark.parametrize("n16", [1, R.ZERO_SPAN + 777])            # 16 bytes; the second trip of the 1024 x 256-unit loop
def test_zero_bytes(n16):
    ops, d = _ops(), dev()
    buf, win, before = window(n16, 8, torch.bfloat16, d, "pattern", extra_rows=0)
    ops.launch(ops.make_zero(win))
    torch.cuda.synchronize()
    exact("zero_bytes", win.cpu(), torch.zeros((n16, 8), dtype=torch.bfloat16))
    untouched(buf, before, region(win, n16, 0, 8))


# =====================================================================================================================================
# 6. softmax_rows
# =====================================================================================================================================
def _softmax_rows(case):
    """The live columns of the score rows of a case."""
    if case == "pad8":          # rows = 5, cols = 132 in ld = 136
        return rnd((5, 132), 1600) * 3
    if case == "cols4":
        return rnd((3, 4), 1601) * 3
    if case == "cols1028":      # thread 0 owns a second vector (columns 1024-1027)
        return rnd((3, 1028), 1602) * 3
    if case == "one_row":
        return rnd((1, 132), 1603) * 3
    assert case == "rescale"
    s = torch.full((3, 1028), -80.0)
    s[0, 1026] = 80.0                                      # the row's only large value sits in the last vector: every thread but one
    s[1] = rnd((1028,), 1604)                              # rescales its (max, sum) in the merge, thread 0 inside its own loop
    s[1, 1025] = 12.0
    s[2] = rnd((1028,), 1605)
    s[2, 1] = 12.0                                         # ... and the other way round: the first vector holds the maximum
    return s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["pad8", "cols4", "cols1028", "one_row", "rescale"])
def test_softmax_rows_padded_as_the_vae_attention_passes_it(dtype, case):
    """ld_s = ld_p = cols_pad = round_up(cols, 8) (nets.py: the P V GEMM reads the pad columns of P and relies on exact zeros).
    The pad of s holds NaN (never read), the pad of P must be +0, the rows and guards beyond stay NaN.  Bound: the one
    test_softmax_rows states, elem(p, ref, ref, dtype, cols), plus the named terms of glue16_reference.softmax_ref."""
    ops, d = _ops(), dev()
    s = _softmax_rows(case)
    rows, cols = s.shape
    ld = cols + 8 - cols % 8                              # round_up(cols, 8): every case here has cols % 8 == 4
    buf, win, before = window(rows, ld, dtype, d, "nan")
    ops.launch(ops.make_softmax_rows(dtype=dtype, s=in_nan_columns(s, ld, d), rows=rows, cols=cols, ld_s=ld, p=win, ld_p=ld, cols_pad=ld))
    torch.cuda.synchronize()
    got = win[:rows].cpu()
    ref, extra = R.softmax_ref(s)
    elem("softmax_rows", got[:, :cols], ref, ref, cols, dtype, extra)
    assert torch.equal(bits(got[:, cols:]), torch.zeros((rows, ld - cols), dtype=torch.int16)), "pad columns of P are not +0"
    untouched(buf, before, region(win, rows, 0, ld))
    if case == "rescale":
        assert float(got[0, 1026]) == 1.0 and float(got[0].float().sum()) == 1.0


# =====================================================================================================================================
# 7. layernorm
# =====================================================================================================================================
def _layernorm(dtype, x, d):
    """x [rows, C] 16-bit with ldx = C + 8 (NaN row tails), y in a pattern-filled window with ldy = C + 16."""
    ops = _ops()
    rows, C = x.shape
    gamma, beta = 1 + 0.1 * rnd((C,), 1700), 0.1 * rnd((C,), 1701)
    buf, win, before = window(rows, C + 16, dtype, d, "pattern")
    ops.launch(ops.make_layernorm(dtype=dtype, x=in_nan_columns(x, C + 8, d), rows=rows, C=C, ldx=C + 8, gamma=gamma.to(d), beta=beta.to(d),
                                  eps=1e-5, y=win[:, 8:], ldy=C + 16))
    torch.cuda.synchronize()
    ref, absref = R.norm_ref(x, gamma, beta, 1e-5)
    elem("layernorm", win[:rows, 8:8 + C].cpu(), ref, absref, C, dtype)
    untouched(buf, before, region(win, rows, 8, 8 + C))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [2048, 8])                 # the fourth vector slot (C > 1536); one live lane
@pytest.mark.parametrize("rows", [1, 2, 3])              # fewer rows than the workgroup's four waves
def test_layernorm_row_strides_and_slot_edges(dtype, C, rows):
    _layernorm(dtype, (rnd((rows, C), 1710 + rows) * 1.5 + 0.3).to(dtype), dev())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [2048, 72])
def test_layernorm_rows_offset_by_16_standard_deviations(dtype, C):
    """mean = 16 sigma: a one-pass variance would lose 2 x 8 bits to the cancellation; the kernel is two-pass, so norm_ref's bound
    holds unchanged."""
    _layernorm(dtype, (rnd((3, C), 1720) * 0.5 + 8.0).to(dtype), dev())


# =====================================================================================================================================
# 8. groupnorm: gn_stats + gn_apply against fp64 directly
# =====================================================================================================================================
def _groupnorm(dtype, B, HW, C, d, silu=True, eps=1e-5, x=None, strided=True, in_place=False, sums_zeroed=False, seed=1800):
    """x as columns [16, 16 + C) of a NaN-filled buffer with ldx = C + 32, y as columns [8, 8 + C) of a pattern-filled window with
    ldy = C + 8 (strided), or both dense; in_place: y = x (the strided x buffer).  The fp64 sums sit between sentinels."""
    ops = _ops()
    rows = B * HW
    if x is None:
        x = (rnd((rows, C), seed) * 2 + 0.7).to(dtype)
    gamma, beta = 1 + 0.1 * rnd((C,), seed + 1), 0.1 * rnd((C,), seed + 2)
    ldx, ldy, xo, yo = (C + 32, C + 8, 16, 8) if strided else (C, C, 0, 0)
    if in_place:
        buf, win, _ = window(rows, ldx, dtype, d, "nan")
        win[:rows, xo:xo + C] = x.to(d)
        before = buf.cpu().clone()
        xv = yv = win[:, xo:]
        ldy, yo = ldx, xo
    else:
        buf, win, before = window(rows, ldy, dtype, d, "pattern")
        xv, yv = in_nan_columns(x, ldx, d, xo), win[:, yo:]
    sbuf, swin, s_before = window(B, 64, torch.float64, d, "pattern", extra_rows=1)
    if sums_zeroed:
        swin[:B].zero_()
        s_before = sbuf.cpu().clone()
    st, ap = ops.make_gn(dtype=dtype, x=xv, ldx=ldx, B=B, HW=HW, C=C, sums=swin, gamma=gamma.to(d), beta=beta.to(d), eps=eps, silu=silu,
                         y=yv, ldy=ldy, sums_zeroed=sums_zeroed)
    ops.launch(st)
    ops.launch(ap)
    torch.cuda.synchronize()
    cpg = C // 32
    sums, abs_sums = R.gn_sums_ref(x, B, HW, C)
    elem("gn_stats", swin[:B].cpu().reshape(B, 32, 2), sums, abs_sums, HW * cpg, F32)      # fp32 partial sums, folded in fp64
    untouched(sbuf, s_before, region(swin, B, 0, 64))
    ref, absref = R.norm_ref(R.gn_groups(x, B, HW, C), R.gn_affine(gamma, HW, C), R.gn_affine(beta, HW, C), eps, silu)
    got = R.gn_groups(win[:rows, yo:yo + C].cpu(), B, HW, C)
    elem("gn_apply", got, ref, absref, HW * cpg, dtype)
    if HW * cpg > 4096:         # norm_elem's limitation: the per-block check at 1.25 u catches what the worst-case k term hides
        v = block_rel(got.float().reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]), got.shape[-1])
        ELEM["gn_apply[block / 1.25u]"] = max(ELEM.get("gn_apply[block / 1.25u]", 0.0), v / (1.25 * unit_roundoff(dtype)))
        assert v <= 1.25 * unit_roundoff(dtype), f"per-block error {v:.3g}"
    untouched(buf, before, region(win, rows, yo, yo + C))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C", [(2, 70, 96), (2, 70, 960),      # the generic apply loop: 12 vectors; 3 x 32 and a 24-vector tail chunk
                                    (3, 70, 96), (2, 1, 96), (1, 1, 960)])
def test_groupnorm_generic_apply_loop_in_column_slices(dtype, B, HW, C):
    _groupnorm(dtype, B, HW, C, dev())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("HW,C", [(43013, 96), (5637, 960)])
def test_groupnorm_generic_apply_loop_beyond_its_first_load_slot(dtype, HW, C):
    """A workgroup of the generic loop holds four loads of 256 vectors in flight; at the small shapes above only the first is live.
    B = 1 and HW above 2048 / channel chunks x 21 (11) pixels give workgroups of 22 x 12 = 264 (12 x 24 = 288) vectors: the second
    slot, ragged.  Groups of 129 039 (169 110) elements: the element bound is wide there, the per-block check is not."""
    _groupnorm(dtype, 1, HW, C, dev(), seed=1840)


@pytest.mark.parametrize("dtype", DTYPES)
def test_groupnorm_stats_unrolled_loop_then_tail(dtype):
    """C = 128, HW = 5000, B = 1: 64 chunks of 79 pixels, 16 pixel rows in flight — one trip of the 4-deep loop (64 pixels), then
    the tail (15 more); the last chunk has 23 pixels."""
    _groupnorm(dtype, 1, 5000, 128, dev(), silu=False, eps=1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [96, 128])
def test_groupnorm_in_place_and_sums_already_zeroed(dtype, C):
    d = dev()
    _groupnorm(dtype, 2, 70, C, d, in_place=True, seed=1810)
    _groupnorm(dtype, 2, 70, C, d, sums_zeroed=True, seed=1820)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [96, 128])
def test_groupnorm_groups_offset_by_16_standard_deviations(dtype, C):
    """mean = 16 sigma.  The sums are fp32 per workgroup and fp64 across them, the variance is E[x^2] - mean^2 in fp64: norm_ref's
    bound (whose absref carries rstd^2 E[x^2]) must hold unchanged."""
    x = (rnd((2 * 70, C), 1830) * 0.5 + 8.0).to(dtype)
    _groupnorm(dtype, 2, 70, C, dev(), x=x)


def test_zz_glue16_worst_ratios():
    """Bookkeeping (runs last in this file): the worst element ratio each kernel measured (0 = bit-exact comparisons only)."""
    import json
    print("\n[16-bit glue kernels: worst element ratio] " + "; ".join(f"{k}: {v:.3f}" for k, v in sorted(ELEM.items())))
    path = os.environ.get("EDTR_GLUE16_ERRLOG")
    if path:
        with open(path, "w") as f:
            json.dump(ELEM, f, indent=1)
