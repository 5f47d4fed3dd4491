"""The six MFMA kernels of csrc/swin.hip at their edges (run on the MI355X box: pytest -m gpu): edtr_window_attn, edtr_swin_mlp,
edtr_swin_attn, edtr_swin_layer, edtr_conv64 and edtr_conv128_out.  Conventions of tests/test_gpu_glue16.py: every call goes through
edtr_amd.ops.make_* and ops.launch; every destination is a view PAD elements inside a pre-filled flat buffer with two extra rows
and a row stride 8 elements wider than the written width (200 for the 192-column rows, 80 for conv64's 64; the fp32 NCHW planes are
followed by two guard rows), and everything outside the written region must stay bit-unchanged; every 16-bit source has another
row stride than the destination (208, 72, 136; 3 heads 32 + 16 for the packed qkv) and NaN behind its real width.  Columns 180 to
191 of x are zero and come out exactly zero.  Element checks use edtr_amd.testing.elem_ratio <= 1 with the bounds
tests/test_gpu_ops.py derives (tests/swin_cases.py states them once); the attention half keeps that file's per-block check
BLOCK_TOL["swin_attn"] on the same operand distribution.  tests/test_swin_edges_cpu.py shows on the CPU which defects these checks
reject.  Which case reaches which line of swin.hip:
  window_attn   thin_shift1 / thin_shift7: shifts 1 and 7 (:40-42 the longest wrap, :115 the thinnest mask regions), 18 tasks: the
                last workgroup's waves 2, 3 return (:30).  narrow_heads: d = 6, c_pad = 16: of the store's four register groups only
                g = 0 passes :179 / :181, and only in part; the pad zeroing (:186) starts at column 12.  sharp_logits: logits of
                about +-60 at shift 7: a masked key holds the raw row maximum (:115 before :126-131).
  swin_mlp      one_row: rows = 1, every tile row clamps to row 0 (:258), one store passes :465.  one_live_row_in_last_workgroup:
                rows = 129.  no_pad_columns: c_valid = 192 (:320), all 384 hidden units real.  extreme_rows: |mean| = 16 std and an
                all-zero row through the one-pass variance and its clamp (:322).  row_stats (:442-449) against the documented
                layout.  in place: out == x (:258 reads, :465 stores the workgroup's own rows).
  swin_attn     shift1 / shift7_one_window_per_image (:527-530 wrap on both axes; three windows: workgroup 0 owns windows of two
                images, workgroup 1 one window, :548 / :560 clamp, :842 skips), full_width_heads: head_dim 32, c_valid 192.
  swin_layer    the same cases, bit for bit against the two launches, with every field of the MLP record the header calls ignored
                set to NULL / 0 (swin_mlp_body<T, true> must not touch them).
  conv64        fp32 NCHW planes over three persistent rounds: the counted wait :949 (wait_vm<1>) with n_valid = 1 (one store
                instruction per patch) and n_valid = 4, both patch buffers reused (:953-954), a ragged last round (:952).  16-bit
                NHWC behind upsample2x with B = 3 over two rounds: the source index b * SH (:923).
  conv128_out   three rounds with per-image tables: the table reload :1066 and its index b, n_valid = 4 and 1 (:1141);
                gn_table = NULL on the same geometry.
  rejections    every return before the launch of the six entry points (:1180-1350)."""
import os

import pytest
import torch

import swin_cases as SC
from swin_cases import DTYPES, F32, LD_OUT, LD_OUT64, LD_X, LD_X64, LD_X128, bits, in_nan_columns, region, untouched, window
from edtr_amd.testing import block_rel, elem_ratio

pytestmark = pytest.mark.gpu
CP = SC.CP


def _ops():
    from edtr_amd import ops
    return ops


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


ELEM = {}          # kernel -> worst element ratio measured in this file (0 = bit-exact comparisons only; printed by the last test; EDTR_SWIN_EDGES_ERRLOG=path dumps it)
BLOCK = {}         # dtype -> worst per-block error of the attention half


def elem(kernel, got, ref, absref, k, out_dtype, extra=None):
    """Assert the rounding-aware element bound (edtr_amd/testing.py): |got - ref| <= 2u|ref| + k 2^-22 absref + extra everywhere."""
    r, where = elem_ratio(got, ref, absref, out_dtype, k, extra)
    ELEM[kernel] = max(ELEM.get(kernel, 0.0), r)
    print(f"[{kernel}] worst element ratio {r:.3f}")
    assert r <= 1.0, f"{kernel}: element bound exceeded: ratio {r:.3g} at {where}"
    return r


def exact(kernel, got, want):
    """Bit-exact comparison (recorded as ratio 0 / inf so that the summary lists the kernel)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got), bits(want)
    ok = torch.equal(g, w)
    ELEM[kernel] = max(ELEM.get(kernel, 0.0), 0.0 if ok else float("inf"))
    if not ok:
        bad = (g != w).nonzero()
        raise AssertionError(f"{kernel}: {len(bad)} elements differ bitwise, first at {bad[0].tolist()}")


def zero_columns(got, c0):
    """Columns c0 .. of the 16-bit rows are +0 bit for bit."""
    assert c0 == got.shape[1] or bool((bits(got[:, c0:]) == 0).all()), "pad columns are not +0"


def labels(H, W, shift, d):
    from edtr_amd.model import swinir as S
    return torch.from_numpy(S.region_labels(H, W, 8, shift)).to(d) if shift else None


# =====================================================================================================================================
# 1. edtr_window_attn
# =====================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SC.WINDOW_CASES))
def test_window_attn_thin_shifts_narrow_heads_sharp_logits(dtype, case):
    ops, d = _ops(), dev()
    B, H, W, heads, hd, cp, shift, q_scale = SC.WINDOW_CASES[case]
    rows, C = B * H * W, heads * hd
    qkv, bias = SC.window_qkv(B, H, W, heads, hd, dtype, q_scale)
    assert bool(torch.isfinite(qkv.float()).all())
    ld_qkv, ld_out = 3 * heads * 32 + 16, cp + 8
    src = in_nan_columns(SC.pack_window_qkv(qkv), ld_qkv, d)
    buf, win, before = window(rows, ld_out, dtype, d, "nan")
    ops.launch(ops.make_window_attn(dtype=dtype, qkv=src, ld_qkv=ld_qkv, out=win, ld_out=ld_out, B=B, H=H, W=W, heads=heads, head_dim=hd,
                                    c_pad=cp, shift=shift, bias=bias.to(d), labels=labels(H, W, shift, d), scale=hd ** -0.5))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, rows, 0, cp))
    got = win[:rows, :cp].cpu()
    ref, pv, k, extra = SC.window_elem(qkv, bias, H, W, heads, hd, shift, hd ** -0.5, dtype)
    if case == "sharp_logits":
        lg = SC.window_logits(qkv, H, W, heads, hd, shift)
        assert float(lg.max()) > 50.0 and float(lg.min()) < -50.0, "the logits of this case are meant to reach about +-60"
    elem("window_attn", got[:, :C].float(), ref, pv, k, dtype, extra)
    zero_columns(got, C)


# =====================================================================================================================================
# 2. edtr_swin_mlp
# =====================================================================================================================================
def _mlp_launch(dtype, x, P, d, in_place=False, with_stats=True):
    """Launch into guarded windows; checks the guards; returns (stored [rows, 192] 16-bit on the host, row_stats [rows, 6, 2] or None)."""
    ops = _ops()
    rows, C = x.shape[0], P["C"]
    img1, img2 = ops.pack_swin_mlp_weights(P["w1g"], P["w2p"], dtype)
    buf, win, before = window(rows, LD_OUT, dtype, d, "nan")
    if in_place:
        win[:rows, :CP] = x.to(d)
        src, ldx = win, LD_OUT
    else:
        src, ldx = in_nan_columns(x, LD_X, d), LD_X
    sbuf, swin, sbefore = window(rows, 2 * CP // 32, F32, d, "nan")
    ops.launch(ops.make_swin_mlp(dtype=dtype, x=src, ldx=ldx, rows=rows, c_valid=C, eps=1e-5, w1=img1.to(d), w2=img2.to(d), c1=P["c1"].to(d),
                                 c2b=P["c2b"].to(d), b2=P["b2p"].to(d), out=win, ldo=LD_OUT, row_stats=swin if with_stats else None))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, rows, 0, CP))
    untouched(sbuf, sbefore, region(swin, rows if with_stats else 0, 0, 2 * CP // 32))
    return win[:rows, :CP].cpu(), (swin[:rows].cpu().reshape(rows, CP // 32, 2) if with_stats else None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SC.MLP_CASES))
def test_swin_mlp_row_counts_full_width_extreme_rows(dtype, case):
    d = dev()
    rows, C, HID, kind = SC.MLP_CASES[case]
    P = SC.mlp_operands(dtype, C, HID)
    x = SC.mlp_rows(rows, C, dtype, kind=kind)
    stored, stats = _mlp_launch(dtype, x, P, d)
    ref64, abs64, k, extra = SC.mlp_mirror(x, P, dtype)
    elem("swin_mlp", stored[:, :C].float(), ref64, abs64, k, dtype, extra)
    zero_columns(stored, C)
    r, zeros = SC.row_stats_ratio(stats, stored)
    ELEM["swin_mlp.row_stats"] = max(ELEM.get("swin_mlp.row_stats", 0.0), r)
    print(f"[swin_mlp.row_stats] worst ratio {r:.3f}")
    assert r <= 1.0, f"row_stats: slots 0 / 3 are not the sums of the stored columns 0..95 / 96..191: ratio {r:.3g}"
    assert zeros, "row_stats: slots 1, 2, 4, 5 are not +0"


@pytest.mark.parametrize("dtype", DTYPES)
def test_swin_mlp_in_place_gives_the_bits_of_the_out_of_place_launch(dtype):
    d = dev()
    P = SC.mlp_operands(dtype)
    x = SC.mlp_rows(129, 180, dtype)
    apart, _ = _mlp_launch(dtype, x, P, d, with_stats=False)
    onto, _ = _mlp_launch(dtype, x, P, d, in_place=True, with_stats=False)
    exact("swin_mlp.in_place", onto, apart)


# =====================================================================================================================================
# 3. edtr_swin_attn and edtr_swin_layer
# =====================================================================================================================================
def _attn_rec(dtype, x_dev, ldx, out, ldo, P, B, H, W, shift, d):
    ops = _ops()
    img_qkv, img_proj = ops.pack_swin_attn_weights(P["wg"], P["wpp"], dtype)
    return ops.make_swin_attn(dtype=dtype, x=x_dev, ldx=ldx, out=out, ldo=ldo, B=B, H=H, W=W, head_dim=P["d"], shift=shift, c_valid=P["C"],
                              eps=1e-5, wqkv=img_qkv.to(d), wproj=img_proj.to(d), c1=P["c1"].to(d), c2b=P["c2b"].to(d), bproj=P["bpp"].to(d),
                              bias=ops.swin_attn_bias(P["bias"]).to(d), labels=labels(H, W, shift, d))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SC.ATTN_CASES))
def test_swin_attn_thin_shifts_and_full_width_heads(dtype, case):
    ops, d = _ops(), dev()
    B, H, W, shift, C = SC.ATTN_CASES[case]
    rows = B * H * W
    P = SC.attn_operands(dtype, C)
    x = SC.attn_rows(rows, C, dtype)
    buf, win, before = window(rows, LD_OUT, dtype, d, "nan")
    ops.launch(_attn_rec(dtype, in_nan_columns(x, LD_X, d), LD_X, win, LD_OUT, P, B, H, W, shift, d))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, rows, 0, CP))
    got = win[:rows, :CP].cpu()
    assert bool(torch.isfinite(got.float()).all())
    v = block_rel(got[:, :C].float(), SC.attn_mirror(x, P, B, H, W, shift, dtype), C)
    tol = SC.BLOCK_TOL_SWIN_ATTN[0 if dtype == torch.bfloat16 else 1]
    BLOCK[dtype] = max(BLOCK.get(dtype, 0.0), v)
    print(f"[swin_attn] {case} {dtype}: worst 32 x 32 block {v:.3g} (tolerance {tol})")
    assert v <= tol, f"per-block error {v:.3g} above {tol} (swin_attn, {case})"
    zero_columns(got, C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SC.ATTN_CASES))
def test_swin_layer_is_the_two_launches_and_ignores_what_the_header_calls_ignored(dtype, case):
    ops, d = _ops(), dev()
    B, H, W, shift, C = SC.ATTN_CASES[case]
    rows = B * H * W
    PA, PM = SC.attn_operands(dtype, C), SC.mlp_operands(dtype, C, 2 * C)
    x = in_nan_columns(SC.attn_rows(rows, C, dtype), LD_X, d)
    img1, img2 = (t.to(d) for t in ops.pack_swin_mlp_weights(PM["w1g"], PM["w2p"], dtype))

    def mlp_rec(src, ldx, out, ldo):
        return ops.make_swin_mlp(dtype=dtype, x=src, ldx=ldx, rows=rows, c_valid=C, eps=1e-5, w1=img1, w2=img2, c1=PM["c1"].to(d),
                                 c2b=PM["c2b"].to(d), b2=PM["b2p"].to(d), out=out, ldo=ldo)
    ld1 = LD_X + 8                                                         # the half-way rows: a destination, then a source
    buf1, x1, before1 = window(rows, ld1, dtype, d, "nan")
    buf2, two, before2 = window(rows, LD_OUT, dtype, d, "nan")
    ops.launch(_attn_rec(dtype, x, LD_X, x1, ld1, PA, B, H, W, shift, d))
    ops.launch(mlp_rec(x1, ld1, two, LD_OUT))
    buf, one, before = window(rows, LD_OUT, dtype, d, "nan")
    m = mlp_rec(x1, ld1, two, LD_OUT)
    pm = m.keep[0]
    pm.x, pm.out, pm.row_stats, pm.rows, pm.ldx, pm.ldo = None, None, None, 0, 0, 0
    ops.launch(ops.make_swin_layer(_attn_rec(dtype, x, LD_X, one, LD_OUT, PA, B, H, W, shift, d), m))
    torch.cuda.synchronize()
    for b, bf, w in ((buf1, before1, x1), (buf2, before2, two), (buf, before, one)):
        untouched(b, bf, region(w, rows, 0, CP))
    got = one[:rows, :CP].cpu()
    assert bool(torch.isfinite(got.float()).all())
    exact("swin_layer", got, two[:rows, :CP].cpu())
    zero_columns(got, C)


# =====================================================================================================================================
# 4. edtr_conv64
# =====================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_valid,alpha,slope", [(1, 0.7, None), (4, 1.0, 0.2)])
def test_conv64_fp32_planes_over_three_persistent_rounds(dtype, n_valid, alpha, slope):
    from edtr_amd import lib as L
    ops, d = _ops(), dev()
    B, E = SC.PERSISTENT_B, SC.persistent_edge(cus(), 3)
    SC.check_persistent(B, E, E, cus(), 3)
    x, w, bias = SC.conv64_operands(B, E, E, n_valid, dtype)
    buf, win, before = window(B * n_valid * E, E, F32, d, "nan")
    ops.launch(ops.make_conv64(dtype=dtype, x=in_nan_columns(x.reshape(-1, 64), LD_X64, d), ldx=LD_X64, w=ops.pack_conv64_weight(w, dtype).to(d),
                               bias=bias.to(d), out=win, B=B, H=E, W=E, act=L.ACT_NONE if slope is None else L.ACT_LRELU, act_slope=slope or 0.0,
                               alpha=alpha, ldo=0, out_nchw_f32=True, n_valid=n_valid))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, B * n_valid * E, 0, E))
    r64, a64 = SC.conv64_reference(x, w, bias, dtype, alpha, slope, False)        # (n_valid output channels only)
    elem("conv64", win[:B * n_valid * E].cpu().reshape(B, n_valid, E, E), r64, a64, 576, F32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv64_upsample_of_three_images_over_two_persistent_rounds(dtype):
    from edtr_amd import lib as L
    ops, d = _ops(), dev()
    B, E = SC.PERSISTENT_B, SC.persistent_edge(cus(), 2)
    SC.check_persistent(B, E, E, cus(), 2)
    x, w, bias = SC.conv64_operands(B, E // 2, E // 2, 64, dtype)
    rows = B * E * E
    buf, win, before = window(rows, LD_OUT64, dtype, d, "nan")
    ops.launch(ops.make_conv64(dtype=dtype, x=in_nan_columns(x.reshape(-1, 64), LD_X64, d), ldx=LD_X64, w=ops.pack_conv64_weight(w, dtype).to(d),
                               bias=bias.to(d), out=win, B=B, H=E, W=E, upsample2x=True, act=L.ACT_LRELU, act_slope=0.2, alpha=1.0, ldo=LD_OUT64))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, rows, 0, 64))
    r64, a64 = SC.conv64_reference(x, w, bias, dtype, 1.0, 0.2, True)
    elem("conv64", win[:rows, :64].float().cpu().reshape(B, E, E, 64).permute(0, 3, 1, 2), r64, a64, 576, dtype)


# =====================================================================================================================================
# 5. edtr_conv128_out
# =====================================================================================================================================
_C128 = {}         # dtype -> the shared operands, device table and references of the three-round geometry (computed once, never changed)


def _conv128_shared(dtype, d):
    if dtype not in _C128:
        ops = _ops()
        B, E = SC.PERSISTENT_B, SC.persistent_edge(cus(), 3)
        HW = E * E
        x, w, bias, gamma, beta = SC.conv128_operands(B, HW, dtype, per_image=True)
        xd = in_nan_columns(x, LD_X128, d)
        gamma, beta = gamma.to(d), beta.to(d)
        sums = torch.zeros((B, 32, 2), dtype=torch.float64, device=d)
        st, _ = ops.make_gn(dtype=dtype, x=xd, ldx=LD_X128, B=B, HW=HW, C=128, sums=sums, gamma=gamma, beta=beta, eps=1e-6, silu=True, y=xd,
                            ldy=LD_X128, sums_zeroed=True)
        ops.launch(st)
        table = torch.empty((B, 128, 2), dtype=torch.float32, device=d)
        ops.launch(ops.make_gn_table(partial=None, tiles_per_image=0, sums=sums, B=B, C=128, HW=HW, gamma=gamma, beta=beta, eps=1e-6, table=table))
        torch.cuda.synchronize()
        tb = table.cpu()
        # the tables are what the case needs them to be: the one of the fp64 statistics, and grossly different between the images
        want = SC.gn_table_reference(x, gamma.cpu(), beta.cpu(), 1e-6, B)
        assert float((tb - want).abs().max() / want.abs().max()) < 1e-4
        assert float((tb[0, :, 0] / tb[1, :, 0]).min()) > 2.5 and float((tb[2, :, 0] / tb[0, :, 0]).min()) > 2.5
        _C128[dtype] = dict(B=B, E=E, x=x, xd=xd, w=w, bias=bias, table=table, wimg=ops.pack_conv128_out_weight(w, dtype).to(d),
                            ref=SC.conv128_reference(x, w, bias, dtype, tb, 0.9, B, E, E))
    return _C128[dtype]


def _conv128_launch(dtype, S, n_valid, table, d):
    ops = _ops()
    B, E = S["B"], S["E"]
    SC.check_persistent(B, E, E, cus(), 3)
    buf, win, before = window(B * n_valid * E, E, F32, d, "nan")
    ops.launch(ops.make_conv128_out(dtype=dtype, x=S["xd"], ldx=LD_X128, w=S["wimg"], bias=S["bias"].to(d), out=win, B=B, H=E, W=E,
                                    n_valid=n_valid, gn_table=table, alpha=0.9))
    torch.cuda.synchronize()
    untouched(buf, before, region(win, B * n_valid * E, 0, E))
    return win[:B * n_valid * E].cpu().reshape(B, n_valid, E, E)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_valid", [4, 1])
def test_conv128_out_reloads_each_image_s_table_over_three_rounds(dtype, n_valid):
    d = dev()
    S = _conv128_shared(dtype, d)
    got = _conv128_launch(dtype, S, n_valid, S["table"], d)
    r64, a64, extra = S["ref"]
    elem("conv128_out", got, r64[:, :n_valid], a64[:, :n_valid], 1152, F32, {k: v[:, :n_valid] for k, v in extra.items()})


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv128_out_without_a_table_over_three_rounds(dtype):
    d = dev()
    S = _conv128_shared(dtype, d)
    got = _conv128_launch(dtype, S, 1, None, d)
    r64, a64, _ = SC.conv128_reference(S["x"], S["w"][:1], S["bias"], dtype, None, 0.9, S["B"], S["E"], S["E"])
    elem("conv128_out", got, r64, a64, 1152, F32)


# =====================================================================================================================================
# 6. rejections: the documented code by name, and nothing written
# =====================================================================================================================================
class Reject:
    """Builds a valid record with `make(**overrides)`, lets the test break one thing, asserts the code and, at the end, that no
    destination changed."""

    def __init__(self):
        self.guards = []

    def dest(self, rows, ld, dtype, d):
        buf, win, before = window(rows, ld, dtype, d, "pattern")
        self.guards.append((buf, before, win))
        return win

    def check(self, rec, code, **fields):
        for k, v in fields.items():
            setattr(rec.keep[0], k, v)
        with pytest.raises(RuntimeError, match=rf"EDTR_E_{code}\b"):
            _ops().launch(rec)

    def nothing_written(self):
        torch.cuda.synchronize()
        for buf, before, win in self.guards:
            untouched(buf, before, region(win, 0, 0, 0))


def off_by(t, n):
    """The flat view n elements into t (8 bytes off the 16-byte rule for n = 4 16-bit elements)."""
    return t.reshape(-1)[n:]


def test_window_attn_rejections():
    from edtr_amd import lib as L
    ops, d, R = _ops(), dev(), Reject()
    dtype, B, H, W, heads, hd, cp = torch.float16, 1, 16, 8, 6, 30, 192
    qkv = torch.zeros((B * H * W + 1, 3 * heads * 32 + 16), dtype=dtype, device=d)
    out = R.dest(B * H * W, LD_OUT, dtype, d)
    bias = torch.zeros((heads, 64, 64), device=d)
    lab = torch.zeros((H * W + 16,), dtype=torch.uint8, device=d)

    def make(**kw):
        a = dict(dtype=dtype, qkv=qkv, ld_qkv=qkv.shape[1], out=out, ld_out=LD_OUT, B=B, H=H, W=W, heads=heads, head_dim=hd, c_pad=cp, shift=3,
                 bias=bias, labels=lab, scale=0.18)
        a.update(kw)
        return ops.make_window_attn(**a)
    for kw in (dict(qkv=None), dict(out=None), dict(bias=None), dict(shift=1, labels=None)):
        R.check(make(**kw), "NULL")
    R.check(make(), "DTYPE", dtype=L.F32_SPLIT)
    for kw in (dict(H=12), dict(W=12), dict(heads=0), dict(shift=8), dict(shift=-1), dict(ld_qkv=3 * heads * 32 - 8), dict(c_pad=176), dict(ld_out=184)):
        R.check(make(**kw), "SHAPE")
    for kw in (dict(head_dim=34), dict(head_dim=29)):
        R.check(make(**kw), "UNSUPPORTED")
    for kw in (dict(ld_qkv=qkv.shape[1] + 4), dict(ld_out=LD_OUT - 4), dict(c_pad=190), dict(qkv=off_by(qkv, 4)), dict(out=off_by(out, 4)),
               dict(bias=off_by(bias, 2)), dict(labels=off_by(lab, 4))):
        R.check(make(**kw), "ALIGN")
    R.nothing_written()


def _mlp_reject_setup(R, d, dtype=torch.float16, rows=8):
    ops = _ops()
    t = dict(x=torch.zeros((rows + 1, LD_X), dtype=dtype, device=d), w1=torch.zeros(SC.HP * CP + 8, dtype=dtype, device=d),
             w2=torch.zeros(SC.HP * CP + 8, dtype=dtype, device=d), c1=torch.zeros(SC.HP + 4, device=d), c2b=torch.zeros(SC.HP + 4, device=d),
             b2=torch.zeros(CP + 4, device=d), out=R.dest(rows, LD_OUT, dtype, d), row_stats=R.dest(rows, 12, F32, d))

    def make(**kw):
        a = dict(dtype=dtype, ldx=LD_X, rows=rows, c_valid=180, eps=1e-5, ldo=LD_OUT, **t)
        a.update(kw)
        return ops.make_swin_mlp(**a)
    return t, make


def test_swin_mlp_rejections():
    from edtr_amd import lib as L
    d, R = dev(), Reject()
    t, make = _mlp_reject_setup(R, d)
    for name in ("x", "w1", "w2", "c1", "c2b", "b2", "out"):
        R.check(make(**{name: None}), "NULL")
    R.check(make(), "DTYPE", dtype=L.F32_SPLIT)
    for kw in (dict(rows=0), dict(c_valid=0), dict(c_valid=193), dict(ldx=184), dict(ldo=184)):
        R.check(make(**kw), "SHAPE")
    R.check(make(), "UNSUPPORTED", C=224)
    R.check(make(), "UNSUPPORTED", hidden=352)
    for kw in (dict(ldx=LD_X - 4), dict(ldo=LD_OUT - 4), dict(row_stats=off_by(t["row_stats"], 2))) + tuple({n: off_by(t[n], 4 if t[n].element_size() == 2 else 2)}
                                                                                                       for n in ("x", "w1", "w2", "c1", "c2b", "b2", "out")):
        R.check(make(**kw), "ALIGN")
    R.nothing_written()


def _attn_reject_setup(R, d, dtype=torch.float16, B=1, H=8, W=16):
    ops = _ops()
    rows = B * H * W
    t = dict(x=torch.zeros((rows + 1, LD_X), dtype=dtype, device=d), wqkv=torch.zeros(18 * 6144 + 8, dtype=dtype, device=d),
             wproj=torch.zeros(6 * 6144 + 8, dtype=dtype, device=d), c1=torch.zeros(580, device=d), c2b=torch.zeros(580, device=d),
             bproj=torch.zeros(CP + 4, device=d), bias=torch.zeros(6 * 4096 + 4, device=d), labels=torch.zeros(H * W + 16, dtype=torch.uint8, device=d),
             out=R.dest(rows, LD_OUT, dtype, d))

    def make(**kw):
        a = dict(dtype=dtype, ldx=LD_X, ldo=LD_OUT, B=B, H=H, W=W, head_dim=30, shift=3, c_valid=180, eps=1e-5, **t)
        a.update(kw)
        return ops.make_swin_attn(**a)
    return t, make


ATTN_REJECTIONS = (         # (make overrides, record fields set afterwards, code) for edtr_swin_attn and, on the attention record, edtr_swin_layer
    [(dict([(n, None)]), {}, "NULL") for n in ("x", "wqkv", "wproj", "c1", "c2b", "bproj", "bias", "out")]
    + [(dict(shift=1, labels=None), {}, "NULL"), ({}, dict(dtype=2), "DTYPE"),
       (dict(H=12), {}, "SHAPE"), (dict(W=12), {}, "SHAPE"), (dict(B=0), {}, "SHAPE"), (dict(c_valid=0), {}, "SHAPE"), (dict(c_valid=193), {}, "SHAPE"),
       (dict(shift=8), {}, "SHAPE"), (dict(ldx=184), {}, "SHAPE"), (dict(ldo=184), {}, "SHAPE"),
       ({}, dict(C=224), "UNSUPPORTED"), ({}, dict(heads=4), "UNSUPPORTED"), (dict(head_dim=33), {}, "UNSUPPORTED"), (dict(head_dim=0), {}, "UNSUPPORTED"),
       (dict(ldx=LD_X - 4), {}, "ALIGN"), (dict(ldo=LD_OUT - 4), {}, "ALIGN")])


def _attn_rejections(R, t, make, launchable):
    for kw, fields, code in ATTN_REJECTIONS:
        rec = make(**kw)
        for k, v in fields.items():
            setattr(rec.keep[0], k, v)
        R.check(launchable(rec), code)
    R.check(launchable(make(out=t["x"], ldo=LD_X)), "UNSUPPORTED")                  # x == out: workgroups gather rows others scatter
    for n in ("x", "wqkv", "wproj", "c1", "c2b", "bproj", "bias", "out"):
        R.check(launchable(make(**{n: off_by(t[n], 4 if t[n].element_size() == 2 else 2)})), "ALIGN")
    R.check(launchable(make(labels=off_by(t["labels"], 2))), "ALIGN")


def test_swin_attn_rejections():
    d, R = dev(), Reject()
    t, make = _attn_reject_setup(R, d)
    _attn_rejections(R, t, make, lambda rec: rec)
    R.nothing_written()


def test_swin_layer_rejections():
    ops, d, R = _ops(), dev(), Reject()
    t, make = _attn_reject_setup(R, d)
    tm, make_mlp = _mlp_reject_setup(R, d, rows=128)
    _attn_rejections(R, t, make, lambda rec: ops.make_swin_layer(rec, make_mlp()))
    for name in ("w1", "w2", "c1", "c2b", "b2"):
        R.check(ops.make_swin_layer(make(), make_mlp(**{name: None})), "NULL")
        R.check(ops.make_swin_layer(make(), make_mlp(**{name: off_by(tm[name], 4 if tm[name].element_size() == 2 else 2)})), "ALIGN")
    for fields, code in ((dict(dtype=0), "DTYPE"), (dict(c_valid=192), "SHAPE"), (dict(C=224), "UNSUPPORTED"), (dict(hidden=352), "UNSUPPORTED")):
        m = make_mlp()
        for k, v in fields.items():
            setattr(m.keep[0], k, v)
        R.check(ops.make_swin_layer(make(), m), code)
    R.nothing_written()


def test_conv64_rejections():
    from edtr_amd import lib as L
    ops, d, R = _ops(), dev(), Reject()
    dtype, B, H, W = torch.float16, 1, 16, 32
    t = dict(x=torch.zeros((B * H * W + 1, LD_X64), dtype=dtype, device=d), w=torch.zeros(9 * 4096 + 8, dtype=dtype, device=d),
             bias=torch.zeros(68, device=d), out=R.dest(B * H * W, LD_OUT64, dtype, d))
    planes = R.dest(4 * H, W, F32, d)

    def make(**kw):
        a = dict(dtype=dtype, ldx=LD_X64, B=B, H=H, W=W, act=L.ACT_LRELU, act_slope=0.2, ldo=LD_OUT64, **t)
        a.update(kw)
        return ops.make_conv64(**a)
    for name in t:
        R.check(make(**{name: None}), "NULL")
    R.check(make(), "DTYPE", dtype=L.F32_SPLIT)
    for kw in (dict(H=24), dict(W=24), dict(B=0)):
        R.check(make(**kw), "SHAPE")
    for kw in (dict(act=L.ACT_SILU), dict(act=L.ACT_GELU), dict(out=planes, ldo=0, out_nchw_f32=True, n_valid=0),
               dict(out=planes, ldo=0, out_nchw_f32=True, n_valid=5)):
        R.check(make(**kw), "UNSUPPORTED")
    # (a leading dimension below the width is answered with the leading-dimension code here)
    for kw in (dict(ldx=56), dict(ldx=LD_X64 - 4), dict(ldo=56), dict(ldo=LD_OUT64 - 4), dict(out=off_by(planes, 2), ldo=0, out_nchw_f32=True, n_valid=3)) + tuple(
            {n: off_by(t[n], 4 if t[n].element_size() == 2 else 2)} for n in t):
        R.check(make(**kw), "ALIGN")
    R.nothing_written()


def test_conv128_out_rejections():
    from edtr_amd import lib as L
    ops, d, R = _ops(), dev(), Reject()
    dtype, B, H, W = torch.float16, 1, 16, 32
    t = dict(x=torch.zeros((B * H * W + 1, LD_X128), dtype=dtype, device=d), w=torch.zeros(9 * 4096 + 8, dtype=dtype, device=d),
             bias=torch.zeros(36, device=d), out=R.dest(4 * H, W, F32, d))
    table = torch.zeros(B * 256 + 4, device=d)

    def make(**kw):
        a = dict(dtype=dtype, ldx=LD_X128, B=B, H=H, W=W, n_valid=3, gn_table=table, alpha=0.9, **t)
        a.update(kw)
        return ops.make_conv128_out(**a)
    for name in t:
        R.check(make(**{name: None}), "NULL")
    R.check(make(), "DTYPE", dtype=L.F32_SPLIT)
    for kw in (dict(H=24), dict(W=24), dict(B=0)):
        R.check(make(**kw), "SHAPE")
    for kw in (dict(n_valid=0), dict(n_valid=5)):
        R.check(make(**kw), "UNSUPPORTED")
    for kw in (dict(ldx=120), dict(ldx=LD_X128 - 4), dict(gn_table=off_by(table, 2))) + tuple({n: off_by(t[n], 4 if t[n].element_size() == 2 else 2)} for n in t):
        R.check(make(**kw), "ALIGN")
    R.nothing_written()


# =====================================================================================================================================
def test_zz_swin_edges_worst_ratios():
    """Prints the worst element ratio per kernel and the attention half's worst block (EDTR_SWIN_EDGES_ERRLOG=path dumps them)."""
    import json
    for k in sorted(ELEM):
        print(f"{k:24s} worst element ratio {ELEM[k]:.3f}")
    for dt, v in BLOCK.items():
        print(f"swin_attn {str(dt):16s} worst 32 x 32 block {v:.3g} (tolerance {SC.BLOCK_TOL_SWIN_ATTN[0 if dt == torch.bfloat16 else 1]})")
    path = os.environ.get("EDTR_SWIN_EDGES_ERRLOG")
    if path:
        with open(path, "w") as f:
            json.dump({"elem": ELEM, "block": {str(k): v for k, v in BLOCK.items()}}, f, indent=1, sort_keys=True)
    assert all(v <= 1.0 for v in ELEM.values()), ELEM
