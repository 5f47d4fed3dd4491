"""The checks of tests/test_gpu_swin_edges.py on the CPU, in the manner of tests/test_glue16_bound.py and tests/test_parity_bound.py:
for each check, the fp64 or mirrored reference of tests/swin_cases.py, rounded to the output type, stands in for the kernel's output
and passes; one plausible defect of the kernel — the image-0 GroupNorm table applied to every image of conv128_out, or a table kept
for a workgroup's whole walk; the upsample source always read from image 0; fp32 NCHW plane n_valid written as well; the cyclic
shift applied along x only; the mask dropped for a one-pixel region; the row_stats sums in slot 1 instead of slot 3; one row's
LayerNorm statistics taken over 192 instead of c_valid columns; a store into column 192 of a row — fails it.  Where the defect
concerns a case tests/test_gpu_ops.py already had, the old case's check passes the defective output: the gap was real.  Also here:
the persistent-loop geometry rule gives 160 and 224 at 256 CUs, and each geometry sends workgroups through two different images."""
import pytest
import torch

import swin_cases as SC
from swin_cases import DTYPES, F32, LD_OUT
from edtr_amd.testing import block_rel, elem_ratio

FAR = 10.0              # "far above 1"


def ratio(got, ref, absref, k, out_dtype, extra=None):
    return elem_ratio(got, ref, absref, out_dtype, k, extra)[0]


def changed(buf, before, written):
    """Does swin_cases.untouched reject the buffer?"""
    try:
        SC.untouched(buf, before, written)
    except AssertionError:
        return True
    return False


# ---- persistent-loop geometry ------------------------------------------------------------------------------------------------------
def test_geometry_rule_at_256_cus_and_its_walks():
    assert SC.persistent_edge(256, 2) == 160 and SC.persistent_edge(256, 3) == 224
    assert SC.check_persistent(3, 160, 160, 256, 2) == 300 and SC.check_persistent(3, 224, 224, 256, 3) == 588
    two, three = SC.workgroup_images(3, 160, 160, 256), SC.workgroup_images(3, 224, 224, 256)
    assert two[0] == [0, 2] and max(len(w) for w in two) == 2 and min(len(w) for w in two) == 1            # workgroup 0: image 0, then image 2
    assert three[0] == [0, 1, 2] and sorted({len(w) for w in three}) == [2, 3]                               # both patch buffers reused; ragged
    for cus in (8, 64, 80, 104, 120, 256, 304):
        for rounds in (2, 3):
            E = SC.persistent_edge(cus, rounds)
            patches = SC.check_persistent(3, E, E, cus, rounds)
            assert E % 16 == 0 and patches == 3 * (E // 16) ** 2
            assert any(len(set(w)) >= 2 for w in SC.workgroup_images(3, E, E, cus)), (cus, rounds)
    with pytest.raises(AssertionError):
        SC.check_persistent(3, 160, 160, 304, 2)                # a changed CU count fails the case: 300 patches are one round there
    # the old cases: more images than one only with a patch per workgroup, more patches than workgroups only with one image
    assert all(len(w) == 1 for w in SC.workgroup_images(2, 32, 48, 256)) and all(set(w) == {0} for w in SC.workgroup_images(1, 512, 512, 256))
    assert 1024 % 256 == 0                                                                                  # ... and no ragged last round


# ---- edtr_conv128_out ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv128_out_wrong_or_stale_table(dtype):
    cus = 8                                                      # the geometry rule on a small "device": 48 x 48, 27 patches, 4 rounds of 8
    B, E = 3, SC.persistent_edge(cus, 3)
    SC.check_persistent(B, E, E, cus, 3)
    x, w, bias, gamma, beta = SC.conv128_operands(B, E * E, dtype, per_image=True)
    table = SC.gn_table_reference(x, gamma, beta, 1e-6, B)
    assert float((table[0, :, 0] / table[1, :, 0]).min()) > 2.5 and float((table[2, :, 0] / table[0, :, 0]).min()) > 2.5
    r64, a64, extra = SC.conv128_reference(x, w, bias, dtype, table, 0.9, B, E, E)
    assert ratio(r64.float(), r64, a64, 1152, F32, extra) <= 1.0
    image0 = SC.conv128_reference(x, w, bias, dtype, table, 0.9, B, E, E, table_image=0)[0]
    assert torch.equal(image0[0], r64[0]) and ratio(image0.float(), r64, a64, 1152, F32, extra) > FAR
    stale = SC.conv128_by_patch_table(x, w, bias, dtype, table, 0.9, B, E, E, SC.stale_table_images(B, E, E, cus))
    assert ratio(stale.float(), r64, a64, 1152, F32, extra) > FAR
    for n_valid in (1, 4):                                       # the planes the n_valid = 1 and 4 launches store
        assert ratio(stale[:, :n_valid].float(), r64[:, :n_valid], a64[:, :n_valid], 1152, F32, {k: v[:, :n_valid] for k, v in extra.items()}) > FAR
    # without a table the reference is the plain convolution, and differs grossly from the normalised one
    p64, pa64, _ = SC.conv128_reference(x, w[:1], bias, dtype, None, 0.9, B, E, E)
    assert ratio(p64.float(), p64, pa64, 1152, F32) <= 1.0 and ratio(r64[:, :1].float(), p64, pa64, 1152, F32) > FAR


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_old_conv128_out_cases_cannot_see_a_stale_table(dtype):
    """tests/test_gpu_ops.py::test_conv128_out_one_launch: (2, 32, 48) is 12 patches, one per workgroup — a workgroup that keeps its first
    table computes the same values; (1, 512, 512) walks, through one image."""
    assert torch.equal(SC.stale_table_images(2, 32, 48, 256), torch.arange(2)[:, None, None].expand(2, 2, 3))
    assert int(SC.stale_table_images(1, 512, 512, 256).max()) == 0
    B, H, W = 2, 32, 48
    x, w, bias, gamma, beta = SC.conv128_operands(B, H * W, dtype)
    table = SC.gn_table_reference(x, gamma, beta, 1e-6, B)
    r64, a64, extra = SC.conv128_reference(x, w, bias, dtype, table, 0.9, B, H, W)
    stale = SC.conv128_by_patch_table(x, w, bias, dtype, table, 0.9, B, H, W, SC.stale_table_images(B, H, W, 256))
    assert torch.equal(stale, r64) and ratio(stale.float(), r64, a64, 1152, F32, extra) <= 1.0


# ---- edtr_conv64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_conv64_upsample_source_always_image_0(dtype):
    B, E = 3, 32
    x, w, bias = SC.conv64_operands(B, E // 2, E // 2, 64, dtype)
    r64, a64 = SC.conv64_reference(x, w, bias, dtype, 1.0, 0.2, True)
    assert ratio(r64.to(dtype), r64, a64, 576, dtype) <= 1.0
    bad = SC.conv64_reference(x, w, bias, dtype, 1.0, 0.2, True, source_image=0)[0]
    assert torch.equal(bad[0], r64[0]) and ratio(bad.to(dtype), r64, a64, 576, dtype) > FAR
    # the old upsample cases have B = 1: the defect reads what the kernel reads
    x1, w1, b1 = SC.conv64_operands(1, 32, 16, 64, dtype)
    assert torch.equal(SC.conv64_reference(x1, w1, b1, dtype, 1.0, 0.2, True, source_image=0)[0], SC.conv64_reference(x1, w1, b1, dtype, 1.0, 0.2, True)[0])


@pytest.mark.parametrize("n_valid", [1, 4])
def test_fp32_plane_n_valid_written_as_well(n_valid):
    """The guard rows behind the planes see the last image's spill; an exactly sized tensor (the old case) cannot: the other images'
    spill lies under the next image's channel 0."""
    B, E = 3, 16
    x, w, bias = SC.conv64_operands(B, E, E, n_valid + 1, torch.bfloat16)
    r64, a64 = SC.conv64_reference(x, w, bias, torch.bfloat16, 0.7, None, False)
    rows = B * n_valid * E
    for spill in (False, True):
        buf, win, before = SC.window(rows, E, F32, None, "nan")
        SC.nchw_planes_store(win, r64.float(), n_valid, spill=spill)
        assert changed(buf, before, SC.region(win, rows, 0, E)) == spill
        assert ratio(win[:rows].reshape(B, n_valid, E, E), r64[:, :n_valid], a64[:, :n_valid], 576, F32) <= 1.0
        old = torch.full((B, n_valid, E, E), SC.NAN)             # the old case: a NaN-filled tensor of exactly the written size
        SC.nchw_planes_store(old, r64.float(), n_valid, spill=spill)
        assert bool(torch.isfinite(old).all()) and ratio(old, r64[:, :n_valid], a64[:, :n_valid], 576, F32) <= 1.0


# ---- edtr_window_attn ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SC.WINDOW_CASES))
def test_window_attn_cases_and_their_defects(dtype, case):
    B, H, W, heads, d, cp, shift, q_scale = SC.WINDOW_CASES[case]
    qkv, bias = SC.window_qkv(B, H, W, heads, d, dtype, q_scale)
    assert bool(torch.isfinite(qkv.float()).all())
    ref, pv, k, extra = SC.window_elem(qkv, bias, H, W, heads, d, shift, d ** -0.5, dtype)
    assert ratio(ref.to(dtype), ref, pv, k, dtype, extra) <= 1.0
    if case == "sharp_logits":
        lg = SC.window_logits(qkv, H, W, heads, d, shift)
        assert float(lg.max()) > 50.0 and float(lg.min()) < -50.0
        # a masked key is the raw row maximum somewhere
        from edtr_amd.model import swinir as S
        m = torch.from_numpy(S.shift_mask(H, W, 8, shift)).double()[:, None]
        raw = lg + bias.double()
        assert bool(((raw.argmax(-1, keepdim=True) != (raw + m).argmax(-1, keepdim=True))).any())
    for defect in ("shift_x_only", "thin_mask"):
        bad = SC.window_elem(qkv, bias, H, W, heads, d, shift, d ** -0.5, dtype, defect)[0]
        has_thin_band = shift in (1, 7)
        assert (ratio(bad.to(dtype), ref, pv, k, dtype, extra) > FAR) == (defect == "shift_x_only" or has_thin_band), (case, defect)


@pytest.mark.parametrize("shift", [0, 3, 4])
def test_the_old_shifts_cannot_see_a_mask_dropped_for_a_one_pixel_region(shift):
    """tests/test_gpu_ops.py launched shifts 0, 3 and 4 only: their bands are 8 - shift >= 4 and shift >= 3 pixels wide."""
    from edtr_amd.model import swinir as S
    for H, W in ((16, 24), (8, 8), (24, 8), (64, 64)):
        lab = S.region_labels(H, W, 8, shift)
        assert (SC.thin_band_merged(lab, H, W, shift) == lab).all()
    qkv, bias = SC.window_qkv(2, 16, 24, 6, 30, torch.float16)
    good = SC.window_attn_reference(qkv.double(), bias.double(), 16, 24, 6, 30, shift)
    assert torch.equal(SC.window_attn_reference(qkv.double(), bias.double(), 16, 24, 6, 30, shift, "thin_mask"), good)
    for s in (1, 7):
        lab = S.region_labels(16, 24, 8, s)
        assert (SC.thin_band_merged(lab, 16, 24, s) != lab).any()


# ---- edtr_swin_attn ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SC.ATTN_CASES))
def test_swin_attn_block_check_and_its_defects(dtype, case):
    B, H, W, shift, C = SC.ATTN_CASES[case]
    rows = B * H * W
    P = SC.attn_operands(dtype, C)
    assert P["d"] == C // 6 and (C == 192) == (P["d"] == 32)
    x = SC.attn_rows(rows, C, dtype)
    tol = SC.BLOCK_TOL_SWIN_ATTN[0 if dtype == torch.bfloat16 else 1]
    mirror = SC.attn_mirror(x, P, B, H, W, shift, dtype)
    assert block_rel(mirror.to(dtype), mirror, C) <= tol
    # (H = 8 at shift 4: the rows roll by half the one window row, the two row bands keep their members and their relative positions —
    # the shift along y cannot be observed there; the cases with shifts 1 and 7 see it)
    x_only = block_rel(SC.attn_mirror(x, P, B, H, W, shift, dtype, "shift_x_only").to(dtype), mirror, C)
    assert (x_only > FAR * tol) == (not (H == 8 and shift == 4)), x_only
    if shift in (1, 7):
        assert block_rel(SC.attn_mirror(x, P, B, H, W, shift, dtype, "thin_mask").to(dtype), mirror, C) > FAR * tol


# ---- edtr_swin_mlp -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(SC.MLP_CASES))
def test_swin_mlp_cases_and_statistics_over_the_wrong_width(dtype, case):
    rows, C, HID, kind = SC.MLP_CASES[case]
    P = SC.mlp_operands(dtype, C, HID)
    x = SC.mlp_rows(rows, C, dtype, kind=kind)
    assert float(x[:, C:].abs().max()) == 0.0 if C < SC.CP else True
    ref64, abs64, k, extra = SC.mlp_mirror(x, P, dtype)
    assert ratio(ref64.to(dtype), ref64, abs64, k, dtype, extra) <= 1.0
    if kind == "extreme":
        xd = x.double()[:, :C]
        r = xd.mean(1).abs() / xd.std(1, unbiased=False).clamp_min(1e-30)
        odd = torch.cat([r[1:5:2], r[7::2]])                     # (row 5 is the all-zero row)
        assert 15.0 < float(odd.min()) and float(odd.max()) < 17.0 and float(x[5].abs().max()) == 0.0
    if C < SC.CP:                                                # (with c_valid = 192 there is no other width)
        row = rows - 1
        bad = SC.mlp_mirror(x, P, dtype, wide_stats_row=row)[0]
        assert ratio(bad.to(dtype), ref64, abs64, k, dtype, extra) > (FAR if kind == "extreme" else 1.0)         # (192 / 180: 6 % of the mean)
        assert ratio(bad.to(dtype)[:row], ref64[:row], abs64[:row], k, dtype, {n: v[:row] for n, v in extra.items()}) <= 1.0 or row == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_stats_layout_and_sums_in_the_wrong_slot(dtype):
    rows = 129
    stored = torch.zeros((rows, SC.CP))
    stored[:, :180] = SC.rnd((rows, 180), 7, 1.5) + 0.4
    stored = stored.to(dtype)

    def stats(second_slot):
        xs = stored.float().reshape(rows, 2, 96)
        st = torch.zeros((rows, 6, 2))
        for half, slot in ((0, 0), (1, second_slot)):
            st[:, slot, 0], st[:, slot, 1] = xs[:, half].sum(-1), (xs[:, half] ** 2).sum(-1)         # fp32 sums
        return st
    r, zeros = SC.row_stats_ratio(stats(3), stored)
    assert r <= 1.0 and zeros
    r, zeros = SC.row_stats_ratio(stats(1), stored)
    assert r > FAR and not zeros
    minus_zero = stats(3)
    minus_zero[:, 4, 1] = -0.0
    assert not SC.row_stats_ratio(minus_zero, stored)[1]
    # the old check summed the slots: it cannot tell slot 1 from slot 3
    for st in (stats(3), stats(1)):
        tot = st.double().sum(1)
        assert float((tot[:, 0] - stored.double().sum(1)).norm() / stored.double().sum(1).norm()) < 2e-6
        assert float((tot[:, 1] - (stored.double() ** 2).sum(1)).norm() / (stored.double() ** 2).sum(1).norm()) < 2e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_store_into_column_192(dtype):
    """Column 192 of row r is column 0 of row r + 1 in an exactly sized [rows, 192] tensor — overwritten by that row's own store, the
    last row's lies behind the tensor — and a guard column at row stride 200."""
    rows = 5
    val = (SC.rnd((rows, SC.CP), 8) + 2.0).to(dtype)

    def store(flat, ld, stray):
        for r in range(rows):
            if stray and r * ld + SC.CP < flat.numel():
                flat[r * ld + SC.CP] = 77.0
        for r in range(rows):
            flat[r * ld:r * ld + SC.CP] = val[r]
    for stray in (False, True):
        old = torch.full((rows, SC.CP), SC.NAN, dtype=dtype)
        store(old.reshape(-1), SC.CP, stray)
        assert torch.equal(SC.bits(old), SC.bits(val))
        buf, win, before = SC.window(rows, LD_OUT, dtype, None, "nan")
        store(win.reshape(-1), LD_OUT, stray)
        assert torch.equal(SC.bits(win[:rows, :SC.CP]), SC.bits(val))
        assert changed(buf, before, SC.region(win, rows, 0, SC.CP)) == stray
