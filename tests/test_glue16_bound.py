"""The checks of tests/test_gpu_glue16.py on the CPU, in the manner of tests/test_glue_bound.py: each 16-bit layout, elementwise and
normalisation kernel emulated in fp32 torch (tests/glue16_reference.py) stays below its bound against the fp64 reference, or equals
the bit-exact statement, at the shapes the GPU tests launch; and each defect such a kernel could have — the transpose's second channel
pass missing, pad columns left unzeroed (softmax P, nchw pad), pad columns included in a statistic, the grid-stride loop's second trip
missing, add_stats writing slot s with slot s + 1's sums, timestep-embedding indices >= 256 missing, LayerNorm's fourth vector slot
dropped, the softmax sum not rescaled when the running maximum moves, gn_apply's (pixel, vector) indices swapped in its generic loop —
pushes the ratio far above 1 or breaks bit equality.  The last tests document why the new cases exist: at the one friendly shape the
suite had before, those defects compute the same bits as the correct kernel."""
import pytest
import torch

import glue16_reference as R
from edtr_amd.testing import elem_ratio

F32 = torch.float32
DTYPES = [torch.bfloat16, torch.float16]
NAN = float("nan")
STALE = 199.0            # a finite value a pre-filled destination might hold (exact in both 16-bit formats)
FAR = 100.0            # "far above 1" (a wrong value of the right magnitude is at most 1 / 2u = 128 bounds away in bf16)


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                     b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


# ---- nchw_to_nhwc ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES + [F32])
def test_nchw_to_nhwc_bound_and_its_defects(dtype):
    src = _rnd((2, 70, 130), 1)
    ref, absref = R.nchw_to_nhwc_ref(src, 0.7, -0.3)
    good = R.nchw_to_nhwc_emulated(src, 0.7, -0.3, dtype, 72, STALE)
    assert elem_ratio(good[..., :70], ref, absref, dtype, 2)[0] <= 1.0
    assert float(good[..., 70:].float().abs().max()) == 0.0
    for stale in (NAN, STALE, 0.0):                       # even a stale zero: channels 64-69 are N(0, 1) values, not 0
        bad = R.nchw_to_nhwc_emulated(src, 0.7, -0.3, dtype, 72, stale, defect="one_pass")
        assert elem_ratio(bad[..., :70], ref, absref, dtype, 2)[0] > FAR
    bad = R.nchw_to_nhwc_emulated(src, 0.7, -0.3, dtype, 72, STALE, defect="pad_unzeroed")
    assert elem_ratio(bad[..., :70], ref, absref, dtype, 2)[0] <= 1.0 and float(bad[..., 70:].float().abs().max()) != 0.0
    # identity scale / shift: the bit-exact statement
    ident = R.nchw_to_nhwc_emulated(src, 1.0, 0.0, dtype, 72, STALE)
    assert _same_bits(ident[..., :70].contiguous(), src.permute(0, 2, 1).to(dtype).contiguous())
    assert not _same_bits(R.nchw_to_nhwc_emulated(src, 1.0, 0.0, dtype, 72, STALE, defect="one_pass")[..., :70].contiguous(),
                          src.permute(0, 2, 1).to(dtype).contiguous())


def test_the_old_nchw_to_nhwc_case_cannot_see_a_missing_second_pass():
    """tests/test_gpu_ops.py::test_layout_and_elementwise: C = 4 — the c0 loop runs once whether or not it could run twice."""
    src = _rnd((2, 4, 130), 2)
    for dtype in DTYPES:
        assert _same_bits(R.nchw_to_nhwc_emulated(src, 2.0, -1.0, dtype, 8, STALE, defect="one_pass"),
                          R.nchw_to_nhwc_emulated(src, 2.0, -1.0, dtype, 8, STALE))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nhwc_to_nchw_is_one_rounded_product(dtype):
    x = _rnd((2, 130, 70), 3).to(dtype)
    want = R.nhwc_to_nchw_exact(x, 70, 0.3)
    assert elem_ratio(want, x.double().permute(0, 2, 1) * R.f32(0.3), None, F32, 0)[0] <= 1.0
    one_pass = want.clone()
    one_pass[:, 64:] = NAN
    assert not _same_bits(one_pass, want)


# ---- grid-stride loops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_missing_second_trip_breaks_the_16_bit_add_only_above_one_grid_span(dtype):
    """add / split / embed_tokens move eight-wide vectors: 4096 x 256 of them per trip.  At the 3000 vectors the suite launched
    before, a one-trip kernel writes the same bits; at rows = 4100, C = 2056 the last 5124 vectors keep the destination's pattern."""
    for rows, C, seen in ((1000, 24, False), (4100, 2056, True)):
        a, b = _rnd((rows, C), 4).to(dtype), _rnd((rows, C), 5).to(dtype)
        want = R.add16_exact(a, b, dtype)
        assert elem_ratio(want, a.double() + b.double(), a.double().abs() + b.double().abs(), dtype, 1)[0] <= 1.0
        for stale in (NAN, STALE):
            got = R.second_trip_missing_units(want, stale, 8)
            assert (elem_ratio(got, want.double(), None, dtype, 0)[0] > FAR) == seen, (rows, stale)
            assert int((got != want.double()).sum()) == max(rows * C // 8 - R.GRID_SPAN, 0) * 8          # (NaN != x counts)


def test_a_missing_second_trip_of_the_other_loops():
    # fp32-stream add: four-wide vectors
    rows, C = 349600, 12
    a = _rnd((rows, C), 6)
    got = R.second_trip_missing_units(a, STALE, 4)
    assert int((got != a.double()).sum()) == (rows * C // 4 - R.GRID_SPAN) * 4
    # zero_bytes: 16-byte units, 1024 x 256 per trip
    n16 = R.ZERO_SPAN + 777
    want = torch.zeros((n16, 8), dtype=torch.bfloat16)
    got = R.second_trip_missing_units(want, STALE, 8, span=R.ZERO_SPAN)
    assert int((got != 0).sum()) == 777 * 8
    assert int((R.second_trip_missing_units(torch.zeros((2048, 8)), STALE, 8, span=R.ZERO_SPAN) != 0).sum()) == 0        # the old 32 KiB case
    # embed_tokens: the clamp of out-of-range ids and the row % L position are part of the bit-exact statement
    table, pos = _rnd((64, 16), 7), _rnd((77, 16), 8)
    tokens = torch.tensor([-1, 64, 0, 63] + [5] * 150)
    want = R.embed_tokens_exact(tokens, table, pos, torch.float16)
    assert _same_bits(want[0], (table[0] + pos[0]).half()) and _same_bits(want[1], (table[63] + pos[1]).half())
    assert _same_bits(want[77], (table[5] + pos[0]).half())
    wrapped = (table[tokens % 64] + pos[torch.arange(154) % 77]).half()
    assert not _same_bits(wrapped, want)


@pytest.mark.parametrize("src", [F32, torch.float16, torch.bfloat16])
def test_split_parts_reconstruct_the_source(src):
    """The restatement itself: hi + lo reproduces an fp32 source to 2 x the part's precision, and a 16-bit source of the same
    type exactly (lo = 0)."""
    x = (_rnd((301, 200), 9) * 3).to(src)
    for dt, u in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
        p = R.parts_exact(x, dt, "hlh").double()
        assert torch.equal(p[:, :200], p[:, 400:])
        err = (p[:, :200] + p[:, 200:400] - x.double()).abs()
        assert bool((err <= 4 * u * u * x.double().abs() + 2.0 ** -25).all())          # (2^-25: half the spacing of fp16 subnormals)
        if src == dt:
            assert float(p[:, 200:400].abs().max()) == 0.0
        assert torch.equal(R.parts_exact(x, dt, "hhl")[:, 400:], R.parts_exact(x, dt, "hl")[:, 200:])


# ---- add_stats -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slot_rows", [64, 128])
@pytest.mark.parametrize("with_b", [True, False])
def test_add_stats_bound_and_a_neighbouring_slots_sums(dtype, slot_rows, with_b):
    C = 96
    a = (_rnd((3 * slot_rows, C), 10) + 0.5).to(dtype)
    b = (_rnd((3 * slot_rows, C), 11) * 0.5 - 0.2).to(dtype) if with_b else None
    sums, absr = R.add_stats_ref(a, b, slot_rows)
    assert elem_ratio(R.add_stats_emulated(a, b, slot_rows), sums, absr, F32, slot_rows)[0] <= 1.0
    bad, _ = R.add_stats_ref(a, b, slot_rows, defect="next_slot")
    assert elem_ratio(bad, sums, absr, F32, slot_rows)[0] > FAR
    # the statistics of the ROUNDED output instead of the fp32 sum: visible to this bound where b is given (a 16-bit rounding of
    # every term against slot_rows 2^-22), invisible through a GroupNorm of the concatenation
    if with_b:
        rounded, _ = R.add_stats_ref(R.add16_exact(a, b, dtype), None, slot_rows)
        assert elem_ratio(rounded, sums, absr, F32, slot_rows)[0] > 1.0


# ---- timestep embedding ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES + [F32])
def test_timestep_embedding_bound_and_the_loops_later_trips(dtype):
    t = torch.tensor([0, 1, 999])
    for dim, seen in ((2, False), (64, False), (320, False), (1280, True)):        # 320: the only case before (half = 160 < 256 threads)
        ref, arg_err = R.temb_ref(t, dim)
        good = R.temb_emulated(t, dim, dtype)
        assert elem_ratio(good, ref, None, dtype, 0, {"fp32 argument": arg_err})[0] <= 1.0
        assert torch.equal(good[0].float(), torch.cat([torch.ones(dim // 2), torch.zeros(dim // 2)]))
        for stale in (NAN, STALE, 0.0):
            bad = R.temb_emulated(t, dim, dtype, stale, defect="one_trip")
            assert (elem_ratio(bad, ref, None, dtype, 0, {"fp32 argument": arg_err})[0] > FAR) == seen, (dim, stale)


# ---- softmax_rows ------------------------------------------------------------------------------------------------------------------
def _rescale_rows():
    s = torch.full((3, 1028), -80.0)
    s[0, 1026] = 80.0
    s[1] = _rnd((1028,), 12)
    s[1, 1025] = 12.0
    s[2] = _rnd((1028,), 13)
    s[2, 1] = 12.0
    return s


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_bound_and_its_defects(dtype):
    cases = {"pad8": _rnd((5, 132), 14) * 3, "cols4": _rnd((3, 4), 15) * 3, "cols1028": _rnd((3, 1028), 16) * 3, "rescale": _rescale_rows()}
    for name, live in cases.items():
        rows, cols = live.shape
        ld = cols + 8 - cols % 8
        s = torch.full((rows, ld), NAN)
        s[:, :cols] = live
        ref, extra = R.softmax_ref(live)
        good = R.softmax_emulated(s, cols, dtype, ld)
        assert elem_ratio(good[:, :cols], ref, ref, dtype, cols, extra)[0] <= 1.0, name
        assert float(good[:, cols:].float().abs().max()) == 0.0
        # the sum not rescaled when the maximum moves: every row with columns in more than one thread
        bad = R.softmax_emulated(s, cols, dtype, ld, defect="no_rescale")
        assert (elem_ratio(bad[:, :cols], ref, ref, dtype, cols, extra)[0] > 10.0) == (cols > 4), name
        # pad columns of P left as they were
        for stale in (NAN, STALE):
            bad = R.softmax_emulated(s, cols, dtype, ld, stale=stale, defect="pad_unzeroed")
            assert float(bad[:, cols:].float().abs().nan_to_num(nan=1.0).max()) != 0.0
        # pad columns of s read into the statistics: NaN there poisons the row whatever the scores are; a finite pad shows only
        # where it is large against the row (20 here; zeros next to a maximum of 9 would move the sum by 1e-4 and pass)
        bad = R.softmax_emulated(s, cols, dtype, ld, defect="pad_in_sum")
        assert elem_ratio(bad[:, :cols], ref, ref, dtype, cols, extra)[0] == float("inf"), name
        bad = R.softmax_emulated(s.nan_to_num(nan=20.0), cols, dtype, ld, defect="pad_in_sum")
        if name != "rescale":
            assert elem_ratio(bad[:, :cols], ref, ref, dtype, cols, extra)[0] > 10.0, name


def test_the_old_softmax_case_never_ran_the_zeroing_loop():
    """tests/test_gpu_ops.py::test_softmax_rows passes ld_p = cols and no cols_pad: there is no pad to leave unzeroed."""
    s = _rnd((10, 136), 17) * 3
    assert _same_bits(R.softmax_emulated(s, 136, torch.float16, 0, defect="pad_unzeroed"), R.softmax_emulated(s, 136, torch.float16, 0))


# ---- layernorm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bound_and_a_dropped_fourth_slot(dtype):
    for C, rows, shift, scale in ((2048, 3, 0.3, 1.5), (8, 2, 0.3, 1.5), (2048, 3, 8.0, 0.5), (72, 3, 8.0, 0.5), (1280, 3, 0.3, 1.5)):
        x = (_rnd((rows, C), 18) * scale + shift).to(dtype)
        gamma, beta = 1 + 0.1 * _rnd((C,), 19), 0.1 * _rnd((C,), 20)
        ref, absref = R.norm_ref(x, gamma, beta, 1e-5)
        assert elem_ratio(R.layernorm_emulated(x, gamma, beta, 1e-5, dtype), ref, absref, dtype, C)[0] <= 1.0, (C, shift)
        for defect in ("drop_slot3", "slot3_not_summed"):
            for stale in (NAN, STALE):
                bad = R.layernorm_emulated(x, gamma, beta, 1e-5, dtype, stale, defect)
                assert (elem_ratio(bad, ref, absref, dtype, C)[0] > 10.0) == (C > 1536), (C, defect, stale)      # C <= 1280 before: never seen


# ---- groupnorm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,HW,C,shift,scale", [(2, 70, 96, 0.7, 2.0), (2, 70, 960, 0.7, 2.0), (2, 1, 96, 0.7, 2.0), (2, 70, 96, 8.0, 0.5),
                                               (2, 70, 128, 8.0, 0.5), (1, 5000, 128, 0.7, 2.0)])
def test_groupnorm_bound_and_swapped_indices_in_the_generic_loop(dtype, B, HW, C, shift, scale):
    x = (_rnd((B * HW, C), 21) * scale + shift).to(dtype)
    gamma, beta = 1 + 0.1 * _rnd((C,), 22), 0.1 * _rnd((C,), 23)
    cpg = C // 32
    ref, absref = R.norm_ref(R.gn_groups(x, B, HW, C), R.gn_affine(gamma, HW, C), R.gn_affine(beta, HW, C), 1e-5, True)

    def ratio(y):
        return elem_ratio(R.gn_groups(y, B, HW, C), ref, absref, dtype, HW * cpg)[0]
    assert ratio(R.gn_emulated(x, gamma, beta, 1e-5, True, dtype, B, HW, C)) <= 1.0
    # C = 128 takes the power-of-two loop only: the defect in the generic loop cannot show there — nor at HW = 1 (one pixel per
    # workgroup: both splits of the index agree)
    seen = C in (96, 960) and HW > 1
    assert (ratio(R.gn_emulated(x, gamma, beta, 1e-5, True, dtype, B, HW, C, defect="swap")) > 10.0) == seen
    if HW == 70:
        # the statistics run over the neighbouring columns of the wider buffer (finite sentinels there)
        wide = torch.full((B * HW, C + 32), STALE, dtype=dtype)
        wide[:, 16:16 + C] = x
        assert ratio(R.gn_emulated(x, gamma, beta, 1e-5, True, dtype, B, HW, C, ld_stat=(wide, 16))) > 10.0


def test_gn_sums_reference_is_the_groups_own_sum():
    x = _rnd((2 * 5, 96), 24)
    s, a = R.gn_sums_ref(x, 2, 5, 96)
    assert abs(float(s[1, 31, 0]) - float(x[5:, 93:].double().sum())) < 1e-12 and abs(float(s[0, 0, 1]) - float((x[:5, :3].double() ** 2).sum())) < 1e-12
    assert bool((a[..., 0] >= s[..., 0].abs()).all())
