"""tests/igemm_cells.py without a GPU: every cell's edtr_igemm_plan answer, the automatic tile of the production shapes at full size,
and the reference builders against themselves (placeholder pointers: the planner touches no memory and makes no HIP call, as in
tests/test_igemm_plan_cpu.py).  tests/test_gpu_igemm_cells.py launches the same cells."""
import pytest
import torch

import igemm_cells as IC
from edtr_amd.testing import elem_ratio

DTYPES = [torch.bfloat16, torch.float16]


def _plan(c, **kw):
    f, ptrs, _ = IC.layout(c, **kw)
    return IC.plan_of(IC.to_params(f, ptrs))


def test_the_table_covers_what_it_claims():
    names = set(IC.BY_NAME)
    for t in IC.GEMM_TILES:      # z-batches on every GEMM template: fp32 + alpha, bias_m + n_valid, shared A, zdiv = 1
        assert {f"z6-t{t}-f32alpha", f"z6-t{t}-biasm-nvalid", f"z6-t{t}-sharedA", f"z6-t{t}-zdiv1"} <= names
        bm, bn = IC.TILE_BM_BN[t]
        M, N, _ = IC.dims(IC.BY_NAME[f"z6-t{t}-f32alpha"])
        assert M > 2 * bm and M % bm and N > bn and N % bn, "more than one tile and a ragged tail both ways"
    for c in IC.cells("z"):
        if c.name.startswith("z6-") and "zdiv1" not in c.name:
            assert c.s["Z"] == 6 and c.s["zdiv"] == 3
            f, _, slabs = IC.layout(c)
            for k in ("a", "w", "out"):      # distinct non-zero outer / inner strides, slices not in z order
                outer, inner = f[k[0] + "_zs_outer"], f[k[0] + "_zs_inner"]
                if k == "a" and c.o.get("shared_a"):
                    assert (outer, inner) == (0, 0)
                else:
                    assert outer and inner and outer != inner and slabs[k].offs != sorted(slabs[k].offs), (c.name, k)
            assert len({f["a_zs_outer"], f["a_zs_inner"], f["w_zs_outer"], f["w_zs_inner"], f["o_zs_outer"], f["o_zs_inner"]} - {0}) >= (4 if c.o.get("shared_a") else 6)
    assert {c.tile for c in IC.cells("splitk") if "empty" in c.name} >= {1, 2, 3}
    assert {c.tile for c in IC.cells("splitk") if "empty" not in c.name} == {8, 14}
    assert {IC.dims(c)[1] for c in IC.cells("t14")} == {8, 24, 32, 40} and {IC.dims(c)[0] for c in IC.cells("t14") if c.kind == "gemm"} == {513, 300}
    assert len(IC.cells("refuse")) >= 3 + 15 + 1


@pytest.mark.parametrize("c", IC.CELLS, ids=IC.ids(IC.CELLS))
def test_plan_answers_the_table(c):
    for code in (0, 1):
        assert _plan(c, dtype_code=code) == c.expect, (c.name, c.path)


@pytest.mark.parametrize("c", [c for c in IC.cells("wide") if c.name.startswith("wide")], ids=lambda c: c.name)
def test_wide_operands_fall_to_the_64_bit_form_of_tile_3_only(c):
    """Past kBufferLimit (igemm_plan.h: 0xF0000000 bytes) no buffer-addressed tile may run: the automatic choice and tile 3 answer 3,
    every fast-only or halo tile refuses; with the ordinary row stride the same shape is admitted by tiles 6 / 8."""
    assert _plan(c, tile=0) == 3 and _plan(c, tile=3) == 3
    for t in (6, 8, 14, 16, 17):
        assert _plan(c, tile=t) == IC.E_UNSUPPORTED, t
    narrow = c._replace(o={k: v for k, v in c.o.items() if k not in ("ld1", "ldw")})
    assert _plan(narrow, tile=6) == 6 and _plan(narrow, tile=8) == 8


@pytest.mark.parametrize("c", [c for c in IC.CELLS if c.auto], ids=lambda c: c.name)
def test_production_shapes_choose_their_tile_at_full_size(c):
    """tile = 0 at the full-size shape (and its neighbour one batch lower): if a threshold of choose() moves, the cell fails instead of
    quietly testing another kernel.  IC.PLAN_CUS: the planner's CU count without a device; none of these rules reads it."""
    assert c.auto[0][1] == c.tile, "the first `auto` entry is the production shape the cell stands for"
    for shape, want in c.auto:
        assert _plan(c, shape=shape, tile=0) == want, (c.name, shape)


def test_the_planner_assumes_plan_cus_without_a_device():
    """IC.PLAN_CUS = 256 is what edtr_igemm_plan counts with when no device is there: the one whole-chip rule with a plain threshold
    (16 -> 17 from one 512-pixel unit per CU) flips between 255 and 256 units."""
    import test_igemm_plan_cpu as P
    for units, want in ((IC.PLAN_CUS, 17), (IC.PLAN_CUS - 1, 16)):
        d = P.conv(1, 16 * units, 32, 128, 128)        # M >> 9 = units, one 128-column tile
        assert IC.plan_of(P.to_params(d)) == want, units


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [c for c in IC.CELLS if c.group != "refuse"], ids=lambda c: c.name)
def test_reference_builders_are_sound(c, dtype):
    """The fp64 reference against the same expression in fp32: the element bound (k = K, fp32 `output`) must hold with ratio <= 1 before
    any kernel is involved — it shows the bound, the operands' scale and the absref are sound."""
    M, N, K = IC.dims(c)
    d = IC.operands(c, dtype)
    ref, ab = IC.reference(c, d)
    got, _ = IC.reference(c, d, torch.float32)
    assert ref.shape == (c.s["Z"], M, N) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert bool((ab >= ref.abs() * (1 - 1e-12)).all()), "absref bounds |ref|"
    r, where = elem_ratio(got, ref, ab, torch.float32, K)
    assert r <= 1.0, (r, where)
    assert r > 0.0, "fp32 and fp64 differ somewhere: the comparison is not vacuous"
