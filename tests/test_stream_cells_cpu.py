"""tests/stream_cells.py without a GPU: every cell's edtr_igemm_plan answer (refusals as refusals), the census of what the parity modes
emit against the cells' `covers`, the references and the layout against themselves, and the named defects: stream_cells.simulate() is a
kernel that computes the fp64 reference and rounds once — stream_cells.judge(), which is every check tests/test_gpu_stream_cells.py
applies to what the device wrote, must accept it and must reject each of its defects on every cell that carries the feature."""
import json
import os
import sys

import pytest
import torch

import igemm_cells as IC
import stream_cells as S
from edtr_amd.testing import elem_bound, elem_ratio

MODES = ("mixed", "hybrid", "robust", "high")


# ---- plans --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", S.CELLS, ids=lambda sc: sc.name)
def test_plan_answers_the_table(sc):
    for code in (0, 1):
        f, ptrs, _ = IC.layout(sc.cell, code)
        assert IC.plan_of(IC.to_params(f, ptrs)) == sc.cell.expect, (sc.name, sc.launch)
    assert (sc.cell.expect == S.E_UNSUPPORTED) == (sc.cell.group == "refuse") and bool(sc.covers) == (sc.cell.expect > 0)


def test_the_layout_is_hostile():
    """ld = width + 8 / + 4 floats / + 16, all different; guard rows behind every slice; a guard slot behind the statistics."""
    for sc in S.LAUNCHED:
        f, _, slabs = IC.layout(sc.cell)
        n = IC.n_out(sc.cell)
        lds = [f["ldc"]] + [f[k] for k in ("ldr", "ld16") if k in f]
        assert f["ldc"] == n + 8 and len(set(lds)) == len(lds) and all(ld > n for ld in lds), sc.name
        if sc.cell.o.get("res_f32"):
            assert f["ldr"] == n + 4 and f["residual_f32"] == 1
        for k, sl in slabs.items():
            if k == "gnp":
                assert sl.numel == (sl.rows + 1) * sl.cols, "one guard slot"
            else:
                assert sl.numel >= max(sl.offs) + (sl.rows + 2) * sl.ld and sl.ld >= sl.cols + 4, (sc.name, k)
        if "gnp" in slabs:
            assert len(S.slot_rows(sc.cell)) == slabs["gnp"].rows
            every = torch.cat(S.slot_rows(sc.cell)).sort().values
            assert torch.equal(every, torch.arange(IC.dims(sc.cell)[0])), "the slots cover every output row once"


def test_the_table_covers_what_it_claims():
    by = S.BY_NAME
    # split-K cells leave a split short or empty
    for name, tiles, S_ in (("t3-sk", 5, 4), ("t3-2w-sk", 4, 3), ("t3-s2-gnp-sk64", 9, 6)):
        c = by[name].cell
        assert (IC.dims(c)[2] + 63) // 64 == tiles and c.o["splitk"] == S_
        per = -(-tiles // S_)
        assert per * (S_ - 1) >= tiles, "the trailing split owns no K-tile"
    c = by["t16-img8-r32-gnp-sk64"].cell
    chunks = [(y + 1) * (c.s["cin"] // 64) // c.o["splitk"] - y * (c.s["cin"] // 64) // c.o["splitk"] for y in range(c.o["splitk"])]
    assert len(set(chunks)) > 1 and IC.dims(c)[0] == 512 and c.s["B"] == 8
    # every halo tile at three parts per tap; a real split per format
    assert {sc.cell.expect for sc in S.LAUNCHED if sc.cell.o.get("parts") == 3} >= {16, 17, 20}
    assert {(sc.dtypes, sc.cell.o["split"]) for sc in S.LAUNCHED if sc.cell.o.get("split")} == {(("bf16",), 3), (("fp16",), 2), (("fp16",), 3)}
    # ragged M where the form admits it
    for sc in S.LAUNCHED:
        c, (M, N, _) = sc.cell, IC.dims(sc.cell)
        if c.kind == "gemm" and not c.o.get("gnp"):
            bm = IC.TILE_BM_BN[c.expect][0]
            assert M == 2 * bm + 1 or c.expect == 1, sc.name
        if c.o.get("gnp"):
            assert M % 128 == 0 and M // (c.o.get("slot") or 128) >= 2, sc.name
    # the forms the issue names, each as a `covers` of a launched cell
    named = ["t16 taps9 f32 r32 gnp slot64 sk", "t16 taps9 f32 r32 gnp slot128 sk", "t16 taps9 f32 r32 m16 gnp slot64 sk", "t16 taps9 f32 gnp rv",
             "t16 taps9 f32 gnp slot128 sk rv", "t16 taps9 f32 gnp slot64 sk rv", "t20 taps9 f32 gnp rv", "t16 taps9 up2 f32 m16 sk ldc>N",
             "t16 taps9 up2sp f32 m16 ldc>N", "t16 taps9 up2sp f32 gnp", "t17 taps9 f32 r32 gnp gnin", "t3 taps9 s2 f32 gnp", "t3 taps9 s2 f32 gnp slot64 sk",
             "t3 taps9 s2 f32 gnp slot128 sk", "t3 taps9 s2 f32 m16 gnp slot64 sk", "t3 taps9 s2 f32 m16 gnp slot128 sk", "t6 taps9 s2 f32 gnp", "t6 taps1 f32",
             "t6 taps1 f32 Z", "t6 taps1 f32 r32 gnp", "t8 taps1 o16 r32", "t3 taps1 o16 r32 sk", "t8 taps1 f32 r32 m16 gnp", "t3 taps1 f32 r32 m16 gnp",
             "t8 taps1 f32 r32 m16 ldc>N", "t3 taps1 f32 r32 m16 ldc>N", "t3 taps1 f32 2w sk"]
    covered = {k for sc in S.LAUNCHED for k in sc.covers}
    assert not [k for k in named if k not in covered]


# ---- the census ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emitted():
    """{key: {"launch", "bf16"}} over the four parity modes, each built in a fresh child process (at most 4 side by side)."""
    import test_program_signatures_cpu as P
    procs = [(m, P.start_child("full.mixed", [os.path.abspath(__file__), m])) for m in MODES]      # ("full.mixed": a group without switches)
    out = {}
    for m, proc in procs:
        text, err = proc.communicate()
        lines = [ln for ln in text.splitlines() if ln.startswith("CENSUS ")]
        assert proc.returncode == 0 and len(lines) == 1, f"{m}: the child process failed ({proc.returncode})\n{err[-4000:]}"
        for k, v in json.loads(lines[0][len("CENSUS "):]).items():
            e = out.setdefault(k, {"launch": v["launch"], "bf16": False})
            e["bf16"] = e["bf16"] or v["bf16"]
    return out


def test_every_emitted_form_has_a_cell(emitted):
    covered = {k for sc in S.LAUNCHED for k in sc.covers}
    missing = [f"{k}  <-  {v['launch']}" for k, v in sorted(emitted.items()) if k not in covered]
    assert not missing, "forms the engine emits and no cell launches:\n" + "\n".join(missing)


def test_every_cell_stands_for_an_emitted_form(emitted):
    """... unless it is marked `extra` with its reason; and no two cells that are not `extra` share a key, so deleting any one of them
    leaves an emitted form without a cell (test_every_emitted_form_has_a_cell then names its launch)."""
    owner = {}
    for sc in S.LAUNCHED:
        if sc.extra:
            assert isinstance(sc.extra, str) and sc.extra
            continue
        for k in sc.covers:
            assert k in emitted, (sc.name, k)
            assert owner.setdefault(k, sc.name) == sc.name, (k, owner[k], sc.name)
    assert sorted(owner) == sorted(emitted)


def test_cells_run_in_bf16_where_the_high_mode_emits_them(emitted):
    for sc in S.LAUNCHED:
        if not sc.cell.o.get("split"):
            assert ("bf16" in sc.dtypes) == any(emitted[k]["bf16"] for k in sc.covers if k in emitted) and "fp16" in sc.dtypes, sc.name


# ---- references, the perfect kernel, the defects ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc,dt", S.RUNS, ids=S.RUN_IDS)
def test_references_are_sound_and_the_perfect_kernel_passes(sc, dt):
    """The fp64 reference against the same expression in fp32 under the element bound (ratio in (0, 1]: the bound, the operands' scale and
    the absref are sound before any kernel is involved), then judge() on simulate()'s buffers."""
    cs = S.case(sc.name, dt)
    ref, ab, extra = cs.reference
    assert ref.shape == (sc.cell.s["Z"], cs.M, cs.No) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    if sc.cell.o.get("act") != IC.GEGLU:
        assert bool((ab >= ref.abs() * (1 - 1e-12)).all()), "absref bounds |ref|"
    if not sc.cell.o.get("a_gn"):      # (the fp32 form of the normalisation may round to a neighbouring 16-bit value: that is the `extra` term)
        got32, _ = IC.reference(sc.cell, cs.ops, torch.float32)
        r, where = elem_ratio(got32, ref, ab, torch.float32, S.kred(sc.cell), extra)
        assert 0.0 < r <= 1.0, (r, where)
    fig = S.judge(cs, S.simulate(cs), cs.inputs)
    assert fig["out"] <= 0.5 + 1e-9, "one rounding of the output is half the bound's 2 u |ref|"


# (a residual rounded to 16 bits is no defect the element bound can see at a long K: stream_cells' docstring, res16_visible)
DEFECT_RUNS = [(d, sc, dt) for d in S.DEFECTS for sc, dt in S.RUNS if S.applies(sc, d) and (d != "res16" or S.res16_visible(sc, dt))]


@pytest.mark.parametrize("defect,sc,dt", DEFECT_RUNS, ids=[f"{d}-{sc.name}-{dt}" for d, sc, dt in DEFECT_RUNS])
def test_defects_are_rejected(defect, sc, dt):
    cs = S.case(sc.name, dt)
    with pytest.raises(AssertionError):
        S.judge(cs, S.simulate(cs, defect), cs.inputs)


def test_every_defect_meets_a_cell():
    for d in S.DEFECTS:
        assert [1 for dd, _, _ in DEFECT_RUNS if dd == d], d
    seen = [sc for d, sc, _ in DEFECT_RUNS if d == "res16"]
    assert {sc.cell.expect for sc in seen} >= {3, 6, 8, 16, 17, 20}, "the residual's rounding is visible on every tile that adds one (bf16 on the halo tiles)"


@pytest.mark.parametrize("sc,dt", [(sc, dt) for d, sc, dt in DEFECT_RUNS if d == "res16"], ids=lambda v: v if isinstance(v, str) else v.name)
def test_the_fp32_residual_cannot_pass_as_a_16_bit_one(sc, dt):
    """Rounding the residual to the operand type exceeds the element bound 4 x on at least half the elements."""
    cs = S.case(sc.name, dt)
    ref, ab, extra = cs.reference
    res = cs.ops["res"]
    err = (res.to(cs.dtype).double() - res.double()).abs()
    over = err > 4 * elem_bound(ref, ab, cs.out_dtype, S.kred(sc.cell), extra)[0]
    assert float(over.double().mean()) >= 0.5, float(over.double().mean())


def child_main(mode):
    torch.set_num_threads(2)
    print("CENSUS " + json.dumps(S.census(mode), sort_keys=True))


if __name__ == "__main__":
    child_main(sys.argv[1])
