"""The igemm cells of tests/igemm_cells.py on the device (pytest -m gpu): z-batched launches of every GEMM template, the 64-bit-address
form of tile 3, tile 14 on its own, split-K on tiles 8 / 14 and with empty trailing splits, and the refusals.  tests/test_gpu_ops.py's
two gates and no new tolerance: the rounding-aware element bound against fp64 with k = K (edtr_amd.testing.elem_ratio <= 1) and the
whole-tensor relative L2 under its TOL (16-bit stores) or its fp32-output values (2e-5 plain, 5e-5 behind an activation:
test_gemm_batched_strided, test_gemm_bias_residual).

Every operand and every output is a view into a poisoned buffer (igemm_cells.layout: ld = width + 8, guard rows behind every slice, z
slices out of z order), so a finite result that meets the gates is the check that no stray row, column or slice was multiplied in,
and a store outside the [M, N] views fails.  The poison is NaN everywhere: include/edtr_hip.h gives edtr_igemm no pad it may read —
"out-of-range taps read 0" (the A operand, line 86), "Rows n >= n_valid read as zero" (the W operand, line 100), K is a multiple of 8
and the kernels fetch 8-element chunks inside [0, K) only — unlike edtr_flash_attn64's V^T pad, which must be finite (VT_PAD there).
edtr_igemm_plan's answer is asserted on the very parameter block before every launch."""
import ctypes
import os

import pytest
import torch

import igemm_cells as IC
import test_gpu_ops as G
from edtr_amd.testing import elem_ratio

pytestmark = pytest.mark.gpu

DTYPES = G.DTYPES
F32_TOL, F32_ACT_TOL = 2e-5, 5e-5      # test_gpu_ops.py's fp32-output values: test_gemm_batched_strided, test_gemm_bias_residual
FIGURES = {}                           # group -> {"ratio": worst element ratio, "rel_bf16" / "rel_fp16" / "rel_f32": worst relative L2}
NAN = float("nan")


def _code(dtype):
    from edtr_amd import lib as L
    return {torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _view(buf, sl, z):
    return buf.as_strided((sl.rows, sl.cols), (sl.ld, 1), sl.offs[z])


class Launch:
    """One cell on the device: NaN-filled buffers with the operands' slices written into their views, the parameter block, the
    output read back slice by slice with everything around the slices still NaN."""

    def __init__(self, c, dtype, d):
        self.c, self.dtype, self.d = c, dtype, d
        self.f, self.ptrs, self.slabs = IC.layout(c, _code(dtype))
        self.ops = IC.operands(c, dtype)
        self.out_dtype = torch.float32 if c.o.get("out_f32") else dtype
        self.bufs = {k: torch.full((sl.numel,), NAN, dtype=dtype, device=d) for k, sl in self.slabs.items() if k != "out"}
        dense = {"a": self.ops["a"], "w": self.ops["w"]}
        if "res" in self.ops:
            dense["res"] = self.ops["res"][None]
        for k, t in dense.items():
            for z in range(t.shape[0]):
                _view(self.bufs[k], self.slabs[k], z).copy_(t[z].to(d))
        self.vecs = {k: self.ops[k].to(d) for k in ("bias_n", "bias_m", "rowvec") if k in self.ops}
        M, N, _ = IC.dims(c)
        self.ws = torch.full((c.o["splitk"] * M * N,), NAN, dtype=torch.float32, device=d) if c.o.get("splitk", 0) > 1 else None

    def new_out(self):
        return torch.full((self.slabs["out"].numel,), NAN, dtype=self.out_dtype, device=self.d)

    def params(self, out, z=None):
        """The parameter block of the whole launch, or of slice z alone (Z = 1, the three pointers moved to the slice by hand)."""
        f, addr = dict(self.f), {"a1": self.bufs["a"].data_ptr(), "w": self.bufs["w"].data_ptr(), "out": out.data_ptr()}
        if z is not None:
            addr["a1"] += self.slabs["a"].offs[z] * 2
            addr["w"] += self.slabs["w"].offs[z] * 2
            addr["out"] += self.slabs["out"].offs[z] * out.element_size()
            f.update(Z=1, zdiv=1, a_zs_outer=0, a_zs_inner=0, w_zs_outer=0, w_zs_inner=0, o_zs_outer=0, o_zs_inner=0)
        for k, t in self.vecs.items():
            addr[k] = t.data_ptr()
        if "res" in self.bufs:
            addr["residual"] = self.bufs["res"].data_ptr()
        if self.ws is not None:
            addr["workspace"] = self.ws.data_ptr()
        return IC.to_params(f, self.ptrs, addr)

    def run(self, p, expect=None):
        """Assert the plan, then launch; returns edtr_igemm's code."""
        from edtr_amd import lib as L
        want = self.c.expect if expect is None else expect
        assert IC.plan_of(p) == want, (self.c.name, self.c.path)
        rc = int(L.load().edtr_igemm(ctypes.byref(p), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def read(self, out):
        """[Z, M, N] of the output's slices; every slice finite, every other element of the buffer still NaN."""
        sl = self.slabs["out"]
        host = out.cpu()
        got = torch.stack([_view(host, sl, z).clone() for z in range(len(sl.offs))])
        assert bool(torch.isfinite(got).all()), "non-finite values in the valid region: a poisoned row, column or slice was multiplied in"
        for z in range(len(sl.offs)):
            _view(host, sl, z).fill_(NAN)
        assert bool(torch.isnan(host).all()), "a store landed outside the [M, N] views: guard rows, guard columns or the gap between slices"
        return got

    def gates(self, got):
        c, K = self.c, IC.dims(self.c)[2]
        ref, ab = IC.reference(c, self.ops)
        r, where = elem_ratio(got, ref, ab, self.out_dtype, K)
        e = float((got.double() - ref).norm() / ref.norm())
        kind = "f32" if c.o.get("out_f32") else ("bf16" if self.dtype == torch.bfloat16 else "fp16")
        print(f"[igemm cell] {c.name} {kind}: element ratio {r:.3f}, relative L2 {e:.3e}")
        fig = FIGURES.setdefault(c.group, {})
        fig["ratio"] = max(fig.get("ratio", 0.0), r)
        fig["rel_" + kind] = max(fig.get("rel_" + kind, 0.0), e)
        assert r <= 1.0, f"element bound exceeded: ratio {r:.3g} at {where}"
        tol = (F32_ACT_TOL if c.o.get("act") else F32_TOL) if c.o.get("out_f32") else G.TOL[self.dtype]
        assert e < tol, (e, tol)


def _run_cell(c, dtype):
    la = Launch(c, dtype, G.dev())
    out = la.new_out()
    assert la.run(la.params(out)) == 0
    la.gates(la.read(out))
    return la, out


# ---- a. z-batches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", IC.cells("z"), ids=IC.ids(IC.cells("z")))
def test_z_batched_launch(c, dtype):
    """blockIdx.z > 0 in every GEMM template with zdiv > 1 and non-zero inner strides: the fp64 gates, and bit-identical to Z launches
    of the same tile on the slices (the same kernel in the same order: any difference is an offset bug)."""
    la, out = _run_cell(c, dtype)
    single = la.new_out()
    for z in range(c.s["Z"]):
        assert la.run(la.params(single, z)) == 0
    assert torch.equal(_bits(out), _bits(single)), "the z-batched launch differs from the per-slice launches"


# ---- b. the 64-bit-address form of tile 3 (bf16 only) -----------------------------------------------------------------------------------------
SMALL_ROUTE = [c for c in IC.cells("wide") if c.name.startswith("up2")]
WIDE = [c for c in IC.cells("wide") if c.name.startswith("wide")]


@pytest.mark.parametrize("c", SMALL_ROUTE, ids=IC.ids(SMALL_ROUTE))
def test_nearest2x_source_off_the_fast_path(c):
    """upsample2x with stride 2 takes tile 3 off its buffer-addressed path (igemm_plan.h fast_path): launch_dma<T, true, false>, and the
    register-staged tiles 1 / 2 on a nearest-2x source at either stride."""
    _run_cell(c, torch.bfloat16)


@pytest.mark.parametrize("c", WIDE, ids=IC.ids(WIDE))
def test_wide_operand_runs_the_64_bit_form(c):
    """An A or W operand whose row stride carries its last rows past 4 GiB: igemm_fast_addressable is false, tile 0 and tile 3 both
    run launch_dma<T, SPATIAL, false>.  One buffer of a little over 4 GiB alive at a time."""
    try:
        la, out = _run_cell(c, torch.bfloat16)
        k = "w" if "ldw" in c.o else "a"
        sl = la.slabs[k]
        assert (sl.rows - 1) * sl.ld * 2 >= 1 << 32 and la.bufs[k].numel() * 2 > 1 << 32, "the last rows lie past a 4 GiB byte offset"
    finally:
        la = out = None
        torch.cuda.empty_cache()


# ---- c. tile 14 on its own --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", IC.cells("t14"), ids=IC.ids(IC.cells("t14")))
def test_tile14_against_fp64(c, dtype):
    _run_cell(c, dtype)


# ---- d. split-K ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", IC.cells("splitk"), ids=IC.ids(IC.cells("splitk")))
def test_splitk_cells(c, dtype):
    """Split-K on tiles 8 / 14, and trailing splits that own no K-tile: the workspace starts as NaN, so a slab that is not written —
    zeros for an empty split — turns the reducer's sum into NaN."""
    la, _ = _run_cell(c, dtype)
    assert bool(torch.isfinite(la.ws).all()), "a slab element was not written"


# ---- e. refusals launch nothing -----------------------------------------------------------------------------------------------------------------
REFUSALS = [(c, dt) for c in IC.cells("refuse") for dt in (DTYPES if not c.name.startswith("wide") else DTYPES[:1])]


@pytest.mark.parametrize("c,dtype", REFUSALS, ids=[f"{c.name}-{'bf16' if dt == torch.bfloat16 else 'fp16'}" for c, dt in REFUSALS])
def test_refusals_launch_nothing(c, dtype):
    try:
        la = Launch(c, dtype, G.dev())
        out = la.new_out()
        p = la.params(out)
        want = IC.plan_of(p)
        assert want == IC.E_UNSUPPORTED
        assert la.run(p) == want, "edtr_igemm returns the planner's error"
        for t in (out, la.ws):
            if t is not None:
                assert bool((_bits(t) == _bits(torch.full((1,), NAN, dtype=t.dtype, device=t.device))).all()), "a refused launch wrote something"
    finally:
        la = out = None
        torch.cuda.empty_cache()


def test_zz_cells_figures():
    """Bookkeeping (runs last in this file): the worst element ratio and relative L2 error per group; EDTR_CELLS_ERRLOG=path dumps them."""
    import json
    for g, fig in sorted(FIGURES.items()):
        print(f"\n[igemm cells] group {g}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(fig.items())))
    path = os.environ.get("EDTR_CELLS_ERRLOG")
    if path:
        with open(path, "w") as fh:
            json.dump(FIGURES, fh, indent=1)
