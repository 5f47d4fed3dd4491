"""The fp32-stream cells of tests/stream_cells.py on the device (pytest -m gpu), one launch per cell and dtype (a second, unsplit one for
the split-K cells).  Every check is stream_cells.judge() on what the device wrote, the function tests/test_stream_cells_cpu.py shows to
accept a correct kernel and to reject the named defects: guards intact on out, out16, gn_partial, the workspace tail and the operands;
the output inside edtr_amd.testing.elem_bound of the fp64 reference (k = the reduction length); the mirror bit-equal to the cast of the
stored output; every statistics slot inside the same bound form of fp64 sums of the stored output over that slot's rows; the split-K
result inside the element bound of the unsplit launch.  edtr_igemm_plan's answer is asserted on the very parameter block before every
launch.  No tolerance of its own."""
import ctypes
import json
import os

import pytest
import torch

import igemm_cells as IC
import stream_cells as S
import test_gpu_ops as G

pytestmark = pytest.mark.gpu

ELEM = {}      # "cell-dtype" -> {"out": worst element ratio, "stats": worst statistics-slot ratio, "unsplit": split-K against the unsplit launch}


def _launch(cs, d, dev_in, vecs, splitk=True):
    """One launch of the cell into fresh NaN-filled outputs; returns the host copies of the outputs."""
    from edtr_amd import lib as L
    outs = {k: t.to(d) for k, t in cs.new_outputs(splitk).items()}
    f, ptrs = dict(cs.f), list(cs.ptrs)
    if not splitk and cs.splitk > 1:      # the unsplit launch of a split-K cell: no workspace, and no statistics (64-row slots are the reducer's)
        f.update(splitk=0, workspace_bytes=0, gn_slot_rows=0)
        ptrs = [p for p in ptrs if p not in ("workspace", "gn_partial")]
        outs.pop("gnp", None)
    addr = {"a1": dev_in["a"].data_ptr(), "w": dev_in["w"].data_ptr(), "out": outs["out"].data_ptr()}
    if "res" in dev_in:
        addr["residual"] = dev_in["res"].data_ptr()
    for k, t in vecs.items():
        addr[k] = t.data_ptr()
    for k, name in (("out16", "out16"), ("gnp", "gn_partial"), ("ws", "workspace")):
        if k in outs:
            addr[name] = outs[k].data_ptr()
    p = IC.to_params(f, ptrs, addr)
    assert IC.plan_of(p) == cs.c.expect, (cs.sc.name, cs.c.path)
    rc = int(L.load().edtr_igemm(ctypes.byref(p), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, rc
    return {k: t.cpu() for k, t in outs.items()}


@pytest.mark.parametrize("sc,dt", S.RUNS, ids=S.RUN_IDS)
def test_stream_cell(sc, dt):
    d = G.dev()
    cs = S.case(sc.name, dt)
    dev_in = {k: t.to(d) for k, t in cs.inputs.items()}
    vecs = {k: t.to(d) for k, t in cs.vecs.items()}
    outs = _launch(cs, d, dev_in, vecs)
    fig = S.judge(cs, outs, {k: t.cpu() for k, t in dev_in.items()})
    if cs.splitk > 1:
        plain = _launch(cs, d, dev_in, vecs, splitk=False)
        fig["unsplit"] = S.same_as_unsplit(cs, outs["out"], plain["out"])
    print(f"[stream cell] {sc.name} {dt}: " + ", ".join(f"{k} {v:.3f}" for k, v in fig.items()))
    ELEM[f"{sc.name}-{dt}"] = fig


def test_zz_stream_cells_figures():
    """Bookkeeping (runs last in this file): the worst ratios per cell; EDTR_STREAM_ERRLOG=path dumps them."""
    for k, fig in sorted(ELEM.items()):
        print(f"\n[stream cells] {k}: " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(fig.items())))
    path = os.environ.get("EDTR_STREAM_ERRLOG")
    if path:
        with open(path, "w") as fh:
            json.dump(ELEM, fh, indent=1, sort_keys=True)
