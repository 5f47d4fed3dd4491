"""edtr_flash_attn64_plan without a GPU: which kernel edtr_flash_attn64 would run (the launch dispatches on the same function,
edtr_amd/csrc/attention.hip: attn64_choose), for the launch geometries of tests/attn_cases.py — the GPU cases of
tests/test_gpu_ops.py assert the same answers on their real operands before they launch — the thresholds between the kernels,
and the error codes of the rejects.  The switches EDTR_ATTN_V3 / EDTR_ATTN_V3_MIN_NQ / EDTR_ATTN_SMALLK are read once per process
and must be unset (their defaults are what production runs)."""
import ctypes
import os

import pytest
import torch

import attn_cases
from attn_cases import GENERIC, SMALLK, SPLIT_QK, SPLIT_QKPV, V3

E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_UNSUPPORTED = -1, -2, -3, -4, -5      # include/edtr_hip.h: enum edtr_error
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _default_switches():
    if any(os.environ.get(v) is not None for v in ("EDTR_ATTN_V3", "EDTR_ATTN_V3_MIN_NQ", "EDTR_ATTN_SMALLK")):
        pytest.fail("an EDTR_ATTN_* switch is set: the plans below are those of the default launch rules")


def test_ids_match_the_header():
    from edtr_amd import lib, ops
    for name, value in (("GENERIC", GENERIC), ("SPLIT_QK", SPLIT_QK), ("SPLIT_QKPV", SPLIT_QKPV), ("SMALLK", SMALLK), ("V3", V3)):
        assert getattr(lib, f"ATTN_{name}") == value            # enum edtr_attn_kernel, as the binding reads it from the header
        assert getattr(ops, f"ATTN_{name}") == value
    assert (lib.E_NULL, lib.E_SHAPE, lib.E_ALIGN, lib.E_DTYPE, lib.E_UNSUPPORTED) == (E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_UNSUPPORTED)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", attn_cases.CASES, ids=[c.name for c in attn_cases.CASES])
def test_plan_of_every_launch_geometry(dtype, case):
    """Dense strides and the guarded layout of the GPU cases (q | k in one [N + 2, 2C + 8] buffer, V^T rows of round_up(Nk, 8) + 8,
    an output pitch of C + 8) plan alike: the choice depends on the shape, never on the strides."""
    from edtr_amd import ops
    C = case.H * 64
    want = (case.kernel, case.bpw)
    kw = dict(causal=case.causal, prescaled=case.prescaled)
    assert ops.flash_attn_plan_shape(dtype, case.B, case.H, case.Nq, case.Nk, **kw) == want
    assert ops.flash_attn_plan_shape(dtype, case.B, case.H, case.Nq, case.Nk, q_ld=2 * C + 8, k_ld=2 * C + 8,
                                     vt_ld=ops.round_up(case.Nk, 8) + 8, o_ld=C + 8, **kw) == want
    if case.head_map is not None:
        assert ((case.B * case.H) % 8 == 0) == case.head_map
    if case.kernel == SMALLK:       # the geometry the row is named for
        total = case.B * case.H * -(-case.Nq // 32)
        assert case.bpw == 4 * min(4, max(1, total // 2048))


def test_small_nk_blocks_per_workgroup():
    """One to four 32-query blocks per wave from B H ceil(Nq / 32) / 2048, and what the two new GPU cases are there for: a last
    workgroup that is not whole."""
    from edtr_amd import ops
    plan = lambda *a, **k: ops.flash_attn_plan_shape(torch.bfloat16, *a, **k)
    assert plan(8, 20, 256, 77, prescaled=True) == (SMALLK, 4)          # 16x16 latents at batch 8: 1280 blocks
    assert plan(8, 5, 4096, 77, prescaled=True) == (SMALLK, 8)          # 64x64 latents at batch 8: 5120 blocks, two per wave
    assert plan(1, 1, 32 * 2047, 77) == (SMALLK, 4) and plan(1, 1, 32 * 2048, 77) == (SMALLK, 4)      # 2047, 2048 blocks: 0 and 1 -> 1
    assert plan(1, 1, 32 * 4095, 77) == (SMALLK, 4) and plan(1, 1, 32 * 4096, 77) == (SMALLK, 8)
    assert plan(1, 1, 32 * 6144, 77) == (SMALLK, 12) and plan(1, 1, 32 * 8192, 77) == (SMALLK, 16) and plan(1, 3, 32 * 8192, 77) == (SMALLK, 16)
    nblk = -(-4123 // 32)
    assert nblk % 8 == 1 and -(-6170 // 32) % 12 == 1                    # both GPU cases end in a workgroup with a single block


def test_thresholds_between_the_kernels():
    from edtr_amd import ops
    plan = lambda *a, **k: ops.flash_attn_plan_shape(torch.float16, *a, **k)[0]
    # the large-N kernel: prescaled, not causal, Nq >= 2048, whole unrolled trips of 256 keys
    assert plan(1, 8, 2047, 256, prescaled=True) == GENERIC and plan(1, 8, 2048, 256, prescaled=True) == V3
    assert plan(1, 8, 2048, 256) == GENERIC                                              # unscaled scores
    assert plan(1, 8, 2048, 2048, prescaled=True, causal=True) == GENERIC
    assert plan(1, 8, 2048, 320, prescaled=True) == GENERIC and plan(1, 8, 2048, 192, prescaled=True) == GENERIC
    assert plan(1, 8, 4096, 768, prescaled=True) == V3 and plan(1, 8, 4096, 4096, prescaled=True) == V3
    # the small-Nk kernel: Nk <= 128, not causal (prescaled or not); Nk = 128 with Nq >= 2048 stays below the large-N kernel's 256
    assert plan(2, 4, 300, 128) == SMALLK and plan(2, 4, 300, 129) == GENERIC
    assert plan(2, 4, 4096, 128, prescaled=True) == SMALLK and plan(2, 4, 4096, 129, prescaled=True) == GENERIC
    assert plan(1, 16, 77, 77) == SMALLK and plan(1, 16, 77, 77, causal=True) == GENERIC
    # split operands go to their own kernels whatever the shape
    assert plan(*attn_cases.SPLIT_SHAPE, split=1) == SPLIT_QK and plan(*attn_cases.SPLIT_SHAPE, split=2, out_f32=True) == SPLIT_QKPV
    assert plan(1, 8, 2048, 256, prescaled=True, split=1) == SPLIT_QK and plan(1, 8, 2048, 77, split=2) == SPLIT_QKPV


def _params(**over):
    from edtr_amd import lib, ops
    p = lib.AttnParams()
    B, H, Nq, Nk = 2, 4, 130, 77
    C = H * 64
    p.dtype, p.B, p.H, p.Nq, p.Nk = ops.dt_code(torch.bfloat16), B, H, Nq, Nk
    p.q, p.q_bs, p.q_ld = 0x1000, Nq * C, C
    p.k, p.k_bs, p.k_ld = 0x1000, Nk * C, C
    p.vt, p.vt_bs, p.vt_ld = 0x1000, C * 80, 80
    p.out, p.o_bs, p.o_ld = 0x1000, Nq * C, C
    p.scale = 0.125
    for name, value in over.items():
        setattr(p, name, value)
    return p


def test_rejects_answer_the_launch_error_codes():
    """Every reject of edtr_flash_attn64, from the plan and (nothing is launched on an error, so no device is needed) from the launch
    itself: the same code."""
    from edtr_amd import lib
    handle = lib.load()

    def both(**over):
        p = _params(**over)
        bpw = ctypes.c_int32(99)
        code = handle.edtr_flash_attn64_plan(ctypes.byref(p), ctypes.byref(bpw))
        assert code < 0 and bpw.value == 0
        assert handle.edtr_flash_attn64_plan(ctypes.byref(p), None) == code         # the pointer is optional
        assert handle.edtr_flash_attn64(ctypes.byref(p), None) == code
        return code

    assert handle.edtr_flash_attn64_plan(None, None) == E_NULL and handle.edtr_flash_attn64(None, None) == E_NULL
    assert handle.edtr_flash_attn64_plan(ctypes.byref(_params()), None) == SMALLK             # the case itself is a valid launch
    assert both(q=None) == E_NULL and both(out=None) == E_NULL
    assert both(dtype=2) == E_DTYPE
    assert both(Nq=0) == E_SHAPE and both(B=0) == E_SHAPE
    assert both(causal=1) == E_SHAPE                                                       # causal with Nq != Nk
    assert both(vt_ld=72) == E_SHAPE                                                       # V^T rows shorter than round_up(Nk, 8)
    assert both(q_ld=4 * 64 + 4) == E_ALIGN and both(k_ld=4 * 64 + 2) == E_ALIGN and both(vt_ld=84) == E_ALIGN and both(o_ld=4 * 64 + 4) == E_ALIGN
    assert both(q_bs=130 * 256 + 4) == E_ALIGN and both(o_bs=130 * 256 + 1) == E_ALIGN
    assert both(q=0x1008) == E_ALIGN and both(vt=0x1002) == E_ALIGN
    assert both(out_f32=1) == E_UNSUPPORTED                                                # fp32 output without split operands
    assert both(vt_lo=0x1000) == E_UNSUPPORTED                                             # vt_lo without q_lo / k_lo
    assert both(q_lo=0x1000) == E_NULL                                                     # q and k are split together
    assert both(q_lo=0x1000, k_lo=0x1008) == E_ALIGN
    assert both(q_lo=0x1000, k_lo=0x1000, out_f32=1, o_ld=4 * 64 + 2) == E_ALIGN           # fp32 rows: whole 16-byte pieces
    assert both(Nk=1 << 20, vt_ld=1 << 20, k_ld=1 << 11) == E_UNSUPPORTED                  # K slice beyond 32-bit buffer offsets
