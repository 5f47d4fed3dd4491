"""The launch geometries of edtr_flash_attn64 that a batch-8 run takes and the kernel tests reach, one table for the GPU cases
(tests/test_gpu_ops.py: test_flash_attn64_launch_geometry) and the device-free plan check (tests/test_attn_plan_cpu.py).  Each row is the
smallest shape that reaches its branch of edtr_amd/csrc/attention.hip; `kernel` / `bpw` are what edtr_flash_attn64_plan must answer
(ids of include/edtr_hip.h: enum edtr_attn_kernel), `head_map` whether B * H % 8 == 0 is the point of the row (the generic and the
large-N kernel then deal heads, not query blocks, to the XCDs)."""
from collections import namedtuple

GENERIC, SPLIT_QK, SPLIT_QKPV, SMALLK, V3 = 1, 2, 3, 4, 5

Case = namedtuple("Case", "name B H Nq Nk kernel bpw head_map causal prescaled")


def _c(name, B, H, Nq, Nk, kernel, bpw=0, head_map=None, causal=False, prescaled=False):
    return Case(name, B, H, Nq, Nk, kernel, bpw, head_map, causal, prescaled)


CASES = [
    _c("generic-headmap", 2, 4, 300, 203, GENERIC, head_map=True),                       # nqb = 3, ragged Nq, Nk % 8 != 0, scale 0.125
    _c("generic-headmap-batch-stride", 8, 1, 129, 136, GENERIC, head_map=True),          # H = 1: b = bh
    _c("generic-headmap-causal-clip", 1, 16, 77, 77, GENERIC, head_map=True, causal=True),
    _c("generic-headmap-causal-130", 1, 8, 130, 130, GENERIC, head_map=True, causal=True),
    _c("generic-prescaled-headmap", 4, 2, 2048, 320, GENERIC, head_map=True, prescaled=True),     # Nk % 256 != 0 falls back from v3
    _c("v3-headmap-one-trip", 1, 8, 2048, 256, V3, head_map=True, prescaled=True),
    _c("v3-plain-one-trip", 1, 3, 2048, 256, V3, head_map=False, prescaled=True),
    _c("v3-headmap-three-trips-ragged", 2, 4, 2100, 768, V3, head_map=True, prescaled=True),      # store predicate on the last query block
    _c("smallk-2-per-wave-partial-wg", 4, 8, 4123, 77, SMALLK, bpw=8, prescaled=True),            # 129 blocks: 17 workgroups, the last has one
    _c("smallk-3-per-wave", 4, 8, 6170, 100, SMALLK, bpw=12),                                      # unscaled scores; keys end inside the fourth block of 32
]
SPLIT_SHAPE = (2, 4, 130, 77)       # the split-operand kernels (q_lo / k_lo, and with vt_lo + out_f32)
