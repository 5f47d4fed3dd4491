"""The 1x1 skip convolution of a width-changing ResBlock as a K tail of conv2 (edtr_hip.h: a3 / C3 / ld3): the host side, checked
without a GPU — the ABI of the three fields, the packed [9*Cin | C3] weight with its summed bias, edtr_igemm_plan's answers, and
the programs the emitters build with and without the tail."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, SHAPE = -5, -2


def test_error_codes_match_the_header():
    text = open(os.path.join(ROOT, "include", "edtr_hip.h")).read()
    import re
    codes = dict(re.findall(r"\b(EDTR_E_[A-Z]+)\s*=\s*(-?\d+)", text))
    assert int(codes["EDTR_E_UNSUPPORTED"]) == UNSUPPORTED and int(codes["EDTR_E_SHAPE"]) == SHAPE


def test_tail_fields_match_the_c_layout(tmp_path):
    from edtr_amd import lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edtr_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",'
                   'sizeof(edtr_igemm_params),offsetof(edtr_igemm_params,gn_ld),offsetof(edtr_igemm_params,a3),'
                   'offsetof(edtr_igemm_params,C3),offsetof(edtr_igemm_params,ld3));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = lib.IgemmParams
    assert out == [ctypes.sizeof(P), P.gn_ld.offset, P.a3.offset, P.C3.offset, P.ld3.offset]
    assert P.a3.offset > P.gn_ld.offset and [n for n, _ in P._fields_][-3:] == ["a3", "C3", "ld3"], "appended: the ABI version stays 10"
    assert lib.load().edtr_abi_version() == 10


def test_packed_tail_weight_and_summed_bias():
    from edtr_amd.engine import WeightStore
    g = torch.Generator().manual_seed(5)
    N, Cin, C3 = 24, 16, 40
    params = {"c.weight": torch.randn(N, Cin, 3, 3, generator=g), "c.bias": torch.randn(N, generator=g),
              "s.weight": torch.randn(N, C3, 1, 1, generator=g), "s.bias": torch.randn(N, generator=g)}
    for dt in (torch.bfloat16, torch.float16):
        store = WeightStore(params, dt, torch.device("cpu"))
        ref, bias = store.conv_tail("c.", "s.")
        w = ref.get()
        assert ref.shape == (N, 9 * Cin + C3) and tuple(w.shape) == ref.shape and w.dtype == dt and w.stride(0) == 9 * Cin + C3
        assert torch.equal(w[:, 9 * Cin:], params["s.weight"][:, :, 0, 0].to(dt))                  # column 9*Cin + c of row n = W_skip[n, c]
        assert torch.equal(w[:, :9 * Cin].reshape(N, 3, 3, Cin), params["c.weight"].permute(0, 2, 3, 1).to(dt))
        assert torch.equal(w[:, :9 * Cin], store.conv("c.")[0].get())
        assert bias.dtype == torch.float32 and torch.equal(bias, params["c.bias"] + params["s.bias"])
        # input channels padded to the activation's width: the tail still starts at column 9 * Cin_p
        w2 = store.conv_tail("c.", "s.", cin_pad=32, tail_pad=64)[0].get()
        assert tuple(w2.shape) == (N, 9 * 32 + 64) and torch.equal(w2[:, 9 * 32:9 * 32 + C3], params["s.weight"][:, :, 0, 0].to(dt))
        assert not w2[:, 9 * 32 + C3:].any() and not w2[:, :9 * 32].reshape(N, 9, 32)[:, :, Cin:].any()


def test_plan_takes_a_tail_on_the_halo_tiles_only():
    """edtr_igemm_plan (no device) for the headline's shapes: tile 16 (8 x 8 images with split-K, 16 x 16 patches), tile 20, tile 17
    (also with the fused input GroupNorm) — and UNSUPPORTED wherever another tile would run, or the geometry is not the plain one."""
    from edtr_amd import ops
    bf = torch.bfloat16
    plan = ops.ktail_plan
    assert plan(bf, 8, 8, 8, 1280, 1280, 1280, 2560, 2560, splitk=10) == 16         # 8 x 8 level, four images per workgroup
    assert plan(bf, 8, 16, 16, 1280, 1280, 1280, 1920, 1920, splitk=2) == 16
    assert plan(bf, 8, 32, 32, 640, 640, 640, 320, 320) == 16
    assert plan(torch.float16, 8, 32, 32, 640, 640, 640, 1920, 1920) == 16
    assert plan(bf, 8, 64, 64, 320, 320, 320, 960, 960) == 20                       # one 160-column unit per CU
    assert plan(bf, 8, 512, 512, 128, 128, 128, 256, 256) == 17 and plan(bf, 8, 512, 512, 128, 128, 128, 256, 256, a_gn=True) == 17
    assert plan(bf, 8, 256, 256, 256, 256, 256, 512, 512) == 17
    assert plan(bf, 8, 32, 32, 640, 640, 640, 320, 512) == 16                       # a column slice of a wider tensor (ld3 > C3)
    assert plan(bf, 8, 32, 32, 640, 640, 640, 320 + 32, 512) < 0                    # C3 % 64
    assert plan(bf, 8, 32, 32, 640, 640, 640, 320, 256) == SHAPE                    # ld3 < C3
    assert plan(bf, 2, 32, 32, 128, 128, 128, 64, 64) == UNSUPPORTED                # 8 units: the 128 x 128 loop would run
    assert plan(bf, 8, 32, 32, 640, 640, 640, 320, 320, a_gn=True) == UNSUPPORTED   # tile 16 normalises no tail operand apart

    def explicit(**kw):
        return ops.conv3x3_plan(8, 32, 32, 128, 128, tail=(64, 64), raw=kw)

    assert explicit(tile=16) == 16 and explicit(tile=0) == UNSUPPORTED               # (32 units: the automatic choice is the 128 x 128 loop)
    for t in (1, 2, 3, 6, 8, 14, 21):
        assert explicit(tile=t) == UNSUPPORTED, t
    assert explicit(tile=16, upsample2x=1, IH=16, IW=16) == UNSUPPORTED
    assert explicit(tile=16, stride=2, OH=16, OW=16, M=8 * 16 * 16) == UNSUPPORTED
    assert explicit(tile=16, a2=0x1000, C2=64, ld2=64, K=9 * 192 + 64) == UNSUPPORTED
    assert explicit(tile=16, C3=72, ld3=72, K=9 * 128 + 72, ldw=9 * 128 + 72) == UNSUPPORTED
    assert explicit(tile=16, K=9 * 128) == SHAPE                                    # K must count the tail
    assert explicit(tile=16, a3=None, K=9 * 128) == 16 and explicit(tile=16, C3=0, K=9 * 128) == 16      # no tail: the launch as it was


@pytest.fixture(scope="module")
def programs():
    """One ControlNet + UNet evaluation and one VAE decode, built on the CPU (no launch) at a size where tile 16 takes the 32 x 32
    level of the tiny configuration (16 images: 64 units of 256 pixels x 128 channels)."""
    from edtr_amd import synth
    from edtr_amd.model.cldm import CldmEngine
    from edtr_amd.testing import build_synthetic_cldm
    cfg = synth.tiny_config()
    out = {}
    old = os.environ.get("EDTR_KTAIL")
    try:
        for prec in ("fast", "mixed", "high"):
            for sw in ("1", "0"):
                os.environ["EDTR_KTAIL"] = sw
                cldm = build_synthetic_cldm(cfg, "cpu", torch.bfloat16, precision=prec)
                out[prec, sw] = CldmEngine(cldm, 16, 64, 64, 77).step_prog.recs
    finally:
        if old is None:
            os.environ.pop("EDTR_KTAIL", None)
        else:
            os.environ["EDTR_KTAIL"] = old
    return out


def _sig(recs):
    return [(r.name, r.tag) for r in recs]


def test_fast_program_folds_the_skips_the_plan_allows(programs):
    from edtr_amd import ops
    on, off = programs["fast", "1"], programs["fast", "0"]
    n_skip = sum(r.name == "res.skip1x1" for r in off)
    assert n_skip >= 8 and not any(" kt" in r.tag for r in off)
    fused = [r for r in on if " kt" in r.tag]
    left = [i for i, r in enumerate(on) if r.name == "res.skip1x1"]
    assert fused and len(fused) + len(left) == n_skip and len(on) == len(off) - len(fused)
    for r in fused:
        p = r.keep[0]
        assert r.name == "res.conv2" and not p.residual and p.a3 and p.C3 % 64 == 0 and p.K == 9 * p.C1 + p.C3 and p.ldw == p.K
        assert r.flops == 2.0 * p.M * p.N * (9 * p.C1 + p.C3)                      # the algorithmic FLOP of both convolutions
    for i in left:      # a skip that kept its launch: the plan refuses a tail for the conv2 that follows it
        conv2 = next(r for r in on[i + 1:] if r.name == "res.conv2")
        p, s = conv2.keep[0], on[i].keep[0]
        assert p.residual and " kt" not in conv2.tag
        assert s.C1 % 64 or p.C1 % 64 or ops.ktail_plan(torch.bfloat16, p.M // (p.OH * p.OW), p.OH, p.OW, p.C1, p.ld1, p.N, s.C1, s.ld1,
                                                       max(p.splitk, 1), bool(p.a_gn)) < 0
    # the FLOP the roofline counts do not move
    assert sum(r.flops for r in on) == pytest.approx(sum(r.flops for r in off), rel=1e-12)


def test_switch_off_is_the_program_as_it_was(programs):
    off = programs["fast", "0"]
    assert not any(" kt" in r.tag for r in off) and all(not r.keep[0].a3 for r in off if r.name.startswith("res.conv"))
    skips = [r for r in off if r.name == "res.skip1x1"]
    conv2 = [r for r in off if r.name == "res.conv2"]
    assert skips and all(r.keep[0].residual for r in conv2)


def test_parity_modes_do_not_move(programs):
    for prec in ("mixed", "high"):
        assert _sig(programs[prec, "1"]) == _sig(programs[prec, "0"])
        assert not any(" kt" in r.tag for r in programs[prec, "1"])
    assert all(" 2w" in r.tag for r in programs["mixed", "1"] if r.name == "res.skip1x1")


def test_fast_section_of_the_hybrid_mode_keeps_its_skips():
    from edtr_amd import synth
    from edtr_amd.model.cldm import CldmEngine
    from edtr_amd.testing import build_synthetic_cldm
    cldm = build_synthetic_cldm(synth.tiny_config(), "cpu", torch.bfloat16, precision="hybrid")
    recs = CldmEngine(cldm, 16, 64, 64, 77).step_prog.recs
    assert any(r.name == "res.skip1x1" for r in recs) and not any(" kt" in r.tag for r in recs)
