"""edtr_igemm's tile planner (edtr_amd/csrc/igemm_plan.h), pinned without a GPU.  A deterministic generator builds edtr_igemm_params cases
(placeholder pointers; edtr_igemm_plan touches no memory and makes no HIP call); tools/make_plan_table.py recorded the answers of the
commit BEFORE the planner was separated from the launches in tests/golden/igemm_plan_table.json, and every case must still answer the
same: the tile number, or the exact error code.  The table's own coverage (which tiles it chooses, which rules it pins by a pair of
cases that differ in that rule's input alone) is asserted on the RECORDED answers, so it holds for the old code by itself.

Run as a program this file answers the cases it reads from stdin (one per line, the parameter struct's bytes as hex) with one JSON
list: the fresh child process of the environment switches, which the planner reads once per process (the recording tool uses the
same child, with EDTR_AMD_LIB = the old build)."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TABLE = os.path.join(ROOT, "tests", "golden", "igemm_plan_table.json")
BREAKDOWN = os.path.join(ROOT, "profiles", "r06", "bench_det512_b8_bf16.breakdown.json")
LIVE_TILES = (1, 2, 3, 6, 8, 14, 16, 17, 20, 21)
E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_UNSUPPORTED = -1, -2, -3, -4, -5
PTR = 0x10000           # a 16-byte aligned placeholder: the planner looks at addresses, never through them
GEGLU, SILU, LRELU = 1, 2, 4

# the rules every one of which the table must pin by a pair of cases (names = the tags of pair() in generate())
RULES = [
    # validation
    "v.ptr.a1", "v.ptr.w", "v.ptr.out", "v.taps", "v.K_sum", "v.taps9_not_spatial", "v.M_mod_OHOW", "v.upsample_range", "v.act_range",
    "v.lrelu_slope", "v.rowvec_rows_per_image", "v.mult8.K_C1", "v.mult8.C2", "v.mult8.N", "v.mult8.ld1", "v.mult8.ld2", "v.mult8.ldw",
    "v.geglu_N64", "v.align.operand", "v.align.zstride", "v.n_valid", "v.residual_Z", "v.rowvec_Z", "v.splitk.Z", "v.splitk.geglu",
    "v.splitk.workspace", "v.splitk.max", "v.vt_out", "v.row_stats", "v.ln_stats", "v.ktail",
    # choice
    "c.dma_ok", "c.200_tiles", "c.tile8.N160", "c.tile8.200_tiles", "c.tile8.N128_or_K640", "c.tile6.K1024", "c.tile6.120_tiles",
    "c.tile6.fill", "c.tile16.48_units", "c.ragged16.48_units", "c.ragged16.256_units", "c.ragged16.N128", "c.ragged16.splitk",
    "c.tile14.N32", "c.tile14.M65536", "c.tile17.units", "c.tile20.whole_rounds", "c.tile20.tail", "c.a_gn.force16", "c.a_gn.keep17",
    "c.a_gn.tile21", "c.a_gn.img8", "c.out16", "c.a_wrap.fallback3", "c.subpixel.force16", "c.vt_out.col0_128", "c.vt_out.col0_160",
    "c.ln_stats.fallback", "c.row_stats.fallback", "c.geglu.2_to_1",
    # admission
    "a.dma_ok.tile3", "a.dma_ok.chunk32", "a.a3.tiles", "a.gn_partial.splitk", "a.gn_partial.no_splitk", "a.unknown_tile", "a.fast.6",
    "a.fast.8", "a.fast.14", "a.splitk.6", "a.geglu.6", "a.geglu.8", "a.geglu.14", "a.tile21.out_f32", "a.tile21.residual",
    "a.tile21.rowvec", "a.tile21.N512", "a.tile21.chunks",
]
# the K-tail form of tile 8's `ksel >= 640` and tile 6's `ksel >= 1024` (the 9-tap product, not K, is compared) has no pair: a tail is
# accepted by the halo tiles only, and wherever a halo tile is eligible it overrides tiles 6 and 8 whichever way that comparison went


# ---- case builders: a case is a dict of edtr_igemm_params fields -------------------------------------------------------------------
def gemm(M, N, K, **kw):
    d = dict(dtype=0, taps=1, M=M, N=N, K=K, Z=1, zdiv=1, a1=PTR, C1=K, ld1=K, w=PTR, ldw=K, alpha=1.0, out=PTR, ldc=N)
    d.update(kw)
    return d


def conv(B, H, W, C1, N, stride=1, ups=0, **kw):
    up = 2 if ups else 1
    OH, OW = H * up // stride, W * up // stride
    d = dict(dtype=0, taps=9, M=B * OH * OW, N=N, K=9 * C1, Z=1, zdiv=1, a1=PTR, C1=C1, ld1=C1, w=PTR, ldw=9 * C1, alpha=1.0, out=PTR,
             ldc=N, IH=H, IW=W, OH=OH, OW=OW, stride=stride, pad_t=1, pad_l=1, upsample2x=ups, rows_per_image=OH * OW)
    if ups == 2:
        d.update(ldw=4 * C1, w_phase_stride=N * 4 * C1)
    d.update(kw)
    return d


def _rpi(d):
    return d["OH"] * d["OW"] if d.get("OH") else d["M"]


# features: each returns a changed copy
def f_splitk(d, n=2):
    return dict(d, splitk=n, workspace=PTR, workspace_bytes=n * d["M"] * d["N"] * 4)


def f_tail(d, C3=64):
    return dict(d, a3=PTR, C3=C3, ld3=C3, K=d["K"] + C3, ldw=d["K"] + C3)


def f_gnp(d):
    return dict(d, gn_partial=PTR)


def f_gnin(d):
    return dict(d, a_gn=PTR, a_gn_silu=1)


def f_res(d):
    return dict(d, residual=PTR, ldr=d["N"])


def f_rowvec(d):
    return dict(d, rowvec=PTR, rowvec_ld=d["N"], rows_per_image=_rpi(d))


def f_vt(d, col0=None):
    return dict(d, vt_out=PTR, vt_col0=d["N"] * 2 // 3 if col0 is None else col0, vt_ld=_rpi(d), rows_per_image=_rpi(d), vt_alpha=1.0)


def f_rs(d):
    return dict(d, row_stats=PTR)


def f_ln(d):
    return dict(d, ln_stats=PTR, ln_slots=d["K"] // 32, ln_C=d["K"], ln_eps=1e-5, ln_c1=PTR, ln_c2=PTR)


def f_geglu(d):
    return dict(d, act=GEGLU, ldc=d["N"] // 2)


def f_silu(d):
    return dict(d, act=SILU)


def f_f32(d):
    return dict(d, out_f32=1)


def f_out16(d):
    return dict(d, out_f32=1, out16=PTR, ld16=d["N"])


def f_wrap(d):
    return dict(d, a_wrap=d["K"], K=2 * d["K"], C1=2 * d["K"], ldw=2 * d["K"])


def f_bias(d):
    return dict(d, bias_n=PTR)


def _both(f, g):
    return lambda d: g(f(d))


N_SINGLE = 17          # FEATURES[:N_SINGLE] are the single features, the rest pairs
FEATURES = [
    ("", lambda d: d), ("splitk", f_splitk), ("splitk3", lambda d: f_splitk(d, 3)), ("tail", f_tail), ("gnp", f_gnp), ("gnin", f_gnin),
    ("res", f_res), ("rowvec", f_rowvec), ("vt", f_vt), ("rs", f_rs), ("ln", f_ln), ("geglu", f_geglu), ("silu", f_silu), ("f32", f_f32),
    ("out16", f_out16), ("wrap", f_wrap), ("bias", f_bias),
    # the pairs the rules mention together
    ("gnin+tail", _both(f_gnin, f_tail)), ("gnin+splitk", _both(f_gnin, f_splitk)), ("gnp+splitk", _both(f_gnp, f_splitk)),
    ("tail+splitk", _both(f_tail, f_splitk)), ("vt+ln", _both(f_vt, f_ln)), ("rs+vt", _both(f_rs, f_vt)), ("wrap+ln", _both(f_wrap, f_ln)),
    ("out16+vt", _both(f_out16, f_vt)), ("geglu+splitk", _both(f_geglu, f_splitk)), ("gnp+gnin", _both(f_gnp, f_gnin)),
    ("rs+ln", _both(f_rs, f_ln)), ("gnp+tail", _both(f_gnp, f_tail)), ("res+rowvec", _both(f_res, f_rowvec)),
]


def _isqrt(n):
    r = int(round(n ** 0.5))
    return r if r * r == n else 0


def _profile_shapes():
    """The igemm tags of the committed batch-8 breakdown ("taps9 M32768 N320 K2880 Z1 s2 sk2 gnp"), as cases (batch 8, square images)."""
    with open(BREAKDOWN) as fh:
        tags = list(json.load(fh)["by_shape"])
    out = []
    for tag in tags:
        t = tag.split()
        if not t[0].startswith("taps"):
            continue
        taps, M, N, K, Z = int(t[0][4:]), int(t[1][1:]), int(t[2][1:]), int(t[3][1:]), int(t[4][1:])
        flags = t[5:]
        if taps == 9:
            ups = 2 if "up2sp" in flags else (1 if "up2" in flags else 0)
            stride = 2 if "s2" in flags else 1
            side = _isqrt(M // 8)
            assert side and K % 9 == 0, tag
            src = side * stride // (2 if ups else 1)
            d = conv(8, src, src, K // 9, N, stride=stride, ups=ups)
            assert d["M"] == M, tag
        else:
            d = gemm(M, N, K, Z=Z)
            if Z > 1:
                d.update(a_zs_outer=M * K, w_zs_outer=N * K, o_zs_outer=M * N)
        for fl in flags:
            if fl.startswith("sk"):
                d = f_splitk(d, int(fl[2:]))
            elif fl.startswith("act"):
                d = f_geglu(d) if fl == "act1" else dict(d, act=int(fl[3:]))
            elif fl == "f32":
                d = f_f32(d)
            elif fl == "gnp":
                d = dict(f_gnp(d), gn_slot_rows=64 if d.get("OH") == 8 and d.get("splitk", 0) > 1 else 0)
            elif fl == "vT":
                d = f_vt(d)
            elif fl == "gnin":
                d = f_gnin(d)
        out.append(d)
    return out


def _named_shapes():
    """The shape lists of tests/test_host_logic.py (launch predicates, tile 21) and tests/test_ktail_cpu.py, plus what no list names but
    a tile needs to be chosen at all (tiles 1, 2, 14, the gathered-upsample and 8 x 8-image halo geometries)."""
    out = []
    for (B, H, W, cin, N) in [(8, 512, 512, 128, 128), (8, 1024, 1024, 128, 128), (8, 1024, 1024, 256, 128), (1, 64, 64, 64, 128), (4, 32, 32, 128, 128),
                              (8, 16, 16, 1280, 128), (8, 256, 256, 256, 256), (2, 16, 16, 192, 128), (3, 64, 64, 64, 128), (8, 64, 48, 128, 128),
                              (8, 2048, 1024, 128, 128)]:
        out += [conv(B, H, W, cin, N), conv(B, H, W, cin, N, ld1=2 * cin)]
    for (B, H, W, Ce, N) in [(8, 256, 256, 256, 256), (8, 128, 128, 512, 512), (8, 32, 32, 640, 640), (2, 16, 16, 64, 128), (8, 512, 512, 768, 128),
                             (8, 1024, 1024, 384, 128)]:
        out += [conv(B, H, W, Ce, N, ups=2), conv(B, H, W, Ce, N, ups=2, ld1=3 * Ce), conv(B, H, W, Ce, N, ups=1)]
    for (cin, N, H, W) in [(64, 128, 512, 512), (128, 256, 512, 512), (96, 128, 512, 512), (64, 128, 512, 528), (64, 640, 512, 512)]:
        out.append(conv(1, H, W, cin, N))
    for (B, H, W, C1, N, C3) in [(8, 8, 8, 1280, 1280, 2560), (8, 16, 16, 1280, 1280, 1920), (8, 32, 32, 640, 640, 320), (8, 32, 32, 640, 640, 1920),
                                 (8, 64, 64, 320, 320, 960), (8, 512, 512, 128, 128, 256), (8, 256, 256, 256, 256, 512), (2, 32, 32, 128, 128, 64),
                                 (8, 32, 32, 128, 128, 64)]:
        out.append(f_tail(conv(B, H, W, C1, N), C3))
    out += [f_splitk(f_tail(conv(8, 8, 8, 1280, 1280), 2560), 10), f_splitk(f_tail(conv(8, 16, 16, 1280, 1280), 1920), 2)]
    # tile 1 / 2: operands the LDS-DMA loops cannot take (a channel concat, C1 no multiple of 64), many and few 128 x 128 tiles
    for (M, N, K) in [(32768, 320, 72), (32768, 128, 96), (1024, 128, 96), (256, 64, 32), (65536, 256, 200), (2048, 1280, 840), (512, 96, 160)]:
        out.append(gemm(M, N, K))
    for (B, H, W, C1, C2, N) in [(8, 64, 64, 320, 320, 320), (8, 16, 16, 1280, 640, 1280), (1, 16, 16, 64, 64, 64), (2, 8, 8, 128, 64, 128)]:
        out.append(conv(B, H, W, C1, N, a2=PTR, C2=C2, ld2=C2, K=9 * (C1 + C2), ldw=9 * (C1 + C2)))
    for (B, H, W, C1, N) in [(1, 24, 24, 8, 64), (8, 64, 64, 8, 320), (8, 512, 512, 8, 128), (1, 40, 40, 24, 24)]:
        out.append(conv(B, H, W, C1, N))
    # tile 14: skinny N, large M
    for (B, H, W, C1, N) in [(8, 512, 512, 128, 8), (8, 512, 512, 128, 32), (1, 256, 256, 64, 16), (8, 256, 256, 256, 24), (2, 512, 512, 64, 8)]:
        out.append(conv(B, H, W, C1, N))
    out += [gemm(65536, 32, 64), gemm(131072, 8, 128), gemm(262144, 16, 256)]
    # halo geometries 1 (nearest-2x gather) and 2 (four whole 8 x 8 images per workgroup)
    for (B, H, W, C1, N) in [(8, 8, 8, 1280, 1280), (8, 16, 16, 1280, 640), (8, 32, 32, 640, 640), (48, 8, 8, 128, 128), (8, 64, 64, 256, 128)]:
        out.append(conv(B, H, W, C1, N, ups=1))
    for (B, C1, N, sk) in [(8, 1280, 1280, 10), (8, 1280, 1280, 6), (16, 640, 1280, 3), (64, 128, 128, 2), (192, 128, 128, 1), (256, 64, 256, 1)]:
        d = conv(B, 8, 8, C1, N)
        out.append(f_splitk(d, sk) if sk > 1 else d)
    # ragged-N halo tile: N = 320 = 2.5 column tiles, at most one round of units
    for (B, H, W, C1, N) in [(4, 64, 64, 320, 320), (2, 64, 64, 640, 320), (16, 16, 16, 320, 320), (4, 32, 32, 128, 192)]:
        out.append(conv(B, H, W, C1, N))
    # large transformer GEMMs (tile 6 / 8) and a z-batched one
    for (M, N, K) in [(32768, 512, 1024), (32768, 1024, 2048), (16384, 416, 1024), (8192, 640, 640), (8192, 5120, 640), (4096, 2560, 1280),
                      (32768, 320, 320), (16384, 960, 320), (2048, 1280, 5120)]:
        out.append(gemm(M, N, K))
    out.append(gemm(4096, 512, 1024, Z=8, a_zs_outer=4096 * 1024, w_zs_outer=512 * 1024, o_zs_outer=4096 * 512))
    return out


def generate():
    """-> (cases, pairs): the list of case dicts and {rule: [(index a, index b), ...]} of cases that differ in that rule's input alone."""
    cases, pairs = [], {}

    def add(d):
        cases.append(d)
        return len(cases) - 1

    def pair(rule, a, b):
        pairs.setdefault(rule, []).append((add(a), add(b)))

    # the cross, thinned to what a 200-KB table holds: every feature set on the automatic choice in both dtypes; every live tile plain
    # in both dtypes; every single feature on every explicit tile in bf16, on every third shape (which third rotates with the tile)
    shapes = _profile_shapes() + _named_shapes()
    for si, d in enumerate(shapes):
        for dtype in (0, 1):
            for tile in (0,) + LIVE_TILES:
                feats = FEATURES if tile == 0 else (FEATURES[:N_SINGLE] if dtype == 0 and (si + tile) % 3 == 0 else FEATURES[:1])
                for _, f in feats:
                    add(dict(f(d), dtype=dtype, tile=tile))

    for dtype in (0, 1):
        def G(*a, **kw):
            return gemm(*a, dtype=dtype, **kw)

        def C(*a, **kw):
            return conv(*a, dtype=dtype, **kw)

        g, c = G(8192, 640, 640), C(8, 32, 32, 128, 128)
        # ---- validation
        for f in ("a1", "w", "out"):
            pair("v.ptr." + f, g, dict(g, **{f: 0}))
            pair("v.ptr." + f, c, dict(c, **{f: 0}))
        pair("v.taps", g, dict(g, taps=3))
        pair("v.taps", g, dict(g, taps=0))
        pair("v.K_sum", g, dict(g, K=648))
        pair("v.K_sum", c, dict(c, K=9 * 128 + 64))
        pair("v.taps9_not_spatial", c, dict(c, OH=0))
        pair("v.M_mod_OHOW", c, dict(c, M=c["M"] + 8))
        pair("v.upsample_range", c, dict(c, upsample2x=3))
        pair("v.upsample_range", g, dict(g, upsample2x=-1))
        pair("v.act_range", g, dict(g, act=5))
        pair("v.act_range", dict(g, act=LRELU, act_slope=0.2), dict(g, act=-1, act_slope=0.2))
        pair("v.lrelu_slope", dict(g, act=LRELU, act_slope=0.2), dict(g, act=LRELU, act_slope=1.5))
        pair("v.lrelu_slope", dict(c, act=LRELU, act_slope=1.0), dict(c, act=LRELU, act_slope=-0.1))
        pair("v.rowvec_rows_per_image", f_rowvec(g), dict(f_rowvec(g), rows_per_image=0))
        pair("v.mult8.K_C1", G(8192, 640, 320), dict(G(8192, 640, 324), ldw=328, ld1=328))      # (K = C1: the two move together)
        pair("v.mult8.C2", dict(g, a2=PTR, C2=64, ld2=64, K=704, ldw=704), dict(g, a2=PTR, C2=68, ld2=72, K=708, ldw=712))
        pair("v.mult8.N", dict(g, ldc=1024), dict(g, N=644, ldc=1024))
        pair("v.mult8.ld1", dict(g, ld1=648), dict(g, ld1=644))
        pair("v.mult8.ld2", dict(g, a2=PTR, C2=64, ld2=64, K=704, ldw=704), dict(g, a2=PTR, C2=64, ld2=68, K=704, ldw=704))
        pair("v.mult8.ldw", dict(g, ldw=648), dict(g, ldw=644))
        pair("v.geglu_N64", dict(f_geglu(G(8192, 128, 640)), ldc=64), dict(f_geglu(G(8192, 96, 640)), ldc=64))
        for f in ("a1", "w", "out"):
            pair("v.align.operand", g, dict(g, **{f: PTR + 8}))
        pair("v.align.operand", f_res(g), dict(f_res(g), residual=PTR + 4))
        pair("v.align.operand", f_bias(g), dict(f_bias(g), bias_n=PTR + 8))
        for f in ("a_zs_outer", "a_zs_inner", "w_zs_outer", "w_zs_inner"):
            pair("v.align.zstride", dict(g, **{f: 8}), dict(g, **{f: 4}))
        pair("v.align.zstride", dict(g, o_zs_outer=4), dict(g, o_zs_outer=2))
        pair("v.n_valid", dict(g, n_valid=640), dict(g, n_valid=648))
        pair("v.n_valid", dict(g, n_valid=0), dict(g, n_valid=-8))
        pair("v.residual_Z", f_res(g), dict(f_res(g), Z=2))
        pair("v.rowvec_Z", f_rowvec(g), dict(f_rowvec(g), Z=2))
        sk = f_splitk(c, 2)
        pair("v.splitk.Z", sk, dict(sk, Z=2))
        gg = dict(f_geglu(G(2048, 1280, 5120)))
        pair("v.splitk.geglu", f_splitk(G(2048, 1280, 5120), 3), f_splitk(gg, 3))
        pair("v.splitk.workspace", sk, dict(sk, workspace=0))
        pair("v.splitk.workspace", sk, dict(sk, workspace_bytes=sk["workspace_bytes"] - 4))
        pair("v.splitk.workspace", sk, dict(sk, workspace=PTR + 8))
        pair("v.splitk.max", f_splitk(G(2048, 1280, 320), 5), f_splitk(G(2048, 1280, 320), 6))
        pair("v.splitk.max", dict(g, splitk=0), dict(g, splitk=-1))
        v = f_vt(dict(G(8192, 1920, 640), rows_per_image=1024), 1280)
        for ch in (dict(Z=2), f_res(v), f_rowvec(v), dict(gn_partial=PTR), dict(out_f32=1), dict(rows_per_image=1020), dict(vt_col0=0),
                   dict(vt_col0=1920), dict(vt_ld=1020), dict(vt_ld=1016), dict(vt_out=PTR + 8), dict(M=8196)):
            pair("v.vt_out", v, dict(v, **ch))
        r = f_rs(g)
        for ch in (dict(Z=2), dict(N=624, ldc=640), dict(row_stats=PTR + 8), f_splitk(r, 2), dict(act=GEGLU)):
            pair("v.row_stats", r, dict(r, **ch))
        ln = f_ln(g)
        for ch in (dict(Z=2), dict(ln_c1=0), dict(ln_c2=0), dict(ln_slots=19), dict(ln_C=0), dict(ln_C=648), dict(ln_stats=PTR + 8),
                   dict(a2=PTR, C2=64, ld2=64, K=704, ldw=704, ln_slots=22), f_splitk(ln, 2)):
            pair("v.ln_stats", ln, dict(ln, **ch))
        pair("v.ln_stats", f_ln(C(8, 32, 32, 128, 128, tile=3)), C(8, 32, 32, 128, 128, tile=3))
        t = dict(f_tail(c), tile=16)
        for ch in (dict(C3=96, ld3=96, K=9 * 128 + 96, ldw=9 * 128 + 96), dict(ld3=56), dict(ld3=68), dict(a3=PTR + 8), dict(ldw=9 * 128),
                   dict(pad_t=0), dict(Z=2), dict(act=GEGLU), dict(M=2 ** 22 * 8, OH=2048, OW=2048, IH=2048, IW=2048, ld3=1024)):
            pair("v.ktail", t, dict(t, **ch))

        # ---- choice
        pair("c.dma_ok", G(32768, 128, 320), G(32768, 128, 328))
        pair("c.dma_ok", G(1024, 128, 128), G(1024, 128, 96))
        pair("c.200_tiles", G(128 * 199, 128, 96), G(128 * 200, 128, 96))
        pair("c.200_tiles", G(128 * 100 - 8, 256, 72), G(128 * 100, 256, 72))
        pair("c.tile8.N160", dict(G(32768, 320, 320), ldc=384), dict(G(32768, 384, 320), ldc=384))
        pair("c.tile8.N160", dict(G(32768, 960, 320), ldc=1024), dict(G(32768, 968, 320), ldc=1024))
        pair("c.tile8.200_tiles", G(128 * 99 + 8, 320, 320), G(128 * 99, 320, 320))
        pair("c.tile8.200_tiles", G(128 * 50, 640, 640), G(128 * 50 - 8, 640, 640))
        pair("c.tile8.N128_or_K640", G(8192, 640, 576), G(8192, 640, 640))
        pair("c.tile8.N128_or_K640", C(8, 32, 32, 64, 640, stride=2), C(8, 32, 32, 128, 640, stride=2))
        pair("c.tile6.K1024", G(32768, 512, 960), G(32768, 512, 1024))
        pair("c.tile6.K1024", C(8, 128, 128, 64, 256, stride=2), C(8, 128, 128, 128, 256, stride=2))
        pair("c.tile6.120_tiles", G(256 * 59 + 8, 512, 1024), G(256 * 59, 512, 1024))
        pair("c.tile6.120_tiles", G(256 * 30, 1024, 2048), G(256 * 30 - 8, 1024, 2048))
        pair("c.tile6.fill", dict(G(32768, 416, 1024), ldc=512), dict(G(32768, 408, 1024), ldc=512))
        pair("c.tile6.fill", dict(G(32768, 208, 1024), ldc=512), dict(G(32768, 200, 1024), ldc=512))
        pair("c.tile16.48_units", C(48, 16, 16, 128, 128), C(47, 16, 16, 128, 128))
        pair("c.tile16.48_units", f_splitk(C(8, 16, 16, 1280, 256), 3), f_splitk(C(8, 16, 16, 1280, 256), 2))
        pair("c.tile16.48_units", C(6, 32, 32, 128, 256), C(5, 32, 32, 128, 256))
        pair("c.ragged16.48_units", C(16, 16, 16, 320, 320), C(15, 16, 16, 320, 320))
        pair("c.ragged16.256_units", C(5, 64, 64, 320, 320), C(6, 64, 64, 320, 320))
        pair("c.ragged16.256_units", C(4, 64, 64, 640, 320), C(8, 64, 64, 640, 320))
        pair("c.ragged16.N128", dict(C(100, 16, 16, 128, 192), ldc=256), dict(C(100, 16, 16, 128, 64), ldc=256))
        pair("c.ragged16.splitk", C(4, 64, 64, 320, 320), f_splitk(C(4, 64, 64, 320, 320), 2))
        pair("c.tile14.N32", dict(G(65536, 32, 64), ldc=64), dict(G(65536, 40, 64), ldc=64))
        pair("c.tile14.N32", dict(C(8, 512, 512, 128, 32), ldc=64), dict(C(8, 512, 512, 128, 48), ldc=64))
        pair("c.tile14.M65536", G(65536, 32, 64), G(65528, 32, 64))
        pair("c.tile14.M65536", C(1, 256, 256, 64, 8), C(1, 256, 240, 64, 8))
        pair("c.tile17.units", C(8, 128, 128, 128, 128), C(7, 128, 128, 128, 128))
        pair("c.tile17.units", C(2, 256, 256, 256, 256), C(1, 256, 256, 256, 256))
        pair("c.tile20.whole_rounds", C(8, 64, 64, 320, 320), C(9, 64, 64, 320, 320))
        pair("c.tile20.whole_rounds", C(16, 64, 64, 320, 320), C(17, 64, 64, 320, 320))
        pair("c.tile20.tail", C(14, 64, 64, 320, 320), C(13, 64, 64, 320, 320))
        pair("c.tile20.tail", C(6, 64, 64, 640, 320), C(10, 64, 64, 640, 320))
        pair("c.a_gn.force16", C(2, 32, 32, 128, 128), f_gnin(C(2, 32, 32, 128, 128)))
        pair("c.a_gn.force16", C(8, 64, 64, 320, 320), f_gnin(C(8, 64, 64, 320, 320)))
        pair("c.a_gn.force16", f_gnin(C(2, 32, 32, 128, 128, tile=16)), f_gnin(C(2, 32, 32, 128, 128, tile=3)))
        pair("c.a_gn.keep17", f_gnin(C(8, 128, 128, 128, 128)), f_gnin(C(7, 128, 128, 128, 128)))
        pair("c.a_gn.keep17", f_gnin(C(8, 128, 128, 128, 128, tile=17)), f_gnin(C(8, 128, 144, 128, 128, tile=17)))
        pair("c.a_gn.tile21", f_gnin(C(8, 128, 128, 128, 128, tile=21)), f_f32(f_gnin(C(8, 128, 128, 128, 128, tile=21))))
        pair("c.a_gn.tile21", f_gnin(C(8, 128, 128, 128, 128, tile=21)), f_gnin(C(8, 128, 128, 96, 128, tile=21)))
        pair("c.a_gn.img8", f_splitk(C(64, 8, 8, 128, 128), 2), f_gnin(f_splitk(C(64, 8, 8, 128, 128), 2)))
        pair("c.a_gn.img8", f_gnin(C(16, 16, 16, 128, 128, tile=16)), f_gnin(C(64, 8, 8, 128, 128, tile=16)))
        o = f_out16(g)
        for ch in (dict(out_f32=0), dict(ld16=644), dict(out16=PTR + 8), dict(Z=2), dict(act=GEGLU), f_vt(o, 320)):
            pair("c.out16", o, dict(o, **ch))
        pair("c.a_wrap.fallback3", G(32768, 512, 1024), dict(G(32768, 512, 1024), a_wrap=512))
        pair("c.a_wrap.fallback3", dict(G(32768, 512, 1024), a_wrap=512, tile=8), dict(G(32768, 512, 1024), a_wrap=512, tile=6))
        pair("c.a_wrap.fallback3", dict(G(32768, 512, 1024), a_wrap=512), dict(G(32768, 512, 1024), a_wrap=448))
        pair("c.subpixel.force16", C(2, 16, 16, 64, 128, ups=1, ldw=256, w_phase_stride=128 * 256), C(2, 16, 16, 64, 128, ups=2))
        pair("c.subpixel.force16", C(2, 16, 16, 64, 128, ups=2, tile=16), C(2, 16, 16, 64, 128, ups=2, tile=3))
        pair("c.subpixel.force16", C(2, 16, 16, 64, 128, ups=2), C(2, 16, 16, 64, 128, ups=2, w_phase_stride=128 * 256 - 8))
        vb = dict(G(8192, 1920, 640), rows_per_image=1024)
        pair("c.vt_out.col0_160", f_vt(vb, 1280), f_vt(vb, 1024))
        pair("c.vt_out.col0_128", f_vt(vb, 1024), f_vt(vb, 1000))
        pair("c.vt_out.col0_128", f_vt(dict(vb, tile=3), 1280), f_vt(dict(vb, tile=3), 1120))
        pair("c.vt_out.col0_160", f_vt(dict(vb, tile=8), 1280), f_vt(dict(vb, tile=8), 1024))
        pair("c.ln_stats.fallback", G(32768, 320, 320), f_ln(G(32768, 320, 320)))
        pair("c.ln_stats.fallback", G(32768, 512, 1024), f_ln(G(32768, 512, 1024)))
        pair("c.ln_stats.fallback", G(512, 96, 160), f_ln(G(512, 96, 160)))
        pair("c.ln_stats.fallback", f_ln(G(32768, 320, 320, tile=3)), f_ln(G(32768, 320, 320, tile=8)))
        pair("c.row_stats.fallback", G(32768, 512, 1024), f_rs(G(32768, 512, 1024)))
        pair("c.row_stats.fallback", C(8, 32, 32, 128, 128), f_rs(C(8, 32, 32, 128, 128)))
        pair("c.row_stats.fallback", f_rs(G(32768, 512, 1024, tile=8)), f_rs(G(32768, 512, 1024, tile=6)))
        pair("c.geglu.2_to_1", dict(G(512, 128, 160), ldc=128), dict(f_geglu(G(512, 128, 160)), ldc=128))
        pair("c.geglu.2_to_1", dict(G(512, 128, 160, tile=2), ldc=128), dict(f_geglu(G(512, 128, 160, tile=2)), ldc=128))

        # ---- admission
        pair("a.dma_ok.tile3", G(8192, 640, 640, tile=3), G(8192, 640, 672, tile=3))
        pair("a.dma_ok.tile3", G(8192, 640, 672, tile=1), G(8192, 640, 672, tile=8))
        pair("a.dma_ok.chunk32", C(1, 512, 512, 96, 128, tile=17), C(1, 512, 512, 96, 128, tile=16))
        pair("a.dma_ok.chunk32", C(1, 512, 512, 96, 128, tile=17), C(1, 512, 512, 80, 128, tile=17))
        pair("a.dma_ok.chunk32", C(8, 64, 64, 96, 320, tile=20), C(8, 64, 64, 96, 320, tile=8))
        pair("a.dma_ok.chunk32", C(1, 512, 512, 192, 128, tile=21), C(1, 512, 512, 192, 128, tile=16))
        for tl in (1, 3, 8, 21):
            pair("a.a3.tiles", dict(t, tile=16), dict(t, tile=tl))
        pair("a.a3.tiles", f_tail(C(8, 512, 512, 128, 128, tile=17)), f_tail(C(8, 512, 512, 128, 128, tile=21)))
        pair("a.a3.tiles", f_tail(C(8, 64, 64, 320, 320, tile=20)), f_tail(C(8, 64, 64, 320, 320, tile=8)))
        gs = dict(f_gnp(f_splitk(C(8, 8, 8, 1280, 1280), 10)), gn_slot_rows=64)
        for ch in (dict(gn_slot_rows=32), dict(gn_slot_rows=96), dict(gn_ld=1272), dict(gn_ld=-8)):
            pair("a.gn_partial.splitk", gs, dict(gs, **ch))
        pair("a.gn_partial.splitk", dict(f_gnp(f_splitk(G(2048, 1280, 5120), 3))), dict(f_gnp(f_splitk(G(2048 + 64, 1280, 5120), 3))))
        gp = f_gnp(G(1024, 128, 96))
        for ch in (dict(tile=2), dict(gn_slot_rows=64), dict(M=1088), dict(Z=2), dict(act=GEGLU, ldc=64)):
            pair("a.gn_partial.no_splitk", dict(gp, tile=1), dict(dict(gp, tile=1), **ch))
        pair("a.gn_partial.no_splitk", f_gnp(G(65536, 32, 64, tile=3)), f_gnp(G(65536, 32, 64, tile=14)))
        for tl in (4, 5, 7, 9, 15, 18, 19, 22, -1):
            pair("a.unknown_tile", dict(g, tile=3), dict(g, tile=tl))
        for tl in (6, 8, 14):                      # 2^21 rows of 1024 elements: past 32-bit byte offsets
            pair("a.fast.%d" % tl, G(2 ** 21, 320, 512, tile=tl), G(2 ** 21, 320, 512, tile=tl, ld1=1024))
        pair("a.fast.6", G(2 ** 21, 320, 512, tile=3, ld1=1024), G(2 ** 21, 320, 512, tile=6, ld1=1024))
        pair("a.fast.8", C(8, 32, 32, 128, 320, ups=1, tile=8), C(8, 64, 64, 128, 320, ups=1, stride=2, tile=8))
        pair("a.splitk.6", G(2048, 1280, 5120, tile=6), f_splitk(G(2048, 1280, 5120, tile=6), 3))
        for tl in (6, 8, 14):
            pair("a.geglu.%d" % tl, dict(G(8192, 640, 640, tile=tl), ldc=640), dict(f_geglu(G(8192, 640, 640, tile=tl)), ldc=640))
        t21 = C(1, 512, 512, 128, 256, tile=21)
        pair("a.tile21.out_f32", t21, f_f32(t21))
        pair("a.tile21.out_f32", dict(t21, tile=17), f_out16(t21))
        pair("a.tile21.residual", t21, f_res(t21))
        pair("a.tile21.rowvec", t21, f_rowvec(t21))
        pair("a.tile21.N512", C(1, 512, 512, 128, 512, tile=21), C(1, 512, 512, 128, 640, tile=21))
        pair("a.tile21.chunks", t21, C(1, 512, 512, 96, 256, tile=21))
        pair("a.tile21.chunks", C(1, 512, 512, 96, 256, tile=17), C(1, 512, 512, 96, 256, tile=21))
    return cases, pairs


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------
def case_bytes(cases):
    return [bytes(to_params(d)) for d in cases]


def case_hash(blobs):
    h = hashlib.sha256()
    for b in blobs:
        h.update(b)
    return h.hexdigest()


def library_answers(cases):
    from edtr_amd import lib as L
    plan = L.load().edtr_igemm_plan
    return [int(plan(ctypes.byref(to_params(d)))) for d in cases]


def child_answers(env_over, blobs, lib_path=None):
    """The library's answers for the cases `blobs` (case_bytes) from a fresh process with `env_over` set (the planner reads its
    switches once per process)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("EDTR_IGEMM_")}
    env.update(env_over)
    if lib_path:
        env["EDTR_AMD_LIB"] = lib_path
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], input="".join(b.hex() + "\n" for b in blobs), env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def halo_geometry(d):
    """Which of tile 16's five kernels a case runs (the order of the launch switch in igemm.hip)."""
    if not d.get("upsample2x") and d["OH"] == 8 and d["OW"] == 8 and d["IH"] == 8 and d["IW"] == 8 and d["M"] % 256 == 0:
        return 2
    if d.get("upsample2x") == 2:
        return 3
    if d.get("a3") and d.get("C3"):
        return 4
    return 1 if d.get("upsample2x") else 0


# what each switch setting is recorded for (make_plan_table.py) and checked for: name -> environment
SWITCH_SETTINGS = {
    "NO_AUTO=64": {"EDTR_IGEMM_NO_AUTO": "64"}, "NO_AUTO=256": {"EDTR_IGEMM_NO_AUTO": "256"}, "HALO=0": {"EDTR_IGEMM_HALO": "0"},
    "HALO_RAGGED=0": {"EDTR_IGEMM_HALO_RAGGED": "0"}, "SKINNY=0": {"EDTR_IGEMM_SKINNY": "0"}, "HALO512=0": {"EDTR_IGEMM_HALO512": "0"},
    "HALO512=2": {"EDTR_IGEMM_HALO512": "2"}, "HALO512P=1": {"EDTR_IGEMM_HALO512P": "1"}, "HALO160=0": {"EDTR_IGEMM_HALO160": "0"},
    "N160_TWO_PASS=1": {"EDTR_IGEMM_N160_TWO_PASS": "1"},     # (not only a debug bit: tile 8's two-pass epilogue writes no row statistics)
}


if __name__ == "__main__":
    from edtr_amd import lib as _L
    _plan = _L.load().edtr_igemm_plan
    print(json.dumps([int(_plan(ctypes.byref(_L.IgemmParams.from_buffer_copy(bytes.fromhex(ln.strip()))))) for ln in sys.stdin if ln.strip()]))
    sys.exit(0)


import pytest  # noqa: E402
from igemm_cells import to_params  # noqa: E402  (a case is a dict of fields, pointers included; the child above needs neither)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as fh:
        t = json.load(fh)
    cases, pairs = generate()
    blobs = case_bytes(cases)
    assert t["cases"] == len(cases) == len(t["answers"]) and t["case_hash"] == case_hash(blobs), \
        "the generator no longer builds the cases the table was recorded for (tools/make_plan_table.py records from the OLD build only)"
    assert os.path.getsize(TABLE) < 200 * 1024
    return t, cases, pairs, blobs


def test_every_case_answers_as_recorded(table):
    t, cases, _, _ = table
    got = library_answers(cases)
    bad = [(i, cases[i], t["answers"][i], got[i]) for i in range(len(cases)) if got[i] != t["answers"][i]]
    assert not bad, "%d of %d cases changed their answer; the first (index, case, recorded, now): %r" % (len(bad), len(cases), bad[:3])


def test_the_table_pins_every_tile_error_and_rule(table):
    """Conditions on the RECORDED answers: they hold for the old code alone, whatever the library under test does."""
    t, cases, pairs, _ = table
    ans = t["answers"]
    auto, explicit = {}, set()
    for d, a in zip(cases, ans):
        if a > 0 and not d.get("tile"):
            key = (16, halo_geometry(d)) if a == 16 else a
            auto[key] = auto.get(key, 0) + 1
        elif a > 0 and a == d["tile"]:
            explicit.add(a)
    for key in [1, 2, 3, 6, 8, 14, 17, 20] + [(16, g) for g in range(5)]:
        assert auto.get(key, 0) >= 20, (key, auto)
    assert 21 not in auto, "tile 21 is never automatic without EDTR_IGEMM_HALO512P"
    assert explicit == set(LIVE_TILES)
    assert {E_NULL, E_DTYPE, E_SHAPE, E_ALIGN, E_UNSUPPORTED} <= set(ans)
    assert sorted(pairs) == sorted(RULES)
    unpinned = [r for r in RULES if not any(ans[a] != ans[b] for a, b in pairs[r])]
    assert not unpinned, unpinned
    # a pair is a pair: each differs in a handful of fields, never in the tile unless the rule is about the tile
    for r, pp in pairs.items():
        for a, b in pp:
            diff = {k for k in set(cases[a]) | set(cases[b]) if cases[a].get(k, 0) != cases[b].get(k, 0)}
            assert 1 <= len(diff) <= 8, (r, diff)


@pytest.mark.parametrize("name", sorted(SWITCH_SETTINGS))
def test_switches_are_read_once_and_move_the_recorded_cases(table, name):
    """One fresh process per setting: a dozen or more cases whose recorded answer moves under the switch, and some that stay."""
    t, cases, _, blobs = table
    rec = t["switches"][name]
    moved = [i for i, a in zip(rec["cases"], rec["answers"]) if t["answers"][i] != a]
    assert len(moved) >= 12, (name, len(moved))
    assert child_answers(SWITCH_SETTINGS[name], [blobs[i] for i in rec["cases"]]) == rec["answers"]


# ---- the header stands alone -----------------------------------------------------------------------------------------------------
def _host_compiler():
    for cand in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("igemm_plan") / "igemm_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "edtr_amd", "csrc"), os.path.join(ROOT, "tests", "host", "igemm_plan_main.cpp"), "-o", exe], check=True)
    return exe


def _run_program(exe, blobs, env_over=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EDTR_IGEMM_")}
    env.update(env_over or {})
    r = subprocess.run([exe], input="".join(b.hex() + "\n" for b in blobs), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(blobs) and all(len(row) == 4 for row in rows)
    return rows        # rc fast stagger debug_flags


def test_header_alone_under_sanitizers_answers_the_table(table, plan_program):
    """igemm_plan.h compiled by a host compiler with no HIP in sight, under AddressSanitizer and UBSan: the whole case list, clean."""
    t, cases, _, blobs = table
    rows = _run_program(plan_program, blobs)
    assert [row[0] for row in rows] == t["answers"]
    assert all(row[2] == 0 and row[3] == 0 for row in rows), "no switch set: no stagger, no debug flag"


def test_debug_flags_and_stagger_reach_the_plan(table, plan_program):
    t, cases, _, blobs = table
    for env, bit in (("EDTR_IGEMM_GENERAL_EPILOGUE", 1), ("EDTR_IGEMM_N160_TWO_PASS", 2), ("EDTR_IGEMM_GEGLU_SERIAL", 4)):
        rows = _run_program(plan_program, blobs[:400], {env: "1"})
        assert all(row[3] == bit for row in rows if row[0] > 0) and any(row[0] > 0 for row in rows)
        rows = _run_program(plan_program, blobs[:50], {env: "0"})
        assert all(row[3] == 0 for row in rows)
    rows = _run_program(plan_program, blobs, {"EDTR_IGEMM_STAGGER": "50"})
    assert [row[0] for row in rows] == t["answers"], "the stagger moves no tile"
    n = 0
    for d, row in zip(cases, rows):
        want = 0
        if row[0] in (3, 8) and d.get("splitk", 0) <= 1:
            bn = 160 if row[0] == 8 else 128
            wgs = ((d["M"] + 127) // 128) * ((d["N"] + bn - 1) // bn) * d["Z"]
            nkt = (d["K"] + 63) // 64
            if wgs >= 768 and nkt <= 48:
                want = (4000 + nkt * 1350 + (11000 if d.get("act") == GEGLU else 9000)) * 50 // 200
        assert row[2] == want, (d, row)
        n += want > 0
    assert n >= 20
