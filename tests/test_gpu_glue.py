"""Per-kernel tests of the fp32 "glue" kernels around the MFMA launches (run on the MI355X box: pytest -m gpu): the tiled-path
helpers (edtr_tile_accumulate, edtr_divide, edtr_gn_pool, edtr_copy3d_f32), the wavelet level, the sampler arithmetic and the
fp32 -> 16-bit cast.  Conventions of tests/test_gpu_ops.py: every call goes through edtr_amd.ops.make_* and ops.launch; every
output element is compared with an fp64 reference of the exact fp32 inputs (tests/glue_reference.py) through
edtr_amd.testing.elem_ratio, or bit for bit where the kernel only moves or rounds values.  The bounds follow from the arithmetic
(each fp32 operation contributes at most 2^-24 relative error; elem(..., float32, k) allows 2^-23 |ref| + k 2^-22 absref), they
are not measured.  Every destination sits inside a larger buffer — NaN around pure stores, a finite pattern around
read-modify-write — and everything outside the written region must stay bit-unchanged.  Each kernel with a grid-stride loop
has one case above 4096 x 256 elements (the loop's second trip).  tests/test_glue_bound.py shows on the CPU which defects these
bounds reject."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import glue_reference as R
from edtr_amd.testing import elem_ratio

pytestmark = pytest.mark.gpu

F32 = torch.float32
PAD = 64                # guard elements in front of and behind every destination
GRID_SPAN = R.GRID_SPAN


def _ops():
    from edtr_amd import ops
    return ops


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


ELEM = {}          # kernel -> worst element ratio |got - ref| / bound measured in this file (printed by the last test; EDTR_GLUE_ERRLOG=path dumps it)


def elem(kernel, got, ref, absref, k, extra=None, out_dtype=F32):
    """Assert the rounding-aware element bound (edtr_amd/testing.py): |got - ref| <= 2u|ref| + k 2^-22 absref + extra everywhere."""
    r, where = elem_ratio(got, ref, absref, out_dtype, k, extra)
    ELEM[kernel] = max(ELEM.get(kernel, 0.0), r)
    print(f"[{kernel}] worst element ratio {r:.3f}")
    assert r <= 1.0, f"{kernel}: element bound exceeded: ratio {r:.3g} at {where}"
    return r


def exact(kernel, got, want):
    """Bit-exact comparison (recorded as ratio 0 / inf so that the summary lists the kernel)."""
    ok = torch.equal(bits(got), bits(want))
    ELEM[kernel] = max(ELEM.get(kernel, 0.0), 0.0 if ok else float("inf"))
    if not ok:
        bad = (bits(got) != bits(want)).nonzero()
        raise AssertionError(f"{kernel}: {len(bad)} elements differ bitwise, first at {bad[0].tolist()}: "
                             f"{got.cpu()[tuple(bad[0])]} vs {want.cpu()[tuple(bad[0])]}")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def guard_buf(shape, d, fill=float("nan"), dtype=F32, seed=None):
    """A `shape` view PAD elements inside a flat buffer of numel + 2 PAD: NaN-filled (pure stores), or a finite random pattern when
    `seed` is given (read-modify-write).  Returns (buffer, view, host copy of the buffer before the launch)."""
    n = int(np.prod(shape))
    host = torch.full((n + 2 * PAD,), fill, dtype=dtype) if seed is None else (rnd((n + 2 * PAD,), seed) + 0.25).to(dtype)
    buf = host.to(d)
    return buf, buf[PAD:PAD + n].view(shape), host


def untouched(buf, before, written=None):
    """Everything of `buf` outside the written region equals `before` bit for bit.  `written`: bool mask over the view's
    elements (None: the whole view was written; only the guards are compared)."""
    a, b = bits(buf), bits(before)
    mask = torch.ones(a.shape, dtype=torch.bool)
    n = a.numel() - 2 * PAD
    mask[PAD:PAD + n] = False if written is None else ~written.reshape(-1)
    assert torch.equal(a[mask], b[mask]), f"{int((a[mask] != b[mask]).sum())} elements outside the written region changed"


# =====================================================================================================================================
# 1. tile accumulate + divide
# =====================================================================================================================================
def _gauss(tw, th, d):
    from edtr_amd import tiling
    return torch.tensor(tiling.gaussian_weights(tw, th), dtype=F32)


@pytest.mark.parametrize("H,W", [(20, 28), (21, 30)])          # (21, 30): the last windows of both axes are snapped to the edge
def test_tile_accumulate_overlap_add_then_divide(H, W):
    """Overlap-add onto NON-ZERO out / count over 10 planes: up to 4 windows (9 with the snapped ones) cover a pixel; then
    edtr_divide of the result.  k = covering windows + 1 (one product and one addition per window)."""
    from edtr_amd import tiling
    ops, d = _ops(), dev()
    B, C, size = 2, 5, 8
    windows = [(hi, wi, size, size) for hi, _, wi, _ in tiling.sliding_windows(H, W, size, 4)]
    obuf, out, o_before = guard_buf((B, C, H, W), d, seed=100)
    cbuf, cnt, c_before = guard_buf((B, C, H, W), d, seed=101)
    cnt.abs_().add_(0.5)                                       # a count is positive
    c_before = cbuf.cpu().clone()
    out0, cnt0 = out.cpu().clone(), cnt.cpu().clone()
    w = _gauss(size, size, d)
    tiles = [rnd((B, C, size, size), 110 + i) for i in range(len(windows))]
    wd = w.to(d)
    for t, (hi, wi, th, tw) in zip(tiles, windows):
        ops.launch(ops.make_tile_accumulate(tile=t.to(d), wts=wd, out=out, count=cnt, B=B, C=C, H=H, W=W, th=th, tw=tw, hi=hi, wi=wi))
    torch.cuda.synchronize()
    ref, aref, cref, acref, cover = R.tile_accumulate_ref(out0, cnt0, tiles, [w] * len(windows), windows)
    assert cover.max() - 1 >= 4 and cover.min() - 1 >= 1
    elem("tile_accumulate", out, ref, cover * aref, 1)                     # k folded into absref: it differs per pixel
    elem("tile_accumulate", cnt, cref, cover * acref, 1)                   # EVERY plane of count
    untouched(obuf, o_before)
    untouched(cbuf, c_before)
    # divide: one correctly rounded (or 1-ulp) division of the fp32 values the kernel reads
    rbuf, res, r_before = guard_buf((B, C, H, W), d)
    ops.launch(ops.make_divide(num=out, den=cnt, out=res, n=out.numel()))
    torch.cuda.synchronize()
    elem("divide", res, R.f64(out) / R.f64(cnt), None, 0)
    untouched(rbuf, r_before)


def test_divide_wide_denominator():
    ops, d = _ops(), dev()
    n = 3001
    num = rnd((n,), 120).to(d)
    den = (10.0 ** (torch.rand(n, generator=torch.Generator().manual_seed(121)) * 9 - 6)).to(d)      # 1e-6 ... 1e3
    den[:2] = torch.tensor([1e-6, 1e3])
    rbuf, res, before = guard_buf((n,), d)
    ops.launch(ops.make_divide(num=num, den=den, out=res, n=n))
    torch.cuda.synchronize()
    elem("divide", res, R.f64(num) / R.f64(den), None, 0)
    untouched(rbuf, before)


def test_tile_accumulate_rectangular_tile_at_the_corner():
    """th = 6, tw = 10 with hi + th == H and wi + tw == W: the last element written is the last of each plane; the next plane's
    first pixels, every pixel outside the window and the guards stay bit-unchanged."""
    ops, d = _ops(), dev()
    B, C, H, W, th, tw = 2, 5, 20, 28, 6, 10
    hi, wi = H - th, W - tw
    obuf, out, o_before = guard_buf((B, C, H, W), d, seed=130)
    cbuf, cnt, c_before = guard_buf((B, C, H, W), d, seed=131)
    out0, cnt0 = out.cpu().clone(), cnt.cpu().clone()
    tile, w = rnd((B, C, th, tw), 132), rnd((th, tw), 133).abs() + 0.1
    ops.launch(ops.make_tile_accumulate(tile=tile.to(d), wts=w.to(d), out=out, count=cnt, B=B, C=C, H=H, W=W, th=th, tw=tw, hi=hi, wi=wi))
    torch.cuda.synchronize()
    ref, aref, cref, acref, _ = R.tile_accumulate_ref(out0, cnt0, [tile], [w], [(hi, wi, th, tw)])
    elem("tile_accumulate", out, ref, aref, 2)
    elem("tile_accumulate", cnt, cref, acref, 2)
    written = torch.zeros((B, C, H, W), dtype=torch.bool)
    written[..., hi:, wi:] = True
    untouched(obuf, o_before, written)
    untouched(cbuf, c_before, written)


@pytest.mark.parametrize("weight", ["gaussian", "uniform"])
def test_tiled_fn_of_the_identity_returns_its_input(weight):
    """The public path (tiling.make_tiled_fn: zero, accumulate every window, divide) around the identity: sum(x w) / sum(w) = x at
    every seam.  k = 5: <= 4 products and additions of same-signed terms in the numerator, as many additions in the denominator,
    one division — each 2^-24 relative, no cancellation."""
    from edtr_amd import tiling
    d = dev()
    x = rnd((2, 4, 16, 24), 140)
    got = tiling.make_tiled_fn(lambda t: t, 8, 4, weight=weight)(x.to(d))
    torch.cuda.synchronize()
    assert got.shape == x.shape and got.dtype == F32
    elem("tile_accumulate+divide", got, x, x.abs(), 5)


def test_tile_accumulate_grid_stride():
    """1 x 3 x 640 x 640 = 1 228 800 tile elements (> 4096 x 256) into 648 x 648 planes at (5, 3): the loop's second trip."""
    ops, d = _ops(), dev()
    C, H, W, th, tw, hi, wi = 3, 648, 648, 640, 640, 5, 3
    assert C * th * tw > GRID_SPAN
    obuf, out, o_before = guard_buf((1, C, H, W), d, seed=150)
    cbuf, cnt, c_before = guard_buf((1, C, H, W), d, seed=151)
    out0, cnt0 = out.cpu().clone(), cnt.cpu().clone()
    tile, w = rnd((1, C, th, tw), 152), rnd((th, tw), 153).abs() + 0.1
    ops.launch(ops.make_tile_accumulate(tile=tile.to(d), wts=w.to(d), out=out, count=cnt, B=1, C=C, H=H, W=W, th=th, tw=tw, hi=hi, wi=wi))
    torch.cuda.synchronize()
    ref, aref, cref, acref, _ = R.tile_accumulate_ref(out0, cnt0, [tile], [w], [(hi, wi, th, tw)])
    elem("tile_accumulate", out, ref, aref, 2)
    elem("tile_accumulate", cnt, cref, acref, 2)
    written = torch.zeros((1, C, H, W), dtype=torch.bool)
    written[..., hi:hi + th, wi:wi + tw] = True
    untouched(obuf, o_before, written)
    untouched(cbuf, c_before, written)


def test_tile_accumulate_error_codes():
    ops, d = _ops(), dev()
    out, cnt = torch.zeros((1, 2, 16, 24), device=d), torch.zeros((1, 2, 16, 24), device=d)
    tile, w = torch.zeros((1, 2, 8, 8), device=d), torch.ones((8, 8), device=d)
    kw = dict(tile=tile, wts=w, out=out, count=cnt, B=1, C=2, H=16, W=24, th=8, tw=8, hi=0, wi=0)
    for bad in (dict(hi=9), dict(wi=-1), dict(th=0)):
        with pytest.raises(RuntimeError, match="EDTR_E_SHAPE"):
            ops.launch(ops.make_tile_accumulate(**{**kw, **bad}))
    with pytest.raises(RuntimeError, match="EDTR_E_NULL"):
        ops.launch(ops.make_tile_accumulate(**{**kw, "count": None}))
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(cnt.abs().sum()) == 0.0


# =====================================================================================================================================
# 2. gn_pool
# =====================================================================================================================================
TILE_PIXELS = [48 * 40, 48 * 24, 16 * 40, 32 * 40, 48 * 8, 16 * 24]      # unequal tiles of a tiled VAE
CPG = 2                                                                   # channels per group


def _pool_inputs(T, BG, seed, pixels=None, same=False):
    """Per-tile data [BG, pixels x CPG] (each tile its own mean and spread unless `same`), their fp64 (sum, sumsq), and the
    weights / counts exactly as nets.emit_vae_net_tiled forms them (float32 tensors of pixels / sum(pixels), pixels x cpg)."""
    pix = [float(p) for p in (pixels or TILE_PIXELS[:T])]
    tiles = [(rnd((BG, int(p) * CPG), seed + t) * (1.0 if same else 1.0 + 0.3 * t) + (0.4 if same else 0.4 * t - 0.5)).numpy() for t, p in enumerate(pix)]
    sums, _ = R.tile_sums(tiles)
    weights = torch.tensor([v / sum(pix) for v in pix], dtype=F32)
    counts = torch.tensor([v * CPG for v in pix], dtype=F32)
    return sums, weights, counts


def _pool(sums, weights, counts, d):
    """Launch edtr_gn_pool on a guarded copy of `sums`; returns the pooled [T, BG, 2] as numpy after checking the guards."""
    ops = _ops()
    T, BG = sums.shape[:2]
    buf, view, before = guard_buf((T, BG, 2), d, fill=12345.678, dtype=torch.float64)
    view.copy_(torch.from_numpy(sums))
    before = buf.cpu().clone()
    ops.launch(ops.make_gn_pool(sums=view, weights=weights.to(d), counts=counts.to(d), T=T, BG=BG))
    torch.cuda.synchronize()
    untouched(buf, before)                 # the slots beyond [T][BG][2]
    return view.cpu().numpy()


def _pool_ratio(got, ref, bound):
    r = float((np.abs(got - ref) / bound).max()) if np.isfinite(got).all() else float("inf")
    ELEM["gn_pool"] = max(ELEM.get("gn_pool", 0.0), r)
    print(f"[gn_pool] worst ratio {r:.3f}")
    return r


@pytest.mark.parametrize("T", [1, 3, 6])
@pytest.mark.parametrize("BG", [32, 64, 300])           # 300: a second block with a ragged tail
def test_gn_pool_vs_float64_restatement(T, BG):
    d = dev()
    sums, weights, counts = _pool_inputs(T, BG, 200 + 10 * T)
    got = _pool(sums, weights, counts, d)
    ref, bound = R.gn_pool_ref(sums, weights, counts)
    assert _pool_ratio(got, ref, bound) <= 1.0
    # the statement itself, written the other way round: sum / count is the weighted mean of the tile means for EVERY tile,
    # and sumsq / count - mean^2 the weighted mean of the tile variances
    mean, var = R.gn_pool_stats(sums, weights, counts)
    c = counts.double().numpy()[:, None]
    gm = got[..., 0] / c
    gv = got[..., 1] / c - gm * gm
    assert np.abs(gm - mean).max() <= 1e-14 * (np.abs(mean).max() + 1.0)
    assert np.abs(gv - var).max() <= 1e-13 * (var + mean * mean).max()
    if T == 1:                                          # one tile: the pair is unchanged
        assert np.all(np.abs(got - sums) <= 1e-15 * np.abs(sums))


def test_gn_pool_equal_tiles_share_one_mean():
    """Tiles of one distribution and equal size: after pooling sum / count is the same for every tile and equals the weighted mean
    of the per-tile means."""
    d = dev()
    T, BG = 4, 64
    sums, weights, counts = _pool_inputs(T, BG, 260, pixels=[16 * 40] * T, same=True)
    got = _pool(sums, weights, counts, d)
    c = counts.double().numpy()[:, None]
    m_in, m_out = sums[..., 0] / c, got[..., 0] / c
    want = np.average(m_in, axis=0, weights=weights.double().numpy())
    assert np.abs(m_out - m_out[0]).max() <= 1e-15 * np.abs(m_out).max()
    assert np.abs(m_out[0] - want).max() <= 1e-15 * (np.abs(m_in).max())
    ref, bound = R.gn_pool_ref(sums, weights, counts)
    assert _pool_ratio(got, ref, bound) <= 1.0


def _constant_tile_with_negative_variance(c):
    """(sum, sumsq) of a constant-valued tile of `c` elements with sumsq one ulp below sum^2 / c, chosen so that s1/c - m^2 is
    negative in fp64 whether or not the compiler fuses the product into the subtraction (checked in exact arithmetic)."""
    for v in (0.7, 1.3, 0.37, 2.9, 0.11, 5.3, 0.77):
        s0 = np.float64(v) * c
        s1 = np.nextafter(s0 * s0 / c, 0.0)
        m = s0 / c
        plain = s1 / c - m * m
        fused = Fraction(float(s1 / c)) - Fraction(float(m)) ** 2
        moved = (plain + m * m) * c != (m * m) * c and (float(fused) + m * m) * c != (m * m) * c     # an unclamped kernel writes another value
        if plain < 0.0 and fused < 0 and moved:
            return s0, s1
    raise AssertionError("no constant with a negative cancelled variance found")


def test_gn_pool_clamps_a_cancelled_variance_to_zero():
    """A constant tile whose sumsq is one ulp short has variance -eps by cancellation: it must pool as variance 0, i.e. the pair
    written back is exactly (m c, (0 + m m) c) — bit for bit, since with T = 1 and weight 1 every step is one rounding."""
    d = dev()
    BG, c = 32, float(16 * 40 * CPG)
    s0, s1 = _constant_tile_with_negative_variance(c)
    sums = np.empty((1, BG, 2))
    sums[0, :, 0], sums[0, :, 1] = s0, s1
    assert not np.array_equal(R.gn_pool_ref(sums, [1.0], [c], defect="no_clamp")[0], R.gn_pool_ref(sums, [1.0], [c])[0])
    got = _pool(sums, torch.ones(1), torch.tensor([c]), d)
    m = s0 / c
    assert np.all(got[0, :, 0] == m * c)
    assert np.all(got[0, :, 1] == (0.0 + m * m) * c), (got[0, 0, 1], (m * m) * c)


@pytest.mark.parametrize("dtype", [torch.bfloat16])
def test_gn_pool_pair_makes_gn_apply_reproduce_the_pooled_statistics(dtype):
    """The contract in the kernel's comment: edtr_gn_apply, given a tile's pooled (sum, sumsq), normalises that tile with the POOLED
    mean and variance.  C = 64 (2 channels per group), tile 0 has HW = 256; B = 2.  Bound: 2u|ref| of the bf16 store plus
    k = 4 on absref = |gamma| rstd (|x| + |mean|) + |beta| — the fp32 steps of gn_apply_kernel: (float)var + eps and v_rsq (1 ulp),
    gamma rstd, (float)mean g, beta - ., x g + . : <= 8 roundings of 2^-24 <= 4 2^-22 (no reduction runs on the device here)."""
    ops, d = _ops(), dev()
    B, C, G, eps = 2, 64, 32, 1e-6
    hw = [256, 16 * 24, 8 * 16]
    T, BG = len(hw), B * G
    xs = [(rnd((B, n, C), 270 + t) * (1.0 + 0.5 * t) + 0.3 * t).to(dtype) for t, n in enumerate(hw)]        # NHWC, 16-bit
    # per (image, group) data of tile t: [B, n, G, CPG] -> [BG, n CPG]
    tiles = [x.double().reshape(B, n, G, CPG).permute(0, 2, 1, 3).reshape(BG, n * CPG).numpy() for x, n in zip(xs, hw)]
    sums, _ = R.tile_sums(tiles)
    weights = torch.tensor([float(n) / sum(hw) for n in hw], dtype=F32)
    counts = torch.tensor([float(n * CPG) for n in hw], dtype=F32)
    buf, view, before = guard_buf((T, BG, 2), d, fill=12345.678, dtype=torch.float64)
    view.copy_(torch.from_numpy(sums))
    before = buf.cpu().clone()
    ops.launch(ops.make_gn_pool(sums=view, weights=weights.to(d), counts=counts.to(d), T=T, BG=BG))
    gamma, beta = 1 + 0.1 * rnd((C,), 280), 0.1 * rnd((C,), 281)
    x0 = xs[0].to(d).contiguous()
    ybuf, y, y_before = guard_buf((B * hw[0], C), d, dtype=dtype)
    _, ap = ops.make_gn(dtype=dtype, x=x0, ldx=C, B=B, HW=hw[0], C=C, sums=view[0], gamma=gamma.to(d), beta=beta.to(d), eps=eps,
                        silu=False, y=y, ldy=C)
    ops.launch(ap)
    torch.cuda.synchronize()
    untouched(buf, before)
    untouched(ybuf, y_before)
    mean, var = R.gn_pool_stats(sums, weights, counts)                     # [BG]
    mean = torch.from_numpy(mean).reshape(B, 1, G, 1)
    rstd = 1.0 / torch.sqrt(torch.from_numpy(var).reshape(B, 1, G, 1) + R.f32(eps))
    xd = xs[0].double().reshape(B, hw[0], G, CPG)
    g, b = gamma.double().reshape(1, 1, G, CPG), beta.double().reshape(1, 1, G, CPG)
    ref = (xd - mean) * rstd * g + b
    absref = g.abs() * rstd * (xd.abs() + mean.abs()) + b.abs()
    elem("gn_pool+gn_apply", y.float().cpu().reshape(B, hw[0], G, CPG), ref, absref, 4, out_dtype=dtype)


# =====================================================================================================================================
# 3. copy3d_f32 (bit-exact)
# =====================================================================================================================================
def test_copy3d_extract_and_place():
    ops, d = _ops(), dev()
    # extract a 3-plane 7 x 9 block from the interior of (3, 20, 31) into a dense destination
    src = rnd((3, 20, 31), 300).to(d)
    buf, dst, before = guard_buf((3, 7, 9), d)
    ops.launch(ops.make_copy3d(src=src[:, 5:, 11:], src_plane=20 * 31, src_row=31, dst=dst, dst_plane=63, dst_row=9, planes=3, rows=7, cols=9))
    torch.cuda.synchronize()
    exact("copy3d", dst, src[:, 5:12, 11:20])
    untouched(buf, before)
    # place a dense (5, 6, 10) block into the interior of a NaN-filled (5, 16, 24): dst_row_stride != cols, dst_plane_stride != rows x row_stride
    blk = rnd((5, 6, 10), 301).to(d)
    buf, big, before = guard_buf((5, 16, 24), d)
    ops.launch(ops.make_copy3d(src=blk, src_plane=60, src_row=10, dst=big[:, 3:, 7:], dst_plane=16 * 24, dst_row=24, planes=5, rows=6, cols=10))
    torch.cuda.synchronize()
    exact("copy3d", big[:, 3:9, 7:17], blk)
    written = torch.zeros((5, 16, 24), dtype=torch.bool)
    written[:, 3:9, 7:17] = True
    untouched(buf, before, written)
    assert torch.isnan(big.cpu()[~written]).all()


@pytest.mark.parametrize("planes,rows,cols", [(4, 9, 1), (4, 1, 13), (1, 1, 1)])
def test_copy3d_single_column_and_single_row(planes, rows, cols):
    ops, d = _ops(), dev()
    src = rnd((planes, 12, 17), 310).to(d)
    buf, big, before = guard_buf((planes, 11, 15), d)
    ops.launch(ops.make_copy3d(src=src[:, 2:, 3:], src_plane=12 * 17, src_row=17, dst=big[:, 1:, 2:], dst_plane=11 * 15, dst_row=15,
                               planes=planes, rows=rows, cols=cols))
    torch.cuda.synchronize()
    exact("copy3d", big[:, 1:1 + rows, 2:2 + cols], src[:, 2:2 + rows, 3:3 + cols])
    written = torch.zeros((planes, 11, 15), dtype=torch.bool)
    written[:, 1:1 + rows, 2:2 + cols] = True
    untouched(buf, before, written)


def test_copy3d_source_plane_stride_zero_broadcasts_one_plane():
    """The C ABI places no condition on the strides, so a source plane stride of 0 is accepted and repeats one plane."""
    ops, d = _ops(), dev()
    src = rnd((6, 10), 320).to(d)
    buf, dst, before = guard_buf((5, 6, 10), d)
    ops.launch(ops.make_copy3d(src=src, src_plane=0, src_row=10, dst=dst, dst_plane=60, dst_row=10, planes=5, rows=6, cols=10))
    torch.cuda.synchronize()
    exact("copy3d", dst, src.expand(5, 6, 10))
    untouched(buf, before)


def test_copy3d_grid_stride():
    """2 planes of 800 x 700 = 1 120 000 elements (> 4096 x 256), placed inside (2, 804, 708)."""
    ops, d = _ops(), dev()
    assert 2 * 800 * 700 > GRID_SPAN
    src = rnd((2, 800, 700), 330).to(d)
    buf, big, before = guard_buf((2, 804, 708), d)
    ops.launch(ops.make_copy3d(src=src, src_plane=800 * 700, src_row=700, dst=big[:, 2:, 4:], dst_plane=804 * 708, dst_row=708,
                               planes=2, rows=800, cols=700))
    torch.cuda.synchronize()
    exact("copy3d", big[:, 2:802, 4:704], src)
    written = torch.zeros((2, 804, 708), dtype=torch.bool)
    written[:, 2:802, 4:704] = True
    untouched(buf, before, written)


# =====================================================================================================================================
# 4. cast16 (bit-exact against the CPU's round-to-nearest-even)
# =====================================================================================================================================
DTYPES = [torch.bfloat16, torch.float16]
PATTERN = 0x5A3C                # bit pattern of the pre-filled destination (a finite 16-bit value in both formats)


def _cast(dtype, src_view, rows, C, ld_dst, d, extra_rows=3):
    """edtr_cast16 of src_view [rows, C] into the [rows, C] corner of a pattern-filled [rows + extra_rows, ld_dst] buffer; checks
    that columns >= C, the rows after `rows` and the guards keep the pattern; returns the [rows, C] result on the host."""
    ops = _ops()
    n = (rows + extra_rows) * ld_dst
    host = torch.full((n + 2 * PAD,), PATTERN, dtype=torch.int16).view(dtype)
    buf = host.to(d)
    full = buf[PAD:PAD + n].view(rows + extra_rows, ld_dst)
    ops.launch(ops.make_cast16(dtype=dtype, src=src_view, rows=rows, C=C, dst=full[:rows, :C]))
    torch.cuda.synchronize()
    written = torch.zeros((rows + extra_rows, ld_dst), dtype=torch.bool)
    written[:rows, :C] = True
    untouched(buf, host, written)
    return full[:rows, :C].cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast16_strided_rows(dtype):
    """rows = 37, C = 72, ld_src = 76, ld_dst = 80: three different widths."""
    d = dev()
    rows, C, ld_src, ld_dst = 37, 72, 76, 80
    src = torch.full((rows, ld_src), float("nan"))
    src[:, :C] = rnd((rows, C), 400) * 3
    got = _cast(dtype, src.to(d)[:, :C], rows, C, ld_dst, d)
    exact(f"cast16[{dtype}]", got, src[:, :C].to(dtype))


def _special_values():
    f16, b16 = 2.0 ** -11, 2.0 ** -8                      # half a spacing above 1.0 in fp16 / bf16
    v = [0.0, -0.0, 1.0, -1.0,
         1 + f16, 1 + 3 * f16, -(1 + f16), -(1 + 3 * f16),        # fp16 ties: lower neighbour even (-> down) and odd (-> up)
         1 + b16, 1 + 3 * b16, -(1 + b16), -(1 + 3 * b16),        # bf16 ties likewise
         1 + b16 + 2.0 ** -20, 1 + b16 - 2.0 ** -20, 1 + f16 + 2.0 ** -23, 1 + f16 - 2.0 ** -23,      # just off the ties
         65504.0, 65519.99, 65520.0, 65536.0, -65504.0, -65519.99, -65520.0, 70000.0,     # fp16 overflow: 65520 -> inf under RNE
         2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 3 * 2.0 ** -25, 2.0 ** -26, -2.0 ** -25, -2.0 ** -24,   # fp16 subnormals
         1023.5 * 2.0 ** -24, 1e-7, 6.1e-5,
         float("inf"), float("-inf"), 3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38, 3.39e38, 1e-30, 1e30,
         float("nan")]
    return torch.tensor(v + [0.5] * (-len(v) % 8), dtype=F32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast16_special_values(dtype):
    d = dev()
    row = _special_values()
    C = row.numel()
    src = torch.stack([row, -row])
    got = _cast(dtype, src.to(d), 2, C, C + 8, d)
    want = src.to(dtype)
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(got.float()), nan), "NaN must stay NaN and nothing else may become one"
    exact(f"cast16[{dtype}]", torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))
    # the CPU reference itself rounds to nearest even (a few cases spelled out, so that the test does not rest on it alone)
    one = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 65520.0, 2.0 ** -25, 3 * 2.0 ** -25])
    assert one.to(torch.bfloat16).float().tolist()[:2] == [1.0, 1 + 2.0 ** -6]
    assert one.to(torch.float16).float().tolist()[2:] == [float("inf"), 0.0, 2.0 ** -23]


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast16_grid_stride(dtype):
    """rows = 4100, C = 2560: 1 312 000 eight-wide vectors (> 4096 x 256)."""
    d = dev()
    rows, C = 4100, 2560
    assert rows * C // 8 > GRID_SPAN
    src = rnd((rows, C), 410)
    got = _cast(dtype, src.to(d), rows, C, C, d, extra_rows=1)
    exact(f"cast16[{dtype}]", got, src.to(dtype))


def test_cast16_error_codes():
    ops, d = _ops(), dev()
    src = torch.zeros((4, 80), device=d)
    dst = torch.zeros((4, 80), dtype=torch.bfloat16, device=d)
    with pytest.raises(RuntimeError, match="EDTR_E_ALIGN"):                # C = 12
        ops.launch(ops.make_cast16(dtype=torch.bfloat16, src=src[:, :12], rows=4, C=12, dst=dst[:, :12]))
    src74 = torch.zeros((4, 74), device=d)
    with pytest.raises(RuntimeError, match="EDTR_E_ALIGN"):                # ld_src = 74
        ops.launch(ops.make_cast16(dtype=torch.bfloat16, src=src74[:, :72], rows=4, C=72, dst=dst[:, :72]))
    with pytest.raises(RuntimeError, match="EDTR_E_SHAPE"):                # ld_dst = 64 < C
        ops.launch(ops.make_cast16(dtype=torch.bfloat16, src=src[:, :72], rows=4, C=72, dst=torch.as_strided(dst, (4, 72), (64, 1))))
    with pytest.raises(RuntimeError, match="EDTR_E_DTYPE"):                # an fp32 destination code
        ops.launch(ops.make_cast16(dtype=ops.F32S, src=src[:, :72], rows=4, C=72, dst=dst[:, :72]))
    torch.cuda.synchronize()
    assert float(dst.float().abs().sum()) == 0.0


# =====================================================================================================================================
# 5. wavelet level
# =====================================================================================================================================
def _wavelet_case(planes, H, W, r, seed):
    """One launch with `high` pre-filled non-zero: low within k = 9 of sum w |in| (8 additions and the products of the 9 taps, in
    the kernel's order or any other); high = high0 + (in - low): the low's error plus two more roundings -> k = 11."""
    ops, d = _ops(), dev()
    x = rnd((planes, H, W), seed) + 0.3
    lbuf, low, l_before = guard_buf((planes, H, W), d)
    hbuf, high, h_before = guard_buf((planes, H, W), d, seed=seed + 1)
    high0 = high.cpu().clone()
    ops.launch(ops.make_wavelet_level(src=x.to(d), low=low, high=high, planes=planes, H=H, W=W, radius=r))
    torch.cuda.synchronize()
    lref, alow = R.wavelet_level_ref(x.numpy(), r)
    lref, alow = torch.from_numpy(lref), torch.from_numpy(alow)
    elem("wavelet_level", low, lref, alow, 9)
    elem("wavelet_level", high, high0.double() + (x.double() - lref), high0.double().abs() + x.double().abs() + alow, 11)
    untouched(lbuf, l_before)
    untouched(hbuf, h_before)


@pytest.mark.parametrize("planes,H,W,r", [(7, 12, 17, 1), (7, 12, 17, 16), (7, 12, 17, 64),      # radius above both extents: every neighbour clamps
                                         (1, 1, 33, 2), (1, 33, 1, 2), (2, 5, 5, 4)])
def test_wavelet_level(planes, H, W, r):
    _wavelet_case(planes, H, W, r, 500 + r)


def test_wavelet_level_grid_stride():
    assert 3 * 600 * 600 > GRID_SPAN
    _wavelet_case(3, 600, 600, 8, 520)


def test_wavelet_level_without_high_writes_low_only():
    ops, d = _ops(), dev()
    planes, H, W, r = 7, 12, 17, 2
    x = rnd((planes, H, W), 530)
    lbuf, low, l_before = guard_buf((planes, H, W), d)
    sbuf, _, s_before = guard_buf((planes, H, W), d, seed=531)             # a sentinel where `high` would be
    ops.launch(ops.make_wavelet_level(src=x.to(d), low=low, high=None, planes=planes, H=H, W=W, radius=r))
    torch.cuda.synchronize()
    lref, alow = R.wavelet_level_ref(x.numpy(), r)
    elem("wavelet_level", low, torch.from_numpy(lref), torch.from_numpy(alow), 9)
    untouched(lbuf, l_before)
    assert torch.equal(bits(sbuf), bits(s_before))


def test_wavelet_decomposition_chain_and_reconstruction():
    """wavelet.wavelet_decomposition (5 launches, radii 1 .. 16 on 24 x 20 planes: the last radius clamps everywhere) against the
    numpy reference chained in fp64.  A level's error (9 2^-22 A_i) is blurred by the later levels into <= 9 2^-22 A_5, so the
    low needs k = 45 on A_5 = blur^5 |x|.  The device's high telescopes to x - low_5 in ITS OWN lows plus, per level, the rounding
    of (c - v) and of the accumulation: <= 6 2^-24 (|x| + sum A_i) — k = 46 on that absref for high, and k = 2 for the
    reconstruction identity low + high == x, where the low's own error cancels.  The colour fix relies on that identity."""
    from edtr_amd import wavelet
    d = dev()
    x = rnd((1, 3, 24, 20), 540) + 0.2
    high, low = wavelet.wavelet_decomposition(x.to(d))
    torch.cuda.synchronize()
    href, lref, a5, asum = (torch.from_numpy(v) for v in R.wavelet_chain_ref(x[0].numpy()))
    a_high = x[0].double().abs() + asum
    elem("wavelet_chain", low[0], lref, a5, 45)
    elem("wavelet_chain", high[0], href, a_high, 46)
    elem("wavelet_chain", R.f64(low[0]) + R.f64(high[0]), x[0].double(), a_high, 2)


def test_wavelet_level_error_codes():
    ops, d = _ops(), dev()
    x = torch.zeros((2, 8, 8), device=d)
    low = torch.zeros_like(x)
    with pytest.raises(RuntimeError, match="EDTR_E_UNSUPPORTED"):
        ops.launch(ops.make_wavelet_level(src=x, low=x, high=None, planes=2, H=8, W=8, radius=1))
    with pytest.raises(RuntimeError, match="EDTR_E_SHAPE"):
        ops.launch(ops.make_wavelet_level(src=x, low=low, high=None, planes=2, H=8, W=8, radius=0))


# =====================================================================================================================================
# 6. sampler arithmetic
# =====================================================================================================================================
def _q_sample_case(B, shape, t, seeds):
    from edtr_amd.diffusion import Diffusion
    ops, d = _ops(), dev()
    diff = Diffusion()
    ta, tb = diff.sqrt_alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod
    assert ta.numel() == 1000
    x, noise = rnd((B,) + shape, seeds[0]), rnd((B,) + shape, seeds[1])
    buf, out, before = guard_buf((B,) + shape, d)
    ops.launch(ops.make_q_sample(x=x.to(d), noise=noise.to(d), t=torch.tensor(t, dtype=torch.int64, device=d), tab_a=ta.to(d), tab_b=tb.to(d), out=out))
    torch.cuda.synchronize()
    ref, absref, fp32 = R.q_sample_ref(x.numpy(), noise.numpy(), t, ta.numpy(), tb.numpy())
    elem("q_sample", out, ref, absref, 2)
    exact("q_sample", out, fp32)           # noise_elem.h: two rounded products, one rounded sum — no contraction
    untouched(buf, before)


def test_q_sample_clamps_t_and_respects_image_boundaries():
    """per_image = 4 x 6 x 7 = 168 is no multiple of 64: image boundaries fall inside a wavefront.  t = -3 and 5000 read rows 0 and
    999 of the real 1000-step tables."""
    _q_sample_case(5, (4, 6, 7), [0, 999, 200, -3, 5000], (600, 601))


def test_q_sample_grid_stride():
    _q_sample_case(1, (GRID_SPAN + 777,), [437], (602, 603))


COEFS = (1.0990925, 0.45607486, 0.40786713, 0.59105539, math.sqrt(0.045623116))


def _check_update(kernel, p0, xp, x, eps, noise, coefs):
    """p0 = fma(c_recip, x, -(c_recipm1 e)): two roundings -> k = 3 on |c_recip x| + |c_recipm1 e| covers them with room; x_prev adds
    the product coef2 x and two fmas onto the ROUNDED p0 -> k = 6 on the absref built from p0's."""
    rp0, ap0, rxp, axp = R.sampler_update_ref(x, eps, noise, coefs)
    if p0 is not None:
        elem(kernel, p0, rp0, ap0, 3)
    elem(kernel, xp, rxp, axp, 6)


def test_sampler_update_scalar_coefficients():
    ops, d = _ops(), dev()
    n = 2 * 4 * 16 * 16 + 3
    c32 = tuple(R.f32(c) for c in COEFS)
    x, eps, noise = rnd((n,), 610), rnd((n,), 611), rnd((n,), 612)
    eps[:96] = x[:96] * float(np.float32(c32[0] / c32[1]))        # p0 cancels on a block: |p0| ~ 2^-24 absref, the bound must come from absref
    xbuf, xp, x_before = guard_buf((n,), d)
    pbuf, p0, p_before = guard_buf((n,), d)
    ops.launch(ops.make_sampler_update(x=x.to(d), eps=eps.to(d), noise=noise.to(d), coefs=COEFS, x_prev=xp, pred_x0=p0, n=n))
    torch.cuda.synchronize()
    rp0, ap0, _, _ = R.sampler_update_ref(x, eps, noise, c32)
    assert float((rp0[:96].abs() / ap0[:96]).max()) < 1e-6     # the block does cancel
    _check_update("sampler_update", p0, xp, x, eps, noise, c32)
    untouched(xbuf, x_before)
    untouched(pbuf, p_before)
    # pred_x0 = None: nothing but x_prev is written
    xbuf2, xp2, x_before2 = guard_buf((n,), d)
    sbuf, _, s_before = guard_buf((n,), d, seed=613)
    ops.launch(ops.make_sampler_update(x=x.to(d), eps=eps.to(d), noise=noise.to(d), coefs=COEFS, x_prev=xp2, pred_x0=None, n=n))
    torch.cuda.synchronize()
    _check_update("sampler_update", None, xp2, x, eps, noise, c32)
    exact("sampler_update", xp2, xp)
    untouched(xbuf2, x_before2)
    assert torch.equal(bits(sbuf), bits(s_before))


def test_sampler_update_grid_stride():
    ops, d = _ops(), dev()
    n = GRID_SPAN + 777
    c32 = tuple(R.f32(c) for c in COEFS)
    x, eps, noise = rnd((n,), 620), rnd((n,), 621), rnd((n,), 622)
    xbuf, xp, x_before = guard_buf((n,), d)
    pbuf, p0, p_before = guard_buf((n,), d)
    ops.launch(ops.make_sampler_update(x=x.to(d), eps=eps.to(d), noise=noise.to(d), coefs=COEFS, x_prev=xp, pred_x0=p0, n=n))
    torch.cuda.synchronize()
    _check_update("sampler_update", p0, xp, x, eps, noise, c32)
    untouched(xbuf, x_before)
    untouched(pbuf, p_before)


def test_sampler_update_indexed_vs_fp64_and_index_clamp():
    """Against the fp64 reference (not the scalar kernel, which shares sampler_update_elem); index = -1 and 9 read rows 0 and 3."""
    ops, d = _ops(), dev()
    B, shape, n_steps = 4, (4, 6, 7), 4
    table = torch.tensor([[1.0050, 0.1002, 0.0, 1.0, 0.0],
                          [1.0990925, 0.45607486, 0.40786713, 0.59105539, 0.2135957],
                          [1.9, 1.6155494, 0.21, 0.78, 0.31],
                          [14.7, 14.6659, 0.02, 0.98, 0.09]], dtype=F32)
    index = [3, 0, -1, 9]
    rows = [3, 0, 0, 3]
    x, eps, noise = rnd((B,) + shape, 630), rnd((B,) + shape, 631), rnd((B,) + shape, 632)
    xbuf, xp, x_before = guard_buf((B,) + shape, d)
    pbuf, p0, p_before = guard_buf((B,) + shape, d)
    ops.launch(ops.make_sampler_update_indexed(x=x.to(d), eps=eps.to(d), noise=noise.to(d), index=torch.tensor(index, dtype=torch.int64, device=d),
                                               coefs=table.to(d), x_prev=xp, pred_x0=p0))
    torch.cuda.synchronize()
    coefs = tuple(table[rows, j].double().reshape(B, 1, 1, 1) for j in range(5))
    _check_update("sampler_update_indexed", p0, xp, x, eps, noise, coefs)
    untouched(xbuf, x_before)
    untouched(pbuf, p_before)
    # pred_x0 = None
    xbuf2, xp2, x_before2 = guard_buf((B,) + shape, d)
    ops.launch(ops.make_sampler_update_indexed(x=x.to(d), eps=eps.to(d), noise=noise.to(d), index=torch.tensor(index, dtype=torch.int64, device=d),
                                               coefs=table.to(d), x_prev=xp2, pred_x0=None))
    torch.cuda.synchronize()
    exact("sampler_update_indexed", xp2, xp)
    untouched(xbuf2, x_before2)


def test_gaussian_sample_strided_moments_and_logvar_clamp():
    """ld = 12 > 2 C = 8 (the four trailing columns hold NaN: they must not be read); log-variances at and beyond -30 and 20."""
    ops, d = _ops(), dev()
    B, C, HW, ld, scale = 2, 4, 35, 12, 0.18215
    m = torch.full((B * HW, ld), float("nan"))
    m[:, :C] = rnd((B * HW, C), 640)
    m[:, C:2 * C] = rnd((B * HW, C), 641) * 3
    m[:12, C] = torch.tensor([-30.0, -30.5, -31.0, -45.0, -1e4, -29.999, 20.0, 20.5, 21.0, 40.0, 1e4, 19.999])
    noise = rnd((B, C, HW), 642)
    buf, out, before = guard_buf((B, C, HW), d)
    ops.launch(ops.make_gaussian_sample(moments=m.to(d), ld=ld, noise=noise.to(d), out=out, B=B, C=C, HW=HW, scale=scale))
    torch.cuda.synchronize()
    ref, absref, escale = R.gaussian_sample_ref(m, noise, B, C, HW, scale)
    # k = 3: the fma and the product by scale (0.5 lv is exact); the device expf is documented to 1 ulp (HIP math API) — 2 ulp of the
    # exponential, times |n| |scale|, is that documented accuracy with a factor of two in hand, not a measurement
    elem("gaussian_sample", out, ref, absref, 3, extra={"device expf, 2 ulp": 2 * 2.0 ** -23 * escale})
    untouched(buf, before)
    # noise = None: mean x scale, one rounding
    buf2, out2, before2 = guard_buf((B, C, HW), d)
    ops.launch(ops.make_gaussian_sample(moments=m.to(d), ld=ld, noise=None, out=out2, B=B, C=C, HW=HW, scale=scale))
    torch.cuda.synchronize()
    want = (m[:, :C].reshape(B, HW, C).permute(0, 2, 1).numpy() * np.float32(scale)).astype(np.float32)
    exact("gaussian_sample", out2, torch.from_numpy(np.ascontiguousarray(want)))
    untouched(buf2, before2)


def test_gaussian_sample_grid_stride():
    ops, d = _ops(), dev()
    B, C, HW, scale = 1, 4, 512 * 513, 0.18215
    assert B * C * HW > GRID_SPAN
    m = torch.cat([rnd((B * HW, C), 650), rnd((B * HW, C), 651) * 2], dim=1).contiguous()
    noise = rnd((B, C, HW), 652)
    buf, out, before = guard_buf((B, C, HW), d)
    ops.launch(ops.make_gaussian_sample(moments=m.to(d), ld=2 * C, noise=noise.to(d), out=out, B=B, C=C, HW=HW, scale=scale))
    torch.cuda.synchronize()
    ref, absref, escale = R.gaussian_sample_ref(m, noise, B, C, HW, scale)
    elem("gaussian_sample", out, ref, absref, 3, extra={"device expf, 2 ulp": 2 * 2.0 ** -23 * escale})
    untouched(buf, before)


@pytest.mark.parametrize("n", [2 * 4 * 16 * 16 + 3, GRID_SPAN + 777])
def test_axpby(n):
    """a x + b y: two products and a sum (or a product and an fma) -> k = 2.  The sampler (predict_noise), q_sample's host-t path and
    the wavelet reconstruction all write a fresh tensor, never in place, so no aliased case is tested."""
    ops, d = _ops(), dev()
    a, b = 7.5, 1.0 - 7.5                                       # classifier-free guidance: uncond + s (cond - uncond), large cancellation
    x, y = rnd((n,), 660), rnd((n,), 661)
    y[:64] = x[:64] * (7.5 / 6.5)                              # a x + b y cancels on a block
    buf, out, before = guard_buf((n,), d)
    ops.launch(ops.make_axpby(x=x.to(d), y=y.to(d), a=a, b=b, out=out, n=n))
    torch.cuda.synchronize()
    xd, yd = x.double(), y.double()
    elem("axpby", out, R.f32(a) * xd + R.f32(b) * yd, (R.f32(a) * xd).abs() + (R.f32(b) * yd).abs(), 2)
    untouched(buf, before)


def test_zz_glue_worst_ratios():
    """Bookkeeping (runs last in this file): the worst element ratio each kernel measured (0 = bit-exact comparisons only)."""
    import json
    print("\n[glue kernels: worst element ratio] " + "; ".join(f"{k}: {v:.3f}" for k, v in sorted(ELEM.items())))
    path = os.environ.get("EDTR_GLUE_ERRLOG")
    if path:
        with open(path, "w") as f:
            json.dump(ELEM, f, indent=1)
