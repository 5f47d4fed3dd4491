"""The K tail of the halo tiles (edtr_hip.h: a3 / C3 / ld3): conv3x3(xn) + conv1x1(x) + bias in ONE edtr_igemm launch, the 1x1
product joining the fp32 accumulator at the centre tap.  Every case is checked element by element (edtr_amd/testing.py: 2u|ref| +
k 2^-22 absref, ratio <= 1) against an fp64 reference on the 16-bit-rounded inputs, and so is today's two-launch form (1x1 GEMM,
16-bit store, residual of the 3x3) on the same inputs, with the one extra rounding of its skip tensor as a named term."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from edtr_amd.testing import elem_ratio, rounded_operand, unit_roundoff, LIPSCHITZ

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
UNSUPPORTED, SHAPE = -5, -2


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def elem(got, ref, absref, out_dtype, k, extra=None):
    r, where = elem_ratio(got, ref, absref, out_dtype, k, extra)
    print(f"element ratio {r:.3f}")
    assert r <= 1.0, f"element bound exceeded: ratio {r:.3g} at {where}"
    return r


def nchw(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class Case:
    """Operands of one conv3x3(xn) + conv1x1(x) problem on the device, and its fp64 reference."""

    def __init__(self, dtype, B, H, W, C1, C3, N, ld3=None, a_gn=False):
        from edtr_amd import ops
        self.ops, self.dtype, self.d = ops, dtype, dev()
        self.B, self.H, self.W, self.C1, self.C3, self.N = B, H, W, C1, C3, N
        self.M, self.K = B * H * W, 9 * C1 + C3
        d, M = self.d, self.M
        ld3 = ld3 or C3
        off = 64 if ld3 >= C3 + 64 else 0                   # ld3 > C3: a column slice of a wider tensor (the decoder's concat stream)
        xn = (rnd((M, C1), 11, 1.2) + (0.3 if a_gn else 0.0)).to(dtype)
        xbuf = rnd((M, ld3), 12).to(dtype)
        w9 = rnd((N, 9 * C1), 13, 1 / math.sqrt(9 * C1)).to(dtype)
        w1 = rnd((N, C3), 14, 1 / math.sqrt(C3)).to(dtype)
        b9, b1 = rnd((N,), 15), rnd((N,), 16)
        self.xn, self.xbuf = xn.to(d), xbuf.to(d)
        self.x = self.xbuf[:, off:off + C3]
        self.w9, self.w1, self.wcat = w9.to(d), w1.to(d), torch.cat([w9, w1], dim=1).contiguous().to(d)
        self.b9, self.b1, self.bsum = b9.to(d), b1.to(d), (b9 + b1).to(d)
        self.table = None
        x9, flip = nchw(xn.double(), B, H, W), None
        if a_gn:        # (scale, shift) per image and channel, SiLU: applied to the 9-tap operand only
            tb = torch.stack([1 + 0.2 * rnd((B, C1), 17), 0.2 * rnd((B, C1), 18)], dim=-1).contiguous()
            self.table = tb.to(d)
            xg, fl = rounded_operand(F.silu(xn.double().reshape(B, H * W, C1) * tb[:, None, :, 0].double() + tb[:, None, :, 1].double()),
                                     LIPSCHITZ["silu"] * 2.0 ** -23 * ((xn.double().reshape(B, H * W, C1) * tb[:, None, :, 0].double()).abs()
                                                                       + tb[:, None, :, 1].double().abs())
                                     + 2.0 ** -22 * F.silu(xn.double().reshape(B, H * W, C1) * tb[:, None, :, 0].double() + tb[:, None, :, 1].double()).abs(),
                                     dtype)
            x9, flip = nchw(xg.reshape(M, C1), B, H, W), nchw(fl.reshape(M, C1), B, H, W)
        wc = w9.double().reshape(N, 3, 3, C1).permute(0, 3, 1, 2)
        x3 = xbuf[:, off:off + C3].double()
        self.skip64 = x3 @ w1.double().t() + b1.double()
        self.skipabs = x3.abs() @ w1.double().abs().t() + b1.double().abs()
        self.ref = rows(F.conv2d(x9, wc, b9.double(), padding=1)) + self.skip64
        self.absref = rows(F.conv2d(x9.abs(), wc.abs(), b9.double().abs(), padding=1)) + self.skipabs
        self.extra = {} if flip is None else {"16-bit normalised operand, boundary values": rows(F.conv2d(flip, wc.abs(), None, padding=1))}

    def spatial(self):
        return (self.H, self.W, self.H, self.W, 1, 1, 1, 0)

    def fused(self, tile, splitk=1, gn=False, **kw):
        ops, d, M, N = self.ops, self.d, self.M, self.N
        out = torch.full((M, N), float("nan"), dtype=self.dtype, device=d)
        ws = torch.empty(splitk * M * N, dtype=torch.float32, device=d) if splitk > 1 else None
        slot = (ops.gn_slot_rows(self.H * self.W) if splitk > 1 else 128) if gn else 0
        gnp = torch.full((M // slot, N, 2), float("nan"), dtype=torch.float32, device=d) if gn else None
        args = dict(dtype=self.dtype, a1=self.xn, w=self.wcat, out=out, taps=9, M=M, N=N, C1=self.C1, ld1=self.C1, ldw=self.K, ldc=N,
                    spatial=self.spatial(), bias_n=self.bsum, rows_per_image=self.H * self.W, tile=tile, splitk=splitk, workspace=ws,
                    gn_partial=gnp, gn_slot_rows=slot if splitk > 1 else 0, a_gn=self.table, a_gn_silu=True, a3=self.x, C3=self.C3)
        args.update(kw)
        ops.launch(ops.make_igemm(**args))
        return out, gnp

    def two_launches(self, tile, splitk=1):
        """Today's form: the 1x1 GEMM stores a 16-bit skip tensor, the 3x3 convolution adds it as its residual."""
        ops, d, M, N = self.ops, self.d, self.M, self.N
        skip = torch.full((M, N), float("nan"), dtype=self.dtype, device=d)
        ops.launch(ops.make_igemm(dtype=self.dtype, a1=self.x, w=self.w1, out=skip, M=M, N=N, C1=self.C3, ld1=self.x.stride(0), ldw=self.C3,
                                  ldc=N, bias_n=self.b1))
        out = torch.full((M, N), float("nan"), dtype=self.dtype, device=d)
        ws = torch.empty(splitk * M * N, dtype=torch.float32, device=d) if splitk > 1 else None
        ops.launch(ops.make_igemm(dtype=self.dtype, a1=self.xn, w=self.w9, out=out, taps=9, M=M, N=N, C1=self.C1, ld1=self.C1, ldw=9 * self.C1,
                                  ldc=N, spatial=self.spatial(), bias_n=self.b9, rows_per_image=self.H * self.W, residual=skip, ldr=N, tile=tile,
                                  splitk=splitk, workspace=ws, a_gn=self.table, a_gn_silu=True))
        return out

    def check(self, tile, splitk=1, gn=False):
        out, gnp = self.fused(tile, splitk, gn)
        old = self.two_launches(tile, splitk)
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        elem(out, self.ref, self.absref, self.dtype, self.K, self.extra)
        # the skip tensor of the two-launch form is itself a stored 16-bit value: one more rounding (one spacing: 2u |skip|)
        extra = dict(self.extra)
        extra["16-bit skip tensor"] = 2.0 * unit_roundoff(self.dtype) * self.skipabs
        elem(old, self.ref, self.absref, self.dtype, self.K, extra)
        if gn:
            # the finalized per-image, per-channel sums against fp64 sums of the stored output (the tolerance of the fused-statistics
            # tests of tests/test_gpu_ops.py for a 16-bit output)
            got = gnp.double().reshape(self.B, -1, self.N, 2).sum(1).cpu()
            st = out.double().cpu().reshape(self.B, self.H * self.W, self.N)
            want = torch.stack([st.sum(1), (st * st).sum(1)], -1)
            assert torch.isfinite(got).all()
            assert float((got - want).abs().max() / want.abs().max()) < 5e-3
        return out


# ---- tile 16, 16 x 16 patches: one 48 x 48 image = corner, edge and interior patches; 1 and 3 tail chunks against 1 and 3 main
# chunks; ld3 > C3; split-K 3 with 3 tail chunks (one each) and with 1 (two splits get none); two column tiles
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C1,C3,ld3,N,splitk,gn", [
    (64, 64, 64, 128, 1, True),
    (64, 192, 320, 128, 1, False),
    (192, 64, 128, 128, 1, False),
    (192, 192, 192, 128, 1, False),
    (192, 192, 320, 128, 3, True),
    (192, 64, 64, 128, 3, False),
    (64, 64, 128, 256, 1, False),
])
def test_tile16_patches(dtype, C1, C3, ld3, N, splitk, gn):
    Case(dtype, 1, 48, 48, C1, C3, N, ld3).check(16, splitk, gn)


# ---- tile 16, four whole 8 x 8 images per workgroup
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("splitk,gn", [(1, False), (2, True)])
def test_tile16_8x8_images(dtype, splitk, gn):
    Case(dtype, 4, 8, 8, 128, 256, 128).check(16, splitk, gn)


# ---- tile 20: 16 x 16 pixels x 160 channels, 32-channel chunks (two units side by side: the seam between them)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C3,ld3,gn", [(64, 64, True), (128, 256, False)])
def test_tile20(dtype, C3, ld3, gn):
    Case(dtype, 1, 16, 32, 64, C3, 160, ld3).check(20, 1, gn)


# ---- tile 17: 2 x 2 units of 32 x 16 pixels; plain, and with the GroupNorm + SiLU of the 9-tap operand fused into its staging
# (the tail operand is NOT normalised)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("a_gn,gn", [(False, True), (True, False)])
def test_tile17(dtype, a_gn, gn):
    Case(dtype, 1, 32, 64, 128, 256, 128, a_gn=a_gn).check(17, 1, gn)


# ---- a3 == NULL (or C3 == 0) is the launch as it was, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,B,H,W,C1,N", [(16, 1, 48, 48, 128, 128), (16, 4, 8, 8, 128, 128), (20, 1, 16, 32, 64, 160), (17, 1, 32, 64, 128, 128)])
def test_no_tail_is_the_launch_as_it_was(dtype, tile, B, H, W, C1, N):
    c = Case(dtype, B, H, W, C1, 64, N)
    ops = c.ops
    outs = []
    for kw in (dict(), dict(a3=None, C3=64), dict(a3=c.x, C3=0)):
        out = torch.full((c.M, N), float("nan"), dtype=dtype, device=c.d)
        args = dict(dtype=dtype, a1=c.xn, w=c.w9, out=out, taps=9, M=c.M, N=N, C1=C1, ld1=C1, ldw=9 * C1, ldc=N, spatial=c.spatial(),
                    bias_n=c.b9, rows_per_image=H * W, tile=tile)
        args.update(kw)
        rec = ops.make_igemm(**args)
        assert " kt" not in rec.tag or kw.get("C3") == 0
        ops.launch(rec)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    wc = c.w9.double().cpu().reshape(N, 3, 3, C1).permute(0, 3, 1, 2)
    x9 = nchw(c.xn.double().cpu(), B, H, W)
    elem(outs[0], rows(F.conv2d(x9, wc, c.b9.double().cpu(), padding=1)), rows(F.conv2d(x9.abs(), wc.abs(), c.b9.double().cpu().abs(), padding=1)),
         dtype, 9 * C1)


# ---- everything else refuses a tail, from edtr_igemm and from edtr_igemm_plan alike, and launches nothing
def test_rejections():
    from edtr_amd import lib as L
    c = Case(torch.bfloat16, 1, 32, 32, 128, 64, 128)
    lib = L.load()
    out = torch.full((c.M, c.N), float("nan"), dtype=torch.bfloat16, device=c.d)
    x2 = torch.zeros((c.M, 64), dtype=torch.bfloat16, device=c.d)

    def params(**kw):
        return c.ops.igemm_params(dtype=torch.bfloat16, taps=9, M=c.M, N=c.N, a1=c.xn, C1=c.C1, ld1=c.C1, a3=c.x, C3=c.C3, w=c.wcat, ldw=c.K,
                                  out=out, ldc=c.N, bias_n=c.bsum, spatial=(c.H, c.W, c.H, c.W, 1, 1, 1, 0), rows_per_image=c.H * c.W, tile=16,
                                  raw=kw)

    stream = torch.cuda.current_stream().cuda_stream
    assert lib.edtr_igemm_plan(ctypes.byref(params())) == 16                          # the case itself is a valid launch
    bad = {
        "generic tile 3": dict(tile=3), "generic tile 1": dict(tile=1), "tile 8": dict(tile=8), "tile 6": dict(tile=6),
        "tile 21": dict(tile=21),
        "stride 2": dict(stride=2, OH=16, OW=16, M=256, rows_per_image=256),
        "upsample2x": dict(upsample2x=1, IH=16, IW=16),
        "C3 % 64": dict(C3=40, K=9 * c.C1 + 40),
        "C2 != 0": dict(a2=x2.data_ptr(), C2=64, ld2=64, K=9 * (c.C1 + 64) + c.C3),
        "a_gn on tile 16": dict(a_gn=c.bsum.data_ptr()),
    }
    for what, kw in bad.items():
        p = params(**kw)
        got, planned = lib.edtr_igemm(ctypes.byref(p), stream), lib.edtr_igemm_plan(ctypes.byref(p))
        assert got in (UNSUPPORTED, SHAPE) and planned == got, (what, got, planned)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all(), "a refused launch wrote to the output"
