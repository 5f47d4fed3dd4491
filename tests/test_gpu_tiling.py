"""The tiled flow on the MI355X (pytest -m gpu): the two window-table kernels (edtr_tile_gather, edtr_tile_blend) through
edtr_amd.ops.make_* and ops.launch with the conventions of tests/test_gpu_glue.py — destinations inside guard buffers, everything
outside the written region bit-unchanged, bit-exact where values are only moved, the rounding-aware element bound of
edtr_amd.testing.elem_ratio where they are computed — then `make_tiled_fn`'s batched branch against its per-window branch, and the
four tiling switches through `restore_batch`, `restore_dataset`, `restore_files` and the command line.  No case reaches a launch with
bad arguments: the error codes come from the host check of the table."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from edtr_amd.testing import elem_ratio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = torch.float32
PAD = 64                # guard elements in front of and behind every destination
# (B, C, H, W, size, stride): the last windows snapped on both axes with wi not a multiple of 4 (scalar rows); every wi a multiple
# of 4 (float4 rows); more than 4096 x 256 elements per launch (the grid-stride loops' second trip)
SHAPES = [(2, 5, 21, 30, 8, 4), (2, 5, 24, 32, 8, 4), (1, 3, 640, 640, 512, 128)]
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def guard_buf(shape, d):
    """A `shape` view PAD elements inside a NaN-filled flat buffer; returns (buffer, view, host copy before the launch)."""
    n = int(np.prod(shape))
    host = torch.full((n + 2 * PAD,), float("nan"), dtype=F32)
    buf = host.to(d)
    return buf, buf[PAD:PAD + n].view(shape), host


def guards_untouched(buf, before):
    a, b = bits(buf), bits(before)
    assert torch.equal(a[:PAD], b[:PAD]) and torch.equal(a[-PAD:], b[-PAD:]), "a guard element changed"


def exact(what, got, want):
    a, b = bits(got), bits(want)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError(f"{what}: {len(bad)} elements differ bitwise, first at {bad[0].tolist()}: "
                             f"{got.cpu()[tuple(bad[0])]} vs {want.cpu()[tuple(bad[0])]}")


class Case:
    """One shape's inputs, shared by the tests below and left unchanged: the plane, the table, random tiles, both weightings."""
    _made = {}

    def __init__(self, shape):
        from edtr_amd import tiling
        self.B, self.C, self.H, self.W, self.size, self.stride = shape
        self.windows = tiling.sliding_windows(self.H, self.W, self.size, self.stride)
        self.table = tiling.window_table(self.windows)
        self.n = len(self.windows)
        self.x = rnd((self.B, self.C, self.H, self.W), 300)
        self.tiles = rnd((self.n * self.B, self.C, self.size, self.size), 301)
        self.wts = {"gaussian": torch.tensor(tiling.gaussian_weights(self.size, self.size), dtype=F32),
                    "uniform": torch.ones((self.size, self.size), dtype=F32)}

    @classmethod
    def get(cls, shape):
        if shape not in cls._made:
            cls._made[shape] = cls(shape)
        return cls._made[shape]

    def device_table(self, d):
        from edtr_amd import tiling
        return tiling.device_windows(self.H, self.W, self.size, self.stride, d)


# =====================================================================================================================================
# 1. gather
# =====================================================================================================================================
@pytest.mark.parametrize("shape", SHAPES + [(2, 3, 640, 640, 512, 128)])      # the last: more than 4096 x 256 float4 units
def test_gather_is_slicing_and_cat_bit_for_bit(shape):
    from edtr_amd import ops, tiling
    d, c = dev(), Case.get(shape)
    if shape[0] == 2 and shape[2] == 21:
        assert any(wi % 4 for wi in c.table[:, 1]) and c.table[-1].tolist() == [21 - 8, 30 - 8]
    if shape[2] == 24:
        assert not any(wi % 4 for wi in c.table[:, 1])
    tab = c.device_table(d)
    assert torch.equal(tab.device.cpu(), torch.from_numpy(c.table)) and list(tab.host) == c.table.reshape(-1).tolist()
    x = c.x.to(d)
    buf, dst, before = guard_buf((c.n * c.B, c.C, c.size, c.size), d)
    ops.launch(ops.make_tile_gather(src=x, table_host=tab.host, table=tab.device, th=c.size, tw=c.size, dst=dst))
    torch.cuda.synchronize()
    want = torch.cat([x[..., hi:he, wi:we] for hi, he, wi, we in c.windows], dim=0)
    exact("tile_gather", dst, want)
    guards_untouched(buf, before)
    if c.H < 100:
        assert np.array_equal(dst.cpu().numpy(), tiling.gather_reference(c.x.numpy(), c.table, c.size, c.size))
    # a source that is only 4-byte aligned: every window moves element by element, same bytes
    if c.H < 100:
        xb = torch.empty((c.x.numel() + 1,), dtype=F32, device=d)
        xo = xb[1:].view(c.x.shape)
        xo.copy_(x)
        assert xo.data_ptr() % 16 == 4
        buf2, dst2, before2 = guard_buf((c.n * c.B, c.C, c.size, c.size), d)
        ops.launch(ops.make_tile_gather(src=xo, table_host=tab.host, table=tab.device, th=c.size, tw=c.size, dst=dst2))
        torch.cuda.synchronize()
        exact("tile_gather (unaligned source)", dst2, want)
        guards_untouched(buf2, before2)


# =====================================================================================================================================
# 2. / 3. blend
# =====================================================================================================================================
def _blend(c, d, wts):
    from edtr_amd import ops
    tab = c.device_table(d)
    buf, out, before = guard_buf((c.B, c.C, c.H, c.W), d)
    ops.launch(ops.make_tile_blend(tiles=c.tiles.to(d), wts=wts.to(d), table_host=tab.host, table=tab.device, th=c.size, tw=c.size, out=out))
    torch.cuda.synchronize()
    guards_untouched(buf, before)
    return out


@pytest.mark.parametrize("weight", ["gaussian", "uniform"])
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_against_the_fp64_restatement(shape, weight):
    """Per output pixel with c covering windows the kernel performs c fused multiply-adds for the numerator N = sum t w (one product
    and one addition each; at most 2^-24 relative error per operation on partial sums bounded by A = sum |t w|), c additions for
    the denominator D = sum w (all positive: error at most c 2^-24 D), and one division (the 2 u |ref| term).  To first order
    |err(N / D)| <= err(N) / D + |N| / D * err(D) / D, so with the file's 2^-22 per operation (four times the true unit, as in
    test_tile_accumulate_overlap_add_then_divide): bound = 2 u |ref| + 2^-22 * c * (A + |N|) / D — the cover c is folded into absref
    because it differs per pixel, k = 1."""
    from edtr_amd import tiling
    d, c = dev(), Case.get(shape)
    wts = c.wts[weight]
    out = _blend(c, d, wts)
    ref = tiling.blend_reference(c.tiles.numpy(), wts.numpy(), c.table, c.B, c.H, c.W)
    absn = tiling.blend_reference(c.tiles.abs().numpy(), wts.numpy(), c.table, c.B, c.H, c.W)          # A / D
    cover = np.zeros((c.H, c.W))
    for hi, wi in c.table:
        cover[hi:hi + c.size, wi:wi + c.size] += 1
    assert cover.max() >= 4 and cover.min() >= 1
    absref = torch.from_numpy(cover * (absn + np.abs(ref)))
    r, where = elem_ratio(out, torch.from_numpy(ref), absref, F32, 1)
    print(f"[tile_blend {shape} {weight}] worst element ratio {r:.3f}")
    assert r <= 1.0, f"tile_blend: element bound exceeded: ratio {r:.3g} at {where}"


@pytest.mark.parametrize("weight", ["gaussian", "uniform"])
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_has_the_bits_of_accumulate_then_divide(shape, weight):
    """Zeroed planes -> edtr_tile_accumulate per window in table order -> edtr_divide: the sequence the sampler ran per step."""
    from edtr_amd import ops
    d, c = dev(), Case.get(shape)
    wts = c.wts[weight].to(d)
    tiles = c.tiles.to(d)
    num = torch.zeros((c.B, c.C, c.H, c.W), dtype=F32, device=d)
    den = torch.zeros_like(num)
    for k, (hi, _, wi, _) in enumerate(c.windows):
        ops.launch(ops.make_tile_accumulate(tile=tiles[k * c.B:(k + 1) * c.B], wts=wts, out=num, count=den, B=c.B, C=c.C, H=c.H, W=c.W,
                                            th=c.size, tw=c.size, hi=hi, wi=wi))
    old = torch.empty_like(num)
    ops.launch(ops.make_divide(num=num, den=den, out=old, n=num.numel()))
    exact("tile_blend vs accumulate + divide", _blend(c, d, c.wts[weight]), old)


# =====================================================================================================================================
# 4. error codes (all decided on the host copy of the table: nothing is launched)
# =====================================================================================================================================
def test_error_codes_before_any_launch():
    from edtr_amd import lib, tiling
    d = dev()
    L = lib.load()
    c = Case.get(SHAPES[0])
    tab = c.device_table(d)
    x, tiles, wts = c.x.to(d), c.tiles.to(d), c.wts["gaussian"].to(d)
    bufg, dstg, beforeg = guard_buf((c.n * c.B, c.C, c.size, c.size), d)
    bufb, out, beforeb = guard_buf((c.B, c.C, c.H, c.W), d)
    P = lambda t: t.data_ptr()                                                       # noqa: E731
    s = torch.cuda.current_stream().cuda_stream

    def host(t):
        return (C.c_int32 * t.size)(*t.reshape(-1).tolist())

    def gather(src=P(x), th=None, n=c.n, dev_t=P(tab.device), dst=P(dstg), H=c.H):
        return L.edtr_tile_gather(src, c.B, c.C, H, c.W, th if th is not None else tab.host, dev_t, n, c.size, c.size, dst, s)

    def blend(t=P(tiles), w=P(wts), th=None, n=None, dev_t=P(tab.device), o=P(out)):
        th = th if th is not None else tab.host
        return L.edtr_tile_blend(t, w, th, dev_t, (len(th) // 2) if n is None else n, c.size, c.size, o, c.B, c.C, c.H, c.W, s)

    assert gather(src=None) == E_NULL and gather(dst=None) == E_NULL and gather(dev_t=None) == E_NULL
    assert blend(t=None) == E_NULL and blend(w=None) == E_NULL and blend(o=None) == E_NULL and blend(dev_t=None) == E_NULL
    assert gather(n=0) == E_SHAPE and gather(n=-3) == E_SHAPE and blend(n=0) == E_SHAPE
    outside = c.table.copy()
    outside[-1, 1] += 1                                                              # one column past the plane
    assert gather(th=host(outside)) == E_SHAPE and blend(th=host(outside)) == E_SHAPE
    assert gather(H=c.H - 1) == E_SHAPE                                              # the snapped windows no longer fit
    for drop in (0, c.n - 1):                                                        # a corner pixel lies in that window alone
        assert not tiling.table_covers(np.delete(c.table, drop, axis=0), c.size, c.size, c.H, c.W)
        assert blend(th=host(np.delete(c.table, drop, axis=0))) == E_SHAPE
    assert gather(src=P(x) + 2) == E_ALIGN and gather(dst=P(dstg) + 1) == E_ALIGN and gather(dev_t=P(tab.device) + 2) == E_ALIGN
    assert blend(t=P(tiles) + 2) == E_ALIGN and blend(o=P(out) + 3) == E_ALIGN
    torch.cuda.synchronize()
    assert torch.equal(bits(bufg), bits(beforeg)) and torch.equal(bits(bufb), bits(beforeb))             # nothing was written


# =====================================================================================================================================
# 5. make_tiled_fn: batched branch against per-window branch
# =====================================================================================================================================
@pytest.mark.parametrize("weight", ["gaussian", "uniform"])
def test_batched_branch_equals_per_window_branch(weight):
    """An elementwise fn on (2, 4, 16, 24) with 8 / 4 windows and max_batch 3: one window per group, fifteen groups, so the
    stacked buffer is filled slice by slice."""
    from edtr_amd.tiling import make_tiled_fn, sliding_windows
    d = dev()
    x = rnd((2, 4, 16, 24), 320).to(d)
    calls = []

    def fn(t):
        return t * 1.5 + 0.25

    def batched(tiles, windows):
        calls.append((tuple(tiles.shape), len(windows)))
        return fn(tiles)

    per_window = make_tiled_fn(fn, 8, 4, weight=weight)(x)
    stacked = make_tiled_fn(fn, 8, 4, weight=weight, batched_fn=batched, max_batch=3)(x)
    one_group = make_tiled_fn(fn, 8, 4, weight=weight, batched_fn=batched, max_batch=64)(x)
    torch.cuda.synchronize()
    n = len(sliding_windows(16, 24, 8, 4))
    assert calls == [((2, 4, 8, 8), 1)] * n + [((2 * n, 4, 8, 8), n)]
    exact("batched (15 groups) vs per-window", stacked, per_window)
    exact("batched (one group) vs per-window", one_group, per_window)


# =====================================================================================================================================
# 6. - 9. the switches through the public flow
# =====================================================================================================================================
TINY = dict(pre_res=True, pre_res_size=128, pre_res_stride=64, vae_encoder=True, vae_encoder_size=64, vae_decoder=True,
            vae_decoder_size=8, cldm=True, cldm_size=128, cldm_stride=64)          # the sizes of tests/golden/demo_tiled.npz


def _models(dtype, with_swinir=True):
    from edtr_amd import synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.model.swinir import SwinIR
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    d = dev()
    cfg = synth.tiny_config()
    cldm = build_synthetic_cldm(cfg, d, dtype)
    cldm.clip.set_embedding(synth.synth_input("demo:c_txt", (1, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(d))
    sw = None
    if with_swinir:
        sw = SwinIR(**synth.swinir_small_config())
        sw.load_state_dict({k: (synth.synth_param("swinirsmall." + k, tuple(v.shape)) if v.dtype.is_floating_point and not k.endswith("attn_mask") else v)
                            for k, v in sw.state_dict().items()}, strict=True)
        sw = sw.eval().to(d)
        sw.compute_dtype = dtype
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(d)
    return cldm, sw, diffusion, SpacedSampler(diffusion.betas)


def test_restore_batch_tiled_is_the_composition_of_the_public_pieces():
    """The plumbing adds no arithmetic: restore_batch(tiling = all four) on the 192 x 256 case equals, bit for bit, the pieces
    composed by hand; the caller's `cldm.forward` is what it was; an untiled call afterwards equals an untiled call before."""
    from edtr_amd import evalutil, synth
    from edtr_amd.evalutil import TilingOptions
    from edtr_amd.testing import injected_noise
    from edtr_amd.tiling import make_tiled_fn
    from edtr_amd.wavelet import wavelet_reconstruction
    cldm, sw, diffusion, sampler = _models(torch.float16)
    d = dev()
    x = evalutil.pad_to_multiples_of(evalutil.pad_if_smaller(synth.synth_input("demotiled:lq", (1, 3, 136, 200), 0.0, 1.0).to(d), 128), 64)
    assert tuple(x.shape) == (1, 3, 192, 256)
    noises = [synth.synth_normal(f"demotiled:noise{i}", (1, 4, 24, 32)) for i in range(5)]
    opt = TilingOptions(**TINY)
    assert opt.pre_res_tiled(192, 256) and opt.cldm_tiled(24, 32)
    forward_before = cldm.forward
    assert "forward" not in vars(cldm)

    def run(tiling):
        with injected_noise(noises):
            return evalutil.restore_batch(cldm, diffusion, sampler, x, swinir=sw, tiling=tiling)

    plain_before = run(None)
    got = run(opt)
    assert "forward" not in vars(cldm) and cldm.forward == forward_before              # the same bound method of the class again
    # by hand
    pre = make_tiled_fn(sw, 128, 64, batched_fn=lambda tiles, windows: sw(tiles))(x)
    z_pre = cldm.vae_encode(pre * 2 - 1, sample=False, tiled=True, tile_size=64)
    cldm.clip.compute_dtype = cldm.compute_dtype
    cond = dict(c_txt=cldm.clip.encode([""]), c_img=z_pre)
    try:
        with injected_noise(noises):
            x_T = diffusion.q_sample(z_pre, torch.full((1,), 200, dtype=torch.int64), torch.randn_like(z_pre))
            z = sampler.manual_sample_with_timesteps(model=cldm, device=d, x_T=x_T, steps=4, used_timesteps=[50, 100, 150, 200], batch_size=1,
                                                     cond=cond, uncond=None, cfg_scale=1.0, progress=False, tiled=True, tile_size=16,
                                                     tile_stride=8)
        assert "forward" in vars(cldm)                                                # the sampler itself leaves its patch behind
    finally:
        vars(cldm).pop("forward", None)
    want = wavelet_reconstruction((cldm.vae_decode(z, tiled=True, tile_size=8) + 1) / 2, pre)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())
    exact("restore_batch(tiling) vs the pieces by hand", got, want)
    assert not torch.equal(got, plain_before)                                         # the switches did something
    exact("untiled after tiled vs untiled before", run(None), plain_before)
    # a failing sampler call still takes the patch back
    with pytest.raises(RuntimeError, match="boom"):
        def boom(*a, **k):
            raise RuntimeError("boom")
        orig = sampler._loop
        sampler._loop = boom
        try:
            run(opt)
        finally:
            sampler._loop = orig
    assert "forward" not in vars(cldm)


# measured on the MI355X against tests/golden/demo_tiled.npz: relative L2 error of the restored 136 x 200 image (the max-norm
# max|a - b| / max|b| of the same runs: fp16 1.67e-3, bf16 1.44e-2).  Both are below what the untiled demo-flow test states for the same
# model (4e-3 / 3e-2).  The tolerance is the project's 1.5 x the measured error (the margin covers run-to-run choice of tiles).
MEASURED = {torch.float16: 1.20e-3, torch.bfloat16: 9.37e-3}
TOLERANCE = {dtype: 1.5 * err for dtype, err in MEASURED.items()}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_tiled_demo_flow_vs_reference_golden(golden_dir, dtype):
    """restore_dataset(pad_mode="demo", tiling = all four) on the 136 x 200 image against what the REFERENCE's own functions produced
    with all four stages tiled, on the same weights, input and noise (tools/make_goldens.py gen_demotiled -> demo_tiled.npz).
    Tolerance: 1.5 x the relative L2 error measured on the MI355X (fp16 1.20e-3 -> 1.8e-3, bf16 9.37e-3 -> 1.41e-2); max-norm
    (max|a - b| / max|b|, measured 1.67e-3 / 1.44e-2) below 3 x that tolerance, the project's MAX_OVER_L2."""
    from edtr_amd import evalutil, synth
    from edtr_amd.evalutil import TilingOptions
    from edtr_amd.testing import err_stats, injected_noise
    g = np.load(os.path.join(golden_dir, "demo_tiled.npz"))
    assert g["sizes"].tolist() == [TINY[k] for k in ("pre_res_size", "pre_res_stride", "vae_encoder_size", "vae_decoder_size", "cldm_size", "cldm_stride")]
    cldm, sw, diffusion, sampler = _models(dtype)
    img = synth.synth_input(str(g["input_name"]), (3, 136, 200), 0.0, 1.0)
    assert np.array_equal(img.numpy().astype(np.float16), g["input"])
    noises = [synth.synth_normal(str(n), tuple(g["z_pre"].shape)) for n in g["noise_names"]]
    with injected_noise(noises):
        outs, _ = evalutil.restore_dataset(cldm, diffusion, sampler, [img], img_size=128, swinir=sw, pad_mode="demo", multiple=64,
                                           clamp=False, tiling=TilingOptions(**TINY))
    torch.cuda.synchronize()
    assert len(outs) == 1 and tuple(outs[0].shape) == (3, 136, 200) == tuple(g["res"].shape)
    st = err_stats(outs[0], g["res"])
    tol = TOLERANCE[dtype]
    print(f"\n[tiled demo flow {dtype}] restored image vs the reference golden: {st} (tolerance {tol:.3g})")
    assert st["l2"] < tol and st["max"] < 3.0 * tol
    assert "forward" not in vars(cldm)


@pytest.fixture(scope="module")
def child():
    """One fresh process with EDTR_AMD_BATCH_INVARIANT=1 set before the package is imported (as tests/test_gpu_imagebatch.py does)."""
    dev()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tiling_child.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TILING_CHILD ")][-1]
    found = json.loads(line[len("TILING_CHILD "):])
    print(json.dumps(found, indent=1))
    return found


def test_seeded_tiled_run_does_not_depend_on_batch_size(child):
    """EDTR_AMD_BATCH_INVARIANT=1, seed 7, two images of one padded extent, encoder / sampler / decoder tiled: the batch of two
    (pad_mode="bucket") returns the tensors of one at a time (pad_mode="demo") bit for bit."""
    assert child["chunks"] == [[0, 1]]                                               # they did travel together
    assert child["shapes"] == [[3, 136, 200], [3, 150, 230]] and child["finite"]
    assert child["tiled_differs_from_untiled"] == [True, True]
    assert child["equal"] == [True, True], child["max_abs_diff"]
    assert child["forward_patched"] is False


def test_files_tiled_in_process_and_from_the_command_line(tmp_path):
    """One 136 x 200 PNG (latent 24 x 32: tiled 16 / 8) and one 100 x 100 PNG (latent 16 x 16: not larger than the tile, untiled)
    with --cldm-tiled and --pre-res-tiled at the tiny sizes: restore_files writes restore_dataset(return_uint8=True)'s bytes, and
    `python -m edtr_amd.restore --config tiny` with the flags, in a fresh process, writes the same files."""
    from edtr_amd import evalutil, imageio, restore
    from edtr_amd.evalutil import TilingOptions
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: restore_files has nothing to decode with")
    d = dev()
    rng = np.random.default_rng(11)
    raws = []
    for h, w in ((136, 200), (100, 100)):
        base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        raws.append(np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]))
    src = tmp_path / "in"
    src.mkdir()
    for k, a in enumerate(raws):
        Image.fromarray(a).save(str(src / f"im{k}.png"))
    paths = restore.list_images(str(src))
    opt = TilingOptions(pre_res=True, pre_res_size=128, pre_res_stride=64, cldm=True, cldm_size=128, cldm_stride=64)
    assert opt.cldm_tiled(192 // 8, 256 // 8) and not opt.cldm_tiled(128 // 8, 128 // 8)
    cldm, _, diffusion, sampler, kw = restore._build_tiny(d)
    written = restore.restore_files(cldm, diffusion, sampler, paths, str(tmp_path / "out"), scale=1.0, seed=3, tiling=opt, **kw)
    batched = restore.restore_files(cldm, diffusion, sampler, paths, str(tmp_path / "out_b"), scale=1.0, seed=3, tiling=opt, workers=1, **kw)
    imgs = [torch.from_numpy(a) for a in raws]
    outs, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, pad_mode="demo", seed=3, return_uint8=True, tiling=opt, **kw)
    plain, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, pad_mode="demo", seed=3, return_uint8=True, **kw)
    assert not torch.equal(outs[0], plain[0]) and torch.equal(outs[1], plain[1])      # the first ran tiled, the second did not
    r = subprocess.run([sys.executable, "-m", "edtr_amd.restore", "--input", str(src), "--output", str(tmp_path / "cli"), "--config", "tiny",
                        "--scale", "1.0", "--seed", "3", "--cldm-tiled", "--cldm-tile-size", "128", "--cldm-tile-stride", "64",
                        "--pre-res-tiled", "--pre-res-tile-size", "128", "--pre-res-tile-stride", "64"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cli = [ln for ln in r.stdout.splitlines() if ln.endswith(".png")]
    assert [os.path.basename(p) for p in written] == [os.path.basename(p) for p in cli] == ["im0.png", "im1.png"]
    for a, o, *files in zip(raws, outs, written, batched, cli):
        assert tuple(o.shape) == a.shape
        for path in files:
            with Image.open(path) as im:
                assert np.array_equal(np.array(im.convert("RGB")), o.cpu().numpy()), path
