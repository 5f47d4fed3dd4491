"""The 8-bit image boundary on the device (csrc/imageio.hip, include/edtr_hip.h "Images in, images out"), through the C ABI: Pillow's
bicubic resize, ingest and emit bit for bit against their numpy / torch statements, the PSNR reduction against calculate_psnr_pt, and
the public flow (restore_dataset on uint8 images, pad_mode="seg", return_uint8, restore_files).  Every kernel output sits inside a
guarded buffer — at an aligned offset (the dword / float4 forms) and at an odd one (the element-by-element forms) — whose guards
must come back untouched.

EDTR_IMAGEIO_ERRLOG=<path> writes the figures measured here (profiles/imageio_errors.json is such a file)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS_JSON = os.path.join(ROOT, "profiles", "imageio_errors.json")
MEASURED = {}
USED = [50, 100, 150, 200]
GUARD_BYTE = 0xA5


def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return torch.device("cuda:0")


def _record():
    path = os.environ.get("EDTR_IMAGEIO_ERRLOG")
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def guarded_u8(shape, offset):
    """uint8 output of ``shape`` at byte ``offset`` of a buffer filled with GUARD_BYTE (offset 64: 4-byte aligned; 61: not)."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + 67,), GUARD_BYTE, dtype=torch.uint8, device="cuda:0")
    return buf, buf[offset:offset + n].view(shape)


def check_u8_guards(buf, shape, offset):
    n = int(np.prod(shape))
    assert bool((buf[:offset] == GUARD_BYTE).all()) and bool((buf[offset + n:] == GUARD_BYTE).all()), "a store landed outside the output"


def guarded_f32(shape, offset):
    """fp32 output at element ``offset`` of a NaN-filled buffer (offset 16: 16-byte aligned; 17: not)."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + 19,), float("nan"), dtype=torch.float32, device="cuda:0")
    return buf, buf[offset:offset + n].view(shape)


def check_f32_guards(buf, shape, offset):
    n = int(np.prod(shape))
    assert bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()), "a store landed outside the output"


def abi():
    from edtr_amd import lib, ops
    return lib, lib.load(), ops.stream_ptr()


def device_resize(img: np.ndarray, out_w: int, out_h: int, offset: int) -> np.ndarray:
    from edtr_amd import imageio
    lib, L, s = abi()
    d = dev()
    h, w, _ = img.shape
    src = torch.from_numpy(img).to(d)
    buf, dst = guarded_u8((out_h, out_w, 3), offset)
    tbuf, tmp = guarded_u8((h, out_w, 3), offset)
    ht = [torch.from_numpy(t).to(d) for t in imageio.resize_coeffs(w, out_w)] if out_w != w else None
    vt = [torch.from_numpy(t).to(d) for t in imageio.resize_coeffs(h, out_h)] if out_h != h else None
    P = lambda t: None if t is None else t.data_ptr()
    lib.check(L.edtr_image_resize_u8(P(src), h, w, 3, P(dst), out_h, out_w, P(ht and ht[0]), P(ht and ht[1]), ht[1].shape[1] if ht else 0,
                                     P(vt and vt[0]), P(vt and vt[1]), vt[1].shape[1] if vt else 0, P(tmp), s), "resize")
    torch.cuda.synchronize()
    check_u8_guards(buf, (out_h, out_w, 3), offset)
    check_u8_guards(tbuf, (h, out_w, 3), offset)
    return dst.cpu().numpy()


@pytest.mark.parametrize("offset", [64, 61])
def test_resize_equals_pillow_on_the_golden_shapes(golden_dir, offset):
    from edtr_amd import imageio
    g = np.load(os.path.join(golden_dir, "pillow_bicubic.npz"))
    for n in (str(v) for v in g["names"]):
        src, want = g[f"{n}_in"], g[f"{n}_out"]
        got = device_resize(src, want.shape[1], want.shape[0], offset)
        assert np.array_equal(got, imageio.resize_u8_reference(src, want.shape[1], want.shape[0])), n
        assert np.array_equal(got, want), n


@pytest.mark.parametrize("shape", [((2048, 1536), (512, 384)), ((100, 150), (341, 512))])
def test_resize_equals_the_reference_at_demo_sizes(shape):
    from edtr_amd import imageio
    (h, w), (oh, ow) = shape
    img = np.random.default_rng(h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[: h // 4, : w // 4] = np.where(np.indices((h // 4, w // 4)).sum(0)[..., None] % 2 == 0, 255, 0)       # ringing on both sides of the clamp
    want = imageio.resize_u8_reference(img, ow, oh)
    for offset in (64, 61):
        assert np.array_equal(device_resize(img, ow, oh, offset), want)
    assert np.array_equal(imageio.resize_u8(torch.from_numpy(img), ow, oh, device=dev()).cpu().numpy(), want)    # the public call


INGEST_CASES = [(37, 53, 64, 64), (40, 60, 64, 128), (64, 64, 64, 64), (5, 7, 6, 9), (12, 8, 12, 11), (1, 1, 8, 8)]   # h, w, H, W


@pytest.mark.parametrize("offset", [16, 17])
@pytest.mark.parametrize("replicate", [0, 1])
@pytest.mark.parametrize("f32", [0, 1])
def test_ingest_equals_divide_permute_pad(f32, replicate, offset):
    from edtr_amd import imageio
    lib, L, s = abi()
    d = dev()
    table = torch.from_numpy(imageio.INGEST_TABLE.copy()).to(d)
    for k, (h, w, H, W) in enumerate(INGEST_CASES):
        rng = np.random.default_rng(10 * k + f32)
        B, slot = 3, 1 + k % 2
        if f32:
            a = rng.uniform(-0.5, 1.5, size=(h, w, 3)).astype(np.float32)
            want = torch.from_numpy(a)
        else:
            a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            want = torch.from_numpy((a / 255.0).astype(np.float32))
        want = F.pad(want.permute(2, 0, 1)[None], (0, W - w, 0, H - h), mode="replicate" if replicate else "constant")
        src = torch.from_numpy(a).to(d)
        buf, batch = guarded_f32((B, 3, H, W), offset)
        lib.check(L.edtr_image_ingest(f32, src.data_ptr(), h, w, 3, batch.data_ptr(), slot, B, H, W, replicate, table.data_ptr(), s), "ingest")
        torch.cuda.synchronize()
        check_f32_guards(buf, (B, 3, H, W), offset)
        got = batch.cpu()
        assert torch.equal(got[slot:slot + 1].view(torch.int32), want.view(torch.int32)), (h, w, H, W)
        assert bool(torch.isnan(got[:slot]).all()) and bool(torch.isnan(got[slot + 1:]).all()), "another slot was written"
    # the public call: a mixed-size list, both paddings, pad_if_smaller -> pad_to_multiples_of extents
    imgs = [np.random.default_rng(50 + i).integers(0, 256, size=(hh, ww, 3), dtype=np.uint8) for i, (hh, ww) in enumerate(((37, 53), (64, 40)))]
    batch, sizes = imageio.ingest(imgs, pad="replicate" if replicate else "zero", min_size=48, multiple=32, device=d)
    assert sizes == [(37, 53), (64, 40)] and tuple(batch.shape) == (2, 3, 64, 64)
    for i, a in enumerate(imgs):
        want = F.pad(torch.from_numpy((a / 255.0).astype(np.float32)).permute(2, 0, 1)[None], (0, 64 - a.shape[1], 0, 64 - a.shape[0]),
                     mode="replicate" if replicate else "constant")
        assert torch.equal(batch[i:i + 1].cpu(), want)


@pytest.mark.parametrize("offset", [64, 61])
@pytest.mark.parametrize("f32_offset", [16, 17])
def test_emit_equals_save_image_quantisation(offset, f32_offset):
    from edtr_amd import imageio
    lib, L, s = abi()
    d = dev()
    for k, (h, w, H, W) in enumerate(INGEST_CASES + [(150, 100, 192, 128)]):
        B, slot = 3, k % 3
        g = torch.Generator().manual_seed(k)
        x = torch.rand((B, 3, H, W), generator=g) * 1.4 - 0.2
        x[slot, :, 0, 0] = torch.tensor([(100 + 0.5) / 255.0, 1.0, 0.0])
        x[slot, 1, h - 1, w - 1] = float("nan")
        _, batch = guarded_f32((B, 3, H, W), f32_offset)
        batch.copy_(x)
        buf, dst = guarded_u8((h, w, 3), offset)
        lib.check(L.edtr_image_emit(batch.data_ptr(), slot, B, 3, H, W, dst.data_ptr(), h, w, s), "emit")
        torch.cuda.synchronize()
        check_u8_guards(buf, (h, w, 3), offset)
        crop = x[slot, :, :h, :w]
        want = torch.nan_to_num(crop, nan=-1.0).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0)     # NaN -> 0 (documented)
        got = dst.cpu()
        assert torch.equal(got, want), (h, w, H, W)
        assert int(got[h - 1, w - 1, 1]) == 0
        assert np.array_equal(got.numpy(), imageio.emit_reference(crop.permute(1, 2, 0).numpy()))
        outs = imageio.emit(x.to(d), [(h, w)] * B)                                                                  # the public call
        assert torch.equal(outs[slot].cpu(), want)


def _psnr_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand((B, 3, H, W), generator=g)
    b = (a + 0.05 * torch.randn((B, 3, H, W), generator=g)).clamp(0, 1)          # MSE ~ 2e-3: far above the 1e-8 of the formula
    return a, b


def test_psnr_rgb_matches_calculate_psnr_pt():
    """The bound is derived, not measured: an fp64 sum of n <= 3 * 512^2 terms has relative error at most n 2^-53 = 9e-11 = 4e-10 dB
    on either side; asserted at 1e-9 dB."""
    from edtr_amd import evalutil, imageio
    d = dev()
    worst = 0.0
    for (B, H, W), cb in (((2, 512, 512), 0), ((3, 150, 100), 0), ((2, 37, 53), 4), ((1, 64, 64), 2)):
        a, b = _psnr_inputs(B, H, W, H + cb)
        want = evalutil.calculate_psnr_pt(a, b, crop_border=cb)
        ad, bd = a.to(d), b.to(d)
        got = imageio.psnr(ad, bd, crop_border=cb)
        again = imageio.psnr(ad, bd, crop_border=cb)
        s1, _ = imageio.sqdiff(ad, bd, crop_border=cb)
        s2, _ = imageio.sqdiff(ad, bd, crop_border=cb)
        assert got.dtype == torch.float64 and torch.equal(got, again) and torch.equal(s1.view(torch.int64), s2.view(torch.int64))
        assert float(want.min()) < 40.0                                         # MSE >> 1e-8
        err = float((got.cpu() - want).abs().max())
        print(f"\n[psnr rgb {B}x3x{H}x{W} crop {cb}] {got.cpu().tolist()} dB, max |diff| {err:.3e} dB")
        worst = max(worst, err)
        assert err <= 1e-9
    MEASURED["psnr_rgb_max_abs_diff_db"] = worst
    _record()


def guarded_f64(shape, offset):
    """fp64 output at element ``offset`` of a NaN-filled buffer (8-byte aligned at any offset, as the entry point requires)."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + 19,), float("nan"), dtype=torch.float64, device="cuda:0")
    return buf, buf[offset:offset + n].view(shape)


@pytest.mark.parametrize("y_channel", [0, 1])
@pytest.mark.parametrize("f32_offset", [16, 17])
def test_sqdiff_through_the_c_abi_stays_inside_guarded_partials_and_out(y_channel, f32_offset):
    """edtr_image_sqdiff called directly: fp32 inputs at a 16-byte aligned and at an odd element offset (the float4 and the scalar
    reads), `partials` and `out` inside NaN guards.  The reference is the same sum in fp64 on the host; each side carries at most
    (n + 2) 2^-53 relative error (n additions, one subtraction and one product per term, all terms non-negative), so the two may
    differ by 2 (n + 2) 2^-53 relative."""
    lib, L, s = abi()
    d = dev()
    B, H, W, cb = 3, 40, 52, 3
    sizes = [(40, 52), (37, 49), (7, 9)]
    a, b = _psnr_inputs(B, H, W, 90 + y_channel)
    _, ad = guarded_f32((B, 3, H, W), f32_offset)
    _, bd = guarded_f32((B, 3, H, W), f32_offset)
    ad.copy_(a)
    bd.copy_(b)
    dsizes = torch.tensor(sizes, dtype=torch.int32).to(d)
    pbuf, partials = guarded_f64((B, lib.SQDIFF_BLOCKS), 5)
    obuf, out = guarded_f64((B,), 3)
    lib.check(L.edtr_image_sqdiff(ad.data_ptr(), bd.data_ptr(), B, 3, H, W, dsizes.data_ptr(), cb, y_channel, partials.data_ptr(),
                                  out.data_ptr(), s), "sqdiff")
    torch.cuda.synchronize()
    for buf, offset, n in ((pbuf, 5, B * lib.SQDIFF_BLOCKS), (obuf, 3, B)):
        assert bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all()), "a store landed outside the output"
    got, parts = out.cpu(), partials.cpu()
    assert bool(torch.isfinite(parts).all()) and bool((parts >= 0).all())
    for i, (h, w) in enumerate(sizes):
        ai, bi = a[i, :, cb:h - cb, cb:w - cb].double(), b[i, :, cb:h - cb, cb:w - cb].double()
        if y_channel:
            luma = lambda t: (65.481 * t[0] + 128.553 * t[1] + 24.966 * t[2] + 16.0) / 255.0
            diff = luma(ai) - luma(bi)
        else:
            diff = ai - bi
        want = float((diff * diff).sum())
        n = diff.numel()
        bound = 2 * (n + 2) * 2.0 ** -53 * want
        if y_channel:
            # a luma (< 1.1) is 7 roundings: at most 8 * 2^-53 absolute; two lumas on either side move a difference d by at most
            # 32 * 2^-53, and d^2 by 2 |d| times that
            bound += 2 * 32 * 2.0 ** -53 * float(diff.abs().sum())
        print(f"\n[sqdiff abi y={y_channel} image {i}] {float(got[i])!r} vs {want!r}, |diff| {abs(float(got[i]) - want):.3e}, bound {bound:.3e}")
        assert want > 0 and abs(float(got[i]) - want) <= bound
        assert abs(float(parts[i].sum()) - float(got[i])) <= bound                        # out[i] is the sum of image i's partials


def test_psnr_of_a_padded_batch_is_each_images_own():
    from edtr_amd import evalutil, imageio
    d = dev()
    sizes = [(150, 100), (64, 64), (37, 53), (160, 128)]
    a, b = _psnr_inputs(len(sizes), 160, 128, 5)
    for cb, y in ((0, False), (3, False), (0, True)):
        got = imageio.psnr(a.to(d), b.to(d), sizes=sizes, crop_border=cb, test_y_channel=y).cpu()
        for i, (h, w) in enumerate(sizes):
            ai, bi = a[i:i + 1, :, :h, :w].contiguous(), b[i:i + 1, :, :h, :w].contiguous()
            alone = imageio.psnr(ai.to(d), bi.to(d), crop_border=cb, test_y_channel=y).cpu()
            assert abs(float(got[i]) - float(alone[0])) <= 1e-9, (i, cb, y)          # the same terms in another (fixed) order
            if not y:
                assert abs(float(got[i]) - float(evalutil.calculate_psnr_pt(ai, bi, crop_border=cb)[0])) <= 1e-9
    with pytest.raises(ValueError):
        imageio.psnr(a.to(d), b.to(d), sizes=sizes, crop_border=20)                  # nothing left of the 37 x 53 image


def test_psnr_y_channel_against_the_fp32_luma_of_the_reference():
    """calculate_psnr_pt(test_y_channel=True) rounds the luma to fp32 before the difference; edtr_image_sqdiff forms it in fp64, so
    equality is not owed.  The difference on these inputs is measured (profiles/imageio_errors.json, psnr_y_max_abs_diff_db) and gated
    at 4 x that figure — the margin the project gives sub-ulp reorderings — and never above 1e-4 dB."""
    from edtr_amd import evalutil, imageio
    d = dev()
    worst = 0.0
    for (B, H, W), cb in (((2, 512, 512), 0), ((3, 150, 100), 0), ((2, 37, 53), 4)):
        a, b = _psnr_inputs(B, H, W, 7 * H + cb)
        want = evalutil.calculate_psnr_pt(a, b, crop_border=cb, test_y_channel=True)
        got = imageio.psnr(a.to(d), b.to(d), crop_border=cb, test_y_channel=True)
        assert torch.equal(got, imageio.psnr(a.to(d), b.to(d), crop_border=cb, test_y_channel=True))
        err = float((got.cpu() - want).abs().max())
        print(f"\n[psnr y {B}x3x{H}x{W} crop {cb}] {got.cpu().tolist()} dB, max |diff| {err:.3e} dB")
        worst = max(worst, err)
    MEASURED["psnr_y_max_abs_diff_db"] = worst
    _record()
    assert os.path.exists(ERRORS_JSON), "profiles/imageio_errors.json (the measured figure the gate is derived from) is missing"
    with open(ERRORS_JSON) as f:
        measured = float(json.load(f)["psnr_y_max_abs_diff_db"])
    gate = min(4.0 * measured, 1e-4)
    print(f"[psnr y] worst {worst:.3e} dB, gate {gate:.3e} dB (4 x {measured:.3e})")
    assert worst <= gate


def test_bad_arguments_answer_the_documented_codes_and_launch_nothing():
    lib, L, s = abi()
    d = dev()
    u8 = torch.full((16 * 16 * 3,), 7, dtype=torch.uint8, device=d)
    f32 = torch.full((2 * 3 * 16 * 16,), 7.0, dtype=torch.float32, device=d)
    f64 = torch.full((2 * 64 + 2,), 7.0, dtype=torch.float64, device=d)
    i32 = torch.zeros(64, dtype=torch.int32, device=d)
    P = lambda t: t.data_ptr()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -5
    assert L.edtr_image_resize_u8(P(u8), 8, 8, 4, P(u8), 4, 4, P(i32), P(i32), 5, P(i32), P(i32), 5, P(u8), s) == E_UNSUPPORTED
    assert L.edtr_image_resize_u8(P(u8), 8, 8, 3, P(u8), 4, 4, None, None, 0, P(i32), P(i32), 5, P(u8), s) == E_NULL
    assert L.edtr_image_resize_u8(P(u8), 8, 8, 3, P(u8), 4, 4, P(i32), P(i32), 5, P(i32), P(i32), 5, None, s) == E_NULL      # both passes, no tmp
    assert L.edtr_image_resize_u8(P(u8), 8, 0, 3, P(u8), 4, 4, P(i32), P(i32), 5, P(i32), P(i32), 5, P(u8), s) == E_SHAPE
    assert L.edtr_image_ingest(0, P(u8), 16, 16, 1, P(f32), 0, 2, 16, 16, 0, P(f32), s) == E_UNSUPPORTED
    assert L.edtr_image_ingest(0, P(u8), 16, 16, 3, P(f32), 2, 2, 16, 16, 0, P(f32), s) == E_SHAPE                  # slot 2 of 2
    assert L.edtr_image_ingest(0, P(u8), 16, 17, 3, P(f32), 0, 2, 16, 16, 0, P(f32), s) == E_SHAPE                  # image wider than the slot
    assert L.edtr_image_ingest(0, P(u8), 16, 16, 3, P(f32), 0, 2, 16, 16, 0, None, s) == E_NULL                     # uint8 source, no table
    assert L.edtr_image_emit(P(f32), 0, 2, 1, 16, 16, P(u8), 16, 16, s) == E_UNSUPPORTED
    assert L.edtr_image_emit(P(f32), 0, 2, 3, 16, 16, P(u8), 17, 16, s) == E_SHAPE
    assert L.edtr_image_emit(P(f32), -1, 2, 3, 16, 16, P(u8), 16, 16, s) == E_SHAPE
    assert L.edtr_image_sqdiff(P(f32), P(f32), 2, 1, 16, 16, None, 0, 0, P(f64), P(f64), s) == E_UNSUPPORTED
    assert L.edtr_image_sqdiff(P(f32), P(f32), 2, 3, 16, 16, None, 0, 0, None, P(f64), s) == E_NULL
    assert L.edtr_image_sqdiff(P(f32), P(f32), 2, 3, 16, 16, None, -1, 0, P(f64), P(f64), s) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((u8 == 7).all()) and bool((f32 == 7.0).all()) and bool((f64 == 7.0).all())          # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------------
# the public flow on the tiny synthetic model
# ---------------------------------------------------------------------------------------------------------------------------------
_TINY = {}


def _tiny():
    from edtr_amd import synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    d = dev()
    if "cldm" not in _TINY:
        cfg = synth.tiny_config()
        cldm = build_synthetic_cldm(cfg, d, torch.float16)
        cldm.clip.set_embedding(synth.synth_input("demo:c_txt", (1, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(d))
        _TINY["cldm"] = cldm
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(d)
    return _TINY["cldm"], diffusion, SpacedSampler(diffusion.betas)


def _bytes_images():
    rng = np.random.default_rng(3)
    out = []
    for h, w in ((100, 75), (64, 128), (37, 53)):
        base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        out.append(np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]))        # 8 x 8 blocks: an image, not noise
    return out


def _as_float_chw(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy((a / 255.0).astype(np.float32)).permute(2, 0, 1).contiguous()


@pytest.mark.parametrize("pad_mode", ["batch", "demo"])
def test_restore_dataset_on_bytes_equals_restore_dataset_on_floats(pad_mode):
    from edtr_amd import evalutil
    cldm, diffusion, sampler = _tiny()
    imgs = _bytes_images()
    kw = dict(img_size=128, batch_size=2, pad_mode=pad_mode, multiple=64, seed=11)
    outs_f, psnr_f = evalutil.restore_dataset(cldm, diffusion, sampler, [_as_float_chw(a) for a in imgs], gts=[_as_float_chw(a) for a in imgs], **kw)
    outs_b, psnr_b = evalutil.restore_dataset(cldm, diffusion, sampler, [torch.from_numpy(a) for a in imgs], gts=imgs, **kw)
    outs_n, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, **kw)                              # numpy arrays
    torch.cuda.synchronize()
    assert len(outs_b) == len(imgs)
    for a, of, ob, on in zip(imgs, outs_f, outs_b, outs_n):
        assert tuple(ob.shape) == (3,) + a.shape[:2] and torch.isfinite(ob).all()
        assert torch.equal(of, ob) and torch.equal(of, on)
    assert abs(float(psnr_f) - float(psnr_b)) <= 1e-9 and 0.0 < float(psnr_b) < 60.0
    # return_uint8 = emit of the float result
    from edtr_amd import imageio
    outs_u, psnr_u = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, gts=imgs, return_uint8=True, **kw)
    for a, of, ou in zip(imgs, outs_f, outs_u):
        assert ou.dtype == torch.uint8 and tuple(ou.shape) == a.shape
        assert torch.equal(ou, imageio.emit(of[None].contiguous(), [a.shape[:2]])[0])
    assert 0.0 < float(psnr_u) < 60.0


@pytest.mark.parametrize("as_bytes", [False, True])
def test_pad_mode_seg_equals_the_steps_composed_by_hand(as_bytes):
    """main/seg/test_edtr.py:113-136 by hand: F.pad(mode='replicate') to multiples of 64 -> prepare_condition -> q_sample -> sampler ->
    vae_decode -> wavelet_reconstruction -> crop, with the seeded ids restore_dataset gives image k."""
    from edtr_amd import evalutil
    from edtr_amd.rng import NoiseSource
    from edtr_amd.wavelet import wavelet_reconstruction
    cldm, diffusion, sampler = _tiny()
    d = dev()
    imgs = _bytes_images()
    given = imgs if as_bytes else [_as_float_chw(a) for a in imgs]
    outs, _ = evalutil.restore_dataset(cldm, diffusion, sampler, given, pad_mode="seg", multiple=64, seed=5, clamp=False)
    assert len(outs) == len(imgs)
    for k, a in enumerate(imgs):
        h, w = a.shape[:2]
        x = _as_float_chw(a)[None].to(d)
        pre = F.pad(x, pad=(0, -w % 64, 0, -h % 64), mode="replicate")
        src = NoiseSource(5, [k])
        cond = cldm.prepare_condition(pre, [""])
        x_T = diffusion.q_sample(cond["c_img"], torch.full((1,), 200, dtype=torch.int64), src)
        z = sampler.manual_sample_with_timesteps(model=cldm, device=d, x_T=x_T, steps=4, used_timesteps=USED, batch_size=1, cond=cond,
                                                 uncond=None, cfg_scale=1.0, progress=False, noise_source=src)
        want = wavelet_reconstruction((cldm.vae_decode(z) + 1) / 2, pre)[0, :, :h, :w]
        torch.cuda.synchronize()
        assert tuple(outs[k].shape) == (3, h, w) and torch.isfinite(outs[k]).all()
        assert torch.equal(outs[k], want), k


def test_restore_files_writes_what_restore_dataset_returns(tmp_path):
    from edtr_amd import evalutil, imageio, restore
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("Pillow is not installed: restore_files has nothing to decode with")
    cldm, diffusion, sampler = _tiny()
    d = dev()
    src_dir, out_dir = tmp_path / "in", tmp_path / "out"
    src_dir.mkdir()
    raws = {}
    for name, a in zip(("a", "b", "c"), _bytes_images()):
        Image.fromarray(a).save(str(src_dir / f"{name}.png"))
        raws[name] = a
    paths = restore.list_images(str(src_dir))
    assert [os.path.basename(p) for p in paths] == ["a.png", "b.png", "c.png"]
    kw = dict(img_size=128, multiple=64)
    written = restore.restore_files(cldm, diffusion, sampler, paths, str(out_dir), scale=1.5, seed=9, **kw)
    assert [os.path.basename(p) for p in written] == ["a.png", "b.png", "c.png"]
    resized = [imageio.resize_u8(torch.from_numpy(raws[n]), *imageio.demo_size(raws[n].shape[1], raws[n].shape[0], 1.5), device=d) for n in "abc"]
    outs, _ = evalutil.restore_dataset(cldm, diffusion, sampler, resized, pad_mode="demo", seed=9, return_uint8=True, **kw)
    for n, path, r, o in zip("abc", written, resized, outs):
        with Image.open(path) as im:
            got = np.array(im.convert("RGB"))
        ow, oh = imageio.demo_size(raws[n].shape[1], raws[n].shape[0], 1.5)
        assert got.shape == (oh, ow, 3) == tuple(r.shape)
        assert np.array_equal(r.cpu().numpy(), np.array(Image.fromarray(raws[n]).resize((ow, oh), Image.BICUBIC)))
        assert np.array_equal(got, o.cpu().numpy())
