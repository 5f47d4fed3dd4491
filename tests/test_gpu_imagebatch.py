"""The ragged, batched image boundary on the device (csrc/imageio.hip: edtr_image_resize_h_batch, edtr_image_resize_ingest_batch,
edtr_image_emit_batch) through the C ABI — every slot / crop bit for bit what the per-image entry points and the numpy restatements
give, outputs inside NaN- / sentinel-filled buffers whose guards must come back untouched — and the flows built on it:
restore_dataset(pad_mode="bucket") and restore_files(batch_size, workers) on the tiny synthetic model."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD_BYTE = 0xA5
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -5


def dev():
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return torch.device("cuda:0")


def abi():
    from edtr_amd import lib, ops
    return lib, lib.load(), ops.stream_ptr()


def guarded_u8(n, offset):
    buf = torch.full((offset + n + 67,), GUARD_BYTE, dtype=torch.uint8, device="cuda:0")
    return buf, buf[offset:offset + n]


def guarded_f32(shape, offset):
    n = int(np.prod(shape))
    buf = torch.full((offset + n + 19,), float("nan"), dtype=torch.float32, device="cuda:0")
    return buf, buf[offset:offset + n].view(shape)


def f32_guards_ok(buf, shape, offset):
    n = int(np.prod(shape))
    return bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + n:]).all())


P = lambda t: None if t is None else t.data_ptr()       # noqa: E731


def _tables(n_in, n_out, d):
    from edtr_amd import imageio
    return [torch.from_numpy(t).to(d) for t in imageio.resize_coeffs(n_in, n_out)] if n_in != n_out else None


# (in_h, in_w) -> (out_h, out_w), the slot of the batch, the byte offset of the source inside its allocation
SIX = [((67, 45), (23, 16), 3, 0),          # both passes, downscale; out_w % 4 == 0: dword stores of the horizontal pass
       ((20, 30), (51, 77), 0, 0),          # both passes, upscale; odd widths: element by element
       ((33, 40), (33, 64), 6, 0),          # horizontal pass only (its scratch piece starts at an odd byte: no dwords despite out_w % 4 == 0)
       ((50, 28), (31, 28), 1, 0),          # vertical pass only, dword reads of the source
       ((24, 20), (24, 20), 5, 0),          # no pass: a plain ingest
       ((19, 13), (27, 13), 2, 1)]          # the source at an odd byte offset, w % 4 != 0
SLOTS = 7                                   # slot 4 belongs to nobody and must stay NaN


def _six_batch(d):
    """(sources, descriptors, device copy, scratch buffer + its guarded parent, everything to keep alive)"""
    from edtr_amd import lib
    keep, srcs = [], []
    descs = (lib.ImageDesc * len(SIX))()
    at = 0
    for i, ((h, w), (oh, ow), b, odd) in enumerate(SIX):
        a = np.random.default_rng(20 + i).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        a[: h // 3, : w // 3] = np.where(np.indices((h // 3, w // 3)).sum(0)[..., None] % 2 == 0, 255, 0)     # ringing on both sides of the clamp
        raw = torch.zeros(odd + a.size, dtype=torch.uint8, device=d)
        raw[odd:] = torch.from_numpy(a).reshape(-1).to(d)
        src = raw[odd:].view(h, w, 3)
        assert src.data_ptr() % 4 == odd
        ht, vt = _tables(w, ow, d), _tables(h, oh, d)
        x = descs[i]
        x.src, x.in_h, x.in_w, x.out_h, x.out_w, x.b = src.data_ptr(), h, w, oh, ow, b
        if ht:
            if i == 2:
                at += 1                                     # an odd start for the piece of image 2
            x.h_bounds, x.h_coefs, x.h_ksize, x.tmp_offset = ht[0].data_ptr(), ht[1].data_ptr(), ht[1].shape[1], at
            at += h * ow * 3
            at += -at % 4
        if vt:
            x.v_bounds, x.v_coefs, x.v_ksize = vt[0].data_ptr(), vt[1].data_ptr(), vt[1].shape[1]
        keep += [raw, ht, vt]
        srcs.append((a, src, ht, vt))
    tbuf, tmp = guarded_u8(at, 64)
    ddescs = torch.frombuffer(descs, dtype=torch.uint8).to(d)
    return srcs, descs, ddescs, tbuf, tmp, keep


@pytest.mark.parametrize("W,offset", [(80, 16), (79, 17)])
@pytest.mark.parametrize("replicate", [0, 1])
def test_six_ragged_images_in_one_launch_pair_equal_resize_then_ingest(replicate, W, offset):
    """One batch that takes every branch: the slots equal edtr_image_resize_u8 + edtr_image_ingest on the same bytes and the numpy
    restatement, exactly; the guards around the batch and the scratch buffer, and the slot nobody owns, come back untouched."""
    from edtr_amd import imageio
    lib, L, s = abi()
    d = dev()
    H = 55
    srcs, descs, ddescs, tbuf, tmp, keep = _six_batch(d)
    table = torch.from_numpy(imageio.INGEST_TABLE.copy()).to(d)
    buf, batch = guarded_f32((SLOTS, 3, H, W), offset)
    lib.check(L.edtr_image_resize_h_batch(descs, P(ddescs), len(SIX), 3, P(tmp), tmp.numel(), s), "resize_h_batch")
    lib.check(L.edtr_image_resize_ingest_batch(descs, P(ddescs), len(SIX), 3, P(tmp), tmp.numel(), P(batch), SLOTS, H, W, replicate,
                                               P(table), s), "resize_ingest_batch")
    torch.cuda.synchronize()
    assert f32_guards_ok(buf, (SLOTS, 3, H, W), offset), "a store landed outside the batch"
    assert bool((tbuf[:64] == GUARD_BYTE).all()) and bool((tbuf[64 + tmp.numel():] == GUARD_BYTE).all()), "a store landed outside the scratch buffer"
    got = batch.cpu()
    assert bool(torch.isnan(got[4]).all()), "the slot of no image was written"
    want_np, sizes = imageio.ingest_resized_reference([a for a, *_ in srcs], [(ow, oh) for _, (oh, ow), _, _ in SIX], size=(H, W),
                                                      pad="replicate" if replicate else "zero")
    assert sizes == [o for _, o, _, _ in SIX]
    # the per-image entry points on the same bytes
    _, ref = guarded_f32((SLOTS, 3, H, W), offset)
    for (a, src, ht, vt), ((h, w), (oh, ow), b, _) in zip(srcs, SIX):
        small = torch.empty((oh, ow, 3), dtype=torch.uint8, device=d)
        t1 = torch.empty((h, ow, 3), dtype=torch.uint8, device=d)
        lib.check(L.edtr_image_resize_u8(P(src), h, w, 3, P(small), oh, ow, P(ht and ht[0]), P(ht and ht[1]), ht[1].shape[1] if ht else 0,
                                         P(vt and vt[0]), P(vt and vt[1]), vt[1].shape[1] if vt else 0, P(t1), s), "resize")
        lib.check(L.edtr_image_ingest(0, P(small), oh, ow, 3, P(ref), b, SLOTS, H, W, replicate, P(table), s), "ingest")
    torch.cuda.synchronize()
    ref = ref.cpu()
    for i, (_, _, b, _) in enumerate(SIX):
        assert torch.equal(got[b].view(torch.int32), ref[b].view(torch.int32)), f"image {i}: not what resize_u8 + ingest write"
        assert np.array_equal(got[b].numpy().view(np.uint32), want_np[i].view(np.uint32)), f"image {i}: not the numpy restatement"
    del keep


def test_golden_shapes_through_the_batch_path_equal_pillow(golden_dir, monkeypatch):
    """`imageio.ingest_resized` (the public call: host images in one upload, at most two launches) on tests/golden/pillow_bicubic.npz:
    every slot's top-left corner is Pillow's bytes / 255, the rest of the slot is zero."""
    from edtr_amd import imageio, ops
    d = dev()
    g = np.load(os.path.join(golden_dir, "pillow_bicubic.npz"))
    names = [str(n) for n in g["names"]]
    images, wants = [g[f"{n}_in"] for n in names], [g[f"{n}_out"] for n in names]
    launched = []
    real = ops.launch
    monkeypatch.setattr(ops, "launch", lambda rec: (launched.append(rec.name), real(rec))[1])
    batch, sizes = imageio.ingest_resized(images, [(w.shape[1], w.shape[0]) for w in wants], multiple=64, device=d)
    torch.cuda.synchronize()
    assert launched == ["image.resize_h_batch", "image.resize_ingest_batch"]
    assert sizes == [w.shape[:2] for w in wants]
    H, W = imageio.batch_extent(sizes, multiple=64)
    assert tuple(batch.shape) == (len(names), 3, H, W)
    got = batch.cpu().numpy()
    for b, want in enumerate(wants):
        ref = np.zeros((3, H, W), dtype=np.float32)
        ref[:, :want.shape[0], :want.shape[1]] = (want / 255.0).astype(np.float32).transpose(2, 0, 1)
        assert np.array_equal(got[b].view(np.uint32), ref.view(np.uint32)), names[b]
    # device-resident sources and replicate padding: the same bits as resize_u8 -> ingest
    on_dev = [torch.from_numpy(a).to(d) for a in images[:3]]
    outs = [(w.shape[1], w.shape[0]) for w in wants[:3]]
    b2, _ = imageio.ingest_resized(on_dev, outs, pad="replicate", min_size=48, multiple=32)
    b1, _ = imageio.ingest([imageio.resize_u8(t, ow, oh) for t, (ow, oh) in zip(on_dev, outs)], pad="replicate", min_size=48, multiple=32)
    assert torch.equal(b1, b2)


CROPS = [(2, 24, 20), (0, 5, 7), (4, 1, 1), (1, 17, 16)]           # slot, h, w: 5 x 7 and 1 x 1 have w % 4 != 0


@pytest.mark.parametrize("W,f32_offset", [(20, 16), (21, 17)])
def test_four_ragged_crops_in_one_launch_equal_emit_per_image(W, f32_offset):
    from edtr_amd import imageio
    lib, L, s = abi()
    d = dev()
    B, H = 5, 24
    g = torch.Generator().manual_seed(W)
    x = torch.rand((B, 3, H, W), generator=g) * 1.4 - 0.2                       # below 0 and above 1 on both sides
    x[0, :, 0, 0] = torch.tensor([(100 + 0.5) / 255.0, 1.0, 0.0])
    x[0, 1, 4, 6] = float("nan")
    x[2, 2, 23, 19] = float("nan")
    x[1, 0, 0, 1], x[1, 1, 0, 1], x[1, 2, 0, 1] = -3.0, 7.0, float("inf")
    _, batch = guarded_f32((B, 3, H, W), f32_offset)
    batch.copy_(x)
    # offsets of the host's choosing: 4-byte aligned, with gaps between the crops
    offs, at = [], 8
    for _, h, w in CROPS:
        offs.append(at)
        at += h * w * 3
        at += -at % 4 + 12
    n_bytes = at
    buf, dst = guarded_u8(n_bytes, 64)
    rows = [v for (b, h, w), o in zip(CROPS, offs) for v in (b, h, w, o)]
    host = (ctypes.c_int64 * len(rows))(*rows)
    table = torch.tensor(rows, dtype=torch.int64).to(d)
    lib.check(L.edtr_image_emit_batch(P(batch), B, 3, H, W, host, P(table), len(CROPS), P(dst), n_bytes, s), "emit_batch")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    covered = np.zeros(got.shape, dtype=bool)
    for (b, h, w), o in zip(CROPS, offs):
        one = torch.empty((h, w, 3), dtype=torch.uint8, device=d)
        lib.check(L.edtr_image_emit(P(batch), b, B, 3, H, W, P(one), h, w, s), "emit")
        torch.cuda.synchronize()
        mine = got[64 + o:64 + o + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(mine, one.cpu().numpy()), (b, h, w)
        assert np.array_equal(mine, imageio.emit_reference(x[b, :, :h, :w].permute(1, 2, 0).numpy())), (b, h, w)
        covered[64 + o:64 + o + h * w * 3] = True
    assert (got[~covered] == GUARD_BYTE).all(), "a byte outside the crops was written"
    assert got[64 + offs[1] + (4 * 7 + 6) * 3 + 1] == 0                          # the NaN of slot 0 inside the 5 x 7 crop
    assert got[64 + offs[3] + 3:64 + offs[3] + 6].tolist() == [0, 255, 255]      # -3, 7, inf
    # the public call: `emit`'s bytes at the packed offsets, one buffer
    packed, views = imageio.emit_packed(x.to(d), [(h, w) for _, h, w in [(0, 24, 20), (1, 5, 7), (2, 1, 1), (3, 17, 16), (4, 24, 3)]])
    singles = imageio.emit(x.to(d), [(24, 20), (5, 7), (1, 1), (17, 16), (24, 3)])
    want, want_offs = imageio.emit_packed_reference(x.numpy(), [(24, 20), (5, 7), (1, 1), (17, 16), (24, 3)])
    assert packed.numel() == want.size
    for v, one, o in zip(views, singles, want_offs):
        assert torch.equal(v, one) and v.data_ptr() - packed.data_ptr() == o


def test_bad_arguments_answer_the_documented_codes_and_launch_nothing():
    from edtr_amd import imageio
    lib, L, s = abi()
    d = dev()
    u8 = torch.full((4096,), 7, dtype=torch.uint8, device=d)
    f32 = torch.full((2 * 3 * 16 * 16,), float("nan"), dtype=torch.float32, device=d)
    tabs = _tables(8, 16, d)
    table = torch.from_numpy(imageio.INGEST_TABLE.copy()).to(d)

    def desc(**kw):
        x = (lib.ImageDesc * 1)()
        v = dict(src=P(u8), in_h=8, in_w=8, out_h=16, out_w=16, b=0, h_bounds=P(tabs[0]), h_coefs=P(tabs[1]), h_ksize=tabs[1].shape[1],
                 v_bounds=P(tabs[0]), v_coefs=P(tabs[1]), v_ksize=tabs[1].shape[1], tmp_offset=1024)
        v.update(kw)
        for k, val in v.items():
            setattr(x[0], k, val)
        return x, torch.frombuffer(x, dtype=torch.uint8).to(d)

    def h_batch(x, dx, B=1, ch=3, tmp=u8, n=2048):
        return L.edtr_image_resize_h_batch(x, P(dx), B, ch, P(tmp), n, s)

    def ingest(x, dx, B=1, ch=3, tmp=u8, n=2048, batch=f32, slots=2, H=16, W=16, tab=table):
        return L.edtr_image_resize_ingest_batch(x, P(dx), B, ch, P(tmp), n, P(batch), slots, H, W, 0, P(tab), s)

    good = desc()
    for call in (h_batch, ingest):
        assert call(*good, B=0) == E_SHAPE
        assert call(*good, ch=4) == E_UNSUPPORTED
        assert call(*desc(h_bounds=None)) == E_NULL                 # a horizontal pass is requested, its table is not there
        assert call(*desc(v_coefs=None)) == E_NULL
        assert call(*desc(src=None)) == E_NULL
        assert call(*good, tmp=None) == E_NULL                      # a horizontal pass and no scratch buffer
        assert call(*desc(out_w=-16)) == E_SHAPE
        assert call(*desc(in_h=-8)) == E_SHAPE
        assert call(*desc(tmp_offset=2048 - 8 * 16 * 3 + 1)) == E_SHAPE      # the horizontal result would end past the scratch buffer
        assert call(*desc(h_bounds=P(tabs[0]) + 2)) == E_ALIGN
        assert call(None, good[1]) == E_NULL
    assert ingest(*good, H=15) == E_SHAPE                           # a slot smaller than the image
    assert ingest(*good, W=12) == E_SHAPE
    assert ingest(*desc(b=2)) == E_SHAPE                            # slot 2 of 2
    assert ingest(*good, batch=None) == E_NULL
    assert ingest(*good, tab=None) == E_NULL
    rows = lambda *v: ((ctypes.c_int64 * 4)(*v), torch.tensor(v, dtype=torch.int64).to(d))      # noqa: E731

    def emit(host, table_d, B=2, ch=3, H=16, W=16, n=1, dst=u8, n_bytes=2048):
        return L.edtr_image_emit_batch(P(f32), B, ch, H, W, host, P(table_d), n, P(dst), n_bytes, s)

    assert emit(*rows(0, 16, 16, 0), B=0) == E_SHAPE
    assert emit(*rows(0, 16, 16, 0), ch=1) == E_UNSUPPORTED
    assert emit(*rows(2, 16, 16, 0)) == E_SHAPE                     # slot 2 of 2
    assert emit(*rows(0, 17, 16, 0)) == E_SHAPE                     # a crop larger than the slot
    assert emit(*rows(0, -1, 16, 0)) == E_SHAPE
    assert emit(*rows(0, 16, 16, 2)) == E_ALIGN                     # offsets are multiples of 4
    assert emit(*rows(0, 16, 16, 2048 - 16 * 16 * 3 + 4)) == E_SHAPE        # the crop would end past dst
    assert emit(*rows(0, 16, 16, 0), dst=None) == E_NULL
    assert emit(None, None) == E_NULL
    torch.cuda.synchronize()
    assert bool((u8 == 7).all()) and bool(torch.isnan(f32).all())           # nothing was launched
    # and the good arguments are good
    assert h_batch(*good) == 0 and ingest(*good) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f32[:3 * 16 * 16]).all()) and bool(torch.isnan(f32[3 * 16 * 16:]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the flows on the tiny synthetic model
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


def _images():
    """the child's images (same sizes, same bytes), without running the child's module-level environment change in this process"""
    rng = np.random.default_rng(3)
    out = []
    for h, w in ((100, 75), (64, 128), (37, 53), (130, 60), (90, 100)):
        base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        out.append(np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]))
    return out


def test_bucket_mode_on_bytes_equals_bucket_mode_on_floats_in_data_set_order():
    from edtr_amd import evalutil, imageio
    cldm, diffusion, sampler = _tiny()
    imgs = _images()
    floats = [torch.from_numpy((a / 255.0).astype(np.float32)).permute(2, 0, 1).contiguous() for a in imgs]
    kw = dict(img_size=128, batch_size=3, pad_mode="bucket", multiple=64, seed=7)
    plan = imageio.plan_buckets([a.shape[:2] for a in imgs], 3, min_size=128, multiple=64)
    assert [idx for _, idx in plan] == [[0, 1, 2], [4], [3]]                    # image 3 runs last and must come back fourth
    outs_b, psnr_b = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, gts=imgs, **kw)
    outs_f, psnr_f = evalutil.restore_dataset(cldm, diffusion, sampler, floats, gts=floats, **kw)
    torch.cuda.synchronize()
    assert len(outs_b) == len(outs_f) == len(imgs)
    for a, ob, of in zip(imgs, outs_b, outs_f):
        assert tuple(ob.shape) == (3,) + a.shape[:2] and bool(torch.isfinite(ob).all())
        assert torch.equal(ob, of)
    assert abs(float(psnr_b) - float(psnr_f)) <= 1e-9 and 0.0 < float(psnr_b) < 60.0
    outs_u, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, return_uint8=True, **kw)            # through emit_packed
    for a, of, ou in zip(imgs, outs_f, outs_u):
        assert ou.dtype == torch.uint8 and tuple(ou.shape) == a.shape
        assert torch.equal(ou, imageio.emit(of[None].contiguous(), [a.shape[:2]])[0])
    outs_n, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, **dict(kw, seed=None))               # unseeded: it runs
    assert [tuple(o.shape) for o in outs_n] == [tuple(o.shape) for o in outs_b]


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """One fresh process with EDTR_AMD_BATCH_INVARIANT=1 set before the package is imported; the tests below read what it found."""
    pytest.importorskip("PIL", reason="Pillow is not installed: restore_files has nothing to decode with")
    dev()
    work = tmp_path_factory.mktemp("imagebatch")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "imagebatch_child.py"), str(work)], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("IMAGEBATCH_CHILD ")][-1]
    found = json.loads(line[len("IMAGEBATCH_CHILD "):])
    print(json.dumps(found, indent=1))
    return found


def test_bucketed_in_threes_equals_one_at_a_time_in_invariant_mode(child):
    """The claim that makes batching safe to offer: pad_mode="bucket", batch_size=3, seed=7 returns, image for image, the exact
    tensors of pad_mode="demo", seed=7 (EDTR_AMD_BATCH_INVARIANT=1; without it no bit equality is claimed)."""
    assert child["dataset_shapes"] == [[3, 100, 75], [3, 64, 128], [3, 37, 53], [3, 130, 60], [3, 90, 100]]
    assert child["dataset_finite"]
    assert child["dataset_equal"] == [True] * 5, child["dataset_max_abs_diff"]


def test_files_in_batches_with_workers_equal_files_one_at_a_time(child):
    names = [f"im{k}.png" for k in range(5)]
    assert child["files_names"] == [names, names, names]                        # data-set order, whatever the bucket order
    # scale 1.25: images 0, 2 and 4 share the 128 x 128 bucket, 80 x 160 pads to 128 x 192 and 162 x 75 to 192 x 128
    assert child["files_shapes"] == [[125, 93, 3], [80, 160, 3], [46, 66, 3], [162, 75, 3], [112, 125, 3]]
    assert child["files_equal"] == [True] * 5
    assert child["corrupt_raised"] is not None, "a corrupt file went unnoticed"


def test_restore_files_without_the_new_keywords_is_the_demo_flow(tmp_path):
    from edtr_amd import evalutil, imageio, restore
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: restore_files has nothing to decode with")
    cldm, diffusion, sampler = _tiny()
    d = dev()
    src_dir = tmp_path / "in"
    src_dir.mkdir()
    raws = _images()[:3]
    for k, a in enumerate(raws):
        Image.fromarray(a).save(str(src_dir / f"im{k}.png"))
    paths = restore.list_images(str(src_dir))
    kw = dict(img_size=128, multiple=64)
    written = restore.restore_files(cldm, diffusion, sampler, paths, str(tmp_path / "out"), scale=1.5, seed=9, **kw)
    assert [os.path.basename(p) for p in written] == ["im0.png", "im1.png", "im2.png"]
    resized = [imageio.resize_u8(torch.from_numpy(a), *imageio.demo_size(a.shape[1], a.shape[0], 1.5), device=d) for a in raws]
    outs, _ = evalutil.restore_dataset(cldm, diffusion, sampler, resized, pad_mode="demo", seed=9, return_uint8=True, **kw)
    for path, o in zip(written, outs):
        with Image.open(path) as im:
            assert np.array_equal(np.array(im.convert("RGB")), o.cpu().numpy())
