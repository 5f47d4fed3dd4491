"""The degradation kernels on the device against their numpy restatements (edtr_amd/degrade.py), by EQUALITY: every kernel of
csrc/degrade.hip is a bit-exact function of its inputs.  Shapes are the smallest at which each can still go wrong: reflect borders on
all four sides and several 32 x 32 tiles for the blur, a halo larger than the image interior at k = 41, uneven `area` windows and
clamped bicubic borders for the resize, padding on both axes and both branches of quality_to_factor for the JPEG step."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from edtr_amd import degrade, lib, ops, rng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
FILL_TOL = 1e-5             # tests/test_gpu_rng.py's tolerance of edtr_normal_fill against rng.normal_reference


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "degrade.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rand(*shape, seed=0):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def same(got, want, what=""):
    """bit equality of two arrays (device tensors are copied); what differs is printed before the assertion"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    if bad.any():
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print(f"\n[{what}] {int(bad.sum())} of {bad.size} elements differ, max abs {np.nanmax(d):.3e}, first at {tuple(np.argwhere(bad)[0])}")
    return not bad.any()


def kernels(n, k, seed=1):
    gen = np.random.default_rng(seed)
    return np.stack([degrade.random_mixed_kernel(gen, list(degrade.KERNEL_TYPES), [1] * 6, k, (0.3, 4.0)) for _ in range(n)]).astype(np.float32)


@pytest.mark.parametrize("k", [3, 13])
def test_filter2d_equals_the_restatement(k, gold):
    x = rand(2, 3, 20, 28)
    for ker in (kernels(2, k), kernels(1, k, seed=2)):          # per-image and shared
        got = degrade.filter2d(dev(x), ker).cpu().numpy()
        assert same(got, degrade.filter2d_reference(x, ker))
    # and the reference's own output on its fixture, within the tolerance the fixture carries (4 x the reference's fp32 error)
    got = degrade.filter2d(dev(gold["filter_x"]), gold[f"filter_k{k}"]).cpu().numpy()
    assert np.abs(got.astype(np.float64) - gold[f"filter_out{k}"]).max() <= float(gold["filter_tol"])


def test_filter2d_k41_halo_larger_than_the_image():
    """1 x 3 x 24 x 48 at k = 41: the halo (20) nearly covers the image; 20 rows are refused, 24 accepted.  48 columns: two tiles."""
    x = rand(1, 3, 24, 48, seed=3)
    for ker in (kernels(1, 41, seed=4), kernels(1, 41, seed=5)[0]):
        assert same(degrade.filter2d(dev(x), ker), degrade.filter2d_reference(x, ker))
    two = rand(2, 3, 24, 48, seed=6)
    ker = kernels(2, 41, seed=7)
    assert same(degrade.filter2d(dev(two), ker), degrade.filter2d_reference(two, ker))
    with pytest.raises(RuntimeError):
        degrade.filter2d(dev(x[:, :, :20]), ker[:1])
    with pytest.raises(RuntimeError):
        degrade.filter2d(dev(x), np.ones((1, 4, 4), np.float32))


@pytest.mark.parametrize("size", [(7, 9), (24, 40), (37, 61)])
@pytest.mark.parametrize("mode", degrade.MODES)
def test_resize_equals_the_restatement(mode, size, gold):
    x = gold["resize_x"]                                        # 2 x 3 x 24 x 40
    got = degrade.resize(dev(x), size, mode).cpu().numpy()
    assert got.shape == (2, 3) + size
    assert same(got, degrade.resize_reference(x, size, mode))
    if size == (24, 40):
        assert same(got, x)
    n = [tuple(s) for s in gold["resize_sizes"].tolist()].index(size)
    assert np.abs(got.astype(np.float64) - gold[f"resize_{mode}_{n}"]).max() <= float(gold[f"resize_{mode}_tol"])


def test_noise_stream_add_and_clamp(gold):
    """3 x 3 x 8 x 12, ids [5, 0, 2^32 - 1], image 1 grey.  The stream meets the host reference at rng's tolerance; the add and the clamp
    around it are bit-equal to the restatement given the device's own noise; an image's result does not depend on its companions."""
    x, sigma, gray = gold["noise_x"], gold["noise_sigma"], gold["noise_gray"]
    seed, ids = int(gold["noise_seed"]), gold["noise_ids"].tolist()
    assert ids == [5, 0, 2 ** 32 - 1] and gray.tolist() == [0, 1, 0]
    src = rng.NoiseSource(seed, ids)
    out, noise = degrade.add_gaussian_noise(dev(x), sigma, gray, src, return_noise=True)
    n = noise.cpu().numpy()
    want = degrade.degrade_noise_reference(seed, ids, gray, 0, 8, 12)
    e = float(np.abs(n.astype(np.float64) - want).max())
    print(f"\n[degrade noise] stream max abs err {e:.2e} (tol {FILL_TOL:g})")
    assert e <= FILL_TOL
    assert torch.equal(noise[1, 0], noise[1, 1]) and torch.equal(noise[1, 0], noise[1, 2]) and not torch.equal(noise[0, 0], noise[0, 1])
    assert same(out, degrade.add_gaussian_noise_reference(x, sigma, gray, noise=n))
    assert torch.equal(out, degrade.add_gaussian_noise(dev(x), sigma, gray, src))              # without noise_out: the same bits
    rounded = degrade.add_gaussian_noise(dev(x), sigma, gray, src, rounds=True).cpu().numpy()
    assert same(rounded, degrade.add_gaussian_noise_reference(x, sigma, gray, noise=n, rounds=True))
    another = degrade.add_gaussian_noise(dev(x), sigma, gray, src, draw=1)
    assert not torch.equal(another, out)
    # batch-position independence: every image alone, and the batch in another order
    for b in range(3):
        one = degrade.add_gaussian_noise(dev(x[b:b + 1]), sigma[b:b + 1], gray[b:b + 1], rng.NoiseSource(seed, [ids[b]]))
        assert torch.equal(one[0], out[b])
    perm = [2, 0, 1]
    moved = degrade.add_gaussian_noise(dev(x[perm]), sigma[perm], gray[perm], rng.NoiseSource(seed, [ids[p] for p in perm]))
    assert torch.equal(moved, out[perm])
    # ids by base (image_ids == NULL): ids 15, 16
    L, xs = lib.load(), dev(x[:2])
    o = torch.empty_like(xs)
    sg, gr = dev(sigma[:2]), dev(gray[:2])
    lib.check(L.edtr_degrade_gaussian_noise(xs.data_ptr(), o.data_ptr(), None, 2, 3, 8, 12, (C.c_float * 2)(*[float(v) for v in sigma[:2]]), sg.data_ptr(),
                                            (C.c_int32 * 2)(*[int(v) for v in gray[:2]]), gr.data_ptr(), seed, None, 15, 0, 0, ops.stream_ptr()), "noise")
    assert torch.equal(o, degrade.add_gaussian_noise(xs, sigma[:2], gray[:2], rng.NoiseSource.for_shard(seed, 15, 2)))


def test_jpeg_equals_the_restatement_and_the_reference_coefficients(gold):
    """The golden's 2 x 3 x 24 x 40 at qualities 35 and 90: padding on both axes (to 32 x 48), both branches of quality_to_factor."""
    x, q = gold["jpeg_x"], gold["jpeg_quality"]
    assert q.tolist() == [35.0, 90.0]
    out, coefs = degrade.jpeg(dev(x), q, return_coefs=True)
    want, want_coefs = degrade.jpeg_reference(x, q, return_coefs=True)
    assert same(coefs, want_coefs)
    assert same(coefs, gold["jpeg_coefs"])                  # the reference's own coefficients: no flips
    assert same(out, want)
    assert np.abs(out.cpu().numpy().astype(np.float64) - gold["jpeg_out"]).max() <= float(gold["jpeg_tol"])
    assert torch.equal(degrade.jpeg(dev(x), q), out)                                # without the coefficient output: the same bits
    # per-image quality: each image alone gives its rows of the batch
    for b in range(2):
        assert torch.equal(degrade.jpeg(dev(x[b:b + 1]), q[b:b + 1])[0], out[b])


def test_jpeg_without_padding_and_over_many_mcus():
    x = rand(1, 3, 16, 16, seed=8)
    out, coefs = degrade.jpeg(dev(x), 75.0, return_coefs=True)
    want, want_coefs = degrade.jpeg_reference(x, 75.0, return_coefs=True)
    assert same(coefs, want_coefs) and same(out, want)
    big = rand(1, 3, 40, 280, seed=9)          # 3 x 18 = 54 MCUs in one image, odd crop on both axes
    assert same(degrade.jpeg(dev(big), 20.0), degrade.jpeg_reference(big, 20.0))
    with pytest.raises(ValueError):
        degrade.jpeg(dev(x), 0.0)


def _params(n, seed=11):
    cfg = degrade.DegradeConfig(blur_kernel_size=7, kernel_list=degrade.KERNEL_TYPES, kernel_prob=(1,) * 6, blur_sigma=(0.3, 2.0),
                                downsample_range=(1.0, 2.5), noise_range=(1.0, 20.0), jpeg_range=(30.0, 95.0), gray_noise_prob=0.5,
                                resize_back=True, resize_modes=degrade.MODES)
    return cfg, [degrade.draw_params(cfg, seed, i) for i in range(n)]


def test_degrade_batch_equals_the_images_one_at_a_time():
    """two images of different extents in one padded batch = each degraded alone = the chain of the numpy restatements"""
    sizes = [(24, 40), (32, 28)]
    hq = np.zeros((2, 3, 32, 40), np.float32)
    for b, (h, w) in enumerate(sizes):
        hq[b, :, :h, :w] = rand(3, h, w, seed=20 + b)
    _, params = _params(2)
    ids = [9, 4]
    both = degrade.degrade_batch(dev(hq), params, 77, ids, sizes)
    for b, (h, w) in enumerate(sizes):
        alone = degrade.degrade_batch(dev(hq[b:b + 1, :, :h, :w]), [params[b]], 77, [ids[b]])[0]
        assert tuple(both[b].shape) == (3, h, w) and torch.equal(both[b], alone)
        p = params[b]
        x = degrade.filter2d_reference(hq[b:b + 1, :, :h, :w], p.kernel)
        x = degrade.resize_reference(x, p.lq_size(h, w), p.mode)
        noise = degrade.add_gaussian_noise(dev(x), [p.sigma], [p.gray], rng.NoiseSource(77, [ids[b]]), return_noise=True)[1].cpu().numpy()
        x = degrade.add_gaussian_noise_reference(x, [p.sigma], [p.gray], noise=noise)
        x = degrade.resize_reference(degrade.jpeg_reference(x, [p.quality]), (h, w), p.back_mode)
        assert same(both[b], x[0])


def test_degrade_files_writes_the_same_bytes_for_batch_size_1_and_2(tmp_path):
    from PIL import Image
    src = tmp_path / "in"
    src.mkdir()
    gen = np.random.default_rng(5)
    for name, (h, w) in (("a", (24, 40)), ("b", (32, 28)), ("c", (24, 40))):
        Image.fromarray(gen.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / f"{name}.png")
    cfg, _ = _params(0)
    paths = sorted(str(p) for p in src.iterdir())
    one = degrade.degrade_files(paths, str(tmp_path / "one"), cfg, 3, batch_size=1)
    two = degrade.degrade_files(paths, str(tmp_path / "two"), cfg, 3, batch_size=2, workers=2)
    assert len(one) == len(two) == 3
    for (g1, l1), (g2, l2), p in zip(one, two, paths):
        assert os.path.basename(l1) == os.path.basename(p) and l1.endswith(os.path.join("lq", os.path.basename(p)))
        for f1, f2 in ((g1, g2), (l1, l2)):
            with open(f1, "rb") as a, open(f2, "rb") as b:
                assert a.read() == b.read()
        assert same(np.array(Image.open(g1)), np.array(Image.open(p)))
        assert Image.open(l1).size == Image.open(p).size and not same(np.array(Image.open(l1)), np.array(Image.open(p)))


def test_bad_arguments_answer_the_documented_codes_and_launch_nothing():
    """every rejection of the four entry points of csrc/degrade.hip, code by code: one thing changed at a time on a valid call"""
    L, s = lib.load(), ops.stream_ptr()
    x = torch.zeros((2, 3, 4, 4), dtype=torch.float32, device=DEV)
    out, noise_out = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    ker = torch.full((2, 3, 3), 1.0 / 9.0, dtype=torch.float32, device=DEV)
    sig = torch.ones(2, dtype=torch.float32, device=DEV)
    gry = torch.zeros(2, dtype=torch.int32, device=DEV)
    ids = torch.zeros(2, dtype=torch.int64, device=DEV)
    dct = torch.zeros((64, 64), dtype=torch.float32, device=DEV)
    P = lambda t: t.data_ptr()
    f32s, i32s = lambda *v: (C.c_float * len(v))(*v), lambda *v: (C.c_int32 * len(v))(*v)
    E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_UNSUPPORTED = -1, -2, -3, -4, -5
    batch = dict(x=P(x), out=P(out), B=2, channels=3, H=4, W=4)
    noise = dict(x=P(x), out=P(out), noise_out=P(noise_out), B=2, channels=3, H=4, W=4)
    valid = {      # the arguments in the order of the entry point (H, W: in_h, in_w of the resize)
        "filter2d": (L.edtr_degrade_filter2d, dict(batch, kernels=P(ker), n_kernels=2, k=3)),
        "resize": (L.edtr_degrade_resize, dict(batch, out_h=4, out_w=4, mode=lib.RESIZE_BILINEAR)),
        "gaussian_noise": (L.edtr_degrade_gaussian_noise, dict(noise, sigma_host=f32s(1.0, 1.0), sigma=P(sig), gray_host=i32s(0, 0), gray=P(gry),
                                                               seed=1, image_ids=None, image_id_base=0, draw=0, rounds=0)),
        "jpeg": (L.edtr_degrade_jpeg, dict(batch, quality_host=f32s(50.0, 50.0), factor=P(sig), dct=P(dct), coefs=None)),
    }

    def code(name, **change):
        fn, args = valid[name]
        assert set(change) <= set(args)
        return fn(*{**args, **change}.values(), s)

    for name in valid:
        for change, want in ((dict(channels=1), E_UNSUPPORTED), (dict(channels=1, x=None), E_UNSUPPORTED),      # the channel check comes first
                             (dict(x=None), E_NULL), (dict(out=None), E_NULL), (dict(B=0), E_SHAPE), (dict(B=65536), E_SHAPE),
                             (dict(H=(1 << 24) + 4), E_UNSUPPORTED), (dict(x=P(x) + 2), E_ALIGN)):
            assert code(name, **change) == want, (name, change)
    for change, want in ((dict(sigma_host=None), E_NULL), (dict(rounds=2), E_DTYPE), (dict(rounds=2, draw=-1), E_DTYPE),   # rounds before draw
                         (dict(draw=-1), E_SHAPE), (dict(draw=1 << 32), E_SHAPE), (dict(H=3, W=3), E_ALIGN),              # H W % 4
                         (dict(sigma_host=f32s(-1.0, 1.0)), E_SHAPE), (dict(sigma_host=f32s(1.0, float("nan"))), E_SHAPE),
                         (dict(gray_host=i32s(2, 0)), E_DTYPE), (dict(image_ids=P(ids) + 4), E_ALIGN),
                         (dict(image_ids=None, image_id_base=(1 << 32) - 1), E_SHAPE),                                   # image_id_base + B > 2^32
                         (dict(x=P(x) + 4), E_ALIGN)):                                                                    # the 16-byte rule
        assert code("gaussian_noise", **change) == want, change
    for change, want in ((dict(k=4), E_SHAPE), (dict(k=43), E_SHAPE), (dict(n_kernels=3), E_SHAPE), (dict(out=P(x)), E_UNSUPPORTED)):
        assert code("filter2d", **change) == want, change
    for change, want in ((dict(mode=3), E_DTYPE), (dict(out_h=0), E_SHAPE)):
        assert code("resize", **change) == want, change
    for q in (0.0, 101.0):
        assert code("jpeg", quality_host=f32s(50.0, q)) == E_SHAPE, q
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((noise_out == 7.0).all()) and bool((x == 0.0).all())      # nothing was launched
