"""The degradation stage without a GPU (edtr_amd/degrade.py, include/edtr_hip.h "Low-quality inputs"): the numpy restatements against
tests/golden/degrade.npz — outputs of the reference's own filter2D, F.interpolate, add_gaussian_noise_pt, DiffJPEG and blur-kernel
formulas, written by tools/make_degrade_goldens.py — the parameter draw, and the entry points' argument checks, which answer before
anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

from edtr_amd import degrade, lib, rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "degrade.npz"))


def err(a, b) -> float:
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def test_filter2d_reference_meets_the_reference(gold):
    """Tolerance (stored in the fixture): 4 x the error of the reference's fp32 filter2D against its own fp64 evaluation on these
    inputs, 4 x 4.6e-7 = 1.8e-6 — the factor is for a different summation order."""
    tol = float(gold["filter_tol"])
    assert 0 < tol < 1e-5 and tol == pytest.approx(4 * float(gold["filter_ref_err"]))
    for name in ("13", "3"):
        e = err(degrade.filter2d_reference(gold["filter_x"], gold[f"filter_k{name}"]), gold[f"filter_out{name}"])
        print(f"\n[filter2d k={name}] max abs err {e:.2e} (tol {tol:.2e})")
        assert e <= tol


@pytest.mark.parametrize("mode", degrade.MODES)
def test_resize_reference_meets_the_reference(gold, mode):
    """Tolerance per mode (stored in the fixture): 4 x the error of F.interpolate in fp32 against F.interpolate in fp64 over the three
    sizes — bilinear 4 x 1.9e-6, bicubic 4 x 2.3e-6, area 4 x 1.3e-7.  The identity resize must be exact."""
    tol = float(gold[f"resize_{mode}_tol"])
    assert 0 < tol < 2e-5 and tol == pytest.approx(4 * float(gold[f"resize_{mode}_ref_err"]))
    for n, size in enumerate(gold["resize_sizes"]):
        got = degrade.resize_reference(gold["resize_x"], tuple(int(v) for v in size), mode)
        e = err(got, gold[f"resize_{mode}_{n}"])
        print(f"\n[resize {mode} -> {tuple(size)}] max abs err {e:.2e} (tol {tol:.2e})")
        assert got.shape == gold[f"resize_{mode}_{n}"].shape and e <= tol
    assert np.array_equal(degrade.resize_reference(gold["resize_x"], (24, 40), mode), gold["resize_x"])


def test_noise_reference_equals_the_reference_given_its_noise(gold):
    """add_gaussian_noise_pt with torch.randn answered from the stream: (n * sigma) / 255 is the reference's own operation order, so
    the restatement is bit-equal — inside the issue's allowance of one fp32 rounding of sigma / 255."""
    x, n = gold["noise_x"], gold["noise_n"]
    got = degrade.add_gaussian_noise_reference(x, gold["noise_sigma"], gold["noise_gray"], noise=n)
    assert np.array_equal(got, gold["noise_out"])
    # the stream itself: grey images share one plane, colour images do not, and the supplied tensor is the float32 of the stream
    assert np.array_equal(n[1, 0], n[1, 1]) and np.array_equal(n[1, 0], n[1, 2]) and not np.array_equal(n[0, 0], n[0, 1])
    seed, ids = int(gold["noise_seed"]), gold["noise_ids"].tolist()
    assert np.array_equal(degrade.degrade_noise_reference(seed, ids, gold["noise_gray"], 0, 8, 12).astype(np.float32), n)
    assert np.array_equal(degrade.add_gaussian_noise_reference(x, gold["noise_sigma"], gold["noise_gray"], seed, ids), got)
    assert np.array_equal(n[1, 0].reshape(-1), rng.stream_reference(seed, [ids[1]], rng.PURPOSE_DEGRADE_GRAY, 0, 96)[0].astype(np.float32))
    rounded = degrade.add_gaussian_noise_reference(x, gold["noise_sigma"], gold["noise_gray"], noise=n, rounds=True)
    assert np.array_equal(rounded, (np.rint(rounded * np.float32(255)) / np.float32(255)).astype(np.float32)) and err(rounded, got) <= 0.5 / 255 + 1e-7
    with pytest.raises(ValueError):
        degrade.add_gaussian_noise_reference(np.zeros((1, 3, 3, 3), np.float32), 1.0, 0)        # H W % 4


def test_jpeg_reference_gives_the_reference_coefficients(gold):
    """Coefficients EQUAL: the fixture keeps every fp64 quotient >= 1e-4 from a rounding boundary while the fp32 quotient error is below
    2e-5.  Image within 4 x the reference's fp32-against-fp64 error, 4 x 1.7e-7."""
    assert float(gold["jpeg_margin"]) >= 1e-4 and float(gold["jpeg_quot_err"]) < 0.5 * float(gold["jpeg_margin"])
    tol = float(gold["jpeg_tol"])
    assert 0 < tol < 5e-6 and tol == pytest.approx(4 * float(gold["jpeg_ref_err"]))
    out, coefs, quot = degrade.jpeg_reference(gold["jpeg_x"], gold["jpeg_quality"], return_coefs=True, with_quotients=True)
    assert coefs.shape == gold["jpeg_coefs"].shape == (2, 36, 64)
    assert np.array_equal(coefs, gold["jpeg_coefs"])
    ours = float(np.abs(np.abs(quot - np.floor(quot)) - 0.5).min())
    e = err(out, gold["jpeg_out"])
    print(f"\n[jpeg] image max abs err {e:.2e} (tol {tol:.2e}); our quotients' margin {ours:.2e}")
    assert e <= tol
    assert np.array_equal(degrade.quality_to_factor([35.0, 90.0, 50.0]), np.array([5000 / 35 / 100, 0.2, 1.0], dtype=np.float32))
    for bad in (0.0, -1.0, 100.5, float("nan")):
        with pytest.raises(ValueError):
            degrade.quality_to_factor(bad)


def test_kernel_synthesis_matches_the_reference_formulas(gold):
    for n, kind in enumerate(gold["kernel_kinds"]):
        size, sx, sy, theta, beta = gold["kernel_args"][n]
        iso = kind == "iso" or kind.endswith("_iso")
        if kind in ("iso", "aniso"):
            k = degrade.bivariate_gaussian(int(size), sx, sy, theta, iso)
        elif kind.startswith("generalized"):
            k = degrade.bivariate_generalized_gaussian(int(size), sx, sy, theta, beta, iso)
        else:
            k = degrade.bivariate_plateau(int(size), sx, sy, theta, beta, iso)
        assert k.shape == gold[f"kernel{n}"].shape and err(k, gold[f"kernel{n}"]) <= 1e-6, kind
        assert abs(k.sum() - 1.0) < 1e-12
    gen = np.random.default_rng(1)
    for _ in range(20):
        k = degrade.random_mixed_kernel(gen, list(degrade.KERNEL_TYPES), [1] * 6, 21, (0.2, 3.0))
        assert k.shape == (21, 21) and np.isfinite(k).all() and (k >= 0).all() and abs(k.sum() - 1.0) < 1e-9


def test_draw_params_depends_on_seed_and_image_id_alone():
    cfg = degrade.load_config("realesrgan-stage1")

    def key(p):
        return (p.kernel.tobytes(), p.scale, p.mode, p.sigma, p.gray, p.quality, p.resize_back)

    ids = [7, 0, 2 ** 32 - 1, 3, 12]
    one_by_one = {i: key(degrade.draw_params(cfg, 99, i)) for i in ids}
    # another order, other companions, and the shards two ranks would walk: the same parameters for the same (seed, id)
    for order in (list(reversed(ids)), ids[1::2], ids[0::2]):
        for i in order:
            assert key(degrade.draw_params(cfg, 99, i)) == one_by_one[i]
    assert len(set(one_by_one.values())) == len(ids)
    assert key(degrade.draw_params(cfg, 100, 7)) != one_by_one[7]
    for i in ids:
        p = degrade.draw_params(cfg, 99, i)
        assert p.kernel.dtype == np.float32 and p.kernel.shape == (21, 21) and abs(float(p.kernel.sum()) - 1) < 1e-5
        assert 1.0 <= p.scale <= 1 / 0.15 and p.mode in degrade.MODES and 1.0 <= p.sigma <= 30.0 and 30.0 <= p.quality <= 95.0
        h, w = p.lq_size(101, 203)
        assert h % 2 == 0 and w % 2 == 0 and 2 <= h <= 101 and 2 <= w <= 203
    cf = degrade.draw_params(degrade.load_config("codeformer"), 1, 2)
    assert cf.resize_back and cf.mode == "bilinear" and cf.kernel.shape == (41, 41) and not cf.gray and 50.0 <= cf.quality < 100.0
    nested = degrade.DegradeConfig.from_dict({"dataset": {"target": "x", "params": {"blur_kernel_size": 21, "jpeg_range": [60, 90], "out_size": 512}}})
    assert nested.blur_kernel_size == 21 and list(nested.jpeg_range) == [60, 90]
    for bad in (dict(blur_kernel_size=20), dict(jpeg_range=(0, 50)), dict(downsample_range=(0.5, 2)), dict(kernel_list=("sinc",), kernel_prob=(1,))):
        with pytest.raises(ValueError):
            degrade.DegradeConfig(**bad)
    with pytest.raises(ValueError):
        degrade.draw_params(cfg, 1, 2 ** 32)


def test_new_symbols_resolve_and_the_abi_version_stays():
    L = lib.load()
    assert L.edtr_abi_version() == 10
    for name in ("edtr_degrade_filter2d", "edtr_degrade_resize", "edtr_degrade_gaussian_noise", "edtr_degrade_jpeg"):
        assert name in lib.DECLARED_SYMBOLS and getattr(L, name) is not None
    assert (rng.PURPOSE_DEGRADE, rng.PURPOSE_DEGRADE_GRAY) == (4, 5)
    assert np.array_equal(rng.stream_reference(3, [1], rng.PURPOSE_STEP, 2, 16), rng.normal_reference(3, [1], rng.PURPOSE_STEP, 2, 16))
    assert (lib.RESIZE_BILINEAR, lib.RESIZE_BICUBIC, lib.RESIZE_AREA) == (0, 1, 2) and degrade.MODES == ("bilinear", "bicubic", "area")


def test_entry_points_check_their_arguments_before_any_launch():
    """Every call below is refused on its arguments (host tables included) and launches nothing: the pointers are never followed."""
    L = lib.load()
    OK, E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5
    x, y, k = 0x10000, 0x20000, 0x30000                # 16-byte aligned stand-ins for device tensors
    f32s = lambda *v: (C.c_float * len(v))(*v)
    i32s = lambda *v: (C.c_int32 * len(v))(*v)
    # filter2d: even k, k out of range, k / 2 >= H (20 rows are too few for k = 41, 24 would do: the GPU test runs that one)
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 24, 48, k, 1, 4, None) == E_SHAPE
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 24, 48, k, 1, 1, None) == E_SHAPE
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 64, 64, k, 1, 43, None) == E_SHAPE
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 20, 48, k, 1, 41, None) == E_SHAPE
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 48, 20, k, 1, 41, None) == E_SHAPE
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 3, 48, k, 1, 7, None) == E_SHAPE
    assert L.edtr_degrade_filter2d(x, y, 2, 3, 24, 48, k, 3, 5, None) == E_SHAPE          # 3 kernels for 2 images
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 24, 48, None, 1, 5, None) == E_NULL
    assert L.edtr_degrade_filter2d(None, y, 1, 3, 24, 48, k, 1, 5, None) == E_NULL
    assert L.edtr_degrade_filter2d(x, y, 1, 4, 24, 48, k, 1, 5, None) == E_UNSUPPORTED
    assert L.edtr_degrade_filter2d(x, x, 1, 3, 24, 48, k, 1, 5, None) == E_UNSUPPORTED    # in place
    assert L.edtr_degrade_filter2d(x + 2, y, 1, 3, 24, 48, k, 1, 5, None) == E_ALIGN
    # resize
    assert L.edtr_degrade_resize(x, y, 1, 3, 24, 40, 0, 9, 0, None) == E_SHAPE
    assert L.edtr_degrade_resize(x, y, 0, 3, 24, 40, 7, 9, 0, None) == E_SHAPE
    assert L.edtr_degrade_resize(x, y, 1, 3, 24, 40, 7, 9, 3, None) == E_DTYPE
    assert L.edtr_degrade_resize(x, None, 1, 3, 24, 40, 7, 9, 0, None) == E_NULL
    # noise: per_image % 4, sigma and gray through the host copies, ids, draw
    sig, gry = f32s(5.0, 1.0), i32s(0, 1)
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 3, 6, sig, k, gry, k, 1, None, 0, 0, 0, None) == E_ALIGN     # H W = 18
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 5, 5, sig, k, gry, k, 1, None, 0, 0, 0, None) == E_ALIGN
    assert L.edtr_degrade_gaussian_noise(x + 4, y, None, 2, 3, 8, 12, sig, k, gry, k, 1, None, 0, 0, 0, None) == E_ALIGN  # not 16-byte
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, f32s(5.0, -1.0), k, gry, k, 1, None, 0, 0, 0, None) == E_SHAPE
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, f32s(float("nan"), 1.0), k, gry, k, 1, None, 0, 0, 0, None) == E_SHAPE
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, sig, k, i32s(0, 2), k, 1, None, 0, 0, 0, None) == E_DTYPE
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, sig, k, gry, k, 1, None, 0, 0, 2, None) == E_DTYPE       # rounds
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, sig, k, gry, k, 1, None, (1 << 32) - 1, 0, 0, None) == E_SHAPE
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, sig, k, gry, k, 1, None, 0, -1, 0, None) == E_SHAPE
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, None, k, gry, k, 1, None, 0, 0, 0, None) == E_NULL
    assert L.edtr_degrade_gaussian_noise(x, y, None, 2, 3, 8, 12, sig, None, gry, k, 1, None, 0, 0, 0, None) == E_NULL
    # jpeg: quality outside (0, 100] through the host copy
    for bad in (0.0, -5.0, 100.5, float("nan")):
        assert L.edtr_degrade_jpeg(x, y, 2, 3, 24, 40, f32s(50.0, bad), k, k, None, None) == E_SHAPE
    assert L.edtr_degrade_jpeg(x, y, 2, 3, 24, 40, None, k, k, None, None) == E_NULL
    assert L.edtr_degrade_jpeg(x, y, 2, 3, 24, 40, f32s(50.0, 100.0), None, k, None, None) == E_NULL
    assert L.edtr_degrade_jpeg(x, y, 2, 3, 24, 40, f32s(50.0, 100.0), k, None, None, None) == E_NULL
    assert L.edtr_degrade_jpeg(x, y, 2, 3, 0, 40, f32s(50.0, 100.0), k, k, None, None) == E_SHAPE
    assert OK == 0
    # the Python layer refuses the same things before it touches a device
    with pytest.raises(ValueError):
        degrade.filter2d_reference(np.zeros((1, 3, 20, 48), np.float32), np.ones((1, 41, 41), np.float32))
    with pytest.raises(ValueError):
        degrade.filter2d_reference(np.zeros((1, 3, 24, 48), np.float32), np.ones((1, 4, 4), np.float32))
    with pytest.raises(ValueError):
        degrade.resize_reference(np.zeros((1, 3, 8, 8), np.float32), (4, 4), "nearest")
