"""The host side of the second-order degradation chain (edtr_amd/degrade.py): the Poisson inversion tables and their sampler, the sinc
and USM kernels, `RealESRGANConfig` / `draw_params2`, the numpy chain, and the argument checks of the three new entry points.  The
reference's own outputs and every tolerance come from tests/golden/degrade2.npz (tools/make_degrade2_goldens.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from edtr_amd import degrade, lib, rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2024


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "degrade2.npz"))


def test_new_symbols_resolve_and_the_abi_version_stays():
    L = lib.load()
    assert L.edtr_abi_version() == 10
    for name in ("edtr_degrade_poisson_noise", "edtr_degrade_sepblur", "edtr_degrade_usm_apply"):
        assert name in lib.DECLARED_SYMBOLS and getattr(L, name) is not None
    assert (rng.PURPOSE_DEGRADE_POISSON, rng.PURPOSE_DEGRADE_POISSON_GRAY) == (6, 7)
    # the raw words are those the normals are made of, and the normal stream keeps refusing the Poisson purposes
    w = rng.uniform_words_reference(3, [1, 9], rng.PURPOSE_DEGRADE, 2, 16)
    assert w.dtype == np.uint32 and w.shape == (2, 16)
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    z = rng.stream_reference(3, [1, 9], rng.PURPOSE_DEGRADE, 2, 16)
    assert np.array_equal(z[:, 0], np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    with pytest.raises(ValueError):
        rng.stream_reference(3, [1], rng.PURPOSE_DEGRADE_POISSON, 0, 16)
    assert not np.array_equal(rng.uniform_words_reference(3, [1], 6, 0, 16), rng.uniform_words_reference(3, [1], 7, 0, 16))


def test_entry_points_check_their_arguments_before_any_launch():
    """Every call below is refused on its arguments (host arrays included) and launches nothing: the pointers are never followed."""
    L = lib.load()
    E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_UNSUPPORTED = -1, -2, -3, -4, -5
    x, y, k, m = 0x10000, 0x20000, 0x30000, 0x40000        # 16-byte aligned stand-ins for device tensors
    f32s = lambda *v: (C.c_float * len(v))(*v)
    i32s = lambda *v: (C.c_int32 * len(v))(*v)
    # sepblur: NULLs, channels, k even / above 63 / too large for the extent, aliasing
    assert L.edtr_degrade_sepblur(None, y, None, 1, 3, 40, 70, k, 51, 0.0, None) == E_NULL
    assert L.edtr_degrade_sepblur(x, None, None, 1, 3, 40, 70, k, 51, 0.0, None) == E_NULL
    assert L.edtr_degrade_sepblur(x, y, None, 1, 3, 40, 70, None, 51, 0.0, None) == E_NULL
    assert L.edtr_degrade_sepblur(x, y, None, 1, 4, 40, 70, k, 51, 0.0, None) == E_UNSUPPORTED
    assert L.edtr_degrade_sepblur(x, y, None, 1, 3, 40, 70, k, 50, 0.0, None) == E_SHAPE
    assert L.edtr_degrade_sepblur(x, y, None, 1, 3, 40, 70, k, 1, 0.0, None) == E_SHAPE
    assert L.edtr_degrade_sepblur(x, y, None, 1, 3, 80, 80, k, 65, 0.0, None) == E_SHAPE
    assert L.edtr_degrade_sepblur(x, y, None, 1, 3, 25, 70, k, 51, 0.0, None) == E_SHAPE           # k / 2 = 25 >= H
    assert L.edtr_degrade_sepblur(x, y, None, 1, 3, 70, 31, k, 63, 0.0, None) == E_SHAPE           # k / 2 = 31 >= W
    assert L.edtr_degrade_sepblur(x, y, m, 1, 3, 40, 70, k, 51, float("nan"), None) == E_SHAPE
    assert L.edtr_degrade_sepblur(x, x, None, 1, 3, 40, 70, k, 51, 0.0, None) == E_UNSUPPORTED
    assert L.edtr_degrade_sepblur(x, y, y, 1, 3, 40, 70, k, 51, 0.0, None) == E_UNSUPPORTED
    assert L.edtr_degrade_sepblur(x + 2, y, None, 1, 3, 40, 70, k, 51, 0.0, None) == E_ALIGN
    # usm_apply
    assert L.edtr_degrade_usm_apply(x, None, k, y, 1, 3, 40, 70, 0.5, None) == E_NULL
    assert L.edtr_degrade_usm_apply(x, k, None, y, 1, 3, 40, 70, 0.5, None) == E_NULL
    assert L.edtr_degrade_usm_apply(x, k, m, None, 1, 3, 40, 70, 0.5, None) == E_NULL
    assert L.edtr_degrade_usm_apply(x, k, m, y, 1, 1, 40, 70, 0.5, None) == E_UNSUPPORTED
    assert L.edtr_degrade_usm_apply(x, k, m, y, 0, 3, 40, 70, 0.5, None) == E_SHAPE
    assert L.edtr_degrade_usm_apply(x, k, m, y, 1, 3, 40, 70, float("nan"), None) == E_SHAPE
    # poisson noise: (x, out, noise_out, B, ch, H, W, scale_host, scale, gray_host, gray, tables, lows, levels, counts_out, seed, ids, base, draw, rounds)
    sc, gry = f32s(1.0, 2.0), i32s(0, 1)

    def poisson(xx=x, out=y, ch=3, H=8, W=12, sh=sc, sd=k, gh=gry, gd=k, tables=m, lows=m, levels=m, base=0, draw=0, rounds=0):
        return L.edtr_degrade_poisson_noise(xx, out, None, 2, ch, H, W, sh, sd, gh, gd, tables, lows, levels, None, 1, None, base, draw, rounds, None)

    assert poisson(xx=None) == E_NULL and poisson(out=None) == E_NULL and poisson(sh=None) == E_NULL and poisson(sd=None) == E_NULL
    assert poisson(gh=None) == E_NULL and poisson(gd=None) == E_NULL
    assert poisson(tables=None) == E_NULL and poisson(lows=None) == E_NULL and poisson(levels=None) == E_NULL
    assert poisson(ch=4) == E_UNSUPPORTED
    assert poisson(H=3, W=6) == E_ALIGN and poisson(H=5, W=5) == E_ALIGN                           # H W % 4
    assert poisson(xx=x + 4) == E_ALIGN                                                             # not 16-byte aligned
    assert poisson(sh=f32s(1.0, -1.0)) == E_SHAPE and poisson(sh=f32s(float("nan"), 1.0)) == E_SHAPE
    assert poisson(gh=i32s(0, 2)) == E_DTYPE and poisson(gh=i32s(-1, 0)) == E_DTYPE
    assert poisson(draw=-1) == E_SHAPE and poisson(draw=1 << 32) == E_SHAPE
    assert poisson(rounds=2) == E_DTYPE
    assert poisson(base=(1 << 32) - 1) == E_SHAPE
    assert poisson(out=x) == E_UNSUPPORTED
    # what the issue says must stay: the 2-D blur still refuses k = 43, DegradeConfig still refuses a sinc kernel type
    assert L.edtr_degrade_filter2d(x, y, 1, 3, 64, 64, k, 1, 43, None) == E_SHAPE
    with pytest.raises(ValueError):
        degrade.DegradeConfig(kernel_list=("sinc",), kernel_prob=(1,))
    # the Python layer refuses the same things before it touches a device
    with pytest.raises(ValueError):
        degrade.sepblur_reference(np.zeros((1, 3, 25, 70), np.float32), np.ones(51, np.float32))
    with pytest.raises(ValueError):
        degrade.sepblur_reference(np.zeros((1, 3, 80, 80), np.float32), np.ones(65, np.float32))
    with pytest.raises(ValueError):
        degrade.add_poisson_noise_reference(np.zeros((1, 3, 5, 5), np.float32), 1.0, 0)
    with pytest.raises(ValueError):
        degrade.add_poisson_noise_reference(np.zeros((1, 3, 4, 4), np.float32), -1.0, 0)


def _poisson_pmf(lam: float, n: int) -> float:
    return math.exp(n * math.log(lam) - lam - math.lgamma(n + 1)) if lam > 0 else float(n == 0)


@pytest.mark.parametrize("vals", [1, 2, 16, 256])
def test_poisson_table_is_the_cdf(vals):
    """Rows never decrease; the implied pmf (first differences, closed by 2^32) sums to 2^32; against an fp64 Poisson CDF (lgamma pmf,
    math.fsum) the error of every entry of every level is at most the 2^-32 quantum + 1e-12."""
    T, lo = degrade.poisson_table(vals)
    assert T.dtype == np.uint32 and T.shape == (256, 256) and lo.dtype == np.int32 and lo.shape == (256,)
    t = T.astype(np.int64)
    assert (np.diff(t, axis=1) >= 0).all()
    pmf = np.diff(np.concatenate([np.zeros((256, 1), np.int64), t[:, :255], np.full((256, 1), 1 << 32, np.int64)], axis=1), axis=1)
    assert (pmf >= 0).all() and (pmf.sum(axis=1) == 1 << 32).all()
    lam = ((np.arange(256, dtype=np.float32) / np.float32(255.0)) * np.float32(vals)).astype(np.float64)
    assert (lo == np.maximum(0, np.ceil(lam) - 128)).all()
    assert (T[0] == 0xFFFFFFFF).all()                                                   # lambda = 0: n = 0
    worst = 0.0
    for k in range(256):
        terms = [_poisson_pmf(lam[k], n) for n in range(int(lo[k]) + 256)]
        base = math.fsum(terms[:int(lo[k])])
        cdf = np.array([math.fsum([base] + terms[int(lo[k]):int(lo[k]) + j + 1]) for j in range(256)])
        worst = max(worst, float(np.abs(t[k] / 4294967296.0 - np.minimum(cdf, 1.0)).max()))
    print(f"\n[poisson table vals {vals}] max CDF error {worst:.3e} (bound {2.0 ** -32 + 1e-12:.3e})")
    assert worst <= 2.0 ** -32 + 1e-12


def test_poisson_table_builds_the_same_bytes_twice():
    first = [(T.tobytes(), lo.tobytes()) for T, lo in (degrade.poisson_table(v) for v in degrade.POISSON_VALS)]
    degrade._POISSON_TABLES.clear()
    again = [(T.tobytes(), lo.tobytes()) for T, lo in (degrade.poisson_table(v) for v in degrade.POISSON_VALS)]
    assert first == again
    T, lo = degrade.poisson_tables()
    assert T.shape == (9, 256, 256) and lo.shape == (9, 256) and T[8].tobytes() == first[8][0]
    with pytest.raises(ValueError):
        degrade.poisson_table(3)


def _chi2_sf(x: float, df: int) -> float:
    """P(chi-square(df) > x) = Q(df / 2, x / 2): the series of the lower incomplete gamma function below a + 1, Lentz's continued
    fraction of the upper one above (Numerical Recipes 6.2); no scipy"""
    a, x = df / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lead = math.exp(a * math.log(x) - x - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        for n in range(1, 10000):
            term *= x / (a + n)
            total += term
            if term < total * 1e-17:
                break
        return 1.0 - lead * total
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return lead * h


def _chi2_quantile(df: int, tail: float = 1e-6) -> float:
    """the 1 - tail quantile of chi-square(df), by bisection on `_chi2_sf`"""
    lo, hi = float(df), float(df) + 40.0 * math.sqrt(2.0 * df) + 100.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _chi2_sf(mid, df) > tail else (lo, mid)
    return hi


@pytest.mark.parametrize("level", [3, 128, 255])
def test_poisson_sampler_follows_the_pmf(level):
    """12288 draws of `poisson_reference` at vals = 256 and level 3 / 128 / 255 (lambda = 3.01, 128.5, 256) on the fixed seed:
    chi-square against the exact pmf, bins pooled from both ends to an expected count of at least 5."""
    N = 12288
    lam = float((np.float32(level) / np.float32(255.0)) * np.float32(256))
    n = degrade.poisson_reference(SEED, [11], rng.PURPOSE_DEGRADE_POISSON, 0, np.full((1, N), level), [256])[0]
    hi = int(lam + 12 * math.sqrt(lam) + 12)
    expect = np.array([_poisson_pmf(lam, j) for j in range(hi)]) * N
    expect = np.append(expect, N - expect.sum())                            # the upper tail as one cell
    seen = np.bincount(np.minimum(n, hi), minlength=hi + 1).astype(np.float64)
    cells_e, cells_o, acc_e, acc_o = [], [], 0.0, 0.0
    for e, o in zip(expect, seen):
        acc_e, acc_o = acc_e + e, acc_o + o
        if acc_e >= 5.0:
            cells_e.append(acc_e)
            cells_o.append(acc_o)
            acc_e = acc_o = 0.0
    cells_e[-1] += acc_e
    cells_o[-1] += acc_o
    e, o = np.array(cells_e), np.array(cells_o)
    stat, df = float(((o - e) ** 2 / e).sum()), len(e) - 1
    print(f"\n[poisson sampler lambda {lam:.2f}] mean {n.mean():.2f} var {n.var():.2f} chi2 {stat:.1f} df {df} bound {_chi2_quantile(df):.1f}")
    assert stat < _chi2_quantile(df)


def test_sinc_kernel_and_gaussian_taps(gold):
    for n, (size, cutoff) in enumerate(gold["sinc_args"]):
        assert np.abs(degrade.circular_lowpass_kernel(cutoff, int(size)) - gold[f"sinc{n}"]).max() <= 1e-12
        padded = degrade.circular_lowpass_kernel(cutoff, int(size), pad_to=21)
        assert padded.shape == (21, 21) and np.abs(padded - gold[f"sinc{n}_pad"]).max() <= 1e-12
    g = degrade.gaussian_taps(51)
    i = np.arange(51) - 25.0
    want = np.exp(-i * i / (2 * 8.0 ** 2))
    # (the same formula written another way: a few fp64 roundings of values up to g.max() = 0.05 apart, and of a sum near 1)
    eps = float(np.finfo(np.float64).eps)
    assert g.dtype == np.float64 and abs(g.sum() - 1.0) <= 8 * eps and np.abs(g - want / want.sum()).max() <= 8 * eps * g.max()
    assert abs(0.3 * ((51 - 1) * 0.5 - 1) + 0.8 - 8.0) < 1e-12
    with pytest.raises(ValueError):
        degrade.gaussian_taps(50)
    with pytest.raises(ValueError):
        degrade.gaussian_taps(7)                # cv2 answers this one from a table
    with pytest.raises(ValueError):
        degrade.circular_lowpass_kernel(1.0, 8)


def test_usm_and_poisson_restatements_meet_the_reference(gold):
    got = degrade.usm_sharpen_reference(gold["usm_x"])
    e = float(np.abs(got.astype(np.float64) - gold["usm_out"]).max())
    print(f"\n[usm] max abs err {e:.3e} (tol {float(gold['usm_tol']):.3e}, margin at the threshold {float(gold['usm_margin']):.2e})")
    assert got.dtype == np.float32 and e <= float(gold["usm_tol"])
    x, scale, gray = gold["poisson_x"], gold["poisson_scale"], gold["poisson_gray"]
    got, noise = degrade.add_poisson_noise_reference(x, scale, gray, int(gold["poisson_seed"]), gold["poisson_ids"], return_noise=True)
    e = float(np.abs(got.astype(np.float64) - gold["poisson_out"]).max())
    print(f"[poisson] max abs err {e:.3e} (tol {float(gold['poisson_tol']):.3e})")
    assert got.dtype == np.float32 and e <= float(gold["poisson_tol"])
    assert np.array_equal(degrade.level_counts(x), gold["poisson_counts"])
    assert np.array_equal(noise[1, 0], noise[1, 1]) and np.array_equal(noise[1, 0], noise[1, 2]) and not np.array_equal(noise[0, 0], noise[0, 1])


def test_vals_is_the_next_power_of_two_of_the_level_count():
    def image(levels):
        v = np.resize(np.asarray(levels, dtype=np.float32) / np.float32(255.0), 3 * 8 * 8)
        return v.reshape(1, 3, 8, 8)

    assert degrade.level_counts(image(range(0, 160, 10))).tolist()[0][0] == 16 and degrade.vals_of(16) == 16
    assert degrade.level_counts(image(range(0, 170, 10))).tolist()[0][0] == 17 and degrade.vals_of(17) == 32
    assert degrade.level_counts(image([77])).tolist() == [[1, 1]] and degrade.vals_of(1) == 1
    assert [degrade.vals_of(c) for c in (2, 3, 4, 5, 128, 129, 256)] == [2, 4, 4, 8, 128, 256, 256]
    # values between two levels and outside [0, 1] land on the clamped grid
    x = np.array([-0.3, 0.0, 0.0019, 1.0, 1.7, 0.5], dtype=np.float32)
    assert degrade._level(x).tolist() == [0, 0, 0, 255, 255, 128]
    # a constant image receives n / 1 - q with n from Poisson(q): integers minus q
    const = image([102])
    out, noise = degrade.add_poisson_noise_reference(const, 1.0, 0, SEED, [4], return_noise=True)
    n = noise + np.float32(102) / np.float32(255.0)
    assert np.abs(n - np.rint(n)).max() < 1e-6 and n.min() >= 0


def _key(p):
    opt = lambda a: None if a is None else a.tobytes()
    return (p.kernel1.tobytes(), opt(p.kernel2), opt(p.sinc_kernel), p.scale1, p.mode1, p.noise1, p.level1, p.gray1, p.quality1,
            p.stage2_scale, p.scale2, p.mode2, p.noise2, p.level2, p.gray2, p.sinc_first, p.back_mode, p.quality2)


def test_draw_params2_depends_on_seed_and_image_id_alone():
    cfg = degrade.load_config("realesrgan")
    assert isinstance(cfg, degrade.RealESRGANConfig)
    ids = [7, 0, 2 ** 32 - 1, 3, 12]
    one_by_one = {i: _key(degrade.draw_params2(cfg, 99, i)) for i in ids}
    for order in (list(reversed(ids)), ids[1::2], ids[0::2]):
        for i in order:
            assert _key(degrade.draw_params2(cfg, 99, i)) == one_by_one[i]
    assert len(set(one_by_one.values())) == len(ids)
    assert _key(degrade.draw_params2(cfg, 100, 7)) != one_by_one[7]
    with pytest.raises(ValueError):
        degrade.draw_params2(cfg, 1, 2 ** 32)
    # no decision shifts another: switching the sinc choice and the second blur off changes the kernels and nothing else
    a = degrade.draw_params2(cfg, 5, 21)
    b = degrade.draw_params2(degrade.RealESRGANConfig(sinc_prob=0.0, sinc_prob2=1.0, final_sinc_prob=0.0, second_blur_prob=1.0), 5, 21)
    assert _key(a)[3:] == _key(b)[3:] and b.sinc_kernel is None and b.kernel2 is not None and b.sinc2 and not b.sinc1
    # the existing presets and draws stay as they are
    assert isinstance(degrade.load_config("realesrgan-stage1"), degrade.DegradeConfig)
    assert isinstance(degrade.load_config("codeformer"), degrade.DegradeConfig)


def test_draw_params2_ranges_and_frequencies():
    cfg = degrade.load_config("realesrgan")
    N = 2000
    ps = [degrade.draw_params2(cfg, 17, i) for i in range(N)]
    for p in ps:
        assert p.kernel1.shape == (21, 21) and p.kernel1.dtype == np.float32 and abs(float(p.kernel1.sum()) - 1) < 1e-4
        assert p.kernel_size1 in degrade.KERNEL_RANGE and p.kernel_size2 in degrade.KERNEL_RANGE
        pad = (21 - p.kernel_size1) // 2
        assert pad == 0 or (p.kernel1[:pad] == 0).all() and (p.kernel1[:, -pad:] == 0).all()
        assert p.kernel2 is None or (p.kernel2.shape == (21, 21) and abs(float(p.kernel2.sum()) - 1) < 1e-4)
        assert p.sinc_kernel is None or (p.sinc_kernel.shape == (21, 21) and abs(float(p.sinc_kernel.sum()) - 1) < 1e-4)
        assert 0.15 <= p.scale1 <= 1.5 and 0.3 <= p.scale2 <= 1.2 and p.stage2_scale == 4.0
        assert p.mode1 in degrade.MODES and p.mode2 in degrade.MODES and p.back_mode in degrade.MODES
        assert p.noise1 in degrade.NOISE_TYPES and p.noise2 in degrade.NOISE_TYPES
        assert (1.0 <= p.level1 <= 30.0) if p.noise1 == "gaussian" else (0.05 <= p.level1 <= 3.0)
        assert (1.0 <= p.level2 <= 25.0) if p.noise2 == "gaussian" else (0.05 <= p.level2 <= 2.5)
        assert 30.0 <= p.quality1 <= 95.0 and 30.0 <= p.quality2 <= 95.0 and p.use_sharpener and p.resize_back
        s1, s2, ss, final = p.sizes(101, 203)
        assert all(v % 2 == 0 and v >= 2 for v in s1 + s2 + ss) and ss == (24, 50) and final == (101, 203)
        assert s1[0] <= int(101 * p.scale1) and s2[1] <= int(50 * p.scale2)

    def within(count, prob, what):
        sd = math.sqrt(N * prob * (1 - prob))
        print(f"[draw_params2] {what}: {count} of {N}, expected {N * prob:.0f} +- {4 * sd:.0f}")
        return abs(count - N * prob) <= 4 * sd

    assert within(sum(p.sinc1 for p in ps), 0.1, "sinc, stage 1")
    assert within(sum(p.sinc2 for p in ps), 0.1, "sinc, stage 2")
    assert within(sum(p.sinc_kernel is not None for p in ps), 0.8, "final sinc")
    assert within(sum(p.sinc_first for p in ps), 0.5, "sinc-first order")
    assert within(sum(p.noise1 == "gaussian" for p in ps), 0.5, "gaussian, stage 1")
    assert within(sum(p.noise2 == "gaussian" for p in ps), 0.5, "gaussian, stage 2")
    assert within(sum(p.kernel2 is not None for p in ps), 0.8, "second blur")
    assert within(sum(p.gray1 for p in ps), 0.4, "grey, stage 1")
    assert within(sum(p.scale1 > 1 for p in ps), 0.2, "up, stage 1") and within(sum(p.scale1 == 1 for p in ps), 0.1, "keep, stage 1")
    ranged = [degrade.draw_params2(degrade.RealESRGANConfig(stage2_scale=[2, 4]), 17, i).stage2_scale for i in range(50)]
    assert all(2.0 <= s <= 4.0 for s in ranged) and len(set(ranged)) == 50


REFERENCE_LAYOUT = """
dataset:
  val:
    target: datasets.detection_cocov2.DegradedDetectionDatasetCocov2
    params:
      root: somewhere
      gt_size: 512
      blur_kernel_size: 21
      kernel_list: ['iso', 'aniso']
      kernel_prob: [0.6, 0.4]
      sinc_prob: 0.25
      blur_sigma: [0.2, 3]
      blur_sigma2: [0.2, 1.25]
      final_sinc_prob: 0.5
  batch_transform:
    target: datasets.detection_cocov2.RealESRGANBatchTransform
    params:
      hq_key: hq
      use_sharpener: false
      queue_size: QUEUE
      resize_prob: [0.2, 0.7, 0.1]
      resize_range: RANGE
      jpeg_range: [40, 90]
      stage2_scale: 2
      resize_back: false
"""


def test_yaml_inputs(tmp_path):
    def write(name, queue="0", rng_="[0.5, 1.5]"):
        path = tmp_path / name
        path.write_text(REFERENCE_LAYOUT.replace("QUEUE", queue).replace("RANGE", rng_))
        return str(path)

    cfg = degrade.load_config(write("ok.yaml"))
    assert isinstance(cfg, degrade.RealESRGANConfig)
    assert list(cfg.kernel_list) == ["iso", "aniso"] and cfg.sinc_prob == 0.25 and list(cfg.blur_sigma2) == [0.2, 1.25]
    assert cfg.final_sinc_prob == 0.5 and cfg.use_sharpener is False and list(cfg.resize_range) == [0.5, 1.5]
    assert list(cfg.jpeg_range) == [40, 90] and cfg.stage2_scale == 2 and cfg.resize_back is False
    assert list(cfg.jpeg_range2) == [30.0, 95.0] and cfg.second_blur_prob == 0.8          # not in the file: the defaults
    p = degrade.draw_params2(cfg, 1, 2)
    assert not p.use_sharpener and p.stage2_scale == 2.0 and p.sizes(64, 96)[3] == (32, 48)
    with pytest.raises(ValueError, match="queue_size"):
        degrade.load_config(write("queue.yaml", queue="180"))
    with pytest.raises(ValueError, match="resize_range"):
        degrade.load_config(write("range.yaml", rng_="[1.5, 0.5]"))
    with pytest.raises(ValueError, match="resize_range"):
        degrade.load_config(write("range2.yaml", rng_="[0.5]"))
    for bad in (dict(jpeg_range2=(0, 50)), dict(noise_range=(5, 1)), dict(stage2_scale=0), dict(stage2_scale=(4, 2)), dict(resize_prob=(1, 1)),
                dict(kernel_list=("sinc",), kernel_prob=(1,)), dict(sinc_prob=1.5), dict(queue_size=8)):
        with pytest.raises(ValueError):
            degrade.RealESRGANConfig(**bad)
    # a YAML without batch_transform is still a first-order configuration
    flat = tmp_path / "flat.yaml"
    flat.write_text("dataset:\n  params:\n    blur_kernel_size: 21\n    jpeg_range: [60, 90]\n")
    assert isinstance(degrade.load_config(str(flat)), degrade.DegradeConfig)


def test_degrade2_reference_runs_the_whole_chain():
    """2 images of 3 x 64 x 96 through the numpy chain: the result has the input extent and lies on the 1/255 grid; an image alone gives
    the same values; an extent too small for the 21 x 21 reflect border is refused, not skipped."""
    cfg = degrade.RealESRGANConfig(resize_range=(0.5, 1.5), stage2_scale=2)
    hq = np.random.default_rng(3).random((2, 3, 64, 96), dtype=np.float32)
    params = [degrade.draw_params2(cfg, 7, i) for i in (3, 4)]
    lqs, gts = degrade.degrade2_reference(hq, params, 7, [3, 4], return_gt=True)
    for b in range(2):
        assert lqs[b].shape == (3, 64, 96) and lqs[b].dtype == np.float32 and gts[b].shape == (3, 64, 96)
        grid = lqs[b].astype(np.float64) * 255.0
        assert np.abs(grid - np.rint(grid)).max() < 1e-4 and lqs[b].min() >= 0.0 and lqs[b].max() <= 1.0
        assert np.array_equal(lqs[b], (np.rint(grid) / 255.0).astype(np.float32))
        assert not np.array_equal(gts[b], hq[b]) and np.array_equal(gts[b], degrade.usm_sharpen_reference(hq[b:b + 1])[0])
    alone = degrade.degrade2_reference(hq[1:], params[1:], 7, [4])
    assert np.array_equal(alone[0], lqs[1])
    small = degrade.draw_params2(degrade.RealESRGANConfig(resize_prob=(0, 1, 0), resize_range=(0.15, 1.0), use_sharpener=False), 7, 0)
    small.scale1, small.kernel2 = 0.15, small.kernel1                   # 64 x 0.15 = 9 rows: fewer than the border of 10 needs
    with pytest.raises(ValueError, match="second blur"):
        degrade.degrade2_reference(hq[:1], [small], 7, [0])
