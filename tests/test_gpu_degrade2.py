"""The kernels of the second-order degradation chain on the device against their numpy restatements (edtr_amd/degrade.py), by EQUALITY:
csrc/degrade2.hip is a bit-exact function of its inputs — the Poisson sampler included, whose stream is used as integers.  Shapes are
the smallest at which each can still go wrong: reflect borders on all four sides, a halo of 25 (and of 31) against the 32-wide tile and
partial tiles for the separable blur; 256, 5 and 1 levels, a grey image and the largest image id for the Poisson noise."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from edtr_amd import degrade, rng

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "degrade2.npz"))


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


@pytest.mark.parametrize("k,shape", [(3, (2, 3, 40, 70)), (51, (2, 3, 40, 70)), (63, (1, 3, 32, 33))])
def test_sepblur_equals_the_restatement(k, shape):
    x = rand(*shape, seed=k)
    taps = degrade.gaussian_taps(k, sigma=0.0 if k > 7 else 0.8).astype(np.float32)
    want, want_mask = degrade.sepblur_reference(x, taps, threshold=10)
    got, mask = degrade.sepblur(dev(x), taps, threshold=10)
    assert same(got, want, f"sepblur k {k}") and same(mask, want_mask, f"mask k {k}")
    assert 0 < float(want_mask.mean()) < 1                              # both sides of the threshold occur
    assert same(degrade.sepblur(dev(x), taps), want)                    # without the mask: the same bits
    uneven = rand(k, seed=100 + k)                                      # taps that are not symmetric: rows and columns are not confused
    assert same(degrade.sepblur(dev(x), uneven), degrade.sepblur_reference(x, uneven), f"uneven taps k {k}")
    with pytest.raises(RuntimeError):
        degrade.sepblur(dev(x[:, :, :k // 2]), taps)


def test_usm_sharpen_equals_the_restatement_and_meets_the_reference(gold):
    x = gold["usm_x"]                                                   # 2 x 3 x 40 x 70
    got = degrade.usm_sharpen(dev(x))
    assert same(got, degrade.usm_sharpen_reference(x), "usm")
    e = float(np.abs(got.cpu().numpy().astype(np.float64) - gold["usm_out"]).max())
    print(f"\n[usm] max abs err against the reference {e:.3e} (tol {float(gold['usm_tol']):.3e})")
    assert e <= float(gold["usm_tol"])
    other = degrade.usm_sharpen(dev(x), weight=1.5, threshold=3, radius=20)
    assert same(other, degrade.usm_sharpen_reference(x, weight=1.5, threshold=3, radius=20), "usm, other arguments")


def test_poisson_noise_equals_the_restatement(gold):
    """3 x 3 x 16 x 24, ids [5, 0, 2^32 - 1]: a ramp over 256 levels, a grey image of 5 levels, a constant image."""
    x, scale, gray = gold["poisson_x"], gold["poisson_scale"], gold["poisson_gray"]
    seed, ids = int(gold["poisson_seed"]), gold["poisson_ids"].tolist()
    assert ids == [5, 0, 2 ** 32 - 1] and gray.tolist() == [0, 1, 0] and x.shape == (3, 3, 16, 24)
    src = rng.NoiseSource(seed, ids)
    out, noise, counts = degrade.add_poisson_noise(dev(x), scale, gray, src, return_noise=True, return_counts=True)
    want_counts = degrade.level_counts(x)
    assert want_counts[:, 0].tolist() == [256, 5, 1]
    assert same(counts, want_counts, "level counts")
    want, want_noise = degrade.add_poisson_noise_reference(x, scale, gray, seed, ids, return_noise=True)
    assert same(noise, want_noise, "poisson noise") and same(out, want, "poisson out")
    assert torch.equal(noise[1, 0], noise[1, 1]) and torch.equal(noise[1, 0], noise[1, 2]) and not torch.equal(noise[0, 0], noise[0, 1])
    assert torch.equal(out, degrade.add_poisson_noise(dev(x), scale, gray, src))                  # without the optional outputs
    e = float(np.abs(out.cpu().numpy().astype(np.float64) - gold["poisson_out"]).max())
    print(f"\n[poisson] max abs err against the reference {e:.3e} (tol {float(gold['poisson_tol']):.3e})")
    assert e <= float(gold["poisson_tol"])
    # every image alone, and the batch in another order: the same bits
    for b in range(3):
        one = degrade.add_poisson_noise(dev(x[b:b + 1]), scale[b:b + 1], gray[b:b + 1], rng.NoiseSource(seed, [ids[b]]))
        assert torch.equal(one[0], out[b])
    perm = [2, 0, 1]
    moved = degrade.add_poisson_noise(dev(x[perm]), scale[perm], gray[perm], rng.NoiseSource(seed, [ids[p] for p in perm]))
    assert torch.equal(moved, out[perm])
    another = degrade.add_poisson_noise(dev(x), scale, gray, src, draw=1)
    assert not torch.equal(another, out)
    assert same(another, degrade.add_poisson_noise_reference(x, scale, gray, seed, ids, draw=1), "draw 1")
    rounded = degrade.add_poisson_noise(dev(x), scale, gray, src, rounds=True)
    assert same(rounded, degrade.add_poisson_noise_reference(x, scale, gray, seed, ids, rounds=True), "rounds")
    # all three grey, and values outside [0, 1] / between two levels
    wild = (rand(2, 3, 16, 24, seed=5) * 1.4 - 0.2).astype(np.float32)
    for g in ([1, 1], [0, 1]):
        got = degrade.add_poisson_noise(dev(wild), [0.7, 2.0], g, rng.NoiseSource(9, [1, 2]))
        assert same(got, degrade.add_poisson_noise_reference(wild, [0.7, 2.0], g, 9, [1, 2]), f"wild, grey {g}")


def _forced(order_first: bool):
    """two images' parameters with both stages forced to Poisson noise and the order of the end fixed"""
    cfg = degrade.RealESRGANConfig(resize_range=(0.5, 1.5), stage2_scale=2, gaussian_noise_prob=0.0, gaussian_noise_prob2=0.0,
                                   final_sinc_prob=1.0, second_blur_prob=1.0)
    params = [degrade.draw_params2(cfg, 31, i) for i in (8, 2)]
    for p in params:
        assert p.noise1 == p.noise2 == "poisson" and p.sinc_kernel is not None and p.kernel2 is not None
        p.sinc_first = order_first
    return params


@pytest.mark.parametrize("order_first", [True, False], ids=["sinc-first", "jpeg-first"])
def test_whole_chain_equals_the_numpy_chain(order_first):
    """`degrade_batch2` on 2 images of 3 x 64 x 96 with Poisson noise in both stages = `degrade2_reference`, bit for bit (the stream is
    used as integers: nothing depends on a device transcendental)."""
    hq = rand(2, 3, 64, 96, seed=12)
    params = _forced(order_first)
    ids = [8, 2]
    lqs, gts = degrade.degrade_batch2(dev(hq), params, 31, ids, return_gt=True)
    want, want_gt = degrade.degrade2_reference(hq, params, 31, ids, return_gt=True)
    for b in range(2):
        assert tuple(lqs[b].shape) == (3, 64, 96)
        assert same(gts[b], want_gt[b], f"gt {b}") and same(lqs[b], want[b], f"lq {b}")
        alone = degrade.degrade_batch2(dev(hq[b:b + 1]), [params[b]], 31, [ids[b]])[0]
        assert torch.equal(alone, lqs[b])
    # the two images through the SAME launches (one group): image 1 takes image 0's extents and modes, everything else stays its own
    q = copy.copy(params[1])
    for field in ("scale1", "mode1", "scale2", "mode2", "back_mode", "stage2_scale"):
        setattr(q, field, getattr(params[0], field))
    assert degrade._group_key2((64, 96), q) == degrade._group_key2((64, 96), params[0])
    together = degrade.degrade_batch2(dev(hq), [params[0], q], 31, ids)
    assert torch.equal(together[0], lqs[0])
    assert same(together[1], degrade.degrade2_reference(hq[1:], [q], 31, ids[1:])[0], "image 1 beside image 0")


def test_degrade_files_writes_the_same_bytes_for_batch_size_1_and_4(tmp_path):
    from PIL import Image
    src = tmp_path / "in"
    src.mkdir()
    gen = np.random.default_rng(5)
    for name, (h, w) in (("a", (64, 96)), ("b", (80, 64)), ("c", (64, 96)), ("d", (72, 72)), ("e", (64, 96))):
        Image.fromarray(gen.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / f"{name}.png")
    cfg = degrade.RealESRGANConfig(resize_range=(0.5, 1.5), stage2_scale=2)
    paths = sorted(str(p) for p in src.iterdir())
    one = degrade.degrade_files(paths, str(tmp_path / "one"), cfg, 3, batch_size=1)
    four = degrade.degrade_files(paths, str(tmp_path / "four"), cfg, 3, batch_size=4, workers=2)
    assert len(one) == len(four) == 5
    for (g1, l1), (g2, l2), p in zip(one, four, paths):
        for f1, f2 in ((g1, g2), (l1, l2)):
            with open(f1, "rb") as a, open(f2, "rb") as b:
                assert a.read() == b.read()
        assert Image.open(l1).size == Image.open(p).size and Image.open(g1).size == Image.open(p).size
        assert not np.array_equal(np.array(Image.open(g1)), np.array(Image.open(p)))       # gt/ is the sharpened image
        assert not np.array_equal(np.array(Image.open(l1)), np.array(Image.open(g1)))


def test_bad_arguments_answer_the_documented_codes_and_launch_nothing():
    """every rejection of the three entry points of csrc/degrade2.hip, code by code: one thing changed at a time on a valid call"""
    from edtr_amd import lib, ops
    L, s = lib.load(), ops.stream_ptr()
    x = torch.zeros((2, 3, 4, 4), dtype=torch.float32, device=DEV)
    out, aux = torch.full_like(x, 7.0), torch.full_like(x, 7.0)            # aux: mask_out / noise_out
    taps = torch.full((3,), 1.0 / 3.0, dtype=torch.float32, device=DEV)
    sc = torch.ones(2, dtype=torch.float32, device=DEV)
    gry = torch.zeros(2, dtype=torch.int32, device=DEV)
    ids = torch.zeros(2, dtype=torch.int64, device=DEV)
    tables = torch.zeros((9, 256, 256), dtype=torch.int32, device=DEV)     # (the sizes a launch would read)
    lows = torch.zeros((9, 256), dtype=torch.int32, device=DEV)
    levels = torch.full((2, 16), 7, dtype=torch.int32, device=DEV)
    P = lambda t: t.data_ptr()
    f32s, i32s = lambda *v: (C.c_float * len(v))(*v), lambda *v: (C.c_int32 * len(v))(*v)
    E_NULL, E_SHAPE, E_ALIGN, E_DTYPE, E_UNSUPPORTED = -1, -2, -3, -4, -5
    shape = dict(B=2, channels=3, H=4, W=4)
    valid = {      # the arguments in the order of the entry point
        "sepblur": (L.edtr_degrade_sepblur, dict(x=P(x), out=P(out), mask_out=P(aux), **shape, taps=P(taps), k=3, threshold=10.0)),
        "usm_apply": (L.edtr_degrade_usm_apply, dict(x=P(x), blur=P(x), soft=P(x), out=P(out), **shape, weight=0.5)),
        "poisson_noise": (L.edtr_degrade_poisson_noise, dict(x=P(x), out=P(out), noise_out=P(aux), **shape, scale_host=f32s(1.0, 1.0), scale=P(sc),
                                                             gray_host=i32s(0, 0), gray=P(gry), tables=P(tables), lows=P(lows), levels=P(levels),
                                                             counts_out=None, seed=1, image_ids=None, image_id_base=0, draw=0, rounds=0)),
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
    for change, want in ((dict(scale_host=None), E_NULL), (dict(rounds=2), E_DTYPE), (dict(rounds=2, draw=-1), E_DTYPE),    # rounds before draw
                         (dict(draw=-1), E_SHAPE), (dict(draw=1 << 32), E_SHAPE), (dict(H=3, W=3), E_ALIGN),              # H W % 4
                         (dict(scale_host=f32s(-1.0, 1.0)), E_SHAPE), (dict(scale_host=f32s(1.0, float("nan"))), E_SHAPE),
                         (dict(gray_host=i32s(2, 0)), E_DTYPE), (dict(image_ids=P(ids) + 4), E_ALIGN),
                         (dict(image_ids=None, image_id_base=(1 << 32) - 1), E_SHAPE),                                   # image_id_base + B > 2^32
                         (dict(x=P(x) + 4), E_ALIGN),                                                                     # the 16-byte rule
                         (dict(tables=None), E_NULL), (dict(out=P(x)), E_UNSUPPORTED), (dict(levels=P(x)), E_UNSUPPORTED)):
        assert code("poisson_noise", **change) == want, change
    for change, want in ((dict(k=65), E_SHAPE), (dict(mask_out=P(out)), E_UNSUPPORTED)):
        assert code("sepblur", **change) == want, change
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((aux == 7.0).all()) and bool((x == 0.0).all()) and bool((levels == 7).all())   # nothing was launched
