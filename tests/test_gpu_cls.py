"""The classification launches on the device (csrc/cls.hip) against their numpy restatements (edtr_amd/cls.py), by equality: the rank
behind topk on rows full of ties, NaN and signed zeros; the running record and its overflow; the feature distance bit for bit at
every element count where the order changes shape; the normalisation; the crop / flip / transpose window around the LDS tile's
edges; and `evaluate` with stub callables against the restatement loop."""
import numpy as np
import pytest
import torch

from edtr_amd import cls

pytestmark = pytest.mark.gpu
F32 = np.float32
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def tied_logits(rng, B, C, dtype):
    """[B, C] drawn from four values (ties everywhere); where there is room, a row with NaN and one with both zeros"""
    x = rng.choice(np.array([-1.5, 0.0, 0.25, 3.0], dtype=F32), size=(B, C))
    if C >= 2:
        x[0, rng.integers(0, C, max(1, C // 8))] = np.nan
        x[B - 1, ::2] = -0.0
    return torch.from_numpy(x).to(dtype)


def assert_records_equal(got, want):
    assert set(got) == set(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert got[name].tobytes() == want[name].tobytes(), name


# ---- rank ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 200, 1000])
def test_rank_equals_the_restatement(C, dtype):
    rng = np.random.default_rng(1000 + C)
    for B in (1, 3, 67):
        logits = tied_logits(rng, B, C, DTYPES[dtype])
        labels = rng.integers(0, C, B)
        labels[rng.random(B) < 0.2] = rng.choice([-1, C, C + 5, -7])            # labels outside the range
        for keep in (1, 5, 8):                                                   # (keep > C for the small C)
            want_rank, want_top = cls.rank_reference(logits, labels, keep)
            rank, top = cls.rank(logits.cuda(), torch.from_numpy(labels).cuda(), keep)
            assert rank.dtype == torch.int32 and top.dtype == torch.int32
            assert np.array_equal(rank.cpu().numpy(), want_rank), (B, keep)
            assert np.array_equal(top.cpu().numpy(), want_top), (B, keep)
            if keep > C:
                assert np.all(want_top[:, C:] == -1)
        assert np.all(want_rank[(labels < 0) | (labels >= C)] == C)


def test_rank_of_two_dimensional_targets_and_host_inputs():
    rng = np.random.default_rng(7)
    logits, target = tied_logits(rng, 5, 33, torch.float32), tied_logits(rng, 5, 33, torch.float32)
    want = cls.target_labels_reference(target)
    assert np.array_equal(want, target.max(dim=1)[1].numpy())                    # torch's CPU max: the first NaN, else the first maximum
    assert np.array_equal(cls.target_labels(target.cuda()).cpu().numpy(), want)
    rank, top = cls.rank(logits.numpy(), target.numpy(), 5)                      # numpy inputs are uploaded first
    want_rank, want_top = cls.rank_reference(logits, want, 5)
    assert np.array_equal(rank.cpu().numpy(), want_rank) and np.array_equal(top.cpu().numpy(), want_top)


# ---- the running record -----------------------------------------------------------------------------------------------------------------------
def test_updates_append_at_the_advanced_offsets_with_the_right_batch_rows():
    rng = np.random.default_rng(11)
    batches = []
    for B, C, dtype, with_fd in ((3, 40, torch.float32, True), (67, 40, torch.float16, False), (1, 40, torch.bfloat16, True)):
        logits = tied_logits(rng, B, C, dtype)
        labels = torch.from_numpy(rng.integers(-1, C + 1, B))
        feats = (torch.from_numpy(rng.standard_normal((B, 5, 3, 3)).astype(F32)), torch.from_numpy(rng.standard_normal((B, 5, 3, 3)).astype(F32))) if with_fd else (None, None)
        batches.append((logits, labels) + feats)
    scores = cls.Scores(80, topk=(1, 5, 8), keep=8, device="cuda", batch_capacity=3)
    for logits, labels, a, b in batches:
        scores.update(logits.cuda(), labels.cuda(), None if a is None else a.cuda(), None if b is None else b.cuda())
    got, want = scores.to_host(), cls.records_reference(batches, topk=(1, 5, 8), keep=8)
    assert_records_equal(got, want)
    assert got["batch"].tolist() == [0] * 3 + [1] * 67 + [2] and got["n"].tolist() == [3, 67, 1] and scores.offsets.tolist() == [71, 3]
    assert np.isnan(got["fd"][3:70]).all() and not np.isnan(got["fd"][:3]).any()
    out = cls.summarize(got)
    assert out["images"] == 71 and np.isnan(out["fd"]) and out["batch_acc"].tobytes() == cls.summarize(want)["batch_acc"].tobytes()
    # 2-D targets take the first place of their rows as the label
    target = tied_logits(rng, 3, 40, torch.float32)
    other = cls.Scores(3, device="cuda")
    other.update(batches[0][0].cuda(), target.cuda())
    assert_records_equal(other.to_host(), cls.records_reference([(batches[0][0], target)]))


def test_overflow_raises_after_the_copy_and_leaves_the_guard_rows():
    rng = np.random.default_rng(12)
    logits, labels = tied_logits(rng, 3, 9, torch.float32), torch.tensor([0, 4, 8])
    feat = torch.from_numpy(rng.standard_normal((3, 7)).astype(F32))
    scores = cls.Scores(2, topk=(1, 5), keep=5, device="cuda")
    scores.update(logits.cuda(), labels.cuda(), feat.cuda(), (feat + 1).cuda())
    with pytest.raises(RuntimeError, match=r"3 images in 1 batches .* 2 image rows"):
        scores.to_host()
    raw = scores.buffer.cpu().numpy()
    want = cls.records_reference([(logits, labels, feat, feat + 1)])
    for name, (at, rows, width, dt) in scores._layout.items():
        col = raw[at:at + rows * width * 4]
        assert np.all(col[(rows - 1) * width * 4:] == cls.Scores.GUARD), name                      # no launch wrote a guard row
        if name in dict(cls.IMAGE_FIELDS):
            assert col[:2 * width * 4].tobytes() == want[name][:2].tobytes(), name                  # the rows that fit are there
    # the batch capacity alone overflowing is reported too
    small = cls.Scores(8, device="cuda", batch_capacity=1)
    small.update(logits.cuda(), labels.cuda())
    small.update(logits.cuda(), labels.cuda())
    with pytest.raises(RuntimeError, match="6 images in 2 batches"):
        small.to_host()


# ---- feature distance ---------------------------------------------------------------------------------------------------------------------
FD_SIZES = [255, 256, 257, cls.FD_CHUNK - 1, cls.FD_CHUNK, cls.FD_CHUNK + 1, 2 * cls.FD_CHUNK + 3]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("n", FD_SIZES)
def test_fdist_is_bit_equal_to_the_restatement(n, dtype):
    rng = np.random.default_rng(2000 + n)
    for B in (1, 3):
        a = torch.from_numpy((rng.standard_normal((B, n)) * 3).astype(F32)).to(DTYPES[dtype])
        b = torch.from_numpy((rng.standard_normal((B, n)) * 3).astype(F32)).to(DTYPES[dtype])
        got = cls.fdist(a.cuda(), b.cuda())
        assert got.dtype == torch.float32 and got.cpu().numpy().tobytes() == cls.fdist_reference(a, b).tobytes(), B


def test_fdist_of_a_feature_map_and_of_nan():
    rng = np.random.default_rng(13)
    a, b = rng.standard_normal((2, 64, 7, 7)).astype(F32), rng.standard_normal((2, 64, 7, 7)).astype(F32)
    a[1, 3, 2, 1] = np.nan
    got = cls.fdist(a, b).cpu().numpy()                                          # numpy inputs are uploaded first
    want = cls.fdist_reference(a, b)
    assert got[:1].tobytes() == want[:1].tobytes() and np.isnan(got[1]) and np.isnan(want[1])
    assert abs(float(got[0]) - float(torch.nn.functional.l1_loss(torch.from_numpy(a[:1]), torch.from_numpy(b[:1]), reduction="none").mean())) < 1e-6


# ---- normalisation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 64, 64)])
def test_normalize_equals_the_restatement_also_in_place(shape):
    rng = np.random.default_rng(14)
    x = rng.random(shape).astype(F32)
    want = cls.normalize_reference(x)
    dev = torch.from_numpy(x).cuda()
    out = cls.normalize(dev)
    assert out.cpu().numpy().tobytes() == want.tobytes() and dev.cpu().numpy().tobytes() == x.tobytes()
    back = cls.normalize(out, cls.IMAGENET_INV_MEAN, cls.IMAGENET_INV_STD)
    assert back.cpu().numpy().tobytes() == cls.normalize_reference(want, cls.IMAGENET_INV_MEAN, cls.IMAGENET_INV_STD).tobytes()
    assert cls.normalize(dev, out=dev) is dev and dev.cpu().numpy().tobytes() == want.tobytes()
    odd = dev.reshape(-1)[1:1 + 3 * 4 * 5].reshape(1, 3, 4, 5).contiguous()     # (a base that is not 16-byte aligned takes the scalar path)
    view = dev.reshape(-1)[1:1 + 60].view(1, 3, 4, 5)
    assert cls.normalize(view).cpu().numpy().tobytes() == cls.normalize_reference(odd.cpu().numpy()).tobytes()


def test_prepare_is_the_composition():
    rng = np.random.default_rng(15)
    x = rng.random((2, 3, 9, 11)).astype(F32)
    dev = torch.from_numpy(x).cuda()
    for kw in (dict(), dict(size=(6, 8)), dict(upsample=2), dict(size=(6, 8), upsample=2, normalize=False), dict(normalize=False)):
        got = cls.prepare(dev, **kw).cpu().numpy()
        assert got.tobytes() == cls.prepare_reference(x, **kw).tobytes(), kw
    assert dev.cpu().numpy().tobytes() == x.tobytes() and cls.prepare(dev, normalize=False) is dev


# ---- the window ---------------------------------------------------------------------------------------------------------------------------
def position_image(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x % 16) + 16 * (y % 16), x // 16 + 16 * (y // 16), (x + 3 * y) % 251], axis=-1).astype(np.uint8)


@pytest.mark.parametrize("crop", [(5, 7), (31, 33), (64, 32)])
def test_window_equals_the_restatement_in_all_eight_states(crop):
    src = position_image(70, 45)
    dev = torch.from_numpy(src).cuda()
    for state in range(8):
        h, v, r = bool(state & 1), bool(state & 2), bool(state & 4)
        for origin, fill in (((3, 2), 0), ((-2, 20), 9), ((40, -5), 255)):       # inside; off the top and the right; off the bottom and the left
            want = cls.window_reference(src, crop, origin, h, v, r, fill)
            got = cls.window(dev, crop, origin, h, v, r, fill)
            assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (state, origin)
            want1 = cls.window_reference(src[:, :, 0], crop, origin, h, v, r, fill)
            got1 = cls.window(dev[:, :, 0], crop, origin, h, v, r, fill)
            assert got1.shape == want1.shape and np.array_equal(got1.cpu().numpy(), want1), (state, origin)


def test_prepare_image_equals_its_restatement():
    img = position_image(30, 40)
    for image_id in range(4):
        geom = cls.draw_cls_geometry(cls.ClsGeometry(24, 20, "random", True, True), 11, image_id, img.shape[:2])
        assert np.array_equal(cls.prepare_image(img, geom).cpu().numpy(), cls.prepare_image_reference(img, geom))


# ---- evaluate -----------------------------------------------------------------------------------------------------------------------------
def test_evaluate_with_stub_callables_equals_the_restatement_loop():
    rng = np.random.default_rng(16)
    N, C = 11, 20
    images = torch.from_numpy(rng.random((N, 3, 8, 8)).astype(F32)).cuda()
    gts = torch.from_numpy(rng.random((N, 3, 8, 8)).astype(F32)).cuda()
    labels = rng.integers(0, C, N)
    w = torch.from_numpy(rng.integers(-2, 3, (C, 3)).astype(F32)).cuda()

    def clsnet(x):                      # logits from small integers times 8-bit levels: ties happen
        return (torch.round(x[:, :, ::4, ::4] * 4).sum(dim=(2, 3)) @ w.t()).contiguous()

    def teacher(x):
        return x[:, :, ::2, ::2] * 2 - 1

    out = cls.evaluate(images, labels, clsnet, teacher=teacher, gts=gts, batch_size=4, topk=(1, 5))
    batches = [(clsnet(images[lo:lo + 4]).cpu(), labels[lo:lo + 4], teacher(images[lo:lo + 4]).cpu(), teacher(gts[lo:lo + 4]).cpu()) for lo in range(0, N, 4)]
    want = cls.records_reference(batches, topk=(1, 5), keep=5)
    assert_records_equal(out["records"], want)
    ref = cls.summarize(want)
    for key in ("acc1", "acc5", "acc1_exact", "acc5_exact", "fd", "images"):
        assert out[key] == ref[key], key
    assert out["records"]["n"].tolist() == [4, 4, 3] and np.array_equal(out["pred"], want["top"][:, 0]) and np.array_equal(out["rank"], want["rank"])
    assert out["fd"] == float(F32(np.mean(want["fd"].astype(np.float64)))) and out["fd"] > 0 and out["fd_image"].tobytes() == want["fd"].tobytes()
    plain = cls.evaluate([im for im in images], torch.from_numpy(labels).cuda(), clsnet, batch_size=8)
    assert plain["acc1_exact"] == out["acc1_exact"] and np.isnan(plain["fd"]) and plain["records"]["n"].tolist() == [8, 3]
