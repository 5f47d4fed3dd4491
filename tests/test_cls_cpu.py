"""The classification rules on the host (edtr_amd/cls.py): the numpy restatements against the reference's own `calculate_accuracy`,
crops and `augment`, and against plain torch (tests/golden/cls.npz, tools/make_cls_goldens.py); hand-built rows for what torch leaves
unspecified — equal keys, NaN, signed zeros; the data set's geometry and listing; and the C ABI's checks of the five entry points,
which refuse bad arguments before any launch.  No GPU is needed."""
import math
import os
import re

import numpy as np
import pytest
import torch

from edtr_amd import cls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "cls.npz")) as z:
        return {k: z[k] for k in z.files}


def ulp(v) -> float:
    return float(np.spacing(F32(abs(v))))


# ---- the order rule ---------------------------------------------------------------------------------------------------------------------
def test_rank_equals_topk_and_calculate_accuracy_on_the_tie_free_rows(golden):
    for i, B in enumerate(golden["acc_batches"].tolist()):
        logits, lab = golden[f"acc{i}_logits"], golden[f"acc{i}_labels"]
        assert all(np.unique(row).size == row.size for row in logits)
        rank, top = cls.rank_reference(logits, lab, keep=5)
        assert rank.dtype == np.int32 and top.dtype == np.int32 and top.shape == (B, 5)
        assert np.array_equal(top, golden[f"acc{i}_topk"])
        assert np.array_equal(top, torch.from_numpy(logits).topk(5, 1, True, True)[1].numpy())
        correct = np.array([int((rank < k).sum()) for k in (1, 5)])
        got = cls.batch_accuracy(correct, np.array(B))
        assert got.dtype == F32 and got.tobytes() == golden[f"acc{i}_out"].tobytes()
        assert 0 < correct[0] <= correct[1] or B == 1
    recs = cls.records_reference([(golden[f"acc{i}_logits"], golden[f"acc{i}_labels"]) for i in range(len(golden["acc_batches"]))])
    want = np.stack([golden[f"acc{i}_out"] for i in range(len(golden["acc_batches"]))])
    assert cls.summarize(recs)["batch_acc"].tobytes() == want.tobytes()


def test_two_dimensional_targets_are_the_first_place(golden):
    logits, target = golden["acc2d_logits"], golden["acc2d_target"]
    lab = cls.target_labels_reference(target)
    assert np.array_equal(lab, golden["acc2d_labels"]) and np.array_equal(lab, torch.from_numpy(target).max(dim=1)[1].numpy())
    rank, _ = cls.rank_reference(logits, lab, keep=5)
    got = cls.batch_accuracy(np.array([int((rank < k).sum()) for k in (1, 5)]), np.array(6))
    assert got.tobytes() == golden["acc2d_out"].tobytes()
    recs = cls.records_reference([(logits, target)])
    assert np.array_equal(recs["label"], lab) and np.array_equal(recs["rank"], rank)
    # the first NaN, else the first maximum; -0.0 and 0.0 tie
    hard = np.array([[1, NAN, 3, NAN], [2, 5, 5, 1], [-0.0, 0.0, -1, -2], [0.0, -0.0, -1, -2], [-INF, -INF, -INF, -INF]], dtype=F32)
    assert cls.target_labels_reference(hard).tolist() == [1, 1, 0, 0, 0] == torch.from_numpy(hard).max(dim=1)[1].tolist()


def test_hand_built_rows_follow_the_written_rule():
    def one(row, label, keep=5):
        rank, top = cls.rank_reference(np.array([row], dtype=F32), np.array([label]), keep)
        return int(rank[0]), top[0].tolist()
    # all equal: index order, and a label tied at the k-th place is correct at k iff its index is below k
    assert one([2.0] * 7, 4) == (4, [0, 1, 2, 3, 4]) and one([2.0] * 7, 5) == (5, [0, 1, 2, 3, 4])
    # several NaN: all of them first, in index order, whatever their sign or payload
    row = np.array([1.0, NAN, 3.0, -NAN, 2.0], dtype=F32)
    row[3:4].view(np.uint32)[0] = 0xFFC00123
    assert one(row, 2) == (2, [1, 3, 2, 4, 0]) and one(row, 3) == (1, [1, 3, 2, 4, 0])
    # -0.0 against 0.0: one key
    assert one([-0.0, 0.0, -1.0], 1) == (1, [0, 1, 2, -1, -1]) and one([0.0, -0.0, 1.0], 1) == (2, [2, 0, 1, -1, -1])
    # infinities
    assert one([-INF, INF, 0.0, INF, -INF], 4) == (4, [1, 3, 2, 0, 4]) and one([-INF, INF, 0.0, INF, -INF], 3) == (1, [1, 3, 2, 0, 4])
    # labels outside [0, C): rank C, never correct
    assert one([1.0, 2.0, 3.0], -1)[0] == 3 and one([1.0, 2.0, 3.0], 3)[0] == 3 and one([1.0, 2.0, 3.0], 2 ** 31 - 1)[0] == 3
    # C = 1, keep > C, keep = 1, keep = 8
    assert one([NAN], 0, 8) == (0, [0] + [-1] * 7) and one([5.0], 0, 1) == (0, [0])
    # halves are widened exactly: fp16 values that differ stay different, bf16 comes through torch
    h = np.array([[1.0, 1.0009765625, 0.99951171875]], dtype=np.float16)
    assert cls.rank_reference(h, np.array([0]), 3)[1].tolist() == [[1, 0, 2]]
    b = torch.tensor([[1.0, 1.0078125, 0.99609375]], dtype=torch.bfloat16)
    assert cls.rank_reference(b, np.array([2]), 3)[0].tolist() == [2]


def test_rank_is_the_count_of_predecessors_on_rows_full_of_ties():
    rng = np.random.default_rng(5)
    logits = rng.choice(np.array([-1.0, 0.0, -0.0, 2.5], dtype=F32), size=(9, 37))
    lab = rng.integers(-1, 38, 9)
    rank, top = cls.rank_reference(logits, lab, 8)
    keys = cls._boxes.score_keys(logits.reshape(-1)).reshape(9, 37).astype(np.int64)
    for b in range(9):
        before = lambda i: sum(1 for j in range(37) if keys[b, j] > keys[b, i] or (keys[b, j] == keys[b, i] and j < i))  # noqa: E731
        assert rank[b] == (before(lab[b]) if 0 <= lab[b] < 37 else 37)
        assert [before(int(c)) for c in top[b]] == list(range(8))


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------------
def test_one_fp32_product_is_torchs_scaling_for_every_batch_size(golden):
    pairs = golden["scale_pairs"]
    got = cls.batch_accuracy(pairs[:, 1], pairs[:, 0])
    assert got.tobytes() == golden["scale_out"].tobytes()
    late = (pairs[:, 1].astype(np.float64) * (100.0 / pairs[:, 0])).astype(F32)       # the fp64 product rounded afterwards is not it
    assert np.count_nonzero(late != golden["scale_out"]) > 0


def test_summarize_per_batch_and_data_set_means(golden):
    n, correct = golden["mean_n"], golden["mean_correct"]
    N = int(n.sum())
    recs = {"n": n, "correct": correct, "topk": np.array([1, 5], dtype=np.int32), "rank": np.zeros(N, dtype=np.int32), "fd": np.full(N, np.nan, dtype=F32)}
    out = cls.summarize(recs)
    assert out["batch_acc"].tobytes() == golden["mean_batch_acc"].tobytes() and out["images"] == N == 301
    for t, k in enumerate((1, 5)):
        values = np.repeat(golden["mean_batch_acc"][:, t], n)
        exact = math.fsum(values.astype(np.float64).tolist()) / N
        ref = float(golden[f"mean_acc{k}"])
        print(k, out[f"acc{k}"], ref, exact)
        assert abs(out[f"acc{k}"] - ref) <= abs(ref - exact) + ulp(ref)
        assert abs(out[f"acc{k}"] - exact) <= ulp(exact)
        assert out[f"acc{k}_exact"] == 100.0 * int(correct[:, t].sum()) / N
    assert math.isnan(out["fd"])


def test_merge_records_concatenates_and_renumbers(golden):
    parts = [[(golden[f"acc{i}_logits"], golden[f"acc{i}_labels"]) for i in idx] for idx in ((0, 1), (2,), (3, 4))]
    whole = cls.records_reference([b for p in parts for b in p])
    merged = cls.merge_records([cls.records_reference(p) for p in parts])
    for name in whole:
        assert np.array_equal(whole[name], merged[name], equal_nan=name == "fd") and whole[name].dtype == merged[name].dtype, name
    assert merged["batch"].tolist() == np.repeat(np.arange(5), golden["acc_batches"]).tolist()
    with pytest.raises(ValueError):
        cls.merge_records([cls.records_reference(parts[0]), cls.records_reference(parts[1], topk=(1,))])


# ---- feature distance ---------------------------------------------------------------------------------------------------------------------
def exact_mean(a, b):
    d = np.abs(a.astype(F32) - b.astype(F32)).astype(F32).reshape(a.shape[0], -1)
    return [math.fsum(row.astype(np.float64).tolist()) / row.size for row in d]


def test_fdist_is_one_rounding_from_exact_and_within_torchs_own_error(golden):
    a, b = golden["fd_res"], golden["fd_gt"]
    got = cls.fdist_reference(a, b)
    assert got.dtype == F32 and got.shape == (3,)
    for g, e, t in zip(got.tolist(), exact_mean(a, b), golden["fd_out"].tolist()):
        print(g, e, t, abs(t - e) / ulp(e))
        assert abs(g - e) <= ulp(e)
        assert abs(g - t) <= abs(t - e) + ulp(t)
    recs = cls.records_reference([(np.zeros((3, 4), dtype=F32), np.zeros(3, dtype=np.int64), a, b)])
    ours, ref, exact = cls.summarize(recs)["fd"], float(golden["fd_mean"]), math.fsum(got.astype(np.float64).tolist()) / 3
    assert recs["fd"].tobytes() == got.tobytes() and abs(ours - ref) <= abs(ref - exact) + ulp(ref)


@pytest.mark.parametrize("n", [1, 255, 256, 257, cls.FD_CHUNK - 1, cls.FD_CHUNK, cls.FD_CHUNK + 1, 2 * cls.FD_CHUNK + 3])
def test_fdist_order_is_the_written_one(n):
    """the restatement's reshapes against the rule as a plain loop: lane sums in element order, the tree, the chunks in order"""
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal((2, n)).astype(F32), rng.standard_normal((2, n)).astype(F32)
    want = []
    for row in np.abs(a - b).astype(F32).astype(np.float64):
        total = 0.0
        for lo in range(0, n, cls.FD_CHUNK):
            chunk = row[lo:lo + cls.FD_CHUNK]
            lanes = [0.0] * 256
            for i, v in enumerate(chunk.tolist()):
                lanes[i % 256] += v
            step = 128
            while step:
                for l in range(step):
                    lanes[l] += lanes[l + step]
                step //= 2
            total += lanes[0]
        want.append(F32(total / n))
    got = cls.fdist_reference(a, b)
    assert got.tobytes() == np.array(want, dtype=F32).tobytes()
    for g, e in zip(got.tolist(), exact_mean(a, b)):
        assert abs(g - e) <= ulp(e)


def test_fdist_halves_take_the_difference_in_fp32():
    a = np.array([[1.0, 2048.0, 0.5]], dtype=np.float16)
    b = np.array([[0.99951171875, 0.5, -65504.0]], dtype=np.float16)
    want = F32((np.float64(F32(1.0) - F32(0.99951171875)) + 2047.5 + 65504.5) / 3)       # fp16 would round 2047.5 and overflow 65504.5
    assert cls.fdist_reference(a, b).tolist() == [float(want)]
    t = torch.tensor([[1.0, 3.0]], dtype=torch.bfloat16)
    assert cls.fdist_reference(t, torch.zeros_like(t)).tolist() == [2.0]
    assert math.isnan(cls.fdist_reference(np.array([[NAN, 1.0]], dtype=F32), np.zeros((1, 2), dtype=F32))[0])


# ---- normalisation and geometry -------------------------------------------------------------------------------------------------------------
def test_normalize_is_sub_then_div_with_fp32_constants(golden):
    k = golden["norm_constants"]
    assert all(np.array_equal(a, b) for a, b in zip(k, (cls.IMAGENET_MEAN, cls.IMAGENET_STD, cls.IMAGENET_INV_MEAN, cls.IMAGENET_INV_STD)))
    y = cls.normalize_reference(golden["norm_x"])
    assert y.dtype == F32 and y.tobytes() == golden["norm_out"].tobytes()
    back = cls.normalize_reference(y, cls.IMAGENET_INV_MEAN, cls.IMAGENET_INV_STD)
    assert back.tobytes() == golden["norm_inv_out"].tobytes() and np.abs(back - golden["norm_x"]).max() < 1e-6
    assert cls.prepare_reference(golden["norm_x"]).tobytes() == y.tobytes()
    assert cls.prepare_reference(golden["norm_x"], size=(4, 6), upsample=2, normalize=False).shape == (2, 3, 8, 12)
    with pytest.raises(ValueError):
        cls.normalize_reference(golden["norm_x"], std=[1.0, 0.0, 1.0])


def test_window_equals_the_references_crops_and_augment_in_all_eight_states(golden):
    src = golden["geo_src"]
    assert "stand-in for cv2.flip" in str(golden["flip_stand_in"])
    assert np.array_equal(cls.window_reference(src, (5, 5), ((9 - 5) // 2, (11 - 5) // 2)), golden["geo_center5"])
    assert np.array_equal(cls.window_reference(src, (5, 5), tuple(golden["geo_random5_pos"])), golden["geo_random5"])
    origin, hw = tuple(golden["geo_aug_origin"]), tuple(golden["geo_aug_hw"])
    seen = set()
    for state in range(8):
        h, v, r = bool(state & 1), bool(state & 2), bool(state & 4)
        got = cls.window_reference(src, hw, origin, h, v, r)
        assert got.shape == ((7, 5, 3) if r else (5, 7, 3)) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, golden[f"geo_aug{state}"]), state
        assert np.array_equal(cls.window_reference(src[:, :, 0], hw, origin, h, v, r), golden[f"geo_aug{state}"][:, :, 0])
        seen.add(got.tobytes())
    assert len(seen) == 8
    # fill outside the source, through the transpose
    out = cls.window_reference(src, (4, 3), (-1, 9), True, False, True, fill=7)
    assert out.shape == (3, 4, 3) and np.all(out[0, :, :] == 7) and np.all(out[:, 0, :] == 7) and np.array_equal(out[2, 1], src[0, 9])


def test_resized_extent_truncates_in_double():
    assert cls.cls_resized_extent(256, 375, 500) == (341, 256)          # 256 * 500 / 375 = 341.33
    assert cls.cls_resized_extent(256, 500, 375) == (256, 341)
    assert cls.cls_resized_extent(256, 300, 300) == (256, 256)
    assert cls.cls_resized_extent(224, 333, 500) == (336, 224) and 224 * 500 / 333 > 336.3        # int() truncates, never rounds up
    assert cls.cls_resized_extent(7, 3, 5) == (int(7 * 5 / 3), 7) == (11, 7)
    with pytest.raises(ValueError):
        cls.cls_resized_extent(0, 3, 5)


def test_draw_cls_geometry_is_reproducible_and_leaves_the_other_streams_alone():
    from edtr_amd import degrade, labels
    seg, deg = labels.SegGeometry(gt_size=40, resize_range=[0.5, 2.0], out_size=32, crop_type="random", hflip=True), degrade.DegradeConfig()
    before = (labels.draw_geometry(seg, 7, 3, (50, 70)), degrade.draw_params(deg, 7, 3))
    cfg = cls.ClsGeometry(gt_size=40, out_size=32, crop_type="random", hflip=True, rotation=True)
    a = cls.draw_cls_geometry(cfg, 7, 3, (50, 70))
    assert a == cls.draw_cls_geometry(cfg, 7, 3, (50, 70)) and a.size == (40, 56) and a.out_hw == (32, 32)
    assert 0 <= a.origin[0] <= 8 and 0 <= a.origin[1] <= 24
    after = (labels.draw_geometry(seg, 7, 3, (50, 70)), degrade.draw_params(deg, 7, 3))
    assert repr(before) == repr(after)
    assert cls.CLS_GEOMETRY_WORD not in (labels.GEOMETRY_WORD,) and labels.draw_geometry(seg, 7, 3, (50, 70)).origin == before[0].origin
    draws = [cls.draw_cls_geometry(cfg, 7, i, (50, 70)) for i in range(64)]
    assert {(d.hflip, d.vflip, d.rot90) for d in draws} == {(h, v, r) for h in (False, True) for v in (False, True) for r in (False, True)}
    assert len({d.origin for d in draws}) > 16
    still = [cls.draw_cls_geometry(cls.ClsGeometry(40, 32, "center"), 7, i, (50, 70)) for i in range(8)]
    assert all(d.origin == (4, 12) and not (d.hflip or d.vflip or d.rot90) for d in still)
    assert cls.draw_cls_geometry(cls.ClsGeometry(32, 32, "none"), 1, 1, (9, 9)).origin == (0, 0)
    with pytest.raises(ValueError):
        cls.draw_cls_geometry(cls.ClsGeometry(32, 32, "none"), 1, 1, (9, 12))
    nested = {"dataset": {"train": {"params": {"gt_size": 256, "out_size": 224, "crop_type": "center", "hflip": True, "rotation": False, "blur_kernel_size": 41}}}}
    assert cls.load_cls_geometry(nested) == cls.ClsGeometry(256, 224, "center", True, False)


def test_prepare_image_reference_is_resize_then_window(golden):
    from edtr_amd.imageio import resize_u8_reference
    img = np.tile(golden["geo_src"], (4, 4, 1))[:30, :40]
    geom = cls.draw_cls_geometry(cls.ClsGeometry(24, 20, "random", True, True), 11, 5, img.shape[:2])
    want = cls.window_reference(resize_u8_reference(img, 32, 24), (20, 20), geom.origin, geom.hflip, geom.vflip, geom.rot90)
    assert geom.size == (24, 32) and np.array_equal(cls.prepare_image_reference(img, geom), want)


def test_image_folder_lists_as_torchvision_does(tmp_path):
    for rel in ("b/2.png", "b/1.JPG", "b/sub/0.jpeg", "b/notes.txt", "a/z.bmp", "a/deep/er/x.webp", "c/only.tif"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    (tmp_path / "stray.png").write_bytes(b"")
    samples, classes = cls.image_folder(tmp_path)
    assert classes == ["a", "b", "c"]
    assert [(os.path.relpath(p, tmp_path), i) for p, i in samples] == [
        ("a/z.bmp", 0), ("a/deep/er/x.webp", 0), ("b/1.JPG", 1), ("b/2.png", 1), ("b/sub/0.jpeg", 1), ("c/only.tif", 2)]
    (tmp_path / "d").mkdir()
    with pytest.raises(FileNotFoundError, match="d"):
        cls.image_folder(tmp_path)
    with pytest.raises(FileNotFoundError):
        cls.image_folder(tmp_path / "d")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("edtr_cls_rank", "edtr_cls_fdist", "edtr_cls_commit", "edtr_cls_normalize", "edtr_cls_window")


def test_the_new_symbols_are_declared_bound_exported_and_built_behind_the_glue_wall():
    from edtr_amd import build, lib
    assert all(s in lib.DECLARED_SYMBOLS for s in SYMBOLS)
    assert "cls.hip" in build.GLUE_SOURCES and "cls.hip" not in build.SOURCES
    assert "glue.h" in [os.path.basename(d) for d in build.object_deps("cls.hip")]
    caps = (lib.CLS_MAX_CLASSES, lib.CLS_MAX_KEEP, lib.CLS_MAX_TOPK, lib.CLS_FD_CHUNK, lib.CLS_FD_MAX_ELEMS)
    assert caps == (cls.MAX_CLASSES, cls.MAX_KEEP, cls.MAX_TOPK, cls.FD_CHUNK, cls.FD_MAX_ELEMS) and cls.FD_CHUNK % cls.FD_LANES == 0
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == 10 and all(hasattr(handle, s) for s in SYMBOLS)


def test_the_entry_points_reject_bad_arguments_before_any_launch():
    import ctypes
    from edtr_amd import build, lib
    build.build_library()
    h = lib.load()
    p = 4096            # a non-NULL, aligned stand-in: every call below fails its checks before the pointer is used
    NULL, SHAPE, ALIGN, DTYPE, UNSUPPORTED = -1, -2, -3, -4, -5

    def rank(**kw):
        a = dict(dt=0, logits=p, labels=p, B=4, C=10, K=5, rl=p, rr=p, rt=p, off=p, cap=16)
        a.update(kw)
        return h.edtr_cls_rank(*a.values(), None)
    assert rank(logits=None) == NULL and rank(rr=None) == NULL and rank(rt=None) == NULL
    assert rank(B=0) == SHAPE and rank(C=0) == SHAPE and rank(K=-1) == SHAPE and rank(cap=0) == SHAPE and rank(labels=None, rr=None, K=0, rt=None) == SHAPE
    assert rank(B=65536) == UNSUPPORTED and rank(C=65537) == UNSUPPORTED and rank(K=9) == UNSUPPORTED and rank(cap=(1 << 30) + 1) == UNSUPPORTED
    assert rank(dt=3) == DTYPE and rank(dt=-1) == DTYPE
    assert rank(logits=p + 2) == ALIGN and rank(dt=1, logits=p + 1) == ALIGN and rank(labels=p + 2) == ALIGN and rank(off=p + 1) == ALIGN and rank(rt=p + 2) == ALIGN
    assert rank(B=0, logits=None) == NULL and rank(B=0, dt=9) == SHAPE and rank(C=65537, dt=9) == UNSUPPORTED and rank(dt=9, logits=p + 1) == DTYPE      # the order

    def fdist(**kw):
        a = dict(dt=0, a=p, b=p, B=2, n=100, part=p)
        a.update(kw)
        return h.edtr_cls_fdist(*a.values(), None)
    assert fdist(a=None) == NULL and fdist(b=None) == NULL and fdist(part=None) == NULL
    assert fdist(B=0) == SHAPE and fdist(n=0) == SHAPE and fdist(B=65536) == UNSUPPORTED and fdist(n=(1 << 28) + 1) == UNSUPPORTED
    assert fdist(dt=7) == DTYPE and fdist(a=p + 2) == ALIGN and fdist(dt=2, b=p + 1) == ALIGN and fdist(part=p + 4) == ALIGN

    topk = (ctypes.c_int32 * 2)(1, 5)

    def commit(**kw):
        a = dict(rr=p, fd=p, rb=p, B=4, part=p, n=100, topk=topk, nt=2, bn=p, bc=p, off=p, cap=16, bcap=4)
        a.update(kw)
        return h.edtr_cls_commit(*a.values(), None)
    assert commit(fd=None) == NULL and commit(rb=None) == NULL and commit(bn=None) == NULL and commit(off=None) == NULL
    assert commit(rr=None) == NULL and commit(topk=None) == NULL and commit(bc=None) == NULL
    assert commit(B=0) == SHAPE and commit(nt=-1) == SHAPE and commit(cap=0) == SHAPE and commit(bcap=0) == SHAPE and commit(n=0) == SHAPE
    assert commit(topk=(ctypes.c_int32 * 2)(1, 0)) == SHAPE
    assert commit(B=65536) == UNSUPPORTED and commit(nt=5) == UNSUPPORTED and commit(topk=(ctypes.c_int32 * 2)(1, 9)) == UNSUPPORTED
    assert commit(n=(1 << 28) + 1) == UNSUPPORTED and commit(bcap=(1 << 30) + 1) == UNSUPPORTED
    assert commit(rr=p + 2) == ALIGN and commit(fd=p + 1) == ALIGN and commit(part=p + 4) == ALIGN and commit(off=p + 2) == ALIGN

    consts = (ctypes.c_float * 3)(0.5, 0.5, 0.5)

    def norm(**kw):
        a = dict(x=p, out=p, B=2, ch=3, H=5, W=7, mean=consts, std=consts)
        a.update(kw)
        return h.edtr_cls_normalize(*a.values(), None)
    assert norm(ch=1) == UNSUPPORTED and norm(x=None) == NULL and norm(out=None) == NULL and norm(mean=None) == NULL and norm(std=None) == NULL
    assert norm(B=0) == SHAPE and norm(B=65536) == SHAPE and norm(H=0) == SHAPE and norm(W=(1 << 24) + 1) == UNSUPPORTED and norm(x=p + 2) == ALIGN
    assert norm(std=(ctypes.c_float * 3)(1, 0, 1)) == SHAPE and norm(mean=(ctypes.c_float * 3)(1, NAN, 1)) == SHAPE

    def window(**kw):
        a = dict(src=p, h=9, w=11, ch=3, dst=p, H=5, W=7, y0=0, x0=0, hf=0, vf=0, tr=1, fill=0)
        a.update(kw)
        return h.edtr_cls_window(*a.values(), None)
    assert window(ch=2) == UNSUPPORTED and window(src=None) == NULL and window(dst=None) == NULL
    assert window(h=0) == SHAPE and window(W=0) == SHAPE and window(H=(1 << 24) + 1) == UNSUPPORTED and window(y0=-(1 << 24) - 1) == UNSUPPORTED
    assert window(hf=2) == DTYPE and window(vf=-1) == DTYPE and window(tr=2) == DTYPE and window(fill=256) == DTYPE
