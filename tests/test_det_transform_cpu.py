"""Host side of edtr_amd/detinput.py: the extent rule and the numpy restatement against the reference's own GeneralizedRCNNTransform
(tests/golden/det_transform.npz, written by tools/make_det_transform_goldens.py), the wrappers' refusals, and the C ABI.  No GPU."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from edtr_amd import boxes, detinput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMED = {(375, 500): (799, 1066), (500, 375): (1066, 799), (333, 500): (800, 1201), (480, 640): (800, 1066), (427, 640): (800, 1199), (512, 512): (800, 800)}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "det_transform.npz"))


def set_of(gold, tag):
    n = len(gold[f"{tag}_image_sizes"])
    kw = dict(min_size=tuple(gold[f"{tag}_min_size"].tolist()), max_size=int(gold[f"{tag}_max_size"]), image_mean=gold[f"{tag}_mean"],
              image_std=gold[f"{tag}_std"], size_divisible=int(gold[f"{tag}_size_divisible"]), fixed_size=tuple(gold[f"{tag}_fixed_size"].tolist()) or None)
    return [gold[f"{tag}_image{i}"] for i in range(n)], kw


def naive_extent(h, w, lo, hi):
    s = min(lo / min(h, w), hi / max(h, w))
    return math.floor(h * s), math.floor(w * s)


# ---- extents -----------------------------------------------------------------------------------------------------------------------------
def test_resized_extent_equals_every_recorded_row_and_the_naive_rule_does_not(gold):
    rows = gold["extent_rows"].tolist()
    assert len(rows) >= 2000
    assert all(detinput.resized_extent(h, w, lo, hi) == (oh, ow) for h, w, lo, hi, oh, ow in rows)
    differ = sum(naive_extent(h, w, lo, hi) != (oh, ow) for h, w, lo, hi, oh, ow in rows)
    print(f"the Python-float rule differs on {differ} of {len(rows)} rows")
    assert differ > 0.05 * len(rows)                    # the golden can tell the two rules apart
    named = {(h, w): (oh, ow) for h, w, lo, hi, oh, ow in rows if (lo, hi) == (800, 1333)}
    assert all(named.get(k) == v for k, v in NAMED.items())
    assert detinput.resized_extent(375, 500) == (799, 1066) and naive_extent(375, 500, 800, 1333) == (800, 1066)


def test_resized_extent_arguments():
    assert detinput.resized_extent(53, 47, 64, 100, fixed_size=(48, 40)) == (40, 48)            # (fw, fh) -> (fh, fw)
    assert detinput.resized_extent(53, 47, (32, 64), 100) == detinput.resized_extent(53, 47, 64, 100) == (72, 63)
    assert [detinput.resized_extent(h, w, 64, 100) for h, w in ((40, 167), (61, 163), (64, 64), (17, 9))] == [(23, 100), (37, 99), (64, 64), (100, 52)]
    with pytest.raises(ValueError):
        detinput.resized_extent(0, 5)
    with pytest.raises(ValueError):
        detinput.resized_extent(1, 4000, 1, 2)          # nothing left of the short side


def test_batch_extent():
    assert detinput.batch_extent([(72, 63), (23, 100), (37, 99), (64, 64)]) == (96, 128)
    assert detinput.batch_extent([(37, 99)], 1) == (37, 99) and detinput.batch_extent([(800, 1066), (799, 1201)]) == (800, 1216)
    assert detinput.batch_extent([(64, 64)], 32) == (64, 64) and detinput.batch_extent([(65, 64)], 32) == (96, 64)
    with pytest.raises(ValueError):
        detinput.batch_extent([])
    with pytest.raises(ValueError):
        detinput.batch_extent([(4, 4)], 0)


# ---- the restatement against the reference's forward ---------------------------------------------------------------------------------------
def test_the_sets_cover_what_they_are_there_for(gold):
    assert gold["set_tags"].tolist() == ["ragged", "odd", "fixed", "four"]
    assert gold["ragged_image_sizes"].tolist() == [[72, 63], [23, 100], [37, 99], [64, 64]] and gold["ragged_batch"].shape == (4, 3, 96, 128)
    shapes = [gold[f"ragged_image{i}"].shape[1:] for i in range(4)]
    assert sum(naive_extent(h, w, 64, 100) != tuple(e) for (h, w), e in zip(shapes, gold["ragged_image_sizes"].tolist())) == 3
    assert gold["odd_batch"].shape == (2, 3, 100, 99) and gold["fixed_image_sizes"].tolist() == [[40, 48]] * 2 and gold["four_batch"].shape[1] == 4


@pytest.mark.parametrize("tag", ["ragged", "odd", "fixed", "four"])
def test_transform_reference_meets_the_references_forward(gold, tag):
    """Shapes, image_sizes and the padding (+0.0 in bits) exactly; an image whose scale is exactly 1 bit for bit; every other image
    within 4 x ref_err, the reference's own distance from itself in fp64 (both from the golden): CPU ATen's bilinear kernel cannot be
    reproduced bit for bit from its written rule.  Measured when the goldens were made — max |restatement - reference| / ref_err:
    ragged 7.5e-6 / 4.6e-5, odd 7.0e-6 / 4.5e-5, fixed 1.6e-6 / 9.8e-6, four 3.6e-6 / 3.6e-6."""
    images, kw = set_of(gold, tag)
    want, ref_err = gold[f"{tag}_batch"], float(gold[f"{tag}_ref_err"])
    assert 0 < ref_err < 1e-4
    got, sizes, original = detinput.transform_reference(images, **kw)
    assert got.dtype == F32 and got.shape == want.shape and sizes == [tuple(s) for s in gold[f"{tag}_image_sizes"].tolist()]
    assert original == [v.shape[1:] for v in images]
    identities = 0
    for i, ((oh, ow), (h, w)) in enumerate(zip(sizes, original)):
        pad = np.ones(want.shape[2:], dtype=bool)
        pad[:oh, :ow] = False
        assert not got[i].view(np.uint32)[:, pad].any() and not want[i].view(np.uint32)[:, pad].any()
        e = float(np.abs(got[i].astype(np.float64) - want[i]).max())
        print(f"[{tag} image {i}: {h} x {w} -> {oh} x {ow}] max abs err {e:.3e} (4 x ref_err {4 * ref_err:.3e})")
        if (oh, ow) == (h, w):
            identities += 1
            assert np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32))
        assert e <= 4 * ref_err
    assert identities == (1 if tag in ("ragged", "four") else 0)
    for i, (o, e) in enumerate(zip(original, sizes)):
        assert np.array_equal(boxes.resize_boxes_reference(gold[f"{tag}_boxes{i}"], o, e), gold[f"{tag}_resized_boxes{i}"])


def test_transform_reference_rounds_a_16_bit_batch_once(gold):
    from edtr_amd import labels
    images, kw = set_of(gold, "fixed")
    full = detinput.transform_reference(images, **kw)[0]
    for dtype in ("float16", "bfloat16"):
        got = detinput.transform_reference(images, dtype=dtype, **kw)[0]
        assert got.dtype == F32 and np.array_equal(got, labels._round_to(full, dtype)) and not np.array_equal(got, full)
    torch = pytest.importorskip("torch")
    bf = torch.from_numpy(full).to(torch.bfloat16).float().numpy()
    assert np.array_equal(detinput.transform_reference(images, dtype="bfloat16", **kw)[0], bf)
    with pytest.raises(ValueError):
        detinput.transform_reference(images, dtype="float64", **kw)


def test_one_batched_array_is_the_list_of_its_images_and_other_channel_counts_normalise_alike():
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (2, 3, 20, 31)).astype(F32)
    a, b = detinput.transform_reference(x, 32, 50), detinput.transform_reference([x[0], x[1]], 32, 50)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    one = detinput.transform_reference([x[0, 1:2]], 32, 50, [0.456], [0.224])[0]
    three = detinput.transform_reference([x[0]], 32, 50)[0]
    assert np.array_equal(one[:, 0], three[:, 1])                   # the per-plane path of another channel count gives the same bits


def test_the_wrappers_refuse_what_the_reference_refuses():
    x = np.zeros((3, 8, 8), dtype=F32)
    for fn in (detinput.transform_reference, detinput.transform):
        with pytest.raises(TypeError, match="floating type"):
            fn([np.zeros((3, 8, 8), dtype=np.uint8)])
        with pytest.raises(ValueError, match="3d tensors"):
            fn([np.zeros((8, 8), dtype=F32)])
        with pytest.raises(ValueError):
            fn([x], image_std=[0.2, 0.0, 0.2])
        with pytest.raises(ValueError):
            fn([x], image_mean=[0.5], image_std=[0.5])
        with pytest.raises(ValueError):
            fn([])
    with pytest.raises(ValueError):
        detinput.transform_reference([x, np.zeros((1, 8, 8), dtype=F32)])
    with pytest.raises(TypeError):
        detinput.transform_reference([np.zeros((3, 8, 8), dtype=np.float64)])


def test_detector_transform_arguments_and_targets():
    t = detinput.DetectorTransform((480, 64), 100, [0.5, 0.5, 0.5], [0.25, 0.25, 0.25], size_divisible=16, fixed_size=None)
    assert t.min_size == (480, 64) and t.max_size == 100 and t.size_divisible == 16 and t.fixed_size is None
    assert detinput.DetectorTransform(64, 100, [0.5], [0.5]).min_size == (64,)
    with pytest.raises(ValueError):
        detinput.DetectorTransform(64, 100, [0.5, 0.5], [0.5, 0.0])
    for missing in ("masks", "keypoints"):
        with pytest.raises(ValueError, match=missing):
            detinput._resize_targets([{"boxes": np.zeros((1, 4), dtype=F32), missing: None}], [(8, 8)], [(16, 16)])
    with pytest.raises(ValueError):
        detinput._resize_targets([], [(8, 8)], [(16, 16)])
    assert detinput._resize_targets(None, [(8, 8)], [(16, 16)]) is None
    assert detinput._resize_targets([{"labels": 3}], [(8, 8)], [(16, 16)]) == [{"labels": 3}]
    assert detinput.ImageBatch._fields == ("tensors", "image_sizes")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_exported_and_the_abi_is_still_10():
    from edtr_amd import build, lib
    assert "edtr_det_transform" in lib.DECLARED_SYMBOLS
    assert lib.ABI_VERSION == 10
    assert "det_transform.hip" in build.GLUE_SOURCES and "det_transform.hip" not in build.SOURCES
    assert "glue.h" in [os.path.basename(d) for d in build.object_deps("det_transform.hip")]
    caps = (lib.DET_MAX_CHANNELS, lib.DET_MAX_EXTENT, lib.DET_TILE_W, lib.DET_TILE_H)
    assert caps == (detinput.MAX_CHANNELS, detinput.MAX_EXTENT, detinput.TILE_W, detinput.TILE_H)
    # the blend and its indices live once, in glue.h, and the new unit calls them
    src = {n: open(os.path.join(ROOT, "edtr_amd", "csrc", n)).read() for n in ("glue.h", "det_transform.hip")}
    for helper in ("source_index(", "index_lambda(", "blend_taps("):
        assert f"float {helper}" in src["glue.h"] or f"void {helper}" in src["glue.h"]
        assert helper in src["det_transform.hip"] and f"float {helper}" not in src["det_transform.hip"] and f"void {helper}" not in src["det_transform.hip"]
    build.build_library()
    handle = lib.load()
    assert handle.edtr_abi_version() == 10 and hasattr(handle, "edtr_det_transform")


def test_the_descriptor_mirror_has_the_c_layout(tmp_path):
    from edtr_amd import lib
    fields = [n for n, _ in lib.DetImage._fields_]
    names = ",".join(f"offsetof(edtr_det_image,{n})" for n in fields)
    src = tmp_path / "det.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edtr_hip.h"\nint main(){size_t v[]={sizeof(edtr_det_image),' + names +
                   '};for(unsigned i=0;i<sizeof v/sizeof*v;++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / "det"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(lib.DetImage) == 24
    assert out[1:] == [getattr(lib.DetImage, n).offset for n in fields] == [0, 8, 12, 16, 20]


def test_the_entry_point_rejects_bad_arguments_before_any_launch():
    from edtr_amd import build, lib
    build.build_library()
    h = lib.load()
    p = 4096            # a non-NULL, aligned stand-in: every call below fails its checks before the pointer is used
    NULL, SHAPE, ALIGN, DTYPE = -1, -2, -3, -4

    def descs(*rows):
        d = (lib.DetImage * len(rows))()
        for e, row in zip(d, rows):
            e.src, e.h, e.w, e.oh, e.ow = row
        return d

    def floats(*v):
        return (C.c_float * len(v))(*v)

    def call(**kw):
        a = dict(host=descs((p, 8, 8, 16, 16)), dev=p, N=1, C=3, mean=floats(0.5, 0.5, 0.5), std=floats(0.25, 0.25, 0.25), dt=0, batch=p, H=32, W=32)
        a.update(kw)
        return h.edtr_det_transform(*a.values(), None)
    assert call(host=None) == NULL and call(dev=None) == NULL and call(mean=None) == NULL and call(std=None) == NULL and call(batch=None) == NULL
    assert call(host=descs((None, 8, 8, 16, 16))) == NULL
    assert call(N=0) == SHAPE and call(N=65536) == SHAPE and call(C=0) == SHAPE and call(C=5) == SHAPE
    for bad in ((p, 0, 8, 16, 16), (p, 8, 0, 16, 16), (p, 8, 8, 0, 16), (p, 8, 8, 16, 0), (p, 32769, 8, 16, 16), (p, 8, 32769, 16, 16)):
        assert call(host=descs(bad)) == SHAPE
    assert call(H=0) == SHAPE and call(W=0) == SHAPE and call(H=32769) == SHAPE and call(W=32769) == SHAPE
    assert call(host=descs((p, 8, 8, 33, 16))) == SHAPE and call(host=descs((p, 8, 8, 16, 33))) == SHAPE              # oh > H, ow > W
    assert call(H=32768, W=32768, host=descs((p, 8, 8, 32769, 16))) == SHAPE
    assert call(std=floats(0.25, 0.0, 0.25)) == SHAPE and call(std=floats(0.25, 0.25, float("nan"))) == SHAPE
    assert call(C=4, mean=floats(0.5, 0.5, 0.5, 0.5), std=floats(0.25, 0.25, 0.25, 0.0)) == SHAPE
    assert call(dt=3) == DTYPE and call(dt=-1) == DTYPE
    assert call(host=descs((p + 2, 8, 8, 16, 16))) == ALIGN and call(batch=p + 2) == ALIGN and call(dt=1, batch=p + 1) == ALIGN and call(dev=p + 4) == ALIGN
    assert call(N=2, host=descs((p, 8, 8, 16, 16), (p, 8, 8, 16, 64))) == SHAPE                                   # the second image is checked too
