"""Host side of the ragged, batched image boundary (edtr_amd/imageio.py `plan_buckets`, `ingest_resized_reference`,
`emit_packed_reference`; lib.ImageDesc against include/edtr_hip.h; rng.shard_bucket_ids; the restore command line).  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "edtr_hip.h")
BATCH_SYMBOLS = ("edtr_image_resize_h_batch", "edtr_image_resize_ingest_batch", "edtr_image_emit_batch")

# (h, w) that pad (min_size 128, multiple 64) to 128 x 128 (A), 128 x 192 (B) and 192 x 128 (C), interleaved; five images in A
SIZES = [(100, 75), (64, 150), (37, 53), (130, 60), (128, 128), (90, 192), (1, 1), (129, 128), (120, 17)]
EXTENTS = [(128, 128), (128, 192), (128, 128), (192, 128), (128, 128), (128, 192), (128, 128), (192, 128), (128, 128)]


def test_plan_buckets_partitions_in_data_set_order():
    from edtr_amd import imageio
    assert [imageio.batch_extent([s], multiple=64, min_size=128) for s in SIZES] == EXTENTS
    plan = imageio.plan_buckets(SIZES, 2, min_size=128, multiple=64)
    assert plan == [((128, 128), [0, 2]), ((128, 128), [4, 6]), ((128, 128), [8]),          # five images: chunks of 2, 2, 1
                    ((128, 192), [1, 5]), ((192, 128), [3, 7])]                             # buckets in the order they were opened
    seen = sorted(k for _, idx in plan for k in idx)
    assert seen == list(range(len(SIZES)))                                                  # every index exactly once
    for hw, idx in plan:
        assert idx == sorted(idx) and 1 <= len(idx) <= 2
        assert all(EXTENTS[k] == hw for k in idx)
    assert imageio.plan_buckets(list(SIZES), 2, min_size=128, multiple=64) == plan          # the same input, the same plan
    ones = imageio.plan_buckets(SIZES, 1, min_size=128, multiple=64)
    assert all(len(idx) == 1 for _, idx in ones) and len(ones) == len(SIZES)
    for hw in set(EXTENTS):                                                                 # data-set order inside every bucket
        assert [idx[0] for h, idx in ones if h == hw] == [k for k, e in enumerate(EXTENTS) if e == hw]
    same = imageio.plan_buckets([(128, 128)] * 4, 1, min_size=128, multiple=64)
    assert [idx for _, idx in same] == [[0], [1], [2], [3]]                                 # one bucket: plain data-set order
    assert imageio.plan_buckets(SIZES, 100, min_size=128, multiple=64) == [((128, 128), [0, 2, 4, 6, 8]), ((128, 192), [1, 5]), ((192, 128), [3, 7])]
    assert imageio.plan_buckets([], 4, min_size=128, multiple=64) == []
    with pytest.raises(ValueError):
        imageio.plan_buckets(SIZES, 0, min_size=128, multiple=64)


@pytest.mark.parametrize("pad", ["zero", "replicate"])
def test_ingest_resized_reference_is_resize_then_divide_permute_pad(golden_dir, pad):
    from edtr_amd import imageio
    g = np.load(os.path.join(golden_dir, "pillow_bicubic.npz"))
    names = [str(n) for n in g["names"]]
    images = [g[f"{n}_in"] for n in names]
    wants = [g[f"{n}_out"] for n in names]
    out_sizes = [(w.shape[1], w.shape[0]) for w in wants]
    batch, sizes = imageio.ingest_resized_reference(images, out_sizes, pad=pad, multiple=64)
    H, W = imageio.batch_extent([w.shape[:2] for w in wants], multiple=64)
    assert batch.dtype == np.float32 and batch.shape == (len(names), 3, H, W) and sizes == [w.shape[:2] for w in wants]
    for b, (im, want, (ow, oh)) in enumerate(zip(images, wants, out_sizes)):
        small = imageio.resize_u8_reference(im, ow, oh)
        assert np.array_equal(small, want)                                                  # Pillow's recorded bytes
        x = torch.from_numpy((small / 255.0).astype(np.float32)).permute(2, 0, 1)[None]
        ref = torch.nn.functional.pad(x, (0, W - ow, 0, H - oh), mode="replicate" if pad == "replicate" else "constant")[0].numpy()
        assert np.array_equal(batch[b].view(np.uint32), ref.view(np.uint32)), names[b]
    with pytest.raises(ValueError):
        imageio.ingest_resized_reference(images, out_sizes, pad="reflect")


def test_emit_packed_reference_is_emit_reference_at_the_packed_offsets():
    from edtr_amd import imageio
    rng = np.random.default_rng(1)
    batch = rng.uniform(-0.2, 1.2, size=(4, 3, 24, 20)).astype(np.float32)
    batch[1, 2, 0, 0] = np.nan
    sizes = [(24, 20), (5, 7), (1, 1), (17, 16)]
    packed, offs = imageio.emit_packed_reference(batch, sizes)
    assert packed.dtype == np.uint8 and len(offs) == 4 and offs[0] == 0
    end = 0
    for i, ((h, w), o) in enumerate(zip(sizes, offs)):
        assert o % 4 == 0 and o >= end and o - end < 4                                      # back to back, 4-byte aligned
        end = o + h * w * 3
        want = imageio.emit_reference(batch[i, :, :h, :w].transpose(1, 2, 0))
        assert np.array_equal(packed[o:end].reshape(h, w, 3), want)
    assert packed.size == -(-end // 4) * 4
    assert packed[offs[1] + 2] == 0                                                         # the NaN of image 1


def test_image_desc_has_the_layout_the_header_documents(tmp_path):
    from edtr_amd import lib
    text = open(HEADER).read()
    doc = text[text.index("One edtr_image_desc per image"):text.index("typedef struct edtr_image_desc")]
    stated = {name: int(off) for off, name in re.findall(r"\b(\d+) ([a-z_]+)\b", doc.split("8-byte aligned):", 1)[1].split("The bits are", 1)[0])}
    fields = [n for n, _ in lib.ImageDesc._fields_]
    assert sorted(stated) == sorted(fields), (stated, fields)
    for name in fields:
        assert getattr(lib.ImageDesc, name).offset == stated[name], name
    assert "(80 bytes" in doc and ctypes.sizeof(lib.ImageDesc) == 80
    # and the C compiler agrees with both
    names = ",".join(f"offsetof(edtr_image_desc,{n})" for n in fields)
    src = tmp_path / "desc.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edtr_hip.h"\nint main(){size_t v[]={sizeof(edtr_image_desc),' + names +
                   '};for(unsigned i=0;i<sizeof v/sizeof*v;++i)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / "desc"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(lib.ImageDesc)
    assert out[1:] == [getattr(lib.ImageDesc, n).offset for n in fields]


def test_the_three_entry_points_are_declared_and_bound():
    from edtr_amd import lib, ops
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in BATCH_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in edtr_hip.h"
        assert name in lib.DECLARED_SYMBOLS
    handle = lib.load()                                                                     # (loads the built library: no GPU call)
    assert handle.edtr_abi_version() == 10
    for name, n_args in zip(BATCH_SYMBOLS, (7, 13, 11)):
        assert len(getattr(handle, name).argtypes) == n_args
    for rec in ("make_image_resize_h_batch", "make_image_resize_ingest_batch", "make_image_emit_batch"):
        assert callable(getattr(ops, rec))
    # the argument checks run before any HIP call
    assert handle.edtr_image_resize_h_batch(None, None, 1, 3, None, 0, None) == -1
    assert handle.edtr_image_resize_h_batch(None, None, 1, 4, None, 0, None) == -5
    assert handle.edtr_image_emit_batch(None, 1, 3, 8, 8, None, None, 1, None, 0, None) == -1


def test_bucket_ids_are_the_global_indices_and_the_other_modes_keep_theirs():
    from edtr_amd import imageio, rng
    from edtr_amd.parallel import shard_slice
    n = len(SIZES)
    for world in (1, 2, 3):
        seen = []
        for rank in range(world):
            sl = shard_slice(rank, world, n)
            plan = imageio.plan_buckets(SIZES[sl], 2, min_size=128, multiple=64)
            ids = rng.shard_bucket_ids(n, rank, world, plan)
            assert [len(c) for c in ids] == [len(idx) for _, idx in plan]
            for chunk, (hw, idx) in zip(ids, plan):
                assert chunk == [sl.start + k for k in idx]
                assert all(EXTENTS[g] == hw for g in chunk)                                 # id g really is image g of the data set
            seen += [g for c in ids for g in c]
        assert sorted(seen) == list(range(n)), world
    with pytest.raises(ValueError):
        rng.shard_bucket_ids(4, 0, 2, [((128, 128), [0, 2])])                               # rank 0 of 2 holds two images
    # the three existing modes answer what they answered before this mode existed (values written out, not recomputed)
    assert rng.shard_chunk_ids(7, 0, 1, 3, "batch") == [[0, 1, 2], [3, 4, 5], [6]]
    assert rng.shard_chunk_ids(7, 1, 2, 3, "batch") == [[4, 5, 6]] and rng.shard_chunk_ids(7, 0, 2, 3, "batch") == [[0, 1, 2], [3]]
    assert rng.shard_chunk_ids(7, 2, 3, 2, "batch") == [[5, 6]]
    for mode in ("demo", "seg"):
        assert rng.shard_chunk_ids(5, 0, 1, 4, mode) == [[0], [1], [2], [3], [4]]
        assert rng.shard_chunk_ids(5, 1, 2, 4, mode) == [[3], [4]]
    with pytest.raises(ValueError):
        rng.shard_chunk_ids(5, 0, 1, 4, "bucket")                                           # the plan-taking function is the one to ask


class _FakeCldm:
    unet = torch.nn.Linear(1, 1)


def test_restore_dataset_and_restore_files_know_the_new_arguments():
    import inspect
    from edtr_amd import evalutil, restore
    assert evalutil.restore_dataset(_FakeCldm(), None, None, [], pad_mode="bucket", seed=3, return_uint8=True) == ([], None)
    assert evalutil.restore_dataset(_FakeCldm(), None, None, [], pad_mode="bucket", batch_size=3) == ([], None)
    with pytest.raises(ValueError, match="pad_mode"):
        evalutil.restore_dataset(_FakeCldm(), None, None, [], pad_mode="buckets")
    assert "only a SEEDED run is independent of ``batch_size``" in evalutil.restore_dataset.__doc__
    sig = inspect.signature(restore.restore_files)
    assert sig.parameters["batch_size"].default == 1 and sig.parameters["workers"].default == 0
    with pytest.raises(ValueError):
        restore.restore_files(_FakeCldm(), None, None, [], "unused", batch_size=0)
    with pytest.raises(TypeError):
        restore.restore_files(_FakeCldm(), None, None, [], "unused", batch_size=2, pad_mode="seg")
    assert restore.MAX_WORKERS == 16 and "cpu_count" not in inspect.getsource(restore)


def test_restore_command_line_offers_batch_size_and_workers():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "edtr_amd.restore", "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--batch-size", "--workers", "--seed"):
        assert flag in r.stdout
