"""Host side of the seeded per-image noise (edtr_amd/rng.py): the Philox restatement against the published known answers, the
statistics and the value bound of the normal stream, the shard -> image-id bookkeeping of restore_dataset, NoiseSource's
validation and the sampler signatures.  No GPU."""
import inspect

import numpy as np
import pytest


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("ctr,key,expect", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, expect):
    """The three known-answer vectors of the Random123 distribution (philox4x32-10)."""
    from edtr_amd import rng
    assert _hex(rng.philox4x32_10(ctr, key)) == expect
    batched = rng.philox4x32_10(np.array([ctr, [1, 2, 3, 4]], dtype=np.uint32), np.array(key, dtype=np.uint32))   # broadcast key
    assert _hex(batched[0]) == expect and _hex(batched[1]) != expect


def _sample_1m():
    """seed 7, image ids 0..7, purpose 1, draws 0..7, per_image 16384: 8 x 8 x 16384 = 1 048 576 values"""
    from edtr_amd import rng
    return np.stack([rng.normal_reference(7, range(8), rng.PURPOSE_STEP, d, 16384) for d in range(8)])


def test_normal_reference_statistics_and_bound():
    """4.5-sigma gates on mean / variance / kurtosis of 2^20 values (standard errors 1/sqrt(N), sqrt(2/N), sqrt(24/N) of a
    normal sample), every value finite and inside the stream's hard bound sqrt(48 ln 2)."""
    from edtr_amd import rng
    z = _sample_1m().reshape(-1)
    N = z.size
    assert N == 1 << 20
    assert np.isfinite(z).all()
    assert float(np.abs(z).max()) <= 5.77 and float(np.abs(z).max()) <= rng.Z_MAX
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    g = (abs(mean) * np.sqrt(N), abs(var - 1.0) * np.sqrt(N / 2.0), abs(kurt - 3.0) * np.sqrt(N / 24.0))
    print(f"\n[normal_reference] |mean| sqrt(N) {g[0]:.2f}, |var-1| sqrt(N/2) {g[1]:.2f}, |kurt-3| sqrt(N/24) {g[2]:.2f}, "
          f"max |z| {np.abs(z).max():.2f}")
    assert max(g) < 4.5, g


def test_normal_reference_streams_are_uncorrelated():
    """corrcoef * sqrt(n) (a unit normal for independent streams) between neighbouring images, draws, seeds, and the stream
    against itself shifted by 1 and by 4 elements (inside / across a Philox call): each below 4.5 in magnitude."""
    from edtr_amd import rng
    n = 16384

    def stream(seed, image, draw):
        return rng.normal_reference(seed, [image], rng.PURPOSE_STEP, draw, n)[0]

    base = stream(1234, 0, 0)
    pairs = {"image 0 / 1": (base, stream(1234, 1, 0)), "draw 0 / 1": (base, stream(1234, 0, 1)),
             "seed 1234 / 1235": (base, stream(1235, 0, 0)), "shift 1": (base[:-1], base[1:]), "shift 4": (base[:-4], base[4:])}
    for name, (a, b) in pairs.items():
        c = float(np.corrcoef(a, b)[0, 1] * np.sqrt(a.size))
        print(f"[normal_reference] {name}: {c:+.2f}")
        assert abs(c) < 4.5, (name, c)
    # and every coordinate of the counter matters: purposes differ too, same arguments give the same values
    assert not np.array_equal(base, rng.normal_reference(1234, [0], rng.PURPOSE_Q_SAMPLE, 0, n)[0])
    assert np.array_equal(base, stream(1234, 0, 0))


def test_normal_reference_is_per_image_and_per_group():
    """An image's row depends on its id alone (not on its position or its neighbours); element e comes from counter word e >> 2, so
    a shorter image is a prefix of a longer one; a per-image draw list equals the per-draw calls."""
    from edtr_amd import rng
    full = rng.normal_reference(99, [3, 17, 9, 0, 2], rng.PURPOSE_X_T, 0, 256)
    assert np.array_equal(full[1], rng.normal_reference(99, [17], rng.PURPOSE_X_T, 0, 256)[0])
    assert np.array_equal(full[:, :64], rng.normal_reference(99, [3, 17, 9, 0, 2], rng.PURPOSE_X_T, 0, 64))
    per = rng.normal_reference(5, [4, 4], rng.PURPOSE_STEP, [0, 49], 64)
    assert np.array_equal(per[0], rng.normal_reference(5, [4], rng.PURPOSE_STEP, 0, 64)[0])
    assert np.array_equal(per[1], rng.normal_reference(5, [4], rng.PURPOSE_STEP, 49, 64)[0])
    with pytest.raises(ValueError):
        rng.normal_reference(5, [0], rng.PURPOSE_STEP, 0, 6)
    with pytest.raises(ValueError):
        rng.normal_reference(5, [0], 4, 0, 8)


@pytest.mark.parametrize("n_images", [0, 1, 7, 64])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("batch_size", [1, 3, 8])
def test_shard_chunk_ids_cover_the_data_set_once(n_images, world, batch_size):
    """The ids handed to the ranks' chunks are each of 0..N-1 exactly once, image k gets id k (the chunks follow restore_dataset's
    own slicing of `pre_restored`), and no chunk is larger than the batch size."""
    from edtr_amd import rng
    from edtr_amd.parallel import shard_slice
    data = list(range(n_images))
    seen = []
    for pad_mode in ("batch", "demo"):
        seen = []
        for rank in range(world):
            chunks = rng.shard_chunk_ids(n_images, rank, world, batch_size, pad_mode)
            mine = data[shard_slice(rank, world, n_images)]
            step = 1 if pad_mode == "demo" else batch_size
            assert chunks == [mine[i:i + step] for i in range(0, len(mine), step)]      # image k carries id k
            assert all(0 < len(c) <= step for c in chunks)
            seen += [i for c in chunks for i in c]
        assert sorted(seen) == data


def test_noise_source_validation():
    from edtr_amd import rng
    src = rng.NoiseSource(11, [5, 0, 4_000_000_000])
    assert src.seed == 11 and src.image_ids == (5, 0, 4_000_000_000) and len(src) == 3
    assert src.check_batch(3) is src
    with pytest.raises(ValueError):
        src.check_batch(2)
    for bad in ([-1], [1 << 32], [0, 1 << 40]):
        with pytest.raises(ValueError):
            rng.NoiseSource(11, bad)
    with pytest.raises(ValueError):
        rng.NoiseSource(-1, [0])
    with pytest.raises(ValueError):
        rng.NoiseSource(1 << 64, [0])
    with pytest.raises(ValueError):
        rng.NoiseSource(0, [])
    with pytest.raises(AttributeError):
        src.seed = 12
    import torch
    assert rng.NoiseSource(3, torch.tensor([7, 8], dtype=torch.int64)).image_ids == (7, 8)
    assert rng.NoiseSource.for_shard(3, 10, 4).image_ids == (10, 11, 12, 13)
    assert np.array_equal(src.reference(rng.PURPOSE_STEP, 2, 16), rng.normal_reference(11, [5, 0, 4_000_000_000], 1, 2, 16))


def test_sampler_signatures_keep_the_reference_order_and_end_with_noise_source():
    """The reference's positional order is intact and the one new keyword is the LAST parameter, default None."""
    from edtr_amd.evalutil import restore_dataset
    from edtr_amd.model.cldm import ControlLDM
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.workloads import restore_pass
    expect = {
        SpacedSampler.p_sample: ["self", "model", "x", "t", "index", "cond", "uncond", "cfg_scale"],
        SpacedSampler.sample: ["self", "model", "device", "steps", "batch_size", "x_size", "cond", "uncond", "cfg_scale", "tiled",
                               "tile_size", "tile_stride", "x_T", "progress", "progress_leave", "return_intermediates"],
        SpacedSampler.manual_sample_with_timesteps: ["self", "model", "device", "x_T", "steps", "used_timesteps", "batch_size", "cond",
                                                     "uncond", "cfg_scale", "tiled", "tile_size", "tile_stride", "progress",
                                                     "progress_leave", "return_intermediates"],
        ControlLDM.vae_encode: ["self", "image", "sample", "tiled", "tile_size"],
    }
    for fn, names in expect.items():
        fn = inspect.unwrap(fn)
        params = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in params] == names + ["noise_source"], fn.__qualname__
        assert params[-1].default is None
    assert list(inspect.signature(restore_pass).parameters)[-1] == "noise_source"
    seed = list(inspect.signature(inspect.unwrap(restore_dataset)).parameters.values())[-1]
    assert seed.name == "seed" and seed.default is None
