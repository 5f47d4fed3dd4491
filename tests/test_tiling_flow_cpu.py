"""Host-side checks of the tiled flow (no GPU): the window table and its coverage rule, the numpy restatements of edtr_tile_gather /
edtr_tile_blend, `evalutil.TilingOptions` (defaults, units, tile-or-not rules at the boundary sizes), the command line's ten flags,
`restore_files`' keyword check, and the two new C-ABI symbols — whose argument checks run on the host table before anything is
launched, so they are exercised here with pointers that are never dereferenced."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from edtr_amd import evalutil, lib, restore, tiling
from edtr_amd.evalutil import TilingOptions

CASES = [(21, 30, 8, 4), (24, 32, 8, 4)]
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
FAKE = 0x10000          # a 16-byte aligned non-NULL address: the calls below are all refused before a launch could read it


def _host(table):
    return (C.c_int32 * table.size)(*table.reshape(-1).tolist())


@pytest.mark.parametrize("h,w,size,stride", CASES)
def test_window_table_order_and_coverage(h, w, size, stride):
    wins = tiling.sliding_windows(h, w, size, stride)
    table = tiling.window_table(wins)
    assert table.dtype == np.int32 and table.shape == (len(wins), 2)
    assert [tuple(r) for r in table.tolist()] == [(hi, wi) for hi, _, wi, _ in wins]
    assert table.tolist() == sorted(table.tolist())                    # row-major: hi outer, wi inner
    assert table[-1].tolist() == [h - size, w - size]                  # the last window is snapped to the edge
    assert tiling.table_covers(table, size, size, h, w)
    for drop in (0, len(wins) - 1):                                     # a corner pixel lies in exactly one window
        assert not tiling.table_covers(np.delete(table, drop, axis=0), size, size, h, w)
    assert tiling.table_covers(np.delete(table, len(wins) // 2, axis=0), size, size, h, w)      # an inner window's pixels stay covered
    outside = table.copy()
    outside[1, 1] = w - size + 1
    assert not tiling.table_covers(outside, size, size, h, w)


@pytest.mark.parametrize("h,w,size,stride", CASES)
def test_entry_points_refuse_on_the_host(h, w, size, stride):
    L = lib.load()
    table = tiling.window_table(tiling.sliding_windows(h, w, size, stride))
    n = len(table)

    def blend(t, tiles=FAKE, wts=FAKE, dev=FAKE, out=FAKE, cnt=None):
        return L.edtr_tile_blend(tiles, wts, _host(t), dev, len(t) if cnt is None else cnt, size, size, out, 2, 5, h, w, None)

    def gather(t, src=FAKE, dev=FAKE, dst=FAKE, cnt=None):
        return L.edtr_tile_gather(src, 2, 5, h, w, _host(t), dev, len(t) if cnt is None else cnt, size, size, dst, None)

    for drop in (0, n - 1):
        assert blend(np.delete(table, drop, axis=0)) == E_SHAPE         # an uncovered pixel
    outside = table.copy()
    outside[n - 1, 0] += 1
    assert blend(outside) == E_SHAPE and gather(outside) == E_SHAPE
    negative = table.copy()
    negative[0, 1] = -1
    assert blend(negative) == E_SHAPE and gather(negative) == E_SHAPE
    assert blend(table, cnt=0) == E_SHAPE and gather(table, cnt=-1) == E_SHAPE
    assert blend(table, cnt=lib.TILE_WINDOWS_MAX + 1) == E_SHAPE
    assert blend(table, tiles=None) == E_NULL and blend(table, out=None) == E_NULL and blend(table, dev=None) == E_NULL
    assert gather(table, src=None) == E_NULL and gather(table, dst=None) == E_NULL
    assert blend(table, wts=FAKE + 2) == E_ALIGN and gather(table, dst=FAKE + 1) == E_ALIGN and gather(table, dev=FAKE + 2) == E_ALIGN


def test_abi_is_additive():
    L = lib.load()
    assert L.edtr_abi_version() == 10
    for name in ("edtr_tile_gather", "edtr_tile_blend"):
        assert name in lib.DECLARED_SYMBOLS and getattr(L, name).argtypes is not None
    assert {"edtr_tile_accumulate", "edtr_divide"} <= set(lib.DECLARED_SYMBOLS)          # the per-window forms stay entry points


@pytest.mark.parametrize("h,w,size,stride", CASES)
@pytest.mark.parametrize("weight", ["gaussian", "uniform"])
def test_restatements(h, w, size, stride, weight):
    """`gather_reference` is slicing + concatenation; `blend_reference` is the reference's make_tiled_fn arithmetic
    (utils/common.py:415-425: preds[window] += tile * weights, count[window] += weights, preds / count) in fp64."""
    rng = np.random.default_rng(5)
    B, Cn = 2, 3
    wins = tiling.sliding_windows(h, w, size, stride)
    table = tiling.window_table(wins)
    x = rng.standard_normal((B, Cn, h, w)).astype(np.float32)
    got = tiling.gather_reference(x, table, size, size)
    assert got.shape == (len(wins) * B, Cn, size, size) and got.dtype == np.float32
    for k, (hi, he, wi, we) in enumerate(wins):
        assert np.array_equal(got[k * B:(k + 1) * B], x[:, :, hi:he, wi:we])
    wts = tiling.gaussian_weights(size, size) if weight == "gaussian" else np.ones((size, size))
    tiles = rng.standard_normal((len(wins) * B, Cn, size, size)).astype(np.float32)
    preds, count = np.zeros((B, Cn, h, w)), np.zeros((B, Cn, h, w))
    for k, (hi, he, wi, we) in enumerate(wins):
        preds[:, :, hi:he, wi:we] += tiles[k * B:(k + 1) * B].astype(np.float64) * wts
        count[:, :, hi:he, wi:we] += wts
    ref = tiling.blend_reference(tiles, wts, table, B, h, w)
    assert ref.dtype == np.float64 and np.array_equal(ref, preds / count)
    # blending the windows of a plane gives the plane back (a weighted mean of equal values), whatever the weights
    back = tiling.blend_reference(got, wts, table, B, h, w)
    assert np.allclose(back, x, rtol=1e-12, atol=1e-12)


def test_tiling_options_defaults_and_units():
    opt = TilingOptions()
    assert dataclasses.asdict(opt) == dict(pre_res=False, pre_res_size=512, pre_res_stride=256, vae_encoder=False, vae_encoder_size=256,
                                           vae_decoder=False, vae_decoder_size=256, cldm=False, cldm_size=512, cldm_stride=256)
    with pytest.raises(dataclasses.FrozenInstanceError):
        opt.cldm = True
    on = TilingOptions(pre_res=True, vae_encoder=True, vae_decoder=True, cldm=True)
    assert on.sampler_kwargs(128, 128) == dict(tiled=True, tile_size=64, tile_stride=32)           # cldm sizes // 8
    assert on.encoder_kwargs() == dict(tiled=True, tile_size=256) and on.decoder_kwargs() == dict(tiled=True, tile_size=256)   # as they are
    assert opt.encoder_kwargs()["tiled"] is False and opt.decoder_kwargs()["tiled"] is False
    tiny = TilingOptions(cldm=True, cldm_size=128, cldm_stride=64)
    assert tiny.sampler_kwargs(24, 32) == dict(tiled=True, tile_size=16, tile_stride=8)


def test_tile_or_not_at_the_boundary_sizes():
    on = TilingOptions(pre_res=True, cldm=True)
    size = on.pre_res_size
    # SwinIR: tiled as soon as a window fits on both axes
    assert on.pre_res_tiled(size, size) and on.pre_res_tiled(size + 1, 4 * size) and on.pre_res_tiled(size, size + 1)
    assert not on.pre_res_tiled(size - 1, size) and not on.pre_res_tiled(4 * size, size - 1)
    assert not TilingOptions().pre_res_tiled(4 * size, 4 * size)
    # sampler: untiled when the latent is not larger than the tile on BOTH axes (h1 <= size // 8 or w1 <= size // 8)
    tile = on.cldm_size // 8
    assert on.cldm_tiled(tile + 1, tile + 1) and on.cldm_tiled(tile + 1, 3 * tile)
    assert not on.cldm_tiled(tile, tile + 1) and not on.cldm_tiled(tile + 1, tile) and not on.cldm_tiled(tile - 1, 3 * tile)
    assert not on.cldm_tiled(tile, tile)
    assert on.sampler_kwargs(tile, tile + 1)["tiled"] is False
    assert not TilingOptions().cldm_tiled(3 * tile, 3 * tile)


def test_command_line_takes_the_ten_flags():
    ap = restore.build_parser()
    base = ["--input", "a", "--output", "b", "--config", "tiny"]
    args = ap.parse_args(base)
    assert restore.tiling_from_args(args) is None                       # no switch: the untiled flow, as before
    for flag in ("pre_res_tiled", "vae_encoder_tiled", "vae_decoder_tiled", "cldm_tiled"):
        assert getattr(args, flag) is False
    assert (args.pre_res_tile_size, args.pre_res_tile_stride, args.vae_encoder_tile_size, args.vae_decoder_tile_size,
            args.cldm_tile_size, args.cldm_tile_stride) == (512, 256, 256, 256, 512, 256)
    assert restore.tiling_from_args(ap.parse_args(base + ["--cldm-tiled"])) == TilingOptions(cldm=True)
    args = ap.parse_args(base + ["--pre-res-tiled", "--pre-res-tile-size", "128", "--pre-res-tile-stride", "64", "--vae-encoder-tiled",
                                 "--vae-encoder-tile-size", "64", "--vae-decoder-tiled", "--vae-decoder-tile-size", "8", "--cldm-tiled",
                                 "--cldm-tile-size", "128", "--cldm-tile-stride", "64"])
    assert restore.tiling_from_args(args) == TilingOptions(True, 128, 64, True, 64, True, 8, True, 128, 64)


def test_restore_files_keywords():
    assert "tiling" in restore._BATCHED_KEYWORDS
    with pytest.raises(TypeError, match="bogus"):                       # refused before anything is touched, as today
        restore.restore_files(None, None, None, [], "unused", batch_size=2, bogus=1, tiling=TilingOptions())
    import inspect
    for fn in (evalutil.restore_batch, evalutil.restore_dataset, restore._restore_files_batched):
        assert inspect.signature(fn).parameters["tiling"].default is None
    assert inspect.signature(evalutil.restore_dataset).parameters["tiling"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(evalutil.restore_dataset).parameters)[-1] == "seed"
