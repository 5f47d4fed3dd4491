"""Latent tiling of a model forward with Gaussian-weighted overlap-add: host-side mirror of reference
utils/common.py `sliding_windows` (:351-364), `gaussian_weights` (:151-165) and `make_tiled_fn` (:367-427), with the
accumulate / normalise steps as libedtr_hip launches (edtr_tile_accumulate, edtr_divide).  Where the windows are evaluated stacked on
the batch axis, they are cut by ONE launch (edtr_tile_gather) and blended by ONE launch (edtr_tile_blend) from a window table:
int32 [n, 2], row k = (hi, wi) of window k in `sliding_windows` order, kept as a host array (checked by the entry points) and as a
device tensor (read by the kernels).  `gather_reference` / `blend_reference` restate the two launches in numpy."""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops


def sliding_windows(h: int, w: int, tile_size: int, tile_stride: int) -> List[Tuple[int, int, int, int]]:
    def starts(n: int) -> List[int]:
        s = list(range(0, n - tile_size + 1, tile_stride))
        if (n - tile_size) % tile_stride != 0:
            s.append(n - tile_size)     # last window snapped to the edge
        return s
    return [(hi, hi + tile_size, wi, wi + tile_size) for hi in starts(h) for wi in starts(w)]


def gaussian_weights(tile_width: int, tile_height: int) -> np.ndarray:
    """var = 0.01; the x midpoint is (w-1)/2 while the y midpoint is h/2 — kept as in the reference."""
    var = 0.01
    xs, ys = np.arange(tile_width, dtype=np.float64), np.arange(tile_height, dtype=np.float64)
    norm = np.sqrt(2 * np.pi * var)
    xp = np.exp(-(xs - (tile_width - 1) / 2) ** 2 / (tile_width * tile_width) / (2 * var)) / norm
    yp = np.exp(-(ys - tile_height / 2) ** 2 / (tile_height * tile_height) / (2 * var)) / norm
    return np.outer(yp, xp)


def window_table(windows: Sequence[Tuple[int, int, int, int]]) -> np.ndarray:
    """int32 [n, 2]: (hi, wi) of every (hi, hi_end, wi, wi_end) window, in the order given."""
    return np.array([(hi, wi) for hi, _, wi, _ in windows], dtype=np.int32).reshape(-1, 2)


def table_covers(table: np.ndarray, th: int, tw: int, H: int, W: int) -> bool:
    """Every window lies inside the H x W plane and every pixel of the plane lies in a window: what edtr_tile_blend checks on the
    host copy of the table before it launches."""
    table = np.asarray(table).reshape(-1, 2)
    cover = np.zeros((H, W), dtype=bool)
    for hi, wi in table:
        if hi < 0 or wi < 0 or hi + th > H or wi + tw > W:
            return False
        cover[hi:hi + th, wi:wi + tw] = True
    return bool(len(table)) and bool(cover.all())


def gather_reference(x: np.ndarray, table: np.ndarray, th: int, tw: int) -> np.ndarray:
    """edtr_tile_gather: [n B, C, th, tw], entry k B + b = window k of image b (the concatenation of the window slices)."""
    return np.concatenate([x[..., hi:hi + th, wi:wi + tw] for hi, wi in np.asarray(table).reshape(-1, 2)], axis=0)


def blend_reference(tiles: np.ndarray, wts: np.ndarray, table: np.ndarray, B: int, H: int, W: int) -> np.ndarray:
    """edtr_tile_blend in fp64: the weighted tiles added window by window in table order, divided by the added weights
    (reference utils/common.py:415-425).  ``tiles`` [n B, C, th, tw] window-major, ``wts`` [th, tw]; returns fp64 [B, C, H, W]."""
    tiles, wts = np.asarray(tiles, dtype=np.float64), np.asarray(wts, dtype=np.float64)
    th, tw = wts.shape
    out = np.zeros((B, tiles.shape[1], H, W), dtype=np.float64)
    count = np.zeros_like(out)
    for k, (hi, wi) in enumerate(np.asarray(table).reshape(-1, 2)):
        out[..., hi:hi + th, wi:wi + tw] += tiles[k * B:(k + 1) * B] * wts
        count[..., hi:hi + th, wi:wi + tw] += wts
    return out / count


class DeviceWindows:
    """The windows of one (h, w, size, stride) on one device: the list, the table's host and device copies, window -> position."""

    def __init__(self, h: int, w: int, size: int, stride: int, device) -> None:
        self.windows = sliding_windows(h, w, size, stride)
        table = window_table(self.windows)
        self.n = len(self.windows)
        self.host = (ctypes.c_int32 * (2 * self.n))(*table.reshape(-1).tolist())
        self.device = torch.from_numpy(table).to(device).contiguous()
        self.index = {win: k for k, win in enumerate(self.windows)}


_DEVICE_WINDOWS: Dict[tuple, DeviceWindows] = {}
_DEVICE_WEIGHTS: Dict[tuple, torch.Tensor] = {}


def device_windows(h: int, w: int, size: int, stride: int, device) -> DeviceWindows:
    """Built once per (h, w, size, stride, device): a denoise step re-uses the table of the step before."""
    key = (h, w, size, stride, str(device))
    hit = _DEVICE_WINDOWS.get(key)
    if hit is None:
        hit = _DEVICE_WINDOWS[key] = DeviceWindows(h, w, size, stride, device)
    return hit


def _device_weights(size: int, weight: str, device) -> torch.Tensor:
    key = (size, weight == "gaussian", str(device))
    hit = _DEVICE_WEIGHTS.get(key)
    if hit is None:
        wts_np = gaussian_weights(size, size) if weight == "gaussian" else np.ones((size, size))
        hit = _DEVICE_WEIGHTS[key] = torch.tensor(wts_np, dtype=torch.float32, device=device).contiguous()
    return hit


def gather_windows(x: torch.Tensor, tab: DeviceWindows, size: int) -> torch.Tensor:
    """fp32 [n B, C, size, size]: every window of ``x`` [B, C, H, W], window-major, by one edtr_tile_gather launch."""
    x = x.contiguous().float()
    out = torch.empty((tab.n * x.shape[0], x.shape[1], size, size), dtype=torch.float32, device=x.device)
    ops.launch(ops.make_tile_gather(src=x, table_host=tab.host, table=tab.device, th=size, tw=size, dst=out))
    return out


def make_tiled_fn(fn: Callable, size: int, stride: int, weight: str = "gaussian", batched_fn: Callable = None,
                  max_batch: int = 16) -> Callable:
    """Only the first argument (the latent, fp32 NCHW) is split; `fn` receives the tile plus hi/hi_end/wi/wi_end
    keyword arguments when it has extra arguments (reference utils/common.py:413-414).

    MI355X addition: all windows have the same size, and the wrapped network treats batch entries independently, so
    when ``batched_fn(x_tiles, windows, *args, **kwargs)`` is given the windows are evaluated in groups stacked on the
    batch axis (<= max_batch entries per call) instead of one forward per window — the same numbers, several times the
    work per launch (9 windows of a 1024x1024 image become one batch-9 forward per denoise step).  That branch cuts all windows
    with one edtr_tile_gather, collects the groups' outputs in one stacked buffer and blends them with one edtr_tile_blend: the
    bits of the per-window accumulate launches in window order followed by the divide."""

    def tiled_batched(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        b, _, h, w = x.shape
        tab = device_windows(h, w, size, stride, x.device)
        xs = gather_windows(x, tab, size)
        per_call = max(1, max_batch // b)
        ys = None
        for g0 in range(0, tab.n, per_call):
            group = tab.windows[g0:g0 + per_call]
            y = batched_fn(xs[g0 * b:(g0 + len(group)) * b], group, *args, **kwargs)
            if len(group) == tab.n:             # one group: its output is the stacked buffer
                ys = y.contiguous().float()
                break
            if ys is None:
                ys = torch.empty((tab.n * b,) + tuple(y.shape[1:]), dtype=torch.float32, device=x.device)
            ys[g0 * b:(g0 + len(group)) * b].copy_(y)
        res = torch.empty((b, ys.shape[1], h, w), dtype=torch.float32, device=x.device)
        ops.launch(ops.make_tile_blend(tiles=ys, wts=_device_weights(size, weight, x.device), table_host=tab.host, table=tab.device,
                                       th=size, tw=size, out=res))
        return res

    def tiled_fn(x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        b, c, h, w = x.shape
        if batched_fn is not None and len(sliding_windows(h, w, size, stride)) > 1:
            return tiled_batched(x, *args, **kwargs)
        out = torch.zeros((b, c, h, w), dtype=torch.float32, device=x.device)
        count = torch.zeros_like(out)
        wts_np = gaussian_weights(size, size) if weight == "gaussian" else np.ones((size, size))
        wts = torch.tensor(wts_np, dtype=torch.float32, device=x.device).contiguous()
        windows = sliding_windows(h, w, size, stride)

        def accumulate(y: torch.Tensor, hi: int, wi: int) -> None:
            ops.launch(ops.make_tile_accumulate(tile=y.contiguous().float(), wts=wts, out=out, count=count, B=b, C=c, H=h,
                                                W=w, th=size, tw=size, hi=hi, wi=wi))

        for hi, hi_end, wi, wi_end in windows:
            x_tile = x[..., hi:hi_end, wi:wi_end]
            if len(args) or len(kwargs):
                kwargs.update(dict(hi=hi, hi_end=hi_end, wi=wi, wi_end=wi_end))
            accumulate(fn(x_tile, *args, **kwargs), hi, wi)
        res = torch.empty_like(out)
        ops.launch(ops.make_divide(num=out, den=count, out=res, n=out.numel()))
        return res

    return tiled_fn
