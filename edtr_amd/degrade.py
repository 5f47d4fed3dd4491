"""Low-quality inputs from high-quality ones, on the device: the blur -> resize -> noise -> JPEG chain that the reference applies on the
CPU before every evaluation.  One stage of it (`degrade_batch`: datasets/detection_cocov2.py:426-460; with a final resize back to the
input extent, the CodeFormer-style chain of datasets/detection.py:155-181) is four launches of include/edtr_hip.h "Low-quality inputs"
(five with the resize back); the whole second-order Real-ESRGAN chain (`degrade_batch2`: RealESRGANBatchTransform.__call__, :413-539 —
USM sharpening, two stages with Gaussian or Poisson noise, the final sinc filter, the resize back) adds the launches of "Low-quality
inputs, second order".  All on the fp32 NCHW batches that `imageio.ingest` writes.

    python -m edtr_amd.degrade --input DIR --output DIR --config YAML|codeformer|realesrgan-stage1|realesrgan --seed N [--batch-size N --workers N]

writes ``gt/<stem>.png`` and ``lq/<stem>.png`` under the output folder, as the reference's generators do (``gt/`` is the sharpened
image where the configuration sharpens, as the reference's GT is).  ``--geometry YAML [--masks DIR]`` first applies the resize, pad,
crop and flip of the reference's segmentation data sets to image and mask together (edtr_amd/labels.py) and adds ``mask/<stem>.png``.

Three layers:
  * `filter2d`, `resize`, `add_gaussian_noise`, `jpeg`, `add_poisson_noise`, `sepblur`, `usm_sharpen`: thin wrappers over the launches
    (torch tensors on the device);
  * `*_reference`: the numpy restatement of each, operation for operation in fp32.  They are the NORMATIVE definition: the kernels are
    tested against them by equality, and they against the reference's own functions within its fp32 error (tests/golden/degrade.npz,
    tests/golden/degrade2.npz);
  * host-side parameter synthesis in numpy: the isotropic / anisotropic Gaussian, generalized Gaussian and plateau blur kernels and
    their mixture draw (our restatement of datasets/degradation.py:17-387), the sinc kernel (`circular_lowpass_kernel`, with a Bessel J1
    of its own), the Poisson inversion tables (`poisson_table`), `DegradeConfig` / `RealESRGANConfig` with the reference's YAML keys,
    and `draw_params` / `draw_params2`, which draw one image's parameters from ``numpy.random.default_rng([seed, image_id])``.
    An image's low-quality version therefore depends on its bytes, the seed and its data-set index alone — not on the batch it
    travels in, the order, or the number of ranks: the promise `rng.NoiseSource` makes for the sampler's noise.

Poisson noise is not torch.poisson (which has no stream that could be restated) but table inversion on the seeded Philox stream:
integer-only and loop-free, so kernel and numpy agree by construction.  Left out: the training pair pool (`queue_size` > 0), which
mixes images across batches and would break that promise."""
from __future__ import annotations

import argparse
import math
import os
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .rng import (PURPOSE_DEGRADE, PURPOSE_DEGRADE_GRAY, PURPOSE_DEGRADE_POISSON, PURPOSE_DEGRADE_POISSON_GRAY, stream_reference,
                  uniform_words_reference)

F32 = np.float32
MODES = ("bilinear", "bicubic", "area")                  # EDTR_RESIZE_BILINEAR / _BICUBIC / _AREA, in that order
K_MIN, K_MAX = 3, 41

# the standard JPEG tables as datasets/diffjpeg.py holds them: the luminance table TRANSPOSED, the chrominance table as is
Y_TABLE = np.array(
    [[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
     [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
     [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=F32).T.copy()
C_TABLE = np.full((8, 8), 99, dtype=F32)
C_TABLE[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=F32).T
RGB2YCC = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], dtype=F32)
YCC2RGB = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=F32)
_ALPHA = np.array([1.0 / np.sqrt(2)] + [1.0] * 7)
DCT_SCALE = (np.outer(_ALPHA, _ALPHA) * 0.25).astype(F32)       # [u][v]
DCT_ALPHA = np.outer(_ALPHA, _ALPHA).astype(F32)


def dct_table() -> np.ndarray:
    """fp32 [64][64]: T[x*8 + y][u*8 + v] = float32(cos((2x+1) u pi/16) * cos((2y+1) v pi/16)), the product formed in fp64 —
    DCT8x8's tensor; iDCT8x8's is its transpose."""
    i = np.arange(8)
    c = np.cos((2 * i[:, None] + 1) * i[None, :] * np.pi / 16)          # [x][u]
    return (c[:, None, :, None] * c[None, :, None, :]).astype(F32).reshape(64, 64)


def quality_to_factor(quality) -> np.ndarray:
    """diffjpeg.quality_to_factor on fp32 values, every step rounded to fp32 (as on the reference's 0-dim fp32 tensors)."""
    q = np.atleast_1d(np.asarray(quality, dtype=F32))
    if ((q <= 0) | (q > 100)).any() or np.isnan(q).any():
        raise ValueError(f"JPEG quality must be in (0, 100], got {q.tolist()}")
    with np.errstate(divide="ignore"):
        return np.where(q < 50, (F32(5000.0) / q) / F32(100.0), (F32(200.0) - q * F32(2.0)) / F32(100.0)).astype(F32)


def _batch(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=F32)
    if x.ndim != 4 or x.shape[1] != 3:
        raise ValueError(f"expected a [B, 3, H, W] batch, got {x.shape}")
    return x


# ----------------------------------------------------------------------------------------------------------------------------------
# numpy restatements (normative)
# ----------------------------------------------------------------------------------------------------------------------------------
def _check_kernels(kernels, B: int, H: int, W: int) -> np.ndarray:
    k = np.ascontiguousarray(kernels, dtype=F32)
    if k.ndim == 2:
        k = k[None]
    if k.ndim != 3 or k.shape[1] != k.shape[2]:
        raise ValueError(f"kernels must be [n, k, k], got {k.shape}")
    ks = k.shape[1]
    if ks % 2 == 0 or not K_MIN <= ks <= K_MAX:
        raise ValueError(f"kernel size must be odd and in [{K_MIN}, {K_MAX}], got {ks}")
    if ks // 2 >= min(H, W):
        raise ValueError(f"a {ks} x {ks} kernel needs reflect padding of {ks // 2}, more than a {H} x {W} image allows")
    if k.shape[0] not in (1, B):
        raise ValueError(f"{k.shape[0]} kernels for a batch of {B}")
    return k


def filter2d_reference(x, kernels) -> np.ndarray:
    """filter2D: correlation over reflect-padded borders; acc = acc + p * w per tap, ky major, from 0, each step rounded to fp32."""
    x = _batch(x)
    B, _, H, W = x.shape
    k = _check_kernels(kernels, B, H, W)
    ks = k.shape[1]
    r = ks // 2
    pad = np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)), mode="reflect")
    acc = np.zeros_like(x)
    for ky in range(ks):
        for kx in range(ks):
            w = k[:, ky, kx].reshape(-1, 1, 1, 1)
            acc = acc + pad[:, :, ky:ky + H, kx:kx + W] * w
    return acc


def _source_index(n_in: int, n_out: int) -> np.ndarray:
    scale = F32(n_in) / F32(n_out)
    return (scale * (np.arange(n_out, dtype=F32) + F32(0.5))) - F32(0.5)


def _index_lambda(src: np.ndarray, n: int):
    idx = np.minimum(np.floor(src).astype(np.int64), n - 1)
    return idx, np.clip(src - idx.astype(F32), F32(0), F32(1)).astype(F32)


def _cubic1(v):
    return (((F32(1.25) * v - F32(2.25)) * v) * v + F32(1.0)).astype(F32)


def _cubic2(v):
    return ((((F32(-0.75) * v + F32(3.75)) * v - F32(6.0)) * v) + F32(3.0)).astype(F32)


def _cubic_weights(t):
    u = F32(1.0) - t
    return [_cubic2(t + F32(1.0)), _cubic1(t), _cubic1(u), _cubic2(u + F32(1.0))]


def _check_size(size) -> Tuple[int, int]:
    oh, ow = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if oh <= 0 or ow <= 0:
        raise ValueError(f"output size must be positive, got {oh} x {ow}")
    return oh, ow


def bilinear_planes_reference(x: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """The bilinear branch of `resize_reference` on fp32 [B, C, ih, iw] with any number of planes (`labels.upsample_logits_reference`
    blends logit planes with it): the source index clamped at 0, `_index_lambda`, columns blended first, every step rounded."""
    ih, iw = x.shape[2:]
    y0, ty = _index_lambda(np.maximum(_source_index(ih, oh), F32(0)), ih)
    x0, tx = _index_lambda(np.maximum(_source_index(iw, ow), F32(0)), iw)
    y1, x1 = y0 + (y0 < ih - 1), x0 + (x0 < iw - 1)
    wy0, wx0 = (F32(1) - ty)[:, None], F32(1) - tx
    ty = ty[:, None]
    top = wx0 * x[:, :, y0][:, :, :, x0] + tx * x[:, :, y0][:, :, :, x1]
    bot = wx0 * x[:, :, y1][:, :, :, x0] + tx * x[:, :, y1][:, :, :, x1]
    return (wy0 * top + ty * bot).astype(F32)


def resize_reference(x, size, mode: str) -> np.ndarray:
    """F.interpolate(x, size=size, mode=mode) (align_corners=False, no antialias) with edtr_hip.h's operation order."""
    x = _batch(x)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    ih, iw = x.shape[2:]
    oh, ow = _check_size(size)
    if mode == "area":
        ys, ye = (np.arange(oh) * ih) // oh, ((np.arange(oh) + 1) * ih + oh - 1) // oh
        xs, xe = (np.arange(ow) * iw) // ow, ((np.arange(ow) + 1) * iw + ow - 1) // ow
        out = np.empty(x.shape[:2] + (oh, ow), dtype=F32)
        for i in range(oh):
            for j in range(ow):
                s = np.zeros(x.shape[:2], dtype=F32)
                for yy in range(ys[i], ye[i]):
                    for xx in range(xs[j], xe[j]):
                        s = s + x[:, :, yy, xx]
                out[:, :, i, j] = s / F32((ye[i] - ys[i]) * (xe[j] - xs[j]))
        return out
    if mode == "bilinear":
        return bilinear_planes_reference(x, oh, ow)
    sy, sx = _source_index(ih, oh), _source_index(iw, ow)
    y0, ty = _index_lambda(sy, ih)
    x0, tx = _index_lambda(sx, iw)
    wy, wx = _cubic_weights(ty), _cubic_weights(tx)
    cols = [np.clip(x0 - 1 + j, 0, iw - 1) for j in range(4)]
    out = None
    for i in range(4):
        rows = x[:, :, np.clip(y0 - 1 + i, 0, ih - 1)]
        s = wx[0] * rows[:, :, :, cols[0]]
        for j in range(1, 4):
            s = s + wx[j] * rows[:, :, :, cols[j]]
        term = wy[i][:, None] * s
        out = term if out is None else out + term
    return out.astype(F32)


def degrade_noise_reference(seed: int, image_ids, gray, draw: int, H: int, W: int) -> np.ndarray:
    """float64 [B][3][H][W]: the stream values `add_gaussian_noise` adds — purpose PURPOSE_DEGRADE over the [3][H][W] image, or
    PURPOSE_DEGRADE_GRAY over the [H][W] plane, repeated for the three channels, where ``gray[b]`` is set."""
    ids = list(image_ids.tolist() if hasattr(image_ids, "tolist") else image_ids)
    gray = [int(g) for g in np.asarray(gray).reshape(-1)]
    out = np.empty((len(ids), 3, H, W), dtype=np.float64)
    for b, (i, g) in enumerate(zip(ids, gray)):
        if g:
            out[b] = stream_reference(seed, [i], PURPOSE_DEGRADE_GRAY, draw, H * W).reshape(1, H, W)
        else:
            out[b] = stream_reference(seed, [i], PURPOSE_DEGRADE, draw, 3 * H * W).reshape(3, H, W)
    return out


def add_gaussian_noise_reference(x, sigma, gray, seed: int = 0, image_ids=None, draw: int = 0, rounds: bool = False, noise=None) -> np.ndarray:
    """add_gaussian_noise_pt(clip=True): clamp(x + (n * sigma) / 255, 0, 1), or clamp(round(. * 255), 0, 255) / 255 with ``rounds``.
    ``noise`` (fp32 [B, 3, H, W]) stands in for the stream; without it n = float32(`degrade_noise_reference`), which the device's own
    Box-Muller evaluation meets only to rng's tolerance."""
    x = _batch(x)
    B, _, H, W = x.shape
    if (H * W) % 4:
        raise ValueError(f"H * W must be a multiple of 4 (the stream is drawn four elements at a time), got {H} x {W}")
    sigma = np.broadcast_to(np.asarray(sigma, dtype=F32).reshape(-1), (B,)).reshape(B, 1, 1, 1)
    if not np.isfinite(sigma).all() or (sigma < 0).any():
        raise ValueError("sigma must be finite and non-negative")
    if noise is None:
        gray = np.broadcast_to(np.asarray(gray, dtype=np.int32).reshape(-1), (B,))
        noise = degrade_noise_reference(seed, image_ids if image_ids is not None else range(B), gray, draw, H, W).astype(F32)
    noise = np.asarray(noise, dtype=F32)
    out = x + (noise * sigma) / F32(255.0)
    if rounds:
        return (np.clip(np.rint(out * F32(255.0)), F32(0), F32(255)) / F32(255.0)).astype(F32)
    return np.clip(out, F32(0), F32(1)).astype(F32)


def _sum3(m, a, b, c):
    return (a * m[0] + b * m[1]) + c * m[2]


def _dct_sum(d: np.ndarray, T: np.ndarray) -> np.ndarray:
    """[N, 64] x T[64, 64] -> [N, 64] with the 64 terms added in index order from 0, each step rounded to fp32"""
    acc = np.zeros_like(d)
    for i in range(64):
        acc = acc + d[:, i:i + 1] * T[i][None, :]
    return acc


def _split(plane: np.ndarray) -> np.ndarray:          # [B, h, w] -> [B, h/8 * w/8, 64], blocks in raster order, element x*8 + y
    B, h, w = plane.shape
    return plane.reshape(B, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4).reshape(B, -1, 64)


def _merge(blocks: np.ndarray, h: int, w: int) -> np.ndarray:
    B = blocks.shape[0]
    return blocks.reshape(B, h // 8, w // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(B, h, w)


def jpeg_reference(x, quality, return_coefs: bool = False, with_quotients: bool = False):
    """DiffJPEG(differentiable=False)(x, quality) with edtr_hip.h's operation order.  ``return_coefs``: also the quantised coefficients
    as fp32 [B][ny + 2 nc][64] (luma blocks, then Cb, then Cr); ``with_quotients``: also the quotients before rounding, same layout."""
    x = _batch(x)
    B, _, H, W = x.shape
    factor = np.broadcast_to(quality_to_factor(quality), (B,))
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    p = np.zeros((B, 3, Hp, Wp), dtype=F32)
    p[:, :, :H, :W] = x * F32(255.0)
    r, g, b = p[:, 0], p[:, 1], p[:, 2]
    planes = [_sum3(RGB2YCC[0], r, g, b)]
    for c in (1, 2):
        full = _sum3(RGB2YCC[c], r, g, b) + F32(128.0)
        s = ((full[:, 0::2, 0::2] + full[:, 0::2, 1::2]) + full[:, 1::2, 0::2]) + full[:, 1::2, 1::2]
        planes.append(s * F32(0.25))
    T = dct_table()
    coefs, quots, rec = [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for c, plane in enumerate(planes):
            d = _split(plane - F32(128.0))                                      # [B, n, 64]
            n = d.shape[1]
            F = DCT_SCALE.reshape(1, 64) * _dct_sum(d.reshape(-1, 64), T)
            tq = ((Y_TABLE if c == 0 else C_TABLE).reshape(1, 1, 64) * factor.reshape(B, 1, 1)).astype(F32)
            quot = F.reshape(B, n, 64) / tq
            q = np.rint(quot)
            coefs.append(q)
            quots.append(quot)
            cin = ((q * tq) * DCT_ALPHA.reshape(1, 1, 64)).reshape(-1, 64)
            pix = F32(0.25) * _dct_sum(cin, T.T.copy()) + F32(128.0)
            h, w = (Hp, Wp) if c == 0 else (Hp // 2, Wp // 2)
            rec.append(_merge(pix.reshape(B, n, 64), h, w))
        y = rec[0]
        cb = np.repeat(np.repeat(rec[1], 2, axis=1), 2, axis=2) - F32(128.0)
        cr = np.repeat(np.repeat(rec[2], 2, axis=1), 2, axis=2) - F32(128.0)
        out = np.stack([_sum3(YCC2RGB[c], y, cb, cr) for c in range(3)], axis=1)
        out = (np.minimum(F32(255.0), np.maximum(F32(0.0), out)) / F32(255.0))[:, :, :H, :W].astype(F32)
    res = (np.ascontiguousarray(out),)
    if return_coefs:
        res += (np.concatenate(coefs, axis=1).astype(F32),)
    if with_quotients:
        res += (np.concatenate(quots, axis=1).astype(F32),)
    return res[0] if len(res) == 1 else res


# ----------------------------------------------------------------------------------------------------------------------------------
# blur kernels (fp64 on the host, as the reference builds them)
# ----------------------------------------------------------------------------------------------------------------------------------
KERNEL_TYPES = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")


def _grid(kernel_size: int) -> np.ndarray:
    ax = np.arange(-kernel_size // 2 + 1.0, kernel_size // 2 + 1.0)
    xx, yy = np.meshgrid(ax, ax)
    return np.stack([xx, yy], axis=-1)                                          # [k, k, 2]: (x, y) of every tap


def _inverse_sigma(sig_x: float, sig_y: float, theta: float, isotropic: bool) -> np.ndarray:
    if isotropic:
        m = np.array([[sig_x ** 2, 0.0], [0.0, sig_x ** 2]])
    else:
        u = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        m = u @ (np.array([[sig_x ** 2, 0.0], [0.0, sig_y ** 2]]) @ u.T)
    return np.linalg.inv(m)


def _quadratic(kernel_size, sig_x, sig_y, theta, isotropic) -> np.ndarray:
    g = _grid(kernel_size)
    return np.sum(np.dot(g, _inverse_sigma(sig_x, sig_y, theta, isotropic)) * g, 2)


def bivariate_gaussian(kernel_size: int, sig_x: float, sig_y: float = 0.0, theta: float = 0.0, isotropic: bool = True) -> np.ndarray:
    k = np.exp(-0.5 * _quadratic(kernel_size, sig_x, sig_y, theta, isotropic))
    return k / np.sum(k)


def bivariate_generalized_gaussian(kernel_size: int, sig_x: float, sig_y: float, theta: float, beta: float, isotropic: bool = True) -> np.ndarray:
    k = np.exp(-0.5 * np.power(_quadratic(kernel_size, sig_x, sig_y, theta, isotropic), beta))
    return k / np.sum(k)


def bivariate_plateau(kernel_size: int, sig_x: float, sig_y: float, theta: float, beta: float, isotropic: bool = True) -> np.ndarray:
    k = np.reciprocal(np.power(_quadratic(kernel_size, sig_x, sig_y, theta, isotropic), beta) + 1)
    return k / np.sum(k)


def random_mixed_kernel(gen: np.random.Generator, kernel_list: Sequence[str], kernel_prob: Sequence[float], kernel_size: int,
                        sigma_range: Sequence[float], rotation_range=(-math.pi, math.pi), betag_range=(0.5, 4.0),
                        betap_range=(1.0, 2.0)) -> np.ndarray:
    """One kernel of the reference's mixture (random_mixed_kernels), drawn from ``gen`` instead of the global random state."""
    prob = np.asarray(kernel_prob, dtype=np.float64)
    kind = kernel_list[int(gen.choice(len(kernel_list), p=prob / prob.sum()))]
    if kind not in KERNEL_TYPES:
        raise ValueError(f"kernel type must be one of {KERNEL_TYPES}, got {kind!r}")
    iso = kind.endswith("iso") and not kind.endswith("aniso")
    sig_x = gen.uniform(sigma_range[0], sigma_range[1])
    sig_y = sig_x if iso else gen.uniform(sigma_range[0], sigma_range[1])
    theta = 0.0 if iso else gen.uniform(rotation_range[0], rotation_range[1])
    if kind in ("iso", "aniso"):
        return bivariate_gaussian(kernel_size, sig_x, sig_y, theta, iso)
    lo, hi = betag_range if kind.startswith("generalized") else betap_range
    beta = gen.uniform(lo, 1.0) if gen.uniform() < 0.5 and lo < 1.0 else gen.uniform(max(lo, 1.0), hi)
    fn = bivariate_generalized_gaussian if kind.startswith("generalized") else bivariate_plateau
    return fn(kernel_size, sig_x, sig_y, theta, beta, iso)


# ----------------------------------------------------------------------------------------------------------------------------------
# configuration and per-image parameters
# ----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class DegradeConfig:
    """The reference's YAML keys (configs/*/train/*.yaml, `dataset.params`).  ``blur_kernel_size`` None: no blur; ``noise_range`` /
    ``jpeg_range`` None: that step is skipped; ``resize_back``: resize to the input extent at the end (CodeFormer style).
    ``resize_modes``: what the resize mode is drawn from (the first stage of RealESRGANBatchTransform draws from all three)."""
    blur_kernel_size: Optional[int] = 41
    kernel_list: Sequence[str] = ("iso", "aniso")
    kernel_prob: Sequence[float] = (0.5, 0.5)
    blur_sigma: Sequence[float] = (0.1, 8.0)
    downsample_range: Sequence[float] = (1.0, 16.0)
    noise_range: Optional[Sequence[float]] = (0.0, 10.0)
    jpeg_range: Optional[Sequence[float]] = (50.0, 100.0)
    gray_noise_prob: float = 0.0
    resize_back: bool = True
    resize_modes: Sequence[str] = ("bilinear",)

    def __post_init__(self):
        k = self.blur_kernel_size
        if k is not None and (int(k) % 2 == 0 or not K_MIN <= int(k) <= K_MAX):
            raise ValueError(f"blur_kernel_size must be odd and in [{K_MIN}, {K_MAX}], got {k}")
        if len(self.kernel_list) != len(self.kernel_prob) or not self.kernel_list:
            raise ValueError("kernel_list and kernel_prob must have the same, positive length")
        for name in self.kernel_list:
            if name not in KERNEL_TYPES:
                raise ValueError(f"kernel type must be one of {KERNEL_TYPES}, got {name!r}")
        for m in self.resize_modes:
            if m not in MODES:
                raise ValueError(f"resize mode must be one of {MODES}, got {m!r}")
        if self.downsample_range[0] < 1.0 or self.downsample_range[1] < self.downsample_range[0]:
            raise ValueError(f"downsample_range must be [a, b] with 1 <= a <= b, got {list(self.downsample_range)}")
        if self.jpeg_range is not None and not 0 < self.jpeg_range[0] <= self.jpeg_range[1] <= 100:
            raise ValueError(f"jpeg_range must lie in (0, 100], got {list(self.jpeg_range)}")
        if self.noise_range is not None and not 0 <= self.noise_range[0] <= self.noise_range[1]:
            raise ValueError(f"noise_range must be [a, b] with 0 <= a <= b, got {list(self.noise_range)}")
        if not 0.0 <= float(self.gray_noise_prob) <= 1.0:
            raise ValueError(f"gray_noise_prob must be in [0, 1], got {self.gray_noise_prob}")

    KEYS = ("blur_kernel_size", "kernel_list", "kernel_prob", "blur_sigma", "downsample_range", "noise_range", "jpeg_range",
            "gray_noise_prob", "resize_back", "resize_modes")

    @classmethod
    def from_dict(cls, d: dict) -> "DegradeConfig":
        """From a mapping that holds the keys, at its top level or under dataset.params as the reference's configs do; other keys of
        the reference's data sets (file lists, crop sizes, ...) are ignored."""
        node = d
        for key in ("dataset", "params"):
            if isinstance(node, dict) and key in node and isinstance(node[key], dict):
                node = node[key]
        return cls(**{k: node[k] for k in cls.KEYS if k in node})


PRESETS = {
    # datasets/detection.py's chain with the values of configs/cls/cub200/train/001_lq.yaml
    "codeformer": dict(),
    # the first stage of RealESRGANBatchTransform with Real-ESRGAN's published first-stage ranges; Gaussian noise only
    "realesrgan-stage1": dict(blur_kernel_size=21, kernel_list=KERNEL_TYPES, kernel_prob=(0.45, 0.25, 0.12, 0.03, 0.12, 0.03),
                              blur_sigma=(0.2, 3.0), downsample_range=(1.0, 1.0 / 0.15), noise_range=(1.0, 30.0), jpeg_range=(30.0, 95.0),
                              gray_noise_prob=0.4, resize_back=False, resize_modes=("area", "bilinear", "bicubic")),
}


def load_config(spec):
    """A `DegradeConfig` / `RealESRGANConfig`, the name of a preset, or the path of a YAML file with the keys.  "realesrgan", or a YAML
    that carries a `batch_transform` node (the reference's layout of the second-order chain), gives a `RealESRGANConfig`."""
    if isinstance(spec, (DegradeConfig, RealESRGANConfig)):
        return spec
    if spec == "realesrgan":
        return RealESRGANConfig()
    if spec in PRESETS:
        return DegradeConfig(**PRESETS[spec])
    if not os.path.exists(spec):
        raise ValueError(f"--config must be one of {sorted(PRESETS) + ['realesrgan']} or a YAML file, got {spec!r}")
    try:
        import yaml
    except ImportError as e:
        raise RuntimeError("reading a YAML configuration needs PyYAML (`import yaml` failed); the presets need nothing") from e
    with open(spec) as fh:
        d = yaml.safe_load(fh)
    if isinstance(d, dict) and ("batch_transform" in d or (isinstance(d.get("dataset"), dict) and "batch_transform" in d["dataset"])):
        return RealESRGANConfig.from_dict(d)
    return DegradeConfig.from_dict(d)


@dataclass
class DegradeParams:
    """What `draw_params` drew for one image.  The extents are not part of it: `lq_size` forms them from the image's own."""
    kernel: Optional[np.ndarray]        # fp32 [k, k], or None: no blur
    scale: float                        # the low-quality extent is `lq_size(h, w)`
    mode: str
    sigma: Optional[float]              # None: no noise
    gray: bool
    quality: Optional[float]            # None: no JPEG
    resize_back: bool
    back_mode: str = "bilinear"

    def lq_size(self, h: int, w: int) -> Tuple[int, int]:
        """(int(h // scale), int(w // scale)) as datasets/detection.py:172, lowered to even numbers (2 at the least): the noise stream
        is drawn four elements at a time, so H W has to be a multiple of 4"""
        lh, lw = int(h // self.scale), int(w // self.scale)
        return max(2, lh - lh % 2), max(2, lw - lw % 2)


def draw_params(cfg: DegradeConfig, seed: int, image_id: int) -> DegradeParams:
    """One image's parameters from ``numpy.random.default_rng([seed, image_id])``: a function of the configuration, the seed and the
    image's data-set index, whatever else is degraded beside it.  Every draw is made whether or not its step is enabled."""
    seed, image_id = int(seed), int(image_id)
    if not 0 <= seed < 1 << 64 or not 0 <= image_id < 1 << 32:
        raise ValueError(f"seed must be in [0, 2^64) and image_id in [0, 2^32), got {seed} and {image_id}")
    gen = np.random.default_rng([seed, image_id])
    kernel = None
    if cfg.blur_kernel_size is not None:
        kernel = random_mixed_kernel(gen, list(cfg.kernel_list), list(cfg.kernel_prob), int(cfg.blur_kernel_size), cfg.blur_sigma).astype(F32)
    scale = float(gen.uniform(cfg.downsample_range[0], cfg.downsample_range[1]))
    mode = cfg.resize_modes[int(gen.integers(len(cfg.resize_modes)))]
    u_sigma, u_gray, u_q = gen.uniform(), gen.uniform(), gen.uniform()
    sigma = None if cfg.noise_range is None else float(cfg.noise_range[0] + u_sigma * (cfg.noise_range[1] - cfg.noise_range[0]))
    quality = None
    if cfg.jpeg_range is not None:
        lo, hi = float(cfg.jpeg_range[0]), float(cfg.jpeg_range[1])
        quality = float(F32(lo + u_q * (hi - lo)))
        if quality >= 100.0:                # (the factor of quality 100 is 0: the reference's uniform draw never reaches its upper end either)
            quality = float(np.nextafter(F32(100.0), F32(0.0)))
    return DegradeParams(kernel, scale, mode, sigma, bool(u_gray < cfg.gray_noise_prob), quality, bool(cfg.resize_back))


# ----------------------------------------------------------------------------------------------------------------------------------
# second order: Poisson noise by table inversion (numpy restatement, normative; edtr_hip.h "Low-quality inputs, second order")
# ----------------------------------------------------------------------------------------------------------------------------------
POISSON_VALS = tuple(1 << t for t in range(9))                    # the 9 values 2^ceil(log2(count)) can take for count in 1..256
GRAY_WEIGHTS = (F32(0.2989), F32(0.587), F32(0.114))              # torchvision's rgb_to_grayscale
_POISSON_TABLES: dict = {}


def poisson_table(vals: int) -> Tuple[np.ndarray, np.ndarray]:
    """(T uint32 [256][256], lo int32 [256]) for ``vals``: row k inverts the CDF of Poisson(lambda_k) on a 32-bit uniform, n = lo[k] +
    #{j < 255 : T[k][j] <= u}.  fp64 with + * / alone, every sum in index order (edtr_hip.h states each step): the same bits on every
    host.  Cached."""
    vals = int(vals)
    if vals not in POISSON_VALS:
        raise ValueError(f"vals must be one of {POISSON_VALS}, got {vals}")
    if vals not in _POISSON_TABLES:
        lam = ((np.arange(256, dtype=F32) / F32(255.0)) * F32(vals)).astype(np.float64)
        fl = np.floor(lam).astype(np.int64)
        lo = np.maximum(0, np.ceil(lam).astype(np.int64) - 128)
        J = 128 + 256 + 1                                       # indices 0 .. lo + 256 with lo <= 128; floor(lambda) <= 256 lies inside
        rows = np.arange(256)
        w = np.zeros((256, J), dtype=np.float64)
        w[rows, fl] = 1.0
        for j in range(1, J):
            w[:, j] = np.where(j > fl, (w[:, j - 1] * lam) / np.float64(j), w[:, j])
        with np.errstate(divide="ignore", invalid="ignore"):
            for j in range(J - 2, -1, -1):
                w[:, j] = np.where(j < fl, (w[:, j + 1] * np.float64(j + 1)) / lam, w[:, j])
        w = np.where(np.arange(J)[None, :] <= (lo + 256)[:, None], w, 0.0)
        c = np.add.accumulate(w, axis=1)                        # strictly sequential: c[j] = c[j - 1] + w[j]
        total = c[rows, lo + 256]
        cdf = c[rows[:, None], lo[:, None] + np.arange(256)[None, :]] / total[:, None]
        T = np.minimum(np.floor(cdf * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)
        _POISSON_TABLES[vals] = (np.ascontiguousarray(T), lo.astype(np.int32))
    return _POISSON_TABLES[vals]


def poisson_tables() -> Tuple[np.ndarray, np.ndarray]:
    """(uint32 [9][256][256], int32 [9][256]): `poisson_table` of 1, 2, ..., 256 — what edtr_degrade_poisson_noise reads."""
    pairs = [poisson_table(v) for v in POISSON_VALS]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def vals_of(count: int) -> int:
    """2^ceil(log2(count)) in integers"""
    count = int(count)
    if not 1 <= count <= 256:
        raise ValueError(f"a level count lies in [1, 256], got {count}")
    return 1 << (count - 1).bit_length()


def _level(v: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(v * F32(255.0)), F32(0), F32(255)).astype(np.int64)


def _gray_plane(x: np.ndarray) -> np.ndarray:
    return (GRAY_WEIGHTS[0] * x[:, 0] + GRAY_WEIGHTS[1] * x[:, 1]) + GRAY_WEIGHTS[2] * x[:, 2]


def poisson_levels(x) -> Tuple[np.ndarray, np.ndarray]:
    """(int64 [B][3][H][W] colour levels, int64 [B][H][W] grey levels) of a batch"""
    x = _batch(x)
    return _level(x), _level(_gray_plane(x))


def level_counts(x) -> np.ndarray:
    """int32 [B][2]: the number of distinct colour levels of each image, and of distinct grey levels"""
    kc, kg = poisson_levels(x)
    return np.array([[len(np.unique(kc[b])), len(np.unique(kg[b]))] for b in range(kc.shape[0])], dtype=np.int32).reshape(-1, 2)


def poisson_reference(seed: int, image_ids, purpose: int, draw, levels, vals) -> np.ndarray:
    """int64 [B][per_image]: the Poisson draws n of elements whose levels are ``levels`` (int [B][per_image]) under ``vals`` (one per
    image): table inversion of the raw stream words, by the kernel's 8-step search."""
    levels = np.asarray(levels, dtype=np.int64)
    B, per = levels.shape
    vals = np.broadcast_to(np.asarray(vals, dtype=np.int64).reshape(-1), (B,))
    u = uniform_words_reference(seed, image_ids, purpose, draw, per)
    out = np.empty((B, per), dtype=np.int64)
    for b in range(B):
        T, lo = poisson_table(int(vals[b]))
        k = levels[b]
        pos = np.zeros(per, dtype=np.int64)
        for step in (128, 64, 32, 16, 8, 4, 2, 1):
            pos = pos + step * (T[k, pos + step - 1] <= u[b])
        out[b] = lo[k] + pos
    return out


def poisson_noise_reference(x, gray, seed: int = 0, image_ids=None, draw: int = 0) -> np.ndarray:
    """fp32 [B][3][H][W]: n / vals - q per element (colour), or per pixel of the grey plane repeated over the channels"""
    x = _batch(x)
    B, _, H, W = x.shape
    if (H * W) % 4:
        raise ValueError(f"H * W must be a multiple of 4 (the stream is drawn four elements at a time), got {H} x {W}")
    gray = np.broadcast_to(np.asarray(gray, dtype=np.int32).reshape(-1), (B,))
    ids = _ids_list(image_ids, B)
    kc, kg = poisson_levels(x)
    counts = level_counts(x)
    noise = np.empty_like(x)
    for b in range(B):
        if gray[b]:
            k, vals, purpose = kg[b].reshape(1, -1), vals_of(counts[b, 1]), PURPOSE_DEGRADE_POISSON_GRAY
        else:
            k, vals, purpose = kc[b].reshape(1, -1), vals_of(counts[b, 0]), PURPOSE_DEGRADE_POISSON
        n = poisson_reference(seed, [ids[b]], purpose, draw, k, [vals])
        nz = (n.astype(F32) / F32(vals) - k.astype(F32) / F32(255.0)).astype(F32)
        noise[b] = nz.reshape((1, H, W) if gray[b] else (3, H, W))
    return noise


def _ids_list(image_ids, B: int) -> List[int]:
    ids = list(range(B)) if image_ids is None else list(image_ids.tolist() if hasattr(image_ids, "tolist") else image_ids)
    if len(ids) != B:
        raise ValueError(f"{len(ids)} image ids for a batch of {B}")
    return [int(i) for i in ids]


def add_poisson_noise_reference(x, scale, gray, seed: int = 0, image_ids=None, draw: int = 0, rounds: bool = False, return_noise: bool = False):
    """add_poisson_noise_pt(clip=True) with torch.poisson replaced by `poisson_reference`: clamp(x + noise * scale, 0, 1), or
    clamp(round(. * 255), 0, 255) / 255 with ``rounds``."""
    x = _batch(x)
    B = x.shape[0]
    scale = np.broadcast_to(np.asarray(scale, dtype=F32).reshape(-1), (B,)).reshape(B, 1, 1, 1)
    if not np.isfinite(scale).all() or (scale < 0).any():
        raise ValueError("scale must be finite and non-negative")
    noise = poisson_noise_reference(x, gray, seed, image_ids, draw)
    out = x + noise * scale
    if rounds:
        out = (np.clip(np.rint(out * F32(255.0)), F32(0), F32(255)) / F32(255.0)).astype(F32)
    else:
        out = np.clip(out, F32(0), F32(1)).astype(F32)
    return (out, noise) if return_noise else out


# ----------------------------------------------------------------------------------------------------------------------------------
# second order: USM sharpening and the sinc kernels
# ----------------------------------------------------------------------------------------------------------------------------------
SEP_K_MIN, SEP_K_MAX = 3, 63


def gaussian_taps(k: int, sigma: float = 0.0) -> np.ndarray:
    """float64 [k]: cv2.getGaussianKernel(k, sigma) by its formula — with a non-positive sigma, sigma = 0.3 ((k - 1) 0.5 - 1) + 0.8 (8.0
    at k = 51); g_i proportional to exp(-(i - (k - 1)/2)^2 / (2 sigma^2)), normalised in fp64.  cv2 answers k <= 7 with a non-positive
    sigma from fixed tables instead, so that case is refused."""
    k = int(k)
    if k % 2 == 0 or k < 1:
        raise ValueError(f"the tap count must be odd and positive, got {k}")
    if sigma <= 0:
        if k <= 7:
            raise ValueError("cv2 takes the taps of k <= 7 with a non-positive sigma from fixed tables; give a sigma")
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    i = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return g / g.sum()


def _check_taps(taps, H: int, W: int) -> np.ndarray:
    g = np.ascontiguousarray(taps, dtype=F32).reshape(-1)
    k = g.shape[0]
    if k % 2 == 0 or not SEP_K_MIN <= k <= SEP_K_MAX:
        raise ValueError(f"the tap count must be odd and in [{SEP_K_MIN}, {SEP_K_MAX}], got {k}")
    if k // 2 >= min(H, W):
        raise ValueError(f"{k} taps need reflect padding of {k // 2}, more than a {H} x {W} image allows")
    return g


def sepblur_reference(x, taps, threshold: Optional[float] = None):
    """Separable correlation over reflect-padded borders: along rows, t = t + p * g[kx] from 0 in tap order for every padded row, then
    along columns the same over t.  With ``threshold`` also the mask (|x - out| * 255 > threshold) as fp32 0 / 1."""
    x = _batch(x)
    H, W = x.shape[2:]
    g = _check_taps(taps, H, W)
    k = g.shape[0]
    r = k // 2
    pad = np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)), mode="reflect")
    t = np.zeros(pad.shape[:3] + (W,), dtype=F32)
    for kx in range(k):
        t = t + pad[:, :, :, kx:kx + W] * g[kx]
    out = np.zeros_like(x)
    for ky in range(k):
        out = out + t[:, :, ky:ky + H] * g[ky]
    if threshold is None:
        return out
    return out, (np.abs(x - out) * F32(255.0) > F32(threshold)).astype(F32)


def usm_apply_reference(x, blur, soft, weight: float) -> np.ndarray:
    x = _batch(x)
    sharp = np.clip(x + F32(weight) * (x - blur), F32(0), F32(1))
    return (soft * sharp + (F32(1.0) - soft) * x).astype(F32)


def _usm_taps(radius: int) -> np.ndarray:
    k = int(radius) + (1 if int(radius) % 2 == 0 else 0)
    if not SEP_K_MIN <= k <= SEP_K_MAX:
        raise ValueError(f"the USM radius must give a tap count in [{SEP_K_MIN}, {SEP_K_MAX}], got {k}")
    return gaussian_taps(k).astype(F32)


def usm_sharpen_reference(x, weight: float = 0.5, threshold: float = 10, radius: int = 50) -> np.ndarray:
    """USMSharp(radius)(x, weight, threshold) with the 2-D kernel g g^T applied as two 1-D passes of float32(g)."""
    g = _usm_taps(radius)
    blur, mask = sepblur_reference(x, g, threshold)
    return usm_apply_reference(x, blur, sepblur_reference(mask, g), weight)


def bessel_j1(x) -> np.ndarray:
    """J1(x) = (1 / pi) * integral over [0, pi] of cos(theta - x sin(theta)), by the midpoint rule with 128 points: no scipy.  Exact to
    1e-15 for |x| <= 45 (the integrand is periodic and analytic); the chain's largest argument is pi * sqrt(200) = 44.4."""
    x = np.asarray(x, dtype=np.float64)
    theta = (np.arange(128, dtype=np.float64) + 0.5) * (np.pi / 128.0)
    return np.cos(theta - x[..., None] * np.sin(theta)).sum(axis=-1) / 128.0


def circular_lowpass_kernel(cutoff: float, kernel_size: int, pad_to: int = 0) -> np.ndarray:
    """The 2-D sinc filter of datasets/degradation.py:390-410 (float64 [k, k], or [pad_to, pad_to] zero-padded)."""
    kernel_size = int(kernel_size)
    if kernel_size % 2 != 1:
        raise ValueError("Kernel size must be an odd number.")
    c = (kernel_size - 1) / 2
    ax = np.arange(kernel_size, dtype=np.float64) - c
    rad = np.sqrt(ax[:, None] ** 2 + ax[None, :] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        kernel = cutoff * bessel_j1(cutoff * rad) / (2 * np.pi * rad)
    kernel[(kernel_size - 1) // 2, (kernel_size - 1) // 2] = cutoff ** 2 / (4 * np.pi)
    kernel = kernel / np.sum(kernel)
    if pad_to > kernel_size:
        p = (int(pad_to) - kernel_size) // 2
        kernel = np.pad(kernel, ((p, p), (p, p)))
    return kernel


# ----------------------------------------------------------------------------------------------------------------------------------
# second order: configuration and per-image parameters
# ----------------------------------------------------------------------------------------------------------------------------------
KERNEL_RANGE = tuple(range(7, 22, 2))           # datasets/detection_cocov2.py:100
KERNEL_PAD = 21                                 # every kernel is zero-padded to 21 x 21 (:218, :243, :250)
NOISE_TYPES = ("gaussian", "poisson")


def _range(name: str, v, lo: float, hi: float = math.inf) -> Tuple[float, float]:
    try:
        a, b = float(v[0]), float(v[1])
        ok = len(v) == 2
    except (TypeError, IndexError, ValueError):
        ok, a, b = False, 0.0, 0.0
    if not ok or not lo <= a <= b <= hi:
        raise ValueError(f"{name} must be [a, b] with {lo:g} <= a <= b <= {hi:g}, got {v!r}")
    return a, b


def _prob(name: str, v) -> float:
    if not 0.0 <= float(v) <= 1.0:
        raise ValueError(f"{name} must be in [0, 1], got {v}")
    return float(v)


@dataclass
class RealESRGANConfig:
    """The reference's keys of the second-order chain: the data set's (`dataset.val.params` / `dataset.params`: the kernels) and the
    batch transform's (`batch_transform.params`: everything else).  The defaults are configs' coco-deg-realesrgan.yaml."""
    blur_kernel_size: int = 21
    kernel_list: Sequence[str] = KERNEL_TYPES
    kernel_prob: Sequence[float] = (0.45, 0.25, 0.12, 0.03, 0.12, 0.03)
    sinc_prob: float = 0.1
    blur_sigma: Sequence[float] = (0.2, 3.0)
    betag_range: Sequence[float] = (0.5, 4.0)
    betap_range: Sequence[float] = (1.0, 2.0)
    blur_kernel_size2: int = 21
    kernel_list2: Sequence[str] = KERNEL_TYPES
    kernel_prob2: Sequence[float] = (0.45, 0.25, 0.12, 0.03, 0.12, 0.03)
    sinc_prob2: float = 0.1
    blur_sigma2: Sequence[float] = (0.2, 1.5)
    betag_range2: Sequence[float] = (0.5, 4.0)
    betap_range2: Sequence[float] = (1.0, 2.0)
    final_sinc_prob: float = 0.8
    use_sharpener: bool = True
    queue_size: int = 0
    resize_prob: Sequence[float] = (0.2, 0.7, 0.1)
    resize_range: Sequence[float] = (0.15, 1.5)
    gray_noise_prob: float = 0.4
    gaussian_noise_prob: float = 0.5
    noise_range: Sequence[float] = (1.0, 30.0)
    poisson_scale_range: Sequence[float] = (0.05, 3.0)
    jpeg_range: Sequence[float] = (30.0, 95.0)
    second_blur_prob: float = 0.8
    stage2_scale: object = 4                    # a number, or a range [a, b] that the scale is drawn from
    resize_prob2: Sequence[float] = (0.3, 0.4, 0.3)
    resize_range2: Sequence[float] = (0.3, 1.2)
    gray_noise_prob2: float = 0.4
    gaussian_noise_prob2: float = 0.5
    noise_range2: Sequence[float] = (1.0, 25.0)
    poisson_scale_range2: Sequence[float] = (0.05, 2.5)
    jpeg_range2: Sequence[float] = (30.0, 95.0)
    resize_back: bool = True

    DATASET_KEYS = ("blur_kernel_size", "kernel_list", "kernel_prob", "sinc_prob", "blur_sigma", "betag_range", "betap_range",
                    "blur_kernel_size2", "kernel_list2", "kernel_prob2", "sinc_prob2", "blur_sigma2", "betag_range2", "betap_range2",
                    "final_sinc_prob")
    TRANSFORM_KEYS = ("use_sharpener", "queue_size", "resize_prob", "resize_range", "gray_noise_prob", "gaussian_noise_prob", "noise_range",
                      "poisson_scale_range", "jpeg_range", "second_blur_prob", "stage2_scale", "resize_prob2", "resize_range2",
                      "gray_noise_prob2", "gaussian_noise_prob2", "noise_range2", "poisson_scale_range2", "jpeg_range2", "resize_back")

    def __post_init__(self):
        if int(self.queue_size) > 0:
            raise ValueError("queue_size > 0 (the training pair pool) is not provided: it mixes images across batches, so an image's "
                             "low-quality version would no longer depend on the image, the seed and its index alone")
        for s in ("", "2"):
            names, probs = getattr(self, "kernel_list" + s), getattr(self, "kernel_prob" + s)
            if len(names) != len(probs) or not names or min(float(p) for p in probs) < 0 or sum(float(p) for p in probs) <= 0:
                raise ValueError(f"kernel_list{s} and kernel_prob{s} must have the same, positive length and non-negative weights")
            for name in names:
                if name not in KERNEL_TYPES:
                    raise ValueError(f"kernel type must be one of {KERNEL_TYPES}, got {name!r}")
            _range("blur_sigma" + s, getattr(self, "blur_sigma" + s), 1e-6)
            _range("betag_range" + s, getattr(self, "betag_range" + s), 1e-6)
            _range("betap_range" + s, getattr(self, "betap_range" + s), 1e-6)
            _prob("sinc_prob" + s, getattr(self, "sinc_prob" + s))
            _prob("gray_noise_prob" + s, getattr(self, "gray_noise_prob" + s))
            _prob("gaussian_noise_prob" + s, getattr(self, "gaussian_noise_prob" + s))
            _range("noise_range" + s, getattr(self, "noise_range" + s), 0.0, 3.0e38)
            _range("poisson_scale_range" + s, getattr(self, "poisson_scale_range" + s), 0.0, 3.0e38)
            lo, hi = _range("jpeg_range" + s, getattr(self, "jpeg_range" + s), 0.0, 100.0)
            if lo <= 0:
                raise ValueError(f"jpeg_range{s} must lie in (0, 100], got {list(getattr(self, 'jpeg_range' + s))}")
            rr = getattr(self, "resize_range" + s)
            _range("resize_range" + s, rr, 1e-6)
            if float(rr[0]) > 1.0 or float(rr[1]) < 1.0:
                raise ValueError(f"resize_range{s} must be [a, b] with a <= 1 <= b, got {list(rr)}")
            rp = getattr(self, "resize_prob" + s)
            if len(rp) != 3 or min(float(p) for p in rp) < 0 or sum(float(p) for p in rp) <= 0:
                raise ValueError(f"resize_prob{s} must be three non-negative weights (up, down, keep), got {list(rp)}")
        _prob("final_sinc_prob", self.final_sinc_prob)
        _prob("second_blur_prob", self.second_blur_prob)
        if isinstance(self.stage2_scale, (int, float)):
            if not self.stage2_scale >= 1e-6:
                raise ValueError(f"stage2_scale must be positive, got {self.stage2_scale}")
        else:
            _range("stage2_scale", self.stage2_scale, 1e-6)

    @classmethod
    def from_dict(cls, d: dict) -> "RealESRGANConfig":
        """From the reference's layout: the kernel keys under dataset.val.params or dataset.params, the others under batch_transform.params
        (at the top level or under dataset), or all keys flat at the top level.  Keys of neither group are ignored."""
        ds = d.get("dataset", d) if isinstance(d, dict) else {}
        bt = d.get("batch_transform") or (ds.get("batch_transform") if isinstance(ds, dict) else None) or d
        node = ds
        for key in ("val", "params"):
            if isinstance(node, dict) and isinstance(node.get(key), dict):
                node = node[key]
        bt = bt.get("params", bt) if isinstance(bt, dict) else {}
        kw = {k: node[k] for k in cls.DATASET_KEYS if isinstance(node, dict) and k in node}
        kw.update({k: bt[k] for k in cls.TRANSFORM_KEYS if k in bt})
        return cls(**kw)


@dataclass
class Degrade2Params:
    """What `draw_params2` drew for one image.  Extents are formed from the image's own by `sizes`."""
    kernel1: np.ndarray                 # fp32 [21, 21]
    kernel2: Optional[np.ndarray]       # fp32 [21, 21], or None: second_blur_prob decided against the second blur
    sinc_kernel: Optional[np.ndarray]   # fp32 [21, 21], or None: the pulse (identity), which is not launched
    scale1: float
    mode1: str
    noise1: str                         # "gaussian" | "poisson"
    level1: float                       # sigma (gaussian, in 1/255) or scale (poisson)
    gray1: bool
    quality1: float
    stage2_scale: float
    scale2: float
    mode2: str
    noise2: str
    level2: float
    gray2: bool
    sinc_first: bool                    # [resize + sinc] then JPEG; otherwise JPEG first
    back_mode: str
    quality2: float
    use_sharpener: bool
    resize_back: bool
    kernel_size1: int = 0               # what was decided on the way (for statistics; the chain does not read them)
    kernel_size2: int = 0
    sinc1: bool = False
    sinc2: bool = False

    def sizes(self, h: int, w: int):
        """((h1, w1), (h2, w2), (hs, ws), (hf, wf)): the extents after the first resize, after the second, of stage 2 (int(h / s2)), and
        of the result.  Intermediate extents are int(.) as the reference forms them, lowered to even numbers, 2 at the least: the
        noise stream is drawn four elements at a time."""
        even = lambda v: max(2, int(v) - int(v) % 2)
        s1 = (even(h * self.scale1), even(w * self.scale1))
        ss = (even(h / self.stage2_scale), even(w / self.stage2_scale))
        s2 = (even(ss[0] * self.scale2), even(ss[1] * self.scale2))
        final = (int(h), int(w)) if self.resize_back and self.stage2_scale != 1 else ss
        return s1, s2, ss, final


def _quality(lo: float, hi: float, u: float) -> float:
    q = float(F32(lo + u * (hi - lo)))
    return float(np.nextafter(F32(100.0), F32(0.0))) if q >= 100.0 else q


def _mixed_kernel_fixed(gen: np.random.Generator, kernel_list, kernel_prob, kernel_size, sigma_range, betag_range, betap_range) -> np.ndarray:
    """`random_mixed_kernel` with a FIXED number of draws (six uniforms: kind, sigma x, sigma y, rotation, beta branch, beta), each
    made whether or not the kind needs it."""
    u_kind, u_sx, u_sy, u_th, u_branch, u_beta = (float(v) for v in gen.uniform(size=6))
    prob = np.cumsum(np.asarray(kernel_prob, dtype=np.float64))
    kind = kernel_list[min(int(np.searchsorted(prob / prob[-1], u_kind, side="right")), len(kernel_list) - 1)]
    iso = kind.endswith("iso") and not kind.endswith("aniso")
    lo, hi = float(sigma_range[0]), float(sigma_range[1])
    sig_x = lo + u_sx * (hi - lo)
    sig_y = sig_x if iso else lo + u_sy * (hi - lo)
    theta = 0.0 if iso else -math.pi + u_th * 2.0 * math.pi
    if kind in ("iso", "aniso"):
        return bivariate_gaussian(kernel_size, sig_x, sig_y, theta, iso)
    blo, bhi = (float(v) for v in (betag_range if kind.startswith("generalized") else betap_range))
    if u_branch < 0.5 and blo < 1.0:            # (random_mixed_kernels: half of the draws below 1, half above)
        beta = blo + u_beta * (1.0 - blo)
    else:
        beta = max(blo, 1.0) + u_beta * (bhi - max(blo, 1.0))
    fn = bivariate_generalized_gaussian if kind.startswith("generalized") else bivariate_plateau
    return fn(kernel_size, sig_x, sig_y, theta, beta, iso)


def _pad_kernel(k: np.ndarray) -> np.ndarray:
    p = (KERNEL_PAD - k.shape[0]) // 2
    return np.pad(k, ((p, p), (p, p))).astype(F32)


def draw_params2(cfg: RealESRGANConfig, seed: int, image_id: int) -> Degrade2Params:
    """One image's decisions of datasets/detection_cocov2.py:197-253 and :426-532 from ``numpy.random.default_rng([seed, image_id])``.
    Every draw is made whether or not it is used, in this order (u: uniform(), i(n): integers(n)):
      stage-1 kernel   i(8) size of KERNEL_RANGE, u sinc?, u omega_c, then the six uniforms of `_mixed_kernel_fixed`
      stage-2 kernel   the same nine
      final sinc       u sinc?, i(8) size, u omega_c
      stage 1          u up / down / keep, u scale, i(3) resize mode, u gaussian?, u sigma or scale, u grey?, u JPEG quality
      stage 2          u second blur?, u stage2_scale, u up / down / keep, u scale, i(3) mode, u gaussian?, u sigma or scale, u grey?
      the end          u order, i(3) mode of the resize to the stage-2 extent, u JPEG quality
    so that no decision shifts another."""
    seed, image_id = int(seed), int(image_id)
    if not 0 <= seed < 1 << 64 or not 0 <= image_id < 1 << 32:
        raise ValueError(f"seed must be in [0, 2^64) and image_id in [0, 2^32), got {seed} and {image_id}")
    gen = np.random.default_rng([seed, image_id])
    modes = ("area", "bilinear", "bicubic")

    def blur_kernel(s: str):
        size = KERNEL_RANGE[int(gen.integers(len(KERNEL_RANGE)))]
        u_sinc, u_omega = float(gen.uniform()), float(gen.uniform())
        mixed = _mixed_kernel_fixed(gen, list(getattr(cfg, "kernel_list" + s)), list(getattr(cfg, "kernel_prob" + s)), size,
                                    getattr(cfg, "blur_sigma" + s), getattr(cfg, "betag_range" + s), getattr(cfg, "betap_range" + s))
        sinc = u_sinc < float(getattr(cfg, "sinc_prob" + s))
        if sinc:
            lo = np.pi / 3 if size < 13 else np.pi / 5
            mixed = circular_lowpass_kernel(lo + u_omega * (np.pi - lo), size)
        return _pad_kernel(mixed), size, sinc

    def updown(s: str):
        u_type, u_scale = float(gen.uniform()), float(gen.uniform())
        p = np.cumsum(np.asarray(getattr(cfg, "resize_prob" + s), dtype=np.float64))
        which = min(int(np.searchsorted(p / p[-1], u_type, side="right")), 2)
        lo, hi = (float(v) for v in getattr(cfg, "resize_range" + s))
        return (1.0 + u_scale * (hi - 1.0), lo + u_scale * (1.0 - lo), 1.0)[which]

    def noise(s: str):
        u_type, u_level, u_gray = float(gen.uniform()), float(gen.uniform()), float(gen.uniform())
        kind = "gaussian" if u_type < float(getattr(cfg, "gaussian_noise_prob" + s)) else "poisson"
        lo, hi = (float(v) for v in getattr(cfg, ("noise_range" if kind == "gaussian" else "poisson_scale_range") + s))
        return kind, lo + u_level * (hi - lo), bool(u_gray < float(getattr(cfg, "gray_noise_prob" + s)))

    kernel1, size1, sinc1 = blur_kernel("")
    kernel2, size2, sinc2 = blur_kernel("2")
    u_final, i_final, u_omega = float(gen.uniform()), int(gen.integers(len(KERNEL_RANGE))), float(gen.uniform())
    sinc_kernel = None
    if u_final < float(cfg.final_sinc_prob):
        sinc_kernel = circular_lowpass_kernel(np.pi / 3 + u_omega * (np.pi - np.pi / 3), KERNEL_RANGE[i_final], pad_to=KERNEL_PAD).astype(F32)
    scale1 = updown("")
    mode1 = modes[int(gen.integers(3))]
    noise1, level1, gray1 = noise("")
    quality1 = _quality(float(cfg.jpeg_range[0]), float(cfg.jpeg_range[1]), float(gen.uniform()))
    u_blur2, u_s2 = float(gen.uniform()), float(gen.uniform())
    if isinstance(cfg.stage2_scale, (int, float)):
        s2 = float(cfg.stage2_scale)
    else:
        s2 = float(cfg.stage2_scale[0]) + u_s2 * (float(cfg.stage2_scale[1]) - float(cfg.stage2_scale[0]))
    scale2 = updown("2")
    mode2 = modes[int(gen.integers(3))]
    noise2, level2, gray2 = noise("2")
    u_order, i_back, u_q2 = float(gen.uniform()), int(gen.integers(3)), float(gen.uniform())
    return Degrade2Params(kernel1=kernel1, kernel2=kernel2 if u_blur2 < float(cfg.second_blur_prob) else None, sinc_kernel=sinc_kernel,
                          scale1=scale1, mode1=mode1, noise1=noise1, level1=level1, gray1=gray1, quality1=quality1, stage2_scale=s2,
                          scale2=scale2, mode2=mode2, noise2=noise2, level2=level2, gray2=gray2, sinc_first=bool(u_order < 0.5),
                          back_mode=modes[i_back], quality2=_quality(float(cfg.jpeg_range2[0]), float(cfg.jpeg_range2[1]), u_q2),
                          use_sharpener=bool(cfg.use_sharpener), resize_back=bool(cfg.resize_back), kernel_size1=size1, kernel_size2=size2,
                          sinc1=sinc1, sinc2=sinc2)


def _chain2(x, p: Degrade2Params, ops2: dict, noise_args):
    """The second-order chain on ONE group of images that share every extent and launch-level choice; ``ops2`` maps the step names to
    the device wrappers or to the numpy restatements, so that both walk the same code.  Returns (lq, gt)."""
    h, w = x.shape[2:]
    s1, s2, ss, final = p[0].sizes(h, w)
    f2d, rs, gn, pn, jp, usm = (ops2[k] for k in ("filter2d", "resize", "gaussian", "poisson", "jpeg", "usm"))

    def blur(x, kernels, what):
        if KERNEL_PAD // 2 >= min(x.shape[2:]):
            raise ValueError(f"{what}: a {KERNEL_PAD} x {KERNEL_PAD} kernel needs reflect padding of {KERNEL_PAD // 2}, more than the "
                             f"{x.shape[2]} x {x.shape[3]} extent of this step allows; the step is not skipped silently — narrow the resize ranges or use larger images")
        return f2d(x, np.stack(kernels))

    def noise(x, kind, levels, grays, draw):
        return (gn if kind == "gaussian" else pn)(x, levels, grays, noise_args, draw)

    if p[0].use_sharpener:
        x = usm(x)
    gt = x
    x = blur(x, [q.kernel1 for q in p], "the first blur")
    x = rs(x, s1, p[0].mode1)
    x = noise(x, p[0].noise1, [q.level1 for q in p], [q.gray1 for q in p], 0)
    x = jp(x, [q.quality1 for q in p])
    if p[0].kernel2 is not None:
        x = blur(x, [q.kernel2 for q in p], "the second blur")
    x = rs(x, s2, p[0].mode2)
    x = noise(x, p[0].noise2, [q.level2 for q in p], [q.gray2 for q in p], 1)

    def back_and_sinc(x):
        x = rs(x, ss, p[0].back_mode)
        if p[0].sinc_kernel is not None:
            x = blur(x, [q.sinc_kernel for q in p], "the final sinc filter")
        return x

    if p[0].sinc_first:
        # (the clamp to [0, 1] before the JPEG step, :518: a noise launch with sigma 0, as `degrade_batch` does)
        x = jp(gn(back_and_sinc(x), [0.0] * len(p), [False] * len(p), noise_args, 0), [q.quality2 for q in p])
    else:
        x = back_and_sinc(jp(x, [q.quality2 for q in p]))
    if final != ss:
        x = rs(x, final, "bicubic")
    if (final[0] * final[1]) % 4:
        raise ValueError(f"the final rounding is a noise launch and needs H * W % 4 == 0, got {final[0]} x {final[1]}")
    return gn(x, [0.0] * len(p), [False] * len(p), noise_args, 0, True), gt


def _group_key2(size, p: Degrade2Params):
    """what the launches of one `_chain2` call have to share: every extent, the resize modes, the noise types, which steps run"""
    return (tuple(size), p.sizes(*size), p.mode1, p.mode2, p.back_mode, p.noise1, p.noise2, p.kernel2 is None, p.sinc_kernel is None,
            p.sinc_first, p.use_sharpener)


def degrade2_reference(hq, params: Sequence[Degrade2Params], seed: int, image_ids: Sequence[int], return_gt: bool = False):
    """The second-order chain in numpy, image by image: ``hq`` a list of fp32 [3, h, w] arrays (or one [B, 3, H, W] batch).  Returns one
    fp32 [3, h', w'] array per image (and the sharpened inputs with ``return_gt``).  With Gaussian noise the stream values are the host's
    (`degrade_noise_reference`), which the device meets only to rng's tolerance; with Poisson noise every bit is the device's."""
    def gn(x, sigma, gray, ids, draw, rounds=False):
        return add_gaussian_noise_reference(x, sigma, gray, seed, ids, draw, rounds)

    def pn(x, scale, gray, ids, draw):
        return add_poisson_noise_reference(x, scale, gray, seed, ids, draw)

    ops2 = dict(filter2d=filter2d_reference, resize=resize_reference, gaussian=gn, poisson=pn, jpeg=jpeg_reference, usm=usm_sharpen_reference)
    lqs, gts = [], []
    for b, p in enumerate(params):
        lq, gt = _chain2(np.ascontiguousarray(hq[b], dtype=F32)[None], [p], ops2, [int(image_ids[b])])
        lqs.append(lq[0])
        gts.append(gt[0])
    return (lqs, gts) if return_gt else lqs


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _dct_on(device):
    from .imageio import on_device
    return on_device(("dct",), device, dct_table)


def _per_image(values, gray, B: int):
    """one float and one 0 / 1 per image from ``values`` / ``gray`` given per image or once for all"""
    return ([float(v) for v in np.broadcast_to(np.asarray(values, dtype=np.float64).reshape(-1), (B,))],
            [int(bool(v)) for v in np.broadcast_to(np.asarray(gray).reshape(-1), (B,))])


def _check_device_batch(x, what: str):
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.ndim != 4 or x.shape[1] != 3 or not x.is_contiguous() or not x.is_cuda:
        raise TypeError(f"{what} takes a contiguous fp32 [B, 3, H, W] tensor on the device")
    return x


def filter2d(x, kernels):
    """`filter2d_reference` on the device: ``kernels`` fp32 [B, k, k] (or [1, k, k] / [k, k]: one kernel for every image)."""
    import torch
    from . import ops
    _check_device_batch(x, "filter2d")
    k = torch.as_tensor(kernels, dtype=torch.float32)
    k = (k[None] if k.ndim == 2 else k).to(x.device).contiguous()
    out = torch.empty_like(x)
    ops.launch(ops.make_degrade_filter2d(x=x, kernels=k, out=out))
    return out


def resize(x, size, mode: str):
    """`resize_reference` on the device.  ``size`` only: see edtr_hip.h on why scale_factor is not offered."""
    import torch
    from . import ops
    _check_device_batch(x, "resize")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    oh, ow = _check_size(size)
    out = torch.empty((x.shape[0], 3, oh, ow), dtype=torch.float32, device=x.device)
    ops.launch(ops.make_degrade_resize(x=x, out=out, mode=MODES.index(mode)))
    return out


def add_gaussian_noise(x, sigma, gray, source, draw: int = 0, rounds: bool = False, return_noise: bool = False):
    """`add_gaussian_noise_reference` on the device with the stream of ``source`` (a `rng.NoiseSource`: seed and global image ids).
    ``sigma`` / ``gray``: one value per image (or one for all).  ``return_noise``: also the fp32 noise tensor that was added."""
    import torch
    from . import ops
    _check_device_batch(x, "add_gaussian_noise")
    sigma, gray = _per_image(sigma, gray, x.shape[0])
    out = torch.empty_like(x)
    noise = torch.empty_like(x) if return_noise else None
    ops.launch(ops.make_degrade_gaussian_noise(x=x, out=out, noise_out=noise, sigma=sigma, gray=gray, source=source, draw=draw, rounds=rounds))
    return (out, noise) if return_noise else out


def jpeg(x, quality, return_coefs: bool = False):
    """`jpeg_reference` on the device: ``quality`` one value per image (or one for all), each in (0, 100]."""
    import torch
    from . import ops
    _check_device_batch(x, "jpeg")
    B, _, H, W = x.shape
    q = np.broadcast_to(np.atleast_1d(np.asarray(quality, dtype=F32)).reshape(-1), (B,))
    factor = torch.from_numpy(quality_to_factor(q).copy()).to(x.device)
    out = torch.empty_like(x)
    coefs = None
    if return_coefs:
        mcus = ((H + 15) // 16) * ((W + 15) // 16)
        coefs = torch.empty((B, 6 * mcus, 64), dtype=torch.float32, device=x.device)
    ops.launch(ops.make_degrade_jpeg(x=x, out=out, quality=[float(v) for v in q], factor=factor, dct=_dct_on(x.device), coefs=coefs))
    return (out, coefs) if return_coefs else out


def _groups(keys: Sequence) -> List[List[int]]:
    out: dict = {}
    for i, k in enumerate(keys):
        out.setdefault(k, []).append(i)
    return list(out.values())


def degrade_batch(hq, params: Sequence[DegradeParams], seed: int, image_ids: Sequence[int], sizes: Optional[Sequence[Tuple[int, int]]] = None,
                  draw: int = 0) -> List:
    """The chain on a batch: ``hq`` fp32 [B, 3, H, W] on the device (image b in the top-left ``sizes[b]`` = (h, w) of its slot; the whole
    slot without ``sizes``), one `DegradeParams` and one global id per image.  Returns one fp32 [3, h', w'] tensor per image.  Images
    are grouped by what a launch has to share — extent and kernel size for the blur, extents and mode for a resize — and every other
    parameter travels per image, so an image's result does not depend on its companions."""
    import torch
    from .rng import NoiseSource
    _check_device_batch(hq, "degrade_batch")
    B = hq.shape[0]
    if len(params) != B or len(image_ids) != B:
        raise ValueError(f"{len(params)} parameter sets and {len(image_ids)} ids for a batch of {B}")
    sizes = [(int(h), int(w)) for h, w in sizes] if sizes is not None else [tuple(hq.shape[2:])] * B
    ids = [int(i) for i in image_ids]
    cur = [hq[b:b + 1, :, :h, :w].contiguous() for b, (h, w) in enumerate(sizes)]       # [1, 3, h, w] each

    def run(keys, fn):
        for idx in _groups(keys):
            if keys[idx[0]] is None:
                continue
            res = fn(torch.cat([cur[i] for i in idx]) if len(idx) > 1 else cur[idx[0]], idx)
            for j, i in enumerate(idx):
                cur[i] = res[j:j + 1]

    run([None if p.kernel is None else (sizes[b], p.kernel.shape[0]) for b, p in enumerate(params)],
        lambda x, idx: filter2d(x, np.stack([params[i].kernel for i in idx])))
    lq = [p.lq_size(*sizes[b]) for b, p in enumerate(params)]
    run([(sizes[b], lq[b], p.mode) for b, p in enumerate(params)], lambda x, idx: resize(x, lq[idx[0]], params[idx[0]].mode))
    # (an image that is compressed without noise still takes the noise launch, with sigma 0: its clamp to [0, 1] is the one the
    # reference applies before the JPEG step, datasets/detection_cocov2.py:459)
    run([None if p.sigma is None and p.quality is None else lq[b] for b, p in enumerate(params)],
        lambda x, idx: add_gaussian_noise(x, [params[i].sigma or 0.0 for i in idx], [params[i].gray for i in idx],
                                          NoiseSource(seed, [ids[i] for i in idx]), draw=draw))
    run([None if p.quality is None else lq[b] for b, p in enumerate(params)], lambda x, idx: jpeg(x, [params[i].quality for i in idx]))
    run([(lq[b], sizes[b], p.back_mode) if p.resize_back else None for b, p in enumerate(params)],
        lambda x, idx: resize(x, sizes[idx[0]], params[idx[0]].back_mode))
    return [c[0] for c in cur]


# ----------------------------------------------------------------------------------------------------------------------------------
# second order: device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _poisson_arrays():
    T, lo = poisson_tables()
    return T.view(np.int32), lo


def poisson_tables_on(device):
    """(uint32-as-int32 [9, 256, 256], int32 [9, 256]) tensors of `poisson_tables` on ``device``: built once, uploaded once per device"""
    from .imageio import on_device
    return on_device(("poisson",), device, _poisson_arrays)


def add_poisson_noise(x, scale, gray, source, draw: int = 0, rounds: bool = False, return_noise: bool = False, return_counts: bool = False):
    """`add_poisson_noise_reference` on the device with the stream of ``source`` (a `rng.NoiseSource`).  ``scale`` / ``gray``: one value
    per image (or one for all).  ``return_noise``: also the fp32 noise tensor; ``return_counts``: also the int32 [B, 2] level counts."""
    import torch
    from . import ops
    _check_device_batch(x, "add_poisson_noise")
    B = x.shape[0]
    scale, gray = _per_image(scale, gray, B)
    tables, lows = poisson_tables_on(x.device)
    out = torch.empty_like(x)
    noise = torch.empty_like(x) if return_noise else None
    levels = torch.empty((B, 16), dtype=torch.int32, device=x.device)
    counts = torch.empty((B, 2), dtype=torch.int32, device=x.device) if return_counts else None
    ops.launch(ops.make_degrade_poisson_noise(x=x, out=out, noise_out=noise, scale=scale, gray=gray, tables=tables, lows=lows, levels=levels,
                                              counts_out=counts, source=source, draw=draw, rounds=rounds))
    res = (out,) + ((noise,) if return_noise else ()) + ((counts,) if return_counts else ())
    return res[0] if len(res) == 1 else res


def sepblur(x, taps, threshold: Optional[float] = None):
    """`sepblur_reference` on the device: ``taps`` fp32 [k]; with ``threshold`` also the 0 / 1 mask."""
    import torch
    from . import ops
    _check_device_batch(x, "sepblur")
    g = torch.as_tensor(np.ascontiguousarray(taps, dtype=F32).reshape(-1)).to(x.device)
    out = torch.empty_like(x)
    mask = torch.empty_like(x) if threshold is not None else None
    ops.launch(ops.make_degrade_sepblur(x=x, taps=g, out=out, mask_out=mask, threshold=0.0 if threshold is None else float(threshold)))
    return out if threshold is None else (out, mask)


def usm_sharpen(x, weight: float = 0.5, threshold: float = 10, radius: int = 50):
    """`usm_sharpen_reference` on the device, three launches: the blur with its mask, the blur of the mask, the blend."""
    import torch
    from . import ops
    _check_device_batch(x, "usm_sharpen")
    g = _usm_taps(radius)
    blur, mask = sepblur(x, g, threshold)
    soft = sepblur(mask, g)
    out = torch.empty_like(x)
    ops.launch(ops.make_degrade_usm_apply(x=x, blur=blur, soft=soft, out=out, weight=float(weight)))
    return out


def degrade_batch2(hq, params: Sequence[Degrade2Params], seed: int, image_ids: Sequence[int], sizes: Optional[Sequence[Tuple[int, int]]] = None,
                   return_gt: bool = False):
    """The second-order chain on a batch: ``hq`` fp32 [B, 3, H, W] on the device (image b in the top-left ``sizes[b]`` of its slot), one
    `Degrade2Params` and one global id per image: USM (when `use_sharpener`) -> blur, resize, noise (draw 0), JPEG -> [blur], resize,
    noise (draw 1) -> [resize to (int(h / s2), int(w / s2)), sinc] and JPEG in the drawn order -> bicubic resize back (when
    `resize_back` and s2 != 1) -> clamp(rint(. 255)) / 255.  Returns one fp32 [3, h', w'] tensor per image (and the sharpened inputs,
    the reference's GT, with ``return_gt``).  Images that share every extent and launch-level choice (`_group_key2`) travel through the
    launches together; every other parameter travels per image, so an image's result does not depend on its companions.

    Two deviations from the reference, both on extents: its first resize is F.interpolate(scale_factor=), which maps coordinates
    with 1 / scale instead of in / out (edtr_hip.h explains why only explicit extents are offered); and intermediate extents are
    lowered to even numbers.  Where an extent is too small for a 21 x 21 kernel's reflect border, the blur is refused (ValueError)."""
    import torch
    from .rng import NoiseSource
    _check_device_batch(hq, "degrade_batch2")
    B = hq.shape[0]
    if len(params) != B or len(image_ids) != B:
        raise ValueError(f"{len(params)} parameter sets and {len(image_ids)} ids for a batch of {B}")
    sizes = [(int(h), int(w)) for h, w in sizes] if sizes is not None else [tuple(hq.shape[2:])] * B
    ids = [int(i) for i in image_ids]

    def gn(x, sigma, gray, who, draw, rounds=False):
        return add_gaussian_noise(x, sigma, gray, NoiseSource(seed, who), draw=draw, rounds=rounds)

    def pn(x, scale, gray, who, draw):
        return add_poisson_noise(x, scale, gray, NoiseSource(seed, who), draw=draw)

    ops2 = dict(filter2d=filter2d, resize=resize, gaussian=gn, poisson=pn, jpeg=jpeg, usm=usm_sharpen)
    lqs, gts = [None] * B, [None] * B
    for idx in _groups([_group_key2(sizes[b], p) for b, p in enumerate(params)]):
        h, w = sizes[idx[0]]
        x = torch.cat([hq[i:i + 1, :, :h, :w] for i in idx]).contiguous()
        lq, gt = _chain2(x, [params[i] for i in idx], ops2, [ids[i] for i in idx])
        for j, i in enumerate(idx):
            lqs[i], gts[i] = lq[j], gt[j]
    return (lqs, gts) if return_gt else lqs


def degrade_files(paths: Sequence[str], out_dir: str, cfg, seed: int, batch_size: int = 1, workers: int = 0, device=None,
                  geometry=None, masks: Optional[str] = None) -> List[Tuple[str, str]]:
    """Decode every file of ``paths`` (Pillow, RGB), degrade it with `draw_params(cfg, seed, k)` (`draw_params2` for a `RealESRGANConfig`)
    for its index k in ``paths`` and write ``out_dir``/gt/<stem>.png (the decoded image; the sharpened one where the configuration
    sharpens) and ``out_dir``/lq/<stem>.png.  Files are grouped by extent (`imageio.plan_buckets`)
    and cross the 8-bit boundary through `imageio.ingest` / `imageio.emit`; ``workers`` threads decode and encode.
    Returns [(gt path, lq path), ...].

    ``geometry`` (a `labels.SegGeometry`, a mapping or a YAML path with its keys): every decoded file first goes through the resize,
    pad, crop and flip of the reference's segmentation data sets (`labels.draw_geometry(geometry, seed, k, (h, w))` ->
    `labels.prepare_pair`), and gt/ holds the prepared image.  ``masks`` (a folder with <stem>.png label maps, read as
    np.array(Image.open(...)): palette indices, as the reference reads them): the mask goes through the same geometry and is written
    to ``out_dir``/mask/<stem>.png as mode "L".  Image ids and the degradation's draws are the same with and without either."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from . import imageio
    from .restore import MAX_WORKERS, _pillow
    Image = _pillow()
    cfg = load_config(cfg)
    if int(batch_size) <= 0 or int(workers) < 0:
        raise ValueError(f"batch_size must be positive and workers non-negative, got {batch_size} and {workers}")
    paths = list(paths)
    for sub in ("gt", "lq") + (("mask",) if masks is not None else ()):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    names = [(os.path.join(out_dir, "gt", s + ".png"), os.path.join(out_dir, "lq", s + ".png")) for s in stems]
    if geometry is not None or masks is not None:
        from . import labels
        geometry = None if geometry is None else labels.load_geometry(geometry)

    def header(path):
        with Image.open(path) as im:
            return im.size

    def decode(path):
        with Image.open(path) as im:
            return np.array(im.convert("RGB"), dtype=np.uint8)

    def decode_mask(stem):
        with Image.open(os.path.join(masks, stem + ".png")) as im:
            m = np.array(im)
        if m.dtype != np.uint8 or m.ndim != 2:
            raise ValueError(f"the mask of {stem} is not a uint8 label map (mode 'P' or 'L'), got {m.dtype} {m.shape}")
        return m

    def encode(arr, name):
        Image.fromarray(arr).save(name)

    pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)))
    try:
        wh = list(pool.map(header, paths))
        geoms = None if geometry is None else [labels.draw_geometry(geometry, seed, k, (h, w)) for k, (w, h) in enumerate(wh)]
        plan = imageio.plan_buckets([(h, w) for w, h in wh] if geoms is None else [g.out_hw for g in geoms], int(batch_size))
        jobs = []
        for _, idx in plan:
            raws = list(pool.map(decode, [paths[k] for k in idx]))
            if masks is not None:
                for k, m in zip(idx, pool.map(decode_mask, [stems[k] for k in idx])):
                    if geoms is not None:
                        m = labels.prepare_mask(m, geoms[k], device=device).cpu().numpy()
                    jobs.append(pool.submit(encode, m, os.path.join(out_dir, "mask", stems[k] + ".png")))
            if geoms is not None:
                # the prepared images stay on the device for the degradation; the host copies are what gt/ is written from
                prepared = [labels.prepare_image(raw, geoms[k], device=device) for k, raw in zip(idx, raws)]
                batch, sizes = imageio.ingest(prepared, device=device)
                raws = [p.cpu().numpy() for p in prepared]
            else:
                batch, sizes = imageio.ingest(raws, device=device)
            if isinstance(cfg, RealESRGANConfig):
                lqs, gts = degrade_batch2(batch, [draw_params2(cfg, seed, k) for k in idx], seed, idx, sizes, return_gt=True)
            else:
                lqs, gts = degrade_batch(batch, [draw_params(cfg, seed, k) for k in idx], seed, idx, sizes), None
            for j, (k, raw, lq) in enumerate(zip(idx, raws, lqs)):
                out = imageio.emit(lq[None].contiguous(), [tuple(lq.shape[1:])])[0].cpu().numpy()
                if gts is not None and cfg.use_sharpener:       # the reference's GT is the sharpened image
                    raw = imageio.emit(gts[j][None].contiguous(), [tuple(gts[j].shape[1:])])[0].cpu().numpy()
                jobs.append(pool.submit(encode, raw, names[k][0]))
                jobs.append(pool.submit(encode, out, names[k][1]))
        for j in jobs:
            j.result()
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
    return names


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m edtr_amd.degrade", description="Write gt/ and lq/ versions of a folder of images.")
    ap.add_argument("--input", required=True, help="folder of png / jpg images")
    ap.add_argument("--output", required=True, help="folder that receives gt/<stem>.png and lq/<stem>.png")
    ap.add_argument("--config", required=True, help=f"a YAML file with the reference's degradation keys, or one of {sorted(PRESETS) + ['realesrgan']}")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--workers", type=int, default=0)
    ap.add_argument("--geometry", default=None, help="a YAML file with the reference's segmentation geometry keys (gt_size, resize_range, "
                    "out_size, crop_type, hflip): resize, pad, crop and flip every image before it is degraded")
    ap.add_argument("--masks", default=None, help="folder of <stem>.png label maps: each goes through the same geometry into mask/<stem>.png")
    return ap


def main(argv=None) -> int:
    from .restore import list_images
    args = build_parser().parse_args(argv)
    paths = list_images(args.input)
    if not paths:
        print(f"no images in {args.input}", file=sys.stderr)
        return 1
    written = degrade_files(paths, args.output, args.config, args.seed, args.batch_size, args.workers, geometry=args.geometry, masks=args.masks)
    print(f"wrote {len(written)} gt / lq pairs to {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
