"""Low-quality inputs from high-quality ones, on the device: the blur -> resize -> Gaussian noise -> JPEG chain that the reference
applies on the CPU before every evaluation (one stage of RealESRGANBatchTransform, datasets/detection_cocov2.py:426-460; with a final
resize back to the input extent, the CodeFormer-style chain of datasets/detection.py:155-181).  Four launches of
include/edtr_hip.h "Low-quality inputs" (five with the resize back) on the fp32 NCHW batches that `imageio.ingest` writes.

    python -m edtr_amd.degrade --input DIR --output DIR --config YAML|codeformer|realesrgan-stage1 --seed N [--batch-size N --workers N]

writes ``gt/<stem>.png`` and ``lq/<stem>.png`` under the output folder, as the reference's generators do.

Three layers:
  * `filter2d`, `resize`, `add_gaussian_noise`, `jpeg`: thin wrappers over the launches (torch tensors on the device);
  * `*_reference`: the numpy restatement of each, operation for operation in fp32.  They are the NORMATIVE definition: the kernels are
    tested against them by equality, and they against the reference's own functions within its fp32 error (tests/golden/degrade.npz);
  * host-side parameter synthesis in numpy: the isotropic / anisotropic Gaussian, generalized Gaussian and plateau blur kernels and
    their mixture draw (our restatement of datasets/degradation.py:17-387), `DegradeConfig` with the reference's YAML keys, and
    `draw_params(cfg, seed, image_id)`, which draws one image's parameters from ``numpy.random.default_rng([seed, image_id])``.
    An image's low-quality version therefore depends on its bytes, the seed and its data-set index alone — not on the batch it
    travels in, the order, or the number of ranks: the promise `rng.NoiseSource` makes for the sampler's noise.

Left out: Poisson noise (torch.poisson has no stream that could be restated), the sinc filter, and USM sharpening (its kernel comes
from cv2).  The noise here is always Gaussian."""
from __future__ import annotations

import argparse
import math
import os
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .rng import PURPOSE_DEGRADE, PURPOSE_DEGRADE_GRAY, stream_reference

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
    sy, sx = _source_index(ih, oh), _source_index(iw, ow)
    if mode == "bilinear":
        y0, ty = _index_lambda(np.maximum(sy, F32(0)), ih)
        x0, tx = _index_lambda(np.maximum(sx, F32(0)), iw)
        y1, x1 = y0 + (y0 < ih - 1), x0 + (x0 < iw - 1)
        wy0, wx0 = (F32(1) - ty)[:, None], F32(1) - tx
        ty = ty[:, None]
        top = wx0 * x[:, :, y0][:, :, :, x0] + tx * x[:, :, y0][:, :, :, x1]
        bot = wx0 * x[:, :, y1][:, :, :, x0] + tx * x[:, :, y1][:, :, :, x1]
        return (wy0 * top + ty * bot).astype(F32)
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


def load_config(spec) -> DegradeConfig:
    """A `DegradeConfig`, the name of a preset, or the path of a YAML file with the keys."""
    if isinstance(spec, DegradeConfig):
        return spec
    if spec in PRESETS:
        return DegradeConfig(**PRESETS[spec])
    if not os.path.exists(spec):
        raise ValueError(f"--config must be one of {sorted(PRESETS)} or a YAML file, got {spec!r}")
    try:
        import yaml
    except ImportError as e:
        raise RuntimeError("reading a YAML configuration needs PyYAML (`import yaml` failed); the presets need nothing") from e
    with open(spec) as fh:
        return DegradeConfig.from_dict(yaml.safe_load(fh))


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
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
_DCT_TABLES: dict = {}


def _dct_on(device):
    import torch
    from .imageio import _device_key
    key = _device_key(device)
    if key not in _DCT_TABLES:
        _DCT_TABLES[key] = torch.from_numpy(dct_table()).to(device)
    return _DCT_TABLES[key]


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
    B = x.shape[0]
    sigma = [float(v) for v in np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(-1), (B,))]
    gray = [int(bool(v)) for v in np.broadcast_to(np.asarray(gray).reshape(-1), (B,))]
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


def degrade_files(paths: Sequence[str], out_dir: str, cfg, seed: int, batch_size: int = 1, workers: int = 0, device=None) -> List[Tuple[str, str]]:
    """Decode every file of ``paths`` (Pillow, RGB), degrade it with `draw_params(cfg, seed, k)` for its index k in ``paths`` and write
    ``out_dir``/gt/<stem>.png (the decoded image) and ``out_dir``/lq/<stem>.png.  Files are grouped by extent (`imageio.plan_buckets`)
    and cross the 8-bit boundary through `imageio.ingest` / `imageio.emit`; ``workers`` threads decode and encode.  The low-quality
    Returns [(gt path, lq path), ...]."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from . import imageio
    from .restore import MAX_WORKERS, _pillow
    Image = _pillow()
    cfg = load_config(cfg)
    if int(batch_size) <= 0 or int(workers) < 0:
        raise ValueError(f"batch_size must be positive and workers non-negative, got {batch_size} and {workers}")
    paths = list(paths)
    for sub in ("gt", "lq"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    names = [(os.path.join(out_dir, "gt", s + ".png"), os.path.join(out_dir, "lq", s + ".png")) for s in stems]

    def header(path):
        with Image.open(path) as im:
            return im.size

    def decode(path):
        with Image.open(path) as im:
            return np.array(im.convert("RGB"), dtype=np.uint8)

    def encode(arr, name):
        Image.fromarray(arr).save(name)

    pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)))
    try:
        wh = list(pool.map(header, paths))
        plan = imageio.plan_buckets([(h, w) for w, h in wh], int(batch_size))
        jobs = []
        for _, idx in plan:
            raws = list(pool.map(decode, [paths[k] for k in idx]))
            batch, sizes = imageio.ingest(raws, device=device)
            params = [draw_params(cfg, seed, k) for k in idx]
            lqs = degrade_batch(batch, params, seed, idx, sizes)
            for k, raw, lq in zip(idx, raws, lqs):
                out = imageio.emit(lq[None].contiguous(), [tuple(lq.shape[1:])])[0].cpu().numpy()
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
    ap.add_argument("--config", required=True, help=f"a YAML file with the reference's degradation keys, or one of {sorted(PRESETS)}")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--workers", type=int, default=0)
    return ap


def main(argv=None) -> int:
    from .restore import list_images
    args = build_parser().parse_args(argv)
    paths = list_images(args.input)
    if not paths:
        print(f"no images in {args.input}", file=sys.stderr)
        return 1
    written = degrade_files(paths, args.output, args.config, args.seed, args.batch_size, args.workers)
    print(f"wrote {len(written)} gt / lq pairs to {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
