"""Write tests/golden/degrade.npz: inputs, parameters and outputs of the REFERENCE's degradation functions on the CPU — filter2D
(datasets/utils.py), F.interpolate, add_gaussian_noise_pt (datasets/degradation.py; its torch.randn supplied from our seeded stream),
DiffJPEG (datasets/diffjpeg.py) and the blur-kernel formulas — for tests/test_degrade_cpu.py and tests/test_gpu_degrade.py.

Every tolerance a test uses is measured here and stored beside the data: the reference's fp32 output against an fp64 evaluation of
the same formula on the same fixture, times 4 for a different summation order.  The JPEG fixture must not depend on summation order
at all: a seed is kept only if every quotient before rounding, evaluated in fp64, is at least JPEG_MARGIN from a rounding boundary;
the margin found and the fp32-against-fp64 quotient error are stored too.

    python tools/make_degrade_goldens.py           (needs the reference tree; see tools/ref_import.py)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ref_import  # noqa: E402
from edtr_amd import degrade  # noqa: E402

JPEG_MARGIN = 1e-4
ORDER = 4.0                 # a tolerance = ORDER * (the reference's own fp32 error): room for another summation order
NOISE_SEED, NOISE_IDS, NOISE_SIGMA, NOISE_GRAY = 2024, [5, 0, 2 ** 32 - 1], [5.0, 20.0, 0.5], [0, 1, 0]
RESIZE_SIZES = [(7, 9), (24, 40), (37, 61)]
KERNEL_CASES = [("iso", 21, 2.0, 2.0, 0.0, 1.0), ("aniso", 21, 2.0, 3.5, 0.7, 1.0), ("generalized_aniso", 21, 1.5, 2.5, -0.4, 1.7),
                ("plateau_aniso", 21, 1.2, 2.2, 1.1, 1.5), ("generalized_iso", 13, 1.8, 1.8, 0.0, 0.6), ("plateau_iso", 13, 2.4, 2.4, 0.0, 1.9)]


def err(a, b) -> float:
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def jpeg_fp64(x: np.ndarray, quality: np.ndarray):
    """The JPEG formula with the reference's fp32 parameters and fp64 arithmetic: (image, quotients before rounding), both fp64, the
    quotients in degrade.jpeg_reference's layout"""
    B, _, H, W = x.shape
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    p = np.zeros((B, 3, Hp, Wp))
    p[:, :, :H, :W] = x.astype(np.float64) * 255.0
    ycc = np.einsum("bchw,dc->bdhw", p, degrade.RGB2YCC.astype(np.float64)) + np.array([0.0, 128.0, 128.0]).reshape(1, 3, 1, 1)
    pool = lambda a: (a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]) / 4.0
    planes = [ycc[:, 0], pool(ycc[:, 1]), pool(ycc[:, 2])]
    T = degrade.dct_table().astype(np.float64)
    factor = degrade.quality_to_factor(quality).astype(np.float64).reshape(B, 1, 1)
    quots, rec = [], []
    for c, plane in enumerate(planes):
        d = degrade._split(plane - 128.0)
        tq = (degrade.Y_TABLE if c == 0 else degrade.C_TABLE).astype(np.float64).reshape(1, 1, 64) * factor
        quot = degrade.DCT_SCALE.astype(np.float64).reshape(1, 1, 64) * (d @ T) / tq
        quots.append(quot)
        pix = 0.25 * ((np.rint(quot) * tq * degrade.DCT_ALPHA.astype(np.float64).reshape(1, 1, 64)) @ T.T) + 128.0
        rec.append(degrade._merge(pix, *((Hp, Wp) if c == 0 else (Hp // 2, Wp // 2))))
    up = lambda a: np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)
    img = np.stack([rec[0], up(rec[1]) - 128.0, up(rec[2]) - 128.0], axis=1)
    out = np.einsum("bchw,dc->bdhw", img, degrade.YCC2RGB.astype(np.float64))
    return (np.clip(out, 0.0, 255.0) / 255.0)[:, :, :H, :W], np.concatenate(quots, axis=1)


def main() -> int:
    ref_import.install_degrade_stubs()
    utils = ref_import.import_reference_file("ref_datasets_utils", "datasets/utils.py")
    degr = ref_import.import_reference_file("ref_datasets_degradation", "datasets/degradation.py")
    djpg = ref_import.import_reference_file("ref_datasets_diffjpeg", "datasets/diffjpeg.py")
    out = {}
    torch.manual_seed(0)

    # ---- blur kernels: the reference's formulas with fixed arguments --------------------------------------------------------------
    for n, (kind, size, sx, sy, theta, beta) in enumerate(KERNEL_CASES):
        iso = kind.endswith("_iso") or kind == "iso"
        if kind in ("iso", "aniso"):
            k = degr.bivariate_Gaussian(size, sx, sy, theta, isotropic=iso)
        elif kind.startswith("generalized"):
            k = degr.bivariate_generalized_Gaussian(size, sx, sy, theta, beta, isotropic=iso)
        else:
            k = degr.bivariate_plateau(size, sx, sy, theta, beta, isotropic=iso)
        out[f"kernel{n}"] = np.asarray(k, dtype=np.float64)
    out["kernel_args"] = np.array([[s, sx, sy, th, be] for _, s, sx, sy, th, be in KERNEL_CASES], dtype=np.float64)
    out["kernel_kinds"] = np.array([c[0] for c in KERNEL_CASES])

    # ---- filter2D: per-image 13 x 13 kernels and one shared 3 x 3 kernel on 2 x 3 x 20 x 28 ---------------------------------------
    x = torch.rand(2, 3, 20, 28)
    k13 = torch.from_numpy(np.stack([degr.bivariate_Gaussian(13, 2.0, 3.5, 0.7, isotropic=False),
                                     degr.bivariate_Gaussian(13, 1.1, 1.1, 0.0, isotropic=True)])).float()
    k3 = torch.from_numpy(degr.bivariate_Gaussian(3, 0.8, 0.8, 0.0, isotropic=True)).float()[None]
    out["filter_x"], out["filter_k13"], out["filter_k3"] = x.numpy(), k13.numpy(), k3.numpy()
    tol = 0.0
    for name, k in (("13", k13), ("3", k3)):
        got = utils.filter2D(x, k).numpy()
        tol = max(tol, err(got, utils.filter2D(x.double(), k.double()).numpy()))
        out[f"filter_out{name}"] = got
    out["filter_ref_err"], out["filter_tol"] = np.float64(tol), np.float64(ORDER * tol)

    # ---- F.interpolate(size=): three modes x (extreme downscale, identity, upscale) on 2 x 3 x 24 x 40 -----------------------------
    x = torch.rand(2, 3, 24, 40)
    out["resize_x"], out["resize_sizes"] = x.numpy(), np.array(RESIZE_SIZES, dtype=np.int64)
    for mode in degrade.MODES:
        tol = 0.0
        for n, size in enumerate(RESIZE_SIZES):
            got = F.interpolate(x, size=size, mode=mode).numpy()
            tol = max(tol, err(got, F.interpolate(x.double(), size=size, mode=mode).numpy()))
            out[f"resize_{mode}_{n}"] = got
        out[f"resize_{mode}_ref_err"], out[f"resize_{mode}_tol"] = np.float64(tol), np.float64(ORDER * tol)

    # ---- add_gaussian_noise_pt, image by image, torch.randn answered from the seeded stream ----------------------------------------
    x = torch.rand(3, 3, 8, 12)
    noise = degrade.degrade_noise_reference(NOISE_SEED, NOISE_IDS, NOISE_GRAY, 0, 8, 12).astype(np.float32)
    got = []
    real_randn = torch.randn
    for b in range(3):
        queue = [torch.from_numpy(noise[b, 0].copy())] if NOISE_GRAY[b] else []       # (the grey plane is drawn first, as [h, w])
        queue.append(torch.from_numpy(noise[b:b + 1].copy()))
        torch.randn = lambda *size, **kw: queue.pop(0)
        try:
            got.append(degr.add_gaussian_noise_pt(x[b:b + 1], sigma=torch.tensor([NOISE_SIGMA[b]]), gray_noise=torch.tensor([float(NOISE_GRAY[b])]),
                                                  clip=True, rounds=False))
        finally:
            torch.randn = real_randn
        assert not queue
    out["noise_x"], out["noise_n"], out["noise_out"] = x.numpy(), noise, torch.cat(got).numpy()
    out["noise_seed"], out["noise_ids"] = np.int64(NOISE_SEED), np.array(NOISE_IDS, dtype=np.int64)
    out["noise_sigma"], out["noise_gray"] = np.array(NOISE_SIGMA, dtype=np.float32), np.array(NOISE_GRAY, dtype=np.int32)

    # ---- DiffJPEG at qualities 35 and 90 on torch.rand(2, 3, 24, 40): the first seed whose quotients keep the margin ----------------
    quality = np.array([35.0, 90.0], dtype=np.float32)
    jpeger = djpg.DiffJPEG(differentiable=False)
    seen = []

    def recording_round(t):
        seen.append(t.detach().clone())
        return torch.round(t)

    jpeger.compress.y_quantize.rounding = recording_round
    jpeger.compress.c_quantize.rounding = recording_round
    for seed in range(64):
        x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(seed))
        img64, quot64 = jpeg_fp64(x.numpy(), quality)
        margin = float(np.abs(np.abs(quot64 - np.floor(quot64)) - 0.5).min())
        if margin < JPEG_MARGIN:
            print(f"  jpeg seed {seed}: margin {margin:.2e} < {JPEG_MARGIN:g}, skipped")
            continue
        del seen[:]
        with torch.no_grad():
            got = jpeger(x, quality=torch.from_numpy(quality.copy())).numpy()
        quot32 = torch.cat([s.reshape(2, -1, 64) for s in seen], dim=1).numpy()      # (y, cb, cr: the order CompressJpeg walks)
        flips = int((np.rint(quot32) != np.rint(quot64)).sum())
        print(f"  jpeg seed {seed}: margin {margin:.2e}, fp32 quotient error {err(quot32, quot64):.2e}, {flips} of {quot32.size} coefficients differ")
        assert flips == 0
        out["jpeg_x"], out["jpeg_quality"], out["jpeg_out"] = x.numpy(), quality, got
        out["jpeg_coefs"] = np.rint(quot32).astype(np.float32)
        out["jpeg_seed"], out["jpeg_margin"], out["jpeg_quot_err"] = np.int64(seed), np.float64(margin), np.float64(err(quot32, quot64))
        out["jpeg_ref_err"] = np.float64(err(got, img64))
        out["jpeg_tol"] = np.float64(ORDER * err(got, img64))
        break
    else:
        raise SystemExit("no seed keeps the JPEG margin")

    path = os.path.join(ROOT, "tests", "golden", "degrade.npz")
    np.savez_compressed(path, **out)
    for k in sorted(out):
        if k.endswith(("_tol", "_err", "_margin")):
            print(f"  {k} = {float(out[k]):.3e}")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
