"""Write tests/golden/degrade2.npz: inputs and outputs of the REFERENCE's functions of the second-order chain on the CPU —
circular_lowpass_kernel and add_poisson_noise_pt (datasets/degradation.py) and USMSharp (datasets/utils.py) — for
tests/test_degrade2_cpu.py and tests/test_gpu_degrade2.py.  Data only.

Every tolerance a test uses is measured here and stored beside the data: the reference's fp32 output against an fp64 evaluation of
the same formula on the same fixture, times ORDER for a different summation order.  The USM fixture must not depend on summation
order at its threshold: a seed is kept only if every |residual| * 255, evaluated in fp64, is at least USM_MARGIN from the threshold
(the method of the JPEG fixture of tools/make_degrade_goldens.py); the margin found is stored.  torch.poisson has no stream of its
own that could be restated, so it is answered from our table sampler (`degrade.poisson_reference`), as that tool answers torch.randn.

    python tools/make_degrade2_goldens.py           (needs the reference tree; see tools/ref_import.py)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ref_import  # noqa: E402
from edtr_amd import degrade, rng  # noqa: E402

ORDER = 4.0
USM_MARGIN = 1e-3           # in units of 1/255, as the threshold
SINC_CASES = [(7, 2.0), (13, 1.1), (21, 2.9)]
P_SEED, P_IDS, P_SCALE, P_GRAY = 2024, [5, 0, 2 ** 32 - 1], [1.5, 0.8, 2.5], [0, 1, 0]


def err(a, b) -> float:
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def poisson_fixture() -> np.ndarray:
    """3 x 3 x 16 x 24: image 0 a ramp over all 256 levels, image 1 five grey levels, image 2 constant"""
    x = np.empty((3, 3, 16, 24), dtype=np.float32)
    ramp = (np.arange(3 * 16 * 24) % 256).astype(np.float32) / np.float32(255.0)
    x[0] = ramp.reshape(3, 16, 24)
    x[1] = (np.array([0, 64, 128, 191, 255], dtype=np.float32)[np.arange(16 * 24) % 5] / np.float32(255.0)).reshape(1, 16, 24)
    x[2] = np.float32(0.4)
    return x


def usm_fp64(x: np.ndarray, kernel2d: np.ndarray, weight: float, threshold: float):
    """USMSharp.forward with the reference's fp32 kernel and fp64 arithmetic: (result, |residual| * 255)"""
    x = x.astype(np.float64)
    k = kernel2d.astype(np.float64)
    r = k.shape[0] // 2

    def blur(a):
        pad = np.pad(a, ((0, 0), (0, 0), (r, r), (r, r)), mode="reflect")
        out = np.zeros_like(a)
        for ky in range(k.shape[0]):
            for kx in range(k.shape[1]):
                out += pad[:, :, ky:ky + a.shape[2], kx:kx + a.shape[3]] * k[ky, kx]
        return out

    residual = x - blur(x)
    mask = (np.abs(residual) * 255 > threshold).astype(np.float64)
    soft = blur(mask)
    sharp = np.clip(x + weight * residual, 0, 1)
    return soft * sharp + (1 - soft) * x, np.abs(residual) * 255


def main() -> int:
    ref_import.install_degrade2_stubs()
    utils = ref_import.import_reference_file("ref_datasets_utils", "datasets/utils.py")
    degr = ref_import.import_reference_file("ref_datasets_degradation", "datasets/degradation.py")
    out = {}

    # ---- circular_lowpass_kernel at sizes 7, 13, 21, with and without pad_to=21 ------------------------------------------------------
    out["sinc_args"] = np.array(SINC_CASES, dtype=np.float64)
    for n, (size, cutoff) in enumerate(SINC_CASES):
        out[f"sinc{n}"] = np.asarray(degr.circular_lowpass_kernel(cutoff, size, pad_to=False), dtype=np.float64)
        out[f"sinc{n}_pad"] = np.asarray(degr.circular_lowpass_kernel(cutoff, size, pad_to=21), dtype=np.float64)

    # ---- USMSharp on 2 x 3 x 40 x 70: the first seed whose residuals keep the margin from the threshold --------------------------------
    sharpener = utils.USMSharp()
    kernel2d = sharpener.kernel[0].numpy()
    assert kernel2d.shape == (51, 51)
    for seed in range(64):
        x = torch.rand(2, 3, 40, 70, generator=torch.Generator().manual_seed(seed))
        want64, res64 = usm_fp64(x.numpy(), kernel2d, 0.5, 10)
        margin = float(np.abs(res64 - 10).min())
        if margin < USM_MARGIN:
            print(f"  usm seed {seed}: margin {margin:.2e} < {USM_MARGIN:g}, skipped")
            continue
        with torch.no_grad():
            got = sharpener(x, weight=0.5, threshold=10).numpy()
        out["usm_x"], out["usm_out"], out["usm_seed"], out["usm_margin"] = x.numpy(), got, np.int64(seed), np.float64(margin)
        out["usm_ref_err"], out["usm_tol"] = np.float64(err(got, want64)), np.float64(ORDER * err(got, want64))
        print(f"  usm seed {seed}: margin {margin:.2e}")
        break
    else:
        raise SystemExit("no seed keeps the USM margin")

    # ---- add_poisson_noise_pt, image by image, torch.poisson answered from the table sampler -------------------------------------------
    x = poisson_fixture()
    kc, kg = degrade.poisson_levels(x)
    counts = degrade.level_counts(x)
    got, want64 = [], []
    real_poisson = torch.poisson
    for b in range(3):
        vc, vg = degrade.vals_of(counts[b, 0]), degrade.vals_of(counts[b, 1])
        nc = degrade.poisson_reference(P_SEED, [P_IDS[b]], rng.PURPOSE_DEGRADE_POISSON, 0, kc[b].reshape(1, -1), [vc]).reshape(1, 3, 16, 24)
        ng = degrade.poisson_reference(P_SEED, [P_IDS[b]], rng.PURPOSE_DEGRADE_POISSON_GRAY, 0, kg[b].reshape(1, -1), [vg]).reshape(1, 1, 16, 24)
        queue = ([torch.from_numpy(ng.astype(np.float32))] if P_GRAY[b] else []) + [torch.from_numpy(nc.astype(np.float32))]
        rates = []

        def fake_poisson(rate, generator=None):
            rates.append(rate.clone())
            return queue.pop(0)

        torch.poisson = fake_poisson
        try:
            got.append(degr.add_poisson_noise_pt(torch.from_numpy(x[b:b + 1]), scale=torch.tensor([P_SCALE[b]]),
                                                 gray_noise=torch.tensor([float(P_GRAY[b])]), clip=True, rounds=False).numpy())
        finally:
            torch.poisson = real_poisson
        assert not queue
        # the rate the reference hands to torch.poisson is the table's lambda: level / 255 * vals in fp32
        k, v = (kg[b][None, None], vg) if P_GRAY[b] else (kc[b][None], vc)
        assert np.array_equal(rates[0].numpy(), (k.astype(np.float32) / np.float32(255.0)) * np.float32(v))
        n = (ng if P_GRAY[b] else nc).astype(np.float64)
        noise64 = n / v - k.astype(np.float64) / 255.0
        want64.append(np.clip(x[b:b + 1].astype(np.float64) + noise64 * np.float64(np.float32(P_SCALE[b])), 0.0, 1.0))
    got, want64 = np.concatenate(got), np.concatenate(want64)
    out["poisson_x"], out["poisson_out"], out["poisson_counts"] = x, got, counts
    out["poisson_seed"], out["poisson_ids"] = np.int64(P_SEED), np.array(P_IDS, dtype=np.int64)
    out["poisson_scale"], out["poisson_gray"] = np.array(P_SCALE, dtype=np.float32), np.array(P_GRAY, dtype=np.int32)
    e = err(got, want64)
    out["poisson_ref_err"], out["poisson_tol"] = np.float64(e), np.float64(ORDER * e)

    path = os.path.join(ROOT, "tests", "golden", "degrade2.npz")
    np.savez_compressed(path, **out)
    for k in sorted(out):
        if k.endswith(("_tol", "_err", "_margin")):
            print(f"  {k} = {float(out[k]):.3e}")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
