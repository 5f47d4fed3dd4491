"""Time the degradation stage (edtr_amd/degrade.py) on the device: each of the launches and the whole chains at batch 8 of
512 x 512 with 41 x 41 blur kernels, next to the same operations as the reference performs them — torch on the host CPU
(F.pad + grouped F.conv2d as filter2D, F.interpolate, randn-based noise, DiffJPEG's tensordot formulation) — in the same call.
Writes profiles/degrade_timing.json; commit that file only after this has run on the device.

    python tools/bench_degrade.py [--batch 8] [--size 512] [--kernel 41] [--iters 20] [--cpu-iters 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from edtr_amd import degrade, ops  # noqa: E402
from edtr_amd.build import source_hash  # noqa: E402
from edtr_amd.rng import NoiseSource  # noqa: E402


def gpu_ms(fn, iters: int) -> float:
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def cpu_ms(fn, iters: int) -> float:
    fn()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t) * 1e3 / iters


def cpu_filter2d(x, k):
    b, c, h, w = x.shape
    r = k.shape[-1] // 2
    p = F.pad(x, (r, r, r, r), mode="reflect").view(1, b * c, h + 2 * r, w + 2 * r)
    return F.conv2d(p, k.view(b, 1, *k.shape[1:]).repeat(1, c, 1, 1).view(b * c, 1, *k.shape[1:]), groups=b * c).view(b, c, h, w)


def cpu_noise(x, sigma):
    return torch.clamp(x + torch.randn_like(x) * sigma.view(-1, 1, 1, 1) / 255.0, 0, 1)


def cpu_jpeg(x, quality):
    """DiffJPEG's formulation (tensordot per stage) on CPU tensors, extents multiples of 16"""
    T = torch.from_numpy(degrade.dct_table()).view(8, 8, 8, 8)
    factor = torch.from_numpy(degrade.quality_to_factor(quality)).view(-1, 1, 1, 1)
    scale, alpha = torch.from_numpy(degrade.DCT_SCALE), torch.from_numpy(degrade.DCT_ALPHA)
    ycc = torch.tensordot((x * 255).permute(0, 2, 3, 1), torch.from_numpy(degrade.RGB2YCC).T, dims=1) + torch.tensor([0.0, 128.0, 128.0])
    planes = [ycc[..., 0]] + [F.avg_pool2d(ycc[..., c].unsqueeze(1), 2).squeeze(1) for c in (1, 2)]
    rec = []
    for c, p in enumerate(planes):
        B, h, w = p.shape
        blocks = p.view(B, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4).reshape(B, -1, 8, 8)
        table = torch.from_numpy(degrade.Y_TABLE if c == 0 else degrade.C_TABLE) * factor
        q = torch.round(scale * torch.tensordot(blocks - 128, T, dims=2) / table)
        pix = 0.25 * torch.tensordot(q * table * alpha, T.permute(2, 3, 0, 1), dims=2) + 128
        rec.append(pix.view(B, h // 8, w // 8, 8, 8).permute(0, 1, 3, 2, 4).reshape(B, h, w))
    up = lambda a: a.repeat_interleave(2, 1).repeat_interleave(2, 2)
    img = torch.stack([rec[0], up(rec[1]) - 128, up(rec[2]) - 128], dim=3)
    return (torch.tensordot(img, torch.from_numpy(degrade.YCC2RGB).T, dims=1).clamp(0, 255) / 255).permute(0, 3, 1, 2)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--kernel", type=int, default=41)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-iters", type=int, default=2)
    ap.add_argument("--cpu-threads", type=int, default=16)
    args = ap.parse_args()
    torch.set_num_threads(args.cpu_threads)
    B, S, K = args.batch, args.size, args.kernel
    lq = S // 4
    gen = np.random.default_rng(0)
    hq = torch.from_numpy(gen.random((B, 3, S, S), dtype=np.float32))
    kern = torch.from_numpy(np.stack([degrade.random_mixed_kernel(gen, ["iso", "aniso"], [0.5, 0.5], K, (0.1, 8.0)) for _ in range(B)]).astype(np.float32))
    sigma, gray = gen.uniform(0, 10, B).astype(np.float32), [0] * B
    quality = gen.uniform(50, 99, B).astype(np.float32)
    src = NoiseSource(0, range(B))
    d_hq, d_k = hq.cuda(), kern.cuda()
    d_lq = degrade.resize(degrade.filter2d(d_hq, d_k), (lq, lq), "bilinear")
    c_lq = d_lq.cpu()

    def chain():
        x = degrade.resize(degrade.filter2d(d_hq, d_k), (lq, lq), "bilinear")
        x = degrade.jpeg(degrade.add_gaussian_noise(x, sigma, gray, src), quality)
        return degrade.resize(x, (S, S), "bilinear")

    def cpu_chain():
        x = F.interpolate(cpu_filter2d(hq, kern), size=(lq, lq), mode="bilinear")
        x = cpu_jpeg(cpu_noise(x, torch.from_numpy(sigma)), quality)
        return F.interpolate(x, size=(S, S), mode="bilinear")

    gpu = {
        "filter2d": gpu_ms(lambda: degrade.filter2d(d_hq, d_k), args.iters),
        "resize_down_bilinear": gpu_ms(lambda: degrade.resize(d_hq, (lq, lq), "bilinear"), args.iters),
        "resize_down_bicubic": gpu_ms(lambda: degrade.resize(d_hq, (lq, lq), "bicubic"), args.iters),
        "resize_down_area": gpu_ms(lambda: degrade.resize(d_hq, (lq, lq), "area"), args.iters),
        "resize_back_bilinear": gpu_ms(lambda: degrade.resize(d_lq, (S, S), "bilinear"), args.iters),
        "gaussian_noise_full_size": gpu_ms(lambda: degrade.add_gaussian_noise(d_hq, sigma, gray, src), args.iters),
        "jpeg_full_size": gpu_ms(lambda: degrade.jpeg(d_hq, quality), args.iters),
        "chain": gpu_ms(chain, args.iters),
    }
    # the second-order chain (degrade.degrade_batch2): its three new launches, the separable blur beside the 2-D launch with the same
    # (outer-product) kernel at k = 41 — 82 taps against 1681 — and the whole chain with the parameters of the "realesrgan" preset
    g41 = degrade.gaussian_taps(41).astype(np.float32)
    d_outer = torch.from_numpy(np.outer(g41, g41).astype(np.float32)[None]).cuda()
    g51 = degrade.gaussian_taps(51).astype(np.float32)
    d_blur = degrade.sepblur(d_hq, g51)
    d_soft = degrade.sepblur(d_blur, g51)
    scale = gen.uniform(0.05, 3.0, B).astype(np.float32)
    cfg2 = degrade.load_config("realesrgan")
    params2 = [degrade.draw_params2(cfg2, 0, i) for i in range(B)]
    degrade.poisson_tables_on(d_hq.device)
    gpu2 = {
        "poisson_noise_full_size": gpu_ms(lambda: degrade.add_poisson_noise(d_hq, scale, gray, src), args.iters),
        "poisson_noise_grey_full_size": gpu_ms(lambda: degrade.add_poisson_noise(d_hq, scale, [1] * B, src), args.iters),
        "sepblur_k51_with_mask": gpu_ms(lambda: degrade.sepblur(d_hq, g51, 10.0), args.iters),
        "usm_apply": gpu_ms(lambda: ops.launch(ops.make_degrade_usm_apply(x=d_hq, blur=d_blur, soft=d_soft, out=d_soft, weight=0.5)), args.iters),
        "usm_sharpen": gpu_ms(lambda: degrade.usm_sharpen(d_hq), args.iters),
        "sepblur_k41": gpu_ms(lambda: degrade.sepblur(d_hq, g41), args.iters),
        "filter2d_k41_outer_product": gpu_ms(lambda: degrade.filter2d(d_hq, d_outer), args.iters),
        "chain2_realesrgan_preset": gpu_ms(lambda: degrade.degrade_batch2(d_hq, params2, 0, range(B)), args.iters),
    }
    cpu = {
        "filter2d": cpu_ms(lambda: cpu_filter2d(hq, kern), args.cpu_iters),
        "resize_down_bilinear": cpu_ms(lambda: F.interpolate(hq, size=(lq, lq), mode="bilinear"), args.cpu_iters),
        "resize_down_bicubic": cpu_ms(lambda: F.interpolate(hq, size=(lq, lq), mode="bicubic"), args.cpu_iters),
        "resize_down_area": cpu_ms(lambda: F.interpolate(hq, size=(lq, lq), mode="area"), args.cpu_iters),
        "resize_back_bilinear": cpu_ms(lambda: F.interpolate(c_lq, size=(S, S), mode="bilinear"), args.cpu_iters),
        "gaussian_noise_full_size": cpu_ms(lambda: cpu_noise(hq, torch.from_numpy(sigma)), args.cpu_iters),
        "jpeg_full_size": cpu_ms(lambda: cpu_jpeg(hq, quality), args.cpu_iters),
        "chain": cpu_ms(cpu_chain, args.cpu_iters),
    }
    out = {"batch": B, "size": S, "kernel": K, "lq_size": lq, "device": torch.cuda.get_device_name(0), "source_hash": source_hash(),
           "cpu_threads": args.cpu_threads, "unit": "ms per call (the GPU figures include the wrappers' allocations and uploads)",
           "gpu_ms": gpu, "second_order_gpu_ms": gpu2, "host_cpu_torch_ms": cpu, "speedup": {k: cpu[k] / gpu[k] for k in gpu}}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "degrade_timing.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
