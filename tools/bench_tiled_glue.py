#!/usr/bin/env python
"""Times of the glue around one tiled network evaluation (profiles/tiled_glue_timing.json), old sequence against window table:

  old   per denoise step: torch.cat of the n window slices, two zeroed planes, n edtr_tile_accumulate launches, one edtr_divide
  new   one edtr_tile_gather, one edtr_tile_blend
  at    1 x 4 x 128 x 128 with 64 / 32 windows (the latent of the seg1024tiled workload: 9 windows)
        1 x 3 x 1024 x 1024 with 512 / 256 windows (SwinIR per window on a 1024 x 1024 image: 9 windows)

and of the seg1024tiled workload through `workloads.restore_pass` (one 1024 x 1024 image, bf16, the synthetic SD-2.1 model), eager
passes on one stream: a host clock around PASSES passes that end in a device synchronise.  ``--against DIR`` times the same workload
from another checkout of this package (the parent commit, built in DIR) in fresh processes alternating with this one, ROUNDS times
each, so that both numbers come from one device in one call.

Glue times are device events around ITERS repetitions after WARMUP, alternating old and new over ROUNDS rounds; the median round is
reported with the spread.  Launch overhead is inside them (it is what the change removes), the network evaluation is not.
Recorded, not gated.

    python tools/bench_tiled_glue.py [--against DIR] [--out profiles/tiled_glue_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, ITERS, ROUNDS = 5, 50, 5
PASSES, PASS_WARMUP = 12, 3
GLUE_SHAPES = [((1, 4, 128, 128), 64, 32), ((1, 3, 1024, 1024), 512, 256)]


def seg1024tiled_ms(root: str) -> float:
    """ms per eager seg1024tiled pass with the package found under ``root`` (called in a fresh process per measurement)."""
    sys.path.insert(0, root)
    import torch
    from edtr_amd import synth, workloads
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    dev = torch.device("cuda:0")
    cfg = synth.sd21_config()
    cldm = build_synthetic_cldm(cfg, dev, torch.bfloat16)
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(dev)
    sampler = SpacedSampler(diffusion.betas)
    B, S, _ = workloads.WORKLOADS["seg1024tiled"]
    inp = workloads.make_inputs("seg1024tiled", cfg["unet_cfg"]["context_dim"], dev, B, S)
    untiled = type(cldm).forward.__get__(cldm)

    def run(n):
        for _ in range(n):
            workloads.restore_pass(cldm, diffusion, sampler, inp, "seg1024tiled", untiled, inject=False)
        torch.cuda.synchronize()

    run(PASS_WARMUP)
    t0 = time.perf_counter()
    run(PASSES)
    return (time.perf_counter() - t0) / PASSES * 1e3


def glue_times(dev) -> dict:
    import torch
    from edtr_amd import ops, tiling
    out = {}
    for shape, size, stride in GLUE_SHAPES:
        b, c, h, w = shape
        x = torch.rand(shape, device=dev)
        tab = tiling.device_windows(h, w, size, stride, dev)
        wts = torch.tensor(tiling.gaussian_weights(size, size), dtype=torch.float32, device=dev)
        ys = tiling.gather_windows(x, tab, size)                     # stands for the network's output on the stacked windows

        def old():
            xs = torch.cat([x[..., hi:he, wi:we] for hi, he, wi, we in tab.windows], dim=0)
            num = torch.zeros(shape, dtype=torch.float32, device=dev)
            den = torch.zeros_like(num)
            for k, (hi, _, wi, _) in enumerate(tab.windows):
                ops.launch(ops.make_tile_accumulate(tile=ys[k * b:(k + 1) * b], wts=wts, out=num, count=den, B=b, C=c, H=h, W=w,
                                                    th=size, tw=size, hi=hi, wi=wi))
            res = torch.empty_like(num)
            ops.launch(ops.make_divide(num=num, den=den, out=res, n=num.numel()))
            return xs, res

        def new():
            xs = tiling.gather_windows(x, tab, size)
            res = torch.empty(shape, dtype=torch.float32, device=dev)
            ops.launch(ops.make_tile_blend(tiles=ys, wts=wts, table_host=tab.host, table=tab.device, th=size, tw=size, out=res))
            return xs, res

        (xo, ro), (xn, rn) = old(), new()
        torch.cuda.synchronize()
        same = bool(torch.equal(xo, xn) and torch.equal(ro.view(torch.int32), rn.view(torch.int32)))

        def timed(fn):
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(ITERS):
                fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) * 1e3 / ITERS          # us

        rounds = [(timed(old), timed(new)) for _ in range(ROUNDS)]
        o, n = [r[0] for r in rounds], [r[1] for r in rounds]
        out["x".join(map(str, shape)) + f"_{size}_{stride}"] = {
            "windows": tab.n, "same_bits": same,
            "old_us_per_step": {"median": statistics.median(o), "min": min(o), "max": max(o)},
            "new_us_per_step": {"median": statistics.median(n), "min": min(n), "max": max(n)}}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_glue_timing.json"))
    ap.add_argument("--against", default=None, help="another checkout of this package, built: its seg1024tiled passes are timed too")
    ap.add_argument("--seg-child", default=None, help=argparse.SUPPRESS)          # a measurement process: print ms per pass for this root
    args = ap.parse_args()
    if args.seg_child:
        print("SEG1024TILED_MS " + json.dumps(seg1024tiled_ms(args.seg_child)))
        return 0
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")

    def child(root):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--seg-child", root], capture_output=True, text=True, timeout=900, cwd=root)
        if r.returncode != 0:
            raise SystemExit(f"the seg1024tiled measurement under {root} failed:\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SEG1024TILED_MS ")][-1].split(" ", 1)[1])

    result = {
        "device": torch.cuda.get_device_name(0),
        "method": f"glue: device events around {ITERS} repetitions after {WARMUP} warm-up repetitions, old and new alternating over {ROUNDS} "
                  f"rounds, per step, launch overhead included; seg1024tiled: host clock around {PASSES} eager passes of "
                  f"workloads.restore_pass ending in a device synchronise, after {PASS_WARMUP} warm-up passes, a fresh process per figure",
        "glue": glue_times(dev),
    }
    rounds = 2 if args.against else 1
    mine, theirs = [], []
    for _ in range(rounds):                                   # alternating, one process at a time
        mine.append(child(ROOT))
        if args.against:
            theirs.append(child(os.path.abspath(args.against)))
    seg = {"this_tree_ms_per_pass": mine}
    if args.against:
        seg["parent_ms_per_pass"] = theirs
        seg["this_over_parent"] = statistics.mean(mine) / statistics.mean(theirs)
    result["seg1024tiled"] = seg
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
