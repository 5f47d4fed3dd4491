#!/usr/bin/env python
"""Isolated times of the 8-bit image boundary for a batch of eight 512 x 512 images (profiles/imageio_timing.json):

  in    eight uint8 1024 x 1024 images already on the device -> imageio.resize_u8 to 512 x 512 -> imageio.ingest into (8, 3, 512, 512)
  out   imageio.emit of an (8, 3, 512, 512) fp32 batch -> eight uint8 512 x 512 images
  host  Pillow's Image.resize((512, 512), BICUBIC) of the same eight images, for scale (not measured where Pillow is missing)

Device times are device events around ITERS repetitions after WARMUP repetitions, divided by ITERS: launch overhead of the 24 / 8
launches is inside them, uploads and downloads are not.  Recorded, not gated.

    python tools/bench_imageio.py [--out profiles/imageio_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, ITERS = 5, 50


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imageio_timing.json"))
    args = ap.parse_args()
    import torch
    from edtr_amd import imageio
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    raws = [np.random.default_rng(i).integers(0, 256, size=(1024, 1024, 3), dtype=np.uint8) for i in range(8)]
    srcs = [torch.from_numpy(a).to(dev) for a in raws]
    batch = torch.rand((8, 3, 512, 512), device=dev)

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

    result = {
        "workload": "eight images, 1024 x 1024 -> 512 x 512, batch (8, 3, 512, 512)",
        "method": f"device events around {ITERS} repetitions after {WARMUP} warm-up repetitions, per repetition; inputs resident on the "
                  "device, launch overhead included, copies excluded; Pillow timed with a host clock over 3 repetitions",
        "device": torch.cuda.get_device_name(0),
        "resize_u8_plus_ingest_us": timed(lambda: imageio.ingest([imageio.resize_u8(s, 512, 512) for s in srcs], size=(512, 512))),
        "resize_u8_us": timed(lambda: [imageio.resize_u8(s, 512, 512) for s in srcs]),
        "emit_us": timed(lambda: imageio.emit(batch, [(512, 512)] * 8)),
    }
    try:
        import PIL
        from PIL import Image
        ims = [Image.fromarray(a) for a in raws]
        t = time.perf_counter()
        for _ in range(3):
            for im in ims:
                im.resize((512, 512), Image.BICUBIC)
        result["host_pillow_resize_us"] = (time.perf_counter() - t) / 3 * 1e6
        result["pillow_version"] = PIL.__version__
    except ImportError:
        result["host_pillow_resize_us"] = None
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
