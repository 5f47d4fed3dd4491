"""Files per second of `edtr_amd.restore.restore_files` on a folder of synthetic 8-bit images of mixed sizes (seeded, written to a
temporary directory; nothing outside the repository is read), at batch_size 1 and 8 with workers 0 and 8, on the tiny synthetic model
and on the SD-2.1-width synthetic model, plus the launches and milliseconds of the 8-bit boundary alone for one batch of eight.

    python tools/bench_restore_files.py --label this [--models tiny,sd21] [--images 16] [--out profiles/restore_files_timing.json]

Results are merged into the JSON under ``--label``, so that a run of a checkout of the parent commit (whose restore_files has no
batch_size: only the default configuration is timed there) and a run of this one on the same device land in one file.  Every
configuration is run once untimed first (engines are built per batch shape) and then timed end to end, files written included."""
import argparse
import inspect
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("EDTR_BENCH_TREE", ROOT))            # EDTR_BENCH_TREE: another checkout of the package to time

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (h, w) of the source files: landscape, portrait, square, small, large.  --scale -1 brings every longer side to 512
SHAPES = ((480, 640), (600, 400), (512, 512), (300, 500), (768, 1024), (333, 500), (640, 480), (200, 200))


def write_folder(folder: str, n: int):
    from PIL import Image
    rng = np.random.default_rng(2024)
    for k in range(n):
        h, w = SHAPES[k % len(SHAPES)]
        base = rng.integers(0, 256, size=(h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        Image.fromarray(np.ascontiguousarray(np.kron(base, np.ones((16, 16, 1), dtype=np.uint8))[:h, :w])).save(os.path.join(folder, f"im{k:03d}.png"))


def build(model: str, dev):
    from edtr_amd import synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    if model == "tiny":
        cfg = synth.tiny_config()
        cldm = build_synthetic_cldm(cfg, dev, torch.float16)
        cldm.clip.set_embedding(synth.synth_input("demo:c_txt", (1, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(dev))
        kw, scale = dict(img_size=128, multiple=64), 0.25                # the tiny model's 128-pixel slots: quarter-size images
    else:
        cldm = build_synthetic_cldm(synth.sd21_config(), dev, torch.bfloat16, precision="fast")
        cldm.clip.set_embedding(synth.synth_normal("inv:c_txt", (1, 77, 1024)).to(dev))
        kw, scale = dict(img_size=512, multiple=64), -1.0
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(dev)
    return cldm, diffusion, SpacedSampler(diffusion.betas), kw, scale


def boundary(dev, batched: bool):
    """launches and milliseconds of resize + ingest + emit for eight 512-slot images, per image and (where it exists) per batch"""
    from edtr_amd import imageio, ops
    rng = np.random.default_rng(7)
    raws = [torch.from_numpy(rng.integers(0, 256, size=SHAPES[k] + (3,), dtype=np.uint8)).to(dev) for k in range(8)]
    outs = [imageio.demo_size(r.shape[1], r.shape[0]) for r in raws]
    count = [0]
    real = ops.launch

    def counting(rec):
        count[0] += 1
        real(rec)

    def per_image():
        batch, sizes = None, None
        for r, (ow, oh) in zip(raws, outs):
            batch, sizes = imageio.ingest([imageio.resize_u8(r, ow, oh)], min_size=512, multiple=64)
            imageio.emit(batch, sizes)

    def per_batch():
        batch, sizes = imageio.ingest_resized(raws, outs, min_size=512, multiple=64)
        imageio.emit_packed(batch, sizes)

    found = {}
    for name, fn in (("per_image", per_image),) + ((("per_batch", per_batch),) if batched else ()):
        ops.launch = counting
        try:
            count[0] = 0
            fn()
            launches = count[0]
        finally:
            ops.launch = real
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        found[name] = {"launches": launches, "ms": round((time.perf_counter() - t0) / 20 * 1e3, 4), "images": 8,
                       "what": "resize + ingest + emit on device-resident bytes, host time of issue included"}
    return found


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--label", required=True, help="key of this run in the JSON, e.g. 'parent' or 'this'")
    ap.add_argument("--models", default="tiny,sd21")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore_files_timing.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_restore_files.py needs a GPU")
    from edtr_amd import restore
    dev = torch.device("cuda")
    batched = "batch_size" in inspect.signature(restore.restore_files).parameters
    configs = [(1, 0), (1, 8), (8, 0), (8, 8)] if batched else [(1, 0)]
    run = {"device": torch.cuda.get_device_name(0), "images": args.images, "source_shapes_hw": [list(s) for s in SHAPES],
           "batched_restore_files": batched, "boundary_8_images": boundary(dev, batched), "models": {}}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        write_folder(src, args.images)
        paths = restore.list_images(src)
        for model in args.models.split(","):
            cldm, diffusion, sampler, kw, scale = build(model, dev)
            rows = []
            for bs, workers in configs:
                extra = dict(batch_size=bs, workers=workers) if batched else {}
                secs = []
                for rep in range(2):                                    # the first pass builds the engines of every batch shape
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    written = restore.restore_files(cldm, diffusion, sampler, paths, os.path.join(tmp, f"out_{model}_{bs}_{workers}"),
                                                    scale=scale, seed=1, **extra, **kw)
                    torch.cuda.synchronize()
                    secs.append(time.perf_counter() - t0)
                assert len(written) == len(paths)
                rows.append({"batch_size": bs, "workers": workers, "files_per_s": round(len(paths) / secs[1], 3),
                             "seconds": round(secs[1], 4), "first_pass_seconds": round(secs[0], 4)})
                print(f"[{args.label}] {model} batch_size={bs} workers={workers}: {rows[-1]['files_per_s']} files/s", flush=True)
            run["models"][model] = rows
            del cldm
            torch.cuda.empty_cache()
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged[args.label] = run
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
    print(json.dumps({"label": args.label, "out": args.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
