"""Image files in, restored image files out: the file loop of demo.py:76-90,163-165 around `evalutil.restore_dataset`.  Pillow decodes
and encodes on the host and does nothing else; the resize to `imageio.demo_size`, the /255, the padding, the crop and save_image's
quantisation are launches of edtr_amd.imageio on the uploaded bytes.

    python -m edtr_amd.restore --input DIR --output DIR --config YAML-or-"tiny" [--seed N] [--scale S] [--batch-size N] [--workers N]
                               [--pre-res-tiled] [--vae-encoder-tiled] [--vae-decoder-tiled] [--cldm-tiled] [--*-tile-size N] [--*-tile-stride N]

``--batch-size N`` restores images of one padded extent N at a time (`imageio.plan_buckets`; the whole batch crosses the 8-bit boundary in
three launches and one copy to the host), ``--workers N`` decodes and encodes in N threads while the GPU works.  With ``--seed`` and
EDTR_AMD_BATCH_INVARIANT=1 the files written are the same bytes whatever the two say.

The four ``--*-tiled`` switches and their sizes are demo.py's (:183-192, same spellings, units and defaults): they become one
`evalutil.TilingOptions` that every image of the folder is restored with; a stage too small for its tile runs untiled.

``--config tiny`` builds the synthetic tiny model of edtr_amd.synth (no checkpoints: a way to see the tool run); a YAML file in the
reference's layout (configs/det/demo.yaml) is instantiated through edtr_amd.shim and loaded with the strict loaders of INTEGRATION.md §1
from ``--sd-weight`` and ``--edtr-weight``.  Everything runs in this process."""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import List, Optional, Sequence

EXTENSIONS = ("png", "jpg", "jpeg", "JPG", "JPEG")          # demo.py:57


def _pillow():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("edtr_amd.restore needs Pillow to decode and encode image files (`import PIL` failed); "
                           "evalutil.restore_dataset takes already decoded uint8 (h, w, 3) arrays without it") from e
    return Image


def list_images(folder: str) -> List[str]:
    """The image files of ``folder`` as demo.py:57-58 lists them."""
    from glob import glob
    return sorted(sum([glob(os.path.join(folder, f"*.{e}")) for e in EXTENSIONS], []))


MAX_WORKERS = 16            # decode / encode threads at the most, whatever is asked for (never sized by the machine's CPU count)
_BATCHED_KEYWORDS = ("img_size", "multiple", "used_timesteps", "start_timestep", "colour_fix", "tiling")


def _out_name(out_dir: str, path: str) -> str:
    return os.path.join(out_dir, os.path.splitext(os.path.basename(path))[0] + ".png")


def _restore_files_batched(cldm, diffusion, sampler, paths, out_dir, swinir, scale, seed, batch_size, workers, img_size=512,
                           multiple=64, used_timesteps=(50, 100, 150, 200), start_timestep=200, colour_fix=True, tiling=None) -> List[str]:
    """`restore_files` for batch_size > 1 or workers > 0: the shard's files are grouped by the padded extent of their resized size and
    every chunk runs `imageio.ingest_resized` -> `evalutil.restore_batch` -> `imageio.emit_packed` -> one copy into a pinned buffer.
    All GPU work is issued from the calling thread; with ``workers`` the next chunk is decoded and the previous one encoded by a thread
    pool meanwhile.  A worker's exception is raised here."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from concurrent.futures import ThreadPoolExecutor
    from . import evalutil, imageio
    from .parallel import shard_slice
    from .rng import NoiseSource, shard_bucket_ids
    Image = _pillow()
    dev = next(cldm.unet.parameters()).device
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    sl = shard_slice(rank, world, len(paths))
    mine = paths[sl]
    os.makedirs(out_dir, exist_ok=True)
    names = [_out_name(out_dir, p) for p in mine]

    def header(path):                           # (w, h) from the file's header: the plan needs every size before anything is decoded
        with Image.open(path) as im:
            return im.size

    def decode(path, size):
        with Image.open(path) as im:
            raw = np.array(im.convert("RGB"), dtype=np.uint8)
        if (raw.shape[1], raw.shape[0]) != tuple(size):
            raise ValueError(f"{path} decodes to {raw.shape[1]} x {raw.shape[0]}, its header says {size[0]} x {size[1]}")
        return raw

    def encode(view, name):
        Image.fromarray(view).save(name)        # (uint8 [h, w, 3]: Pillow infers RGB)

    pool = ThreadPoolExecutor(max_workers=min(int(workers), MAX_WORKERS)) if workers > 0 else None

    class _Done:                                # what `submit` returns without a pool: the work already ran on the calling thread
        def __init__(self, value):
            self.value = value

        def result(self):
            return self.value

    def submit(fn, *args):
        return pool.submit(fn, *args) if pool is not None else _Done(fn(*args))

    try:
        in_sizes = [f.result() for f in [submit(header, p) for p in mine]]
        out_sizes = [imageio.demo_size(w, h, scale) for w, h in in_sizes]
        plan = imageio.plan_buckets([(oh, ow) for ow, oh in out_sizes], batch_size, min_size=img_size, multiple=multiple)
        ids = shard_bucket_ids(len(paths), rank, world, plan) if seed is not None else None
        encodes = []

        def finish(done):                       # a chunk whose copy to the host was queued: wait for it, hand its images to the encoders
            event, host, views, idx = done
            event.synchronize()
            flat = host.numpy()
            for k, (o, h, w) in zip(idx, views):
                encodes.append(submit(encode, flat[o:o + h * w * 3].reshape(h, w, 3), names[k]))

        decodes = [submit(decode, mine[k], in_sizes[k]) for k in plan[0][1]] if plan else []
        pending = None
        for c, (_, idx) in enumerate(plan):
            raws = [f.result() for f in decodes]
            decodes = [submit(decode, mine[k], in_sizes[k]) for k in plan[c + 1][1]] if c + 1 < len(plan) else []
            if pending is not None:             # (before this chunk's launches, so that its encoding runs beside them)
                finish(pending)
            pre, sizes = imageio.ingest_resized(raws, [out_sizes[k] for k in idx], min_size=img_size, multiple=multiple, device=dev)
            source = NoiseSource(seed, ids[c]) if seed is not None else None
            res = evalutil.restore_batch(cldm, diffusion, sampler, pre, source, used_timesteps, start_timestep, colour_fix, swinir, tiling)
            packed, views = imageio.emit_packed(res.float().contiguous(), sizes)
            host = torch.empty((packed.numel(),), dtype=torch.uint8, pin_memory=True)
            host.copy_(packed, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            base = packed.data_ptr()
            pending = (event, host, [(v.data_ptr() - base, v.shape[0], v.shape[1]) for v in views], idx)
        if pending is not None:
            finish(pending)
        for f in encodes:
            f.result()
    finally:
        if pool is not None:
            pool.shutdown(wait=True, cancel_futures=True)
    return names


def restore_files(cldm, diffusion, sampler, paths: Sequence[str], out_dir: str, swinir=None, scale: float = -1.0,
                  seed: Optional[int] = None, batch_size: int = 1, workers: int = 0, **kwargs) -> List[str]:
    """Decode every file of ``paths`` (Pillow, RGB), upload its bytes, resize them on the device to `imageio.demo_size(w, h, scale)`
    (Image.BICUBIC's bits), run `evalutil.restore_dataset(..., pad_mode="demo", return_uint8=True)` (``kwargs`` are its keywords)
    and write this rank's restored images to ``out_dir`` as <stem>.png.  Returns the written paths, in the order of ``paths``.
    ``batch_size`` > 1: images whose resized size pads to the same extent are restored together, ``batch_size`` at a time (the flow of
    `restore_dataset(pad_mode="bucket")`; ``kwargs`` may then be img_size, multiple, used_timesteps, start_timestep, colour_fix, tiling);
    ``workers`` > 0: that many threads (16 at the most) decode and encode while the calling thread drives the GPU.  Only a run with
    ``seed`` (and, for equal bits, EDTR_AMD_BATCH_INVARIANT=1) writes the same files whatever ``batch_size`` is."""
    if int(batch_size) <= 0 or int(workers) < 0:
        raise ValueError(f"batch_size must be positive and workers non-negative, got {batch_size} and {workers}")
    if int(batch_size) > 1 or int(workers) > 0:
        if kwargs.get("pad_mode", "bucket") not in ("demo", "bucket"):
            raise TypeError("restore_files in batches is the demo flow: pad_mode must be 'demo' or 'bucket'")
        extra = sorted(set(kwargs) - set(_BATCHED_KEYWORDS) - {"pad_mode"})
        if extra:
            raise TypeError(f"restore_files in batches takes {', '.join(_BATCHED_KEYWORDS)}; got {', '.join(extra)}")
        kw = {k: v for k, v in kwargs.items() if k != "pad_mode"}
        return _restore_files_batched(cldm, diffusion, sampler, list(paths), out_dir, swinir, scale, seed, int(batch_size), int(workers), **kw)
    import numpy as np
    import torch
    import torch.distributed as dist
    from . import evalutil, imageio
    from .parallel import shard_slice
    Image = _pillow()
    if "return_uint8" in kwargs or "gts" in kwargs:
        raise TypeError("restore_files decides return_uint8 itself and takes no ground truth")
    kwargs.setdefault("pad_mode", "demo")
    dev = next(cldm.unet.parameters()).device
    paths = list(paths)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    sl = shard_slice(rank, world, len(paths))
    images = [None] * len(paths)                 # other ranks' files are not decoded: restore_dataset reads its own shard only
    for k in range(sl.start, sl.stop):
        with Image.open(paths[k]) as im:
            raw = torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)).to(dev)
        out_w, out_h = imageio.demo_size(raw.shape[1], raw.shape[0], scale)
        images[k] = imageio.resize_u8(raw, out_w, out_h)
    outs, _ = evalutil.restore_dataset(cldm, diffusion, sampler, images, swinir=swinir, seed=seed, return_uint8=True, **kwargs)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for path, out in zip(paths[sl], outs):
        name = os.path.join(out_dir, os.path.splitext(os.path.basename(path))[0] + ".png")
        Image.fromarray(out.cpu().numpy()).save(name)               # (uint8 [h, w, 3]: Pillow infers RGB)
        written.append(name)
    return written


def _build_tiny(device):
    import torch
    from . import synth
    from .diffusion import Diffusion
    from .sampler import SpacedSampler
    from .testing import build_synthetic_cldm
    cfg = synth.tiny_config()
    cldm = build_synthetic_cldm(cfg, device, torch.float16)
    cldm.clip.set_embedding(synth.synth_input("demo:c_txt", (1, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(device))
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(device)
    return cldm, None, diffusion, SpacedSampler(diffusion.betas), dict(img_size=128)


def _build_from_yaml(path: str, sd_weight: str, edtr_weight: str, device):
    import torch
    import yaml
    from . import shim
    from .sampler import SpacedSampler
    if not sd_weight or not edtr_weight:
        raise SystemExit("a YAML --config needs --sd-weight and --edtr-weight")
    with open(path) as fh:
        cfg = yaml.safe_load(fh)
    shim.install(overlay=False)
    swinir = shim.instantiate_from_config(cfg["model"]["swinir"])
    cldm = shim.instantiate_from_config(cfg["model"]["cldm"])
    diffusion = shim.instantiate_from_config(cfg["model"]["diffusion"])
    cldm.load_pretrained_sd(torch.load(sd_weight, map_location="cpu")["state_dict"])
    weights = torch.load(edtr_weight, map_location="cpu")
    swinir.load_state_dict(weights["swinir"], strict=True)
    cldm.load_controlnet_from_ckpt(weights["cldm"])
    cldm.vae.decoder.load_state_dict(weights["decoder"])
    ts, n = cfg["test"]["start_timestep"], cfg["test"]["num_timesteps"]
    used = [math.floor(ts / n * i) for i in range(1, n + 1)]            # demo.py:64
    return (cldm.eval().to(device), swinir.eval().to(device), diffusion.to(device), SpacedSampler(diffusion.betas),
            dict(used_timesteps=used, start_timestep=ts))


def tiling_from_args(args):
    """The `evalutil.TilingOptions` of the parsed ``--*-tiled`` flags; None when no switch is on (the untiled flow)."""
    from .evalutil import TilingOptions
    opt = TilingOptions(pre_res=args.pre_res_tiled, pre_res_size=args.pre_res_tile_size, pre_res_stride=args.pre_res_tile_stride,
                        vae_encoder=args.vae_encoder_tiled, vae_encoder_size=args.vae_encoder_tile_size,
                        vae_decoder=args.vae_decoder_tiled, vae_decoder_size=args.vae_decoder_tile_size,
                        cldm=args.cldm_tiled, cldm_size=args.cldm_tile_size, cldm_stride=args.cldm_tile_stride)
    return opt if (opt.pre_res or opt.vae_encoder or opt.vae_decoder or opt.cldm) else None


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m edtr_amd.restore", description="Restore every image of a folder on the GPU.")
    ap.add_argument("--input", required=True, help="folder of png / jpg / jpeg files")
    ap.add_argument("--output", required=True, help="folder the restored <stem>.png files are written to")
    ap.add_argument("--config", required=True, help='a YAML file in the layout of configs/det/demo.yaml, or "tiny" (synthetic tiny model)')
    ap.add_argument("--seed", type=int, default=None, help="seeded per-image noise (edtr_amd.rng); default: torch's generator")
    ap.add_argument("--scale", type=float, default=-1.0, help="resize factor; -1 (default) brings the longer side to 512")
    ap.add_argument("--batch-size", type=int, default=1, help="restore images of one padded extent this many at a time (default 1)")
    ap.add_argument("--workers", type=int, default=0, help="threads that decode and encode beside the GPU work (default 0, at most 16)")
    ap.add_argument("--sd-weight", default=None, help="Stable Diffusion 2.1 checkpoint (YAML configs)")
    ap.add_argument("--edtr-weight", default=None, help="EDTR checkpoint with swinir / cldm / decoder entries (YAML configs)")
    # the tiling switches of demo.py:183-192
    ap.add_argument("--pre-res-tiled", action="store_true", help="SwinIR per sliding window")
    ap.add_argument("--pre-res-tile-size", type=int, default=512)
    ap.add_argument("--pre-res-tile-stride", type=int, default=256)
    ap.add_argument("--vae-encoder-tiled", action="store_true")
    ap.add_argument("--vae-encoder-tile-size", type=int, default=256)
    ap.add_argument("--vae-decoder-tiled", action="store_true")
    ap.add_argument("--vae-decoder-tile-size", type=int, default=256)
    ap.add_argument("--cldm-tiled", action="store_true", help="latent-tiled denoiser")
    ap.add_argument("--cldm-tile-size", type=int, default=512, help="image pixels (the sampler gets it // 8)")
    ap.add_argument("--cldm-tile-stride", type=int, default=256)
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("edtr_amd.restore needs a GPU: the restoration path has no CPU fallback")
    device = torch.device("cuda")
    paths = list_images(args.input)
    if not paths:
        raise SystemExit(f"no image files in {args.input}")
    build = _build_tiny(device) if args.config == "tiny" else _build_from_yaml(args.config, args.sd_weight, args.edtr_weight, device)
    cldm, swinir, diffusion, sampler, kw = build
    tiling = tiling_from_args(args)
    if tiling is not None:
        kw = dict(kw, tiling=tiling)
    written = restore_files(cldm, diffusion, sampler, paths, args.output, swinir=swinir, scale=args.scale, seed=args.seed,
                            batch_size=args.batch_size, workers=args.workers, **kw)
    for name in written:
        print(name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
