"""Image files in, restored image files out: the file loop of demo.py:76-90,163-165 around `evalutil.restore_dataset`.  Pillow decodes
and encodes on the host and does nothing else; the resize to `imageio.demo_size`, the /255, the padding, the crop and save_image's
quantisation are launches of edtr_amd.imageio on the uploaded bytes.

    python -m edtr_amd.restore --input DIR --output DIR --config YAML-or-"tiny" [--seed N] [--scale S]

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


def restore_files(cldm, diffusion, sampler, paths: Sequence[str], out_dir: str, swinir=None, scale: float = -1.0,
                  seed: Optional[int] = None, **kwargs) -> List[str]:
    """Decode every file of ``paths`` (Pillow, RGB), upload its bytes, resize them on the device to `imageio.demo_size(w, h, scale)`
    (Image.BICUBIC's bits), run `evalutil.restore_dataset(..., pad_mode="demo", return_uint8=True)` (``kwargs`` are its keywords)
    and write this rank's restored images to ``out_dir`` as <stem>.png.  Returns the written paths."""
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m edtr_amd.restore", description="Restore every image of a folder on the GPU.")
    ap.add_argument("--input", required=True, help="folder of png / jpg / jpeg files")
    ap.add_argument("--output", required=True, help="folder the restored <stem>.png files are written to")
    ap.add_argument("--config", required=True, help='a YAML file in the layout of configs/det/demo.yaml, or "tiny" (synthetic tiny model)')
    ap.add_argument("--seed", type=int, default=None, help="seeded per-image noise (edtr_amd.rng); default: torch's generator")
    ap.add_argument("--scale", type=float, default=-1.0, help="resize factor; -1 (default) brings the longer side to 512")
    ap.add_argument("--sd-weight", default=None, help="Stable Diffusion 2.1 checkpoint (YAML configs)")
    ap.add_argument("--edtr-weight", default=None, help="EDTR checkpoint with swinir / cldm / decoder entries (YAML configs)")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("edtr_amd.restore needs a GPU: the restoration path has no CPU fallback")
    device = torch.device("cuda")
    paths = list_images(args.input)
    if not paths:
        raise SystemExit(f"no image files in {args.input}")
    build = _build_tiny(device) if args.config == "tiny" else _build_from_yaml(args.config, args.sd_weight, args.edtr_weight, device)
    cldm, swinir, diffusion, sampler, kw = build
    written = restore_files(cldm, diffusion, sampler, paths, args.output, swinir=swinir, scale=args.scale, seed=args.seed, **kw)
    for name in written:
        print(name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
