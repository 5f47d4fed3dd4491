"""Evaluation-harness helpers around the restoration path: host-side mirrors of the reference's
batch padding (`utils/detection.py:141-165`) and PSNR metric (`utils/common.py:194-247`), plus an accelerate-free
data-parallel driver that shards a list of pre-restored images over the ranks of `torch.distributed`, runs the
edtr_amd path on each shard and reports PSNR.  The helpers up to `calculate_psnr_pt` are plain tensor bookkeeping on float tensors
(today's path of `restore_dataset`, kept bit for bit); 8-bit images and the "seg" padding go through the launches of edtr_amd.imageio."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from .parallel import shard_slice
from .rng import NoiseSource, shard_bucket_ids, shard_chunk_ids


def list_to_batch(img_list: Sequence[torch.Tensor], img_size: int, device) -> torch.Tensor:
    """Zero-pad every (C, H, W) image at the bottom / right to (C, img_size, img_size) and stack (detection.py:141-157)."""
    out = []
    for img in img_list:
        ph, pw = img_size - img.size(1), img_size - img.size(2)
        out.append(torch.nn.functional.pad(img.unsqueeze(0).to(device), pad=(0, pw, 0, ph), mode="constant"))
    return torch.cat(out, dim=0) if out else torch.Tensor().to(device)


def batch_to_list(img_batch: torch.Tensor, img_list: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """Crop every batch entry back to the size of the matching list entry (detection.py:160-165)."""
    return [img_batch[i][:, :img.size(1), :img.size(2)] for i, img in enumerate(img_list)]


def pad_if_smaller(imgs: torch.Tensor, size: int) -> torch.Tensor:
    """Zero-pad (n, c, h, w) at the bottom / right up to ``size`` in each dimension that is smaller (utils/common.py:337-340)."""
    _, _, h, w = imgs.size()
    return torch.nn.functional.pad(imgs, pad=(0, max(size - w, 0), 0, max(size - h, 0)), mode="constant", value=0)


def pad_to_multiples_of(imgs: torch.Tensor, multiple: int) -> torch.Tensor:
    """Zero-pad (n, c, h, w) at the bottom / right to the next multiples of ``multiple`` (utils/common.py:343-348)."""
    _, _, h, w = imgs.size()
    if h % multiple == 0 and w % multiple == 0:
        return imgs.clone()
    ph, pw = ((x + multiple - 1) // multiple * multiple - x for x in (h, w))
    return torch.nn.functional.pad(imgs, pad=(0, pw, 0, ph), mode="constant", value=0)


def rgb2ycbcr_pt(img: torch.Tensor, y_only: bool = False) -> torch.Tensor:
    """ITU-R BT.601 RGB -> YCbCr on (n, 3, h, w) in [0, 1] (common.py:194-216)."""
    if y_only:
        weight = torch.tensor([[65.481], [128.553], [24.966]]).to(img)
        out = torch.matmul(img.permute(0, 2, 3, 1), weight).permute(0, 3, 1, 2) + 16.0
    else:
        weight = torch.tensor([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]]).to(img)
        bias = torch.tensor([16, 128, 128]).view(1, 3, 1, 1).to(img)
        out = torch.matmul(img.permute(0, 2, 3, 1), weight).permute(0, 3, 1, 2) + bias
    return out / 255.0


def calculate_psnr_pt(img: torch.Tensor, img2: torch.Tensor, crop_border: int, test_y_channel: bool = False) -> torch.Tensor:
    """Per-image PSNR in dB of (n, 3/1, h, w) tensors in [0, 1] (common.py:219-247)."""
    assert img.shape == img2.shape, f"Image shapes are different: {img.shape}, {img2.shape}."
    if crop_border != 0:
        img = img[:, :, crop_border:-crop_border, crop_border:-crop_border]
        img2 = img2[:, :, crop_border:-crop_border, crop_border:-crop_border]
    if test_y_channel:
        img, img2 = rgb2ycbcr_pt(img, y_only=True), rgb2ycbcr_pt(img2, y_only=True)
    img, img2 = img.to(torch.float64), img2.to(torch.float64)
    mse = torch.mean((img - img2) ** 2, dim=[1, 2, 3])
    return 10.0 * torch.log10(1.0 / (mse + 1e-8))


def _as_hwc(img):
    """A uint8 (h, w, 3) image as it is; a float (C, h, w) tensor as its (h, w, C) view (imageio.ingest copies it as fp32)."""
    from . import imageio
    return img if imageio.is_u8_image(img) else img.permute(1, 2, 0)


def _image_hw(img) -> Tuple[int, int]:
    """(h, w) of a uint8 (h, w, 3) image or of a float (C, h, w) tensor"""
    from . import imageio
    return (int(img.shape[0]), int(img.shape[1])) if imageio.is_u8_image(img) else (int(img.shape[1]), int(img.shape[2]))


@dataclass(frozen=True)
class TilingOptions:
    """The four tiling switches of demo.py:183-192 and their six sizes, in the demo's units and with its defaults: ``pre_res_*`` and
    ``vae_encoder_size`` in image pixels, ``cldm_*`` in image pixels (the sampler gets them // 8, demo.py:114,120), ``vae_decoder_size``
    handed to `vae_decode` as it is (demo.py:123: latent pixels).  A stage whose switch is off runs untiled whatever its sizes say."""
    pre_res: bool = False
    pre_res_size: int = 512
    pre_res_stride: int = 256
    vae_encoder: bool = False
    vae_encoder_size: int = 256
    vae_decoder: bool = False
    vae_decoder_size: int = 256
    cldm: bool = False
    cldm_size: int = 512
    cldm_stride: int = 256

    def pre_res_tiled(self, H: int, W: int) -> bool:
        """SwinIR runs per window when the switch is on and a window fits on both axes (the demo's "tiny and unnecessary to tile")."""
        return bool(self.pre_res) and min(H, W) >= self.pre_res_size

    def cldm_tiled(self, h: int, w: int) -> bool:
        """demo.py:113-116 on the latent's (h, w): untiled unless the latent is larger than the tile on both axes."""
        return bool(self.cldm) and not (h <= self.cldm_size // 8 or w <= self.cldm_size // 8)

    def sampler_kwargs(self, h: int, w: int) -> dict:
        """What `SpacedSampler.manual_sample_with_timesteps` gets for a latent of (h, w) (demo.py:120)."""
        return dict(tiled=self.cldm_tiled(h, w), tile_size=self.cldm_size // 8, tile_stride=self.cldm_stride // 8)

    def encoder_kwargs(self) -> dict:
        return dict(tiled=bool(self.vae_encoder), tile_size=self.vae_encoder_size)

    def decoder_kwargs(self) -> dict:
        return dict(tiled=bool(self.vae_decoder), tile_size=self.vae_decoder_size)


def _tiled_swinir(swinir, tiling: TilingOptions):
    """SwinIR per sliding window with the windows stacked on the batch axis (demo.py:98 with the options' sizes)."""
    from .tiling import make_tiled_fn
    return make_tiled_fn(swinir, tiling.pre_res_size, tiling.pre_res_stride, batched_fn=lambda tiles, windows: swinir(tiles))


@torch.no_grad()
def restore_batch(cldm, diffusion, sampler, pre: torch.Tensor, source: Optional[NoiseSource] = None,
                  used_timesteps=(50, 100, 150, 200), start_timestep: int = 200, colour_fix: bool = True, swinir=None,
                  tiling: Optional[TilingOptions] = None) -> torch.Tensor:
    """One padded fp32 (B, 3, H, W) batch through (SwinIR ->) prepare_condition -> q_sample(start_timestep) -> spaced sampler ->
    vae_decode (-> wavelet colour fix): what `restore_dataset` runs on every chunk, whatever built the batch.  ``source``: the seeded
    noise of the batch's images, or None for torch's generator.  ``tiling`` (a `TilingOptions`): the stages whose switch is on run
    tiled as in demo.py:94-123 — SwinIR per window, `vae_encode(tiled=)`, the latent-tiled sampler, `vae_decode(tiled=)`; a stage too
    small for its tile runs untiled.  The sampler's patch of ``cldm.forward`` is taken back before this returns."""
    from .wavelet import wavelet_reconstruction
    dev = pre.device
    if swinir is not None:
        pre = (_tiled_swinir(swinir, tiling) if tiling is not None and tiling.pre_res_tiled(pre.size(2), pre.size(3)) else swinir)(pre)
    if tiling is not None and tiling.vae_encoder:   # prepare_condition does not expose the encoder's tiling: its two calls, as demo.py:102-104
        cldm.clip.compute_dtype = cldm.compute_dtype
        cond = dict(c_txt=cldm.clip.encode([""] * pre.size(0)), c_img=cldm.vae_encode(pre * 2 - 1, sample=False, **tiling.encoder_kwargs()))
    else:
        cond = cldm.prepare_condition(pre, [""] * pre.size(0))
    t = torch.full((pre.size(0),), start_timestep, dtype=torch.int64)
    x_T = diffusion.q_sample(cond["c_img"], t, torch.randn_like(cond["c_img"]) if source is None else source)
    tiled = {} if tiling is None else tiling.sampler_kwargs(x_T.size(2), x_T.size(3))
    had, saved = "forward" in vars(cldm), vars(cldm).get("forward")
    try:
        z = sampler.manual_sample_with_timesteps(model=cldm, device=dev, x_T=x_T, steps=len(used_timesteps),
                                                 used_timesteps=list(used_timesteps), batch_size=pre.size(0), cond=cond,
                                                 uncond=None, cfg_scale=1.0, progress=False, **tiled,
                                                 **({} if source is None else {"noise_source": source}))
    finally:                                # the sampler never restores the forward it patches (reference utils/sampler.py:288-303)
        if had:
            cldm.forward = saved
        elif "forward" in vars(cldm):
            del cldm.forward
    res = (cldm.vae_decode(z, **({} if tiling is None else tiling.decoder_kwargs())) + 1) / 2
    if colour_fix:
        res = wavelet_reconstruction(res, pre)
    return res


@torch.no_grad()
def restore_dataset(cldm, diffusion, sampler, pre_restored: Sequence[torch.Tensor], gts: Optional[Sequence[torch.Tensor]] = None,
                    img_size: int = 512, batch_size: int = 8, used_timesteps=(50, 100, 150, 200), start_timestep: int = 200,
                    colour_fix: bool = True, swinir=None, pad_mode: str = "batch", multiple: int = 64,
                    clamp: bool = True, *, return_uint8: bool = False, tiling: Optional[TilingOptions] = None,
                    seed: Optional[int] = None) -> Tuple[List[torch.Tensor], Optional[torch.Tensor]]:
    """The restoration loop of main/det/test_edtr.py:121-135 without accelerate: this rank's shard of the
    (C, h, w <= img_size) pre-restored images is padded, pushed through vae_encode -> q_sample(t) -> spaced sampler ->
    vae_decode (-> wavelet colour fix), cropped back, and — when ground truth is given — scored with PSNR; the scalar
    PSNR sums are all-reduced, nothing else crosses ranks.  With ``swinir`` (an edtr_amd.model.SwinIR) the inputs are the
    low-quality images themselves and the pre-restoration runs on the padded batch first (`cfg.model.pre_restoration`,
    main/det/test_edtr.py:118).  ``pad_mode="demo"`` is the single-image flow of demo.py:84-131,165 instead: every image on its own,
    `pad_if_smaller(img_size)` -> `pad_to_multiples_of(multiple)` -> (SwinIR) -> the same path -> crop back to the input's size
    (``clamp=False`` keeps the values the reference hands to `save_image`).  ``seed``: None = the noise comes from torch's generator
    as in the reference; an int = every image gets the seeded stream of its index in the GLOBAL ``pre_restored`` list
    (edtr_amd.rng), so its noise — and, with EDTR_AMD_BATCH_INVARIANT=1, its restoration bit for bit — does not depend on
    ``batch_size``, ``pad_mode`` or the number of ranks.  ``pad_mode="seg"`` is the loop of main/seg/test_edtr.py:113-136: every image on
    its own, replicate-padded at the bottom / right to multiples of ``multiple`` -> (SwinIR) -> the same path -> crop back; its chunking and
    seeded ids are those of "demo".  Entries of ``pre_restored`` / ``gts`` may also be uint8 (h, w, 3) tensors or arrays — what an image
    decoder returns: they are turned into v / 255 and padded on the device by `imageio.ingest` (the same bits as the float (C, h, w) form of
    the same image), and PSNR against uint8 ground truth is `imageio.psnr`.  ``pad_mode="bucket"`` is "demo"'s padding and crop for every
    image, run in batches: this rank's shard is grouped by padded extent (`imageio.plan_buckets`, chunks of at most ``batch_size``), the
    outputs come back in data-set order, ``return_uint8`` goes through `imageio.emit_packed`.  Its noise without ``seed`` is one
    `torch.randn_like` per chunk, as in "batch": only a SEEDED run is independent of ``batch_size`` (image k carries id k), and only with
    EDTR_AMD_BATCH_INVARIANT=1 is it "demo" bit for bit.  ``return_uint8=True`` (keyword only, so that ``seed``
    stays the last parameter) returns `imageio.emit`'s uint8 (h, w, 3) bytes — what `save_image` would write — instead of float tensors.
    ``tiling`` (keyword only, a `TilingOptions`): handed to `restore_batch` for every chunk in all four pad modes; the noise is drawn on
    the whole latent, so a seeded tiled run keeps the guarantee above (EDTR_AMD_BATCH_INVARIANT=1: equal bits whatever ``batch_size``).  Returns (restored images of this shard, mean PSNR or None)."""
    import torch.distributed as dist
    from . import imageio
    dev = next(cldm.unet.parameters()).device
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    sl = shard_slice(rank, world, len(pre_restored))
    mine = list(pre_restored[sl])
    if pad_mode not in ("batch", "demo", "seg", "bucket"):
        raise ValueError(f"pad_mode must be 'batch', 'demo', 'seg' or 'bucket', got {pad_mode!r}")
    if pad_mode == "bucket":
        # chunks of equal padded extent; `where` = the chunk's positions in this shard, the outputs go back to those positions
        plan = imageio.plan_buckets([_image_hw(img) for img in mine], batch_size, min_size=img_size, multiple=multiple)
        where = [idx for _, idx in plan]
        chunk_ids = shard_bucket_ids(len(pre_restored), rank, world, plan) if seed is not None else None
    else:
        step = 1 if pad_mode in ("demo", "seg") else batch_size
        where = [list(range(i, min(i + step, len(mine)))) for i in range(0, len(mine), step)]
        chunk_ids = shard_chunk_ids(len(pre_restored), rank, world, batch_size, pad_mode) if seed is not None else None
    outs: List[Optional[torch.Tensor]] = [None] * len(mine)
    for c, idx in enumerate(where):
        chunk = [mine[k] for k in idx]
        source = NoiseSource(seed, chunk_ids[c]) if seed is not None else None
        sizes = None                   # (h, w) per image where imageio.ingest built the batch; None = today's float path
        if pad_mode == "seg":
            pre, sizes = imageio.ingest([_as_hwc(chunk[0])], pad="replicate", multiple=multiple, device=dev)
        elif imageio.is_u8_image(chunk[0]):
            if pad_mode in ("demo", "bucket"):
                pre, sizes = imageio.ingest(chunk, min_size=img_size, multiple=multiple, device=dev)
            else:
                pre, sizes = imageio.ingest(chunk, size=(img_size, img_size), device=dev)
        elif pad_mode == "demo":
            pre = pad_to_multiples_of(pad_if_smaller(chunk[0][None].to(dev).float(), img_size), multiple)
        elif pad_mode == "bucket":
            pre = torch.cat([pad_to_multiples_of(pad_if_smaller(img[None].to(dev).float(), img_size), multiple) for img in chunk], dim=0)
        else:
            pre = list_to_batch(chunk, img_size, dev).float()
        res = restore_batch(cldm, diffusion, sampler, pre, source, used_timesteps, start_timestep, colour_fix, swinir, tiling)
        if return_uint8:           # (emit clamps: `clamp` has nothing left to decide)
            hw = sizes or [(img.size(1), img.size(2)) for img in chunk]
            got = imageio.emit_packed(res.float().contiguous(), hw)[1] if pad_mode == "bucket" else imageio.emit(res.float().contiguous(), hw)
        elif sizes is None:
            got = batch_to_list(res.clamp(0, 1) if clamp else res, chunk)
        else:
            res = res.clamp(0, 1) if clamp else res
            got = [res[k][:, :h, :w] for k, (h, w) in enumerate(sizes)]
        for k, o in zip(idx, got):
            outs[k] = o
    psnr = None
    if gts is not None:
        mine_gt = list(gts[sl])
        acc = torch.zeros(2, dtype=torch.float64, device=dev)
        for o, g in zip(outs, mine_gt):
            if imageio.is_u8_image(g) or return_uint8:
                a, _ = imageio.ingest([o if return_uint8 else o.permute(1, 2, 0)], device=dev)
                acc[0] += imageio.psnr(a, imageio.ingest([_as_hwc(g)], device=dev)[0], crop_border=0)[0]
            else:
                acc[0] += calculate_psnr_pt(o[None].float(), g[None].to(dev).float(), crop_border=0)[0]
            acc[1] += 1
        if world > 1:
            dist.all_reduce(acc)
        psnr = acc[0] / acc[1].clamp_min(1)
    return outs, psnr
