"""Child process of tests/test_gpu_tiling.py: sets EDTR_AMD_BATCH_INVARIANT=1 BEFORE the package is imported (the variable is read when a
program is emitted), restores two images of one padded extent with the encoder, the sampler and the decoder tiled — one at a time
(pad_mode="demo") and as one batch of two (pad_mode="bucket") — with the same seed, and prints one JSON line with what it found."""
import json
import os
import sys

os.environ["EDTR_AMD_BATCH_INVARIANT"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SIZES = ((136, 200), (150, 230))           # both pad to 192 x 256: a 24 x 32 latent, six 16 / 8 windows


def main() -> dict:
    from edtr_amd import evalutil, imageio, synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.evalutil import TilingOptions
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    d = torch.device("cuda:0")
    cfg = synth.tiny_config()
    cldm = build_synthetic_cldm(cfg, d, torch.float16)
    cldm.clip.set_embedding(synth.synth_input("demo:c_txt", (1, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(d))
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(d)
    sampler = SpacedSampler(diffusion.betas)
    imgs = [synth.synth_input(f"tilechild:img{k}", (3, h, w), 0.0, 1.0) for k, (h, w) in enumerate(SIZES)]
    tiling = TilingOptions(vae_encoder=True, vae_encoder_size=64, vae_decoder=True, vae_decoder_size=8, cldm=True, cldm_size=128, cldm_stride=64)
    kw = dict(img_size=128, multiple=64, seed=7, tiling=tiling)
    plan = imageio.plan_buckets(list(SIZES), 2, min_size=128, multiple=64)
    one, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, pad_mode="demo", **kw)
    two, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, pad_mode="bucket", batch_size=2, **kw)
    plain, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, pad_mode="demo", **dict(kw, tiling=None))
    torch.cuda.synchronize()
    return {"chunks": [idx for _, idx in plan], "shapes": [list(o.shape) for o in two],
            "finite": all(bool(torch.isfinite(o).all()) for o in two),
            "equal": [bool(torch.equal(a, b)) for a, b in zip(one, two)],
            "max_abs_diff": [float((a - b).abs().max()) for a, b in zip(one, two)],
            "tiled_differs_from_untiled": [not torch.equal(a, b) for a, b in zip(one, plain)],
            "forward_patched": "forward" in vars(cldm)}


if __name__ == "__main__":
    print("TILING_CHILD " + json.dumps(main()))
