"""Child process of tests/test_gpu_imagebatch.py: sets EDTR_AMD_BATCH_INVARIANT=1 BEFORE the package is imported (the variable is read
when a program is emitted, and the parent's engines were built without it), runs the batched flows against the one-at-a-time flows
on the tiny synthetic model and prints one JSON line with what it found.  Usage: python imagebatch_child.py WORKDIR"""
import json
import os
import sys

os.environ["EDTR_AMD_BATCH_INVARIANT"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (h, w): with img_size 128 / multiple 64 images 0, 1, 2, 4 share the 128 x 128 bucket and image 3 pads to 192 x 128
SIZES = ((100, 75), (64, 128), (37, 53), (130, 60), (90, 100))


def images():
    rng = np.random.default_rng(3)
    out = []
    for h, w in SIZES:
        base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        out.append(np.ascontiguousarray(np.kron(base, np.ones((8, 8, 1), dtype=np.uint8))[:h, :w]))
    return out


def tiny(d):
    from edtr_amd import synth
    from edtr_amd.diffusion import Diffusion
    from edtr_amd.sampler import SpacedSampler
    from edtr_amd.testing import build_synthetic_cldm
    cfg = synth.tiny_config()
    cldm = build_synthetic_cldm(cfg, d, torch.float16)
    cldm.clip.set_embedding(synth.synth_input("demo:c_txt", (1, 77, cfg["unet_cfg"]["context_dim"]), -1.0, 1.0).to(d))
    diffusion = Diffusion(linear_start=0.00085, linear_end=0.0120, timesteps=1000).to(d)
    return cldm, diffusion, SpacedSampler(diffusion.betas)


def main(work: str) -> dict:
    from PIL import Image
    from edtr_amd import evalutil, restore
    d = torch.device("cuda:0")
    cldm, diffusion, sampler = tiny(d)
    imgs = images()
    kw = dict(img_size=128, multiple=64)
    found = {}
    # restore_dataset: bucketed in threes against one at a time
    one, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, pad_mode="demo", seed=7, **kw)
    bkt, _ = evalutil.restore_dataset(cldm, diffusion, sampler, imgs, pad_mode="bucket", batch_size=3, seed=7, **kw)
    torch.cuda.synchronize()
    found["dataset_shapes"] = [list(o.shape) for o in bkt]
    found["dataset_equal"] = [bool(torch.equal(a, b)) for a, b in zip(one, bkt)]
    found["dataset_max_abs_diff"] = [float((a - b).abs().max()) for a, b in zip(one, bkt)]
    found["dataset_finite"] = all(bool(torch.isfinite(o).all()) for o in bkt)
    # restore_files: batches of three with two workers against the untouched default path
    src = os.path.join(work, "in")
    os.makedirs(src)
    for k, a in enumerate(imgs):
        Image.fromarray(a).save(os.path.join(src, f"im{k}.png"))
    paths = restore.list_images(src)
    fast = restore.restore_files(cldm, diffusion, sampler, paths, os.path.join(work, "fast"), scale=1.25, seed=7, batch_size=3, workers=2, **kw)
    slow = restore.restore_files(cldm, diffusion, sampler, paths, os.path.join(work, "slow"), scale=1.25, seed=7, batch_size=1, workers=0, **kw)
    inline = restore.restore_files(cldm, diffusion, sampler, paths, os.path.join(work, "inline"), scale=1.25, seed=7, batch_size=3, **kw)
    found["files_names"] = [[os.path.basename(p) for p in lst] for lst in (fast, slow, inline)]
    equal, shapes = [], []
    for f, s, i in zip(fast, slow, inline):
        with Image.open(f) as a, Image.open(s) as b, Image.open(i) as c:
            pa, pb, pc = np.array(a.convert("RGB")), np.array(b.convert("RGB")), np.array(c.convert("RGB"))
        shapes.append(list(pa.shape))
        equal.append(bool(pa.shape == pb.shape and np.array_equal(pa, pb) and np.array_equal(pa, pc)))
    found["files_equal"], found["files_shapes"] = equal, shapes
    # a corrupt file: the worker's exception comes back on the caller
    with open(os.path.join(src, "im9.png"), "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\nnot an image at all")
    try:
        restore.restore_files(cldm, diffusion, sampler, restore.list_images(src), os.path.join(work, "bad"), scale=1.25, seed=7,
                              batch_size=3, workers=2, **kw)
        found["corrupt_raised"] = None
    except Exception as e:                              # noqa: BLE001  (the parent asserts on the type's name)
        found["corrupt_raised"] = type(e).__name__
    return found


if __name__ == "__main__":
    print("IMAGEBATCH_CHILD " + json.dumps(main(sys.argv[1])))
