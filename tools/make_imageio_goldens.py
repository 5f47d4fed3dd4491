#!/usr/bin/env python
"""Writes tests/golden/pillow_bicubic.npz: seeded uint8 images and what Pillow's `Image.resize(size, Image.BICUBIC)` returns for
them, plus the Pillow version that produced them.  The tests compare edtr_amd.imageio.resize_u8_reference (CPU) and the device
resize (GPU) with these bytes, so they do not need Pillow installed.  Every array is at most 256 x 256.

    python tools/make_imageio_goldens.py [--out tests/golden/pillow_bicubic.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, input h, input w, output h, output w)
CASES = [
    ("up", 40, 60, 136, 204),                   # up-scale, both axes
    ("down_wide", 256, 192, 50, 37),            # down-scale by more than 2 x: windows wider than the 5 taps of an up-scale
    ("down_mild", 96, 128, 72, 96),             # down-scale by less than 2 x, sizes that are multiples of 4
    ("w_only", 37, 53, 37, 200),                # the vertical pass is skipped
    ("h_only", 64, 64, 33, 64),                 # the horizontal pass is skipped
    ("odd", 111, 167, 37, 55),                  # odd sizes on both sides
    ("one_wide", 90, 1, 31, 1),                 # a 1-pixel-wide image
    ("one_wide_up", 17, 1, 40, 3),              # ... widened: every window is the single column
    ("one_high", 1, 77, 5, 129),                # a 1-pixel-high image
    ("identity", 24, 36, 24, 36),               # both passes skipped
]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pillow_bicubic.npz"))
    args = ap.parse_args()
    import PIL
    from PIL import Image
    arrays = {"pillow_version": np.array(PIL.__version__), "names": np.array([c[0] for c in CASES])}
    for i, (name, h, w, oh, ow) in enumerate(CASES):
        assert max(h, w, oh, ow) <= 256
        rng = np.random.default_rng(20240 + i)
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        if name == "down_mild":                 # saturated blocks: overshoot on both sides of the clamp
            img[::7] = 255
            img[3::7] = 0
        out = np.array(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
        assert out.shape == (oh, ow, 3) and out.dtype == np.uint8
        arrays[f"{name}_in"], arrays[f"{name}_out"] = img, out
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {len(CASES)} cases, Pillow {PIL.__version__}, {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
