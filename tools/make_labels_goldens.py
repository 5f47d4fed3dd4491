#!/usr/bin/env python
"""Write tests/golden/labels.npz for tests/test_labels_cpu.py and tests/test_gpu_labels.py:

  * what Pillow's `Image.resize(size, Image.NEAREST)` returns for seeded label maps (mode "L") and images (mode "RGB") at the extents
    below, with the Pillow version that produced them;
  * the REFERENCE's own functions on recorded inputs, on the CPU: `calculate_mat` as main/seg/test_edtr.py:159 calls it, `compute_iou`
    (also on a matrix with an absent class and on one whose sums exceed 2^24) and `convert2color` through save_image's quantisation;
  * the reference's colour table, recorded by running `convert2color` on the labels 0 ... 20 and 255 (it is not copied into the source).

Only arrays go into the file, and the archive is written with fixed time stamps: the same inputs give the same bytes.

    python tools/make_labels_goldens.py [--out tests/golden/labels.npz]       (needs Pillow and the reference tree; see tools/ref_import.py)
"""
from __future__ import annotations

import argparse
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ref_import  # noqa: E402

# (input h, input w, output h, output w): at 2 -> 7, 2 -> 15 and 500 -> 546 Pillow's accumulating rule and the closed form disagree
NEAREST_CASES = [(2, 2, 7, 15), (3, 2, 21, 7), (1, 5, 1, 1), (5, 1, 3, 9), (2, 64, 23, 33), (9, 9, 9, 9), (281, 500, 307, 546)]
N_CLASSES = 21


def install_segmentation_stubs() -> None:
    """Stand-ins for what utils/segmentation.py imports at module level and the three functions called here never touch:
    `accelerate` (not installed) and the reference's own utils.common (which pulls in the whole model package)."""
    for name, attrs in (("accelerate", {}), ("accelerate.utils", dict(set_seed=lambda seed: None)), ("utils", {}),
                        ("utils.common", dict(copy_opt_file=None, print_attn_type=None, Logger=None))):
        if name not in sys.modules:
            ref_import._module(name, **attrs)


def position_map(h: int, w: int, channels: int) -> np.ndarray:
    """uint8 [h, w] or [h, w, 3] that encodes the position: a 16 x 16 tile of the 256 byte values (a source index that is wrong by
    anything but a multiple of 16 shows), and in the other two channels the tile's column and row (any wrong index shows).
    Repetitive on purpose: the archive deflates it well."""
    y, x = np.mgrid[0:h, 0:w]
    planes = [(x % 16) + 16 * (y % 16), x // 16, y // 16]
    return planes[0].astype(np.uint8) if channels == 1 else np.stack(planes, axis=-1).astype(np.uint8)


def save_image_bytes(x: torch.Tensor) -> np.ndarray:
    """torchvision's save_image quantisation of a [1, 3, H, W] tensor in [0, 1] -> uint8 [H, W, 3]"""
    return x[0].mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()


def write_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed with fixed time stamps and a fixed member order: equal arrays give equal bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "labels.npz"))
    args = ap.parse_args()
    import PIL
    from PIL import Image
    install_segmentation_stubs()
    seg = ref_import.import_reference_file("ref_utils_segmentation", "utils/segmentation.py")

    out = {"pillow_version": np.array(PIL.__version__), "nearest_cases": np.array(NEAREST_CASES, dtype=np.int32)}
    for i, (h, w, oh, ow) in enumerate(NEAREST_CASES):
        for ch in (1, 3):
            src = position_map(h, w, ch)
            dst = np.array(Image.fromarray(src).resize((ow, oh), Image.NEAREST))
            assert dst.shape == (oh, ow) + ((3,) if ch == 3 else ()) and dst.dtype == np.uint8
            out[f"nearest{i}_c{ch}_in"], out[f"nearest{i}_c{ch}_out"] = src, dst

    # calculate_mat(mask, pred, n): two images, every class, the ignore label and two other values >= n among the targets
    rng = np.random.default_rng(20260)
    logits = rng.standard_normal((2, N_CLASSES, 9, 12)).astype(np.float32)
    target = rng.integers(0, N_CLASSES, size=(2, 9, 12)).astype(np.uint8)
    target[0].reshape(-1)[:N_CLASSES] = np.arange(N_CLASSES)
    target[0, 8, 9:] = (255, 21, 200)
    target[1, :2] = 255
    with torch.no_grad():
        mask_t, out_t = torch.from_numpy(target).long(), torch.from_numpy(logits)
        mat = seg.calculate_mat(mask_t.flatten(), out_t.argmax(1).flatten(), n=N_CLASSES)
        iou = seg.compute_iou(mat)
        # a data set's matrix with class 7 absent from truth and prediction alike: its IoU is 0 / 0
        big = torch.from_numpy(rng.integers(0, 40000, size=(N_CLASSES, N_CLASSES)))
        big[7, :] = 0
        big[:, 7] = 0
        big_iou = seg.compute_iou(big)
        # a whole validation set's counts: every row and column sum above 2^24, where the order of the fp32 additions shows
        huge = torch.from_numpy(rng.integers(0, 4_000_000, size=(N_CLASSES, N_CLASSES)))
        huge[torch.arange(N_CLASSES), torch.arange(N_CLASSES)] *= 8
        huge_iou = seg.compute_iou(huge)
    assert mat.dtype == torch.int64 and int(mat.sum()) == int((target < N_CLASSES).sum())
    assert int(huge.sum(0).min()) > 1 << 24 and int(huge.sum(1).min()) > 1 << 24
    assert bool(torch.isnan(big_iou[7])) and int(torch.isnan(big_iou).sum()) == 1 and int(big.sum(0).max()) < 1 << 24
    out.update(conf_logits=logits, conf_target=target, conf_mat=mat.numpy(), conf_iou=iou.numpy(), conf_miou=np.float64(iou.mean().item() * 100),
               iou_mat=big.numpy(), iou_out=big_iou.numpy(), iou_big_mat=huge.numpy(), iou_big_out=huge_iou.numpy())

    # convert2color -> save_image on a map with every class, the ignore label and two labels it does not name; and its colour table
    labels = rng.integers(0, N_CLASSES, size=(6, 10)).astype(np.uint8)
    labels.reshape(-1)[:N_CLASSES] = np.arange(N_CLASSES)
    labels[5, 7:] = (255, 21, 200)
    named = np.array(list(range(N_CLASSES)) + [255], dtype=np.uint8)
    with torch.no_grad():
        colors = save_image_bytes(seg.convert2color(torch.from_numpy(labels).long()[None]))
        table = save_image_bytes(seg.convert2color(torch.from_numpy(named).long()[None, None]))[0]
    palette = np.zeros((256, 3), dtype=np.uint8)
    palette[named] = table
    out.update(color_labels=labels, color_out=colors, ref_palette=palette)

    write_npz(args.out, out)
    print(f"wrote {args.out}: Pillow {PIL.__version__}, {len(out)} arrays, {os.path.getsize(args.out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
