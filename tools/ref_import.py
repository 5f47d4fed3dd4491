"""Make the read-only reference tree at /root/reference importable on CPU in THIS container.

Only used by tools/make_goldens.py, tools/make_degrade_goldens.py and tools/make_degrade2_goldens.py (fixture generation) — never by tests, bench or the
product.  The reference needs four packages the image lacks (torchvision, omegaconf, ftfy,
timm); none of them is touched by the restoration hot path, so inert
stand-in modules are registered before the import.
"""
from __future__ import annotations

import sys
import types

import torch

REFERENCE_ROOT = "/root/reference"


def _module(name: str, **attrs) -> types.ModuleType:
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    return mod


class _PassThrough:
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, x, *args, **kwargs):
        return x


class _NoDropPath(torch.nn.Identity):
    def __init__(self, *args, **kwargs):
        super().__init__()


def install_stubs() -> None:
    if "torchvision" not in sys.modules:
        tv = _module("torchvision")
        tvt = _module("torchvision.transforms")
        tvt.transforms = _module("torchvision.transforms.transforms", Normalize=_PassThrough)
        tvt.functional = _module("torchvision.transforms.functional", normalize=lambda x, *a, **k: x)
        tv.transforms = tvt
        tv.models = _module("torchvision.models", get_model=lambda *a, **k: None)
    if "ftfy" not in sys.modules:
        _module("ftfy", fix_text=lambda s: s)
    if "timm" not in sys.modules:
        _module("timm")
        _module("timm.models")
        _module(
            "timm.models.layers",
            DropPath=_NoDropPath,
            trunc_normal_=torch.nn.init.trunc_normal_,
            to_2tuple=lambda v: v if isinstance(v, tuple) else (v, v),
        )
    if "omegaconf" not in sys.modules:
        _module("omegaconf")
        _module("omegaconf.listconfig", ListConfig=type("ListConfig", (list,), {}))


def install_degrade_stubs() -> None:
    """Stand-ins for what datasets/utils.py and datasets/degradation.py import at module level and the degradation functions
    that tools/make_degrade_goldens.py calls never touch: cv2 and torchvision's rgb_to_grayscale."""
    if "cv2" not in sys.modules:
        _module("cv2")
    install_stubs()
    if "torchvision.transforms._functional_tensor" not in sys.modules:
        _module("torchvision.transforms._functional_tensor", rgb_to_grayscale=lambda x, *a, **k: x)


def install_degrade2_stubs() -> None:
    """`install_degrade_stubs`, with the two stand-ins that tools/make_degrade2_goldens.py DOES call filled in by their published
    formulas: cv2.getGaussianKernel(k, sigma) for a non-positive sigma and k > 7 (sigma = 0.3 ((k - 1) 0.5 - 1) + 0.8, fp64, [k, 1]),
    and torchvision's rgb_to_grayscale ((0.2989 r + 0.587 g) + 0.114 b on the channel axis)."""
    import numpy as np
    install_degrade_stubs()

    def get_gaussian_kernel(ksize, sigma):
        assert ksize > 7 and ksize % 2 == 1, "only the formula branch of cv2.getGaussianKernel is stood in for"
        if sigma <= 0:
            sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
        i = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
        g = np.exp(-(i * i) / (2.0 * sigma * sigma))
        return (g / g.sum()).reshape(ksize, 1)

    def rgb_to_grayscale(img, num_output_channels=1):
        r, g, b = img.unbind(dim=-3)
        gray = (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)
        return gray.expand(img.shape) if num_output_channels == 3 else gray

    sys.modules["cv2"].getGaussianKernel = get_gaussian_kernel
    sys.modules["torchvision.transforms._functional_tensor"].rgb_to_grayscale = rgb_to_grayscale


def import_reference_file(name: str, relpath: str):
    """One source file of the reference as a module of its own (its package's __init__ is not run)."""
    import importlib.util
    import os
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location(name, os.path.join(REFERENCE_ROOT, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    """Returns (ControlLDM, Diffusion, SpacedSampler, ref_common_module)."""
    sys.dont_write_bytecode = True
    install_stubs()
    if REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, REFERENCE_ROOT)
    import model  # noqa: F401  (reference package)
    from model.cldm import ControlLDM
    from model.gaussian_diffusion import Diffusion
    from utils.sampler import SpacedSampler
    import utils.common as ref_common
    return ControlLDM, Diffusion, SpacedSampler, ref_common
