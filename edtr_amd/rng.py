"""Seeded per-image Gaussian noise (include/edtr_hip.h, "Reproducible noise"): the value an element receives is a pure
function of (seed, image id, purpose, draw, element offset inside the image) and of nothing else — not of the batch an
image travels in, its position there, or the number of ranks that share the data set.

The stream (normative; csrc/rng.hip evaluates the same thing inside the kernels that consume the noise):

  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
  key     = (seed & 0xffffffff, seed >> 32)
  counter = (e >> 2, draw, purpose, image_id)       e = (c*H + h)*W + w, the element's offset inside its NCHW image
  one call -> words x0..x3 -> the normals of elements 4*(e>>2) + 0..3 by Box-Muller:
      u1 = ((x0 >> 8) + 1) * 2^-24  in (0, 1],  u2 = (x1 >> 8) * 2^-24  in [0, 1),  r = sqrt(-2 ln u1)
      z0 = r cos(2 pi u2), z1 = r sin(2 pi u2);  z2, z3 the same from (x2, x3)         |z| <= sqrt(48 ln 2) = 5.77

This module is the host side: the numpy restatement the kernels are tested against, and `NoiseSource`, the description of
"whose noise" that the sampler / q_sample / vae_encode / restore_dataset accept.  No kernel is launched from here."""
from __future__ import annotations

from typing import List, Sequence, Union

import numpy as np

PURPOSE_Q_SAMPLE, PURPOSE_STEP, PURPOSE_X_T, PURPOSE_VAE = 0, 1, 2, 3
PURPOSES = (PURPOSE_Q_SAMPLE, PURPOSE_STEP, PURPOSE_X_T, PURPOSE_VAE)
# colour / grey noise of edtr_degrade_gaussian_noise (draw = the degradation stage): the same stream, but drawn by that kernel alone —
# edtr_normal_fill and `normal_reference` keep refusing them, `stream_reference` evaluates them
PURPOSE_DEGRADE, PURPOSE_DEGRADE_GRAY = 4, 5
DEGRADE_PURPOSES = (PURPOSE_DEGRADE, PURPOSE_DEGRADE_GRAY)
# colour / grey noise of edtr_degrade_poisson_noise: the raw words of the same counters (`uniform_words_reference`), never normals
PURPOSE_DEGRADE_POISSON, PURPOSE_DEGRADE_POISSON_GRAY = 6, 7
POISSON_PURPOSES = (PURPOSE_DEGRADE_POISSON, PURPOSE_DEGRADE_POISSON_GRAY)
# the keys of `targets.sample` in place of torch.randperm (draw = the training step), for the RPN's anchors and the box head's proposals:
# raw words again; only `uniform_words_reference` evaluates them
PURPOSE_SAMPLE_RPN, PURPOSE_SAMPLE_ROI = 8, 9
SAMPLE_PURPOSES = (PURPOSE_SAMPLE_RPN, PURPOSE_SAMPLE_ROI)
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))      # u1 >= 2^-24: no value of the stream is larger in magnitude

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 on uint32 arrays: ``counter`` [..., 4], ``key`` [..., 2] (broadcast against each other) -> [..., 4]."""
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).astype(np.uint64) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).astype(np.uint64) for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                 # 32 x 32 -> 64 (no overflow in uint64)
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _check_seed(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    return seed


def _check_ids(image_ids) -> List[int]:
    if hasattr(image_ids, "tolist"):                # torch tensor / numpy array
        image_ids = image_ids.tolist()
    ids = [int(v) for v in image_ids]
    for v in ids:
        if not 0 <= v < 1 << 32:
            raise ValueError(f"image id {v} is outside [0, 2^32)")
    return ids


def normal_reference(seed: int, image_ids, purpose: int, draw, per_image: int) -> np.ndarray:
    """float64 [B][per_image]: the stream of the module docstring, evaluated in double precision from the exact uniforms.
    ``draw`` is one int for the whole batch or one per image (the device-index sampler form reads it per image)."""
    if purpose not in PURPOSES:
        raise ValueError(f"purpose must be one of {PURPOSES}, got {purpose}")
    return stream_reference(seed, image_ids, purpose, draw, per_image)


def uniform_words_reference(seed: int, image_ids, purpose: int, draw, per_image: int) -> np.ndarray:
    """uint32 [B][per_image]: the raw Philox words of the stream, element e of an image receiving word e & 3 of the call on the counter
    (e >> 2, draw, purpose, image id) — what edtr_degrade_poisson_noise inverts its tables with.  Every purpose of the header."""
    if purpose not in PURPOSES + DEGRADE_PURPOSES + POISSON_PURPOSES + SAMPLE_PURPOSES:
        raise ValueError(f"purpose must be one of {PURPOSES + DEGRADE_PURPOSES + POISSON_PURPOSES + SAMPLE_PURPOSES}, got {purpose}")
    return _words(seed, image_ids, purpose, draw, per_image).reshape(-1, per_image)


def _words(seed: int, image_ids, purpose: int, draw, per_image: int) -> np.ndarray:
    """uint32 [B][per_image / 4][4]: one Philox call per group of four elements"""
    seed, ids = _check_seed(seed), _check_ids(image_ids)
    if per_image <= 0 or per_image % 4:
        raise ValueError(f"per_image must be a positive multiple of 4, got {per_image}")
    B, G = len(ids), per_image // 4
    draws = np.broadcast_to(np.asarray(draw, dtype=np.int64).reshape(-1), (B,)) if B else np.zeros(0, np.int64)
    if ((draws < 0) | (draws >= 1 << 32)).any():
        raise ValueError("draw must be in [0, 2^32)")
    ctr = np.empty((B, G, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(G, dtype=np.uint32)[None, :]
    ctr[..., 1] = draws.astype(np.uint32)[:, None]
    ctr[..., 2] = purpose
    ctr[..., 3] = np.asarray(ids, dtype=np.uint32).reshape(B, 1)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))


def stream_reference(seed: int, image_ids, purpose: int, draw, per_image: int) -> np.ndarray:
    """`normal_reference` for every purpose of the header that draws normals, the two of the degradation stage (`DEGRADE_PURPOSES`)
    included."""
    if purpose not in PURPOSES + DEGRADE_PURPOSES:
        raise ValueError(f"purpose must be one of {PURPOSES + DEGRADE_PURPOSES}, got {purpose}")
    x = _words(seed, image_ids, purpose, draw, per_image)
    B, G = x.shape[:2]
    out = np.empty((B, G, 4), dtype=np.float64)
    for j in (0, 2):
        u1 = ((x[..., j] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (x[..., j + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[..., j], out[..., j + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
    return out.reshape(B, per_image)


def shard_chunk_ids(n_images: int, rank: int, world: int, batch_size: int, pad_mode: str = "batch") -> List[List[int]]:
    """The global image ids of every chunk that `evalutil.restore_dataset` runs on this rank: its `shard_slice` of the
    ``n_images`` inputs cut into chunks of ``batch_size`` (of 1 for pad_mode="demo" and "seg").  Image k of the data set has id k
    whatever the rank count and the chunking, which is what makes a seeded restoration independent of both."""
    from .parallel import shard_slice
    if pad_mode not in ("batch", "demo", "seg"):
        raise ValueError(f"pad_mode must be 'batch', 'demo' or 'seg', got {pad_mode!r}")
    step = 1 if pad_mode in ("demo", "seg") else int(batch_size)
    if step <= 0:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    sl = shard_slice(rank, world, n_images)
    mine = list(range(sl.start, sl.stop))
    return [mine[i:i + step] for i in range(0, len(mine), step)]


def shard_bucket_ids(n_images: int, rank: int, world: int, plan) -> List[List[int]]:
    """The global image ids of every chunk of `evalutil.restore_dataset(pad_mode="bucket")` on this rank: ``plan`` is
    `imageio.plan_buckets` of the sizes of this rank's `shard_slice` (indices inside the shard); image k of the data set keeps id k
    whatever bucket it lands in."""
    from .parallel import shard_slice
    sl = shard_slice(rank, world, n_images)
    count = sl.stop - sl.start
    out = []
    for _, idx in plan:
        for i in idx:
            if not 0 <= int(i) < count:
                raise ValueError(f"index {i} of the plan is outside this rank's shard of {count} images")
        out.append([sl.start + int(i) for i in idx])
    return out


class NoiseSource:
    """Whose noise: the 64-bit ``seed`` and the GLOBAL ids (data-set indices, not batch positions) of the images of this
    batch, in batch order.  Immutable; owns the device copy of the ids that the kernels read (built on first use, per device)."""
    __slots__ = ("_seed", "_ids", "_dev")

    def __init__(self, seed: int, image_ids: Union[Sequence[int], "np.ndarray"]):
        object.__setattr__(self, "_seed", _check_seed(seed))
        object.__setattr__(self, "_ids", tuple(_check_ids(image_ids)))
        object.__setattr__(self, "_dev", {})
        if not self._ids:
            raise ValueError("NoiseSource needs at least one image id")

    @classmethod
    def for_shard(cls, seed: int, start: int, count: int) -> "NoiseSource":
        """The contiguous case: images start .. start + count - 1 of the data set."""
        return cls(seed, range(int(start), int(start) + int(count)))

    def __setattr__(self, name, value):
        raise AttributeError("NoiseSource is immutable")

    @property
    def seed(self) -> int:
        return self._seed

    @property
    def image_ids(self) -> tuple:
        return self._ids

    def __len__(self) -> int:
        return len(self._ids)

    def __repr__(self) -> str:
        return f"NoiseSource(seed={self._seed}, image_ids={list(self._ids)})"

    def check_batch(self, batch: int, what: str = "") -> "NoiseSource":
        if len(self._ids) != int(batch):
            raise ValueError(f"{what or 'NoiseSource'}: {len(self._ids)} image ids for a batch of {int(batch)}")
        return self

    def ids_on(self, device):
        """int64 [B] tensor of the ids on ``device`` (cached: a sampler loop uploads them once)."""
        import torch
        key = str(torch.device(device))
        hit = self._dev.get(key)
        if hit is None:
            hit = self._dev[key] = torch.tensor(self._ids, dtype=torch.int64).to(device)
        return hit

    def reference(self, purpose: int, draw, per_image: int) -> np.ndarray:
        return normal_reference(self._seed, self._ids, purpose, draw, per_image)
