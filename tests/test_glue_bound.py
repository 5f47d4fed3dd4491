"""The bounds of tests/test_gpu_glue.py on the CPU, in the manner of tests/test_parity_bound.py: the glue kernels emulated in fp32
torch / numpy stay below the element bound against the fp64 references of tests/glue_reference.py, and each defect such a kernel
could have — one window's accumulation dropped, `count` wrong on a plane > 0, a store where an accumulation belongs, tile weights
swapped between two tiles, zero padding instead of the replicate clamp at one border, an out-of-range t wrapped instead of clamped,
the grid-stride loop's second trip missing — pushes the ratio above 1.  The last tests document why the new cases exist: the gates
the suite had before (`rel < 1e-6` at its one shape, the tiled VAE's whole-tensor tolerance) pass the localised ones."""
import numpy as np
import pytest
import torch

import glue_reference as R
from edtr_amd import tiling
from edtr_amd.testing import elem_ratio, rel_err

F32 = torch.float32
GRID_SPAN = R.GRID_SPAN


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- tile accumulate ---------------------------------------------------------------------------------------------------------------
def _overlap_case(B=2, C=5, H=20, W=28, size=8, stride=4, zero=False):
    windows = [(hi, wi, size, size) for hi, _, wi, _ in tiling.sliding_windows(H, W, size, stride)]
    out0 = torch.zeros((B, C, H, W)) if zero else _rnd((B, C, H, W), 1) + 0.25
    cnt0 = torch.zeros((B, C, H, W)) if zero else _rnd((B, C, H, W), 2).abs() + 0.5
    w = torch.tensor(tiling.gaussian_weights(size, size), dtype=F32)
    tiles = [_rnd((B, C, size, size), 10 + i) for i in range(len(windows))]
    return out0, cnt0, tiles, [w] * len(windows), windows


def _emulated_accumulate(out0, cnt0, tiles, wts, windows):
    """The kernel in fp32: out += tile * w, count += w, window by window."""
    out, cnt = out0.clone(), cnt0.clone()
    for t, w, (hi, wi, th, tw) in zip(tiles, wts, windows):
        out[..., hi:hi + th, wi:wi + tw] += t * w
        cnt[..., hi:hi + th, wi:wi + tw] += w
    return out, cnt


def test_correct_tile_accumulate_stays_below_the_bound():
    case = _overlap_case()
    out, cnt = _emulated_accumulate(*case)
    ref, aref, cref, acref, cover = R.tile_accumulate_ref(*case)
    assert elem_ratio(out, ref, cover * aref, F32, 1)[0] < 0.6
    assert elem_ratio(cnt, cref, cover * acref, F32, 1)[0] < 0.6
    assert elem_ratio(out / cnt, out.double() / cnt.double(), None, F32, 0)[0] <= 1.0              # the division: one rounding of its own operands


@pytest.mark.parametrize("defect", [("drop", 0), ("drop", 7), ("drop", 23), "count_plane0", "store"])
def test_each_tile_accumulate_defect_exceeds_the_bound(defect):
    case = _overlap_case()
    ref, aref, cref, acref, cover = R.tile_accumulate_ref(*case)
    bad, _, bad_cnt, _, _ = R.tile_accumulate_ref(*case, defect=defect)
    worst = max(elem_ratio(bad, ref, cover * aref, F32, 1)[0], elem_ratio(bad_cnt, cref, cover * acref, F32, 1)[0])
    assert worst > 1e3, (defect, worst)


def test_the_old_tile_accumulate_gate_passes_a_wrong_count_plane_and_a_store():
    """What tests/test_gpu_ops.py::test_sampler_kernels checks: one 8 x 8 window into ZEROED 16 x 24 planes with B = 1, `rel < 1e-6`
    on out and on plane 0 of count.  A kernel that accumulates count on plane 0 only, or stores instead of accumulating, passes
    it: nothing is accumulated onto a non-zero value and the other planes of count are never read."""
    out0, cnt0 = torch.zeros((1, 4, 16, 24)), torch.zeros((1, 4, 16, 24))
    tile, w = _rnd((1, 4, 8, 8), 83), _rnd((8, 8), 84).abs() + 0.1
    args = (out0, cnt0, [tile], [w], [(4, 16, 8, 8)])
    want = torch.zeros(1, 4, 16, 24, dtype=torch.float64)
    want[..., 4:12, 16:24] = (tile * w).double()
    for defect in ("count_plane0", "store"):
        out, _, cnt, _, _ = R.tile_accumulate_ref(*args, defect=defect)
        assert rel_err(out, want) < 1e-6 and rel_err(cnt[0, 0, 4:12, 16:24], w) < 1e-6, defect
    # the new overlap-add case rejects both (test above); the correct kernel passes the old gate as well
    out, cnt = _emulated_accumulate(*args)
    assert rel_err(out, want) < 1e-6 and rel_err(cnt[0, 0, 4:12, 16:24], w) < 1e-6


# ---- GroupNorm pooling ---------------------------------------------------------------------------------------------------------------
def _pool_case(T=3, BG=64, cpg=2):
    pix = [48 * 40, 48 * 24, 16 * 40, 32 * 40, 48 * 8, 16 * 24][:T]
    tiles = [(_rnd((BG, p * cpg), 30 + t) * (1.0 + 0.3 * t) + 0.4 * t - 0.5).numpy() for t, p in enumerate(pix)]
    sums, _ = R.tile_sums(tiles)
    weights = np.array([p / sum(pix) for p in pix], dtype=np.float32)
    counts = np.array([p * cpg for p in pix], dtype=np.float32)
    return tiles, sums, weights, counts


def _emulated_pool(sums, weights, counts):
    """The kernel's operations in another association (means and variances of all tiles first, then the weighted sums by a dot
    product): fp64, so it may differ from the restatement in the last bits only."""
    w, c = weights.astype(np.float64)[:, None], counts.astype(np.float64)[:, None]
    m = sums[..., 0] / c
    v = np.maximum(sums[..., 1] / c - m * m, 0.0)
    mean, var = np.einsum("tb,tb->b", np.broadcast_to(w, m.shape), m), np.einsum("tb,tb->b", np.broadcast_to(w, v.shape), v)
    return np.stack([mean[None] * c, (var + mean * mean)[None] * c], axis=-1)


def test_correct_gn_pool_stays_below_the_bound_and_swapped_weights_exceed_it():
    _, sums, weights, counts = _pool_case()
    ref, bound = R.gn_pool_ref(sums, weights, counts)
    assert (np.abs(_emulated_pool(sums, weights, counts) - ref) / bound).max() <= 1.0
    for a, b in ((0, 1), (1, 2), (0, 2)):
        bad, _ = R.gn_pool_ref(sums, weights, counts, defect=("swap", a, b))
        assert (np.abs(bad - ref) / bound).max() > 1e6, (a, b)
    # counts[t] swapped with a neighbour's: the pair no longer reproduces the pooled mean for that tile
    bad = ref.copy()
    bad[0], bad[1] = ref[0] / counts[0] * counts[1], ref[1] / counts[1] * counts[0]
    assert (np.abs(bad - ref) / bound).max() > 1e6


def test_the_tiled_vae_tolerance_passes_swapped_tile_weights():
    """edtr_gn_pool was covered by test_tiled_vae_vs_reference_golden only: whole-tensor relative L2 of the VAE output at 2.2e-3
    (fp16; bf16 is wider).  For two tiles of near-equal size (48 x 40 and 48 x 36 pixels) whose statistics differ by a percent, as
    neighbouring tiles of one image do, normalising with the statistics that SWAPPED weights give moves a layer's output by
    ~1e-3 of its norm: below that gate, while the element check of the pooled pair rejects it by six orders of magnitude."""
    BG, cpg = 64, 2
    pix = [48 * 40, 48 * 36]
    tiles = [(_rnd((BG, p * cpg), 40 + t) * (1.0 + 0.01 * t) + 0.01 * t - 0.5).numpy() for t, p in enumerate(pix)]
    sums, _ = R.tile_sums(tiles)
    weights = np.array([p / sum(pix) for p in pix], dtype=np.float32)
    counts = np.array([p * cpg for p in pix], dtype=np.float32)
    ref, bound = R.gn_pool_ref(sums, weights, counts)
    bad, _ = R.gn_pool_ref(sums, weights, counts, defect=("swap", 0, 1))
    assert (np.abs(bad - ref) / bound).max() > 1e6

    def normalised(pooled):
        outs = []
        for t, x in enumerate(tiles):
            m = pooled[t, :, 0:1] / counts[t]
            v = pooled[t, :, 1:2] / counts[t] - m * m
            outs.append(((x - m) / np.sqrt(v + 1e-6)).reshape(-1))
        return torch.from_numpy(np.concatenate(outs))
    moved = rel_err(normalised(bad), normalised(ref))
    assert 1e-6 < moved < 2.2e-3, moved


# ---- wavelet level -------------------------------------------------------------------------------------------------------------------
def _emulated_wavelet(x, r):
    """The kernel's expression in fp32, in its order: corners, edges, centre."""
    P, H, W = x.shape
    ys, xs = torch.arange(H), torch.arange(W)
    ym, yp, xm, xp = (ys - r).clamp(0, H - 1), (ys + r).clamp(0, H - 1), (xs - r).clamp(0, W - 1), (xs + r).clamp(0, W - 1)

    def g(yi, xi):
        return x[:, yi][:, :, xi]
    return (0.0625 * (g(ym, xm) + g(ym, xp) + g(yp, xm) + g(yp, xp)) + 0.125 * (g(ym, xs) + g(yp, xs) + g(ys, xm) + g(ys, xp))) + 0.25 * x


@pytest.mark.parametrize("planes,H,W,r", [(7, 12, 17, 1), (7, 12, 17, 16), (7, 12, 17, 64), (1, 1, 33, 2), (1, 33, 1, 2), (2, 5, 5, 4)])
def test_correct_wavelet_level_stays_below_the_bound_and_zero_padding_exceeds_it(planes, H, W, r):
    x = _rnd((planes, H, W), 50 + r) + 0.3
    ref, aref = R.wavelet_level_ref(x.numpy(), r)
    assert elem_ratio(_emulated_wavelet(x, r), torch.from_numpy(ref), torch.from_numpy(aref), F32, 9)[0] < 0.6
    if H > 1:
        bad, _ = R.wavelet_level_ref(x.numpy(), r, defect="zero_bottom")
        assert elem_ratio(torch.from_numpy(bad), torch.from_numpy(ref), torch.from_numpy(aref), F32, 9)[0] > 1e3


def test_wavelet_reference_agrees_with_a_padded_convolution():
    """The index-clamp gather against the other formulation (replicate pad + dilated conv2d), so that the reference itself is not
    taken on trust."""
    import torch.nn.functional as F
    x = _rnd((3, 13, 11), 60).double()
    k = torch.tensor([[1.0, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=torch.float64) / 16
    for r in (1, 2, 4):
        ref, _ = R.wavelet_level_ref(x.numpy(), r)
        conv = F.conv2d(F.pad(x[:, None], (r, r, r, r), mode="replicate"), k[None, None], dilation=r)[:, 0]
        assert np.abs(ref - conv.numpy()).max() < 1e-14


# ---- q_sample -------------------------------------------------------------------------------------------------------------------------
def _tables():
    from edtr_amd.diffusion import Diffusion
    diff = Diffusion()
    return diff.sqrt_alphas_cumprod.numpy(), diff.sqrt_one_minus_alphas_cumprod.numpy()


def test_q_sample_bound_rejects_a_wrapped_t_which_the_old_cases_never_reach():
    ta, tb = _tables()
    x, noise = _rnd((5, 4, 6, 7), 70).numpy(), _rnd((5, 4, 6, 7), 71).numpy()
    t = [0, 999, 200, -3, 5000]
    ref, absref, fp32 = R.q_sample_ref(x, noise, t, ta, tb)
    assert elem_ratio(fp32, ref, absref, F32, 2)[0] < 0.6             # the pinned fp32 expression itself
    bad, _, bad32 = R.q_sample_ref(x, noise, t, ta, tb, defect="t_mod")
    assert elem_ratio(bad, ref, absref, F32, 2)[0] > 1e3 and not torch.equal(bad32, fp32)
    # every t the suite used before lies inside the table: there the wrapped read is the clamped read, bit for bit
    t_old = [0, 999, 200, 437, 10]
    assert torch.equal(R.q_sample_ref(x, noise, t_old, ta, tb, defect="t_mod")[2], R.q_sample_ref(x, noise, t_old, ta, tb)[2])
    # an image boundary off by one element (i / per_image rounded the wrong way for the first element of an image)
    off = ref.clone().reshape(5, -1)
    off[1:, 0] = (R.q_sample_ref(x, noise, [0] + t[:-1], ta, tb)[0]).reshape(5, -1)[1:, 0]
    assert elem_ratio(off.reshape(ref.shape), ref, absref, F32, 2)[0] > 1e3


# ---- the grid-stride loop's second trip ----------------------------------------------------------------------------------------------------
def test_a_missing_second_trip_exceeds_the_bound_only_above_one_grid_span():
    """blocks_for() caps the grid at 4096 blocks of 256: a kernel whose loop runs once leaves elements >= 1 048 576 unwritten.  At
    the largest n the suite used before (2048) such a kernel is indistinguishable from a correct one; at n = 2^20 + 777 the 777
    stale elements exceed the bound (a NaN guard makes the ratio infinite, a stale finite value makes it large)."""
    ta, tb = _tables()
    for n, seen in ((2048, False), (GRID_SPAN + 777, True)):
        x, noise = _rnd((1, n), 80).numpy(), _rnd((1, n), 81).numpy()
        ref, absref, fp32 = R.q_sample_ref(x, noise, [437], ta, tb)
        for stale in (float("nan"), 0.0):
            got = R.second_trip_missing(fp32, stale)
            ratio = elem_ratio(got, ref, absref, F32, 2)[0]
            assert (ratio > 1e3) == seen, (n, stale, ratio)
