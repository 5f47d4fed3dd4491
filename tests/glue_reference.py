"""fp64 references of the fp32 "glue" kernels (tile accumulate / divide, GroupNorm pooling, the wavelet level, the sampler
arithmetic), shared by tests/test_gpu_glue.py (which compares the HIP kernels with them) and tests/test_glue_bound.py (which
shows on the CPU that the element bound rejects the defects such kernels typically have).  Plain numpy / torch on the exact fp32
inputs; nothing here calls the library or the CPU oracle.  Each reference takes an optional ``defect`` that makes it compute what
a broken kernel would: the CPU test feeds those to elem_ratio, the GPU tests never pass one."""
import numpy as np
import torch

GRID_SPAN = 4096 * 256          # elements one trip of the grid-stride loop covers (elementwise.hip blocks_for: <= 4096 blocks of 256)


def f64(t):
    return torch.as_tensor(t).detach().double().cpu()


# ---- tile accumulate -------------------------------------------------------------------------------------------------------------
def tile_accumulate_ref(out0, count0, tiles, wts, windows, defect=None):
    """out0 / count0 [B, C, H, W]; tiles[i] [B, C, th, tw] and wts[i] [th, tw] land at windows[i] = (hi, wi, th, tw).
    Returns (out, |out|-sum, count, |count|-sum, cover + 1): out0 + sum tile w, count0 + sum w, the same sums on absolute values
    (the element bound's absref) and the number of additions each pixel received plus one (its k).
    defect: ("drop", i) skips window i; "count_plane0" accumulates count on plane 0 only; "store" writes instead of adding."""
    out, cnt = f64(out0).clone(), f64(count0).clone()
    a_out, a_cnt = out.abs(), cnt.abs()
    cover = torch.ones(out.shape[-2:], dtype=torch.float64)
    for i, (hi, wi, th, tw) in enumerate(windows):
        if defect == ("drop", i):
            continue
        t, w = f64(tiles[i]), f64(wts[i])
        sl = (Ellipsis, slice(hi, hi + th), slice(wi, wi + tw))
        if defect == "store":
            out[sl], cnt[sl] = t * w, w.expand_as(cnt[sl])
        else:
            out[sl] += t * w
            if defect == "count_plane0":
                cnt[0, 0, hi:hi + th, wi:wi + tw] += w
            else:
                cnt[sl] += w
        a_out[sl] += (t * w).abs()
        a_cnt[sl] += w.abs()
        cover[hi:hi + th, wi:wi + tw] += 1
    return out, a_out, cnt, a_cnt, cover


# ---- GroupNorm pooling (norm.hip gn_pool_kernel restated in numpy float64) -----------------------------------------------------------
def gn_pool_ref(sums, weights, counts, defect=None):
    """sums [T, BG, 2] float64, weights / counts [T] (the float32 values the kernel reads).  Returns (pooled sums, bound): the
    kernel does the same fp64 operations, so |got - ref| <= 4 2^-53 (|ref| + T max|term|) with `term` the largest addend of the
    weighted sums (for the second slot the two sides of the s1/c - m^2 cancellation), scaled by the tile's count.
    defect: ("swap", a, b) exchanges the weights of tiles a and b; "no_clamp" leaves a negative variance negative."""
    s = np.asarray(sums, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    c = np.asarray(counts, dtype=np.float32).astype(np.float64)
    if isinstance(defect, tuple) and defect[0] == "swap":
        w = w.copy()
        w[[defect[1], defect[2]]] = w[[defect[2], defect[1]]]
    T = s.shape[0]
    mean = np.zeros(s.shape[1])
    var = np.zeros(s.shape[1])
    term_m = np.zeros(s.shape[1])
    term_v = np.zeros(s.shape[1])
    for t in range(T):
        m = s[t, :, 0] / c[t]
        v = s[t, :, 1] / c[t] - m * m
        if defect != "no_clamp":
            v = np.where(v < 0.0, 0.0, v)
        mean += w[t] * m
        var += w[t] * v
        term_m = np.maximum(term_m, np.abs(w[t] * m))
        term_v = np.maximum(term_v, w[t] * (np.abs(s[t, :, 1]) / c[t] + m * m))
    out = np.empty_like(s)
    bound = np.empty_like(s)
    for t in range(T):
        out[t, :, 0] = mean * c[t]
        out[t, :, 1] = (var + mean * mean) * c[t]
        bound[t, :, 0] = 4 * 2.0 ** -53 * (np.abs(out[t, :, 0]) + T * term_m * c[t])
        bound[t, :, 1] = 4 * 2.0 ** -53 * (np.abs(out[t, :, 1]) + T * (term_v + mean * mean) * c[t])
    return out, bound


def gn_pool_stats(sums, weights, counts):
    """The statement the kernel implements, written the other way round: pooled mean = sum_t w_t mean_t and pooled (biased)
    variance = sum_t w_t var_t per (image, group).  Returns (mean [BG], var [BG])."""
    s = np.asarray(sums, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)[:, None]
    c = np.asarray(counts, dtype=np.float32).astype(np.float64)[:, None]
    m = s[..., 0] / c
    v = np.maximum(s[..., 1] / c - m * m, 0.0)
    return (w * m).sum(0), (w * v).sum(0)


def tile_sums(tiles):
    """[T][BG, n_t] data -> ([T, BG, 2] float64 (sum, sum of squares), n_t list)."""
    out = np.stack([np.stack([np.asarray(t, dtype=np.float64).sum(1), (np.asarray(t, dtype=np.float64) ** 2).sum(1)], axis=-1) for t in tiles])
    return out, [t.shape[1] for t in tiles]


# ---- wavelet level: 3x3 binomial kernel, dilation r, replicate padding, by an index-clamp gather --------------------------------------
def wavelet_level_ref(x, r, defect=None):
    """x [planes, H, W] -> (low, abs_low) in float64: low = sum_k w_k x[clamp(y + dy_k r), clamp(x + dx_k r)], abs_low the same on
    |x|.  defect "zero_bottom": rows past the bottom border read zero instead of the last row."""
    x = np.asarray(x, dtype=np.float64)
    _, H, W = x.shape
    ys, xs = np.arange(H), np.arange(W)
    yi = {-1: np.clip(ys - r, 0, H - 1), 0: ys, 1: np.clip(ys + r, 0, H - 1)}
    xi = {-1: np.clip(xs - r, 0, W - 1), 0: xs, 1: np.clip(xs + r, 0, W - 1)}
    inside = (ys + r <= H - 1).astype(np.float64)[None, :, None]
    low, alow = np.zeros_like(x), np.zeros_like(x)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            wgt = (2.0 - abs(dy)) * (2.0 - abs(dx)) / 16.0          # [1 2 1] x [1 2 1] / 16
            g = x[:, yi[dy]][:, :, xi[dx]]
            if defect == "zero_bottom" and dy == 1:
                g = g * inside
            low += wgt * g
            alow += wgt * np.abs(g)
    return low, alow


def wavelet_chain_ref(x, levels=5):
    """The decomposition of edtr_amd.wavelet chained in float64: radii 1, 2, 4, ...; returns (high = x - low_n, low_n, A_n, sum_i A_i)
    with A_i the chain on |x| (the bound's absref: a level's error, blurred by the later levels, is bounded by k 2^-22 A_n)."""
    cur, acur = np.asarray(x, dtype=np.float64), np.abs(np.asarray(x, dtype=np.float64))
    x0, a_sum = cur, np.zeros_like(cur)
    for i in range(levels):
        cur, _ = wavelet_level_ref(cur, 2 ** i)
        acur, _ = wavelet_level_ref(acur, 2 ** i)
        a_sum = a_sum + acur
    return x0 - cur, cur, acur, a_sum


# ---- sampler arithmetic ----------------------------------------------------------------------------------------------------------------
def q_sample_ref(x, noise, t, tab_a, tab_b, defect=None):
    """x / noise [B, ...], t [B] int64, tables [n_tab] float32 -> (ref, absref, fp32 result): a x + b n with t clamped to the
    table; the third result restates noise_elem.h q_sample_elem in float32 arithmetic (two rounded products, one rounded sum).
    defect "t_mod": an out-of-range t wraps (t mod n_tab) instead of clamping."""
    xn, nn = np.asarray(x, dtype=np.float32), np.asarray(noise, dtype=np.float32)
    ta, tb = np.asarray(tab_a, dtype=np.float32), np.asarray(tab_b, dtype=np.float32)
    ti = np.asarray(t, dtype=np.int64)
    ti = ti % len(ta) if defect == "t_mod" else np.clip(ti, 0, len(ta) - 1)
    shape = (-1,) + (1,) * (xn.ndim - 1)
    a, b = ta[ti].reshape(shape), tb[ti].reshape(shape)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ref = a64 * xn + b64 * nn
    absref = np.abs(a64 * xn) + np.abs(b64 * nn)
    p, q = (a * xn).astype(np.float32), (b * nn).astype(np.float32)
    return torch.from_numpy(ref), torch.from_numpy(absref), torch.from_numpy((p + q).astype(np.float32))


def f32(v):
    """A python float as the C ABI passes it (float argument), in double."""
    return float(np.float32(v))


def sampler_update_ref(x, eps, noise, coefs):
    """coefs: 5 scalars or five broadcastable tensors (c_recip, c_recipm1, coef1, coef2, sigma) already rounded to float32.
    Returns (p0, abs_p0, x_prev, abs_x_prev): p0 = c_recip x - c_recipm1 e; x_prev = coef1 p0 + coef2 x + sigma n."""
    x, e, n = f64(x), f64(eps), f64(noise)
    cr, cm, c1, c2, sg = (f64(c) for c in coefs)
    p0 = cr * x - cm * e
    a_p0 = (cr * x).abs() + (cm * e).abs()
    xp = c1 * p0 + c2 * x + sg * n
    a_xp = c1.abs() * a_p0 + (c2 * x).abs() + (sg * n).abs()
    return p0, a_p0, xp, a_xp


def gaussian_sample_ref(moments, noise, B, C, HW, scale):
    """moments [B HW, ld] NHWC rows (mean | logvar | ...), noise [B, C, HW] or None -> (ref, absref, exp term) as [B, C, HW]:
    (mean + exp(0.5 clamp(logvar, -30, 20)) n) scale; the third result is exp(.) |n| |scale|, what the device expf's error scales."""
    m = f64(moments)
    mean = m[:, :C].reshape(B, HW, C).permute(0, 2, 1)
    lv = m[:, C:2 * C].reshape(B, HW, C).permute(0, 2, 1).clamp(-30.0, 20.0)
    s = f32(scale)
    if noise is None:
        return mean * s, (mean * s).abs(), torch.zeros_like(mean)
    n = f64(noise)
    e = torch.exp(0.5 * lv)
    return (mean + e * n) * s, (mean.abs() + e * n.abs()) * abs(s), e * n.abs() * abs(s)


def second_trip_missing(ref, stale):
    """What a kernel whose grid-stride loop runs one trip only leaves behind: elements past the first 4096 x 256 keep `stale`."""
    got = f64(ref).clone().reshape(-1)
    got[GRID_SPAN:] = f64(stale).reshape(-1)[GRID_SPAN:] if torch.is_tensor(stale) else float(stale)
    return got.reshape(ref.shape)
