"""fp64 references of the 16-bit layout, elementwise and normalisation kernels (csrc/elementwise.hip: nchw_to_nhwc, nhwc_to_nchw, add,
add_stats, split3 / split_operand, timestep_embedding, embed_tokens, zero_bytes; csrc/norm.hip: softmax_rows, layernorm, gn_stats +
gn_apply), shared by tests/test_gpu_glue16.py (which compares the HIP kernels with them) and tests/test_glue16_bound.py (which shows on
the CPU that the bounds and bit comparisons reject the defects such kernels typically have).  Plain torch on the exact values the
kernels read; nothing here calls the library.  The `*_emulated` functions restate a kernel in fp32 torch and take a ``defect`` that
makes them compute what a broken kernel would; the GPU tests never call them."""
import math

import torch
import torch.nn.functional as F

from edtr_amd.testing import LIPSCHITZ
from glue_reference import GRID_SPAN, f32, f64, second_trip_missing

ZERO_SPAN = 1024 * 256          # 16-byte units one trip of zero_kernel covers (edtr_zero_bytes: <= 1024 blocks of 256)
FP32_MIN_NORMAL = 2.0 ** -126   # below this an fp32 intermediate (and a bf16 output) is subnormal or zero


# ---- normalisation: the bound tests/test_gpu_ops.py norm_elem states ------------------------------------------------------------------
def norm_ref(x, gamma, beta, eps, silu=False):
    """(ref, absref) of a normalisation of x's LAST axis (reshape groups there): ref = (x - mean) rstd gamma + beta (+ SiLU) in fp64.
    The fp32 statistics add, per the reduction of k = x.shape[-1] terms, |dmean| rstd + |x - mean| rstd |drstd / rstd| <=
    k 2^-24 rstd (E|x| + |x - mean| rstd^2 E[x^2]) (times |gamma|): absref is that expression, for elem(..., k = x.shape[-1])."""
    xd, g, b = f64(x), f64(gamma), f64(beta)
    mu = xd.mean(-1, keepdim=True)
    rstd = 1.0 / (xd.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    ref = (xd - mu) * rstd * g + b
    absref = g.abs() * rstd * (xd.abs().mean(-1, keepdim=True) + (xd - mu).abs() * rstd ** 2 * (xd * xd).mean(-1, keepdim=True)) + b.abs()
    if silu:
        ref, absref = F.silu(ref), LIPSCHITZ["silu"] * absref
    return ref, absref


def gn_groups(t, B, HW, C, groups=32):
    """NHWC [B HW, C] (or [B, HW, C]) -> [B, groups, HW x channels per group]: a group's elements on the last axis."""
    cpg = C // groups
    return t.reshape(B, HW, groups, cpg).permute(0, 2, 1, 3).reshape(B, groups, HW * cpg)


def gn_affine(v, HW, C, groups=32):
    """Per-channel vector [C] -> [groups, HW x cpg] in gn_groups' order."""
    cpg = C // groups
    return v.reshape(groups, 1, cpg).expand(groups, HW, cpg).reshape(groups, HW * cpg)


def gn_sums_ref(x, B, HW, C, groups=32):
    """fp64 (sum, sum of squares) per (image, group) and the same on absolute values: [B, groups, 2] each."""
    g = f64(gn_groups(x, B, HW, C, groups))
    s = torch.stack([g.sum(-1), (g * g).sum(-1)], dim=-1)
    a = torch.stack([g.abs().sum(-1), (g * g).sum(-1)], dim=-1)
    return s, a


def layernorm_emulated(x, gamma, beta, eps, dtype, stale=float("nan"), defect=None):
    """layernorm_kernel in fp32 torch: two passes over the row held in registers.  defect "drop_slot3": the fourth vector slot
    (columns >= 1536) is neither summed nor written; "slot3_not_summed": it is written but missing from both sums."""
    x32 = x.float()
    C = x32.shape[-1]
    live = torch.ones(C, dtype=torch.bool)
    if defect in ("drop_slot3", "slot3_not_summed"):
        live[1536:] = False
    n = float(C)
    mean = (x32 * live).sum(-1, keepdim=True) / n
    d = x32 - mean
    rstd = torch.rsqrt((d * d * live).sum(-1, keepdim=True) / n + eps)
    y = (d * rstd * gamma.float() + beta.float()).to(dtype)
    if defect == "drop_slot3":
        y[..., 1536:] = stale
    return y


def gn_emulated(x, gamma, beta, eps, silu, dtype, B, HW, C, groups=32, ppb=8, defect=None, ld_stat=None):
    """gn_stats + gn_apply in torch: fp32 sums per (image, group), fp64 mean / variance, one fp32 rsqrt, y = x sc + sh (+ SiLU).
    x [B HW, C] 16-bit.  defect "swap": in the generic apply loop (a channel chunk whose vector count is no power of two) a
    workgroup's flat index is split as (vector, pixel) instead of (pixel, vector).  ld_stat = (wide [B HW, ld], col0): the
    statistics run over ALL ld columns of the buffer x is a slice of ("pad columns included in a statistic")."""
    cpg = C // groups
    x32 = x.float().reshape(B, HW, C)
    if ld_stat is None:
        g = gn_groups(x32, B, HW, C, groups)
        s, q, cnt = g.sum(-1).double(), (g * g).sum(-1).double(), float(HW * cpg)
    else:
        wide, col0 = ld_stat
        w = wide.float().reshape(B, HW, -1)
        per = w.shape[-1] // groups                      # the misreading kernel folds ld / groups columns into a group
        g = w[..., :per * groups].reshape(B, HW, groups, per).permute(0, 2, 1, 3).reshape(B, groups, -1)
        s, q, cnt = g.sum(-1).double(), (g * g).sum(-1).double(), float(HW * per)
    mean = s / cnt
    var = (q / cnt - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var.float() + eps)                                    # [B, groups]
    sc = gamma.float().reshape(1, groups, cpg) * rstd[..., None]
    sh = beta.float().reshape(1, groups, cpg) - mean.float()[..., None] * sc
    y = x32 * sc.reshape(B, 1, C) + sh.reshape(B, 1, C)
    if silu:
        y = F.silu(y)
    y = y.to(dtype)
    if defect == "swap":
        for c0 in range(0, C, 256):
            cc = min(256, C - c0)
            ncv = cc // 8
            if ncv & (ncv - 1) == 0:
                continue
            for p0 in range(0, HW, ppb):
                npix = min(ppb, HW - p0)
                slab = y[:, p0:p0 + npix, c0:c0 + cc].reshape(B, npix, ncv, 8).clone()
                # element i = pi ncv + cv receives what was computed for (pixel i % npix, vector i // npix)
                y[:, p0:p0 + npix, c0:c0 + cc] = slab.transpose(1, 2).reshape(B, npix, ncv, 8).reshape(B, npix, cc)
    return y.reshape(B * HW, C)


# ---- row softmax -----------------------------------------------------------------------------------------------------------------------
def softmax_ref(s):
    """s [rows, cols] (the live columns only) -> (ref, extra): softmax in fp64 and the named terms beside elem(p, ref, ref, dtype,
    cols).  "fast exponential": the kernel's __expf(v - max) is exp2 of the fp32 product (v - max) log2e, whose rounding of
    2^-24 |v - max| log2e moves the result by 2^-24 |v - max| relative; the online pass applies up to three such factors to the
    row sum and the last pass one to the element: 4 2^-24 |v - max| ref.  "fp32 underflow": a probability below the smallest
    normal fp32 number cannot be formed in fp32 (nor stored in bf16): it may come out as zero."""
    sd = f64(s)
    ref = torch.softmax(sd, dim=-1)
    return ref, {"fast exponential": 2.0 ** -22 * (sd - sd.amax(-1, keepdim=True)).abs() * ref, "fp32 underflow": FP32_MIN_NORMAL}


def softmax_emulated(s, cols, dtype, cols_pad=0, stale=float("nan"), defect=None):
    """softmax_rows_kernel in fp32 torch with its thread structure: vector v of four columns belongs to thread v % 256, a thread
    keeps (max, sum) of its own columns, the threads' pairs are merged with exp(m_t - max).  s [rows, ld_s]; returns
    [rows, max(cols, cols_pad)].  defects: "no_rescale" merges the sums without the factor; "pad_unzeroed" leaves columns
    [cols, cols_pad) at `stale`; "pad_in_sum" runs over all ld_s columns of s."""
    rows = s.shape[0]
    live = s.shape[1] if defect == "pad_in_sum" else cols
    v = s[:, :live].float()
    padded = F.pad(v, (0, -live % 1024), value=float("-inf")).reshape(rows, -1, 256, 4)
    m_t = padded.amax((1, 3)).clamp_min(-1e30)                               # [rows, 256]; a thread without columns keeps -1e30
    l_t = torch.exp(padded - m_t[:, None, :, None]).sum((1, 3))
    gm = m_t.amax(-1, keepdim=True)
    gl = (l_t if defect == "no_rescale" else l_t * torch.exp(m_t - gm)).sum(-1, keepdim=True)
    p = (torch.exp(v - gm) * (1.0 / gl)).to(dtype)[:, :cols]
    out = torch.full((rows, max(cols, cols_pad)), stale, dtype=dtype)
    out[:, :cols] = p
    if defect != "pad_unzeroed":
        out[:, cols:] = 0.0
    return out


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc_ref(src, scale, shift):
    """src [B, C, HW] fp32 -> (ref, absref) [B, HW, C]: src scale + shift with the float32 scale / shift the C ABI passes."""
    xd = f64(src).permute(0, 2, 1)
    return xd * f32(scale) + f32(shift), (xd * f32(scale)).abs() + abs(f32(shift))


def nchw_to_nhwc_emulated(src, scale, shift, dtype, cpad, stale, defect=None):
    """nchw_to_nhwc_kernel in fp32 torch -> the [B, HW, cpad] window it writes (columns >= C zero).  defects: "one_pass": only the
    first 64 channels are moved (the c0 loop runs once); "pad_unzeroed": columns [C, cpad) keep `stale`."""
    B, C, HW = src.shape
    v = (src.float() * torch.tensor(scale, dtype=torch.float32) + torch.tensor(shift, dtype=torch.float32)).permute(0, 2, 1).to(dtype)
    out = torch.full((B, HW, cpad), stale, dtype=dtype)
    out[..., :C] = v
    if defect != "pad_unzeroed":
        out[..., C:] = 0.0
    if defect == "one_pass":
        out[..., 64:] = stale
    return out


def nhwc_to_nchw_exact(src, C, scale):
    """src [B, HW, ld] (16-bit or fp32) -> fp32 [B, C, HW]: the first C columns times the float32 scale, rounded once."""
    return (src[..., :C].float() * torch.tensor(scale, dtype=torch.float32)).permute(0, 2, 1).contiguous()


# ---- elementwise -----------------------------------------------------------------------------------------------------------------------
def add16_exact(a, b, dtype):
    """a (+ b) as add_kernel forms it: one fp32 addition of the two 16-bit values, rounded once (b None: a copy)."""
    return a.clone() if b is None else (a.float() + b.float()).to(dtype)


def add_stats_ref(a, b, slot_rows, defect=None):
    """Per-slot column statistics of the fp32 value a + b (what add_stats_kernel accumulates: the sum before it is rounded to 16
    bits) -> (sums, abs) [slots, C, 2] fp64: (sum, sum of squares) and (sum of |v|, sum of squares).  defect "next_slot": slot s
    holds slot s + 1's sums (the last one its own)."""
    v = f64(a.float() if b is None else a.float() + b.float())
    rows, C = v.shape
    v = v.reshape(rows // slot_rows, slot_rows, C)
    sums = torch.stack([v.sum(1), (v * v).sum(1)], dim=-1)
    absr = torch.stack([v.abs().sum(1), (v * v).sum(1)], dim=-1)
    if defect == "next_slot":
        sums = torch.cat([sums[1:], sums[-1:]])
    return sums, absr


def add_stats_emulated(a, b, slot_rows):
    """add_stats_kernel's partials in fp32 torch: [slots, C, 2] float32."""
    v = a.float() if b is None else a.float() + b.float()
    rows, C = v.shape
    v = v.reshape(rows // slot_rows, slot_rows, C)
    return torch.stack([v.sum(1), (v * v).sum(1)], dim=-1)


def parts_exact(x, dtype, order):
    """Split operand of x [rows, C] (fp32 or 16-bit): hi = x rounded to dtype, lo = (x - hi) rounded to dtype (the difference is
    exact in fp32), concatenated in `order`, a string of "h" / "l" ("hlh": split-3 pattern 0, "hhl": pattern 1, "h", "hl")."""
    xf = x.float()
    hi = xf.to(dtype)
    lo = (xf - hi.float()).to(dtype)
    return torch.cat([hi if c == "h" else lo for c in order], dim=1)


def temb_ref(t, dim):
    """t [B] int64 -> (ref [B, dim], argument error [B, dim]): cos | sin in fp64 of the fp32 arguments t exp(-ln(10000) i / half)
    formed as the kernel forms them.  The device's expf and this torch.exp may differ by 2 ulp each in the frequency, and the
    device cosf / sinf carry a few ulp of their own: 8 2^-24 |arg| absolute (the bound tests/test_gpu_ops.py states)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    ad = (t[:, None].float() * freqs[None]).double()
    return torch.cat([torch.cos(ad), torch.sin(ad)], dim=-1), 8 * 2.0 ** -24 * torch.cat([ad, ad], dim=-1).abs()


def temb_emulated(t, dim, dtype, stale=float("nan"), defect=None):
    """temb_kernel in fp32 torch.  defect "one_trip": the 256 threads handle index i = thread only (i >= 256 keeps `stale`)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    c, s = torch.cos(args).to(dtype), torch.sin(args).to(dtype)
    if defect == "one_trip":
        c[:, 256:] = stale
        s[:, 256:] = stale
    return torch.cat([c, s], dim=-1)


def embed_tokens_exact(tokens, table, pos, dtype):
    """tokens [rows] int64, table [vocab, D], pos [L, D] fp32 -> (table[clamp(token)] + pos[row % L]) rounded once: [rows, D]."""
    rows, L = tokens.numel(), pos.shape[0]
    return (table[tokens.reshape(-1).clamp(0, table.shape[0] - 1)] + pos[torch.arange(rows) % L]).to(dtype)


# ---- the grid-stride loop's second trip, in units of what one thread moves per iteration -----------------------------------------------
def second_trip_missing_units(ref, stale, unit, span=GRID_SPAN):
    """`ref` is written in units of `unit` consecutive elements (an 8-wide vector, a 16-byte chunk): a loop that runs one trip only
    leaves the units past `span` at `stale`.  Returns fp64 of ref's shape (glue_reference.second_trip_missing per unit lane)."""
    flat = f64(ref).reshape(-1, unit)
    if span == GRID_SPAN:
        cols = [second_trip_missing(flat[:, j], stale if not torch.is_tensor(stale) else f64(stale).reshape(-1, unit)[:, j]) for j in range(unit)]
        return torch.stack(cols, dim=1).reshape(ref.shape)
    got = flat.clone()
    got[span:] = f64(stale).reshape(-1, unit)[span:] if torch.is_tensor(stale) else float(stale)
    return got.reshape(ref.shape)
