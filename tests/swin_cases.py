"""References, operand builders and case tables of the six MFMA kernels of csrc/swin.hip (edtr_window_attn, edtr_swin_mlp,
edtr_swin_attn, edtr_swin_layer, edtr_conv64, edtr_conv128_out), importable without a GPU.  tests/test_gpu_ops.py (the friendly
layout) and tests/test_gpu_swin_edges.py (guarded buffers, hostile strides, the smallest shape that reaches each branch) share one
statement of each operation from here; tests/test_swin_edges_cpu.py applies defects to these references (the `defect` arguments
below) and shows which checks reject them.  Every reference is a function of the operands: the 16-bit values the kernel reads."""
import math

import torch
import torch.nn.functional as F

from edtr_amd.testing import ACC_F32, GELU_APPROX, LIPSCHITZ, rounded_operand, unit_roundoff

DTYPES = [torch.bfloat16, torch.float16]
F32 = torch.float32
NAN = float("nan")
PAD = 64                        # guard elements in front of and behind every destination
PATTERN = 0x5A3C                # bit pattern of a pre-filled 16-bit destination (a finite value in both formats)
SENTINEL = 12345.678            # pre-filled fp32 destinations
CP, HP, HEADS = 192, 384, 6     # the padded token / hidden width and the head count edtr_swin_mlp / edtr_swin_attn are built for
LD_OUT, LD_OUT64 = 200, 80      # destination row strides: 192 / 64 written columns + 8 guard columns
LD_X, LD_X64, LD_X128 = 208, 72, 136     # source row strides (never the destination's); the columns behind the real width hold NaN


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# =====================================================================================================================================
# guarded destinations (the conventions of tests/test_gpu_glue16.py, on the host so that the CPU file can use them)
# =====================================================================================================================================
def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def filled(n, dtype, fill):
    """Host tensor of n elements: NaN (fill "nan": around pure stores) or a finite pattern (fill "pattern")."""
    if fill == "nan":
        return torch.full((n,), NAN, dtype=dtype)
    if dtype in DTYPES:
        return torch.full((n,), PATTERN, dtype=torch.int16).view(dtype)
    return torch.full((n,), SENTINEL, dtype=dtype)


def window(rows, ld, dtype, d, fill, extra_rows=2):
    """A [rows + extra_rows, ld] view PAD elements inside a flat pre-filled buffer on device d.  Returns (buffer, view, host copy
    before)."""
    n = (rows + extra_rows) * ld
    host = filled(n + 2 * PAD, dtype, fill)
    buf = host.to(d) if d is not None else host.clone()
    return buf, buf[PAD:PAD + n].view(rows + extra_rows, ld), host


def untouched(buf, before, written):
    """Everything of `buf` outside the written region equals `before` bit for bit.  `written`: bool mask over the view's elements."""
    a, b = bits(buf), bits(before)
    mask = torch.ones(a.shape, dtype=torch.bool)
    mask[PAD:PAD + written.numel()] = ~written.reshape(-1)
    assert torch.equal(a[mask], b[mask]), f"{int((a[mask] != b[mask]).sum())} elements outside the written region changed"


def region(view, rows, c0, c1):
    m = torch.zeros(view.shape, dtype=torch.bool)
    m[:rows, c0:c1] = True
    return m


def in_nan_columns(x, ld, d=None):
    """x [rows, C] as the first C columns of a [rows, ld] buffer (on device d) whose other columns hold NaN."""
    host = torch.full((x.shape[0], ld), NAN, dtype=x.dtype)
    host[:, :x.shape[1]] = x
    return (host.to(d) if d is not None else host)[:, :x.shape[1]]


# =====================================================================================================================================
# persistent-loop geometry of edtr_conv64 / edtr_conv128_out (one workgroup per CU, patch += workgroups)
# =====================================================================================================================================
PERSISTENT_B = 3


def persistent_edge(cus, rounds):
    """The smallest square H = W, a multiple of 16, whose PERSISTENT_B (H / 16)^2 patches exceed (rounds - 1) cus and are no multiple of
    cus: `rounds` trips of the persistent loop with a ragged last one.  256 CUs: 160 (300 patches) and 224 (588 patches)."""
    n = 1
    while PERSISTENT_B * n * n <= (rounds - 1) * cus or (PERSISTENT_B * n * n) % cus == 0:
        n += 1
    return 16 * n


def check_persistent(B, H, W, cus, rounds):
    """What a case asserts before it launches: a changed CU count fails the case instead of quietly testing fewer rounds."""
    patches = B * (H // 16) * (W // 16)
    assert patches > (rounds - 1) * cus and patches % cus, f"{patches} patches on {cus} CUs do not give {rounds} ragged rounds"
    return patches


def workgroup_images(B, H, W, cus):
    """Per workgroup of the persistent launch: the images of the patches it walks through, in order."""
    per = (H // 16) * (W // 16)
    grid = min(B * per, cus)
    return [[p // per for p in range(g, B * per, grid)] for g in range(grid)]


# =====================================================================================================================================
# shared fp64 pieces
# =====================================================================================================================================
def conv_ref(x, w, bias=None, **kw):
    """fp64 conv2d and conv2d(|x|, |w|) + |bias| (NCHW)."""
    xd, wd = x.double().cpu(), w.double().cpu()
    b = None if bias is None else bias.double().cpu()
    return F.conv2d(xd, wd, b, **kw), F.conv2d(xd.abs(), wd.abs(), None if b is None else b.abs(), **kw)


def gn_apply16(x, scale, shift, dtype, silu=True):
    """x * scale + shift (+ SiLU) from an exact fp32 (scale, shift) table, rounded to 16 bits as edtr_gn_apply stores it (the fused
    forms round it the same way before their product): fp64 mirror and flip spacing for the fp32 fma (2^-23 (|x scale| + |shift|))
    and SiLU's exp2 / rcp (2^-22 |silu|)."""
    xd, sc, sh = x.double().cpu(), scale.double().cpu(), shift.double().cpu()
    y = xd * sc + sh
    dv = 2.0 ** -23 * ((xd * sc).abs() + sh.abs())
    if silu:
        y = F.silu(y)
        dv = LIPSCHITZ["silu"] * dv + 2.0 ** -22 * y.abs()
    return rounded_operand(y, dv, dtype)


# =====================================================================================================================================
# edtr_window_attn
# =====================================================================================================================================
def thin_band_merged(labels, H, W, shift):
    """DEFECT: the region labels with a band that is one pixel wide merged into its neighbour (shift 1: the last band; shift 7: the
    middle one) — the mask dropped for a one-pixel region.  Other shifts have no such band: the labels come back unchanged."""
    by, bx = labels // 3, labels % 3
    if shift == 1:
        by, bx = by.clip(max=1), bx.clip(max=1)
    elif shift == 7:
        by, bx = by + (by == 1), bx + (bx == 1)
    return (by * 3 + bx).astype(labels.dtype)


def window_attn_reference(qkv, table_bias, H, W, heads, d, shift, defect=None):
    """plain torch restatement of model/swinir.py:254-279 + :120-148 without the two linears, in qkv's precision: qkv [B, H, W, 3,
    heads, d].  defect "shift_x_only": the cyclic shift applied along x alone; "thin_mask": thin_band_merged."""
    from edtr_amd.model import swinir as S
    B = qkv.shape[0]
    C = heads * d
    h = qkv.reshape(B, H, W, 3 * C)
    sy = 0 if defect == "shift_x_only" else shift
    if shift:
        h = torch.roll(h, (-sy, -shift), (1, 2))
    win = h.reshape(B, H // 8, 8, W // 8, 8, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, 3, heads, d)
    q, k, v = win.permute(2, 0, 3, 1, 4)
    att = (q * d ** -0.5) @ k.transpose(-1, -2) + table_bias
    if shift:
        if defect == "thin_mask":
            import numpy as np
            lab = thin_band_merged(S.region_labels(H, W, 8, shift), H, W, shift).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
            m = torch.from_numpy(np.where(lab[:, None, :] != lab[:, :, None], -100.0, 0.0).astype(np.float32))
        else:
            m = torch.from_numpy(S.shift_mask(H, W, 8, shift))
        att = (att.reshape(B, -1, heads, 64, 64) + m[None, :, None]).reshape(-1, heads, 64, 64)
    o = (torch.softmax(att, -1) @ v).transpose(1, 2).reshape(B, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    return torch.roll(o, (sy, shift), (1, 2)) if shift else o


def window_logits(qkv, H, W, heads, d, shift):
    """d^-1/2 q k^T of every window before bias and mask, fp64 [windows, heads, 64, 64] (what WINDOW_SHARP_Q is chosen by)."""
    B = qkv.shape[0]
    h = torch.roll(qkv.double().reshape(B, H, W, -1), (-shift, -shift), (1, 2))
    win = h.reshape(B, H // 8, 8, W // 8, 8, -1).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, 3, heads, d)
    q, k, _ = win.permute(2, 0, 3, 1, 4)
    return (q * d ** -0.5) @ k.transpose(-1, -2)


def window_elem(qkv, bias, H, W, heads, d, shift, scale, dtype, defect=None):
    """(ref, absref, k, extra) of the windowed attention's element bound (attn_elem's terms; window_attn_reference in fp64 gives
    P V, and with |V| in place of V gives P|V|).  The logit term uses each query's bound delta_i = d 2^-22 scale |q_i|_1 max|k| for
    all its keys, which moves the output by at most 2 delta_i P|V|.  All as [B H W, heads d]."""
    q64 = qkv.double()
    ref = window_attn_reference(q64, bias.double(), H, W, heads, d, shift, defect)
    vabs = q64.clone()
    vabs[..., 2, :, :] = vabs[..., 2, :, :].abs()
    pv = window_attn_reference(vabs, bias.double(), H, W, heads, d, shift, defect)
    C = heads * d
    qn = q64[..., 0, :, :].abs().sum(-1, keepdim=True)                                 # [B, H, W, heads, 1]
    delta = d * 2.0 ** -22 * scale * qn * float(q64[..., 1, :, :].abs().max())
    delta = delta.expand(*qn.shape[:-1], d).reshape(*ref.shape)
    rows = ref.numel() // C
    extra = {"16-bit P before P V": 2.0 * unit_roundoff(dtype) * pv.reshape(rows, C), "fp32 logits": (2.0 * delta * pv).reshape(rows, C)}
    return ref.reshape(rows, C), pv.reshape(rows, C), 64, extra


def window_qkv(B, H, W, heads, d, dtype, q_scale=1.0, seed=170):
    """(qkv [B, H, W, 3, heads, d] 16-bit, bias fp32 [heads, 64, 64]) in the distribution of test_window_attention; q_scale sharpens
    the logits (WINDOW_SHARP_Q)."""
    from edtr_amd.model import swinir as S
    qkv = rnd((B, H, W, 3, heads, d), seed) * 1.5
    qkv[..., 0, :, :] *= q_scale
    return qkv.to(dtype), S.expand_bias(rnd((225, heads), seed + 1, 0.7), 8)


def pack_window_qkv(qkv):
    """[B, H, W, 3, heads, d] -> the kernel's [B H W, 3 heads 32] rows, head channels d .. 31 zero."""
    B, H, W, _, heads, d = qkv.shape
    packed = torch.zeros((B * H * W, 3, heads, 32), dtype=qkv.dtype)
    packed[..., :d] = qkv.reshape(B * H * W, 3, heads, d)
    return packed.reshape(B * H * W, -1)


# q ~ 1.5 x 7 N(0, 1), k ~ 1.5 N(0, 1): a logit d^-1/2 q . k has standard deviation 1.5^2 x 7 = 15.75 at d = 30, so the largest of the
# 64 x 64 x heads x windows of case (c) reaches about +-60 (3.8 sigma); |q| stays below 1.5 x 7 x 6 = 63, far inside fp16.
WINDOW_SHARP_Q = 7.0
WINDOW_CASES = {         # name: (B, H, W, heads, d, c_pad, shift, q_scale)
    "thin_shift1": (1, 24, 8, 6, 30, 192, 1, 1.0),           # 18 tasks: the last workgroup has two waves; one window column
    "thin_shift7": (1, 24, 8, 6, 30, 192, 7, 1.0),
    "narrow_heads": (2, 16, 16, 2, 6, 16, 4, 1.0),           # one register group stores, half of it; the pad zeroing starts at column 12
    "sharp_logits": (1, 24, 8, 6, 30, 192, 7, WINDOW_SHARP_Q),
}


# =====================================================================================================================================
# edtr_swin_mlp
# =====================================================================================================================================
def mlp_operands(dtype, C=180, HID=360, seed=190):
    """fc1 / fc2 / LayerNorm parameters in the distribution of test_swin_mlp_one_launch, padded and folded as model/swinir.py does it:
    w1g = gamma . W1 [384, 192], w2p [192, 384], c1 (row sums of the 16-bit w1g), c2b = W1 beta + b1, b2p."""
    gamma, beta = 1 + 0.2 * rnd((C,), seed + 1), 0.3 * rnd((C,), seed + 2)
    w1, b1 = rnd((HID, C), seed + 3, 1 / math.sqrt(C)), 0.2 * rnd((HID,), seed + 4)
    w2, b2 = rnd((C, HID), seed + 5, 1 / math.sqrt(HID)), 0.2 * rnd((C,), seed + 6)
    w1g, w2p, c2b, b2p = torch.zeros((HP, CP)), torch.zeros((CP, HP)), torch.zeros(HP), torch.zeros(CP)
    w1g[:HID, :C] = w1 * gamma[None, :]
    w2p[:C, :HID] = w2
    c2b[:HID] = w1 @ beta + b1
    b2p[:C] = b2
    return dict(C=C, HID=HID, gamma=gamma, beta=beta, w1=w1, b1=b1, w2=w2, b2=b2, w1g=w1g, w2p=w2p, c2b=c2b, b2p=b2p,
                c1=w1g.to(dtype).float().sum(1).contiguous())


def mlp_rows(rows, C, dtype, seed=190, kind="plain"):
    """x [rows, 192] 16-bit, pad columns zero.  "plain": test_swin_mlp_one_launch's rows.  "extreme": the odd rows have |mean| = 16
    std (mean +-4, std 0.25) and row 5 is all zeros."""
    x = torch.zeros((rows, CP))
    x[:, :C] = rnd((rows, C), seed, 1.5) + 0.4
    if kind == "extreme":
        sign = torch.where(torch.arange(rows) % 4 == 1, 1.0, -1.0)[:, None]
        z = rnd((rows, C), seed + 50)
        z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
        x[1::2, :C] = (4.0 * sign + 0.25 * z)[1::2]
        x[5] = 0.0
    return x.to(dtype)


def mlp_reference(x16, P):
    """torch fp32 on the 16-bit rows: x + fc2(GELU(fc1(LayerNorm(x)))), [rows, C]."""
    C = P["C"]
    xf = x16.float()[:, :C]
    h = F.gelu(F.layer_norm(xf, (C,), P["gamma"], P["beta"], 1e-5) @ P["w1"].t() + P["b1"])
    return xf + h @ P["w2"].t() + P["b2"]


def mlp_mirror(x16, P, dtype, wide_stats_row=None):
    """(ref, absref, k, extra) [rows, C] of a reference that mirrors the kernel: LayerNorm folded into the first product over the RAW
    rows (swin.hip:306-324, one-pass statistics: pre = rstd (acc - mean c1) + c2b), GELU, the hidden units packed to 16 bits
    (swin.hip:390), the second product over the 16-bit W2, + b2 + x, one rounding.  Hidden values whose fp32 error bound reaches a
    16-bit rounding boundary may land one spacing away (rounded_operand), propagated through |W2|.  The cen rstd^2 E[x^2] term of that
    bound is the one-pass variance's cancellation: it grows with (mean / std)^2.  DEFECT wide_stats_row: that row's statistics taken
    over all 192 columns instead of c_valid."""
    C = P["C"]
    W1, W2 = P["w1g"].to(dtype).double(), P["w2p"].to(dtype).double()
    xd = x16.double()
    n = torch.full((xd.shape[0], 1), float(C), dtype=torch.float64)
    if wide_stats_row is not None:
        n[wide_stats_row] = float(CP)
    mu = xd[:, :C].sum(1, keepdim=True) / n
    ex2 = (xd[:, :C] ** 2).sum(1, keepdim=True) / n
    rstd = 1.0 / ((ex2 - mu * mu).clamp_min(0) + 1e-5).sqrt()
    c1, c2b, b2p = P["c1"].double(), P["c2b"].double(), P["b2p"].double()
    cen = xd @ W1.t() - mu * c1
    pre = rstd * cen + c2b
    epre = C * ACC_F32 * (rstd * (xd.abs() @ W1.abs().t() + mu.abs() * c1.abs() + cen.abs() * rstd ** 2 * ex2) + c2b.abs())
    g16, flip = rounded_operand(F.gelu(pre), LIPSCHITZ["gelu"] * epre + GELU_APPROX * pre.abs(), dtype)
    ref64 = xd + g16 @ W2.t() + b2p
    abs64 = xd.abs() + g16.abs() @ W2.abs().t() + b2p.abs()
    return ref64[:, :C], abs64[:, :C], HP, {"16-bit hidden units, boundary values": (flip @ W2.abs().t())[:, :C]}


ROW_STATS_K = 96                # terms per slot: columns 0 .. 95 and 96 .. 191


def row_stats_ratio(stats, stored):
    """The documented row_stats layout (include/edtr_hip.h) against the STORED 16-bit output rows [rows, 192]: slots 0 and 3 hold (sum,
    sum of squares) of columns 0 .. 95 / 96 .. 191 within 96 x 2^-24 of the sum of absolute terms (fp32 accumulation of 96 terms in any
    order), slots 1, 2, 4, 5 are exactly +0.  Returns (worst |error| / bound, whether the zero slots are +0 bit for bit)."""
    st = stats.detach().cpu().reshape(-1, CP // 32, 2)
    x = stored.double().cpu().reshape(st.shape[0], 2, ROW_STATS_K)
    got = st[:, [0, 3]].double()
    want = torch.stack([x.sum(-1), (x * x).sum(-1)], -1)
    bound = ROW_STATS_K * 2.0 ** -24 * torch.stack([x.abs().sum(-1), (x * x).sum(-1)], -1) + 1e-300
    err = (got - want).abs() / bound
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    zeros = bool((bits(st[:, [1, 2, 4, 5]]) == 0).all())
    return float(err.max()), zeros


MLP_CASES = {            # name: (rows, C, HID, kind)
    "one_row": (1, 180, 360, "plain"),                       # every load row clamps to row 0; one live lane per statistic
    "one_live_row_in_last_workgroup": (129, 180, 360, "plain"),
    "no_pad_columns": (128, 192, 384, "plain"),
    "extreme_rows": (128, 180, 360, "extreme"),
}


# =====================================================================================================================================
# edtr_swin_attn (and edtr_swin_layer on the same operands)
# =====================================================================================================================================
def attn_operands(dtype, C=180, seed=200):
    """LayerNorm / qkv / proj / relative-position parameters in the distribution of test_swin_attention_half_one_launch, packed
    exactly as model/swinir.py does it (head width d = C / 6 padded to 32; gamma and the q scale folded into wg, beta and the qkv bias
    into c2b)."""
    from edtr_amd.model import swinir as S
    heads, d = HEADS, C // HEADS
    gamma, beta = 1 + 0.2 * rnd((C,), seed + 1), 0.3 * rnd((C,), seed + 2)
    wqkv, bqkv = rnd((3 * C, C), seed + 3, 1.5 / math.sqrt(C)), 0.2 * rnd((3 * C,), seed + 4)
    wp, bp = rnd((C, C), seed + 5, 1 / math.sqrt(C)), 0.2 * rnd((C,), seed + 6)
    bias = S.expand_bias(rnd((225, heads), seed + 7, 0.7), 8)
    wq32, bq32 = S.pack_qkv(wqkv, bqkv, heads, CP)                  # [(s, h, e), CP] with zero pad rows / columns
    g_pad, b_pad = torch.zeros(CP), torch.zeros(CP)
    g_pad[:C], b_pad[:C] = gamma, beta
    scale = torch.ones(3 * heads * 32)
    scale[: heads * 32] = d ** -0.5
    wg = wq32 * g_pad[None, :] * scale[:, None]
    wpp = torch.zeros((CP, heads, 32))
    wpp[:C, :, :d] = wp.reshape(C, heads, d)
    bpp = torch.zeros(CP)
    bpp[:C] = bp
    return dict(C=C, d=d, gamma=gamma, beta=beta, wqkv=wqkv, bqkv=bqkv, wp=wp, bp=bp, bias=bias, wg=wg, wpp=wpp.reshape(CP, heads * 32),
                bpp=bpp, c1=wg.to(dtype).float().sum(1).contiguous(), c2b=(((wq32 @ b_pad) + bq32) * scale).contiguous())


def attn_rows(rows, C, dtype, seed=200):
    x = torch.zeros((rows, CP))
    x[:, :C] = rnd((rows, C), seed, 1.5) + 0.3
    return x.to(dtype)


def attn_reference(x16, P, B, H, W, shift):
    """torch fp32 on the 16-bit rows: x + proj(WindowAttention(LayerNorm(x))), [rows, C]."""
    C, d = P["C"], P["d"]
    xf = x16.float()[:, :C]
    qkv = F.layer_norm(xf, (C,), P["gamma"], P["beta"], 1e-5) @ P["wqkv"].t() + P["bqkv"]
    att = window_attn_reference(qkv.reshape(B, H, W, 3, HEADS, d), P["bias"], H, W, HEADS, d, shift).reshape(-1, C)
    return xf + att @ P["wp"].t() + P["bp"]


def attn_mirror(x16, P, B, H, W, shift, dtype, defect=None):
    """fp64 reference [rows, C] that mirrors the kernel's roundings: the 16-bit weights it reads (gamma and the q scale in wg, beta and
    the qkv bias in c2b, the padded proj), LayerNorm folded into the raw rows (swin.hip:643-658), q / k / v packed to 16 bits
    (swin.hip:665-705), O packed to 16 bits before proj (swin.hip:759-773).  The 16-bit P (swin.hip:754) is not mirrored: its
    rounding, like the flips of the other roundings, is what the per-block tolerance carries."""
    C, d = P["C"], P["d"]
    rows = x16.shape[0]
    xd = x16.double()
    mu = xd[:, :C].mean(1, keepdim=True)
    rstd = 1.0 / ((xd[:, :C] ** 2).mean(1, keepdim=True) - mu * mu + 1e-5).sqrt()
    q16 = (rstd * (xd @ P["wg"].to(dtype).double().t() - mu * P["c1"].double()) + P["c2b"].double()).to(dtype).double()
    q16 = q16.reshape(rows, 3, HEADS, 32)[..., :d].clone()
    q16[:, 0] /= d ** -0.5                                           # (window_attn_reference applies the scale itself)
    att16 = window_attn_reference(q16.reshape(B, H, W, 3, HEADS, d), P["bias"].double(), H, W, HEADS, d, shift, defect)
    att16 = att16.reshape(rows, C).to(dtype).double()
    wp16 = P["wpp"].to(dtype).double()[:C].reshape(C, HEADS, 32)[..., :d].reshape(C, C)
    return xd[:, :C] + att16 @ wp16.t() + P["bp"].double()


# Per-block tolerance (bf16, fp16) of the attention half against attn_mirror, shared by tests/test_gpu_ops.py (BLOCK_TOL["swin_attn"])
# and the edge cases, which keep that test's operand distribution: 1.5 x the worst 32 x 32 block measured on the MI355X.
BLOCK_TOL_SWIN_ATTN = (3.0e-3, 3.7e-4)

ATTN_CASES = {           # name: (B, H, W, shift, C)
    "shift1": (2, 8, 24, 1, 180),
    "shift7_one_window_per_image": (3, 8, 8, 7, 180),        # workgroup 0: windows of images 0 and 1; workgroup 1: one window; wrap on both axes
    "full_width_heads": (1, 8, 16, 4, 192),                  # head_dim 32, c_valid 192: no pad column anywhere
}


# =====================================================================================================================================
# edtr_conv64
# =====================================================================================================================================
def conv64_operands(B, SH, SW, cout, dtype, seed=210):
    """(x [B, SH, SW, 64] 16-bit, w fp32 [cout, 64, 3, 3], bias fp32 [64]) in the distribution of test_conv64_persistent."""
    x = rnd((B, SH, SW, 64), seed, 1.2).to(dtype)
    w = rnd((cout, 64, 3, 3), seed + 1, 1 / math.sqrt(576))
    bias = torch.zeros(64)
    bias[:cout] = 0.3 * rnd((cout,), seed + 2)
    return x, w, bias


def conv64_input(x16, ups, precision=torch.float64, source_image=None):
    """NCHW view of the convolution's input (behind the nearest-2x upsample).  DEFECT source_image: every image reads that one."""
    xin = x16.to(precision).permute(0, 3, 1, 2)
    if source_image is not None:
        xin = xin[source_image:source_image + 1].expand_as(xin)
    return F.interpolate(xin, scale_factor=2, mode="nearest") if ups else xin


def conv64_plain(x16, w, bias, dtype, alpha, slope, ups):
    """torch fp32: act(alpha conv(x, 16-bit w) + bias), NCHW [B, cout, H, W]; slope None = no activation."""
    cout = w.shape[0]
    ref = alpha * F.conv2d(conv64_input(x16, ups, torch.float32), w.to(dtype).float(), None, padding=1) + bias[:cout, None, None]
    return ref if slope is None else F.leaky_relu(ref, slope)


def conv64_reference(x16, w, bias, dtype, alpha, slope, ups, source_image=None):
    """(ref, absref) in fp64, NCHW [B, cout, H, W]; the element bound's k is 576."""
    cout = w.shape[0]
    r64, a64 = conv_ref(conv64_input(x16, ups, source_image=source_image), w.to(dtype).float(), None, padding=1)
    bd = bias[:cout, None, None].double()
    r64, a64 = alpha * r64 + bd, abs(alpha) * a64 + bd.abs()
    return (r64 if slope is None else F.leaky_relu(r64, slope)), a64


# =====================================================================================================================================
# edtr_conv128_out
# =====================================================================================================================================
def conv128_operands(B, HW, dtype, seed=240, per_image=False):
    """(x [B HW, 128] 16-bit, w fp32 [3 or 4, 128, 3, 3], bias fp32 [32], gamma, beta) in the distribution of
    test_conv128_out_one_launch.  per_image: image b is scaled by (1, 3, 0.3)[b % 3] and moved by (0, -1.3, -0.2)[b % 3], so that the
    images' GroupNorm tables differ by factors of 3 to 10 (4 output channels then)."""
    x = rnd((B * HW, 128), seed, 1.3) + 0.3
    cout = 3
    if per_image:
        cout = 4
        s = torch.tensor([1.0, 3.0, 0.3])[torch.arange(B) % 3].repeat_interleave(HW)[:, None]
        o = torch.tensor([0.0, -1.3, -0.2])[torch.arange(B) % 3].repeat_interleave(HW)[:, None]
        x = x * s + o
    w = rnd((cout, 128, 3, 3), seed + 1, 1 / math.sqrt(1152))
    bias = torch.zeros(32)
    bias[:cout] = 0.3 * rnd((cout,), seed + 2)
    return x.to(dtype), w, bias, 1 + 0.2 * rnd((128,), seed + 3), 0.2 * rnd((128,), seed + 4)


def gn_table_reference(x16, gamma, beta, eps, B):
    """The (scale, shift) table edtr_gn_table produces, from fp64 statistics of the 16-bit rows: fp32 [B, 128, 2] (32 groups of 4)."""
    xd = x16.double().reshape(B, -1, 32, 4)
    mu = xd.mean((1, 3))
    rstd = 1.0 / (xd.var((1, 3), unbiased=False) + eps).sqrt()
    scale = gamma.double().reshape(32, 4) * rstd[:, :, None]
    shift = beta.double().reshape(32, 4) - mu[:, :, None] * scale
    return torch.stack([scale.reshape(B, 128), shift.reshape(B, 128)], -1).float()


def conv128_plain(x16, w, bias, dtype, gamma, beta, alpha, B, H, W):
    """torch fp32: alpha conv(silu(group_norm(x)) rounded to 16 bits, 16-bit w) + bias (gamma None: no normalisation)."""
    xin = x16.float().reshape(B, H, W, 128).permute(0, 3, 1, 2)
    if gamma is not None:
        xin = F.silu(F.group_norm(xin, 32, gamma, beta, 1e-6)).to(dtype).float()      # (the kernel rounds the normalised operand to 16 bits)
    return alpha * F.conv2d(xin, w.to(dtype).float(), None, padding=1) + bias[:w.shape[0], None, None]


def conv128_reference(x16, w, bias, dtype, table, alpha, B, H, W, table_image=None):
    """(ref, absref, extra) in fp64, NCHW [B, cout, H, W]; k is 1152.  With a table (fp32 [B, 128, 2], the values the kernel reads) the
    GroupNorm apply + SiLU from it, packed to 16 bits in place before the product (swin.hip:1079-1109), is mirrored.  DEFECT table_image:
    that image's table applied to every image."""
    cout = w.shape[0]
    wf = w.to(dtype).float()
    extra = None
    if table is None:
        r64, a64 = conv_ref(x16.float().reshape(B, H, W, 128).permute(0, 3, 1, 2), wf, None, padding=1)
    else:
        tb = table.cpu()
        if table_image is not None:
            tb = tb[table_image:table_image + 1].expand_as(tb)
        xg, flip = gn_apply16(x16.float().reshape(B, H * W, 128), tb[:, None, :, 0], tb[:, None, :, 1], dtype)
        xg, flip = (t.reshape(B, H, W, 128).permute(0, 3, 1, 2) for t in (xg, flip))
        r64, a64 = conv_ref(xg, wf, None, padding=1)
        extra = {"16-bit normalised operand, boundary values": abs(alpha) * F.conv2d(flip, wf.double().abs(), None, padding=1)}
    bd = bias[:cout, None, None].double()
    return alpha * r64 + bd, abs(alpha) * a64 + bd.abs(), extra


def stale_table_images(B, H, W, cus):
    """DEFECT map for conv128_by_patch_table: the image whose table each patch [B, H / 16, W / 16] is normalised with when a workgroup
    keeps the table of its FIRST patch for its whole walk (the reload at swin.hip:1066 missing)."""
    per = (H // 16) * (W // 16)
    grid = min(B * per, cus)
    return torch.tensor([(p % grid) // per for p in range(B * per)]).reshape(B, H // 16, W // 16)


def conv128_by_patch_table(x16, w, bias, dtype, table, alpha, B, H, W, patch_images):
    """The output of a kernel that normalises every 18 x 18 patch with the table of image patch_images[b, ty, tx]: assembled per 16 x 16
    output patch from the references with one image's table applied everywhere (a patch's output depends on that patch's pixels alone)."""
    out = torch.empty((B, w.shape[0], H, W), dtype=torch.float64)
    for t in sorted(set(patch_images.reshape(-1).tolist())):
        full = conv128_reference(x16, w, bias, dtype, table, alpha, B, H, W, table_image=t)[0]
        m = (patch_images == t).repeat_interleave(16, 1).repeat_interleave(16, 2)[:, None].expand_as(out)
        out[m] = full[m]
    return out


def nchw_planes_store(buf_view, values, n_valid, spill=False):
    """Emulates the fp32 NCHW epilogue's addressing (swin.hip:999-1006, :1136-1142) on a flat host view: image b's channel c at
    (b n_valid + c) H W.  `values` [B, >= n_valid (+ 1), H, W].  DEFECT spill: channel n_valid is stored as well — image b's lands on
    image b + 1's channel 0 before that image is written (the order of one workgroup walking the images), the last image's behind the
    tensor."""
    B, _, H, W = values.shape
    flat = buf_view.reshape(-1)
    for b in range(B):
        for c in range(n_valid + (1 if spill else 0)):
            o = (b * n_valid + c) * H * W
            n = max(min(H * W, flat.numel() - o), 0)            # (what lies behind the view is not emulated)
            flat[o:o + n] = values[b, c].reshape(-1)[:n].to(flat.dtype)
