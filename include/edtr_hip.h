/*
 * edtr_hip.h — C ABI of libedtr_hip.so, the MI355X (gfx950) kernel library underneath the
 * EDTR ControlLDM restoration path.
 *
 * The reference (JaehaKim97/EDTR) has no native code: every device op on its hot path is an
 * ATen call made from torch.nn modules.  Each entry point below therefore names the reference
 * call site(s) (file:line under the reference tree) whose ATen op it replaces.  The Python
 * host (edtr_amd/) binds these with ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain C: pointers, sizes, POD parameter structs; no torch / HIP types in signatures
 *     (a stream is passed as void* = hipStream_t; NULL = the default stream).
 *   - the caller owns every buffer (device memory unless stated); the library allocates
 *     nothing on the device and keeps no global mutable state; every launch is asynchronous
 *     on the given stream and is legal inside hipStreamBeginCapture (hipGraph capture).
 *   - activations are NHWC ("pixel-major") 16-bit (bf16 or fp16, chosen by `dtype`) with
 *     fp32 accumulation inside kernels; boundary tensors of the reference API (latents,
 *     images, eps) are NCHW fp32 and are converted by edtr_nchw_to_nhwc / edtr_nhwc_to_nchw.
 *   - 16-bit rows must be 16-byte aligned: channel counts, leading dimensions and column
 *     offsets are multiples of 8 elements.
 *   - return value: 0 = success; negative = EDTR_E* argument error (nothing was launched);
 *     positive = hipError_t from the launch.  Never throws, never exits.
 *
 * The Python binding is READ from this file at import (edtr_amd/header.py: structs, constants, prototypes), so the file keeps
 * to a narrow dialect and the reader refuses anything else: block comments only; `#define EDTR_NAME <integers, parentheses, <<>`;
 * enums with explicit values; `typedef struct edtr_x { ... } edtr_x;` of int / int32_t / int64_t / uint64_t / float and pointer
 * fields (no arrays, no nested structs); prototypes of such scalars, edtr_stream_t and pointers (no callbacks).  A struct array
 * that is passed twice is named `x_host` (the host reads it), then `x` (its device copy).
 */
#ifndef EDTR_HIP_H
#define EDTR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDTR_ABI_VERSION 10

enum edtr_dtype {
    EDTR_BF16 = 0, EDTR_F16 = 1,
    /* High-precision mode (accepted by the normalisation / layout / elementwise entry points that say so, never by
     * edtr_igemm / edtr_flash_attn64): the activation stream is fp32, and a tensor that feeds a GEMM is written as the bf16
     * "split-3" operand [hi | lo | hi] (3*C columns; hi = bf16(x), lo = bf16(x - hi)).  edtr_igemm (dtype EDTR_BF16, K = 3*C
     * per tap) multiplies it with weights packed [Wh | Wh | Wl]: hi*Wh + lo*Wh + hi*Wl = x*w to ~16 mantissa bits, fp32
     * accumulation, fp32 output.  This is what lets the path meet the 1e-3 parity target that 16-bit operands cannot. */
    EDTR_F32_SPLIT = 2,
    /* Mixed-precision mode: the same fp32 activation stream, but GEMM operands are FP16 and the number of operand parts is
     * chosen per layer (edtr_amd/precision.py): H1 = [x] (one fp16 rounding of the activation: a plain fp16 GEMM over an fp32
     * stream), H2 = [hi | lo] (2*C columns, hi = fp16(x), lo = fp16(x - hi): the activation is exact to ~22 bits, weights
     * packed [Wh | Wh] keep their single fp16 rounding), H3 = [hi | lo | hi] against [Wh | Wh | Wl] (~22 bits on both
     * sides).  A consumer may read a PREFIX of the parts ([hi], [hi | lo]) of a wider operand through ld1.  Every entry
     * point that accepts EDTR_F32_SPLIT accepts these; those that write no GEMM operand treat all four alike. */
    EDTR_F32_H1 = 3, EDTR_F32_H2 = 4, EDTR_F32_H3 = 5
};

enum edtr_error {
    EDTR_OK = 0,
    EDTR_E_NULL = -1,      /* required pointer is NULL */
    EDTR_E_SHAPE = -2,     /* non-positive or inconsistent extent */
    EDTR_E_ALIGN = -3,     /* pointer / leading dimension violates the 16-byte rule */
    EDTR_E_DTYPE = -4,     /* unknown dtype / flag value */
    EDTR_E_UNSUPPORTED = -5
};

enum edtr_act { EDTR_ACT_NONE = 0, EDTR_ACT_GEGLU = 1, EDTR_ACT_SILU = 2, EDTR_ACT_GELU = 3 /* exact erf GELU: the CLIP text MLP, model/open_clip/transformer.py:220-224; SwinIR Mlp, model/swinir.py:28-34 */,
                EDTR_ACT_LRELU = 4 /* x > 0 ? x : act_slope * x — SwinIR reconstruction convs, model/swinir.py:776,787,878-886 */ };

typedef void* edtr_stream_t; /* hipStream_t */

int edtr_abi_version(void);
const char* edtr_error_string(int code);
/* number of compute units / HBM bytes of the current device (0 on failure) */
int edtr_device_info(int* compute_units, int64_t* hbm_bytes, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear / batched GEMM on the matrix cores (MFMA 32x32x16).
 *
 *   out[z][m][n] = epilogue( alpha * sum_k A(z, m, k) * W[z][n][k] )
 *
 * replaces: F.conv2d 3x3 / 1x1 (reference model/unet.py:152,178,99-101,76-78,189;
 *           model/controlnet.py:138,261; model/vae.py:35-39,54-61,74-101), nn.Linear
 *           (model/attention.py:23,43,170-174,266,280; model/unet.py:168,476-480), the
 *           torch.cat feeding a conv (model/controlnet.py:35,37,266), F.interpolate(nearest,x2)
 *           feeding a conv (model/unet.py:76; model/vae.py:36), F.pad(0,1,0,1) (model/vae.py:57),
 *           and the bmm pair of the single-head VAE attention (model/vae.py:298).
 *
 * A operand ("im2col on the fly"): k = tap * (C1 + C2) + c, tap = ky * 3 + kx for taps == 9.
 *   pixel (b, oy, ox) = unflatten(m; OH, OW);  iy = oy*stride + ky - pad_t;  ix likewise;
 *   out-of-range taps read 0;  upsample2x != 0 reads source pixel (iy>>1, ix>>1) of an
 *   (IH, IW) source (logical input is 2IH x 2IW; upsample2x == 2: the same function in its sub-pixel
 *   form, see w_phase_stride);  channels c < C1 come from a1 (pixel stride
 *   ld1), the rest from a2 (pixel stride ld2) — the fused channel concat.
 *   taps == 1 and OH == 0: plain row-major matrix, A(z, m, k) = a1[z][m*ld1 + k] (concat too).
 *   K tail (a3 != NULL and C3 > 0; taps == 9, stride 1, pad 1, no upsample, C2 == 0): K = 9*C1 + C3, and columns
 *   k >= 9*C1 read a3[pixel(m)*ld3 + (k - 9*C1)] — the output pixel itself, no halo, no padding: a 1x1
 *   convolution of a second tensor summed into the same fp32 accumulator (the skip connection of a
 *   width-changing ResBlock, reference model/unet.py:219-223, model/vae.py:103-114, whose product is then
 *   never rounded to 16 bits or stored).  The weight rows are [9*C1 | C3] (ldw >= K), bias_n is the sum of the
 *   two biases.  a_gn applies to the 9-tap operand only.  Halo tiles 16 (16 x 16 patches and the 8 x 8-image
 *   form, split-K allowed: every split takes its proportional share of the C3/64 tail chunks), 17 and 20;
 *   C3 % 64 == 0, ld3 % 8 == 0; any other tile, stride, upsample, concat or a_wrap is EDTR_E_UNSUPPORTED.
 * W operand: row-major [N][K] (K contiguous, i.e. conv weights packed [Cout][ky][kx][Cin]).
 *   Rows n >= n_valid read as zero.
 * z (grid.z) offsets: operand_offset = (z / zdiv) * zs_outer + (z % zdiv) * zs_inner (elements).
 * Epilogue order: *alpha, +bias_n[n], +bias_m[m], GEGLU (value/gate column blocks of 32
 *   interleaved by the weight packer; output has N/2 columns), +rowvec[(m / rows_per_image)][n],
 *   SiLU / GELU / LeakyReLU, +residual[m][n], then store as 16-bit or fp32 at out[m*ldc + n].
 * ---------------------------------------------------------------------------------------- */
typedef struct edtr_igemm_params {
    int32_t dtype;          /* edtr_dtype of a1/a2/w/residual and of a 16-bit output */
    int32_t taps;           /* 1 or 9 */
    int32_t M, N, K;        /* K = taps * (C1 + C2), multiple of 8; N multiple of 8 */
    int32_t n_valid;        /* W rows >= n_valid are zero (0 means N) */
    int32_t Z, zdiv;        /* batch count (grid.z) and its split (zdiv >= 1) */
    /* A */
    const void* a1; const void* a2;
    int32_t C1, C2, ld1, ld2;
    int64_t a_zs_outer, a_zs_inner;
    int32_t IH, IW, OH, OW; /* spatial mode when OH > 0 */
    int32_t stride, pad_t, pad_l, upsample2x;
    /* W */
    const void* w; int32_t ldw;
    int64_t w_zs_outer, w_zs_inner;
    /* epilogue */
    float alpha;
    const float* bias_n; const float* bias_m;
    const float* rowvec; int32_t rowvec_ld; int32_t rows_per_image;
    int32_t act;            /* edtr_act */
    const void* residual; int32_t ldr;
    /* out */
    void* out; int32_t ldc; int32_t out_f32;
    int64_t o_zs_outer, o_zs_inner;
    int32_t tile;           /* 0 = auto; explicit main-loop choice (tests / A-B runs): 1 = 128x128 register-staged, 2 = 64x64,
                               3 = 128x128 LDS-DMA (2 stages), 6 = 256x256 ping-pong, 8 = 128x160, 14 = 256x32 for N <= 32 (automatic for
                               large-M skinny-N convolutions), 16 = halo tile (3x3 / stride 1 / pad 1 convolutions — plain, nearest-2x
                               upsampled as a gather or in the sub-pixel form, or four whole 8x8 images per workgroup — on outputs whose
                               height and width are multiples of 16: the 18x18 input patch of a 16x16 output patch stays in LDS for
                               all taps; automatic for N % 128 == 0 and >= 48 units incl. split-K; EDTR_E_UNSUPPORTED for any other
                               shape); 17 = the halo tile on 32 x 16-pixel units (ABI 9, halo512.hip: 32-channel chunks, a wave owns 128
                               pixels x 64 channels over ALL of K, epilogue straight from the accumulators with whole-line stores; plain
                               3x3 / stride 1 / pad 1 convolutions with OW % 32 == 0, OH % 16 == 0, N % 128 == 0, C1 % 32 == 0, no split-K /
                               activation / bias_m; a_gn allowed; automatic where tile 16 would run and >= 256 such units exist:
                               1.10 - 1.13 x over tile 16 on the VAE's convolutions); 20 = the halo tile on 16 x 16 pixels x 160 channels
                               (ABI 9, halo512.hip: N % 160 == 0, otherwise tile 17's rules with OW % 16 == 0 and no a_gn; automatic
                               where the 128x160 tile would run and the units fill one round of the chip, 192 .. 256: the 64 x 64-latent
                               ResBlock convolutions at batch 8); 21 = tile 17 as a persistent kernel (ABI 10, halo512.hip: one workgroup per
                               CU walks its units, the finished 16-bit output of a unit leaves under the next unit's multiply loop; bit-identical
                               to tile 17; 16-bit output, no residual / rowvec, N <= 512, C1 % 64 == 0; never automatic — 1.00 - 1.05 x in
                               isolation, neutral on the whole path: profiles/r06/halo512p_*.log; EDTR_IGEMM_HALO512P=N picks it from N units
                               per CU for A/B runs).  4, 5, 7, 9 - 13, 15, 18, 19 were experiments (3-stage BK32, 256x128 tiles, 64x128,
                               16x16x32 at 128x128, deeper LDS rings, bank-swizzled epilogue staging, an 8-wave ping-pong 128x128 tile
                               for small grids, two-workgroup and persistent halo variants), measured without a whole-path gain
                               (profiles/r01 - r03) and removed: EDTR_E_DTYPE */
    /* split-K (small-M problems that cannot fill 256 CUs): K is cut into `splitk` runs of K-tiles, each
     * workgroup row writes an fp32 partial slab into `workspace` ([splitk][M][N] floats, caller-owned), and a
     * second launch sums the slabs and applies the epilogue.  splitk <= 1 disables it.  Needs Z == 1, no GEGLU. */
    int32_t splitk;
    void* workspace; int64_t workspace_bytes;
    /* fused GroupNorm statistics of the OUTPUT (optional): the epilogue also writes, per 128-row tile, the per-column
     * sum and sum of squares of the values it stores: gn_partial[(M/128)][N][2] fp32 (which rows a slot covers is the
     * kernel's business — the halo tile fills slot 2k with a 256-pixel patch and zeroes slot 2k+1 — only the per-image
     * totals over an image's H*W/128 consecutive slots are defined).  edtr_gn_finalize folds them into
     * the fp64 sums edtr_gn_apply consumes, so the separate statistics pass over the tensor (edtr_gn_stats) disappears.
     * Needs M % 128 == 0, no GEGLU / z-batching, tile 0/1/3/6/8/16 (16-bit or fp32 output).
     * With split-K (ABI 10) the REDUCER writes them (the main loops only write slabs): slots of gn_slot_rows rows (0 = 128; 64 for the
     * 8 x 8 images of the deepest latent level, where a 128-row slot would straddle two images), gn_partial[M / gn_slot_rows][N][2];
     * needs M % gn_slot_rows == 0 and N % 32 == 0.  Without split-K gn_slot_rows must be 0 or 128. */
    float* gn_partial;
    float act_slope;        /* negative-side slope of EDTR_ACT_LRELU (0 <= slope <= 1) */
    int32_t residual_f32;   /* nonzero: `residual` is fp32 (ldr in floats, multiple of 4): the fp32 activation stream of the
                               high / mixed precision modes adds its skip inside the epilogue instead of in a separate launch */
    /* Transposed second output (optional): the fused [Wq; Wk; Wv] projection of a self-attention in ONE launch.  Output columns
     * n >= vt_col0 are not stored at out[m][n] but TRANSPOSED, as the V^T operand edtr_flash_attn64 reads:
     *   vt_out[(m / rows_per_image) * (N - vt_col0) + (n - vt_col0)][m % rows_per_image]   (row stride vt_ld, 16-bit)
     * scaled by vt_alpha instead of alpha (the q / k halves carry the softmax scale, v does not); bias_n applies to all columns.
     * Needs rows_per_image % 8 == 0, M % 8 == 0, vt_ld % 8 == 0, vt_col0 a multiple of the column-tile width (128, or 160 for
     * tile 8: every SD width), Z == 1, no split-K / GEGLU / residual / rowvec, tile 0 / 1 / 3 / 8.  replaces: `to_v(x)` +
     * the `b n (h d) -> (b h) n d` rearrange of v, reference model/attention.py:172-178. */
    void* vt_out; int32_t vt_col0; int32_t vt_ld; float vt_alpha;
    /* LayerNorm folded into the GEMMs around it (fast modes; reference model/attention.py:222-224,230-234: x + attn(norm(x))).
     * LayerNorm is affine per row, so  LN(x) W^T = rstd_r (x (gamma . W)^T - mean_r c1) + c2  with c1[n] = sum_k (gamma . W)[n][k]
     * (of the packed 16-bit values) and c2[n] = sum_k beta[k] W[n][k]: the GEMM runs on the RAW rows against weights pre-multiplied
     * by gamma, and its epilogue applies the two row scalars — the normalised tensor is never written or read, the edtr_layernorm
     * launch disappears and one 16-bit rounding (of the normalised activations) with it.
     *   producer side — row_stats (optional): the launch that WRITES x also writes, per row, the sum and the sum of squares of
     *     the values it stores: row_stats[m][N / 32][2] fp32; a column tile fills the slot of its first 32 columns and zeroes
     *     the other slots it covers, so the totals over a row's N / 32 slots are defined whatever tile ran (no atomics:
     *     results stay bit-reproducible).  Needs N % 32 == 0, Z == 1, no split-K / GEGLU, a row-major tile (not tile 16).
     *   consumer side — ln_stats (optional): row statistics of the A operand's rows (ln_slots = K / 32 slots per row; ln_C <= K
     *     = the number of real columns the mean / variance run over — pad columns must be zero —, eps ln_eps); the epilogue computes out = rstd (alpha acc - mean alpha c1[n]) + alpha c2[n] + bias_n[n]
     *     (vt_alpha for the transposed V columns), then GEGLU / activation / residual as usual.  Needs Z == 1, no split-K,
     *     taps == 1, tile 0 / 1 / 3 (an automatic 128x160 choice falls back to tile 3). */
    float* row_stats;
    const float* ln_stats; int32_t ln_slots; int32_t ln_C; float ln_eps;
    const float* ln_c1; const float* ln_c2;
    int32_t stagger;        /* set by edtr_igemm itself (the caller's value is ignored): cycles by which the second workgroup of
                               every CU starts late, so that the two resident workgroups of the 128-row tiles do not run their K
                               loops and their store bursts in lockstep */
    int32_t debug_flags;    /* set by edtr_igemm itself from the environment (A/B measurements on one device): bit 0 =
                               EDTR_IGEMM_GENERAL_EPILOGUE=1, every launch takes the general epilogue row loop; bit 1 = EDTR_IGEMM_N160_TWO_PASS=1,
                               the 128x160 tile stages its accumulators in two passes of 64 rows; bit 2 = EDTR_IGEMM_GEGLU_SERIAL=1, the GEGLU epilogue evaluates
                               its gates one value after the other (the form before the eight-value lockstep evaluation) */
    /* Sub-pixel form of `F.interpolate(x, scale_factor=2, mode="nearest")` + 3x3 conv (ABI 7; upsample2x == 2; reference
     * model/unet.py:70-79, model/vae.py:35-39).  The 2 x 2 blocks of the upsampled image are constant, so output pixel
     * (2s + py, 2r + px) is a 2 x 2 convolution of the SOURCE image whose weights are sums of the 3 x 3 kernel's rows / columns:
     *   rows    py = 0: {w[0]} on source row s - 1, {w[1] + w[2]} on s;     py = 1: {w[0] + w[1]} on s, {w[2]} on s + 1   (columns alike)
     * i.e. 4 multiply-adds per output element and input channel instead of 9.  `w` then holds FOUR phase matrices
     * [2 py + px][N][dy][dx][C1] (K' = 4 C1 per row, row stride ldw >= 4 C1), `w_phase_stride` elements apart, summed in fp32 by
     * the packer BEFORE the 16-bit (or multi-part) rounding.  taps stays 9 and K = 9 C1 (the algorithmic shape).  Halo kernel only
     * (tile 0 / 16): IH, IW multiples of 16, C1 % 64 == 0, stride 1, pad 1; anything else is EDTR_E_UNSUPPORTED. */
    int64_t w_phase_stride;
    /* 16-bit MIRROR of an fp32 output (ABI 7; mixed-precision mode): when out_f32 != 0 and out16 != NULL the epilogue also stores
     * the final values rounded to `dtype` at out16[m * ld16 + n] — the one-part GEMM operand that the 16-bit consumers of the fp32
     * residual stream (1x1 skip / zero convolutions, down / upsample convolutions) read, instead of a separate cast launch per
     * consumer (edtr_split_operand).  Needs Z == 1, no GEGLU / transposed output; ld16 % 8 == 0. */
    void* out16; int32_t ld16;
    /* Weights-exact two-part product (ABI 7): a_wrap > 0 reads the A operand's columns TWICE, A(m, k) = a1[m * ld1 + (k mod a_wrap)],
     * K = 2 * a_wrap, against weights packed [Wh | Wl] (hi / lo halves of the fp32 weight): x16 . (Wh + Wl) — the weight rounding
     * disappears at twice the MFMA work, with no low part of the activation to form.  Plain GEMMs (taps 1, non-spatial, no concat),
     * a_wrap % 64 == 0, tiles 0 / 1 / 2 / 3 / 8. */
    int32_t a_wrap;
    /* GroupNorm apply (+ SiLU) of the INPUT fused into the operand staging (ABI 8; fast 16-bit modes): a_gn = fp32 [B][C1][2], the
     * (scale, shift) edtr_gn_table derives from the tensor's statistics; the convolution then multiplies
     *   act(a1 * scale[image][c] + shift[image][c]),  act = SiLU when a_gn_silu != 0, zero outside the image (the padding),
     * rounded to `dtype` exactly as edtr_gn_apply stores it — the normalised tensor is never written or read.  Halo tile only, in
     * its 16 x 16-patch geometry (taps 9, stride 1, pad 1, OH % 16 == OW % 16 == 0, C1 % 64 == 0, no upsample, not the 8 x 8 image
     * form; split-K allowed); anything else is EDTR_E_UNSUPPORTED and the caller issues edtr_gn_apply.
     * replaces: `F.silu(self.norm1(x))` / `in_layers[:2]` in front of the 3 x 3 convolutions of the ResBlocks, reference
     * model/vae.py:103-114, model/unet.py:203-218 (GroupNorm32 + SiLU, model/util.py:146-163). */
    const float* a_gn; int32_t a_gn_silu;
    int32_t gn_slot_rows;   /* rows per gn_partial slot when the split-K reducer writes the statistics (ABI 10; see gn_partial): 0 / 128 / 64 */
    int32_t gn_ld;          /* channels per gn_partial slot (ABI 10): 0 = N; > N when the output is a column slice of a concatenation whose
                               halves share one buffer of slots — gn_partial then points at this launch's first column inside a slot
                               (slot s, column n of this launch at gn_partial[(s * gn_ld + n) * 2]); edtr_add_stats writes the other half */
    /* K tail of a 3x3 convolution (additive in ABI 10; see "K tail" in the A-operand comment above): C3 more columns read at the
     * output pixel itself from a3 (pixel stride ld3).  a3 == NULL or C3 == 0: no tail. */
    const void* a3;
    int32_t C3, ld3;
} edtr_igemm_params;

int edtr_igemm(const edtr_igemm_params* p, edtr_stream_t stream);
/* Which kernel would edtr_igemm run for these parameters (ABI 9)?  All of edtr_igemm's validation and shape rules, no launch and no
 * HIP call (works without a GPU): > 0 = the tile number (see `tile` above), < 0 = the error edtr_igemm would return.  The host side
 * uses it to keep its own launch-shape predicates (edtr_amd/ops.py: gn_in_conv_ok, subpixel_ok) provably inside the library's. */
int edtr_igemm_plan(const edtr_igemm_params* p);

/* ------------------------------------------------------------------------------------------
 * Fused multi-head attention, head width 64: out = softmax(q k^T * scale) v per (batch, head),
 * online softmax, scores never leave the CU.
 * replaces: F.scaled_dot_product_attention, reference model/attention.py:193 (46 calls/step).
 *   q   : [B][Nq][q_ld]  head h occupies columns h*64 .. h*64+63
 *   k   : [B][Nk][k_ld]  same column convention
 *   vt  : [B][H*64][vt_ld]  V transposed ("key-major"): row h*64+d holds v[:, h*64+d] over the
 *         keys; vt_ld >= roundup8(Nk).  The padding keys [Nk, roundup8(Nk)) are read and must be
 *         FINITE (any value: a masked key gets probability exactly 0, so 0 * pad adds nothing,
 *         but 0 * NaN / Inf would); columns at or beyond roundup8(Nk) are never read
 *   out : [B][Nq][o_ld]
 * ---------------------------------------------------------------------------------------- */
typedef struct edtr_attn_params {
    int32_t dtype;
    int32_t B, H, Nq, Nk;
    const void* q; int64_t q_bs; int32_t q_ld;
    const void* k; int64_t k_bs; int32_t k_ld;
    const void* vt; int64_t vt_bs; int32_t vt_ld;
    void* out; int64_t o_bs; int32_t o_ld;
    float scale;
    int32_t causal;                 /* nonzero: key j contributes to query i only if j <= i (the CLIP text tower's attn_mask,
                                       reference model/open_clip/model.py build_attention_mask; Nq == Nk) */
    int32_t q_prescaled;            /* nonzero: the q.k products already carry scale*log2(e) (the projection GEMMs that produced q
                                       and/or k applied it in fp32 before their single 16-bit rounding), so the kernel evaluates
                                       exp2(q.k - max) directly and ignores `scale`: one v_exp and no multiply per score */
    /* Split operands (ABI 7; the robust parity mode): q_lo / k_lo (both or neither) and optionally vt_lo hold the LOW halves of
     * hi + lo fp16 (bf16) pairs, laid out like q / k / vt (same strides): x = hi + lo to ~22 bits, as edtr_split_operand writes
     * them ([hi | lo] columns: lo = hi + C elements).  The products then run as three MFMA products each,
     *   S = Qh Kh^T + Ql Kh^T + Qh Kl^T,   O = Ph Vh + Pl Vh + Ph Vl  (P split in registers; PV only with vt_lo),
     * which removes the 16-bit rounding of the attention operands — on sharp attention (tests/golden/heavy.npz) the rounding
     * of q and k alone costs 2.7e-3 of a denoiser evaluation (tests/heavy_attention_budget.py).  out_f32 != 0 (split mode only):
     * fp32 output (o_ld / o_bs in floats).  replaces: the same F.scaled_dot_product_attention call in fp32. */
    const void* q_lo; const void* k_lo; const void* vt_lo;
    int32_t out_f32;
} edtr_attn_params;

int edtr_flash_attn64(const edtr_attn_params* p, edtr_stream_t stream);

/* Which kernel would edtr_flash_attn64 run for these parameters (additive in ABI 10)?  All of edtr_flash_attn64's validation and its
 * shape rules, no launch and no HIP call (works without a GPU; the pointers are only tested for NULL and alignment): < 0 = the error
 * edtr_flash_attn64 would return, > 0 = one of the ids below.  edtr_flash_attn64 dispatches on the same function, and the switches
 * EDTR_ATTN_V3, EDTR_ATTN_V3_MIN_NQ and EDTR_ATTN_SMALLK act on both alike (read once per process).  blocks_per_wg (may be NULL)
 * receives the 32-query blocks one workgroup of the small-Nk kernel walks (4 / 8 / 12 / 16: one to four per wave, from
 * B * H * ceil(Nq / 32) / 2048), 0 for every other kernel.  The generic and the large-N kernel deal heads, not query blocks, to the
 * XCDs when B * H % 8 == 0. */
enum edtr_attn_kernel {
    EDTR_ATTN_GENERIC = 1,      /* 128 queries per workgroup, online softmax over 64-key tiles: any shape, the causal mask */
    EDTR_ATTN_SPLIT_QK = 2,     /* q_lo / k_lo given: three MFMA products per score */
    EDTR_ATTN_SPLIT_QKPV = 3,   /* and vt_lo: three per output product too */
    EDTR_ATTN_SMALLK = 4,       /* Nk <= 128, not causal: K / V^T resident in LDS, two-pass softmax */
    EDTR_ATTN_V3 = 5            /* q_prescaled, not causal, Nq >= 2048 (EDTR_ATTN_V3_MIN_NQ), Nk % 256 == 0: the generated large-N loop */
};
int edtr_flash_attn64_plan(const edtr_attn_params* p, int* blocks_per_wg);

/* Fused single-head attention with head width 512 (ABI 9): the VAE's AttnBlock, softmax(q k^T * scale) v over the latent positions.
 * Same parameter block as edtr_flash_attn64 with H == 1 and rows of 512 channels: q [B][Nq][q_ld], k [B][Nk][k_ld],
 * vt = V^T [B][512][vt_ld] (vt_ld >= Nk), out [B][Nq][o_ld] (16-bit, or fp32 with out_f32); `scale` is applied inside.
 * Nk must be a multiple of 32 (EDTR_E_UNSUPPORTED otherwise: the caller keeps GEMM -> edtr_softmax_rows -> GEMM); any Nq;
 * no causal mask / pre-scaled q / split operands.  The score matrix never exists in memory (4096^2 fp32 per image before).
 * replaces: F.scaled_dot_product_attention in AttnBlock.forward, reference model/vae.py:279-308 (and the tile-local attention of
 * utils/tilevae/attn.py:85-115). */
int edtr_flash_attn512(const edtr_attn_params* p, edtr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GroupNorm (32 groups in the reference; `groups` here) over NHWC 16-bit activations, fp32 math.
 * replaces: GroupNorm32 (model/util.py:146-163, eps 1e-5), Normalize (model/attention.py:50-51,
 *           model/vae.py:22-23, eps 1e-6) and the SiLU / x*sigmoid(x) that follows
 *           (model/unet.py:150,175,677; model/vae.py:17-19,104-113,443-444,555-556).
 * Two launches: edtr_gn_stats accumulates per-(image, group) sum / sum of squares in fp64
 * (sums[B][groups][2], zeroed by the call itself); edtr_gn_apply normalises, applies the affine
 * and optionally SiLU.
 * ---------------------------------------------------------------------------------------- */
typedef struct edtr_gn_params {
    int32_t dtype;
    int32_t B, HW, C, groups;
    const void* x; int32_t ldx;     /* pixel stride of x (>= C) */
    double* sums;                   /* [B][groups][2] workspace */
    const float* gamma; const float* beta; /* [C] */
    float eps;
    int32_t silu;                   /* 0 / 1 */
    void* y; int32_t ldy;
    int32_t sums_zeroed;            /* edtr_gn_stats only: nonzero = the caller has already zeroed `sums` (e.g. one edtr_zero_bytes
                                       over a pool of them), so no per-call memset node is enqueued */
    /* edtr_gn_apply only (optional): fold the per-tile column partials of the producing edtr_igemm (gn_partial,
     * tiles_per_image = H*W/128 — or H*W/64 where the split-K reducer wrote 64-row slots — <= 64 tiles per image) inside the apply launch itself — `sums` is then ignored and the
     * edtr_gn_finalize launch disappears (one launch less per GroupNorm of the UNet / ControlNet levels). */
    const float* partial; int32_t tiles_per_image;
} edtr_gn_params;

int edtr_gn_stats(const edtr_gn_params* p, edtr_stream_t stream);
/* Fold the per-tile column partials written by an edtr_igemm epilogue (gn_partial, tiles_per_image = H*W/128 tiles per
 * image, C columns) into sums[B][groups][2] — a drop-in replacement for edtr_gn_stats on that tensor. */
int edtr_gn_finalize(const float* partial, int tiles_per_image, int B, int C, int groups, double* sums,
                     edtr_stream_t stream);
int edtr_gn_apply(const edtr_gn_params* p, edtr_stream_t stream);
/* (scale, shift) = (gamma[c] rstd, beta[c] - mean gamma[c] rstd) per image and channel, table[B][C][2] fp32, from the tile partials
 * of the producing edtr_igemm (partial != NULL) or from the fp64 sums of edtr_gn_stats / edtr_gn_finalize: what edtr_gn_apply forms
 * per channel before it touches the tensor — for edtr_igemm's a_gn, which applies it while staging its operand (ABI 8). */
int edtr_gn_table(const float* partial, int tiles_per_image, const double* sums, int B, int C, int groups, int HW,
                  const float* gamma, const float* beta, float eps, float* table, edtr_stream_t stream);

/* LayerNorm over the last dimension, rows x C (C <= 2048, multiple of 8), fp32 math, 16-bit in/out.
 * c_valid (0 = C): only the first c_valid columns are real — the statistics run over them, and columns c_valid..C-1 of y are
 * written as zeros (SwinIR keeps its 180 channels in rows of 192 so that every GEMM has K % 64 == 0; gamma / beta hold C entries).
 * replaces: nn.LayerNorm, reference model/attention.py:222-224; model/swinir.py:208,215,753 (norm1 / norm2 / norm). */
int edtr_layernorm(int dtype, const void* x, int64_t rows, int C, int c_valid, int ldx, const float* gamma,
                   const float* beta, float eps, void* y, int ldy, edtr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Shifted-window multi-head attention of SwinIR, window 8 x 8 (64 tokens), head width <= 32, one launch per layer:
 * cyclic shift, window partition, q k^T * scale + relative-position bias + region mask, softmax, P v, window merge and
 * reverse shift.  One wavefront per (window, head); the 64 x 64 scores never leave registers.
 * replaces: torch.roll + window_partition + WindowAttention.forward (up to, not including, `proj`) + window_reverse +
 *           torch.roll, reference model/swinir.py:254-279 and :120-148.
 *   qkv    : [B*H*W][ld_qkv] 16-bit, token (b, y, x) at row (b*H + y)*W + x of the UNSHIFTED image; columns
 *            s*heads*32 + h*32 + e  (s = 0/1/2 for q/k/v, e < 32; e >= head_dim must be zero — the packed projection
 *            has zero weight rows there)
 *   out    : [B*H*W][ld_out] 16-bit; head h writes columns h*head_dim .. h*head_dim+head_dim-1, and columns
 *            heads*head_dim .. c_pad-1 are written as zeros
 *   bias   : fp32 [heads][64][64], bias[h][i][j] added to the score of query i and key j (the gathered
 *            relative_position_bias_table)
 *   labels : NULL when shift == 0; else uint8 [H][W], the image region of each pixel of the SHIFTED frame; a pair whose
 *            labels differ gets -100 added (the reference's attn_mask values, model/swinir.py:241)
 * ---------------------------------------------------------------------------------------- */
typedef struct edtr_window_attn_params {
    int32_t dtype;
    int32_t B, H, W;                /* token grid; H % 8 == 0, W % 8 == 0 */
    int32_t heads, head_dim;        /* head_dim even, <= 32 */
    int32_t shift;                  /* 0 <= shift < 8: window (wy, wx) token (ty, tx) is pixel ((8wy+ty+shift) % H, (8wx+tx+shift) % W) */
    const void* qkv; int32_t ld_qkv;
    void* out; int32_t ld_out; int32_t c_pad;
    const float* bias;
    const uint8_t* labels;
    float scale;
} edtr_window_attn_params;

int edtr_window_attn(const edtr_window_attn_params* p, edtr_stream_t stream);

/* The MLP half of a Swin layer in one launch (ABI 8):  out = x + fc2(GELU(fc1(LayerNorm(x)))) on 16-bit token rows.
 * replaces: `x = x + self.drop_path(self.mlp(self.norm2(x)))`, reference model/swinir.py:281-283 with Mlp.forward :31-37
 *           (nn.LayerNorm eps 1e-5, nn.GELU exact, both dropouts are p = 0).
 * Specialised for the shipped pre-restorer (configs/det/demo.yaml:2-18: embed_dim 180, mlp_ratio 2): C = 192 padded token
 * columns, hidden = 384 padded hidden units; anything else is EDTR_E_UNSUPPORTED and the caller issues the two edtr_igemm
 * launches instead.  Pad columns of x must be zero and stay zero (zero weight rows / bias entries).
 *   x      : [rows][ldx] 16-bit; LayerNorm statistics run over the first c_valid columns' stored values
 *   w1     : fc1 weights pre-multiplied by the LayerNorm gamma, rounded to `dtype`, as hidden/32 LDS images of 12288 bytes:
 *            image t, byte r*384 + ((c ^ ((r >> 1) & 7)) << 4) + 2 j  =  (gamma . W1)[32 t + r][8 c + j]    (r < 32, c < 24, j < 8)
 *   w2     : fc2 weights as hidden/32 images of 12288 bytes:
 *            image t, byte r*64 + ((c ^ ((r >> 2) & 3)) << 4) + 2 j   =  W2[r][32 t + 8 c + j]                (r < 192, c < 4, j < 8)
 *            (the XOR keys make every ds_read_b128 of an MFMA operand conflict-free; the images are copied by LDS-DMA as they are)
 *   c1     : fp32 [hidden], row sums of the PACKED 16-bit (gamma . W1)    c2b : fp32 [hidden], W1 beta + fc1 bias
 *            pre[u] = rstd (acc[u] - mean c1[u]) + c2b[u]   — the folded LayerNorm of edtr_igemm's ln_stats, with the row
 *            statistics taken inside the kernel from the x rows it already holds
 *   b2     : fp32 [C] fc2 bias (pad entries zero)
 *   out    : [rows][ldo] 16-bit (may be x itself: a workgroup reads only the rows it writes, and has read them all before its first store)
 *   row_stats : optional fp32 [rows][C/32][2], the (sum, sum of squares) slots of the stored output rows in edtr_igemm's
 *            row_stats format (slots 0 and 3 carry the sums of columns 0..95 / 96..191, the others are zero), for the
 *            LayerNorm folded into the next layer's qkv projection.
 * ldx % 8 == 0, ldo % 8 == 0, all pointers 16-byte aligned. */
typedef struct edtr_swin_mlp_params {
    int32_t dtype;
    int32_t rows, C, hidden, c_valid;
    float eps;
    const void* x; int32_t ldx;
    const void* w1; const void* w2;
    const float* c1; const float* c2b; const float* b2;
    void* out; int32_t ldo;
    float* row_stats;
} edtr_swin_mlp_params;

int edtr_swin_mlp(const edtr_swin_mlp_params* p, edtr_stream_t stream);

/* The attention half of a Swin layer in one launch (ABI 8):  out = x + proj(WindowAttention(LayerNorm(x))) on 16-bit token rows.
 * replaces: `shortcut + window_reverse(attn(window_partition(roll(norm1(x)))))`, reference model/swinir.py:254-279 with
 *           WindowAttention.forward :120-148 (qkv linear, q * scale, relative-position bias, shift mask, softmax, proj linear; the
 *           dropouts are p = 0) — i.e. the qkv edtr_igemm, edtr_window_attn and the proj edtr_igemm of the three-launch form.
 * Specialised for the shipped pre-restorer (embed_dim 180 -> C = 192 padded columns, 6 heads of width 30 -> 32, window 8); anything
 * else is EDTR_E_UNSUPPORTED and the caller issues the three launches.  Pad columns of x must be zero and stay zero.
 *   x, out : [B*H*W][ld] 16-bit, token (b, y, x) at row (b*H + y)*W + x; out must not alias x (workgroups gather rows others scatter)
 *   wqkv   : heads * 3 LDS images of 12288 bytes, image 3 h + s (s = 0 / 1 / 2: q / k / v), layout as edtr_swin_mlp's w1 images:
 *            byte r*384 + ((c ^ ((r >> 1) & 7)) << 4) + 2 j = (gamma . Wqkv)[s*C' + h*d + r][8 c + j] for r < d, zero rows above
 *            (C' = heads*d, d = head_dim); the q rows are pre-multiplied by the softmax scale d^-1/2
 *   wproj  : heads images of 12288 bytes, image h, layout as edtr_swin_mlp's w2 images:
 *            byte r*64 + ((c ^ ((r >> 2) & 3)) << 4) + 2 j = Wproj[r][h*d + 8 c + j]   (zero for 8 c + j >= d, r >= C')
 *   c1, c2b: fp32 [3][heads][32]: row sums of the packed 16-bit (gamma . Wqkv) rows / Wqkv beta + bias (q entries scaled), zero pads
 *   bproj  : fp32 [C] (pad entries zero)
 *   bias   : fp32 [heads][16][64][4]: bias[h][kg][i][e] is added to the score of query i and key 4 kg + e (the gathered
 *            relative_position_bias_table, key-group major so that the 32 queries of a wave read contiguous 16-byte entries)
 *   labels : as edtr_window_attn (NULL when shift == 0)
 * LayerNorm statistics come from the gathered rows themselves (c_valid real columns, eps).  ld % 8 == 0, W % 4 == 0, pointers
 * 16-byte aligned. */
typedef struct edtr_swin_attn_params {
    int32_t dtype;
    int32_t B, H, W;                /* token grid; H % 8 == 0, W % 8 == 0 */
    int32_t heads, head_dim, shift;
    int32_t C, c_valid;
    float eps;
    const void* x; int32_t ldx;
    const void* wqkv; const void* wproj;
    const float* c1; const float* c2b; const float* bproj;
    const float* bias;
    const uint8_t* labels;
    void* out; int32_t ldo;
} edtr_swin_attn_params;

int edtr_swin_attn(const edtr_swin_attn_params* p, edtr_stream_t stream);

/* A whole Swin layer in one launch (ABI 8): edtr_swin_attn followed by edtr_swin_mlp on the token tile the attention half leaves in
 * LDS — `attn->out` receives x + attention half + MLP half; `mlp->x`, `->out`, `->rows`, `->row_stats` and the ld fields are ignored
 * (the tile never leaves the workgroup between the halves), its weight / constant operands are those of edtr_swin_mlp.  Same
 * shape and alignment rules as the two entry points.  replaces: SwinTransformerBlock.forward, reference model/swinir.py:254-283. */
int edtr_swin_layer(const edtr_swin_attn_params* attn, const edtr_swin_mlp_params* mlp, edtr_stream_t stream);

/* The feed-forward half of a BasicTransformerBlock in one launch (ABI 10):  out = x + W2 GEGLU(W1 LayerNorm(x) + b1) + b2.
 * replaces: `x = self.ff(self.norm3(x)) + x`, reference model/attention.py:233 with FeedForward :30-47 / GEGLU :20-27
 *           (nn.LayerNorm eps 1e-5, exact GELU, Dropout p = 0) — i.e. the LayerNorm launch (or fold) and the two edtr_igemm
 *           launches `ff.geglu` / `ff.out` of the two-launch form; the (rows, 4 d) hidden tensor never reaches memory.
 * Built for the 64 x 64-latent level of the SD-2.1 UNet / ControlNet: D = 320, H = 4 D = 1280, M % 128 == 0; anything else is
 * EDTR_E_UNSUPPORTED (edtr_ffn_plan answers without a launch) and the caller issues the two edtr_igemm launches.
 *   x   : [M][ldx] 16-bit RAW rows (before the LayerNorm): the kernel normalises them in registers (two-pass statistics over the
 *         stored values, (x - mean) rstd rounded to 16 bits) and reads them again for the residual
 *   w1  : [2 H][D] 16-bit, the GEGLU projection pre-multiplied by the LayerNorm gamma, value / gate rows interleaved in blocks of
 *         32 exactly as edtr_igemm's EDTR_ACT_GEGLU operand (rows 64 J .. 64 J + 31 = values of gated units 32 J .., the next 32
 *         rows their gates)
 *   w2  : [D][H] 16-bit, the output projection with its COLUMNS permuted inside every aligned group of 16:
 *         stored column 16 g + i = original column 16 g + {0,1,2,3, 8,9,10,11, 4,5,6,7, 12,13,14,15}[i]
 *         (the accumulator registers of the first product are then the operand of the second without a shuffle)
 *   cst : fp32 [H / 64][2][64]: the per-unit constant (W1 beta + b1)[R] of chunk c, half hh, at (q*2 + vg)*8 + lh*4 + e  for the
 *         packed w1 row R = 128 c + 64 hh + 32 vg + (e + 8 q + 4 lh)   (q, e < 4; vg = 0 value / 1 gate; lh < 2); the GATE
 *         entries (vg = 1) are stored HALVED (the kernel evaluates gelu from gate / 2)
 *   b2  : fp32 [D]
 *   out : [M][ldo] 16-bit, must not alias x (rows are re-read as the residual)
 * ldx % 8 == 0, ldo % 8 == 0, all pointers 16-byte aligned. */
typedef struct edtr_ffn_params {
    int32_t dtype;
    int32_t M, D, H;
    float eps;
    const void* x; int32_t ldx;
    const void* w1; const void* w2;
    const float* cst; const float* b2;
    void* out; int32_t ldo;
} edtr_ffn_params;

int edtr_ffn(const edtr_ffn_params* p, edtr_stream_t stream);
int edtr_ffn_plan(const edtr_ffn_params* p);      /* no HIP call: EDTR_OK or the error edtr_ffn would return */

/* The K = 320 linear layers of the 64 x 64-latent transformer blocks as a row-resident product, optionally with the LayerNorm in front
 * (ABI 10, lin320.hip):
 *     out[m][n] = alpha * sum_k xhat[m][k] w[n][k] + cvec[n] (+ residual[m][n]),   xhat = x, or (x - mean_m) rstd_m rounded to 16 bits
 * replaces: `attn2.to_q(norm2(x))` (model/attention.py:171, 224-232: ln = 1, alpha = the softmax prescale), `to_out[0](o) + x`
 * (:195), `proj_in` / `proj_out(x) + x_in` (:283-302) — an edtr_layernorm launch + an edtr_igemm launch, or one edtr_igemm launch.
 * A wave keeps 32 token rows in registers (loaded once, normalised in place), LDS holds only the weight stream.
 *   x        [M][ldx] 16-bit rows, K = 320 valid columns
 *   w        the [N][320] weight matrix in FRAGMENT order: 16 bytes per (chunk c of 32 output columns, k-step s of 16, lane l) at
 *            ((c * 20 + s) * 64 + l) * 16 = w[32 c + (l & 31)][16 s + 8 (l >> 5) .. + 7] (ops.pack_lin320_w); with ln != 0 the caller
 *            has folded the LayerNorm's gamma into the columns and put alpha * (W beta) (+ bias) into cvec
 *   cvec     fp32 [N] or NULL; residual: 16-bit [M][ldr] or NULL; out: 16-bit [M][ldo], != x
 *   vt_out   optional (the fused [Wq; Wk; Wv] projection of a self-attention, model/attention.py:170-178): the columns n >= vt_col0 are
 *            not stored at out[m][n] but TRANSPOSED and scaled by vt_alpha instead of alpha, exactly as edtr_igemm's vt_out:
 *            vt_out[(m / rows_per_image) * (N - vt_col0) + (n - vt_col0)][m % rows_per_image], row stride vt_ld, 16-bit (cvec applies to
 *            all columns).  Needs vt_col0 % 64 == 0, rows_per_image % 32 == 0, M % rows_per_image == 0, no residual; ldo >= vt_col0.
 *   gn_table optional (`proj_in(norm(x))`, model/attention.py:283-296): fp32 [M / rows_per_image][320][2] = (scale, shift) per image and
 *            channel, as edtr_gn_table writes it; the rows become x * scale + shift rounded to 16 bits in registers — the edtr_gn_apply launch
 *            in front of the projection is gone.  Not together with ln; rows_per_image % 128 == 0, M % rows_per_image == 0.
 * Needs K == 320, M % 128 == 0, N % 64 == 0, N <= 1024; anything else is EDTR_E_UNSUPPORTED (edtr_lin320_plan answers without a
 * launch) and the caller issues the edtr_igemm form. */
typedef struct edtr_lin320_params {
    int32_t dtype;
    int32_t M, N, K;
    int32_t ln; float eps;
    float alpha;
    const void* x; int32_t ldx;
    const void* w;
    const float* cvec;
    const void* residual; int32_t ldr;
    void* out; int32_t ldo;
    void* vt_out; int32_t vt_col0; int32_t vt_ld; float vt_alpha; int32_t rows_per_image;
    const float* gn_table;
} edtr_lin320_params;

int edtr_lin320(const edtr_lin320_params* p, edtr_stream_t stream);
int edtr_lin320_plan(const edtr_lin320_params* p);      /* no HIP call: EDTR_OK or the error edtr_lin320 would return */

/* 3 x 3 / stride 1 / pad 1 convolution of a 64-channel NHWC image into <= 64 channels, persistent workgroups with the nine tap
 * matrices resident in LDS (ABI 8) — SwinIR's reconstruction tail at the pixel levels, where edtr_igemm's 128-column tiles are
 * half padding.  replaces: conv_up1 / conv_up2 / conv_up3 (behind `F.interpolate(scale_factor=2, mode="nearest")`), conv_hr and
 * conv_last with their LeakyReLUs and the `x / img_range + mean` of the output, reference model/swinir.py:878-886.
 *   x      : [B][SH][SW][ldx] 16-bit, 64 channels read; source size (SH, SW) = (H, W), or (H / 2, W / 2) when upsample2x != 0
 *            (output pixel (Y, X) then reads source pixel (Y >> 1, X >> 1) — the nearest-neighbour upsample is never stored)
 *   w      : 9 LDS images of 8192 bytes, tap t = 3 ky + kx: byte n*128 + ((c ^ ((n >> 1) & 7)) << 4) + 2 j = weight[n][8 c + j][ky][kx]
 *            (n < 64 output channels, zero rows above the real count; 64 input channels)
 *   bias   : fp32 [64];   out = act(alpha * conv + bias), act = EDTR_ACT_NONE or EDTR_ACT_LRELU (act_slope)
 *   out    : 16-bit [B][H][W][ldo] (64 channels written), or — out_nchw_f32 != 0 — fp32 [B][n_valid][H][W] (n_valid <= 4)
 * H % 16 == 0, W % 16 == 0; ldx % 8 == 0, ldo % 8 == 0; pointers 16-byte aligned. */
typedef struct edtr_conv64_params {
    int32_t dtype;
    int32_t B, H, W;
    int32_t upsample2x;
    const void* x; int32_t ldx;
    const void* w;
    const float* bias;
    int32_t act; float act_slope; float alpha;
    void* out; int32_t ldo;
    int32_t out_nchw_f32, n_valid;
} edtr_conv64_params;

int edtr_conv64(const edtr_conv64_params* p, edtr_stream_t stream);

/* The VAE decoder's last step in one launch (ABI 8): GroupNorm + SiLU + 3 x 3 / stride 1 / pad 1 convolution of a 128-channel NHWC
 * image into <= 4 channels, written as fp32 NCHW planes.  replaces: `self.conv_out(nonlinearity(self.norm_out(h)))`, reference
 * model/vae.py:553-560, and the NHWC -> NCHW of the result (model/cldm.py:136-156 returns NCHW).
 *   x        : [B][H][W][ldx] 16-bit, 128 channels read
 *   gn_table : fp32 [B][128][2] from edtr_gn_table (NULL: no normalisation, a plain convolution)
 *   w        : 9 LDS images of 8192 bytes, tap t = 3 ky + kx: byte n*256 + ((c ^ (n & 15)) << 4) + 2 j = weight[n][8 c + j][ky][kx]
 *              (n < 32 rows, zero above the real output channels; 128 input channels)
 *   bias     : fp32 [32];   out = alpha * conv + bias -> fp32 [B][n_valid][H][W]
 * H % 16 == 0, W % 16 == 0, ldx % 8 == 0, n_valid <= 4; pointers 16-byte aligned. */
typedef struct edtr_conv128_out_params {
    int32_t dtype;
    int32_t B, H, W;
    const void* x; int32_t ldx;
    const float* gn_table;
    const void* w;
    const float* bias;
    float alpha;
    void* out; int32_t n_valid;
} edtr_conv128_out_params;

int edtr_conv128_out(const edtr_conv128_out_params* p, edtr_stream_t stream);

/* Row softmax: fp32 scores [rows][cols] (ld_s) -> 16-bit probabilities [rows][cols] (ld_p); columns cols..cols_pad-1
 * of every output row are written as zeros (so the row can feed a GEMM whose K is padded to a multiple of 8).
 * replaces: the softmax inside F.scaled_dot_product_attention of the d=512 single-head VAE
 *           attention, reference model/vae.py:298. */
int edtr_softmax_rows(int dtype, const float* s, int64_t rows, int cols, int64_t ld_s, void* p,
                      int64_t ld_p, int cols_pad, edtr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Layout / elementwise helpers.
 * ---------------------------------------------------------------------------------------- */
/* Token + positional embedding of the CLIP text tower: out[row][:] = table[tokens[row]][:] + pos[row % L][:], 16-bit out
 * (rows = B*L, D % 8 == 0).  replaces: `self.model.token_embedding(text) + self.model.positional_embedding`, reference
 * model/clip.py:41-43. */
int edtr_embed_tokens(int dtype, const int64_t* tokens, const float* table, const float* pos, int rows, int L, int D,
                      int vocab, void* out, int ld, edtr_stream_t stream);
/* Zero `bytes` bytes (a multiple of 16, 16-byte aligned) with ONE kernel launch (hipMemsetAsync costs two tiny kernels per
 * node inside a hipGraph).  replaces: the implicit zero-initialisation of the reduction buffers that torch's
 * native_group_norm allocates per call (reference model/util.py:146-163 via nn.GroupNorm). */
int edtr_zero_bytes(void* ptr, int64_t bytes, edtr_stream_t stream);
/* Pixel-unshuffle front end of SwinIR: NCHW fp32 image [B][C][H][W] -> NHWC 16-bit tokens [B*(H/r)*(W/r)][ld] with
 * dst[row(b, y, x)][c*r*r + dy*r + dx] = (src[b][c][y*r+dy][x*r+dx] - sub[c]) * scale   (sub == NULL: 0);
 * columns C*r*r .. zero_pad_to-1 are written as zeros.  r in 1..8, H % r == 0, W % r == 0.
 * replaces: `(x - self.mean) * self.img_range` and nn.PixelUnshuffle (channel order c*r*r + dy*r + dx), reference
 * model/swinir.py:861 and :700-704. */
int edtr_pixel_unshuffle(int dtype, const float* src, int B, int C, int H, int W, int r, const float* sub, float scale,
                         void* dst, int ld, int zero_pad_to, edtr_stream_t stream);
/* NCHW fp32 [B][C][HW] -> NHWC 16-bit: dst[(b*HW+p)*ld + coff + c] = scale*src + shift; when
 * zero_pad_to > C the channels C..zero_pad_to-1 (relative to coff) are written as 0.
 * replaces: `.type(self.dtype)` + rearranges (model/controlnet.py:266-269; model/attention.py:292)
 * and the `*2-1` / `/scale_factor` scalings at the callers (demo.py:102; model/cldm.py:156). */
int edtr_nchw_to_nhwc(int dtype, const float* src, int B, int C, int64_t HW, void* dst, int ld,
                      int coff, int zero_pad_to, float scale, float shift, edtr_stream_t stream);
/* NHWC (16-bit, or fp32 when src_f32) -> NCHW fp32, first C channels, times scale. */
int edtr_nhwc_to_nchw(int dtype, const void* src, int src_f32, int B, int C, int64_t HW, int ld,
                      float* dst, float scale, edtr_stream_t stream);
/* out[r][c] = a[r][c] + b[r][c] over rows x C 16-bit elements with row strides lda/ldb/ldo (b == NULL: strided copy).
 * Writing straight into a column slice of a wider buffer is how the channel concat is made for free.
 * replaces: `hs.pop() + control.pop()`, `h += control.pop()` and the torch.cat of model/controlnet.py:31,35,37. */
int edtr_add(int dtype, const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows, int C,
             edtr_stream_t stream);
/* edtr_add on 16-bit tensors that also writes the per-slot column statistics of its result in edtr_igemm's gn_partial format (ABI 10):
 * gn_partial[(s * gn_ld + c) * 2 + {0, 1}] = sum / sum of squares over the slot's slot_rows rows (128, or 64 for 8 x 8 images) of column c,
 * of the fp32 sums before the 16-bit store — the skip + control half of the UNet decoder's concatenations (reference
 * model/controlnet.py:35-37), whose GroupNorm then needs no pass over the concatenated tensor (edtr_gn_stats).  rows % slot_rows == 0,
 * C % 32 == 0, gn_ld >= C; otherwise as edtr_add (b may be NULL: a copy). */
int edtr_add_stats(int dtype, const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows, int C,
                   float* gn_partial, int gn_ld, int slot_rows, edtr_stream_t stream);
/* The fp32-stream form of edtr_add that also writes the result's fp16 MIRROR out16[r * ld16 + c] (ABI 7; see edtr_igemm_params.out16):
 * the `hs.pop() + control.pop()` half of a decoder concat whose 1x1 skip convolution reads the mirror (model/controlnet.py:35-37,
 * model/unet.py:189).  C % 8 == 0. */
int edtr_add_mirror(const float* a, int lda, const float* b, int ldb, float* out, int ldo, void* out16, int ld16, int64_t rows, int C,
                    edtr_stream_t stream);
/* Sinusoidal timestep embedding [cos | sin] written as 16-bit rows of `dim` (even).
 * replaces: timestep_embedding, reference model/util.py:98-118. */
int edtr_timestep_embedding(int dtype, const int64_t* t, int B, int dim, void* out, int ld,
                            edtr_stream_t stream);
/* Spaced-sampler update on fp32 NCHW latents, n elements:
 *   pred_x0 = c_recip*x - c_recipm1*eps;  x_prev = coef1*pred_x0 + coef2*x + sigma*noise
 * replaces: utils/sampler.py:160-164,150-153,199-203 (sigma = sqrt(var) * [index != 0]). */
int edtr_sampler_update(const float* x, const float* eps, const float* noise, float c_recip,
                        float c_recipm1, float coef1, float coef2, float sigma, float* x_prev,
                        float* pred_x0, int64_t n, edtr_stream_t stream);
/* The same update with the step index read on the DEVICE (no host round trip for a caller that follows the reference
 * signature literally and hands p_sample a GPU `index` tensor, utils/sampler.py:189-204,311-312):
 *   coefs[n_steps][5] fp32 rows = (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1,
 *   posterior_mean_coef2, sqrt(posterior_variance) * [i != 0]);  image b of B uses row index[b] (clamped into the table). */
int edtr_sampler_update_indexed(const float* x, const float* eps, const float* noise, const int64_t* index,
                                const float* coefs, int n_steps, float* x_prev, float* pred_x0, int B,
                                int64_t per_image, edtr_stream_t stream);
/* DiagonalGaussianDistribution.sample() of the VAE posterior on the quant_conv output (model/distributions.py:24-41,
 * model/cldm.py:131-132):  out[b][c][p] = (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise[b][c][p]) * scale  with
 * mean = moments[(b*HW+p)*ld + c], logvar = moments[(b*HW+p)*ld + C + c] (fp32 NHWC rows of 2*C valid columns);
 * noise == NULL gives mode() * scale.  out / noise: NCHW fp32 [B][C][HW]. */
int edtr_gaussian_sample(const float* moments, int ld, const float* noise, float* out, int B, int C, int64_t HW,
                         float scale, edtr_stream_t stream);
/* out = a*x + b*y (fp32).  replaces: Diffusion.q_sample, model/gaussian_diffusion.py:80-84. */
int edtr_axpby(const float* x, const float* y, float a, float b, float* out, int64_t n,
               edtr_stream_t stream);
/* Diffusion.q_sample with per-image timesteps read on the device (no host round trip for a GPU-resident `t`):
 *   out[b][i] = tab_a[t[b]] * x[b][i] + tab_b[t[b]] * noise[b][i],  tab_a = sqrt_alphas_cumprod, tab_b = sqrt_one_minus_alphas_cumprod
 * (fp32 tables of n_tab entries, t clamped into the table).  replaces: extract_into_tensor + the two multiplies and the add,
 * reference model/gaussian_diffusion.py:34-37,80-84 as called with a device `t` at demo.py:107-108, main/det/test_edtr.py:127-128. */
int edtr_q_sample(const float* x, const float* noise, const int64_t* t, const float* tab_a, const float* tab_b,
                  int n_tab, float* out, int B, int64_t per_image, edtr_stream_t stream);

/* ---- Reproducible noise: a seeded per-image N(0, 1) stream evaluated inside the kernels that consume it ----------------------
 * The value an element receives is a pure function of (seed, image id, purpose, draw, element offset inside the image): not of
 * the batch the image travels in, its position there, or the number of devices that share a data set.  Normative definition
 * (edtr_amd/rng.py restates it in numpy; tests on both sides of this ABI rely on it):
 *   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; multipliers 0xD2511F53, 0xCD9E8D57,
 *   Weyl constants 0x9E3779B9, 0xBB67AE85, ten rounds)
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (e >> 2, draw, purpose, image_id)   four uint32 words; e = the element's offset inside its image (NCHW:
 *             (c*H + h)*W + w), image_id = the image's GLOBAL index (< 2^32), purpose = EDTR_NOISE_* below, draw = the sampler's
 *             table row `index` for EDTR_NOISE_STEP and 0 for the other purposes
 *   one call gives words x0..x3 and the normals of elements 4*(e>>2) + 0..3:
 *             u1 = ((x0 >> 8) + 1) * 2^-24,  u2 = (x1 >> 8) * 2^-24,  r = sqrt(-2 ln u1),  z0 = r cos(2 pi u2),  z1 = r sin(2 pi u2);
 *             z2, z3 the same from (x2, x3).  Both u are exact in fp32 and u1 is in (0, 1]: |z| <= sqrt(48 ln 2) = 5.77, no log(0).
 * Common to the entries below: `seed` by value; the ids either as a device array image_ids[B] (int64, each in [0, 2^32): a
 * captured launch is replayed for another batch by rewriting 8*B bytes) or, when image_ids == NULL, image_id_base + b.
 * per_image % 4 == 0 and 16-byte aligned tensors (EDTR_E_ALIGN otherwise: one lane owns one group of four elements).
 * Every fused form gives the bits of edtr_normal_fill followed by the tensor-noise entry it is named after. */
#define EDTR_NOISE_Q_SAMPLE 0   /* Diffusion.q_sample noise */
#define EDTR_NOISE_STEP 1       /* spaced-sampler step noise (draw = table row) */
#define EDTR_NOISE_X_T 2        /* x_T of SpacedSampler.sample() */
#define EDTR_NOISE_VAE 3        /* DiagonalGaussianDistribution.sample() of the VAE posterior */
/* out[b][0 .. per_image) = the stream of image b, fp32.  replaces: torch.randn((B, *x_size)), utils/sampler.py:245. */
int edtr_normal_fill(float* out, int B, int64_t per_image, uint64_t seed, const int64_t* image_ids, int64_t image_id_base,
                     int purpose, int64_t draw, edtr_stream_t stream);
/* edtr_q_sample with the noise operand replaced by the stream (EDTR_NOISE_Q_SAMPLE, draw 0). */
int edtr_q_sample_rng(const float* x, const int64_t* t, const float* tab_a, const float* tab_b, int n_tab, float* out, int B,
                      int64_t per_image, uint64_t seed, const int64_t* image_ids, int64_t image_id_base, edtr_stream_t stream);
/* edtr_sampler_update with the noise operand replaced by the stream (EDTR_NOISE_STEP, the given draw).
 * replaces: torch.randn_like(x) + the update, utils/sampler.py:199-203. */
int edtr_sampler_update_rng(const float* x, const float* eps, float c_recip, float c_recipm1, float coef1, float coef2,
                            float sigma, float* x_prev, float* pred_x0, int B, int64_t per_image, uint64_t seed,
                            const int64_t* image_ids, int64_t image_id_base, int64_t draw, edtr_stream_t stream);
/* edtr_sampler_update_indexed with the noise operand replaced by the stream; image b's draw is its (clamped) index[b], read on
 * the device like its coefficient row, so a replayed launch needs no new argument per step. */
int edtr_sampler_update_indexed_rng(const float* x, const float* eps, const int64_t* index, const float* coefs, int n_steps,
                                    float* x_prev, float* pred_x0, int B, int64_t per_image, uint64_t seed,
                                    const int64_t* image_ids, int64_t image_id_base, edtr_stream_t stream);
/* edtr_gaussian_sample with the noise operand replaced by the stream (EDTR_NOISE_VAE, draw 0); per_image = C * HW. */
int edtr_gaussian_sample_rng(const float* moments, int ld, float* out, int B, int C, int64_t HW, float scale, uint64_t seed,
                             const int64_t* image_ids, int64_t image_id_base, edtr_stream_t stream);

/* bf16 split-3 GEMM operand of a [rows][C] matrix (high-precision mode, see EDTR_F32_SPLIT): dst[rows][3*C] =
 * [hi | lo | hi] (pattern 0, the activation side) or [hi | hi | lo] (pattern 1, the weight side of an activation x activation
 * product).  src_dtype: EDTR_F32_SPLIT = fp32 source, EDTR_BF16 / EDTR_F16 = 16-bit source.  C, ld_src, ld_dst multiples of 8. */
int edtr_split3(int src_dtype, const void* src, int64_t rows, int C, int64_t ld_src, int pattern, void* dst, int64_t ld_dst,
                edtr_stream_t stream);
/* The general operand writer: dst[rows][parts*C] in the format `op_fmt` (EDTR_F32_SPLIT = bf16 [hi|lo|hi]; EDTR_F32_H1/H2/H3 =
 * fp16 [x] / [hi|lo] / [hi|lo|hi]) from an fp32 (src_dtype = any fp32-stream code) or 16-bit source. */
int edtr_split_operand(int src_dtype, const void* src, int64_t rows, int C, int64_t ld_src, int op_fmt, void* dst,
                       int64_t ld_dst, edtr_stream_t stream);
/* fp32 [rows][C] -> 16-bit [rows][C] with independent row strides (high-precision mode: the fp16 q / k / v^T operands of
 * edtr_flash_attn64 are cut from fp32 projection outputs).  C, ld_dst multiples of 8; ld_src multiple of 4. */
int edtr_cast16(int dst_dtype, const float* src, int64_t rows, int C, int64_t ld_src, void* dst, int64_t ld_dst,
                edtr_stream_t stream);
/* Gaussian-weighted overlap-add of one latent tile (fp32 NCHW):
 *   out[b][c][hi+y][wi+x] += tile[b][c][y][x] * wts[y][x];  count[...] += wts[y][x]
 * replaces: utils/common.py:415-424 (make_tiled_fn accumulation). */
int edtr_tile_accumulate(const float* tile, const float* wts, float* out, float* count, int B,
                         int C, int H, int W, int th, int tw, int hi, int wi, edtr_stream_t stream);
/* out = num / den elementwise (fp32).  replaces: utils/common.py:425. */
int edtr_divide(const float* num, const float* den, float* out, int64_t n, edtr_stream_t stream);
/* ---- The same overlap-add for ALL windows of a plane in one launch each (additive to ABI 10) --------------------------------------
 * Window table: n pairs (hi, wi), int32, table[2 k] = first row and table[2 k + 1] = first column of window k; every window is
 * th x tw.  As with edtr_image_desc the table comes twice: a HOST array the entry point checks everything on before anything is
 * launched, and a DEVICE array with the same values that the kernel reads.  Errors (nothing is launched): a NULL pointer
 * EDTR_E_NULL; a non-positive extent, n <= 0 or n > EDTR_TILE_WINDOWS_MAX, th > H, tw > W, a window outside the plane and — for the
 * blend — a pixel of the plane that no window covers EDTR_E_SHAPE; a pointer that is not 4-byte aligned EDTR_E_ALIGN.  Nothing needs
 * more than that: rows move as float4 where pitch, window start and pointers keep both sides 16-byte aligned, else element-wise. */
#define EDTR_TILE_WINDOWS_MAX 4096
/* dst [n * B][C][th][tw], window-major: entry k * B + b = src[b][:, hi_k : hi_k + th, wi_k : wi_k + tw] of src [B][C][H][W] (fp32):
 * the bytes of torch.cat of the window slices along dim 0.  float4 or scalar is decided per window on the device (wi_k % 4).
 * replaces: the per-window slicing x[..., hi:hi_end, wi:wi_end], utils/common.py:411. */
int edtr_tile_gather(const float* src, int B, int C, int H, int W, const int32_t* table_host, const int32_t* table, int n, int th,
                     int tw, float* dst, edtr_stream_t stream);
/* out [B][C][H][W] = sum_k tiles[k * B + b][c][y - hi_k][x - wi_k] * wts[y - hi_k][x - wi_k] / sum_k wts[...] over the windows k that
 * cover (y, x), walked in table order; tiles [n * B][C][th][tw] window-major, wts [th][tw].  Every output element is written once:
 * no count plane, no zero fill, no read-modify-write, no atomics.  The bits are those of zeroed out / count planes ->
 * edtr_tile_accumulate for k = 0 .. n - 1 -> edtr_divide (one fma per window onto a +0 numerator, one addition per window onto a
 * +0 denominator, one division).  replaces: utils/common.py:415-425. */
int edtr_tile_blend(const float* tiles, const float* wts, const int32_t* table_host, const int32_t* table, int n, int th, int tw,
                    float* out, int B, int C, int H, int W, edtr_stream_t stream);

/* Tiled VAE (reference utils/tilevae/tilevae.py:232-304, GroupNormParam): sums is [T][BG][2] fp64 holding, per tile,
 * the edtr_gn_stats result of each (image, group).  Replaces them IN PLACE by the pair that makes edtr_gn_apply use the
 * tile-pooled statistics: mean = sum_t weights[t]*mean_t, var = sum_t weights[t]*var_t (biased per-tile variances; the
 * between-tile spread of the means is ignored exactly as the reference does); counts[t] = elements per group of tile t. */
int edtr_gn_pool(double* sums, const float* weights, const float* counts, int T, int BG, edtr_stream_t stream);
/* dst[p][y][x] = src[p][y][x] for planes x rows x cols fp32 elements with independent plane / row strides (elements).
 * replaces: the tile slicing `z[:, :, y1:y2, x1:x2]` and crop_valid_region placement, utils/tilevae/tilevae.py:218-229,468,548. */
int edtr_copy3d_f32(const float* src, int64_t src_plane_stride, int64_t src_row_stride, float* dst,
                    int64_t dst_plane_stride, int64_t dst_row_stride, int planes, int rows, int cols,
                    edtr_stream_t stream);

/* One level of the wavelet colour fix on fp32 NCHW planes: low = blur3x3(in; dilation radius, replicate pad) and, when
 * high_accum != NULL, high_accum += in - low.  `low` must not alias `in`.
 * replaces: wavelet_blur / wavelet_decomposition, reference utils/common.py:99-133 (runs right after vae_decode). */
int edtr_wavelet_level(const float* in, float* low, float* high_accum, int planes, int H, int W, int radius,
                       edtr_stream_t stream);

/* ---- Images in, images out: the 8-bit boundary around the fp32 NCHW batches -----------------------------------------------------
 * The reference's callers start and end with 8-bit images (demo.py:79-90,165; main/seg/test_edtr.py:113-115,136; calculate_psnr_pt
 * in main/{cls,det,seg}/test_edtr.py).  Images here are interleaved HWC with `channels` == 3 (EDTR_E_UNSUPPORTED otherwise);
 * batches are fp32 NCHW [B][3][H][W].  Three exactness rules (edtr_amd/imageio.py restates each in numpy):
 *   resize   = Pillow's Image.resize(size, BICUBIC) bit for bit: 22-bit fixed-point coefficients, int32 accumulation from 1 << 21,
 *              clamp(acc >> 22, 0, 255), horizontal pass then vertical pass with a uint8 intermediate
 *   ingest   = float32(float64(v) / 255.0), read from a 256-entry table the host builds that way (no device division)
 *   emit     = trunc(clamp(x * 255 + 0.5, 0, 255)) with the product and the sum each rounded to fp32 (never an FMA); NaN gives 0
 * Rows are moved as dwords / float4 where the pitch keeps them aligned (w % 4 == 0, W % 4 == 0) and element by element otherwise:
 * no extent or pointer needs more than its natural alignment. */
/* src [in_h][in_w][3] -> dst [out_h][out_w][3], uint8.  Per output column x: h_bounds[2 x] = first source column, h_bounds[2 x + 1]
 * = n <= h_ksize taps, h_coefs[x * h_ksize + 0 .. n) their int32 coefficients; v_* the same per output row.  A pass whose extent
 * does not change is skipped and its tables may be NULL.  tmp: [in_h][out_w][3] bytes, needed when both passes run.  The windows
 * are forced inside the source on the device.  replaces: PIL.Image.resize(..., Image.BICUBIC), demo.py:80-84. */
int edtr_image_resize_u8(const uint8_t* src, int in_h, int in_w, int channels, uint8_t* dst, int out_h, int out_w,
                         const int32_t* h_bounds, const int32_t* h_coefs, int h_ksize, const int32_t* v_bounds,
                         const int32_t* v_coefs, int v_ksize, uint8_t* tmp, edtr_stream_t stream);
/* One source image [h][w][3] (uint8, or fp32 when src_f32 = 1: copied) into the top-left corner of slot b of batch [B][3][H][W];
 * the rest of the slot is zero (replicate = 0: F.pad mode 'constant') or repeats the last row / column (replicate = 1: mode
 * 'replicate').  table: fp32 [256] on the device (uint8 sources).  replaces: np.array(img) / 255.0 -> rearrange -> pad_if_smaller
 * -> pad_to_multiples_of, demo.py:85-90; F.pad(..., mode='replicate'), main/seg/test_edtr.py:113-115. */
int edtr_image_ingest(int src_f32, const void* src, int h, int w, int channels, float* batch, int b, int B, int H, int W,
                      int replicate, const float* table, edtr_stream_t stream);
/* The top-left h x w crop of image b of batch [B][3][H][W] -> dst [h][w][3] uint8 with the emit rule above.
 * replaces: res[:, :h0, :w0] -> torchvision save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8), demo.py:165. */
int edtr_image_emit(const float* batch, int b, int B, int channels, int H, int W, uint8_t* dst, int h, int w, edtr_stream_t stream);
/* ---- The same boundary for a whole ragged batch in a fixed number of launches --------------------------------------------------
 * One edtr_image_desc per image, B of them in a DEVICE array that the kernels read, and the same B in a HOST array that the entry
 * point checks its arguments on (and sizes the grid from) before anything is launched.  Layout (80 bytes, 8-byte aligned):
 *    0 src        uint8 [in_h][in_w][3] on the device, any byte alignment
 *    8 h_bounds  16 h_coefs   the horizontal pass's tables as edtr_image_resize_u8 takes them; NULL (both) when out_w == in_w
 *   24 v_bounds  32 v_coefs   the vertical pass's tables; NULL (both) when out_h == in_h
 *   40 tmp_offset  int64: where this image's horizontal result [in_h][out_w][3] starts in the shared scratch buffer `tmp`
 *   48 in_h  52 in_w  56 out_h  60 out_w  64 h_ksize  68 v_ksize  72 b (slot of the batch)  76 reserved (0)       all int32
 * The bits are those of the per-image entry points: slot b after edtr_image_resize_h_batch + edtr_image_resize_ingest_batch equals
 * edtr_image_resize_u8 followed by edtr_image_ingest, and edtr_image_emit_batch writes the bytes of edtr_image_emit.  Which passes
 * run and whether rows move as dwords is decided per image on the device (pitch and pointer alignment of that image); windows are
 * forced inside the source, and an image whose descriptor does not fit the slot / the scratch buffer is left alone by the kernels.
 * Errors (nothing is launched): channels != 3 EDTR_E_UNSUPPORTED; a NULL array, src, batch, table, a NULL table of a pass that is
 * needed or a NULL tmp with a horizontal pass EDTR_E_NULL; B <= 0 or > 65535, a non-positive extent or ksize, b outside [0, slots),
 * out_h > H, out_w > W, a horizontal result outside [0, tmp_bytes) EDTR_E_SHAPE; misaligned tables / batch EDTR_E_ALIGN. */
typedef struct edtr_image_desc {
    const uint8_t* src;
    const int32_t* h_bounds; const int32_t* h_coefs;
    const int32_t* v_bounds; const int32_t* v_coefs;
    int64_t tmp_offset;
    int32_t in_h; int32_t in_w; int32_t out_h; int32_t out_w;
    int32_t h_ksize; int32_t v_ksize;
    int32_t b; int32_t reserved;
} edtr_image_desc;
/* One launch: the horizontal pass of every image with out_w != in_w, src -> tmp + tmp_offset.  No launch when no image has one. */
int edtr_image_resize_h_batch(const edtr_image_desc* descs_host, const edtr_image_desc* descs, int B, int channels, uint8_t* tmp,
                              int64_t tmp_bytes, edtr_stream_t stream);
/* One launch: every image's vertical pass (from its horizontal result, or from src where none ran; no pass at all = a plain ingest)
 * -> the float32(v / 255.0) table -> slot b of batch [slots][3][H][W], the rest of the slot zero (replicate = 0) or the last row /
 * column repeated (replicate = 1), written by the same launch: no uint8 [out_h][out_w][3] intermediate and no memset.  Three float4
 * per lane where W % 4 == 0 and batch is 16-byte aligned, element by element otherwise. */
int edtr_image_resize_ingest_batch(const edtr_image_desc* descs_host, const edtr_image_desc* descs, int B, int channels,
                                   const uint8_t* tmp, int64_t tmp_bytes, float* batch, int slots, int H, int W, int replicate,
                                   const float* table, edtr_stream_t stream);
/* One launch: for i < n, the top-left h x w crop of image b of batch [B][3][H][W] -> dst + offset as uint8 [h][w][3] with the emit
 * rule; (b, h, w, offset) = table[4 i .. 4 i + 3], int64, on the device (table) and on the host (table_host: checked here).  Offsets
 * are the caller's, multiples of 4 (EDTR_E_ALIGN), crops inside [0, dst_bytes) and the slot (EDTR_E_SHAPE); bytes of dst that no
 * crop covers are not written. */
int edtr_image_emit_batch(const float* batch, int B, int channels, int H, int W, const int64_t* table_host, const int64_t* table,
                          int n, uint8_t* dst, int64_t dst_bytes, edtr_stream_t stream);
/* out[i] (fp64) = the sum of squared differences of images i of a and b ([B][3][H][W] fp32) over rows [crop_border, h_i -
 * crop_border) and columns [crop_border, w_i - crop_border), (h_i, w_i) = sizes[2 i], sizes[2 i + 1] (device int32, clamped to
 * H, W; NULL = H, W): over the three planes (y_channel = 0), or over the BT.601 luma (65.481 r + 128.553 g + 24.966 b + 16) / 255
 * formed in fp64 (y_channel = 1).  Accumulated in fp64 in an order fixed by the shapes: EDTR_SQDIFF_BLOCKS partial sums per image
 * (partials: fp64 [B][EDTR_SQDIFF_BLOCKS], overwritten), then one finishing workgroup; no atomics, equal bits on every run.  The
 * caller forms 10 log10(1 / (out / count + 1e-8)).  replaces: calculate_psnr_pt, utils/common.py:219-247. */
#define EDTR_SQDIFF_BLOCKS 64
int edtr_image_sqdiff(const float* a, const float* b, int B, int channels, int H, int W, const int32_t* sizes, int crop_border,
                      int y_channel, double* partials, double* out, edtr_stream_t stream);

/* ---- Low-quality inputs: blur -> resize -> Gaussian noise -> JPEG on the device (additive to ABI 10) -----------------------------
 * One stage of the reference's synthetic degradation (datasets/detection_cocov2.py:426-460; with a second resize back to the input
 * extent, datasets/detection.py:155-181) as four launches on fp32 NCHW batches [B][3][H][W] (`channels` == 3, EDTR_E_UNSUPPORTED
 * otherwise) — the layout edtr_image_ingest writes and edtr_image_emit reads.  Every result is a bit-exact function of its inputs:
 * each product, sum and quotient named below is ONE correctly rounded fp32 operation (fmul, fadd, fdiv; never an FMA) in the order
 * given, and edtr_amd/degrade.py repeats every kernel in numpy.  Common errors (nothing is launched): a NULL tensor EDTR_E_NULL; B
 * <= 0 or > 65535 or a non-positive extent EDTR_E_SHAPE; an extent above 2^24 EDTR_E_UNSUPPORTED; a tensor that is not 4-byte
 * aligned EDTR_E_ALIGN.  Per-image parameters come twice, as the image descriptors do: a HOST array that is checked here and a
 * DEVICE array with the same values that the kernel reads.  Poisson noise and USM sharpening are the entries of "second order" below;
 * the sinc filter is an ordinary edtr_degrade_filter2d launch whose taps the host builds (edtr_amd/degrade.py,
 * circular_lowpass_kernel).  Not provided: the training pair pool (queue_size > 0), which mixes images across batches. */
/* out[b][c][y][x] = sum over (ky, kx), ky major, of fmul(x[b][c][R(y + ky - k/2)][R(x + kx - k/2)], kernels[b][ky][kx]), accumulated
 * with fadd from 0.0f: a correlation (no flip, as F.conv2d) over F.pad(mode="reflect") borders, R(i) = -i below 0 and 2 (n - 1) - i
 * from n on (the edge sample is not repeated).  kernels: fp32 [n_kernels][k][k] on the device, n_kernels == B, or 1 = one kernel for
 * every image.  k odd, 3 <= k <= 41, k / 2 < min(H, W) (EDTR_E_SHAPE otherwise); out must not alias x (EDTR_E_UNSUPPORTED).  The
 * input tile with its halo and the taps are staged in LDS once per 32 x 32 output tile.  replaces: filter2D, datasets/utils.py:71-96. */
int edtr_degrade_filter2d(const float* x, float* out, int B, int channels, int H, int W, const float* kernels, int n_kernels, int k,
                          edtr_stream_t stream);
/* F.interpolate(x, size=(out_h, out_w), mode=..., align_corners=False, antialias=False) for the three modes the reference draws from.
 * Coordinates are ATen's area_pixel_compute_source_index in fp32: scale = fdiv((float)in, (float)out) (formed on the host),
 *   src(dst) = fadd(fmul(scale, fadd((float)dst, 0.5f)), -0.5f);   idx = min(floor(src), in - 1);   t = clamp(fadd(src, -idx), 0, 1)
 * NOTE F.interpolate(scale_factor=s) maps with 1/s instead of in/out unless recompute_scale_factor is set: the two differ whenever
 * in * s is not an integer, so this entry (and the Python layer) takes explicit output extents only.
 *   bilinear: src is first raised to 0; i1 = idx + (idx < in - 1); w0 = fadd(1, -t), w1 = t; per row r: fadd(fmul(w0x, p[r][x0]),
 *             fmul(w1x, p[r][x1])); out = fadd(fmul(w0y, row0), fmul(w1y, row1))
 *   bicubic:  A = -0.75; taps idx - 1 .. idx + 2, each clamped into [0, in - 1]; weights c2(t + 1), c1(t), c1(u), c2(u + 1) with
 *             u = fadd(1, -t), c1(v) = ((1.25 v - 2.25) v) v + 1, c2(v) = ((-0.75 v + 3.75) v - 6) v + 3 evaluated left to right;
 *             per row the four products are added left to right, then the four rows the same way
 *   area:     adaptive_avg_pool2d: rows [floor(oy in_h / out_h), ceil((oy + 1) in_h / out_h)), columns alike (integers); the window
 *             is added row-major from 0.0f and divided (fdiv) by its element count
 * mode outside EDTR_RESIZE_* EDTR_E_DTYPE; out must not alias x. */
#define EDTR_RESIZE_BILINEAR 0
#define EDTR_RESIZE_BICUBIC 1
#define EDTR_RESIZE_AREA 2
int edtr_degrade_resize(const float* x, float* out, int B, int channels, int in_h, int in_w, int out_h, int out_w, int mode,
                        edtr_stream_t stream);
/* out = clamp(fadd(x, fdiv(fmul(n, sigma[b]), 255)), 0, 1), or with rounds = 1 fdiv(clamp(rint(fmul(that sum, 255)), 0, 255), 255)
 * (rint: half to even, as torch.round), n from the stream of "Reproducible noise" with two further purposes: colour noise (gray[b] == 0)
 * is EDTR_NOISE_DEGRADE with per_image = 3 H W and e = (c H + y) W + x; grey noise (gray[b] == 1) is EDTR_NOISE_DEGRADE_GRAY with
 * per_image = H W and e = y W + x, one plane shared by the three channels.  `draw` = the number of the degradation stage; key, image
 * id and the ids' two forms as for every stream consumer.  H W % 4 != 0, or x / out / noise_out not 16-byte aligned: EDTR_E_ALIGN.
 * sigma (fp32 [B], in units of 1/255; finite and >= 0, EDTR_E_SHAPE) and gray (int32 [B]; 0 or 1, EDTR_E_DTYPE) come as host and device
 * arrays.  noise_out (optional, fp32 [B][3][H][W]) receives n itself.  out may alias x.  edtr_normal_fill does not serve these two
 * purposes.  replaces: add_gaussian_noise_pt with torch.randn, datasets/degradation.py:461-512. */
#define EDTR_NOISE_DEGRADE 4        /* colour noise of edtr_degrade_gaussian_noise (draw = stage) */
#define EDTR_NOISE_DEGRADE_GRAY 5   /* grey noise of edtr_degrade_gaussian_noise (draw = stage) */
int edtr_degrade_gaussian_noise(const float* x, float* out, float* noise_out, int B, int channels, int H, int W, const float* sigma_host,
                                const float* sigma, const int32_t* gray_host, const int32_t* gray, uint64_t seed, const int64_t* image_ids,
                                int64_t image_id_base, int64_t draw, int rounds, edtr_stream_t stream);
/* DiffJPEG(differentiable=False) with one quality per image, in one launch; a workgroup owns whole 16 x 16 MCUs (four luma and two
 * chroma blocks) and no intermediate plane reaches memory.  With p = fmul(x, 255) inside the image and 0 in the padding to multiples
 * of 16, m = the float32 values of the file's matrices, and every three-term sum added left to right:
 *   Y = r m00 + g m01 + b m02;  Cb = (r m10 + g m11 + b m12) + 128;  Cr alike;  chroma 2 x 2 mean = fmul(((a00 + a01) + a10) + a11, 0.25)
 *   d = sample - 128;  F[u][v] = fmul(scale[u][v], sum over (x, y), x major, of fmul(d[x][y], T[x][y][u][v])) from 0.0f, x = row
 *   q = rint(fdiv(F, tq)), tq = fmul(table[u][v], factor[b]): the TRANSPOSED luminance table for Y (as the file builds it), the
 *       chrominance table for Cb / Cr;   back: c = fmul(fmul(q, tq), alpha[u][v])
 *   sample' = fadd(fmul(0.25, sum over (u, v), u major, of fmul(c[u][v], T[p][q][u][v])), 128);  chroma repeated 2 x 2
 *   R = Y' 1 + (Cb' - 128) 0 + (Cr' - 128) 1.402, G and B with their rows;  out = fdiv(min(255, max(0, .)), 255), cropped to H x W
 * dct: fp32 [64][64] on the device, dct[x 8 + y][u 8 + v] = float32(cos((2 x + 1) u pi / 16) cos((2 y + 1) v pi / 16)) with the
 * product formed in fp64 (the caller builds it: no device cosine decides a bit); scale = float32(alpha alpha^T / 4), alpha = (1/sqrt 2,
 * 1, ..., 1).  quality_host: fp32 [B], each in (0, 100] (EDTR_E_SHAPE); factor: fp32 [B] on the device, quality_to_factor of it
 * evaluated in fp32 (5000 / q / 100 below 50, (200 - 2 q) / 100 from 50 on; quality 100 gives factor 0 and, as in the file, no finite
 * result).  coefs (optional): fp32 [B][ny + 2 nc][8][8] receives q — the ny = Hp/8 Wp/8 luma blocks in raster order, then the nc =
 * Hp/16 Wp/16 Cb blocks, then Cr (Hp, Wp the padded extents).  out may alias x.  replaces: DiffJPEG.forward, datasets/diffjpeg.py:450-492. */
int edtr_degrade_jpeg(const float* x, float* out, int B, int channels, int H, int W, const float* quality_host, const float* factor,
                      const float* dct, float* coefs, edtr_stream_t stream);

/* ---- Low-quality inputs, second order: Poisson noise and USM sharpening (additive to ABI 10) -----------------------------------------
 * What RealESRGANBatchTransform.__call__ (datasets/detection_cocov2.py:413-539) needs beyond the four launches above.  The same rule:
 * fmul / fadd / fdiv in the order given or integer arithmetic, restated in numpy by edtr_amd/degrade.py, the same common errors. */
/* Poisson noise by table inversion on the stream of "Reproducible noise".  Per image b, per element e:
 *   level  k = (int)clamp(rint(fmul(v, 255)), 0, 255), q = fdiv((float)k, 255); colour noise (gray[b] == 0): v = x[e], e = (c H + y) W + x
 *          of the [3][H][W] image; grey noise (gray[b] == 1): v = fadd(fadd(fmul(0.2989f, r), fmul(0.587f, g)), fmul(0.114f, b)) of
 *          the pixel (torchvision's rgb_to_grayscale), e = y W + x of the [H][W] plane, one value for the three channels
 *   count  = the number of distinct k over the image's [3][H][W] (colour) or over its grey plane (grey); vals = 2^ceil(log2(count)),
 *          formed in integers: one of 1, 2, ..., 256.  A first launch marks the levels in a presence bitmap per image (LDS atomics in
 *          a workgroup, vector atomic ORs into `levels`: int32 [B][16], words 0..7 colour, 8..15 grey; zeroed by this entry), the
 *          noise kernel popcounts it.  Nothing is read back.  counts_out (optional, int32 [B][2]) receives (colour count, grey count).
 *   u      = word x[e & 3] of Philox on the counter (e >> 2, draw, purpose, image id), purpose EDTR_NOISE_DEGRADE_POISSON (colour)
 *          or EDTR_NOISE_DEGRADE_POISSON_GRAY (grey); key, ids and draw as for edtr_degrade_gaussian_noise
 *   n      = lows[t][k] + #{ j < 255 : tables[t][k][j] <= u }, t = log2(vals), by an 8-step binary search of the non-decreasing row
 *   noise  = fadd(fdiv((float)n, (float)vals), -q);   out = clamp(fadd(x, fmul(noise, scale[b])), 0, 1), or with rounds = 1
 *          fdiv(clamp(rint(fmul(that sum, 255)), 0, 255), 255)
 * tables: uint32 [9][256][256] and lows: int32 [9][256] on the device, built by the caller in fp64 with + * / alone (so that every
 * host builds the same bits): for vals = 2^t and level k, lambda = (double)fmul(fdiv((float)k, 255), (float)vals); lo = max(0,
 * ceil(lambda) - 128); weights w[floor lambda] = 1, w[j] = (w[j - 1] lambda) / j upwards and w[j] = (w[j + 1] (j + 1)) / lambda
 * downwards; total = the sum of w[0 .. lo + 256] in index order; cdf_j = (the sum of w[0 .. lo + j] in index order) / total;
 * tables[t][k][j] = min(2^32 - 1, floor(cdf_j 2^32)).  A lambda = 0 row is all 0xffffffff.  The mass outside the 257-wide window is
 * below 1e-13, under the 2^-32 quantum.  scale (fp32 [B], finite and >= 0, EDTR_E_SHAPE) and gray (0 or 1, EDTR_E_DTYPE) come as host
 * and device arrays; H W % 4 != 0 or x / out / noise_out not 16-byte aligned EDTR_E_ALIGN; draw outside [0, 2^32) EDTR_E_SHAPE; rounds
 * outside {0, 1} EDTR_E_DTYPE.  noise_out (optional, fp32 [B][3][H][W]) receives `noise`.  out must not alias x (EDTR_E_UNSUPPORTED):
 * a grey lane reads all three channels.  replaces: add_poisson_noise_pt with torch.poisson, datasets/degradation.py:610-680. */
#define EDTR_NOISE_DEGRADE_POISSON 6        /* colour noise of edtr_degrade_poisson_noise (draw = stage) */
#define EDTR_NOISE_DEGRADE_POISSON_GRAY 7   /* grey noise of edtr_degrade_poisson_noise (draw = stage) */
int edtr_degrade_poisson_noise(const float* x, float* out, float* noise_out, int B, int channels, int H, int W, const float* scale_host,
                               const float* scale, const int32_t* gray_host, const int32_t* gray, const uint32_t* tables,
                               const int32_t* lows, int32_t* levels, int32_t* counts_out, uint64_t seed, const int64_t* image_ids,
                               int64_t image_id_base, int64_t draw, int rounds, edtr_stream_t stream);
/* Separable correlation over F.pad(mode="reflect") borders with one tap vector for rows and columns (fp32 [k] on the device):
 *   t[y'][x] = sum over kx of fmul(x[R(y')][R(x + kx - k/2)], taps[kx]), added with fadd from 0.0f in tap order, for every padded row y';
 *   out[y][x] = sum over ky of fmul(t[y + ky - k/2][x], taps[ky]), added the same way.
 * k odd, 3 <= k <= 63, k / 2 < min(H, W) (EDTR_E_SHAPE otherwise).  One launch: the 32 x 32 tile's patch with its halo and the rows-pass
 * intermediate live in LDS.  mask_out (optional, fp32 [B][3][H][W]) receives fmul(fabs(fadd(x, -out)), 255) > threshold ? 1 : 0.
 * Neither output may alias x or the other.  replaces: the two filter2D calls of USMSharp.forward, datasets/utils.py:110-116, whose
 * kernel is the outer product g g^T. */
int edtr_degrade_sepblur(const float* x, float* out, float* mask_out, int B, int channels, int H, int W, const float* taps, int k,
                         float threshold, edtr_stream_t stream);
/* sharp = clamp(fadd(x, fmul(weight, fadd(x, -blur))), 0, 1);  out = fadd(fmul(soft, sharp), fmul(fadd(1, -soft), x)).  All four fp32
 * [B][3][H][W]; out may alias any input.  weight finite (EDTR_E_SHAPE).  replaces: USMSharp.forward, datasets/utils.py:117-119. */
int edtr_degrade_usm_apply(const float* x, const float* blur, const float* soft, float* out, int B, int channels, int H, int W,
                           float weight, edtr_stream_t stream);

/* ---- Label maps: what sits between the restored image and a segmentation score (additive to ABI 10) ------------------------------
 * The reference's segmentation test goes on after the restoration (main/seg/test_edtr.py:139-174): logits -> argmax -> calculate_mat
 * against the ground-truth mask -> compute_iou, and convert2color for the PNG; its data sets resize, pad, crop and flip image and mask
 * together (datasets/segmentation.py:82-114, 207-215).  A label map here is uint8 [H][W] (255 = "ignore" by the reference's
 * convention), an image uint8 [h][w][3].  Every launch is an integer or gather function of its inputs: edtr_amd/labels.py restates
 * each in numpy and the kernels are tested against that by equality.  Rows move as dwords / float4 where the pitch and the base keep
 * them aligned and element by element otherwise, as in "Images in, images out": nothing needs more than its natural alignment. */
#define EDTR_LOGITS_F32 0
#define EDTR_LOGITS_F16 1
#define EDTR_LOGITS_BF16 2
#define EDTR_SEG_MAX_CLASSES 32
/* mat [n][n] (int64, device) += the confusion matrix of argmax(logits) against target; pred (optional, uint8 [B][H][W]) = the argmax.
 * logits: [B][n][H][W] contiguous, fp32 / fp16 / bf16 by logits_dtype (EDTR_LOGITS_*; 16-bit values are widened exactly).
 * target: uint8 [B][H][W].  sizes (optional): int32 [B][2] = (h, w): only the top-left h x w of image b is counted; passed on the host
 * (sizes_host: checked here) and on the device (sizes: read by the kernel), both or neither.
 *   argmax  torch's CPU rule: the lowest index among the NaN channels if there is one, else the lowest index among the maxima
 *           (-0.0 == 0.0 is a tie)
 *   count   a pixel inside sizes counts iff target < n (255 and every other value is ignored); it adds 1 to mat[target][argmax]
 *   pred    every pixel of every slot is written, counted or not
 * mat is ADDED to (the caller zeroes it: a data set accumulates without a host sync).  Integer sums: the result does not depend on
 * the grid or on the order.  One launch, capped at max_blocks workgroups (0: the default cap) and grid-strided; counts go to LDS
 * histograms and each workgroup adds its non-zero bins to mat once.
 * Errors (nothing is launched): NULL logits / target / mat, or only one of sizes_host / sizes EDTR_E_NULL; unknown logits_dtype
 * EDTR_E_DTYPE; B, n, H, W <= 0, max_blocks < 0 or a sizes_host entry outside [1, H] x [1, W] EDTR_E_SHAPE; n > EDTR_SEG_MAX_CLASSES
 * EDTR_E_UNSUPPORTED; logits not aligned to an element, sizes to 4 or mat to 8 bytes EDTR_E_ALIGN.
 * replaces: output.argmax(1) -> calculate_mat(mask, pred, n), main/seg/test_edtr.py:156-159, utils/segmentation.py:99-102. */
int edtr_seg_confusion(int logits_dtype, const void* logits, const uint8_t* target, int B, int n, int H, int W,
                       const int32_t* sizes_host, const int32_t* sizes, int64_t* mat, uint8_t* pred, int max_blocks,
                       edtr_stream_t stream);
/* edtr_seg_confusion on logits that are still at the network's stride: coarse [B][n][ih][iw] (contiguous, fp32 / fp16 / bf16) stands
 * for F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False), which is blended tile by tile on chip and never
 * stored.  target, sizes_host / sizes, mat (ADDED to), pred, max_blocks, the argmax and counting rules, "pred is written for every
 * pixel of every slot" and the error codes in their order are edtr_seg_confusion's; ih, iw <= 0 is EDTR_E_SHAPE like H, W.  Any
 * ih, iw, H, W >= 1: up-scaling, down-scaling, non-integer ratios.
 *   value   of plane c at (y, x), in fp32 with every product and sum rounded on its own (no FMA) — the bilinear branch of
 *           edtr_degrade_resize: scale = float(in) / float(out); src = max(fadd(fmul(scale, fadd(dst, 0.5)), -0.5), 0);
 *           i0 = min(floor(src), in - 1), i1 = i0 + (i0 < in - 1), t = clamp(fadd(src, -i0), 0, 1) per axis;
 *           top = fadd(fmul(1 - tx, v[y0][x0]), fmul(tx, v[y0][x1])), bot alike on row y1; value = fadd(fmul(1 - ty, top), fmul(ty, bot))
 *   16-bit  inputs are widened exactly, blended in fp32 and the blend is rounded to the input's type (nearest even) before the
 *           comparison, as F.interpolate on a 16-bit tensor hands it to argmax; fp32 input compares the fp32 blend
 * One launch: 256 lanes own a 16 x 64 tile of output pixels (a lane four consecutive pixels of a row); the (i0, i1, t) of the tile's
 * rows and columns are formed once, and the coarse patch they span, all n planes, is staged in LDS as fp32 (the planes of one coarse
 * position side by side, n padded to a multiple of 4: one 16-byte read brings four planes of a tap) while it fits 16 KiB — under
 * strong down-scaling the same arithmetic reads its taps from memory, with the same result.  A 16-bit blend is rounded once.
 * Workgroups stride over the tiles and add their histograms to mat once; integer sums: the result does not depend on the grid.
 * replaces: F.interpolate(x, size=input_shape, mode="bilinear", align_corners=False) -> argmax(1) -> calculate_mat,
 * model/deeplabv3.py:44-47, main/seg/test_edtr.py:156-159. */
int edtr_seg_confusion_coarse(int logits_dtype, const void* coarse, int B, int n, int ih, int iw, const uint8_t* target, int H, int W,
                              const int32_t* sizes_host, const int32_t* sizes, int64_t* mat, uint8_t* pred, int max_blocks,
                              edtr_stream_t stream);
/* Segmentation loss from coarse logits (additive to ABI 10): the loss every segmentation training script of the reference forms,
 *   F.cross_entropy(F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False), target, ignore_index=255),
 * forward and backward without the [B][n][H][W] tensor in either direction.  coarse [B][n][ih][iw] (contiguous, fp32 / fp16 / bf16 by
 * logits_dtype), target uint8 [B][H][W], n <= EDTR_SEG_CE_MAX_CLASSES.  edtr_amd/labels.py restates both launches in numpy
 * (coarse_cross_entropy_reference, coarse_cross_entropy_backward_reference); the launches differ from that only in expf / logf and in
 * the running form of the sum below.
 *   z_c     the value edtr_seg_confusion_coarse compares: seven rounded fp32 operations, then the rounding to a 16-bit input's type
 *   lse     m + logf(sum over c of expf(z_c - m)), m the maximum, c ascending, every step rounded to fp32; the launch takes the planes
 *           once with a running maximum, multiplying the sum so far by expf(old m - new m) where the maximum moves
 *   counts  a pixel counts iff target != ignore_index and target < n; n <= target != ignore_index is counted in counts[1] ("bad") and
 *           ignored, where torch raises (no launch here waits for the device).  ignore_index: any int (one outside [0, 255] ignores nothing)
 *   loss    float(sum of (lse - z_target) over the counted pixels / count), the sum in fp64: per 16 x 64 output tile (a lane's four pixels
 *           left to right, then a tree over the tile's 256 lanes), then over the tiles ascending.  count = 0 gives NaN, as torch does
 * edtr_seg_ce_forward writes lse (fp32 [B][H][W], every word: all the backward needs saved), loss (fp32 [1]) and counts (int64 [2] =
 * count, bad).  Two launches: the tile kernel (edtr_seg_confusion_coarse's tile, tables and staged patch; taps from memory where the
 * patch does not fit) writes one fp64 sum and two int32 counts per TILE into workspace (8-byte aligned, at least
 * edtr_seg_ce_workspace(B, H, W) = 16 bytes per tile; 0 for a non-positive extent), then one workgroup folds them in tile order.  No
 * atomics, no memset; no result depends on the grid (max_blocks caps it; 0: the default cap).
 * edtr_seg_ce_backward writes grad [B][n][ih][iw] in the logits' type, every element, zeros included: the exact adjoint of the rule
 * above scaled by g = grad_loss[0] / float(counts[0]), both read on the device.  A gather, one writer per word: a workgroup owns 8 x 8
 * coarse positions of an image and four of its planes; the output rows whose taps reach coarse row i are the contiguous range
 * [first y with i1 >= i, first y with i0 > i), found with the forward's own index functions, columns alike.  lse and the targets of
 * the tile's footprint are staged in LDS while it has at most 6144 pixels and 160 rows and columns (else read from memory: the same
 * result), each pixel's z_c is blended again by the forward's device function, and element (c, i, j) is
 *   acc = 0; for y ascending { r = 0; for x ascending, counted pixels only { e = fmul(fadd(expf(fadd(z_c, -lse)), -[c == target]), g);
 *   if (j0 == j) r = fadd(r, fmul(1 - tx, e)); if (j1 == j) r = fadd(r, fmul(tx, e)); }
 *   if (i0 == i) acc = fadd(acc, fmul(1 - ty, r)); if (i1 == i) acc = fadd(acc, fmul(ty, r)); }
 * in fp32, rounded once to a 16-bit type (torch rounds the upstream gradient to 16 bits first: a deliberate difference).  A clamped edge
 * puts both taps of an axis on one position: both weights land there, 1 - t first.  counts[0] = 0: every element +0.0.
 * Errors (nothing is launched): a NULL pointer EDTR_E_NULL; unknown logits_dtype EDTR_E_DTYPE; B, n, ih, iw, H, W <= 0, max_blocks < 0
 * or a workspace smaller than edtr_seg_ce_workspace EDTR_E_SHAPE; n > EDTR_SEG_CE_MAX_CLASSES or an extent above 2^24
 * EDTR_E_UNSUPPORTED; coarse / grad not aligned to an element, lse / loss / grad_loss to 4, workspace / counts to 8 bytes EDTR_E_ALIGN.
 * replaces: F.interpolate(x, size=input_shape, mode="bilinear", align_corners=False) -> F.cross_entropy(pred["out"], mask,
 * ignore_index=255) and its backward, model/deeplabv3.py:44-47, main/seg/train_edtr.py:213. */
#define EDTR_SEG_CE_MAX_CLASSES 256
int64_t edtr_seg_ce_workspace(int B, int H, int W);
int edtr_seg_ce_forward(int logits_dtype, const void* coarse, int B, int n, int ih, int iw, const uint8_t* target, int H, int W,
                        int ignore_index, float* lse, void* workspace, int64_t workspace_bytes, float* loss, int64_t* counts,
                        int max_blocks, edtr_stream_t stream);
int edtr_seg_ce_backward(int logits_dtype, const void* coarse, int B, int n, int ih, int iw, const uint8_t* target, int H, int W,
                         int ignore_index, const float* lse, const int64_t* counts, const float* grad_loss, void* grad,
                         int max_blocks, edtr_stream_t stream);
/* src [in_h][in_w][channels] -> dst [out_h][out_w][channels], uint8, channels 1 or 3 (EDTR_E_UNSUPPORTED otherwise):
 * dst (y, x) = src (y_idx[y], x_idx[x]) with the int32 tables y_idx [out_h] / x_idx [out_w] on the device.  The host builds them by
 * Pillow's accumulating rule (ImagingScaleAffine: xo = 0.5 s; idx[x] = (int)xo; xo += s, in double, s = in / out), which is not
 * floor((x + 0.5) in / out); the kernel forces every entry inside the source.
 * replaces: Image.resize(size, Image.NEAREST), datasets/segmentation.py:89,92,210. */
int edtr_label_resize_nearest(const uint8_t* src, int in_h, int in_w, int channels, uint8_t* dst, int out_h, int out_w,
                              const int32_t* y_idx, const int32_t* x_idx, edtr_stream_t stream);
/* src [h][w][channels] -> dst [H][W][channels], uint8, channels 1 or 3: dst (y, x) = src (y0 + y', x0 + x'), y' = H - 1 - y under vflip
 * (else y), x' = W - 1 - x under hflip (else x); a position outside the source gives the byte `fill` (0 for images, 255 for masks).
 * Pad, crop and both flips in one gather; no transposition.  hflip / vflip not 0 / 1 or fill outside [0, 255]: EDTR_E_DTYPE.
 * replaces: np.pad(..., 'constant'), center_crop_arr / random_crop_arr and augment's flips, datasets/segmentation.py:96-114. */
int edtr_label_window(const uint8_t* src, int h, int w, int channels, uint8_t* dst, int H, int W, int y0, int x0, int hflip,
                      int vflip, int fill, edtr_stream_t stream);
/* labels uint8 [B][H][W] -> dst uint8 [B][H][W][3] = palette[label], palette uint8 [256][3] on the device: the bytes save_image
 * writes for convert2color's mask (a colour c / 255 through the emit rule gives c back).
 * replaces: convert2color -> save_image, utils/segmentation.py:52-96, main/seg/test_edtr.py:170-174. */
int edtr_label_colorize(const uint8_t* labels, int B, int H, int W, const uint8_t* palette, uint8_t* dst, edtr_stream_t stream);

/* ---- Detection boxes: what sits between a detector and the boxes a user sees (additive to ABI 10) ---------------------------------
 * The reference's demo runs its detector on the restored image in three modes (demo.py:126-160) and merges the tiled mode's windows
 * with torchvision's batched_nms; the detector's head ends in RoIHeads.postprocess_detections (model/faster_rcnn.py:1187-1244).
 * Boxes are fp32 [n][4] in xyxy, 16-byte aligned; scores fp32 [n].  edtr_amd/boxes.py restates every launch in numpy: all arithmetic
 * is correctly rounded fp32 in the order written here (no contraction), so the restatements agree bit for bit except where expf
 * enters.  No launch waits on another workgroup and none uses an atomic: dependent phases are separate launches on the stream. */
#define EDTR_NMS_MAX_BOXES 32768
/* Non-maximum suppression, per label.  With key(s) the uint32 order of torch's sort (all NaN scores equal and largest, -0.0 == 0.0):
 *   order   rank(i) = #{j : key(s_j) > key(s_i)} + #{j < i : key(s_j) == key(s_i)}; order[rank(i)] = i   (stable, descending)
 *   walk    in that order: a candidate not yet suppressed is kept, and suppresses every LATER candidate j of the SAME label with
 *           inter / ((area_i + area_j) - inter) > iou_threshold, where area = (x2 - x1) * (y2 - y1),
 *           inter = max0(min(x2_i, x2_j) - max(x1_i, x1_j)) * max0(min(y2_i, y2_j) - max(y1_i, y1_j)), max(a, b) = a > b ? a : b,
 *           min(a, b) = a < b ? a : b, max0(d) = d > 0 ? d : 0 (0 / 0 = NaN suppresses nothing)
 *   keep    [max_out] int64: the kept indices into the input in walk order, the walk ending after max_out of them; the rest -1;
 *           *count (int32, device) = the number written
 * labels: NULL (one label), int32 [n] or, with labels_i64 = 1, int64 [n].  Workspaces: order int32 [n], mask uint64
 * [n][ceil(n / 64)] (neither needs zeroing).  Three launches: the counting rank (the j side tiled through LDS), one wave64 workgroup
 * per 64 x 64 block of the upper triangle of (row, column) in rank order whose lane r writes the 64-bit word of row r, and a
 * one-workgroup scan with the removed-set in LDS.
 * Errors: a NULL pointer but labels EDTR_E_NULL; n <= 0 or max_out <= 0 EDTR_E_SHAPE; n > EDTR_NMS_MAX_BOXES EDTR_E_UNSUPPORTED;
 * labels_i64 not 0 / 1 EDTR_E_DTYPE; boxes not aligned to 16 bytes, the others to their element EDTR_E_ALIGN.
 * replaces: torchvision.ops.batched_nms (its per-label form, _batched_nms_vanilla), demo.py:156, model/faster_rcnn.py:1235. */
/* The first launch of edtr_boxes_nms alone: order [n] (int32) = the stable descending argsort of scores by key, by counting — O(n^2)
 * comparisons, deterministic, no atomics.  n <= 0 EDTR_E_SHAPE, n > EDTR_NMS_MAX_BOXES EDTR_E_UNSUPPORTED. */
int edtr_boxes_rank(const float* scores, int n, int32_t* order, edtr_stream_t stream);
int edtr_boxes_nms(const float* boxes, const float* scores, const void* labels, int labels_i64, int n, float iou_threshold,
                   int32_t* order, uint64_t* mask, int64_t* keep, int max_out, int32_t* count, edtr_stream_t stream);
/* The candidate stage of postprocess_detections for one image: logits [P][C], regression [P][4 C], proposals [P][4] ->
 *   score   softmax over the C logits of a row (fp32; maximum and sum by wave reduction, expf)
 *   box     for every class c >= 1, BoxCoder.decode_single (model/util.py:702-743) in its order: w = x2 - x1, cx = x1 + 0.5 w;
 *           dx = r0 / wx, dw = min(r2 / ww, xform_clip); pcx = dx w + cx, pw = expf(dw) w; x1' = pcx - 0.5 pw, x2' = pcx + 0.5 pw
 *           (y alike); then clamped to [0, img_w] / [0, img_h]
 *   flag    score > score_thresh && x2' - x1' >= min_size && y2' - y1' >= min_size
 * out_boxes / out_scores / out_labels (int32, = c) receive the flagged candidates in candidate-index order p (C - 1) + (c - 1), and
 * *count (int32, device) their number.  weights: four floats on the HOST (wx, wy, ww, wh; non-zero).  Workspaces: cand_boxes
 * [P (C - 1)][4], cand_scores and flags (bytes) [P (C - 1)], block_counts int32 [ceil(P / 4)]; the outputs hold up to P (C - 1) rows.
 * Three launches: one wave per proposal row, a one-workgroup prefix sum of the per-workgroup counts, the ordered scatter.
 * Errors: NULL EDTR_E_NULL; P <= 0, C < 2, a zero or NaN weight EDTR_E_SHAPE; P C > 2^24 EDTR_E_UNSUPPORTED; regression, proposals
 * and the box outputs not aligned to 16 bytes EDTR_E_ALIGN.
 * replaces: F.softmax, BoxCoder.decode, clip_boxes_to_image, torch.where, remove_small_boxes, model/faster_rcnn.py:1199-1232. */
int edtr_boxes_candidates(const float* logits, const float* regression, const float* proposals, int P, int C, float img_h, float img_w,
                          float score_thresh, float min_size, const float* weights, float xform_clip, float* cand_boxes,
                          float* cand_scores, uint8_t* flags, int32_t* block_counts, float* out_boxes, float* out_scores,
                          int32_t* out_labels, int32_t* count, edtr_stream_t stream);
/* One window of the tiled mode: the boxes with score >= score_min (a NaN score fails), in their order, shifted by (dx, dy), appended
 * to out_boxes / out_scores / out_labels (int32) at row *offset (int32, device), which is moved on; nothing is written at or past
 * row `capacity`.  labels int64 [n].  One workgroup; the running offset stays on the device, so a loop over windows needs no host sync.
 * replaces: the score filter, move_boxes and the three torch.cat of demo.py:143-155, utils/detection.py:687-692. */
int edtr_boxes_filter_shift(const float* boxes, const float* scores, const int64_t* labels, int n, float score_min, float dx, float dy,
                            float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* offset, int capacity,
                            edtr_stream_t stream);
#define EDTR_BOX_SHIFT 1
#define EDTR_BOX_MUL 2
#define EDTR_BOX_DIV 4
#define EDTR_BOX_CLIP 8
/* dst = src with, in this order and each only under its flag: x += dx, y += dy; x *= fx, y *= fy (or x /= fx, y /= fy); x clamped to
 * [0, clip_w], y to [0, clip_h].  dst may be src.  Unknown flag bits, or MUL and DIV together: EDTR_E_DTYPE.
 * replaces: move_boxes, resize_boxes (model/faster_rcnn.py:2558-2571), boxes /= scale (demo.py:135), clip_boxes_to_image. */
int edtr_boxes_transform(const float* src, float* dst, int n, int flags, float dx, float dy, float fx, float fy, float clip_w,
                         float clip_h, edtr_stream_t stream);
/* F.interpolate(scale_factor=s, mode="bilinear", align_corners=False) of fp32 [planes][ih][iw] -> [planes][oh][ow]: the source
 * coordinate of output o is max(fma(rscale, o + 0.5, -0.5), 0) with rscale = fp32(1 / s) — torch's rule when a scale factor is given,
 * where edtr_degrade_resize uses in / out — and the caller's oh = floor(ih s), ow = floor(iw s).  The product and the sum of the
 * coordinate are ONE rounding, as in torch's builds, which contract them; the weights and the four products are those of
 * edtr_degrade_resize's bilinear mode, each rounded.  rscale_h / rscale_w not positive: EDTR_E_SHAPE.
 * replaces: demo.py:132. */
int edtr_boxes_bilinear_scale(const float* src, float* dst, int planes, int ih, int iw, int oh, int ow, float rscale_h, float rscale_w,
                              edtr_stream_t stream);

/* ---- Detection scores: COCO matching into a running record, for mAP with no host sync in the loop (additive to ABI 10) --------------
 * The reference's detection test hands every image's detections to CocoEvaluator.update (main/det/test_edtr.py:138-190,
 * utils/detection.py:422-480) and reports mAP@[0.5:0.95] and mAP@0.5.  One call here is COCOeval.evaluateImg for one image, every
 * label, IoU threshold and area range at once; accumulate and summarize run on the host from one copy at the end
 * (edtr_amd/coco.py, which restates the launch in numpy: the normative rule is written out there).
 * Detections: boxes fp32 [n][4] xyxy (16-byte aligned), scores fp32 [n], labels; with `count` (int32, device, the form the max_out
 * launches return) rows at or past *count do not exist and are never read.  Ground truth: boxes fp32 [g][4], labels, area fp32 [g],
 * crowd uint8 [g].  labels: int32, or int64 with labels_i64 = 1, for both.  thresholds: fp64 [n_thr] on the device; areas: fp64
 * [4][2] = (lo, hi) per range, on the device.
 *   coordinates  w = x2 - x1 and h = y2 - y1 in fp32; everything after in fp64, each operation rounded (no contraction)
 *   IoU          iw = min(dx + dw, gx + gw) - max(dx, gx), ih alike; 0 if iw <= 0 or ih <= 0; else i = iw ih, u = da for a crowd and
 *                (da + ga) - i otherwise with da = dw dh, ga = gw gh; iou = i / u
 *   rank         per label, by the key of edtr_boxes_rank descending, equal keys by index; ranks 0 .. 99 are matched
 *   ground truth ignored in range a iff crowd or area outside [lo_a, hi_a]; walked not-ignored first, then ignored, each in input order
 *   walk         per (t, a), detections in rank order: best = min(thr_t, 1 - 1e-10), m = none; for each ground truth in order: skip it if
 *                matched at this (t, a) and no crowd; stop if m is not ignored and this one is; skip it if iou < best; else best = iou,
 *                m = this (an equal IoU moves m on).  A matched detection takes m's ignore flag and marks m; an unmatched one is
 *                ignored iff its own area da lies outside [lo_a, hi_a].
 * Detection records (structure of arrays, `capacity` rows), row *det_offset + i for detection i: image = image_id; label, or -1
 * outside [0, n_labels); score; rank within (image, label), -1 for label -1; match and ignore: bit 4 t + a, both zero for rank >= 100
 * and for label -1.  Ground-truth records (`gt_capacity` rows), row *gt_offset + j: image, label (or -1), ignore: bit a.
 * Both offsets (int32, device) are moved on by a dependent one-workgroup launch, by the rows that exist and by g; nothing is written
 * at or past a capacity, and the offset moves on all the same, so the host sees an overflow after its one copy.
 * Two launches: one wave64 workgroup per label (ballot compaction and a counting rank in LDS, one row of IoUs per detection, lane
 * 4 t + a walking the ground truths with its own matched-set bits, the two ballots being the record words) plus one workgroup for the
 * fields that do not depend on the matching; then the offsets.  Every record word has exactly one writer: no atomics, no waiting
 * between workgroups.  n = 0 and g = 0 together launch nothing.
 * Errors: a NULL table, record or offset pointer, or a NULL input whose extent is positive, EDTR_E_NULL; n < 0, g < 0, n_labels <= 0,
 * n_thr <= 0 or a capacity <= 0 EDTR_E_SHAPE; n > EDTR_COCO_MAX_DET, g > EDTR_COCO_MAX_GT, n_labels > EDTR_COCO_MAX_LABELS, n_thr >
 * EDTR_COCO_MAX_THRESHOLDS or a capacity > 2^30 EDTR_E_UNSUPPORTED; labels_i64 not 0 / 1 EDTR_E_DTYPE; boxes not aligned to 16 bytes,
 * the others to their element EDTR_E_ALIGN.
 * replaces: CocoEvaluator.update -> COCOeval.evaluateImg, maskUtils.iou, convert_to_xywh (utils/detection.py:422-480, 576-578). */
#define EDTR_COCO_MAX_DET 1024
#define EDTR_COCO_MAX_GT 1024
#define EDTR_COCO_MAX_LABELS 256
#define EDTR_COCO_MAX_THRESHOLDS 10
#define EDTR_COCO_KEEP 100
int edtr_coco_match(const float* det_boxes, const float* det_scores, const void* det_labels, int n, const int32_t* count,
                    const float* gt_boxes, const void* gt_labels, const float* gt_area, const uint8_t* gt_crowd, int g, int labels_i64,
                    int n_labels, int image_id, const double* thresholds, int n_thr, const double* areas, int32_t* rec_image,
                    int32_t* rec_label, float* rec_score, int32_t* rec_rank, uint64_t* rec_match, uint64_t* rec_ignore,
                    int32_t* det_offset, int capacity, int32_t* gt_image, int32_t* gt_label, uint8_t* gt_ignore, int32_t* gt_offset,
                    int gt_capacity, edtr_stream_t stream);
/* The other half, COCOeval.accumulate and _summarizeDets, from the same record with no host sync and no record copy (csrc/coco_acc.hip;
 * edtr_amd/coco.py restates each launch in numpy: `accumulate`, `accumulate_order_reference`, `summarize_ordered_reference`).  The
 * host never learns a row count: grids are sized by `capacity`, and lanes and workgroups past min(*det_offset, capacity) leave.  Rows
 * at or past the capacity do not exist.  No device-wide atomic, no waiting between workgroups.
 * edtr_coco_accumulate_workspace: the bytes of `workspace` (16-byte aligned) that edtr_coco_order and edtr_coco_accumulate take for
 * these two arguments; host arithmetic only, 0 for arguments the two refuse.  Two buffers of 16 bytes per row of the capacity rounded
 * up to EDTR_COCO_ACC_TILE, and 16 bytes per label. */
#define EDTR_COCO_ACC_TILE 1024
#define EDTR_COCO_ACC_MAX_ROWS (1 << 22)
int64_t edtr_coco_accumulate_workspace(int capacity, int n_labels);
/* The order of accumulate: the rows with 0 <= label < n_labels and 0 <= rank < EDTR_COCO_KEEP, ascending by the composite key
 *   (label, score class, image, rank)
 * which is strict ((image, label, rank) is unique per row), so the result does not depend on how it is sorted.  The score class is
 * numpy's stable argsort of the negated fp64 score: a greater score first, +0.0 and -0.0 equal, +inf first, -inf last of the numbers,
 * every NaN after all of them and equal to each other (NOT the key of edtr_boxes_rank).  A stable sort of a filtered subsequence is
 * the subsequence of the stable sort, so this ONE order serves every (area range, maxDets, threshold).
 * order: int32 [capacity], of which the first *n_kept are written: row indices in key order.  seg_start: int32 [n_labels + 1], label
 * k's rows are order[seg_start[k] .. seg_start[k + 1]) and seg_start[n_labels] = *n_kept.  status: bit 0 iff *det_offset lies outside
 * [0, capacity].
 * 2 + ceil(log2(tiles)) launches, tiles = ceil(capacity / EDTR_COCO_ACC_TILE): each tile keyed (128 bits: the key and the row index)
 * and sorted in LDS, then merge passes between the two workspace buffers, one workgroup per tile of output with a merge-path split,
 * then the indices and the segment bounds (a binary search per label).  No pass has to be stable and nothing uses an atomic.
 * Errors: a NULL pointer EDTR_E_NULL; capacity <= 0, n_labels <= 0 or workspace_bytes too small EDTR_E_SHAPE; capacity >
 * EDTR_COCO_ACC_MAX_ROWS or n_labels > EDTR_COCO_MAX_LABELS EDTR_E_UNSUPPORTED; workspace not aligned to 16 bytes, the others to
 * their element EDTR_E_ALIGN; all before any launch.
 * replaces: the argsort(-dtScores, kind='mergesort') of COCOeval.accumulate, once instead of per (label, area range, maxDets). */
int edtr_coco_order(const int32_t* rec_image, const int32_t* rec_label, const float* rec_score, const int32_t* rec_rank,
                    const int32_t* det_offset, int capacity, int n_labels, void* workspace, int64_t workspace_bytes, int32_t* order,
                    int32_t* seg_start, int32_t* n_kept, int32_t* status, edtr_stream_t stream);
/* precision fp64 [10][101][n_labels][4][3] and recall fp64 [10][n_labels][4][3] (thresholds, recall thresholds, labels, area ranges,
 * maxDets 1 / 10 / 100), every element written, -1 where a (label, area range) has no ground truth that is not ignored: bit for bit
 * coco.accumulate's.  recall_thresholds: fp64 [101] on the device (linspace(0, 1, 101)).  Two launches: the ground truths that are
 * not ignored per (label, area range) by ballot into the workspace, then one wave64 workgroup per (label, area range, threshold)
 * that walks the label's segment of `order` once for the three maxDets.  With tp = match & ~ignore and fp = ~match & ~ignore, the
 * j-th true positive with fp_j false positives before it has P_j = j / ((fp_j + j) + 2^-52) and rc_j = j / npig in fp64;
 * precision[r] = max{P_j : rc_j >= recall_thresholds[r]}, 0 where there is none (precision only rises at a true positive, and the
 * reference's search lands on one), folded into 101 LDS bins by the number of thresholds rc_j reaches — from the division itself —
 * and finished by a suffix maximum; recall = J / npig.  status: bit 1 is set iff *gt_offset lies outside [0, gt_capacity].
 * Errors: as edtr_coco_order, with gt_capacity <= 0 EDTR_E_SHAPE, gt_capacity > 2^30 EDTR_E_UNSUPPORTED and the fp64 and uint64
 * arrays aligned to 8 bytes.
 * replaces: COCOeval.accumulate (utils/detection.py:462-478 -> pycocotools). */
int edtr_coco_accumulate(const int32_t* order, const int32_t* seg_start, const uint64_t* rec_match, const uint64_t* rec_ignore,
                         const int32_t* rec_rank, int capacity, const int32_t* gt_label, const uint8_t* gt_ignore,
                         const int32_t* gt_offset, int gt_capacity, int n_labels, const double* recall_thresholds, void* workspace,
                         int64_t workspace_bytes, double* precision, double* recall, int32_t* status, edtr_stream_t stream);
/* The 12 statistics of COCOeval._summarizeDets into out[0 .. 12) (fp64), and *status as an int64 into the 8 bytes of out[12], so that
 * one copy of 104 bytes fetches both.  Each is the mean of its entries > -1, or -1 without any, summed in an order that depends on the
 * shape alone (coco.summarize_ordered_reference): per (threshold, label) over the recall thresholds in index order, then over the
 * thresholds, then over the labels, each from 0; one division by the count.  One launch of 12 workgroups.
 * Errors: a NULL pointer EDTR_E_NULL; n_labels <= 0 EDTR_E_SHAPE; n_labels > EDTR_COCO_MAX_LABELS EDTR_E_UNSUPPORTED; the fp64
 * arrays not aligned to 8 bytes or status to 4 EDTR_E_ALIGN.
 * replaces: COCOeval.summarize -> _summarizeDets (utils/detection.py:462-478 -> pycocotools). */
int edtr_coco_summarize(const double* precision, const double* recall, int n_labels, const int32_t* status, double* out,
                        edtr_stream_t stream);

/* ---- Classification: top-k rank, feature distance and the data set's geometry, with no host sync in the loop (additive to ABI 10) ---
 * The reference's classification test normalises the restored batch for its classifier, scores calculate_accuracy(pred, label,
 * topk=(1, 5)) and, with --calc-fd, F.l1_loss(feat_res, feat_gt, reduction='none').mean(dim=(1, 2, 3)) (main/cls/test_edtr.py:127-162,
 * utils/classification.py:45-61); its data set crops, flips and transposes the ground truth (datasets/classification.py:65-96).
 * edtr_amd/cls.py restates every launch in numpy and writes the rules out; the kernels are tested against it by equality.  Records are
 * structures of arrays that a running pair of offsets (int32 [2] on the device: images, batches) appends to; nothing is written at or
 * past a capacity, and the offsets move on all the same, so the host sees an overflow after its one copy.  Every output word has
 * one writer: no atomics, no waiting between workgroups. */
#define EDTR_CLS_MAX_CLASSES 65536
#define EDTR_CLS_MAX_KEEP 8
#define EDTR_CLS_MAX_TOPK 4
#define EDTR_CLS_FD_CHUNK 4096
#define EDTR_CLS_FD_MAX_ELEMS (1 << 28)
/* The order behind topk for every row of logits [B][C] (fp32 / fp16 / bf16 by logits_dtype, EDTR_LOGITS_*; 16-bit values are widened
 * exactly).  With key(v) the uint32 key of edtr_boxes_rank (every NaN one largest key, -0.0 and 0.0 one key):
 *   order   class j precedes class i iff key(v_j) > key(v_i), or the keys are equal and j < i
 *   rank    rec_rank[row] = the number of classes that precede class labels[b]; C when labels[b] lies outside [0, C)
 *   top     rec_top[row K + m], m < K = the class with exactly m predecessors; -1 for m >= C
 *   label   rec_label[row] (optional) = labels[b]
 * with row = *offset + b (offset: int32 on the device, or NULL for 0); a row at or past `capacity` is not written.  labels (int32 [B],
 * device) may be NULL: rank and label are then not written (the argmax of 2-D targets is this launch with K = 1).  On rows without
 * equal keys the order is torch.topk(K, 1, True, True)'s, whose order among equal values is unspecified; torch's CPU max / argmax
 * (the first NaN, else the first maximum) is top[., 0].  One launch, one wave64 workgroup per row: the predecessors of the label by
 * ballot and popcount, the K places by K rounds of a wave-wide (greatest key, least index) selection below the place taken last.
 * Errors: NULL logits, labels without rec_rank or K > 0 without rec_top EDTR_E_NULL; B, C, capacity <= 0, K < 0, or neither labels nor
 * K EDTR_E_SHAPE; B > 65535, C > EDTR_CLS_MAX_CLASSES, K > EDTR_CLS_MAX_KEEP, capacity > 2^30 EDTR_E_UNSUPPORTED; unknown logits_dtype
 * EDTR_E_DTYPE; a pointer not aligned to its element EDTR_E_ALIGN.
 * replaces: output.topk(maxk, 1, True, True), pred.eq(target[None]), target.max(dim=1)[1], utils/classification.py:50-55. */
int edtr_cls_rank(int logits_dtype, const void* logits, const int32_t* labels, int B, int C, int K, int32_t* rec_label,
                  int32_t* rec_rank, int32_t* rec_top, const int32_t* offset, int capacity, edtr_stream_t stream);
/* partials [B][chunks] (fp64, device; chunks = ceil(n / EDTR_CLS_FD_CHUNK)) = the chunk sums of |a - b| over the n elements of
 * every image of a, b [B][n] (fp32 / fp16 / bf16 by dtype, EDTR_LOGITS_*).  Each difference is formed in fp32 — widen, subtract,
 * fabsf — and added in fp64 in an order that depends on n alone: one 256-lane workgroup per (image, chunk), lane l adds elements l,
 * l + 256, ... of its chunk in that order, and the tree s = 128, 64, ..., 1 with sum[l] += sum[l + s] over the 256 lane sums gives
 * the partial.  edtr_cls_commit finalises.
 * Errors: NULL EDTR_E_NULL; B <= 0 or n <= 0 EDTR_E_SHAPE; B > 65535 or n > EDTR_CLS_FD_MAX_ELEMS EDTR_E_UNSUPPORTED; unknown dtype
 * EDTR_E_DTYPE; a, b not aligned to an element or partials to 8 bytes EDTR_E_ALIGN.
 * replaces: F.l1_loss(feat_res, feat_gt, reduction='none').mean(dim=(1, 2, 3)), main/cls/test_edtr.py:153. */
int edtr_cls_fdist(int dtype, const void* a, const void* b, int B, int n, double* partials, edtr_stream_t stream);
/* The dependent one-workgroup launch that closes a batch of B images whose ranks lie at rows offsets[0] ... of rec_rank:
 *   batch row  batch_n[offsets[1]] = B; batch_correct[offsets[1] n_topk + t] = #{rows of the batch : rank < topk_host[t]}
 *   fd         rec_fd[row] = fp32(sum of the image's partials in chunk order in fp64 / n in fp64); NaN with partials NULL
 *   batch      rec_batch[row] = offsets[1]
 *   offsets    offsets[0] += B, offsets[1] += 1
 * topk_host: n_topk <= EDTR_CLS_MAX_TOPK ints on the HOST, each in [1, EDTR_CLS_MAX_KEEP]; n_topk = 0 counts nothing (rec_rank,
 * topk_host and batch_correct may then be NULL).  Rows at or past `capacity` / `batch_capacity` are not written or counted.
 * Errors: a NULL record, batch or offsets pointer EDTR_E_NULL; B, a capacity <= 0, n_topk < 0, a topk entry <= 0, or partials with
 * n <= 0 EDTR_E_SHAPE; B > 65535, n_topk > EDTR_CLS_MAX_TOPK, a topk entry > EDTR_CLS_MAX_KEEP, a capacity > 2^30 or n >
 * EDTR_CLS_FD_MAX_ELEMS EDTR_E_UNSUPPORTED; a pointer not aligned to its element EDTR_E_ALIGN.
 * replaces: correct[:k].flatten().sum(), utils/classification.py:57-60, and the list appends of main/cls/test_edtr.py:151-153. */
int edtr_cls_commit(const int32_t* rec_rank, float* rec_fd, int32_t* rec_batch, int B, const double* partials, int n,
                    const int32_t* topk_host, int n_topk, int32_t* batch_n, int32_t* batch_correct, int32_t* offsets, int capacity,
                    int batch_capacity, edtr_stream_t stream);
/* out = (x - mean_c) / std_c on fp32 [B][3][H][W], the subtraction and the division each correctly rounded: torchvision's Normalize
 * (sub_ then div_) with fp32 constants.  mean_host / std_host: three floats each on the HOST.  out may be x.  Errors: those of every
 * fp32 batch ("Low-quality inputs"); NULL constants EDTR_E_NULL; a NaN constant or a zero std EDTR_E_SHAPE.
 * replaces: Normalize / inv_normalize, model/resnet.py:17-27, 293-294. */
int edtr_cls_normalize(const float* x, float* out, int B, int channels, int H, int W, const float* mean_host, const float* std_host,
                       edtr_stream_t stream);
/* edtr_label_window plus the transpose.  crop (r, c) = src (y0 + r, x0 + c) for r < H, c < W, `fill` outside src [h][w][channels]
 * (uint8, channels 1 or 3); then both flips on the crop's indices, then the transpose:
 *   transpose 0  dst [H][W]:  dst (y, x) = crop (y', x'),  y' = H - 1 - y under vflip, x' = W - 1 - x under hflip
 *   transpose 1  dst [W][H]:  dst (y, x) = crop (x', y'),  x' = H - 1 - x under vflip, y' = W - 1 - y under hflip
 * One gather; with the transpose a 32 x 32 tile goes through LDS so that reads and writes both run along rows.  Errors: as
 * edtr_label_window; transpose not 0 / 1 EDTR_E_DTYPE.
 * replaces: center_crop_arr / random_crop_arr and augment (both flips, then img.transpose(1, 0, 2)), datasets/classification.py:82-93,
 * datasets/augment.py:57-68. */
int edtr_cls_window(const uint8_t* src, int h, int w, int channels, uint8_t* dst, int H, int W, int y0, int x0, int hflip, int vflip,
                    int transpose, int fill, edtr_stream_t stream);

/* ---- Region proposals and RoI pooling: the non-learned steps inside the detector (additive to ABI 10) -------------------------------
 * The reference's Faster R-CNN (model/faster_rcnn.py) runs, between its learned parts, AnchorGenerator.forward (:514-589),
 * RegionProposalNetwork.filter_proposals (:2068-2134, 2199-2213) and MultiScaleRoIAlign, the last two through compiled torchvision
 * operators.  edtr_amd/rois.py restates every launch in numpy and writes the rules out; the launches equal the restatements bit for bit
 * except where expf (decoding, sigmoid) and log2f (the level of a roi) enter.  The RPN head's outputs are read as the head wrote them:
 * per level l, objectness [N][A_l][H_l][W_l] and deltas [N][4 A_l][H_l][W_l] (channel 4 a + c), fp32 / fp16 / bf16 by dtype
 * (EDTR_LOGITS_*; 16-bit values are widened exactly).  The LOGICAL index of an element of a level is i = (y W + x) A + a, the row
 * concat_box_prediction_layers would have moved it to.  levels_host: int32 [L][5] on the HOST = H, W, A, stride_h, stride_w per level;
 * objectness_host / deltas_host / features_host: L device pointers in a HOST array; cells: fp32 [sum A_l][4] on the device, the cell
 * anchors of every level in level order.  Every output word has one writer; no global and no floating-point atomics.
 * Common errors (nothing is launched): a NULL pointer EDTR_E_NULL; L, N, pre_nms_top_n, H, W or A <= 0, a negative stride
 * EDTR_E_SHAPE; L > EDTR_RPN_MAX_LEVELS, pre_nms_top_n > EDTR_RPN_MAX_PRE_NMS, H W A >= 2^24, H stride_h or W stride_w >= 2^24,
 * N > 65535 EDTR_E_UNSUPPORTED; unknown dtype EDTR_E_DTYPE; cells and boxes not aligned to 16 bytes, the others to their element
 * EDTR_E_ALIGN. */
#define EDTR_RPN_MAX_LEVELS 8
#define EDTR_RPN_MAX_PRE_NMS 4096
#define EDTR_ROI_MAX_TAPS 64
/* anchors [sum H W A][4] (fp32): anchor i of a level = (float(x stride_w) + cell[a][0], float(y stride_h) + cell[a][1],
 * float(x stride_w) + cell[a][2], float(y stride_h) + cell[a][3]).  For callers and tests: the proposal launches form anchors from
 * the index and read no anchor tensor.
 * replaces: AnchorGenerator.grid_anchors, model/faster_rcnn.py:540-569. */
int edtr_rpn_anchors(const int32_t* levels_host, int L, const float* cells, float* anchors, edtr_stream_t stream);
/* selected [N][sum take_l] (int32), take_l = min(pre_nms_top_n, H_l W_l A_l): for every image and level the take_l level-local logical
 * indices of the greatest objectness, by the key of edtr_boxes_rank descending (every NaN first, -0.0 == 0.0), equal keys by ascending
 * logical index — torch.topk wherever torch defines the order.  One 1024-lane workgroup per (level, image): a radix select on the
 * 32-bit key (four 8-bit passes in memory order; histograms by integer adds in LDS) finds the threshold key and how many elements
 * equal to it to take, an ordered ballot compaction in logical order gathers them into LDS, and a counting rank there orders them.
 * replaces: permute_and_flatten, ob.topk(pre_nms_top_n, dim=1), model/faster_rcnn.py:2068-2077, 2231-2260. */
int edtr_rpn_select(int dtype, const void* const* objectness_host, const int32_t* levels_host, int L, int N, int pre_nms_top_n,
                    int32_t* selected, edtr_stream_t stream);
/* For every selected element, in level order and then selection order: the anchor from its index; BoxCoder.decode_single with weights
 * (1, 1, 1, 1) and xform_clip (the arithmetic of edtr_boxes_candidates); prob = 1 / (1 + expf(-logit)); the corners clamped to
 * [0, w] x [0, h] of image_sizes [N][2] (fp32 h, w on the device); kept iff x2 - x1 >= min_size && y2 - y1 >= min_size && prob >=
 * score_thresh.  boxes [N][sum take][4], probs and level (int32) [N][sum take] receive the kept ones of each image in order from its
 * row's start, counts [N] (int32) their number.  One workgroup per image, ordered ballot compaction.
 * replaces: BoxCoder.decode, the gathers by top_n_idx, torch.sigmoid, clip_boxes_to_image, remove_small_boxes and the score filter,
 * model/faster_rcnn.py:2105-2123, 2211. */
int edtr_rpn_candidates(int dtype, const void* const* objectness_host, const void* const* deltas_host, const int32_t* levels_host, int L,
                        int N, int pre_nms_top_n, const float* cells, const int32_t* selected, const float* image_sizes,
                        float xform_clip, float min_size, float score_thresh, float* boxes, float* probs, int32_t* level,
                        int32_t* counts, edtr_stream_t stream);
/* MultiScaleRoIAlign as one launch: out [K][C][P][P] (fp32) from features [N][C][H_l][W_l] per level (fp32 / fp16 / bf16 by dtype),
 * rois [K][4] (fp32 xyxy in image coordinates, 16-byte aligned) and batch_index [K] (int32: the image of each roi).
 *   level   with L > 1: s = sqrtf((x2 - x1) (y2 - y1)); t = floorf((canonical_level + log2f(s / canonical_scale)) + 1e-6f) clamped to
 *           [k_min, k_max] (NaN: k_min); level = t - k_min.  With L == 1 there is no mapper.
 *   pool    roi_align with aligned = False: the four coordinates times scales_host[level]; roi_w = max(x2 - x1, 1), bin_w = roi_w / P
 *           (h alike); sample (iy, ix) of bin (ph, pw): y = (y1 + ph bin_h) + ((iy + 0.5) bin_h) / S, x alike; a sample with y < -1,
 *           y > H, x < -1 or x > W adds nothing; else y = max(y, 0), y_low = (int)y, and y_low >= H - 1 gives y_low = y_high = H - 1,
 *           y = y_low, otherwise y_high = y_low + 1; ly = y - y_low, hy = 1 - ly (x alike); the sample is
 *           (((hy hx) v11 + (hy lx) v12) + (ly hx) v21) + (ly lx) v22, added to the sum with iy outer and ix inner; out = sum / (S S).
 *           Every step one rounded fp32 operation, no product contracted with a sum.
 * level_hw_host: int32 [L][2] and scales_host: fp32 [L], on the HOST.  One workgroup per (roi, 64 channels): the P S tap positions of
 * each axis go through LDS once, then a lane owns output elements in storage order.
 * Errors: NULL EDTR_E_NULL; a non-positive extent, scale or canonical_scale, or k_max - k_min != L - 1 with L > 1 EDTR_E_SHAPE;
 * L > EDTR_RPN_MAX_LEVELS, N > 65535, P S > EDTR_ROI_MAX_TAPS, an extent >= 2^24 EDTR_E_UNSUPPORTED; unknown dtype EDTR_E_DTYPE; rois
 * not aligned to 16 bytes, the others to their element EDTR_E_ALIGN.
 * replaces: torchvision.ops.MultiScaleRoIAlign (LevelMapper, roi_align), model/faster_rcnn.py:9. */
int edtr_roi_align(int dtype, const void* const* features_host, const int32_t* level_hw_host, const float* scales_host, int L, int N,
                   int C, const float* rois, const int32_t* batch_index, int K, int P, int S, int k_min, int k_max,
                   float canonical_scale, float canonical_level, float* out, edtr_stream_t stream);
/* The gradient of edtr_roi_align with respect to the features (the boxes get none, as in torchvision), deterministic: no atomics, no
 * memset, every output word written by one lane, every sum in a fixed order.  grad [K][C][P][P] (fp32) -> grads_out_host: L device
 * pointers in a HOST array, level l [N][C][H_l][W_l] in fp32 / fp16 / bf16 by dtype; every word of every level is written, +0.0 where no
 * roi reaches.  The other arguments are edtr_roi_align's; batch_index must not decrease (the rois of an image are one range of k).
 * For roi k the level, the image, the scaled box and the tap tables (valid, low, high, l, h of the P S positions per axis) are the
 * forward's, by the same device functions.  Every step below is one rounded fp32 operation, nothing contracted:
 *   g'[c][ph][pw] = grad[k][c][ph][pw] / (S S);
 *   a[y][ph]: from +0, for iy = 0 .. S - 1 in order, if tap (ph, iy) is valid: + hy if y_low == y, then + ly if y_high == y (at the
 *             clamped edge low == high and both are added: l = 0, h = 1 there); b[x][pw] alike on the other axis;
 *   t[ph] = sum_pw b[x][pw] g'[c][ph][pw], pw ascending from +0;  contrib_k[c][y][x] = sum_ph a[y][ph] t[ph], ph ascending from +0;
 *   out_l[n][c][y][x] = sum_k contrib_k over the rois of image n on level l, k ascending from +0, rounded ONCE to dtype (nearest even).
 * A term whose a or b is exactly zero is skipped, which changes no bit for finite gradients; a non-finite grad is unspecified.
 * Two launches.  Pre-pass, one 128-lane workgroup per roi: its record in the workspace (level, image, the footprint [ymin, ymax] x
 * [xmin, xmax] of its valid taps, both tap tables) and the first roi of every image.  Gather, one 256-lane workgroup per (image, level,
 * 16 x 16 pixel tile, EDTR_ROI_BWD_CHUNK channels): walks the image's rois 256 at a time, keeps those of its level whose footprint meets
 * the tile by an ordered ballot compaction (k ascending), stages g' of the chunk in LDS per kept roi, and every lane accumulates its
 * pixel's channels in registers.  workspace: 16-byte aligned, at least edtr_roi_align_backward_workspace(N, K, P, S) bytes, read by
 * nothing afterwards.
 * Errors: those of edtr_roi_align in its order, and P > EDTR_ROI_BWD_MAX_P (g' of a chunk must fit the LDS), more than 65535 chunks or
 * 2^31 tiles EDTR_E_UNSUPPORTED; grad not aligned to 4 bytes, workspace to 16 EDTR_E_ALIGN; a workspace too small EDTR_E_SHAPE.
 * replaces: the backward of torchvision.ops.roi_align (float atomicAdd, not repeatable) under `detnet(...)` + `backward()`,
 * main/det/train_edtr.py:228-241. */
#define EDTR_ROI_BWD_MAX_P 16
#define EDTR_ROI_BWD_CHUNK 32
int64_t edtr_roi_align_backward_workspace(int N, int K, int P, int S);
int edtr_roi_align_backward(int dtype, void* const* grads_out_host, const int32_t* level_hw_host, const float* scales_host, int L, int N,
                            int C, const float* rois, const int32_t* batch_index, int K, int P, int S, int k_min, int k_max,
                            float canonical_scale, float canonical_level, const float* grad, void* workspace, int64_t workspace_bytes,
                            edtr_stream_t stream);

/* ---- Detector input: normalise, resize and pad a ragged list of images in one launch (additive to ABI 10) -------------------------
 * GeneralizedRCNNTransform.forward in eval mode (model/faster_rcnn.py:2266-2435) from the point where every extent is known: the
 * caller works out each image's resized extent (oh, ow) and the padded extent (H, W) of the batch on the host, from shapes alone
 * (edtr_amd/detinput.py `resized_extent`, `batch_extent`).  One edtr_det_image per image, N of them in a DEVICE array that the kernel
 * reads and the same N in a HOST array that the entry point checks before anything is launched.  Layout (24 bytes, 8-byte aligned):
 *    0 src   fp32 planar [channels][h][w] on the device, contiguous, 4-byte aligned
 *    8 h  12 w  the source extent   16 oh  20 ow  the resized extent                                               all int32
 * batch [N][channels][H][W] in fp32 / fp16 / bf16 (out_dtype = EDTR_LOGITS_F32 / _F16 / _BF16).  For image i, channel c and
 * (y, x) in [0, oh) x [0, ow):
 *   taps     the four source elements of F.interpolate(size = (oh, ow), mode = "bilinear", align_corners = False): the source
 *            coordinate fp32(h) / fp32(oh) * (y + 0.5) - 0.5 clamped at 0, each step rounded (what scale_factor = with
 *            recompute_scale_factor = True reduces to), its floor cut at h - 1 and the lambda cut to [0, 1]; x alike
 *   value    every tap normalised as (v - mean_c) / std_c, an fp32 subtraction and an IEEE division as edtr_cls_normalize does; then
 *            the blend, columns first: top = (1 - tx) v00 + tx v01, bottom alike, out = (1 - ty) top + ty bottom, seven rounded fp32
 *            operations, no product contracted with a sum; a 16-bit batch takes the fp32 result rounded once (to nearest even)
 * and every other element of slot i is +0.0, written by the same launch: no memset, no requirement on what batch held, exactly one
 * writer per word, no atomics.  The bits are those of edtr_cls_normalize -> edtr_degrade_resize(bilinear) -> a zeroed batch -> a copy,
 * without the two intermediates.  mean_host / std_host: `channels` floats each, on the HOST.
 * A workgroup owns an EDTR_DET_TILE_H x EDTR_DET_TILE_W tile of a slot; a lane owns four columns, whose taps it works out once for
 * the rows and channels of the tile.  Rows move as 16 bytes per lane (8 for a 16-bit batch) where W % 4 == 0 and batch is aligned
 * to them, element by element otherwise.  Offsets into the batch are 64-bit.
 * Errors (nothing is launched): a NULL array, batch, mean_host, std_host or src EDTR_E_NULL; N outside 1 .. 65535, channels outside
 * 1 .. EDTR_DET_MAX_CHANNELS, any extent (h, w, oh, ow, H, W) below 1 or above EDTR_DET_MAX_EXTENT, oh > H, ow > W, a std of 0 or a
 * NaN constant EDTR_E_SHAPE; an unknown out_dtype EDTR_E_DTYPE; a src or batch not aligned to its element, or descs not to 8 bytes,
 * EDTR_E_ALIGN.
 * replaces: normalize, _resize_image_and_masks' F.interpolate and batch_images, model/faster_rcnn.py:2340-2349, 2519-2526, 2417-2435. */
#define EDTR_DET_MAX_CHANNELS 4
#define EDTR_DET_MAX_EXTENT 32768
#define EDTR_DET_TILE_W 256
#define EDTR_DET_TILE_H 16
typedef struct edtr_det_image {
    const float* src;
    int32_t h; int32_t w; int32_t oh; int32_t ow;
} edtr_det_image;
int edtr_det_transform(const edtr_det_image* descs_host, const edtr_det_image* descs, int N, int channels, const float* mean_host,
                       const float* std_host, int out_dtype, void* batch, int H, int W, edtr_stream_t stream);

/* ---- Detector training targets: match, encode, sample (additive to ABI 10) ------------------------------------------------------------
 * The non-learned half of the reference's Faster R-CNN in train mode (main/det/train_edtr.py:205-240): Matcher over box_iou,
 * BoxCoder.encode and BalancedPositiveNegativeSampler, as RegionProposalNetwork.assign_targets_to_anchors and
 * RoIHeads.select_training_samples run them (model/faster_rcnn.py:2030-2066, 1087-1185; model/util.py:594-679, 746-920).  No gradient
 * flows through any of it.  edtr_amd/targets.py restates every launch in numpy and writes the rules out; the launches equal the
 * restatements bit for bit except where logf enters (the dw and dh of an encoding).
 * The batch is ragged: image n owns boxes [box_start_n, box_start_{n+1}) and ground truths [gt_start_n, gt_start_{n+1}) of the flat
 * arrays.  table_host: int32 [N + 1][2] = box_start, gt_start on the HOST (checked before anything is launched), table: its copy on
 * the device (read by the kernels); both start at 0.  Boxes are fp32 xyxy, 16-byte aligned.
 * Common errors (nothing is launched): a NULL pointer EDTR_E_NULL; N <= 0, a table that does not start at 0, an image without a box
 * or with a negative count EDTR_E_SHAPE; N > 65535, an image of 2^24 boxes or more, or of more than EDTR_TARGETS_MAX_GT ground truths
 * EDTR_E_UNSUPPORTED; an unknown form or flag EDTR_E_DTYPE; boxes not aligned to 16 bytes, the others to their element EDTR_E_ALIGN. */
#define EDTR_TARGETS_MAX_GT 1024        /* ground truths of one image: they are kept in LDS */
#define EDTR_TARGETS_MAX_BATCH 4096     /* batch_size_per_image of the sampler */
#define EDTR_TARGETS_TILE 1024          /* boxes of one workgroup of the match passes */
#define EDTR_TARGETS_RPN 0              /* labels fp32: 1 matched, 0 below the low threshold, -1 between the thresholds */
#define EDTR_TARGETS_ROI 1              /* labels int64: gt_labels[matched], 0 below the low threshold, -1 between the thresholds */
#define EDTR_NOISE_SAMPLE_RPN 8         /* the sampler's keys for the RPN's anchors (draw = the training step): raw words, never normals */
#define EDTR_NOISE_SAMPLE_ROI 9         /* the sampler's keys for the box head's proposals (draw = the training step) */
/* Matcher(high, low, allow_low_quality) over box_iou(gt, boxes) per image, with no [G][P] matrix in memory.
 *   iou      area = (x2 - x1) (y2 - y1); w, h = max(min(rb) - max(lt), 0) (a NaN stays); inter = w h; iou = inter / ((area_g + area_p)
 *            - inter): each step one rounded fp32 operation, IEEE division
 *   best     per box the first maximal ground truth, a NaN counting as the maximum (torch's max(dim=0))
 *   matched  -1 where best < low, -2 where low <= best < high (a NaN compares false both times), else the index
 *   restore  with allow_low_quality: highest[g] = max over the image's boxes of iou[g][p] (a NaN propagates); every box whose iou with
 *            some g equals highest[g] gets its own best index back (set_low_quality_matches_, including that a ground truth which
 *            overlaps nothing restores every box whose iou with it is 0)
 * Two launches: a scan (a workgroup per EDTR_TARGETS_TILE boxes of an image, the image's ground truths in LDS) writes best_val,
 * best_idx [sum P] and partial [N][tiles][gmax] (uint32 order-preserving keys of each tile's greatest iou per ground truth; tiles =
 * ceil(max P / EDTR_TARGETS_TILE), gmax = max(max G, 1); partial_words >= N tiles gmax, EDTR_E_SHAPE otherwise); the assign pass folds
 * the keys in LDS and recomputes the ious it needs with the same code, the same bits.  No device-wide atomic.
 * shared = 1: boxes is one [P][4] set that every image uses (the RPN's anchors; every image's count must be P).  matched: int32
 * [sum P].  labels [sum P] by form (EDTR_TARGETS_RPN / _ROI; gt_labels: int64 [sum G], needed for _ROI).  regression (RPN form,
 * optional): fp32 [sum P][4], the encoding below of gt[max(matched, 0)] against every box with weights_host (four HOST floats).  An
 * image without ground truth: matched 0, label 0, encoded against the zero box (the reference's background branch).
 * low > high or a NaN threshold EDTR_E_SHAPE.
 * replaces: box_iou, Matcher.__call__, set_low_quality_matches_, assign_targets_to_anchors, assign_targets_to_proposals. */
int edtr_targets_match(const float* boxes, int shared, const float* gt_boxes, const int64_t* gt_labels, const int32_t* table_host,
                       const int32_t* table, int N, float high, float low, int allow_low_quality, int form, const float* weights_host,
                       float* best_val, int32_t* best_idx, uint32_t* partial, int64_t partial_words, int32_t* matched, void* labels,
                       float* regression, edtr_stream_t stream);
/* out [K][4] = encode_boxes(reference_boxes [K][4], proposals [K][4], weights) in the reference's operation order, each step rounded:
 * ew = px2 - px1, ecx = px1 + 0.5 ew, gw, gcx alike; dx = (wx (gcx - ecx)) / ew, dw = ww logf(gw / ew); y, h alike.
 * K <= 0 or a NaN weight EDTR_E_SHAPE; K > 2^30 EDTR_E_UNSUPPORTED.  replaces: BoxCoder.encode_single, model/util.py:594-679. */
int edtr_targets_encode(const float* reference_boxes, const float* proposals, int64_t K, const float* weights_host, float* out,
                        edtr_stream_t stream);
/* BalancedPositiveNegativeSampler with torch.randperm replaced by the seeded stream of "Reproducible noise".  Per image: positives are
 * labels >= 1, negatives labels == 0 (labels [sum P]: fp32 for EDTR_TARGETS_RPN, int64 for EDTR_TARGETS_ROI); num_pos = min(#positive,
 * max_pos), num_neg = min(#negative, batch - num_pos) (max_pos = int(batch positive_fraction), the caller's).  The key of box i is word
 * i & 3 of Philox on the counter (i >> 2, draw, purpose, image id), purpose EDTR_NOISE_SAMPLE_RPN or _ROI (EDTR_E_DTYPE otherwise); key,
 * ids and draw as for every stream consumer; keys (optional, uint32 [sum P] on the device) takes the stream's place: tests hand
 * equal keys in, which the stream practically never gives.  Sampled: the num_pos positives with the smallest keys, equal keys to the smaller index;
 * the negatives alike.  mask_pos, mask_neg: uint8 [sum P]; sampled: int32 [N][batch], the sampled image-local indices in ascending
 * order, then -1; counts: int32 [N][2] = num_pos, num_neg.  One 1024-lane workgroup per image: a radix select on the 32-bit key
 * (histograms by integer adds in LDS), then ordered ballots in index order.  No host sync.
 * batch <= 0, max_pos outside [0, batch], draw outside [0, 2^32) EDTR_E_SHAPE; batch > EDTR_TARGETS_MAX_BATCH EDTR_E_UNSUPPORTED.
 * replaces: BalancedPositiveNegativeSampler.__call__ with its two torch.randperm per image, model/util.py:860-920. */
int edtr_targets_sample(const void* labels, int form, const int32_t* table_host, const int32_t* table, int N, int batch, int max_pos,
                        uint64_t seed, const int64_t* image_ids, int64_t image_id_base, int64_t draw, int purpose, const uint32_t* keys,
                        uint8_t* mask_pos, uint8_t* mask_neg, int32_t* sampled, int32_t* counts, edtr_stream_t stream);
/* The last step of select_training_samples in one launch.  For slot (n, j) with i = sampled[n][j] >= 0: out_boxes = boxes[i] of image n,
 * out_labels = labels[i], out_matched = max(matched[i], 0), out_targets = the encoding of that ground truth (the zero box for an image
 * without any) against the box with weights_host.  A slot with i < 0: zeros, label -1.  out_boxes, out_targets: fp32 [N][batch][4];
 * out_labels, out_matched: int64 [N][batch].
 * replaces: the gathers by sampled_inds and BoxCoder.encode, model/faster_rcnn.py:1171-1185. */
int edtr_targets_gather(const float* boxes, const float* gt_boxes, const int32_t* matched, const int64_t* labels, const int32_t* table_host,
                        const int32_t* table, int N, const int32_t* sampled, int batch, const float* weights_host, float* out_boxes,
                        int64_t* out_labels, int64_t* out_matched, float* out_targets, edtr_stream_t stream);

/* ---- Training losses: the feature-matching L1 and the classifier's cross-entropy (additive to ABI 10) -------------------------------
 * The two loss terms every training script of the reference shares: F.l1_loss(feat_a, feat_b, reduction="mean") * w, its loss_fm and
 * loss_hlf (and the val_fd of the segmentation and detection test loops), and F.cross_entropy(pred, label) of the classifier.
 * edtr_amd/losses.py restates every launch in numpy (l1_mean_reference, l1_mean_backward_reference, cross_entropy_reference,
 * cross_entropy_backward_reference): the L1 launches equal the restatements bit for bit, the cross-entropy ones except in expf / logf.
 * No atomics, no memset, one writer per word; no result depends on the grid.
 *
 * Weighted mean-L1 over a list of pairs:  loss = sum over k of w_k mean_i |a_k[i] - b_k[i]|,  pairs <= EDTR_L1_MAX_PAIRS.
 * Per pair, in HOST arrays: dtype_host (EDTR_LOGITS_F32 / _F16 / _BF16), a_host / b_host (device pointers, contiguous, n elements of
 * that type), n_host (int64, 1 ... EDTR_L1_MAX_ELEMS), weight_host (fp32).  Offsets are 64-bit.
 *   difference  formed in fp32: both operands widened exactly, ONE rounded subtraction, fabsf; added in fp64.  For 16-bit inputs this is
 *               what torch computes under autocast (l1_loss runs in fp32 there) and a deliberate difference from a plain 16-bit
 *               l1_loss, which rounds each difference to 16 bits.  A NaN difference makes the loss NaN, as in torch.
 *   order       of the fp64 sum: a function of n alone, the same for the three element types.  A chunk is EDTR_L1_CHUNK elements; lane l
 *               of 256 owns elements 4 l ... 4 l + 3 of each of the chunk's four 1024-element quarters and adds its (up to) 16
 *               differences in ascending order from +0; the tree s = 128, 64, ..., 1 with sum[l] += sum[l + s] gives the chunk's
 *               partial, one fp64 word per chunk in the workspace, the pairs concatenated.  Workgroups stride over the chunks.
 *   finalize    one workgroup: per pair, lane l adds partials l, l + 256, ... ascending from +0, then the same tree; term_k = sum /
 *               (double)n_k; total = sum over k ascending from +0 of (double)w_k term_k; loss[0] = (float)total and, where terms is
 *               not NULL, terms[k] = (float)term_k, the unweighted means.
 *   loads       16 bytes a lane (8 for 16-bit types) where both pointers of a pair are aligned to them, element loads otherwise and in
 *               a pair's last partial group of four: the same bits.
 * edtr_l1_workspace(n_host, pairs) = 8 bytes per chunk (0 for a NULL array, pairs outside 1 ... EDTR_L1_MAX_PAIRS or an n outside
 * 1 ... EDTR_L1_MAX_ELEMS); the workspace may hold anything before the call.  edtr_l1_forward is two launches (chunks, finalize).
 * edtr_l1_backward, one launch for all pairs: grad_a_host[k] / grad_b_host[k] are device pointers of n_k elements in the pair's type,
 * either may be NULL per pair, a pair with both NULL is skipped, all NULL is an error.
 *   c_k      = (float)((double)grad_loss[0] (double)w_k / (double)n_k), grad_loss read on the device
 *   grad_a[i] = +c_k where the fp32 difference is positive, -c_k where it is negative, +0.0 where it is zero or NaN (torch's sign);
 *   grad_b[i] = -grad_a[i] by a flip of the sign bit (-0.0 where grad_a is +0.0).  A 16-bit output takes c_k rounded once (nearest even).
 * Every element is written, one writer per word.  max_blocks caps the grid of both (0: the default cap).
 * Errors (nothing is launched), in this order: a NULL array, loss, workspace or grad_loss EDTR_E_NULL; pairs outside 1 ...
 * EDTR_L1_MAX_PAIRS or max_blocks < 0 EDTR_E_SHAPE; a NULL a / b, or every gradient pointer NULL, EDTR_E_NULL; an unknown dtype
 * EDTR_E_DTYPE; n <= 0 EDTR_E_SHAPE; n > EDTR_L1_MAX_ELEMS EDTR_E_UNSUPPORTED; a workspace smaller than edtr_l1_workspace
 * EDTR_E_SHAPE; a / b / a gradient not aligned to its element, loss / terms / grad_loss to 4 or the workspace to 8 bytes EDTR_E_ALIGN.
 * replaces: F.l1_loss(feat_a, feat_b, reduction="mean") * w and its backward, main/cls/train_edtr.py:175-176, 213,
 * main/seg/train_edtr.py:180-181, 218, main/det/train_edtr.py:194-197, 236-237, main/seg/test_edtr.py:165, main/det/test_edtr.py:167-168. */
#define EDTR_L1_MAX_PAIRS 8
#define EDTR_L1_CHUNK 4096
#define EDTR_L1_MAX_ELEMS (1 << 30)
int64_t edtr_l1_workspace(const int64_t* n_host, int pairs);
int edtr_l1_forward(const int32_t* dtype_host, const void* const* a_host, const void* const* b_host, const int64_t* n_host,
                    const float* weight_host, int pairs, void* workspace, int64_t workspace_bytes, float* loss, float* terms,
                    int max_blocks, edtr_stream_t stream);
int edtr_l1_backward(const int32_t* dtype_host, const void* const* a_host, const void* const* b_host, const int64_t* n_host,
                     const float* weight_host, int pairs, const float* grad_loss, void* const* grad_a_host, void* const* grad_b_host,
                     int max_blocks, edtr_stream_t stream);
/* The classifier's loss: F.cross_entropy(logits [B][C], labels, reduction="mean", ignore_index=), the rule of the segmentation loss
 * ("Label maps") on rows.  logits fp32 / fp16 / bf16 by logits_dtype (widened exactly), labels int32 [B] on the device, C <=
 * EDTR_CLS_MAX_CLASSES, B <= 65535.
 *   lse     one wave64 workgroup per row: m the row maximum; s = sum of expf(z_c - m) in fp32, lane l adding c = l, l + 64, ... ascending
 *           from +0, then the tree o = 32, 16, ..., 1 with s[l] += s[l + o] over the 64 lanes; lse = m + logf(s).  Every step rounded.
 *   counts  a row counts iff label != ignore_index and 0 <= label < C; any other label that is not ignore_index is counted in
 *           counts[1] ("bad") and ignored, where torch raises (no launch here waits for the device)
 *   loss    the row term (double)(lse - z_label) goes to workspace (fp64 [B], 8-byte aligned, at least 8 B bytes; may hold anything
 *           before); one workgroup folds the counted rows in row order in fp64: loss[0] = (float)(sum / count), counts (int64 [2]) =
 *           count, bad.  count = 0 gives NaN, as torch does
 * edtr_cls_ce_forward writes lse (fp32 [B], every row: all the backward needs saved), loss and counts.  edtr_cls_ce_backward writes
 * grad [B][C] in the logits' type, every element: fmul(fadd(expf(fadd(z_c, -lse_b)), -[c == label_b]), g) with g = grad_loss[0] /
 * (float)counts[0], both read on the device; +0.0 on every row that does not count and everywhere with counts[0] = 0; a 16-bit
 * output is rounded once (torch rounds the upstream gradient to 16 bits first: a deliberate difference).
 * Errors (nothing is launched): a NULL pointer EDTR_E_NULL; unknown logits_dtype EDTR_E_DTYPE; B, C <= 0 or a workspace below 8 B
 * bytes EDTR_E_SHAPE; B > 65535 or C > EDTR_CLS_MAX_CLASSES EDTR_E_UNSUPPORTED; logits / grad not aligned to an element, labels / lse /
 * loss / grad_loss to 4, workspace / counts to 8 bytes EDTR_E_ALIGN.
 * replaces: F.cross_entropy(pred, label, reduction="mean", label_smoothing=0.0) and its backward, main/cls/train_edtr.py:208,
 * main/cls/train_cls.py:93. */
int edtr_cls_ce_forward(int logits_dtype, const void* logits, const int32_t* labels, int B, int C, int ignore_index, float* lse,
                        void* workspace, int64_t workspace_bytes, float* loss, int64_t* counts, edtr_stream_t stream);
int edtr_cls_ce_backward(int logits_dtype, const void* logits, const int32_t* labels, int B, int C, int ignore_index, const float* lse,
                         const int64_t* counts, const float* grad_loss, void* grad, edtr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * hipGraph capture of a launch sequence issued on `stream` (one denoise step, or a whole batch).
 * ---------------------------------------------------------------------------------------- */
int edtr_graph_begin(edtr_stream_t stream);
int edtr_graph_end(edtr_stream_t stream, void** graph_exec_out);
int edtr_graph_launch(void* graph_exec, edtr_stream_t stream);
int edtr_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* EDTR_HIP_H */
