// The segmentation loss from coarse logits (edtr_hip.h "Segmentation loss"; the host restatements are edtr_amd/labels.py
// `coarse_cross_entropy_reference` / `coarse_cross_entropy_backward_reference`):
//   F.cross_entropy(F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False), target, ignore_index)
// forward and backward, without the [B][n][H][W] tensor in either direction.  The forward blends a 16 x 64 output tile from its staged
// coarse patch exactly as edtr_seg_confusion_coarse does (glue.h's source_index / index_lambda / blend_taps / blended) and keeps one
// fp32 plane, the log-sum-exp; the backward GATHERS: a workgroup owns 8 x 8 coarse positions of one image, finds the output rows and
// columns whose taps reach them, blends those pixels again with the same device function (the same bits) and adds each element's
// terms in a fixed order.  No atomics, no memset: one writer per word, and nothing depends on the grid.
#include "common.h"
#include "glue.h"

namespace {

constexpr int kMaxClasses = 256;            // EDTR_SEG_CE_MAX_CLASSES
constexpr int kLimit = 1 << 24;             // extents stay below this: every index fits an int
constexpr int kTileH = 16, kTileW = 64;     // the forward's output tile, edtr_seg_confusion_coarse's: 16 rows of 16 lanes, four pixels a lane
constexpr int kPatchFloats = 4096;          // a tile's coarse patch, all n planes as fp32, is staged in LDS while it fits these 16 KiB
constexpr int kPos = 8;                     // the backward's tile: kPos x kPos coarse positions ...
constexpr int kChunk = 4;                   // ... times kChunk planes at a time: 256 lanes, one element each
constexpr int kHalo = kPos + 2;             // the patch of a tile with its one-position halo
constexpr int kFootPixels = 6144;           // lse (fp32) and the targets of a tile's footprint are staged while it has at most this many pixels ...
constexpr int kFootSide = 160;              // ... and at most this many rows and columns (their (i0, t) tables)

// (i0, i1, t) of output index `dst` along an axis of `in` source positions: ATen's rule, as the coarse confusion launch forms it
__device__ __forceinline__ void taps_of(float scale, int dst, int in, int& i0, int& i1, float& t) {
    index_lambda(fmaxf(source_index(scale, dst), 0.0f), in, i0, t);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

// one plane more of a pixel's running log-sum-exp: m the maximum so far, s = sum of exp(z - m) over the planes seen, zt the logit of
// the target's plane.  Each product, sum and difference is rounded on its own.
__device__ __forceinline__ void lse_step(float z, int c, uint32_t t, float& m, float& s, float& zt) {
    if (z > m) {
        s = add_rn(mul_rn(s, expf(add_rn(m, -z))), 1.0f);
        m = z;
    } else {
        s = add_rn(s, expf(add_rn(z, -m)));
    }
    zt = (uint32_t)c == t ? z : zt;
}

// coarse [B][n][ih][iw], target [B][H][W] -> lse [B][H][W] and, per 16 x 64 output tile, the fp64 sum of lse - z_target over the counted
// pixels, their number and the number of "bad" labels (n <= label != ignore).  The tile, its tables and its staged patch are
// coarse_confusion_kernel's; lane (ly, lx) owns pixels 4 lx .. 4 lx + 3 of row ly.  The tile's sum: a lane's pixels left to right, then
// a tree over the 256 lanes (lane i += lane i + o for o = 128, 64, ... 1): fixed by the shape, whatever the grid.
template <int DT>
__global__ void __launch_bounds__(256) seg_ce_forward_kernel(const void* coarse, const uint8_t* target, int B, int n, int ih, int iw, int H, int W,
                                                             float sh, float sw, int ignore, float* lse, double* part, int32_t* cnt, int32_t* bad) {
    __shared__ __attribute__((aligned(16))) float patch[kPatchFloats];
    __shared__ int row_i0[kTileH], row_i1[kTileH], col_i0[kTileW], col_i1[kTileW];
    __shared__ float row_t[kTileH], col_t[kTileW];
    __shared__ double red_s[256];
    __shared__ int red_c[256], red_b[256];
    const int tid = threadIdx.x;
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
    const int64_t per_image = (int64_t)tiles_y * tiles_x, total = (int64_t)B * per_image;
    const int ly = tid >> 4, lx = (tid & 15) << 2;
    for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int b = (int)(tile / per_image);
        const int64_t r = tile - (int64_t)b * per_image;
        const int ty0 = (int)(r / tiles_x) * kTileH, tx0 = (int)(r % tiles_x) * kTileW;
        __syncthreads();                    // the previous tile's readers of the tables, the patch and the sums are done
        if (tid < kTileH) {                 // (rows and columns past the image repeat its last one: their entries stay inside the source)
            const int y = ty0 + tid < H ? ty0 + tid : H - 1;
            taps_of(sh, y, ih, row_i0[tid], row_i1[tid], row_t[tid]);
        } else if (tid >= 64 && tid < 64 + kTileW) {
            const int j = tid - 64, x = tx0 + j < W ? tx0 + j : W - 1;
            taps_of(sw, x, iw, col_i0[j], col_i1[j], col_t[j]);
        }
        __syncthreads();
        // the source index grows with the output index (every step of it is a monotonic rounding), so the first i0 and the last i1 bound the patch
        const int py0 = row_i0[0], ph = row_i1[kTileH - 1] - py0 + 1, px0 = col_i0[0], pw = col_i1[kTileW - 1] - px0 + 1;
        const int npad = (n + 3) & ~3;
        const bool staged = (int64_t)npad * ph * pw <= kPatchFloats;
        const int64_t image = (int64_t)b * n * ih * iw;             // of plane 0 of image b in the coarse logits
        if (staged) {
            const int pp = ph * pw;
            for (int i = tid; i < npad * pp; i += 256) {            // (consecutive lanes read consecutive elements of a coarse row)
                const int c = i / pp, q = i - c * pp, yy = q / pw, xx = q - yy * pw;
                patch[q * npad + c] = c < n ? load1<DT>(coarse, image + ((int64_t)c * ih + py0 + yy) * iw + px0 + xx) : 0.0f;
            }
            __syncthreads();
        }
        const int y = ty0 + ly, x0 = tx0 + lx;
        double sum = 0.0;
        int counted = 0, wrong = 0;
        if (y < H && x0 < W) {
            const int valid = W - x0 < 4 ? W - x0 : 4;
            const int64_t at = ((int64_t)b * H + y) * W + x0;       // in target / lse
            uint32_t t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = j < valid ? (uint32_t)target[at + j] : 0u;
            int c0[4], c1[4];
            float tx[4], m[4], s[4], zt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c0[j] = col_i0[lx + j], c1[j] = col_i1[lx + j], tx[j] = col_t[lx + j], m[j] = -INFINITY, s[j] = 0.0f, zt[j] = 0.0f;
            const int ry0 = row_i0[ly], ry1 = row_i1[ly];
            const float ty = row_t[ly];
            if (staged) {                   // the planes of one coarse position lie side by side: a 16-byte read brings four planes of one tap
                const int r0 = (ry0 - py0) * pw - px0, r1 = (ry1 - py0) * pw - px0;
                int tap[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    tap[j][0] = (r0 + c0[j]) * npad, tap[j][1] = (r0 + c1[j]) * npad, tap[j][2] = (r1 + c0[j]) * npad, tap[j][3] = (r1 + c1[j]) * npad;
                for (int c4 = 0; c4 < n; c4 += 4) {
                    f32x4 q[4][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int k = 0; k < 4; ++k) q[j][k] = *reinterpret_cast<const f32x4*>(patch + tap[j][k] + c4);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (c4 + u >= n) break;             // (the planes that pad n to a multiple of 4 hold nothing)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            lse_step(blended<DT>(q[j][0][u], q[j][1][u], q[j][2][u], q[j][3][u], ty, tx[j]), c4 + u, t[j], m[j], s[j], zt[j]);
                    }
                }
            } else {                        // the same arithmetic with every tap read from memory
                const int64_t plane = (int64_t)ih * iw;
                for (int c = 0; c < n; ++c) {
                    const int64_t p0 = image + c * plane + (int64_t)ry0 * iw, p1 = image + c * plane + (int64_t)ry1 * iw;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        lse_step(blended<DT>(load1<DT>(coarse, p0 + c0[j]), load1<DT>(coarse, p0 + c1[j]), load1<DT>(coarse, p1 + c0[j]),
                                             load1<DT>(coarse, p1 + c1[j]), ty, tx[j]), c, t[j], m[j], s[j], zt[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= valid) continue;
                const float v = add_rn(m[j], logf(s[j]));
                lse[at + j] = v;
                if (t[j] != (uint32_t)ignore && t[j] < (uint32_t)n) {
                    sum += (double)add_rn(v, -zt[j]);
                    ++counted;
                } else if (t[j] != (uint32_t)ignore) {
                    ++wrong;
                }
            }
        }
        red_s[tid] = sum, red_c[tid] = counted, red_b[tid] = wrong;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red_s[tid] += red_s[tid + o], red_c[tid] += red_c[tid + o], red_b[tid] += red_b[tid + o];
            __syncthreads();
        }
        if (tid == 0) part[tile] = red_s[0], cnt[tile] = red_c[0], bad[tile] = red_b[0];
    }
}

// one workgroup: the tiles' sums folded in tile order by lane 0 (256 at a time through LDS) -> loss = float(sum / count), counts = (count, bad)
__global__ void __launch_bounds__(256) seg_ce_finalize_kernel(const double* part, const int32_t* cnt, const int32_t* bad, int64_t tiles, float* loss,
                                                              int64_t* counts) {
    __shared__ double sp[256];
    __shared__ int sc[256], sb[256];
    const int tid = threadIdx.x;
    double sum = 0.0;
    int64_t c = 0, w = 0;
    for (int64_t base = 0; base < tiles; base += 256) {
        if (base + tid < tiles) sp[tid] = part[base + tid], sc[tid] = cnt[base + tid], sb[tid] = bad[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int m = tiles - base < 256 ? (int)(tiles - base) : 256;
            for (int k = 0; k < m; ++k) sum += sp[k], c += sc[k], w += sb[k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        loss[0] = (float)(sum / (double)c);         // no counted pixel: 0 / 0 = NaN, torch's answer
        counts[0] = c, counts[1] = w;
    }
}

// the first index in [0, n_out) whose (i0, i1) satisfies the predicate (n_out if none does).  AFTER: i0 > i; else i1 >= i.  Both are
// monotonic in the index, as the source index is.
template <bool AFTER>
__device__ __forceinline__ int first_reaching(float scale, int n_out, int in, int i) {
    int lo = 0, hi = n_out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int i0, i1;
        float t;
        taps_of(scale, mid, in, i0, i1, t);
        if (AFTER ? i0 > i : i1 >= i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// grad [B][n][ih][iw] (the logits' type) = the adjoint of the forward's rule.  A workgroup owns kPos x kPos coarse positions of one
// image and kChunk of its planes; lane = (plane of the chunk, position).  The output rows whose taps reach coarse row i
// are the contiguous [first y with i1 >= i, first y with i0 > i), columns alike; the tile's footprint is the union.  STAGED: lse and the
// targets of the footprint and the (i0, t) of its rows and columns sit in LDS; else they are read / formed where they are used, with the
// same result.  Element (c, i, j): acc = 0; for y ascending { r = 0; for x ascending, pixels that count only { d = expf(z_c - lse) - [c == t];
// e = d * g; if (j0 == j) r += (1 - tx) * e; if (j1 == j) r += tx * e; }  if (i0 == i) acc += (1 - ty) * r; if (i1 == i) acc += ty * r; }
// with g = grad_loss / float(count), every product, sum and difference rounded on its own.  count == 0: every element +0.0.
template <int DT, bool STAGED>
__device__ __forceinline__ void backward_tile(const void* coarse, const uint8_t* target, const float* lse, void* grad, int b, int n, int ih, int iw, int H,
                                              int W, float sh, float sw, int ignore, float g, bool none, int c0, int i_lo, int j_lo, int fy0, int fr, int fx0,
                                              int fc, const int* ya, const int* yb, const int* xa, const int* xb, float* s_lse, uint8_t* s_tgt,
                                              int* s_ri, float* s_rt, int* s_ci, float* s_ct, float* patch) {
    const int tid = threadIdx.x;
    const int pc = tid >> 6, p = (tid >> 3) & 7, q = tid & 7;
    const int i = i_lo + p, j = j_lo + q;
    const int64_t pixels = ((int64_t)b * H) * W;
    if (STAGED) {
        for (int k = tid; k < fr; k += 256) {
            int i1;
            taps_of(sh, fy0 + k, ih, s_ri[k], i1, s_rt[k]);
        }
        for (int k = tid; k < fc; k += 256) {
            int j1;
            taps_of(sw, fx0 + k, iw, s_ci[k], j1, s_ct[k]);
        }
        for (int k = tid; k < fr * fc; k += 256) {
            const int yy = k / fc, xx = k - yy * fc;
            const int64_t at = pixels + (int64_t)(fy0 + yy) * W + fx0 + xx;
            s_lse[k] = lse[at], s_tgt[k] = target[at];
        }
    }
    __syncthreads();                    // the staged footprint is written
    for (int k = tid; k < kChunk * kHalo * kHalo; k += 256) {           // rows i_lo - 1 .. i_lo + kPos, columns alike, forced inside the source
        const int cc = k / (kHalo * kHalo), rem = k - cc * (kHalo * kHalo), yy = rem / kHalo, xx = rem - yy * kHalo;
        const int c = c0 + cc < n ? c0 + cc : n - 1;
        patch[k] = load1<DT>(coarse, (((int64_t)b * n + c) * ih + clamp_index(i_lo - 1 + yy, ih)) * iw + clamp_index(j_lo - 1 + xx, iw));
    }
    __syncthreads();
    const int c = c0 + pc;
    if (i >= ih || j >= iw || c >= n) return;           // (no lane leaves before the item's last barrier)
    const float* mine = patch + pc * (kHalo * kHalo);
    float acc = 0.0f;
    if (!none) {
        for (int y = ya[p]; y < yb[p]; ++y) {
            int i0, i1;
            float ty;
            if (STAGED) i0 = s_ri[y - fy0], ty = s_rt[y - fy0], i1 = i0 + (i0 < ih - 1 ? 1 : 0);
            else taps_of(sh, y, ih, i0, i1, ty);
            const float* r0 = mine + clamp_index(i0 - i_lo + 1, kHalo) * kHalo;        // (i - 1 <= i0 <= i <= i1 <= i + 1: inside the halo as it is)
            const float* r1 = mine + clamp_index(i1 - i_lo + 1, kHalo) * kHalo;
            float r = 0.0f;
            for (int x = xa[q]; x < xb[q]; ++x) {
                const int64_t at = pixels + (int64_t)y * W + x;
                const int f = (y - fy0) * fc + (x - fx0);
                const uint32_t t = STAGED ? (uint32_t)s_tgt[f] : (uint32_t)target[at];
                if (t == (uint32_t)ignore || t >= (uint32_t)n) continue;
                int j0, j1;
                float tx;
                if (STAGED) j0 = s_ci[x - fx0], tx = s_ct[x - fx0], j1 = j0 + (j0 < iw - 1 ? 1 : 0);
                else taps_of(sw, x, iw, j0, j1, tx);
                const int k0 = clamp_index(j0 - j_lo + 1, kHalo), k1 = clamp_index(j1 - j_lo + 1, kHalo);
                const float z = blended<DT>(r0[k0], r0[k1], r1[k0], r1[k1], ty, tx);
                const float d = add_rn(expf(add_rn(z, -(STAGED ? s_lse[f] : lse[at]))), t == (uint32_t)c ? -1.0f : 0.0f);
                const float e = mul_rn(d, g);
                if (j0 == j) r = add_rn(r, mul_rn(add_rn(1.0f, -tx), e));
                if (j1 == j) r = add_rn(r, mul_rn(tx, e));
            }
            if (i0 == i) acc = add_rn(acc, mul_rn(add_rn(1.0f, -ty), r));
            if (i1 == i) acc = add_rn(acc, mul_rn(ty, r));
        }
    }
    const int64_t o = (((int64_t)b * n + c) * ih + i) * iw + j;
    if (DT == EDTR_LOGITS_F32) static_cast<float*>(grad)[o] = acc;
    else static_cast<uint16_t*>(grad)[o] = DT == EDTR_LOGITS_F16 ? F16::from_f32(acc) : BF16::from_f32(acc);
}

template <int DT>
__global__ void __launch_bounds__(256) seg_ce_backward_kernel(const void* coarse, const uint8_t* target, const float* lse, const int64_t* counts,
                                                              const float* grad_loss, void* grad, int B, int n, int ih, int iw, int H, int W, float sh,
                                                              float sw, int ignore) {
    __shared__ float s_lse[kFootPixels];
    __shared__ uint8_t s_tgt[kFootPixels];
    __shared__ int s_ri[kFootSide], s_ci[kFootSide];
    __shared__ float s_rt[kFootSide], s_ct[kFootSide];
    __shared__ float patch[kChunk * kHalo * kHalo];
    __shared__ int ya[kPos], yb[kPos], xa[kPos], xb[kPos];
    const int tid = threadIdx.x;
    const int64_t count = counts[0];
    const bool none = count <= 0;
    const float g = none ? 0.0f : div_rn(grad_loss[0], (float)count);
    const int tiles_x = (iw + kPos - 1) / kPos, tiles_y = (ih + kPos - 1) / kPos;
    const int chunks = (n + kChunk - 1) / kChunk;
    const int64_t per_image = (int64_t)tiles_y * tiles_x, total = (int64_t)B * per_image * chunks;
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {           // item = (tile, chunk of planes), the chunks of a tile side by side
        const int64_t tile = item / chunks;
        const int c0 = (int)(item - tile * chunks) * kChunk;
        const int b = (int)(tile / per_image);
        const int64_t r = tile - (int64_t)b * per_image;
        const int i_lo = (int)(r / tiles_x) * kPos, j_lo = (int)(r % tiles_x) * kPos;
        __syncthreads();                    // the previous item's readers of the ranges, the staged footprint and the patch are done
        if (tid < kPos) {                   // (a position past the source takes the last one's range: the footprint stays that of the source)
            const int i = i_lo + tid < ih ? i_lo + tid : ih - 1;
            ya[tid] = first_reaching<false>(sh, H, ih, i), yb[tid] = first_reaching<true>(sh, H, ih, i);
        } else if (tid >= 64 && tid < 64 + kPos) {
            const int j = j_lo + tid - 64 < iw ? j_lo + tid - 64 : iw - 1;
            xa[tid - 64] = first_reaching<false>(sw, W, iw, j), xb[tid - 64] = first_reaching<true>(sw, W, iw, j);
        }
        __syncthreads();
        const int fy0 = ya[0], fr = yb[kPos - 1] - fy0, fx0 = xa[0], fc = xb[kPos - 1] - fx0;
        const bool staged = fr <= kFootSide && fc <= kFootSide && fr * fc <= kFootPixels;
        if (staged)
            backward_tile<DT, true>(coarse, target, lse, grad, b, n, ih, iw, H, W, sh, sw, ignore, g, none, c0, i_lo, j_lo, fy0, fr, fx0, fc, ya, yb, xa, xb,
                                    s_lse, s_tgt, s_ri, s_rt, s_ci, s_ct, patch);
        else
            backward_tile<DT, false>(coarse, target, lse, grad, b, n, ih, iw, H, W, sh, sw, ignore, g, none, c0, i_lo, j_lo, fy0, fr, fx0, fc, ya, yb, xa, xb,
                                     s_lse, s_tgt, s_ri, s_rt, s_ci, s_ct, patch);
    }
}

inline bool known_dtype(int dt) { return dt == EDTR_LOGITS_F32 || dt == EDTR_LOGITS_F16 || dt == EDTR_LOGITS_BF16; }

inline int64_t forward_tiles(int B, int H, int W) { return (int64_t)B * ((H + kTileH - 1) / kTileH) * ((W + kTileW - 1) / kTileW); }

// what both entry points check first, in edtr_seg_confusion_coarse's order
inline int check_shapes(int dt, const void* coarse, const uint8_t* target, int B, int n, int ih, int iw, int H, int W, int max_blocks) {
    if (!coarse || !target) return EDTR_E_NULL;
    if (!known_dtype(dt)) return EDTR_E_DTYPE;
    if (B <= 0 || n <= 0 || ih <= 0 || iw <= 0 || H <= 0 || W <= 0 || max_blocks < 0) return EDTR_E_SHAPE;
    if (n > kMaxClasses || B > kLimit || ih > kLimit || iw > kLimit || H > kLimit || W > kLimit) return EDTR_E_UNSUPPORTED;
    if ((double)B * n * ih * iw > 4.0e18 || (double)B * H * W > 4.0e18) return EDTR_E_UNSUPPORTED;       // element offsets are int64
    return EDTR_OK;
}

}  // namespace

extern "C" int64_t edtr_seg_ce_workspace(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 16 * forward_tiles(B, H, W);
}

extern "C" int edtr_seg_ce_forward(int logits_dtype, const void* coarse, int B, int n, int ih, int iw, const uint8_t* target, int H, int W,
                                   int ignore_index, float* lse, void* workspace, int64_t workspace_bytes, float* loss, int64_t* counts,
                                   int max_blocks, edtr_stream_t stream) {
    static_assert(kMaxClasses == EDTR_SEG_CE_MAX_CLASSES, "edtr_hip.h and seg_loss.hip disagree on the class limit");
    if (!lse || !workspace || !loss || !counts) return EDTR_E_NULL;
    const int bad = check_shapes(logits_dtype, coarse, target, B, n, ih, iw, H, W, max_blocks);
    if (bad != EDTR_OK) return bad;
    if (workspace_bytes < edtr_seg_ce_workspace(B, H, W)) return EDTR_E_SHAPE;
    if (!aligned_to(coarse, logits_dtype == EDTR_LOGITS_F32 ? 4 : 2) || !all_aligned_to(4, lse, loss) || !all_aligned_to(8, workspace, counts))
        return EDTR_E_ALIGN;
    const int64_t tiles = forward_tiles(B, H, W);
    const int64_t cap = max_blocks > 0 ? max_blocks : 8 * (int64_t)edtr_cu_count();
    const dim3 grid((unsigned)(tiles > cap ? cap : tiles)), block(256);
    const float sh = (float)ih / (float)H, sw = (float)iw / (float)W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    int32_t* cnt = reinterpret_cast<int32_t*>(part + tiles);
    int32_t* wrong = cnt + tiles;
#define EDTR_SEG_CE(DT) \
    hipLaunchKernelGGL((seg_ce_forward_kernel<DT>), grid, block, 0, st, coarse, target, B, n, ih, iw, H, W, sh, sw, ignore_index, lse, part, cnt, wrong)
    if (logits_dtype == EDTR_LOGITS_F32) EDTR_SEG_CE(EDTR_LOGITS_F32);
    else if (logits_dtype == EDTR_LOGITS_F16) EDTR_SEG_CE(EDTR_LOGITS_F16);
    else EDTR_SEG_CE(EDTR_LOGITS_BF16);
#undef EDTR_SEG_CE
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_ce_finalize_kernel, dim3(1), block, 0, st, part, cnt, wrong, tiles, loss, counts);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_seg_ce_backward(int logits_dtype, const void* coarse, int B, int n, int ih, int iw, const uint8_t* target, int H, int W,
                                    int ignore_index, const float* lse, const int64_t* counts, const float* grad_loss, void* grad,
                                    int max_blocks, edtr_stream_t stream) {
    if (!lse || !counts || !grad_loss || !grad) return EDTR_E_NULL;
    const int bad = check_shapes(logits_dtype, coarse, target, B, n, ih, iw, H, W, max_blocks);
    if (bad != EDTR_OK) return bad;
    const uintptr_t elem = logits_dtype == EDTR_LOGITS_F32 ? 4 : 2;
    if (!aligned_to(coarse, elem) || !aligned_to(grad, elem) || !all_aligned_to(4, lse, grad_loss) || !aligned_to(counts, 8)) return EDTR_E_ALIGN;
    const int64_t tiles = (int64_t)B * ((ih + kPos - 1) / kPos) * ((iw + kPos - 1) / kPos) * ((n + kChunk - 1) / kChunk);     // work items
    const int64_t cap = max_blocks > 0 ? max_blocks : 8 * (int64_t)edtr_cu_count();
    const dim3 grid((unsigned)(tiles > cap ? cap : tiles)), block(256);
    const float sh = (float)ih / (float)H, sw = (float)iw / (float)W;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define EDTR_SEG_CE(DT) \
    hipLaunchKernelGGL((seg_ce_backward_kernel<DT>), grid, block, 0, st, coarse, target, lse, counts, grad_loss, grad, B, n, ih, iw, H, W, sh, sw, ignore_index)
    if (logits_dtype == EDTR_LOGITS_F32) EDTR_SEG_CE(EDTR_LOGITS_F32);
    else if (logits_dtype == EDTR_LOGITS_F16) EDTR_SEG_CE(EDTR_LOGITS_F16);
    else EDTR_SEG_CE(EDTR_LOGITS_BF16);
#undef EDTR_SEG_CE
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
