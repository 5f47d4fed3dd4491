// Segmentation labels on the device (edtr_hip.h "Label maps"; the host restatements are edtr_amd/labels.py): argmax of the logits and
// the confusion matrix in one pass, Pillow's NEAREST resize, the pad / crop / flip window and the palette lookup, all on uint8 label
// maps and uint8 HWC images.  The file follows imageio.hip: one lane owns four pixels of a row and moves them as dwords / float4
// wherever the row pitch and the base keep them aligned, element by element otherwise.  Integer arithmetic and comparisons only:
// every result is a bit-exact function of its inputs, whatever the grid.  The one exception to "integer only" is the confusion
// matrix of COARSE logits (edtr_seg_confusion_coarse), which blends the bilinear upsample on chip before the argmax: its fp32
// products and sums are glue.h's, each rounded on its own in a stated order, so that launch is bit-exact against numpy all the same.
#include "common.h"
#include "glue.h"

namespace {

constexpr int kMaxClasses = 32;             // n of edtr_seg_confusion (EDTR_SEG_MAX_CLASSES): n * n bins of a 4 KiB sub-histogram
constexpr int kBins = kMaxClasses * kMaxClasses;
constexpr int kLimit = 1 << 24;             // extents and origins of the gathers stay below this: every index fits an int

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// four consecutive logits of one plane, widened exactly to fp32.  DT: EDTR_LOGITS_F32 / _F16 / _BF16.  VEC: one 16-byte (fp32) or
// 8-byte (16-bit) load; else the first `valid` of them one by one (the others are never looked at).
template <int DT, bool VEC>
__device__ __forceinline__ void load4(const void* base, int64_t e, int valid, float (&v)[4]) {
    if (DT == EDTR_LOGITS_F32) {
        const float* p = static_cast<const float*>(base) + e;
        if (VEC) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(p);
            v[0] = d.x, v[1] = d.y, v[2] = d.z, v[3] = d.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = j < valid ? p[j] : 0.0f;
        }
    } else {
        const uint16_t* p = static_cast<const uint16_t*>(base) + e;
        uint16_t r[4];
        if (VEC) {
            const u32x2 d = *reinterpret_cast<const u32x2*>(p);
            r[0] = (uint16_t)(d.x & 0xffffu), r[1] = (uint16_t)(d.x >> 16), r[2] = (uint16_t)(d.y & 0xffffu), r[3] = (uint16_t)(d.y >> 16);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = j < valid ? p[j] : (uint16_t)0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = DT == EDTR_LOGITS_F16 ? F16::to_f32(r[j]) : BF16::to_f32(r[j]);
    }
}

// torch's CPU argmax, one channel at a time in index order: a NaN beats every number, and among equals (two NaNs, two maxima,
// -0.0 and 0.0) the earlier channel stays.  Two selects under one condition, no branch: a value that is blended on the way here is
// formed whether or not it wins (a short-circuit would put its LDS reads behind the test of `best`, one pixel at a time).
__device__ __forceinline__ void take(float v, int c, float& best, int& idx) {
    const bool wins = (best == best) & ((v > best) | (v != v));
    best = wins ? v : best;
    idx = wins ? c : idx;
}

// the four targets of a lane's pixels at `at` (VEC: one dword; else the first `valid` bytes, 255 for the others)
template <bool VEC>
__device__ __forceinline__ void load_targets(const uint8_t* target, int64_t at, int valid, uint32_t (&t)[4]) {
    if (VEC) {
        const uint32_t d = *reinterpret_cast<const uint32_t*>(target + at);
        t[0] = d & 255u, t[1] = (d >> 8) & 255u, t[2] = (d >> 16) & 255u, t[3] = d >> 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = j < valid ? (uint32_t)target[at + j] : 255u;
    }
}

// the tail of a lane's four pixels at `at` of pred, with their targets t: pred = idx (VEC: one dword; else the first `valid` bytes),
// and the pixels j < counted with target < n add 1 to bin target * n + idx of the wave's sub-histogram `mine`, equal bins merged
// first (one atomic for a run inside one segment).  counted <= valid: a counted pixel is one of the loaded ones.
template <bool VEC>
__device__ __forceinline__ void count4(const uint32_t (&t)[4], uint8_t* pred, int64_t at, int valid, const int (&idx)[4], int counted, int n,
                                       uint32_t* mine) {
    if (pred) {
        if (VEC) {
            *reinterpret_cast<uint32_t*>(pred + at) = (uint32_t)idx[0] | (uint32_t)idx[1] << 8 | (uint32_t)idx[2] << 16 | (uint32_t)idx[3] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < valid) pred[at + j] = (uint8_t)idx[j];
        }
    }
    uint32_t bin[4];
    bool on[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        on[j] = j < counted && t[j] < (uint32_t)n;
        bin[j] = t[j] * (uint32_t)n + (uint32_t)idx[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!on[j]) continue;
        uint32_t cnt = 1u;
#pragma unroll
        for (int k = j + 1; k < 4; ++k)
            if (on[k] && bin[k] == bin[j]) {
                ++cnt;
                on[k] = false;
            }
        atomicAdd(&mine[bin[j]], cnt);
    }
}

// a workgroup's end: the non-zero sums of its four sub-histograms go to mat, one atomic each
__device__ __forceinline__ void flush_bins(const uint32_t (&hist)[4][kBins], int n, unsigned long long* mat) {
    for (int i = threadIdx.x; i < n * n; i += 256) {
        const uint32_t s = hist[0][i] + hist[1][i] + hist[2][i] + hist[3][i];
        if (s) atomicAdd(mat + i, (unsigned long long)s);
    }
}

// logits [B][n][H][W], target [B][H][W] -> mat [n][n] += counts, pred [B][H][W] = argmax.  A lane owns pixels 4 g .. 4 g + 3 of one
// row and walks the n planes; its counts go to its wave's sub-histogram in LDS (equal bins of the four pixels merged first: one
// atomic for a run inside one segment), and each workgroup adds its non-zero bins to mat once, at its end.
template <int DT, bool VEC>
__global__ void __launch_bounds__(256) confusion_kernel(const void* logits, const uint8_t* target, int B, int n, int H, int W,
                                                        const int32_t* sizes, unsigned long long* mat, uint8_t* pred) {
    __shared__ uint32_t hist[4][kBins];
    for (int i = threadIdx.x; i < 4 * kBins; i += 256) (&hist[0][0])[i] = 0u;
    __syncthreads();
    uint32_t* mine = hist[threadIdx.x >> 6];
    const int groups = (W + 3) >> 2;
    const int64_t plane = (int64_t)H * W, per_image = (int64_t)H * groups, total = (int64_t)B * per_image;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int b = (int)(g / per_image);
        const int64_t r = g - (int64_t)b * per_image;
        const int y = (int)(r / groups), x0 = (int)(r - (int64_t)y * groups) << 2;
        int h = H, w = W;
        if (sizes) {
            h = sizes[2 * b], w = sizes[2 * b + 1];
            h = h < 0 ? 0 : (h > H ? H : h);
            w = w < 0 ? 0 : (w > W ? W : w);
        }
        const bool counts = y < h && x0 < w;
        if (!pred && !counts) continue;             // nothing of this group is counted and nobody asked for its argmax
        const int valid = VEC ? 4 : (W - x0 < 4 ? W - x0 : 4);
        const int64_t at = (int64_t)b * plane + (int64_t)y * W + x0;            // in target / pred
        const int64_t e0 = (int64_t)b * n * plane + (int64_t)y * W + x0;        // in plane 0 of the logits
        float best[4];
        int idx[4] = {0, 0, 0, 0};
        load4<DT, VEC>(logits, e0, valid, best);
        int c = 1;
        for (; c + 3 < n; c += 4) {                 // four planes in flight
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) load4<DT, VEC>(logits, e0 + (int64_t)(c + u) * plane, valid, v[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) take(v[u][j], c + u, best[j], idx[j]);
        }
        for (; c < n; ++c) {
            float v[4];
            load4<DT, VEC>(logits, e0 + (int64_t)c * plane, valid, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) take(v[j], c, best[j], idx[j]);
        }
        uint32_t t[4];
        load_targets<VEC>(target, at, valid, t);
        count4<VEC>(t, pred, at, valid, idx, y < h ? w - x0 : 0, n, mine);
    }
    __syncthreads();
    flush_bins(hist, n, mat);
}

constexpr int kTileH = 16, kTileW = 64;     // the output tile of the coarse launch: 16 rows of 16 lanes, four pixels a lane
constexpr int kPatchFloats = 4096;          // a tile's coarse patch, all n planes as fp32, is staged in LDS while it fits these 16 KiB
// (load1 / as_stored / blended, which the segmentation loss of seg_loss.hip blends with as well, are glue.h's)

// The argmax over the n planes of a lane's four pixels from the staged patch, which holds the planes of one coarse position side by
// side: patch[position * npad + c], npad = n rounded up to 4.  tap[j]: the offsets of pixel j's four positions (row 0 / 1 x column
// 0 / 1), multiples of npad, so a 16-byte read brings four planes of one tap and the sixteen reads of a step feed sixteen blends.
// (-inf, 0) stands for "nothing seen yet": plane 0 replaces it unless it is -inf itself, and then index 0 is right as it is.
template <int DT>
__device__ __forceinline__ void argmax_staged(const float* patch, int n, const int (&tap)[4][4], float ty, const float (&tx)[4], int (&idx)[4]) {
    float best[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) best[j] = -INFINITY, idx[j] = 0;
    for (int c4 = 0; c4 < n; c4 += 4) {
        f32x4 q[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) q[j][k] = *reinterpret_cast<const f32x4*>(patch + tap[j][k] + c4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c4 + u >= n) break;                 // (the planes that pad n to a multiple of 4 hold nothing)
#pragma unroll
            for (int j = 0; j < 4; ++j) take(blended<DT>(q[j][0][u], q[j][1][u], q[j][2][u], q[j][3][u], ty, tx[j]), c4 + u, best[j], idx[j]);
        }
    }
}

// The same from the coarse logits in memory, for a patch that does not fit: plane c of image b starts at first + c * plane; r0 / r1
// are the offsets of the two tap rows in a plane, c0 / c1 the tap columns of each pixel.
template <int DT>
__device__ __forceinline__ void argmax_memory(const void* coarse, int64_t first, int64_t plane, int n, int64_t r0, int64_t r1, const int (&c0)[4],
                                              const int (&c1)[4], float ty, const float (&tx)[4], int (&idx)[4]) {
    float best[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) best[j] = -INFINITY, idx[j] = 0;
    for (int c = 0; c < n; ++c) {
        const int64_t p0 = first + c * plane + r0, p1 = first + c * plane + r1;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = blended<DT>(load1<DT>(coarse, p0 + c0[j]), load1<DT>(coarse, p0 + c1[j]), load1<DT>(coarse, p1 + c0[j]),
                               load1<DT>(coarse, p1 + c1[j]), ty, tx[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) take(v[j], c, best[j], idx[j]);
    }
}

// coarse [B][n][ih][iw], target [B][H][W] -> mat [n][n] += counts, pred [B][H][W] = argmax of the bilinear upsample to H x W, which is
// never stored.  A workgroup walks 16 x 64 output tiles.  Per tile: the (i0, i1, t) of its 16 rows and 64 columns once, into LDS; the
// coarse patch they span, all n planes (padded to a multiple of 4), into LDS as fp32 while it fits kPatchFloats (else every tap is
// read from memory); then lane (ly, lx) owns pixels 4 lx .. 4 lx + 3 of row ly, fetches its targets before it blends, and counts as
// confusion_kernel does.  sh / sw: ATen's scales in / out, from the host.
template <int DT, bool VEC>
__global__ void __launch_bounds__(256) coarse_confusion_kernel(const void* coarse, const uint8_t* target, int B, int n, int ih, int iw,
                                                               int H, int W, float sh, float sw, const int32_t* sizes,
                                                               unsigned long long* mat, uint8_t* pred) {
    __shared__ uint32_t hist[4][kBins];
    __shared__ __attribute__((aligned(16))) float patch[kPatchFloats];
    __shared__ int row_i0[kTileH], row_i1[kTileH], col_i0[kTileW], col_i1[kTileW];
    __shared__ float row_t[kTileH], col_t[kTileW];
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * kBins; i += 256) (&hist[0][0])[i] = 0u;
    uint32_t* mine = hist[tid >> 6];
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
    const int64_t per_image = (int64_t)tiles_y * tiles_x, total = (int64_t)B * per_image;
    const int ly = tid >> 4, lx = (tid & 15) << 2;
    for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int b = (int)(tile / per_image);
        const int64_t r = tile - (int64_t)b * per_image;
        const int ty0 = (int)(r / tiles_x) * kTileH, tx0 = (int)(r % tiles_x) * kTileW;
        __syncthreads();                    // the histograms are zeroed; the previous tile's readers of the tables and the patch are done
        if (tid < kTileH) {                 // (rows and columns past the image repeat its last one: their entries stay inside the source)
            const int y = ty0 + tid < H ? ty0 + tid : H - 1;
            int i0;
            float t;
            index_lambda(fmaxf(source_index(sh, y), 0.0f), ih, i0, t);
            row_i0[tid] = i0, row_i1[tid] = i0 + (i0 < ih - 1 ? 1 : 0), row_t[tid] = t;
        } else if (tid >= 64 && tid < 64 + kTileW) {
            const int j = tid - 64, x = tx0 + j < W ? tx0 + j : W - 1;
            int i0;
            float t;
            index_lambda(fmaxf(source_index(sw, x), 0.0f), iw, i0, t);
            col_i0[j] = i0, col_i1[j] = i0 + (i0 < iw - 1 ? 1 : 0), col_t[j] = t;
        }
        __syncthreads();
        // the source index grows with the output index (every step of it is a monotonic rounding), so the first i0 and the last i1 bound the patch
        const int py0 = row_i0[0], ph = row_i1[kTileH - 1] - py0 + 1, px0 = col_i0[0], pw = col_i1[kTileW - 1] - px0 + 1;
        const int npad = (n + 3) & ~3;
        const bool staged = (int64_t)npad * ph * pw <= kPatchFloats;
        const int64_t image = (int64_t)b * n * ih * iw;             // of plane 0 of image b in the coarse logits
        if (staged) {
            const int pp = ph * pw;
            for (int i = tid; i < n * pp; i += 256) {               // (consecutive lanes read consecutive elements of a coarse row)
                const int c = i / pp, q = i - c * pp, yy = q / pw, xx = q - yy * pw;
                patch[q * npad + c] = load1<DT>(coarse, image + ((int64_t)c * ih + py0 + yy) * iw + px0 + xx);
            }
            __syncthreads();
        }
        const int y = ty0 + ly, x0 = tx0 + lx;
        int h = H, w = W;
        if (sizes) {
            h = sizes[2 * b], w = sizes[2 * b + 1];
            h = h < 0 ? 0 : (h > H ? H : h);
            w = w < 0 ? 0 : (w > W ? W : w);
        }
        if (y >= H || x0 >= W) continue;                    // (no barrier depends on this lane before the next tile's first one)
        if (!pred && !(y < h && x0 < w)) continue;          // nothing of this group is counted and nobody asked for its argmax
        const int valid = VEC ? 4 : (W - x0 < 4 ? W - x0 : 4);
        const int64_t at = ((int64_t)b * H + y) * W + x0;           // in target / pred
        uint32_t t[4];
        load_targets<VEC>(target, at, valid, t);
        int c0[4], c1[4], idx[4];
        float tx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c0[j] = col_i0[lx + j], c1[j] = col_i1[lx + j], tx[j] = col_t[lx + j];
        const int ry0 = row_i0[ly], ry1 = row_i1[ly];
        if (staged) {
            const int r0 = (ry0 - py0) * pw - px0, r1 = (ry1 - py0) * pw - px0;
            int tap[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                tap[j][0] = (r0 + c0[j]) * npad, tap[j][1] = (r0 + c1[j]) * npad, tap[j][2] = (r1 + c0[j]) * npad, tap[j][3] = (r1 + c1[j]) * npad;
            argmax_staged<DT>(patch, n, tap, row_t[ly], tx, idx);
        } else {
            argmax_memory<DT>(coarse, image, (int64_t)ih * iw, n, (int64_t)ry0 * iw, (int64_t)ry1 * iw, c0, c1, row_t[ly], tx, idx);
        }
        count4<VEC>(t, pred, at, valid, idx, y < h ? w - x0 : 0, n, mine);
    }
    __syncthreads();
    flush_bins(hist, n, mat);
}

// one pixel of C bytes as the low bytes of a dword
template <int C>
__device__ __forceinline__ uint32_t load_px(const uint8_t* s) {
    return C == 1 ? (uint32_t)s[0] : ((uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16);
}

// four pixels to o.  VEC: the 4 (C = 1) or 12 (C = 3) bytes are aligned dwords; else the first `valid` pixels byte by byte.
template <int C, bool VEC>
__device__ __forceinline__ void store4(uint8_t* o, const uint32_t (&p)[4], int valid) {
    if (VEC) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
        if (C == 1) {
            o32[0] = p[0] | p[1] << 8 | p[2] << 16 | p[3] << 24;
        } else {
            o32[0] = p[0] | p[1] << 24;
            o32[1] = p[1] >> 8 | p[2] << 16;
            o32[2] = p[2] >> 16 | p[3] << 8;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < valid) {
#pragma unroll
                for (int c = 0; c < C; ++c) o[C * j + c] = (uint8_t)(p[j] >> (8 * c));
            }
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }       // (not glue.h's clamp_index: both ends given)

// dst (y, x) = src (y_idx[y], x_idx[x]); the tables are forced inside the source: a wrong one cannot make the kernel read out of bounds
template <int C, bool VEC>
__global__ void __launch_bounds__(256) resize_nearest_kernel(const uint8_t* src, int in_h, int in_w, uint8_t* dst, int out_h, int out_w,
                                                             const int32_t* y_idx, const int32_t* x_idx) {
    const int groups = (out_w + 3) >> 2;
    const int64_t total = (int64_t)out_h * groups;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        const uint8_t* line = src + (int64_t)clampi(y_idx[y], 0, in_h - 1) * in_w * C;
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j < out_w ? x0 + j : out_w - 1;
            p[j] = load_px<C>(line + (int64_t)clampi(x_idx[x], 0, in_w - 1) * C);
        }
        store4<C, VEC>(dst + ((int64_t)y * out_w + x0) * C, p, out_w - x0);
    }
}

// dst (y, x) = src (y0 + y', x0 + x') with y' = H - 1 - y under vflip and x' = W - 1 - x under hflip; `fill` outside the source
template <int C, bool VEC>
__global__ void __launch_bounds__(256) window_kernel(const uint8_t* src, int h, int w, uint8_t* dst, int H, int W, int y0, int x0,
                                                     int hflip, int vflip, uint32_t fill_px) {
    const int groups = (W + 3) >> 2;
    const int64_t total = (int64_t)H * groups;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), xg = (int)(g - (int64_t)y * groups) << 2;
        const int sy = y0 + (vflip ? H - 1 - y : y);
        const bool row_in = sy >= 0 && sy < h;
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = xg + j;
            const int sx = x0 + (hflip ? W - 1 - x : x);
            p[j] = fill_px;
            if (row_in && x < W && sx >= 0 && sx < w) p[j] = load_px<C>(src + ((int64_t)sy * w + sx) * C);
        }
        store4<C, VEC>(dst + ((int64_t)y * W + xg) * C, p, W - xg);
    }
}

// dst [N][3] = palette[labels [N]]: the palette as 256 packed colours in LDS, a lane owns labels 4 g .. 4 g + 3.
// VEC: 4-byte aligned labels and dst (a last group of fewer than four labels goes byte by byte).
template <bool VEC>
__global__ void __launch_bounds__(256) colorize_kernel(const uint8_t* labels, int64_t N, const uint8_t* palette, uint8_t* dst) {
    __shared__ uint32_t pal[256];
    pal[threadIdx.x] = load_px<3>(palette + 3 * threadIdx.x);
    __syncthreads();
    const int64_t total = (N + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t i0 = g << 2;
        const int valid = N - i0 < 4 ? (int)(N - i0) : 4;
        uint32_t p[4];
        if (VEC && valid == 4) {
            const uint32_t d = *reinterpret_cast<const uint32_t*>(labels + i0);
            p[0] = pal[d & 255u], p[1] = pal[(d >> 8) & 255u], p[2] = pal[(d >> 16) & 255u], p[3] = pal[d >> 24];
            store4<3, true>(dst + i0 * 3, p, 4);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = j < valid ? pal[labels[i0 + j]] : 0u;
            store4<3, false>(dst + i0 * 3, p, valid);
        }
    }
}

}  // namespace

extern "C" int edtr_seg_confusion(int logits_dtype, const void* logits, const uint8_t* target, int B, int n, int H, int W,
                                  const int32_t* sizes_host, const int32_t* sizes, int64_t* mat, uint8_t* pred, int max_blocks,
                                  edtr_stream_t stream) {
    static_assert(kMaxClasses == EDTR_SEG_MAX_CLASSES, "edtr_hip.h and labels.hip disagree on the class limit");
    if (!logits || !target || !mat) return EDTR_E_NULL;
    if ((sizes_host == nullptr) != (sizes == nullptr)) return EDTR_E_NULL;
    if (logits_dtype != EDTR_LOGITS_F32 && logits_dtype != EDTR_LOGITS_F16 && logits_dtype != EDTR_LOGITS_BF16) return EDTR_E_DTYPE;
    if (B <= 0 || n <= 0 || H <= 0 || W <= 0 || max_blocks < 0) return EDTR_E_SHAPE;
    if (n > kMaxClasses || B > kLimit || H > kLimit || W > kLimit) return EDTR_E_UNSUPPORTED;
    if ((double)B * n * H * W > 4.0e18) return EDTR_E_UNSUPPORTED;                  // element offsets are int64
    if (sizes_host)
        for (int b = 0; b < B; ++b)
            if (sizes_host[2 * b] <= 0 || sizes_host[2 * b] > H || sizes_host[2 * b + 1] <= 0 || sizes_host[2 * b + 1] > W) return EDTR_E_SHAPE;
    const uintptr_t elem = logits_dtype == EDTR_LOGITS_F32 ? 4 : 2;
    if (!aligned_to(logits, elem) || !aligned_to(sizes, 4) || !aligned_to(mat, 8)) return EDTR_E_ALIGN;
    const bool vec = W % 4 == 0 && aligned_to(logits, 4 * elem) && aligned_to(target, 4) && aligned_to(pred, 4);
    const int64_t items = (int64_t)B * H * ((W + 3) / 4);
    // the default cap: two workgroups (8 waves) per compute unit.  Every workgroup ends with its atomics into the same n * n words of
    // mat, and those serialise, so a launch pays for every workgroup it has on top of its traffic (DESIGN.md "Label maps" has the
    // sweep of max_blocks this was chosen from: one shape, resident in the Infinity Cache).  The bins of a workgroup are 32-bit, so a
    // grid never gets so few workgroups that one of them could count 2^32 pixels.
    int64_t blocks = (items + 255) / 256;
    const int64_t cap = max_blocks > 0 ? max_blocks : 2 * (int64_t)edtr_cu_count();
    blocks = blocks > cap ? cap : blocks;
    const int64_t least = (((int64_t)B * H * W) >> 30) + 1;
    blocks = blocks < least ? least : blocks;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* m = reinterpret_cast<unsigned long long*>(mat);
#define EDTR_CONFUSION(DT)                                                                                                          \
    do {                                                                                                                            \
        if (vec) hipLaunchKernelGGL((confusion_kernel<DT, true>), grid, block, 0, st, logits, target, B, n, H, W, sizes, m, pred);  \
        else hipLaunchKernelGGL((confusion_kernel<DT, false>), grid, block, 0, st, logits, target, B, n, H, W, sizes, m, pred);     \
    } while (0)
    if (logits_dtype == EDTR_LOGITS_F32) EDTR_CONFUSION(EDTR_LOGITS_F32);
    else if (logits_dtype == EDTR_LOGITS_F16) EDTR_CONFUSION(EDTR_LOGITS_F16);
    else EDTR_CONFUSION(EDTR_LOGITS_BF16);
#undef EDTR_CONFUSION
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_seg_confusion_coarse(int logits_dtype, const void* coarse, int B, int n, int ih, int iw, const uint8_t* target, int H,
                                         int W, const int32_t* sizes_host, const int32_t* sizes, int64_t* mat, uint8_t* pred,
                                         int max_blocks, edtr_stream_t stream) {
    if (!coarse || !target || !mat) return EDTR_E_NULL;
    if ((sizes_host == nullptr) != (sizes == nullptr)) return EDTR_E_NULL;
    if (logits_dtype != EDTR_LOGITS_F32 && logits_dtype != EDTR_LOGITS_F16 && logits_dtype != EDTR_LOGITS_BF16) return EDTR_E_DTYPE;
    if (B <= 0 || n <= 0 || ih <= 0 || iw <= 0 || H <= 0 || W <= 0 || max_blocks < 0) return EDTR_E_SHAPE;
    if (n > kMaxClasses || B > kLimit || ih > kLimit || iw > kLimit || H > kLimit || W > kLimit) return EDTR_E_UNSUPPORTED;
    if ((double)B * n * ih * iw > 4.0e18 || (double)B * H * W > 4.0e18) return EDTR_E_UNSUPPORTED;       // element offsets are int64
    if (sizes_host)
        for (int b = 0; b < B; ++b)
            if (sizes_host[2 * b] <= 0 || sizes_host[2 * b] > H || sizes_host[2 * b + 1] <= 0 || sizes_host[2 * b + 1] > W) return EDTR_E_SHAPE;
    if (!aligned_to(coarse, logits_dtype == EDTR_LOGITS_F32 ? 4 : 2) || !aligned_to(sizes, 4) || !aligned_to(mat, 8)) return EDTR_E_ALIGN;
    const bool vec = W % 4 == 0 && aligned_to(target, 4) && aligned_to(pred, 4);
    const int64_t tiles = (int64_t)B * ((H + kTileH - 1) / kTileH) * ((W + kTileW - 1) / kTileW);
    // the grid: edtr_seg_confusion's default cap and its floor (a workgroup's bins are 32-bit), over tiles of 1024 pixels
    const int64_t cap = max_blocks > 0 ? max_blocks : 2 * (int64_t)edtr_cu_count();
    int64_t blocks = tiles > cap ? cap : tiles;
    const int64_t least = (((int64_t)B * H * W) >> 30) + 1;
    blocks = blocks < least ? least : blocks;
    const float sh = (float)ih / (float)H, sw = (float)iw / (float)W;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* m = reinterpret_cast<unsigned long long*>(mat);
#define EDTR_COARSE(DT)                                                                                                                       \
    do {                                                                                                                                      \
        if (vec) hipLaunchKernelGGL((coarse_confusion_kernel<DT, true>), grid, block, 0, st, coarse, target, B, n, ih, iw, H, W, sh, sw, sizes, m, pred);  \
        else hipLaunchKernelGGL((coarse_confusion_kernel<DT, false>), grid, block, 0, st, coarse, target, B, n, ih, iw, H, W, sh, sw, sizes, m, pred);     \
    } while (0)
    if (logits_dtype == EDTR_LOGITS_F32) EDTR_COARSE(EDTR_LOGITS_F32);
    else if (logits_dtype == EDTR_LOGITS_F16) EDTR_COARSE(EDTR_LOGITS_F16);
    else EDTR_COARSE(EDTR_LOGITS_BF16);
#undef EDTR_COARSE
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

// C of {1, 3} and the dword form of a row of `row_px` pixels written at dst
#define EDTR_LABEL_DISPATCH(KERNEL, channels, vec, grid, st, ...)                                             \
    do {                                                                                                      \
        if (channels == 1) {                                                                                  \
            if (vec) hipLaunchKernelGGL((KERNEL<1, true>), grid, dim3(256), 0, st, __VA_ARGS__);              \
            else hipLaunchKernelGGL((KERNEL<1, false>), grid, dim3(256), 0, st, __VA_ARGS__);                 \
        } else {                                                                                              \
            if (vec) hipLaunchKernelGGL((KERNEL<3, true>), grid, dim3(256), 0, st, __VA_ARGS__);              \
            else hipLaunchKernelGGL((KERNEL<3, false>), grid, dim3(256), 0, st, __VA_ARGS__);                 \
        }                                                                                                     \
    } while (0)

extern "C" int edtr_label_resize_nearest(const uint8_t* src, int in_h, int in_w, int channels, uint8_t* dst, int out_h, int out_w,
                                         const int32_t* y_idx, const int32_t* x_idx, edtr_stream_t stream) {
    if (channels != 1 && channels != 3) return EDTR_E_UNSUPPORTED;
    if (!src || !dst || !y_idx || !x_idx) return EDTR_E_NULL;
    if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return EDTR_E_SHAPE;
    if (in_h > kLimit || in_w > kLimit || out_h > kLimit || out_w > kLimit) return EDTR_E_UNSUPPORTED;
    if (!aligned_to(y_idx, 4) || !aligned_to(x_idx, 4)) return EDTR_E_ALIGN;
    const bool vec = out_w % 4 == 0 && aligned_to(dst, 4);
    const dim3 grid(blocks_for((int64_t)out_h * ((out_w + 3) / 4)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    EDTR_LABEL_DISPATCH(resize_nearest_kernel, channels, vec, grid, st, src, in_h, in_w, dst, out_h, out_w, y_idx, x_idx);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_label_window(const uint8_t* src, int h, int w, int channels, uint8_t* dst, int H, int W, int y0, int x0, int hflip,
                                 int vflip, int fill, edtr_stream_t stream) {
    if (channels != 1 && channels != 3) return EDTR_E_UNSUPPORTED;
    if (!src || !dst) return EDTR_E_NULL;
    if (h <= 0 || w <= 0 || H <= 0 || W <= 0) return EDTR_E_SHAPE;
    if (h > kLimit || w > kLimit || H > kLimit || W > kLimit || y0 < -kLimit || y0 > kLimit || x0 < -kLimit || x0 > kLimit) return EDTR_E_UNSUPPORTED;
    if ((hflip != 0 && hflip != 1) || (vflip != 0 && vflip != 1) || fill < 0 || fill > 255) return EDTR_E_DTYPE;
    const bool vec = W % 4 == 0 && aligned_to(dst, 4);
    const uint32_t f = (uint32_t)fill, fill_px = channels == 1 ? f : (f | f << 8 | f << 16);
    const dim3 grid(blocks_for((int64_t)H * ((W + 3) / 4)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    EDTR_LABEL_DISPATCH(window_kernel, channels, vec, grid, st, src, h, w, dst, H, W, y0, x0, hflip, vflip, fill_px);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
#undef EDTR_LABEL_DISPATCH

extern "C" int edtr_label_colorize(const uint8_t* labels, int B, int H, int W, const uint8_t* palette, uint8_t* dst, edtr_stream_t stream) {
    if (!labels || !palette || !dst) return EDTR_E_NULL;
    if (B <= 0 || H <= 0 || W <= 0) return EDTR_E_SHAPE;
    if (B > kLimit || H > kLimit || W > kLimit || (double)B * H * W > 1.0e18) return EDTR_E_UNSUPPORTED;
    const int64_t N = (int64_t)B * H * W;
    const dim3 grid(blocks_for((N + 3) / 4)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (aligned_to(labels, 4) && aligned_to(dst, 4)) hipLaunchKernelGGL(colorize_kernel<true>, grid, block, 0, st, labels, N, palette, dst);
    else hipLaunchKernelGGL(colorize_kernel<false>, grid, block, 0, st, labels, N, palette, dst);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
