// Low-quality inputs from high-quality ones (edtr_hip.h "Low-quality inputs"; the host restatements are edtr_amd/degrade.py): the
// blur -> resize -> Gaussian noise -> JPEG chain of the reference's degradation, one launch each, on fp32 NCHW batches [B][3][H][W].
// Every product, sum and quotient that decides a result bit is a correctly rounded fp32 operation in a stated order (mul_rn / add_rn
// / div_rn of glue.h, compiled with contraction switched off), so numpy repeats each kernel bit for bit.  No MFMA: the blur and the
// JPEG transform live in LDS, the resize and the noise are streaming kernels.
#include "common.h"
#include "glue.h"
#include "philox.h"

// File scope: no product below is fused into a sum, whatever it is written with.
#pragma clang fp contract(off)

namespace {

constexpr int kFilterTile = 32;             // output tile edge of the blur: 256 lanes x 4 rows
constexpr int kFilterKMin = 3, kFilterKMax = 41;
constexpr int kDctPitch = 65;               // LDS row pitch of the 64 x 64 DCT table: row reads and column reads both hit 32 banks

// ---- filter2D --------------------------------------------------------------------------------------------------------------------

// workgroup (tile, channel, image): the 32 x 32 output tile's input patch with its halo, (32 + k - 1)^2 floats, and the image's k x k
// taps are staged in LDS once; lane (tx, ty) owns output rows ty, ty + 8, ty + 16, ty + 24 of column tx.  Per tap one broadcast read
// of the weight and four conflict-free row reads (32 consecutive floats per half wave).
__global__ void __launch_bounds__(256) filter2d_kernel(const float* x, const float* kernels, int n_kernels, float* out, int H, int W,
                                                       int k, int tiles_x) {
    extern __shared__ float lds[];
    const int tw = kFilterTile + k - 1, r = k >> 1;
    float* tile = lds;                      // [tw][tw]
    float* wk = lds + tw * tw;              // [k][k]
    const int b = blockIdx.z, c = blockIdx.y;
    const int ty0 = ((int)blockIdx.x / tiles_x) * kFilterTile, tx0 = ((int)blockIdx.x % tiles_x) * kFilterTile;
    const int64_t plane_off = ((int64_t)b * 3 + c) * H * W;
    const float* plane = x + plane_off;
    const float* kb = kernels + (n_kernels == 1 ? 0 : (int64_t)b * k * k);
    for (int i = threadIdx.x; i < k * k; i += 256) wk[i] = kb[i];
    for (int i = threadIdx.x; i < tw * tw; i += 256) {
        const int ly = i / tw, lx = i - ly * tw;
        tile[i] = plane[(int64_t)reflect(ty0 + ly - r, H) * W + reflect(tx0 + lx - r, W)];
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int ky = 0; ky < k; ++ky) {
        const float* row = tile + (ty + ky) * tw + tx;
        const float* wrow = wk + ky * k;
        for (int kx = 0; kx < k; ++kx) {
            const float w = wrow[kx];
            a0 = add_rn(a0, mul_rn(row[kx], w));
            a1 = add_rn(a1, mul_rn(row[8 * tw + kx], w));
            a2 = add_rn(a2, mul_rn(row[16 * tw + kx], w));
            a3 = add_rn(a3, mul_rn(row[24 * tw + kx], w));
        }
    }
    const int gx = tx0 + tx;
    if (gx >= W) return;
    float* o = out + plane_off + gx;
    const int gy = ty0 + ty;
    if (gy < H) o[(int64_t)gy * W] = a0;
    if (gy + 8 < H) o[(int64_t)(gy + 8) * W] = a1;
    if (gy + 16 < H) o[(int64_t)(gy + 16) * W] = a2;
    if (gy + 24 < H) o[(int64_t)(gy + 24) * W] = a3;
}

// ---- F.interpolate(size=, align_corners=False) -------------------------------------------------------------------------------------

// (the source coordinate is glue.h's source_index)

// the cubic convolution weights for A = -0.75 (A + 2 = 1.25, A + 3 = 2.25, 5 A = -3.75, 8 A = -6, 4 A = -3: all exact)
__device__ __forceinline__ float cubic1(float v) {      // |v| <= 1: ((A + 2) v - (A + 3)) v v + 1
    return add_rn(mul_rn(mul_rn(add_rn(mul_rn(1.25f, v), -2.25f), v), v), 1.0f);
}
__device__ __forceinline__ float cubic2(float v) {      // 1 < |v| < 2: ((A v - 5 A) v + 8 A) v - 4 A
    return add_rn(mul_rn(add_rn(mul_rn(add_rn(mul_rn(-0.75f, v), 3.75f), v), -6.0f), v), 3.0f);
}
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
    const float u = add_rn(1.0f, -t);
    w[0] = cubic2(add_rn(t, 1.0f));
    w[1] = cubic1(t);
    w[2] = cubic1(u);
    w[3] = cubic2(add_rn(u, 1.0f));
}

// one lane per output element of planes x oh x ow; MODE = EDTR_RESIZE_*
template <int MODE>
__global__ void __launch_bounds__(256) resize_kernel(const float* x, float* out, int planes, int ih, int iw, int oh, int ow, float sh,
                                                     float sw) {
    const int64_t total = (int64_t)planes * oh * ow;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t py = e / ow;
        const int ox = (int)(e - py * ow), p = (int)(py / oh), oy = (int)(py - (int64_t)p * oh);
        const float* src = x + (int64_t)p * ih * iw;
        float v;
        if (MODE == EDTR_RESIZE_BILINEAR) {
            int y0, x0;
            float ty, tx;
            index_lambda(fmaxf(source_index(sh, oy), 0.0f), ih, y0, ty);
            index_lambda(fmaxf(source_index(sw, ox), 0.0f), iw, x0, tx);
            v = bilinear_blend(src, ih, iw, y0, ty, x0, tx);
        } else if (MODE == EDTR_RESIZE_BICUBIC) {
            int y0, x0;
            float ty, tx, wy[4], wx[4];
            index_lambda(source_index(sh, oy), ih, y0, ty);
            index_lambda(source_index(sw, ox), iw, x0, tx);
            cubic_weights(ty, wy);
            cubic_weights(tx, wx);
            const int c0 = clamp_index(x0 - 1, iw), c1 = clamp_index(x0, iw), c2 = clamp_index(x0 + 1, iw), c3 = clamp_index(x0 + 2, iw);
            v = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* r = src + (int64_t)clamp_index(y0 - 1 + i, ih) * iw;
                float s = mul_rn(wx[0], r[c0]);
                s = add_rn(s, mul_rn(wx[1], r[c1]));
                s = add_rn(s, mul_rn(wx[2], r[c2]));
                s = add_rn(s, mul_rn(wx[3], r[c3]));
                v = i == 0 ? mul_rn(wy[0], s) : add_rn(v, mul_rn(wy[i], s));
            }
        } else {        // adaptive_avg_pool2d: rows [floor(oy ih / oh), ceil((oy + 1) ih / oh)), columns alike, in integers
            const int ys = (int)(((int64_t)oy * ih) / oh), ye = (int)((((int64_t)oy + 1) * ih + oh - 1) / oh);
            const int xs = (int)(((int64_t)ox * iw) / ow), xe = (int)((((int64_t)ox + 1) * iw + ow - 1) / ow);
            float s = 0.0f;
            for (int yy = ys; yy < ye; ++yy) {
                const float* r = src + (int64_t)yy * iw;
                for (int xx = xs; xx < xe; ++xx) s = add_rn(s, r[xx]);
            }
            v = div_rn(s, (float)((int64_t)(ye - ys) * (xe - xs)));
        }
        out[e] = v;
    }
}

// ---- Gaussian noise from the seeded stream -------------------------------------------------------------------------------------------

__device__ __forceinline__ float noisy(float xv, float z, float sigma, int rounds) {
    const float o = add_rn(xv, div_rn(mul_rn(z, sigma), 255.0f));
    if (rounds) return round_to_levels(o);
    return fminf(fmaxf(o, 0.0f), 1.0f);
}

// a lane owns four consecutive elements of one plane = one Philox call.  Colour: the counter's group is the element group of the
// [3][H][W] image (EDTR_NOISE_DEGRADE); grey: that of the [H][W] plane, the same for the three channels (EDTR_NOISE_DEGRADE_GRAY).
__global__ void __launch_bounds__(256) noise_kernel(const float* x, float* out, float* noise_out, const float* sigma, const int32_t* gray,
                                                    NoiseArgs a, int64_t n4) {
    const int64_t per4 = 3 * a.plane4;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / per4;
        int64_t eg = g - b * per4;
        const bool grey = gray[b] != 0;
        if (grey) eg %= a.plane4;
        const uint32_t id = EDTR_IMAGE_ID(a, b);
        const f32x4 z = philox_normal4(a.k0, a.k1, (uint32_t)eg, a.draw, grey ? EDTR_NOISE_DEGRADE_GRAY : EDTR_NOISE_DEGRADE, id);
        const float s = sigma[b];
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + g * 4);
        if (noise_out) *reinterpret_cast<f32x4*>(noise_out + g * 4) = z;
        *reinterpret_cast<f32x4*>(out + g * 4) =
            f32x4{noisy(xv.x, z.x, s, a.rounds), noisy(xv.y, z.y, s, a.rounds), noisy(xv.z, z.z, s, a.rounds), noisy(xv.w, z.w, s, a.rounds)};
    }
}

// ---- JPEG (DiffJPEG, differentiable = False) ------------------------------------------------------------------------------------------

// the luminance table as the reference uses it (the standard table TRANSPOSED), and the chrominance table
__device__ const float kJpegTables[2][64] = {
    {16, 12, 14, 14, 18, 24, 49, 72, 11, 12, 13, 17, 22, 35, 64, 92, 10, 14, 16, 22, 37, 55, 78, 95, 16, 19, 24, 29, 56, 64, 87, 98,
     24, 26, 40, 51, 68, 81, 103, 112, 40, 58, 57, 87, 109, 104, 121, 100, 51, 60, 69, 80, 103, 113, 120, 103, 61, 55, 56, 62, 77, 92, 101, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// workgroup (mcu column of the grid, image): one 16 x 16 MCU at a time, lane = pixel.  blk[0..3] the four luma blocks (row-major in
// the MCU), blk[4] Cb, blk[5] Cr; element [x][y] of a block at x * 8 + y (x = row).  Nothing but the input and the result touches HBM.
__global__ void __launch_bounds__(256) jpeg_kernel(const float* x, float* out, int H, int W, const float* factor, const float* dct,
                                                   float* coefs) {
    __shared__ float T[64 * kDctPitch];     // T[xy][uv] = cos((2x+1) u pi/16) cos((2y+1) v pi/16), float32 of the fp64 product
    __shared__ float tab[2][64];
    __shared__ float blk[6][64];            // level-shifted samples, later the reconstructed samples
    __shared__ float cfull[2][256];         // full-resolution Cb, Cr of the MCU
    __shared__ float cf[6][64];             // dequantised coefficients times alpha
    const int tid = threadIdx.x, b = blockIdx.y;
    for (int i = tid; i < 4096; i += 256) T[(i >> 6) * kDctPitch + (i & 63)] = dct[i];
    if (tid < 128) tab[tid >> 6][tid & 63] = kJpegTables[tid >> 6][tid & 63];
    const float f = factor[b];
    const int mw = (W + 15) >> 4, mh = (H + 15) >> 4;
    const int64_t plane = (int64_t)H * W;
    const float* img = x + (int64_t)b * 3 * plane;
    float* res = out + (int64_t)b * 3 * plane;
    const int64_t ny = (int64_t)mh * mw * 4, nc = (int64_t)mh * mw;
    float* cimg = coefs ? coefs + (int64_t)b * (ny + 2 * nc) * 64 : nullptr;
    const int py = tid >> 4, px = tid & 15;
    for (int m = blockIdx.x; m < mh * mw; m += gridDim.x) {
        const int my = m / mw, mx = m - my * mw;
        const int gy = my * 16 + py, gx = mx * 16 + px;
        const bool inside = gy < H && gx < W;
        __syncthreads();                    // the tables are staged; the previous MCU's blk / cfull reads are done
        {
            const int64_t e = (int64_t)gy * W + gx;
            const float r = inside ? mul_rn(img[e], 255.0f) : 0.0f;
            const float g = inside ? mul_rn(img[plane + e], 255.0f) : 0.0f;
            const float bl = inside ? mul_rn(img[2 * plane + e], 255.0f) : 0.0f;
            const float yv = add_rn(add_rn(mul_rn(r, 0.299f), mul_rn(g, 0.587f)), mul_rn(bl, 0.114f));
            const float cb = add_rn(add_rn(add_rn(mul_rn(r, -0.168736f), mul_rn(g, -0.331264f)), mul_rn(bl, 0.5f)), 128.0f);
            const float cr = add_rn(add_rn(add_rn(mul_rn(r, 0.5f), mul_rn(g, -0.418688f)), mul_rn(bl, -0.081312f)), 128.0f);
            blk[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = add_rn(yv, -128.0f);
            cfull[0][tid] = cb;
            cfull[1][tid] = cr;
        }
        __syncthreads();
        if (tid < 128) {                    // 2 x 2 mean: ((a00 + a01) + a10) + a11, times 1/4
            const int c = tid >> 6, i = tid & 63, cy = i >> 3, cx = i & 7;
            const float* q = cfull[c] + (2 * cy) * 16 + 2 * cx;
            const float s = add_rn(add_rn(add_rn(q[0], q[1]), q[16]), q[17]);
            blk[4 + c][i] = add_rn(mul_rn(s, 0.25f), -128.0f);
        }
        __syncthreads();
        for (int o = tid; o < 384; o += 256) {              // forward DCT, quantisation, dequantisation of coefficient uv of block bi
            const int bi = o >> 6, uv = o & 63, u = uv >> 3, v = uv & 7;
            const float* d = blk[bi];
            float acc = 0.0f;
#pragma unroll 8
            for (int xy = 0; xy < 64; ++xy) acc = add_rn(acc, mul_rn(d[xy], T[xy * kDctPitch + uv]));
            const bool u0 = u == 0, v0 = v == 0;
            const float scale = u0 && v0 ? 0.125f : (u0 || v0 ? 0.17677669529663687f : 0.25f);
            const float alpha = u0 && v0 ? 0.5f : (u0 || v0 ? 0.7071067811865475f : 1.0f);
            const float tq = mul_rn(tab[bi < 4 ? 0 : 1][uv], f);
            const float q = rintf(div_rn(mul_rn(scale, acc), tq));        // round half to even
            if (cimg) {
                int64_t bidx;
                if (bi < 4) bidx = ((int64_t)(my * 2 + (bi >> 1)) * (mw * 2) + mx * 2 + (bi & 1));
                else bidx = ny + (bi - 4) * nc + m;
                cimg[bidx * 64 + uv] = q;
            }
            cf[bi][uv] = mul_rn(mul_rn(q, tq), alpha);
        }
        __syncthreads();
        for (int o = tid; o < 384; o += 256) {              // inverse DCT of sample pq of block bi: T'[uv][pq] = T[pq][uv]
            const int bi = o >> 6, pq = o & 63;
            const float* c = cf[bi];
            float acc = 0.0f;
#pragma unroll 8
            for (int uv = 0; uv < 64; ++uv) acc = add_rn(acc, mul_rn(c[uv], T[pq * kDctPitch + uv]));
            blk[bi][pq] = add_rn(mul_rn(0.25f, acc), 128.0f);
        }
        __syncthreads();
        if (inside) {
            const float yv = blk[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)];
            const int ci = (py >> 1) * 8 + (px >> 1);       // nearest chroma upsampling
            const float cb = add_rn(blk[4][ci], -128.0f), cr = add_rn(blk[5][ci], -128.0f);
            const float r = add_rn(add_rn(mul_rn(yv, 1.0f), mul_rn(cb, 0.0f)), mul_rn(cr, 1.402f));
            const float g = add_rn(add_rn(mul_rn(yv, 1.0f), mul_rn(cb, -0.344136f)), mul_rn(cr, -0.714136f));
            const float bl = add_rn(add_rn(mul_rn(yv, 1.0f), mul_rn(cb, 1.772f)), mul_rn(cr, 0.0f));
            const int64_t e = (int64_t)gy * W + gx;
            res[e] = div_rn(fminf(255.0f, fmaxf(0.0f, r)), 255.0f);
            res[plane + e] = div_rn(fminf(255.0f, fmaxf(0.0f, g)), 255.0f);
            res[2 * plane + e] = div_rn(fminf(255.0f, fmaxf(0.0f, bl)), 255.0f);
        }
    }
}

}  // namespace

extern "C" int edtr_degrade_filter2d(const float* x, float* out, int B, int channels, int H, int W, const float* kernels,
                                     int n_kernels, int k, edtr_stream_t stream) {
    if (int rc = check_batch(x, out, B, channels, H, W)) return rc;
    if (!kernels) return EDTR_E_NULL;
    if (x == out) return EDTR_E_UNSUPPORTED;                        // a tile's halo is another tile's output
    if (k < kFilterKMin || k > kFilterKMax || !(k & 1)) return EDTR_E_SHAPE;
    if (k / 2 >= (H < W ? H : W)) return EDTR_E_SHAPE;              // reflect padding needs the mirrored samples to exist
    if (n_kernels != 1 && n_kernels != B) return EDTR_E_SHAPE;
    if (!aligned_to(kernels, 4)) return EDTR_E_ALIGN;
    const int tiles_x = (W + kFilterTile - 1) / kFilterTile, tiles_y = (H + kFilterTile - 1) / kFilterTile;
    if ((int64_t)tiles_x * tiles_y > 0x7fffffff) return EDTR_E_UNSUPPORTED;
    const int tw = kFilterTile + k - 1;
    const size_t lds = (size_t)(tw * tw + k * k) * sizeof(float);   // 27 460 bytes at k = 41
    hipLaunchKernelGGL(filter2d_kernel, dim3(tiles_x * tiles_y, 3, B), dim3(256), lds, static_cast<hipStream_t>(stream), x, kernels,
                       n_kernels, out, H, W, k, tiles_x);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_degrade_resize(const float* x, float* out, int B, int channels, int in_h, int in_w, int out_h, int out_w, int mode,
                                   edtr_stream_t stream) {
    if (int rc = check_batch(x, out, B, channels, in_h, in_w)) return rc;
    if (out_h <= 0 || out_w <= 0) return EDTR_E_SHAPE;
    if (out_h > (1 << 24) || out_w > (1 << 24)) return EDTR_E_UNSUPPORTED;
    if (mode != EDTR_RESIZE_BILINEAR && mode != EDTR_RESIZE_BICUBIC && mode != EDTR_RESIZE_AREA) return EDTR_E_DTYPE;
    if (x == out) return EDTR_E_UNSUPPORTED;
    const float sh = (float)in_h / (float)out_h, sw = (float)in_w / (float)out_w;
    const int planes = B * 3;
    const dim3 grid(blocks_for((int64_t)planes * out_h * out_w)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == EDTR_RESIZE_BILINEAR)
        hipLaunchKernelGGL(resize_kernel<EDTR_RESIZE_BILINEAR>, grid, block, 0, st, x, out, planes, in_h, in_w, out_h, out_w, sh, sw);
    else if (mode == EDTR_RESIZE_BICUBIC)
        hipLaunchKernelGGL(resize_kernel<EDTR_RESIZE_BICUBIC>, grid, block, 0, st, x, out, planes, in_h, in_w, out_h, out_w, sh, sw);
    else
        hipLaunchKernelGGL(resize_kernel<EDTR_RESIZE_AREA>, grid, block, 0, st, x, out, planes, in_h, in_w, out_h, out_w, sh, sw);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_degrade_gaussian_noise(const float* x, float* out, float* noise_out, int B, int channels, int H, int W,
                                           const float* sigma_host, const float* sigma, const int32_t* gray_host, const int32_t* gray,
                                           uint64_t seed, const int64_t* image_ids, int64_t image_id_base, int64_t draw, int rounds,
                                           edtr_stream_t stream) {
    if (int rc = check_batch(x, out, B, channels, H, W)) return rc;
    if (!sigma_host || !sigma || !gray_host || !gray) return EDTR_E_NULL;
    NoiseArgs a;
    if (int rc = make_noise_args(a, x, out, noise_out, B, H, W, sigma_host, gray_host, seed, image_ids, image_id_base, draw, rounds)) return rc;
    if (!all_aligned_to(4, sigma, gray)) return EDTR_E_ALIGN;
    const int64_t n4 = (int64_t)B * 3 * a.plane4;
    hipLaunchKernelGGL(noise_kernel, dim3(blocks_for(n4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, noise_out, sigma,
                       gray, a, n4);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_degrade_jpeg(const float* x, float* out, int B, int channels, int H, int W, const float* quality_host,
                                 const float* factor, const float* dct, float* coefs, edtr_stream_t stream) {
    if (int rc = check_batch(x, out, B, channels, H, W)) return rc;
    if (!quality_host || !factor || !dct) return EDTR_E_NULL;
    for (int b = 0; b < B; ++b)
        if (!(quality_host[b] > 0.0f) || !(quality_host[b] <= 100.0f)) return EDTR_E_SHAPE;
    if (!all_aligned_to(4, factor, dct, coefs)) return EDTR_E_ALIGN;
    const int64_t mcus = (int64_t)((H + 15) / 16) * ((W + 15) / 16);
    if (mcus > 0x7fffffff) return EDTR_E_UNSUPPORTED;
    const unsigned gx = (unsigned)(mcus < 256 ? mcus : 256);        // a workgroup stages the 16 KB table once for the MCUs it walks
    hipLaunchKernelGGL(jpeg_kernel, dim3(gx, B), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, H, W, factor, dct, coefs);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
