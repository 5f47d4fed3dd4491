// The 8-bit image boundary (edtr_hip.h "Images in, images out"; the host restatements are edtr_amd/imageio.py): Pillow's BICUBIC
// resize on uint8 HWC, uint8 / fp32 HWC -> padded fp32 NCHW batch slot, fp32 NCHW -> save_image's uint8 HWC, and the fp64 sum of
// squared differences behind PSNR.  All four are memory-bound: one lane owns four pixels of a row (12 source / destination
// bytes, three float4 of the planes) and moves them as dwords / float4 wherever the row pitch keeps them aligned, element by
// element otherwise.  Integer and correctly rounded fp32 / fp64 arithmetic only: every result is a bit-exact function of its inputs.
#include "common.h"
#include "glue.h"

namespace {

constexpr int kPrecisionBits = 22;          // Pillow: 32 - 8 - 2 (ImagingResample, 8 bits per channel)
constexpr int kSqBlocks = 64;               // partial sums per image of edtr_image_sqdiff (EDTR_SQDIFF_BLOCKS)

__device__ __forceinline__ uint32_t clip8(int acc) {
    const int v = acc >> kPrecisionBits;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the window of one output position, forced inside [0, in_size): a table that is wrong cannot make the kernel read out of bounds
__device__ __forceinline__ void window(const int32_t* bounds, int pos, int in_size, int ksize, int& lo, int& n) {
    lo = bounds[2 * pos];
    n = bounds[2 * pos + 1];
    lo = lo < 0 ? 0 : (lo > in_size ? in_size : lo);
    n = n < 0 ? 0 : (n > ksize ? ksize : n);
    n = n > in_size - lo ? in_size - lo : n;
}

// horizontal pass: src [rows][in_w][3] -> dst [rows][out_w][3]; a lane owns output pixels 4 g .. 4 g + 3 of one row
template <bool VEC>
__global__ void __launch_bounds__(256) resize_h_kernel(const uint8_t* src, uint8_t* dst, int rows, int in_w, int out_w,
                                                       const int32_t* bounds, const int32_t* coefs, int ksize) {
    const int groups = (out_w + 3) >> 2;
    const int64_t total = (int64_t)rows * groups;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        const uint8_t* line = src + (int64_t)y * in_w * 3;
        uint32_t px[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
            if (x0 + j < out_w) {
                int lo, n;
                window(bounds, x0 + j, in_w, ksize, lo, n);
                const int32_t* k = coefs + (int64_t)(x0 + j) * ksize;
                const uint8_t* p = line + lo * 3;
                for (int t = 0; t < n; ++t) {
                    const int c = k[t];
                    a0 += (int)p[3 * t] * c;
                    a1 += (int)p[3 * t + 1] * c;
                    a2 += (int)p[3 * t + 2] * c;
                }
            }
            px[j][0] = clip8(a0), px[j][1] = clip8(a1), px[j][2] = clip8(a2);
        }
        uint8_t* o = dst + ((int64_t)y * out_w + x0) * 3;
        if (VEC) {      // out_w % 4 == 0 and a 4-byte aligned dst: the twelve bytes are three aligned dwords
            uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
            o32[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24;
            o32[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24;
            o32[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < out_w) {
                    o[3 * j] = (uint8_t)px[j][0];
                    o[3 * j + 1] = (uint8_t)px[j][1];
                    o[3 * j + 2] = (uint8_t)px[j][2];
                }
        }
    }
}

// vertical pass: src [in_h][row_bytes] -> dst [out_h][row_bytes] (row_bytes = 3 w: the channels need no telling apart); a lane
// owns bytes 4 g .. 4 g + 3 of one output row, the window and its coefficients are the same for the whole row
template <bool VEC>
__global__ void __launch_bounds__(256) resize_v_kernel(const uint8_t* src, uint8_t* dst, int in_h, int out_h, int row_bytes,
                                                       const int32_t* bounds, const int32_t* coefs, int ksize) {
    const int groups = (row_bytes + 3) >> 2;
    const int64_t total = (int64_t)out_h * groups;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        int lo, n;
        window(bounds, y, in_h, ksize, lo, n);
        const int32_t* k = coefs + (int64_t)y * ksize;
        const uint8_t* p = src + (int64_t)lo * row_bytes + x0;
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0, a3 = a0;
        if (VEC) {      // row_bytes % 4 == 0 and 4-byte aligned src / dst
            for (int t = 0; t < n; ++t) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(p + (int64_t)t * row_bytes);
                const int c = k[t];
                a0 += (int)(v & 255u) * c;
                a1 += (int)((v >> 8) & 255u) * c;
                a2 += (int)((v >> 16) & 255u) * c;
                a3 += (int)(v >> 24) * c;
            }
            *reinterpret_cast<uint32_t*>(dst + (int64_t)y * row_bytes + x0) = clip8(a0) | clip8(a1) << 8 | clip8(a2) << 16 | clip8(a3) << 24;
        } else {
            const bool in1 = x0 + 1 < row_bytes, in2 = x0 + 2 < row_bytes, in3 = x0 + 3 < row_bytes;
            for (int t = 0; t < n; ++t) {
                const uint8_t* q = p + (int64_t)t * row_bytes;
                const int c = k[t];
                a0 += (int)q[0] * c;
                if (in1) a1 += (int)q[1] * c;
                if (in2) a2 += (int)q[2] * c;
                if (in3) a3 += (int)q[3] * c;
            }
            uint8_t* o = dst + (int64_t)y * row_bytes + x0;
            o[0] = (uint8_t)clip8(a0);
            if (in1) o[1] = (uint8_t)clip8(a1);
            if (in2) o[2] = (uint8_t)clip8(a2);
            if (in3) o[3] = (uint8_t)clip8(a3);
        }
    }
}

// one source image into slot b: a lane owns pixels 4 g .. 4 g + 3 of one row of the H x W slot, all three planes.
// U8: uint8 source through the 256-entry table (staged in LDS once per workgroup); else an fp32 source, copied.
// VEC_SRC: w % 4 == 0 and an aligned source (twelve source elements of a lane inside the image are three dwords / float4).
// VEC_DST: W % 4 == 0 and a 16-byte aligned batch.
template <bool U8, bool VEC_SRC, bool VEC_DST>
__global__ void __launch_bounds__(256) ingest_kernel(const void* src_, int h, int w, float* slot, int H, int W, int replicate,
                                                     const float* table) {
    __shared__ float tab[256];
    if (U8) {
        tab[threadIdx.x] = table[threadIdx.x];
        __syncthreads();
    }
    const int groups = (W + 3) >> 2;
    const int64_t total = (int64_t)H * groups, plane = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        const int ys = y < h ? y : h - 1;
        float v[4][3];
        if (VEC_SRC && y < h && x0 + 3 < w) {
            const int64_t e = ((int64_t)ys * w + x0) * 3;
            if (U8) {
                const uint32_t* s = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(src_) + e);
                const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
                v[0][0] = tab[d0 & 255u], v[0][1] = tab[(d0 >> 8) & 255u], v[0][2] = tab[(d0 >> 16) & 255u];
                v[1][0] = tab[d0 >> 24], v[1][1] = tab[d1 & 255u], v[1][2] = tab[(d1 >> 8) & 255u];
                v[2][0] = tab[(d1 >> 16) & 255u], v[2][1] = tab[d1 >> 24], v[2][2] = tab[d2 & 255u];
                v[3][0] = tab[(d2 >> 8) & 255u], v[3][1] = tab[(d2 >> 16) & 255u], v[3][2] = tab[d2 >> 24];
            } else {
                const f32x4* s = reinterpret_cast<const f32x4*>(static_cast<const float*>(src_) + e);
                const f32x4 d0 = s[0], d1 = s[1], d2 = s[2];
                v[0][0] = d0.x, v[0][1] = d0.y, v[0][2] = d0.z;
                v[1][0] = d0.w, v[1][1] = d1.x, v[1][2] = d1.y;
                v[2][0] = d1.z, v[2][1] = d1.w, v[2][2] = d2.x;
                v[3][0] = d2.y, v[3][1] = d2.z, v[3][2] = d2.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                const bool inside = y < h && x < w;
                const int xs = x < w ? x : w - 1;
                const int64_t e = ((int64_t)ys * w + xs) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float val = 0.0f;
                    if (inside || replicate)
                        val = U8 ? tab[static_cast<const uint8_t*>(src_)[e + c]] : static_cast<const float*>(src_)[e + c];
                    v[j][c] = val;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = slot + c * plane + (int64_t)y * W + x0;
            if (VEC_DST) {
                *reinterpret_cast<f32x4*>(o) = f32x4{v[0][c], v[1][c], v[2][c], v[3][c]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < W) o[j] = v[j][c];
            }
        }
    }
}

// save_image's quantisation: trunc(clamp(x * 255 + 0.5, 0, 255)), written with HIP's __f*_rn forms and NOT with glue.h's mul_rn /
// add_rn: as compiled today the product and the sum are one v_fma_f32 (DESIGN.md "glue.h"), and the shared operators would un-fuse
// it and change output bytes.  fmaxf(NaN, 0) = 0: a NaN pixel is written as 0.
__device__ __forceinline__ uint32_t quant8(float x) {
    const float t = __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
    return (uint32_t)fminf(fmaxf(t, 0.0f), 255.0f);
}

// image b's top-left h x w crop -> uint8 HWC: a lane owns pixels 4 g .. 4 g + 3 of one row.
// VEC_SRC: W % 4 == 0 and a 16-byte aligned batch; VEC_DST: w % 4 == 0 and a 4-byte aligned dst.
template <bool VEC_SRC, bool VEC_DST>
__global__ void __launch_bounds__(256) emit_kernel(const float* slot, int H, int W, uint8_t* dst, int h, int w) {
    const int groups = (w + 3) >> 2;
    const int64_t total = (int64_t)h * groups, plane = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        uint32_t q[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* s = slot + c * plane + (int64_t)y * W + x0;
            if (VEC_SRC) {      // x0 + 3 < W always: x0 < w <= W and both W and x0 are multiples of 4
                const f32x4 d = *reinterpret_cast<const f32x4*>(s);
                q[0][c] = quant8(d.x), q[1][c] = quant8(d.y), q[2][c] = quant8(d.z), q[3][c] = quant8(d.w);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j][c] = x0 + j < w ? quant8(s[j]) : 0u;
            }
        }
        uint8_t* o = dst + ((int64_t)y * w + x0) * 3;
        if (VEC_DST) {
            uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
            o32[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[1][0] << 24;
            o32[1] = q[1][1] | q[1][2] << 8 | q[2][0] << 16 | q[2][1] << 24;
            o32[2] = q[2][2] | q[3][0] << 8 | q[3][1] << 16 | q[3][2] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < w) {
                    o[3 * j] = (uint8_t)q[j][0];
                    o[3 * j + 1] = (uint8_t)q[j][1];
                    o[3 * j + 2] = (uint8_t)q[j][2];
                }
        }
    }
}

// fixed-order sum of the 256 values of a workgroup (fp64 through LDS: the same tree on every run)
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double y601(double r, double g, double b) {
    return (65.481 * r + 128.553 * g + 24.966 * b + 16.0) / 255.0;
}

// partials[image][block]: workgroup (block, image) sums, in fp64, the squared differences of the groups of four columns
// block * 256 + lane, + kSqBlocks * 256, ... of its image's rows; a group is four columns 4 q .. 4 q + 3 of the W-wide buffer
// row, masked to the valid cropped columns [cb, w_i - cb).  Y: one item per (row, group) over the BT.601 luma of both images;
// else one item per (plane, row, group).  Which lane adds what, and in which order, depends on the shapes alone.
template <bool Y, bool VEC>
__global__ void __launch_bounds__(256) sqdiff_kernel(const float* a, const float* b, int H, int W, const int32_t* sizes, int cb,
                                                     double* partials) {
    __shared__ double red[256];
    const int img = blockIdx.y;
    int h = sizes ? sizes[2 * img] : H, w = sizes ? sizes[2 * img + 1] : W;
    h = h < 0 ? 0 : (h > H ? H : h);
    w = w < 0 ? 0 : (w > W ? W : w);
    const int rows = h - 2 * cb > 0 ? h - 2 * cb : 0, x_lo = cb, x_hi = w - cb;
    const int groups = (W + 3) >> 2;
    const int64_t plane = (int64_t)H * W, total = (int64_t)(Y ? 1 : 3) * rows * groups;
    const float* ia = a + 3 * plane * img;
    const float* ib = b + 3 * plane * img;
    double acc = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)kSqBlocks * 256) {
        const int64_t r = g / groups;
        const int x0 = (int)(g - r * groups) << 2;
        if (x0 + 3 < x_lo || x0 >= x_hi) continue;
        const int c = (int)(r / rows), y = (int)(r - (int64_t)c * rows) + cb;       // (Y: c == 0)
        const int64_t e = c * plane + (int64_t)y * W + x0;
        float va[3][4], vb[3][4];
#pragma unroll
        for (int p = 0; p < (Y ? 3 : 1); ++p) {
            if (VEC) {
                const f32x4 da = *reinterpret_cast<const f32x4*>(ia + e + p * plane), db = *reinterpret_cast<const f32x4*>(ib + e + p * plane);
                va[p][0] = da.x, va[p][1] = da.y, va[p][2] = da.z, va[p][3] = da.w;
                vb[p][0] = db.x, vb[p][1] = db.y, vb[p][2] = db.z, vb[p][3] = db.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = x0 + j < W;
                    va[p][j] = in ? ia[e + p * plane + j] : 0.0f;
                    vb[p][j] = in ? ib[e + p * plane + j] : 0.0f;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double d;
            if (Y)
                d = y601((double)va[0][j], (double)va[1][j], (double)va[2][j]) - y601((double)vb[0][j], (double)vb[1][j], (double)vb[2][j]);
            else
                d = (double)va[0][j] - (double)vb[0][j];
            if (x0 + j >= x_lo && x0 + j < x_hi) acc += d * d;
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[(int64_t)img * kSqBlocks + blockIdx.x] = s;
}

// the finishing workgroup: out[i] = the kSqBlocks partials of image i added as a fixed tree
__global__ void __launch_bounds__(256) sqdiff_finish_kernel(const double* partials, double* out, int B) {
    __shared__ double red[256];
    for (int i = 0; i < B; ++i) {
        const double s = block_sum((int)threadIdx.x < kSqBlocks ? partials[(int64_t)i * kSqBlocks + threadIdx.x] : 0.0, red);
        if (threadIdx.x == 0) out[i] = s;
        __syncthreads();
    }
}

// ---- the ragged batch forms: workgroup column blockIdx.y works on image blockIdx.y of a device array of edtr_image_desc ----------
// Every choice that a per-image entry point makes on the host (which passes run, the dword forms) is made here per image from its
// descriptor; it is uniform over a workgroup.  The arithmetic is that of resize_h_kernel / resize_v_kernel / ingest_kernel /
// emit_kernel, through the same window / clip8 / quant8 and the same table.

// the twelve bytes of pixels 4 g .. 4 g + 3 of one output row of the horizontal pass
template <bool VEC>
__device__ __forceinline__ void resize_h_group(const uint8_t* line, uint8_t* o, int x0, int in_w, int out_w, const int32_t* bounds,
                                               const int32_t* coefs, int ksize) {
    uint32_t px[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
        if (x0 + j < out_w) {
            int lo, n;
            window(bounds, x0 + j, in_w, ksize, lo, n);
            const int32_t* k = coefs + (int64_t)(x0 + j) * ksize;
            const uint8_t* p = line + lo * 3;
            for (int t = 0; t < n; ++t) {
                const int c = k[t];
                a0 += (int)p[3 * t] * c;
                a1 += (int)p[3 * t + 1] * c;
                a2 += (int)p[3 * t + 2] * c;
            }
        }
        px[j][0] = clip8(a0), px[j][1] = clip8(a1), px[j][2] = clip8(a2);
    }
    if (VEC) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
        o32[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24;
        o32[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24;
        o32[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < out_w) {
                o[3 * j] = (uint8_t)px[j][0];
                o[3 * j + 1] = (uint8_t)px[j][1];
                o[3 * j + 2] = (uint8_t)px[j][2];
            }
    }
}

// does image d run a horizontal / vertical pass, and does its horizontal result [in_h][out_w][3] lie inside the scratch buffer?
__device__ __forceinline__ bool desc_horiz(const edtr_image_desc& d) { return d.out_w != d.in_w; }
__device__ __forceinline__ bool desc_vert(const edtr_image_desc& d) { return d.out_h != d.in_h; }
__device__ __forceinline__ bool desc_sane(const edtr_image_desc& d, int64_t tmp_bytes, const uint8_t* tmp) {
    if (!d.src || d.in_h <= 0 || d.in_w <= 0 || d.out_h <= 0 || d.out_w <= 0) return false;
    if (desc_horiz(d)) {
        if (!d.h_bounds || !d.h_coefs || d.h_ksize <= 0 || !tmp) return false;
        if (d.tmp_offset < 0 || d.tmp_offset + (int64_t)d.in_h * d.out_w * 3 > tmp_bytes) return false;
    }
    if (desc_vert(d) && (!d.v_bounds || !d.v_coefs || d.v_ksize <= 0)) return false;
    return true;
}

// horizontal pass of every image that has one: src [in_h][in_w][3] -> tmp + tmp_offset [in_h][out_w][3]
__global__ void __launch_bounds__(256) resize_h_batch_kernel(const edtr_image_desc* descs, uint8_t* tmp, int64_t tmp_bytes) {
    const edtr_image_desc d = descs[blockIdx.y];
    if (!desc_sane(d, tmp_bytes, tmp) || !desc_horiz(d)) return;
    uint8_t* dst = tmp + d.tmp_offset;
    const bool vec = d.out_w % 4 == 0 && aligned_to(dst, 4);
    const int groups = (d.out_w + 3) >> 2;
    const int64_t total = (int64_t)d.in_h * groups;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        const uint8_t* line = d.src + (int64_t)y * d.in_w * 3;
        uint8_t* o = dst + ((int64_t)y * d.out_w + x0) * 3;
        if (vec) resize_h_group<true>(line, o, x0, d.in_w, d.out_w, d.h_bounds, d.h_coefs, d.h_ksize);
        else resize_h_group<false>(line, o, x0, d.in_w, d.out_w, d.h_bounds, d.h_coefs, d.h_ksize);
    }
}

// vertical pass (or none) -> table -> slot d.b, padding included: a lane owns pixels 4 g .. 4 g + 3 of one row of the H x W slot in
// all three planes.  The source S [in_h][out_w][3] is the horizontal result where that pass ran, the image itself otherwise.  A slot
// position outside the image takes 0 (replicate = 0) or the value of the nearest image pixel (replicate = 1), which is computed again
// from the same window.  VEC_DST: W % 4 == 0 and a 16-byte aligned batch (per launch); the dword reads of S are chosen per image.
template <bool VEC_DST>
__global__ void __launch_bounds__(256) resize_ingest_batch_kernel(const edtr_image_desc* descs, const uint8_t* tmp, int64_t tmp_bytes,
                                                                  float* batch, int B, int H, int W, int replicate, const float* table) {
    __shared__ float tab[256];
    tab[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const edtr_image_desc d = descs[blockIdx.y];
    if (!desc_sane(d, tmp_bytes, tmp) || d.b < 0 || d.b >= B || d.out_h > H || d.out_w > W) return;
    const uint8_t* S = desc_horiz(d) ? tmp + d.tmp_offset : d.src;
    const bool vert = desc_vert(d);
    const int h = d.out_h, w = d.out_w, row_bytes = w * 3;
    const bool vec_src = row_bytes % 4 == 0 && aligned_to(S, 4);
    const int groups = (W + 3) >> 2;
    const int64_t total = (int64_t)H * groups, plane = (int64_t)H * W;
    float* slot = batch + (int64_t)d.b * 3 * plane;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        const int ys = y < h ? y : h - 1;
        int lo = ys, n = 1;
        const int32_t* k = nullptr;
        if (vert) {
            window(d.v_bounds, ys, d.in_h, d.v_ksize, lo, n);
            k = d.v_coefs + (int64_t)ys * d.v_ksize;
        }
        uint32_t q[4][3];                               // the bytes of the four pixels
        const bool whole = x0 + 3 < w;                  // all four pixels inside the image's columns (the row is ys)
        if (!replicate && (y >= h || x0 >= w)) {        // all four in the zero padding
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j][0] = q[j][1] = q[j][2] = 0u;
        } else if (whole && vec_src) {
            const uint8_t* p = S + (int64_t)lo * row_bytes + x0 * 3;
            if (vert) {
                int a[12];
#pragma unroll
                for (int e = 0; e < 12; ++e) a[e] = 1 << (kPrecisionBits - 1);
                for (int t = 0; t < n; ++t) {
                    const uint32_t* s = reinterpret_cast<const uint32_t*>(p + (int64_t)t * row_bytes);
                    const uint32_t v0 = s[0], v1 = s[1], v2 = s[2];
                    const int c = k[t];
                    a[0] += (int)(v0 & 255u) * c, a[1] += (int)((v0 >> 8) & 255u) * c, a[2] += (int)((v0 >> 16) & 255u) * c, a[3] += (int)(v0 >> 24) * c;
                    a[4] += (int)(v1 & 255u) * c, a[5] += (int)((v1 >> 8) & 255u) * c, a[6] += (int)((v1 >> 16) & 255u) * c, a[7] += (int)(v1 >> 24) * c;
                    a[8] += (int)(v2 & 255u) * c, a[9] += (int)((v2 >> 8) & 255u) * c, a[10] += (int)((v2 >> 16) & 255u) * c, a[11] += (int)(v2 >> 24) * c;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j][0] = clip8(a[3 * j]), q[j][1] = clip8(a[3 * j + 1]), q[j][2] = clip8(a[3 * j + 2]);
            } else {
                const uint32_t* s = reinterpret_cast<const uint32_t*>(p);
                const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
                q[0][0] = d0 & 255u, q[0][1] = (d0 >> 8) & 255u, q[0][2] = (d0 >> 16) & 255u;
                q[1][0] = d0 >> 24, q[1][1] = d1 & 255u, q[1][2] = (d1 >> 8) & 255u;
                q[2][0] = (d1 >> 16) & 255u, q[2][1] = d1 >> 24, q[2][2] = d2 & 255u;
                q[3][0] = (d2 >> 8) & 255u, q[3][1] = (d2 >> 16) & 255u, q[3][2] = d2 >> 24;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                const int xs = x < w ? x : w - 1;
                const uint8_t* p = S + (int64_t)lo * row_bytes + xs * 3;
                if (vert) {
                    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
                    for (int t = 0; t < n; ++t) {
                        const uint8_t* s = p + (int64_t)t * row_bytes;
                        const int c = k[t];
                        a0 += (int)s[0] * c;
                        a1 += (int)s[1] * c;
                        a2 += (int)s[2] * c;
                    }
                    q[j][0] = clip8(a0), q[j][1] = clip8(a1), q[j][2] = clip8(a2);
                } else {
                    q[j][0] = p[0], q[j][1] = p[1], q[j][2] = p[2];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (replicate || (y < h && x0 + j < w)) ? tab[q[j][c]] : 0.0f;
            float* o = slot + c * plane + (int64_t)y * W + x0;
            if (VEC_DST) {
                *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < W) o[j] = v[j];
            }
        }
    }
}

// crop i of the table: image b's top-left h x w -> dst + offset, uint8 HWC.  table[i] = (b, h, w, byte offset), int64.
// VEC_SRC: W % 4 == 0 and a 16-byte aligned batch (per launch); the dword stores are chosen per crop.
template <bool VEC_SRC>
__global__ void __launch_bounds__(256) emit_batch_kernel(const float* batch, int B, int H, int W, const int64_t* table, uint8_t* dst,
                                                         int64_t dst_bytes) {
    const int64_t* row = table + 4 * (int64_t)blockIdx.y;
    const int64_t b = row[0], off = row[3];
    if (b < 0 || b >= B || row[1] <= 0 || row[2] <= 0 || row[1] > H || row[2] > W) return;
    const int h = (int)row[1], w = (int)row[2];
    if (off < 0 || off + (int64_t)h * w * 3 > dst_bytes) return;
    uint8_t* out = dst + off;
    const bool vec_dst = w % 4 == 0 && aligned_to(out, 4);
    const int groups = (w + 3) >> 2;
    const int64_t total = (int64_t)h * groups, plane = (int64_t)H * W;
    const float* slot = batch + b * 3 * plane;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int y = (int)(g / groups), x0 = (int)(g - (int64_t)y * groups) << 2;
        uint32_t q[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* s = slot + c * plane + (int64_t)y * W + x0;
            if (VEC_SRC) {      // x0 + 3 < W always: x0 < w <= W and both W and x0 are multiples of 4
                const f32x4 v = *reinterpret_cast<const f32x4*>(s);
                q[0][c] = quant8(v.x), q[1][c] = quant8(v.y), q[2][c] = quant8(v.z), q[3][c] = quant8(v.w);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j][c] = x0 + j < w ? quant8(s[j]) : 0u;
            }
        }
        uint8_t* o = out + ((int64_t)y * w + x0) * 3;
        if (vec_dst) {
            uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
            o32[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[1][0] << 24;
            o32[1] = q[1][1] | q[1][2] << 8 | q[2][0] << 16 | q[2][1] << 24;
            o32[2] = q[2][2] | q[3][0] << 8 | q[3][1] << 16 | q[3][2] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < w) {
                    o[3 * j] = (uint8_t)q[j][0];
                    o[3 * j + 1] = (uint8_t)q[j][1];
                    o[3 * j + 2] = (uint8_t)q[j][2];
                }
        }
    }
}

}  // namespace

extern "C" int edtr_image_resize_u8(const uint8_t* src, int in_h, int in_w, int channels, uint8_t* dst, int out_h, int out_w,
                                    const int32_t* h_bounds, const int32_t* h_coefs, int h_ksize, const int32_t* v_bounds,
                                    const int32_t* v_coefs, int v_ksize, uint8_t* tmp, edtr_stream_t stream) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!src || !dst) return EDTR_E_NULL;
    if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return EDTR_E_SHAPE;
    if (in_h > (1 << 24) || in_w > (1 << 24) || out_h > (1 << 24) || out_w > (1 << 24)) return EDTR_E_UNSUPPORTED;
    const bool horiz = out_w != in_w, vert = out_h != in_h;
    if (horiz && (!h_bounds || !h_coefs)) return EDTR_E_NULL;
    if (vert && (!v_bounds || !v_coefs)) return EDTR_E_NULL;
    if ((horiz && h_ksize <= 0) || (vert && v_ksize <= 0)) return EDTR_E_SHAPE;
    if (horiz && vert && !tmp) return EDTR_E_NULL;
    if (!all_aligned_to(4, h_bounds, h_coefs, v_bounds, v_coefs)) return EDTR_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!horiz && !vert) {
        const hipError_t e = hipMemcpyAsync(dst, src, (size_t)in_h * in_w * 3, hipMemcpyDeviceToDevice, st);
        return e == hipSuccess ? EDTR_OK : (int)e;                     // (the raw HIP error, as EDTR_LAUNCH_CHECK returns it)
    }
    const uint8_t* vsrc = src;
    if (horiz) {
        uint8_t* hdst = vert ? tmp : dst;
        const int64_t n = (int64_t)in_h * ((out_w + 3) / 4);
        if (out_w % 4 == 0 && aligned_to(hdst, 4))
            hipLaunchKernelGGL(resize_h_kernel<true>, dim3(blocks_for(n)), dim3(256), 0, st, src, hdst, in_h, in_w, out_w, h_bounds, h_coefs, h_ksize);
        else
            hipLaunchKernelGGL(resize_h_kernel<false>, dim3(blocks_for(n)), dim3(256), 0, st, src, hdst, in_h, in_w, out_w, h_bounds, h_coefs, h_ksize);
        EDTR_LAUNCH_CHECK();
        vsrc = hdst;
    }
    if (vert) {
        const int row_bytes = out_w * 3;
        const int64_t n = (int64_t)out_h * ((row_bytes + 3) / 4);
        if (row_bytes % 4 == 0 && aligned_to(vsrc, 4) && aligned_to(dst, 4))
            hipLaunchKernelGGL(resize_v_kernel<true>, dim3(blocks_for(n)), dim3(256), 0, st, vsrc, dst, in_h, out_h, row_bytes, v_bounds, v_coefs, v_ksize);
        else
            hipLaunchKernelGGL(resize_v_kernel<false>, dim3(blocks_for(n)), dim3(256), 0, st, vsrc, dst, in_h, out_h, row_bytes, v_bounds, v_coefs, v_ksize);
        EDTR_LAUNCH_CHECK();
    }
    return EDTR_OK;
}

extern "C" int edtr_image_ingest(int src_f32, const void* src, int h, int w, int channels, float* batch, int b, int B, int H, int W,
                                 int replicate, const float* table, edtr_stream_t stream) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!src || !batch || (!src_f32 && !table)) return EDTR_E_NULL;
    if (h <= 0 || w <= 0 || B <= 0 || b < 0 || b >= B || h > H || w > W) return EDTR_E_SHAPE;
    if ((src_f32 != 0 && src_f32 != 1) || (replicate != 0 && replicate != 1)) return EDTR_E_DTYPE;
    if (!all_aligned_to(4, batch, table) || (src_f32 && !aligned_to(src, 4))) return EDTR_E_ALIGN;
    float* slot = batch + (int64_t)b * 3 * H * W;
    const bool vs = w % 4 == 0 && (src_f32 ? aligned16(src) : aligned_to(src, 4));
    const bool vd = W % 4 == 0 && aligned16(slot);
    const dim3 grid(blocks_for((int64_t)H * ((W + 3) / 4))), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define EDTR_INGEST(U8, VS, VD) hipLaunchKernelGGL((ingest_kernel<U8, VS, VD>), grid, block, 0, st, src, h, w, slot, H, W, replicate, table)
    // three of the four (VS, VD) forms exist: a lane owns four destination columns, so without the wide store (!vd) the wide
    // source read buys nothing and `vs && !vd` takes the element-by-element kernel (emit instantiates all four)
    if (src_f32) {
        if (vs && vd) EDTR_INGEST(false, true, true);
        else if (vd) EDTR_INGEST(false, false, true);
        else EDTR_INGEST(false, false, false);
    } else {
        if (vs && vd) EDTR_INGEST(true, true, true);
        else if (vd) EDTR_INGEST(true, false, true);
        else EDTR_INGEST(true, false, false);
    }
#undef EDTR_INGEST
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_image_emit(const float* batch, int b, int B, int channels, int H, int W, uint8_t* dst, int h, int w,
                               edtr_stream_t stream) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!batch || !dst) return EDTR_E_NULL;
    if (h <= 0 || w <= 0 || B <= 0 || b < 0 || b >= B || h > H || w > W) return EDTR_E_SHAPE;
    if (!aligned_to(batch, 4)) return EDTR_E_ALIGN;
    const float* slot = batch + (int64_t)b * 3 * H * W;
    const bool vs = W % 4 == 0 && aligned16(slot), vd = w % 4 == 0 && aligned_to(dst, 4);
    const dim3 grid(blocks_for((int64_t)h * ((w + 3) / 4))), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vs && vd) hipLaunchKernelGGL((emit_kernel<true, true>), grid, block, 0, st, slot, H, W, dst, h, w);
    else if (vs) hipLaunchKernelGGL((emit_kernel<true, false>), grid, block, 0, st, slot, H, W, dst, h, w);
    else if (vd) hipLaunchKernelGGL((emit_kernel<false, true>), grid, block, 0, st, slot, H, W, dst, h, w);
    else hipLaunchKernelGGL((emit_kernel<false, false>), grid, block, 0, st, slot, H, W, dst, h, w);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

// the host copy of the descriptors is what the arguments are checked on (and what sizes the grid); the kernels read the device copy
static int check_descs(const edtr_image_desc* d, int B, const uint8_t* tmp, int64_t tmp_bytes, int64_t* max_h_groups) {
    int64_t mh = 0;
    for (int i = 0; i < B; ++i) {
        if (!d[i].src) return EDTR_E_NULL;
        if (d[i].in_h <= 0 || d[i].in_w <= 0 || d[i].out_h <= 0 || d[i].out_w <= 0) return EDTR_E_SHAPE;
        if (d[i].in_h > (1 << 24) || d[i].in_w > (1 << 24) || d[i].out_h > (1 << 24) || d[i].out_w > (1 << 24)) return EDTR_E_UNSUPPORTED;
        const bool horiz = d[i].out_w != d[i].in_w, vert = d[i].out_h != d[i].in_h;
        if (horiz && (!d[i].h_bounds || !d[i].h_coefs || !tmp)) return EDTR_E_NULL;
        if (vert && (!d[i].v_bounds || !d[i].v_coefs)) return EDTR_E_NULL;
        if ((horiz && d[i].h_ksize <= 0) || (vert && d[i].v_ksize <= 0)) return EDTR_E_SHAPE;
        if (!all_aligned_to(4, d[i].h_bounds, d[i].h_coefs, d[i].v_bounds, d[i].v_coefs)) return EDTR_E_ALIGN;
        if (horiz) {
            const int64_t bytes = (int64_t)d[i].in_h * d[i].out_w * 3;
            if (d[i].tmp_offset < 0 || d[i].tmp_offset + bytes > tmp_bytes) return EDTR_E_SHAPE;
            const int64_t groups = (int64_t)d[i].in_h * ((d[i].out_w + 3) / 4);
            mh = groups > mh ? groups : mh;
        }
    }
    *max_h_groups = mh;
    return EDTR_OK;
}

extern "C" int edtr_image_resize_h_batch(const edtr_image_desc* descs_host, const edtr_image_desc* descs, int B, int channels,
                                         uint8_t* tmp, int64_t tmp_bytes, edtr_stream_t stream) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!descs_host || !descs) return EDTR_E_NULL;
    if (B <= 0 || B > 65535 || tmp_bytes < 0) return EDTR_E_SHAPE;
    if (!aligned_to(descs, 8)) return EDTR_E_ALIGN;
    int64_t groups = 0;
    const int rc = check_descs(descs_host, B, tmp, tmp_bytes, &groups);
    if (rc != EDTR_OK) return rc;
    if (groups == 0) return EDTR_OK;                    // no image has a horizontal pass: nothing to launch
    hipLaunchKernelGGL(resize_h_batch_kernel, dim3(blocks_for(groups), B), dim3(256), 0, static_cast<hipStream_t>(stream), descs, tmp, tmp_bytes);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_image_resize_ingest_batch(const edtr_image_desc* descs_host, const edtr_image_desc* descs, int B, int channels,
                                              const uint8_t* tmp, int64_t tmp_bytes, float* batch, int slots, int H, int W,
                                              int replicate, const float* table, edtr_stream_t stream) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!descs_host || !descs || !batch || !table) return EDTR_E_NULL;
    if (B <= 0 || B > 65535 || slots <= 0 || H <= 0 || W <= 0 || tmp_bytes < 0) return EDTR_E_SHAPE;
    if (replicate != 0 && replicate != 1) return EDTR_E_DTYPE;
    if (!aligned_to(descs, 8) || !all_aligned_to(4, batch, table)) return EDTR_E_ALIGN;
    int64_t groups = 0;
    const int rc = check_descs(descs_host, B, tmp, tmp_bytes, &groups);
    if (rc != EDTR_OK) return rc;
    for (int i = 0; i < B; ++i)
        if (descs_host[i].b < 0 || descs_host[i].b >= slots || descs_host[i].out_h > H || descs_host[i].out_w > W) return EDTR_E_SHAPE;
    const dim3 grid(blocks_for((int64_t)H * ((W + 3) / 4)), B), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (W % 4 == 0 && aligned16(batch))
        hipLaunchKernelGGL(resize_ingest_batch_kernel<true>, grid, block, 0, st, descs, tmp, tmp_bytes, batch, slots, H, W, replicate, table);
    else
        hipLaunchKernelGGL(resize_ingest_batch_kernel<false>, grid, block, 0, st, descs, tmp, tmp_bytes, batch, slots, H, W, replicate, table);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_image_emit_batch(const float* batch, int B, int channels, int H, int W, const int64_t* table_host,
                                     const int64_t* table, int n, uint8_t* dst, int64_t dst_bytes, edtr_stream_t stream) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!batch || !table_host || !table || !dst) return EDTR_E_NULL;
    if (B <= 0 || n <= 0 || n > 65535 || H <= 0 || W <= 0 || dst_bytes < 0) return EDTR_E_SHAPE;
    if (!aligned_to(batch, 4) || !aligned_to(table, 8)) return EDTR_E_ALIGN;
    int64_t groups = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t b = table_host[4 * i], h = table_host[4 * i + 1], w = table_host[4 * i + 2], off = table_host[4 * i + 3];
        if (b < 0 || b >= B || h <= 0 || w <= 0 || h > H || w > W) return EDTR_E_SHAPE;
        if (off < 0 || off + h * w * 3 > dst_bytes) return EDTR_E_SHAPE;
        if (off & 3) return EDTR_E_ALIGN;
        const int64_t gi = h * ((w + 3) / 4);
        groups = gi > groups ? gi : groups;
    }
    const dim3 grid(blocks_for(groups), n), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (W % 4 == 0 && aligned16(batch)) hipLaunchKernelGGL(emit_batch_kernel<true>, grid, block, 0, st, batch, B, H, W, table, dst, dst_bytes);
    else hipLaunchKernelGGL(emit_batch_kernel<false>, grid, block, 0, st, batch, B, H, W, table, dst, dst_bytes);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_image_sqdiff(const float* a, const float* b, int B, int channels, int H, int W, const int32_t* sizes,
                                 int crop_border, int y_channel, double* partials, double* out, edtr_stream_t stream) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!a || !b || !partials || !out) return EDTR_E_NULL;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || crop_border < 0) return EDTR_E_SHAPE;
    if (y_channel != 0 && y_channel != 1) return EDTR_E_DTYPE;
    if (!all_aligned_to(4, a, b, sizes) || !all_aligned_to(8, partials, out)) return EDTR_E_ALIGN;
    static_assert(kSqBlocks == EDTR_SQDIFF_BLOCKS, "edtr_hip.h and imageio.hip disagree on the partials per image");
    const bool vec = W % 4 == 0 && aligned16(a) && aligned16(b);
    const dim3 grid(kSqBlocks, B), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (y_channel) {
        if (vec) hipLaunchKernelGGL((sqdiff_kernel<true, true>), grid, block, 0, st, a, b, H, W, sizes, crop_border, partials);
        else hipLaunchKernelGGL((sqdiff_kernel<true, false>), grid, block, 0, st, a, b, H, W, sizes, crop_border, partials);
    } else {
        if (vec) hipLaunchKernelGGL((sqdiff_kernel<false, true>), grid, block, 0, st, a, b, H, W, sizes, crop_border, partials);
        else hipLaunchKernelGGL((sqdiff_kernel<false, false>), grid, block, 0, st, a, b, H, W, sizes, crop_border, partials);
    }
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sqdiff_finish_kernel, dim3(1), dim3(256), 0, st, partials, out, B);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
