// The rest of the second-order Real-ESRGAN chain (edtr_hip.h "Low-quality inputs", second part; the host restatements are
// edtr_amd/degrade.py): Poisson noise by table inversion on the seeded stream, the separable blur of USM sharpening and its blend.
// The rule of degrade.hip holds: every product, sum and quotient that decides a result bit is a correctly rounded fp32 operation in
// a stated order (compiled with contraction switched off) or integer arithmetic, so numpy repeats each kernel bit for bit.
#include "common.h"
#include "glue.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSepTile = 32;                // output tile edge of the separable blur: 256 lanes x 4 rows
constexpr int kSepKMin = 3, kSepKMax = 63;
constexpr int kMidPitch = 32;               // row pitch of the rows-pass intermediate (see sepblur_kernel)
constexpr int kLevelWords = 16;             // presence bitmap of an image: words 0..7 colour levels, 8..15 grey levels

// ---- separable blur ---------------------------------------------------------------------------------------------------------------

// workgroup (tile, channel, image).  LDS: the 32 x 32 output tile's input patch with its halo, tile[th][th] with th = 32 + k - 1; the
// taps; and the rows-pass intermediate mid[th][32] (one value per patch row and output column).  Rows pass: lane (tx, ty) owns
// column tx of patch rows ty, ty + 8, ...; columns pass: lane (tx, ty) owns output rows ty, ty + 8, ty + 16, ty + 24 of column tx.
// Bank conflicts: in both passes the 32 lanes of a half wave (the conflict group of a 4-byte LDS read) share ty and differ in tx, so
// one read touches 32 CONSECUTIVE floats of one row.  With the intermediate's pitch at 32 floats = the 32 banks of such a read, a
// column-pass read at row (ty + ky) is mid[(ty + ky) * 32 + tx]: bank tx, each bank once, whatever ky.  (The column walk moves by
// whole rows, i.e. by multiples of 32 banks, which is exactly what keeps lane tx on bank tx; a padded pitch would gain nothing.)
__global__ void __launch_bounds__(256) sepblur_kernel(const float* x, float* out, float* mask_out, int H, int W, const float* taps, int k,
                                                      float threshold, int tiles_x) {
    extern __shared__ float lds[];
    const int th = kSepTile + k - 1, r = k >> 1;
    float* tile = lds;                      // [th][th]
    float* mid = lds + th * th;             // [th][kMidPitch]
    float* g = mid + th * kMidPitch;        // [k]
    const int b = blockIdx.z, c = blockIdx.y;
    const int ty0 = ((int)blockIdx.x / tiles_x) * kSepTile, tx0 = ((int)blockIdx.x % tiles_x) * kSepTile;
    const int64_t plane_off = ((int64_t)b * 3 + c) * H * W;
    const float* plane = x + plane_off;
    for (int i = threadIdx.x; i < k; i += 256) g[i] = taps[i];
    for (int i = threadIdx.x; i < th * th; i += 256) {
        const int ly = i / th, lx = i - ly * th;
        tile[i] = plane[(int64_t)reflect(ty0 + ly - r, H) * W + reflect(tx0 + lx - r, W)];
    }
    __syncthreads();
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int row = ty; row < th; row += 8) {
        const float* p = tile + row * th + tx;
        float t = 0.0f;
        for (int kx = 0; kx < k; ++kx) t = add_rn(t, mul_rn(p[kx], g[kx]));
        mid[row * kMidPitch + tx] = t;
    }
    __syncthreads();
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float* m = mid + ty * kMidPitch + tx;
    for (int ky = 0; ky < k; ++ky) {
        const float w = g[ky];
        a0 = add_rn(a0, mul_rn(m[ky * kMidPitch], w));
        a1 = add_rn(a1, mul_rn(m[(ky + 8) * kMidPitch], w));
        a2 = add_rn(a2, mul_rn(m[(ky + 16) * kMidPitch], w));
        a3 = add_rn(a3, mul_rn(m[(ky + 24) * kMidPitch], w));
    }
    const int gx = tx0 + tx;
    if (gx >= W) return;
    const float acc[4] = {a0, a1, a2, a3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gy = ty0 + ty + 8 * j;
        if (gy >= H) continue;
        const int64_t e = plane_off + (int64_t)gy * W + gx;
        out[e] = acc[j];
        if (mask_out) {
            const float xv = tile[(ty + 8 * j + r) * th + tx + r];
            mask_out[e] = mul_rn(fabsf(add_rn(xv, -acc[j])), 255.0f) > threshold ? 1.0f : 0.0f;
        }
    }
}

// sharp = clamp(x + weight (x - blur), 0, 1);  out = soft sharp + (1 - soft) x
__global__ void __launch_bounds__(256) usm_apply_kernel(const float* x, const float* blur, const float* soft, float* out, float weight,
                                                        int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float xv = x[e], s = soft[e];
        const float sharp = fminf(fmaxf(add_rn(xv, mul_rn(weight, add_rn(xv, -blur[e]))), 0.0f), 1.0f);
        out[e] = add_rn(mul_rn(s, sharp), mul_rn(add_rn(1.0f, -s), xv));
    }
}

// ---- Poisson noise ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int level_of(float v) { return (int)level8(v); }
// torchvision's rgb_to_grayscale: (0.2989 r + 0.587 g) + 0.114 b
__device__ __forceinline__ float grey_of(float r, float g, float b) {
    return add_rn(add_rn(mul_rn(0.2989f, r), mul_rn(0.587f, g)), mul_rn(0.114f, b));
}

__global__ void __launch_bounds__(256) zero_levels_kernel(uint32_t* levels, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) levels[i] = 0u;
}

// (a level that is already marked needs no atomic: the plain read may be stale, which only costs an atomic that changes nothing)
__device__ __forceinline__ void mark(uint32_t* bits, int k) {
    const uint32_t bit = 1u << (k & 31);
    if (!(reinterpret_cast<volatile uint32_t*>(bits)[k >> 5] & bit)) atomicOr(bits + (k >> 5), bit);
}

// grid (blocks, image): a workgroup marks the levels of its share of the image's pixels in an LDS bitmap (LDS atomics), then ORs its
// 16 words into the image's bitmap in memory (vector atomics).  An OR is order-free: the bitmap is the same on every run.
__global__ void __launch_bounds__(256) levels_kernel(const float* x, uint32_t* levels, int64_t plane) {
    __shared__ uint32_t bits[kLevelWords];
    if (threadIdx.x < kLevelWords) bits[threadIdx.x] = 0u;
    __syncthreads();
    const float* img = x + (int64_t)blockIdx.y * 3 * plane;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < plane; e += (int64_t)gridDim.x * 256) {
        const float r = img[e], g = img[plane + e], b = img[2 * plane + e];
        mark(bits, level_of(r));
        mark(bits, level_of(g));
        mark(bits, level_of(b));
        mark(bits + 8, level_of(grey_of(r, g, b)));
    }
    __syncthreads();
    if (threadIdx.x < kLevelWords && bits[threadIdx.x]) atomicOr(levels + (int64_t)blockIdx.y * kLevelWords + threadIdx.x, bits[threadIdx.x]);
}

// n = lo + #{ j < 255 : row[j] <= u }: eight steps over the non-decreasing row, the last index read is 254
__device__ __forceinline__ int invert(const uint32_t* row, int lo, uint32_t u) {
    int pos = 0;
#pragma unroll
    for (int step = 128; step >= 1; step >>= 1)
        if (row[pos + step - 1] <= u) pos += step;
    return lo + pos;
}

// a lane owns four consecutive elements of one plane = one Philox call, as noise_kernel of degrade.hip; the element's uniform is the
// raw word x[e & 3].  Colour: level and counter group from the element of the [3][H][W] image; grey: from the pixel of the [H][W]
// grey plane, so the three channels of a pixel receive the same noise.
__global__ void __launch_bounds__(256) poisson_kernel(const float* x, float* out, float* noise_out, const float* scale, const int32_t* gray,
                                                      const uint32_t* levels, const uint32_t* tables, const int32_t* lows, int32_t* counts_out,
                                                      NoiseArgs a, int64_t n4) {
    const int64_t per4 = 3 * a.plane4;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / per4;
        int64_t eg = g - b * per4;
        const bool grey = gray[b] != 0;
        const uint32_t* lv = levels + b * kLevelWords;
        int cc = 0, cg = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            cc += __popc(lv[i]);
            cg += __popc(lv[8 + i]);
        }
        if (counts_out && eg == 0) {
            counts_out[2 * b] = cc;
            counts_out[2 * b + 1] = cg;
        }
        const int count = grey ? cg : cc;
        const int lg = count <= 1 ? 0 : 32 - __clz(count - 1);          // vals = 2^ceil(log2(count)) = 1 << lg, lg in 0..8
        const float vals = (float)(1 << lg);
        const uint32_t* T = tables + (int64_t)lg * 65536;
        const int32_t* lo = lows + lg * 256;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + g * 4);
        f32x4 src = xv;
        if (grey) {
            eg %= a.plane4;
            const float* img = x + b * per4 * 4;
            const f32x4 r = *reinterpret_cast<const f32x4*>(img + eg * 4);
            const f32x4 gg = *reinterpret_cast<const f32x4*>(img + (a.plane4 + eg) * 4);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(img + (2 * a.plane4 + eg) * 4);
            src = f32x4{grey_of(r.x, gg.x, bb.x), grey_of(r.y, gg.y, bb.y), grey_of(r.z, gg.z, bb.z), grey_of(r.w, gg.w, bb.w)};
        }
        const uint32_t id = EDTR_IMAGE_ID(a, b);
        const u32x4 w = philox4x32_10(u32x4{(uint32_t)eg, a.draw, grey ? (uint32_t)EDTR_NOISE_DEGRADE_POISSON_GRAY : (uint32_t)EDTR_NOISE_DEGRADE_POISSON, id},
                                      a.k0, a.k1);
        const float s = scale[b];
        const float sv[4] = {src.x, src.y, src.z, src.w}, xs[4] = {xv.x, xv.y, xv.z, xv.w};
        const uint32_t us[4] = {w.x, w.y, w.z, w.w};
        float nz[4], res[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = level_of(sv[i]);
            const float q = div_rn((float)k, 255.0f);
            const int n = invert(T + k * 256, lo[k], us[i]);
            nz[i] = add_rn(div_rn((float)n, vals), -q);
            const float o = add_rn(xs[i], mul_rn(nz[i], s));
            res[i] = a.rounds ? round_to_levels(o) : fminf(fmaxf(o, 0.0f), 1.0f);
        }
        if (noise_out) *reinterpret_cast<f32x4*>(noise_out + g * 4) = f32x4{nz[0], nz[1], nz[2], nz[3]};
        *reinterpret_cast<f32x4*>(out + g * 4) = f32x4{res[0], res[1], res[2], res[3]};
    }
}

}  // namespace

extern "C" int edtr_degrade_sepblur(const float* x, float* out, float* mask_out, int B, int channels, int H, int W, const float* taps, int k,
                                    float threshold, edtr_stream_t stream) {
    if (int rc = check_batch(x, out, B, channels, H, W)) return rc;
    if (!taps) return EDTR_E_NULL;
    if (x == out || x == mask_out || (mask_out && mask_out == out)) return EDTR_E_UNSUPPORTED;      // a tile's halo is another tile's output
    if (k < kSepKMin || k > kSepKMax || !(k & 1)) return EDTR_E_SHAPE;
    if (k / 2 >= (H < W ? H : W)) return EDTR_E_SHAPE;
    if (mask_out && !(threshold == threshold)) return EDTR_E_SHAPE;
    if (!all_aligned_to(4, taps, mask_out)) return EDTR_E_ALIGN;
    const int tiles_x = (W + kSepTile - 1) / kSepTile, tiles_y = (H + kSepTile - 1) / kSepTile;
    if ((int64_t)tiles_x * tiles_y > 0x7fffffff) return EDTR_E_UNSUPPORTED;
    const int th = kSepTile + k - 1;
    const size_t lds = (size_t)(th * th + th * kMidPitch + k) * sizeof(float);      // 47 628 bytes at k = 63
    hipLaunchKernelGGL(sepblur_kernel, dim3(tiles_x * tiles_y, 3, B), dim3(256), lds, static_cast<hipStream_t>(stream), x, out, mask_out,
                       H, W, taps, k, threshold, tiles_x);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_degrade_usm_apply(const float* x, const float* blur, const float* soft, float* out, int B, int channels, int H, int W,
                                      float weight, edtr_stream_t stream) {
    if (int rc = check_batch(x, out, B, channels, H, W)) return rc;
    if (!blur || !soft) return EDTR_E_NULL;
    if (!(weight == weight) || weight > 3.0e38f || weight < -3.0e38f) return EDTR_E_SHAPE;
    if (!all_aligned_to(4, blur, soft)) return EDTR_E_ALIGN;
    const int64_t n = (int64_t)B * 3 * H * W;
    hipLaunchKernelGGL(usm_apply_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, blur, soft, out, weight, n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_degrade_poisson_noise(const float* x, float* out, float* noise_out, int B, int channels, int H, int W,
                                          const float* scale_host, const float* scale, const int32_t* gray_host, const int32_t* gray,
                                          const uint32_t* tables, const int32_t* lows, int32_t* levels, int32_t* counts_out, uint64_t seed,
                                          const int64_t* image_ids, int64_t image_id_base, int64_t draw, int rounds, edtr_stream_t stream) {
    if (int rc = check_batch(x, out, B, channels, H, W)) return rc;
    if (!scale_host || !scale || !gray_host || !gray || !tables || !lows || !levels) return EDTR_E_NULL;
    NoiseArgs a;
    if (int rc = make_noise_args(a, x, out, noise_out, B, H, W, scale_host, gray_host, seed, image_ids, image_id_base, draw, rounds)) return rc;
    if (!all_aligned_to(4, scale, gray, tables, lows, levels, counts_out)) return EDTR_E_ALIGN;
    if (x == out) return EDTR_E_UNSUPPORTED;        // a grey image's lanes read all three channels of a pixel, which another lane writes
    if (static_cast<const void*>(levels) == x || static_cast<const void*>(levels) == out) return EDTR_E_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* lv = reinterpret_cast<uint32_t*>(levels);
    hipLaunchKernelGGL(zero_levels_kernel, dim3((B * kLevelWords + 255) / 256), dim3(256), 0, st, lv, B * kLevelWords);
    EDTR_LAUNCH_CHECK();
    const int64_t hw = (int64_t)H * W;
    const unsigned per_image = blocks_for(hw) < 64u ? blocks_for(hw) : 64u;
    hipLaunchKernelGGL(levels_kernel, dim3(per_image, B), dim3(256), 0, st, x, lv, hw);
    EDTR_LAUNCH_CHECK();
    const int64_t n4 = (int64_t)B * 3 * a.plane4;
    hipLaunchKernelGGL(poisson_kernel, dim3(blocks_for(n4)), dim3(256), 0, st, x, out, noise_out, scale, gray, lv, tables, lows, counts_out, a,
                       n4);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
