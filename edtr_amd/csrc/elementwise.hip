// Layout conversion and small elementwise kernels (HBM-bound or negligible) + runtime helpers.
#include "common.h"
#include "glue.h"
#include "noise_elem.h"
#include <string.h>
#include <algorithm>
#include <vector>

namespace {

// NCHW fp32 -> NHWC 16-bit through an LDS transpose tile: reads are contiguous along pixels,
// writes are contiguous along channels.  grid (ceil(HW/64), B), 256 threads.
template <typename T>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* src, int C, int64_t HW, typename T::elem* dst, int ld,
                                                          int coff, int cpad, float scale, float shift) {
    __shared__ float tile[64][65];
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c0 = 0; c0 < cpad; c0 += 64) {
        for (int cc = ty; cc < 64; cc += 4) {
            const int c = c0 + cc;
            float v = 0.0f;
            if (c < C && p0 + tx < HW) v = src[((int64_t)b * C + c) * HW + p0 + tx] * scale + shift;
            tile[cc][tx] = v;
        }
        __syncthreads();
        for (int pp = ty; pp < 64; pp += 4) {
            const int c = c0 + tx;
            if (c < cpad && p0 + pp < HW) dst[((int64_t)b * HW + p0 + pp) * ld + coff + c] = T::from_f32(tile[tx][pp]);
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const void* src, int src_f32, int C, int64_t HW, int ld,
                                                          float* dst, float scale) {
    __shared__ float tile[64][65];
    const int b = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c0 = 0; c0 < C; c0 += 64) {
        for (int pp = ty; pp < 64; pp += 4) {
            const int c = c0 + tx;
            float v = 0.0f;
            if (c < C && p0 + pp < HW) {
                const int64_t idx = ((int64_t)b * HW + p0 + pp) * ld + c;
                v = src_f32 ? static_cast<const float*>(src)[idx] : T::to_f32(static_cast<const uint16_t*>(src)[idx]);
            }
            tile[pp][tx] = v;
        }
        __syncthreads();
        for (int cc = ty; cc < 64; cc += 4) {
            const int c = c0 + cc;
            if (c < C && p0 + tx < HW) dst[((int64_t)b * C + c) * HW + p0 + tx] = tile[tx][cc] * scale;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(256) add_kernel(const uint16_t* a, int lda, const uint16_t* b, int ldb, uint16_t* out,
                                                 int ldo, int64_t rows, int CV) {
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / CV;
        const int cv = (int)(i - r * CV);
        U4 va = ldg16(a + r * lda + cv * 8);
        if (b) {
            float fa[8], fb[8];
            unpack8<T>(va, fa);
            unpack8<T>(ldg16(b + r * ldb + cv * 8), fb);
#pragma unroll
            for (int j = 0; j < 8; ++j) fa[j] += fb[j];
            va = pack8<T>(fa);
        }
        stg16(out + r * ldo + cv * 8, va);
    }
}

// a (+ b) -> out with the per-slot column statistics of the result in edtr_igemm's gn_partial format (edtr_hip.h: edtr_add_stats): a block
// owns one slot of SR rows x 32 columns — thread (row lane, column group of 8) like the split-K reducer that writes statistics.
template <typename T>
__global__ void __launch_bounds__(256) add_stats_kernel(const uint16_t* a, int lda, const uint16_t* b, int ldb, uint16_t* out, int ldo, int C,
                                                       float* gn_partial, int gn_ld, int SR) {
    __shared__ float red[64][4][16];
    const int tid = threadIdx.x, g = tid & 3, rl = tid >> 2;
    const int n = blockIdx.x * 32 + g * 8;
    const int64_t m_base = (int64_t)blockIdx.y * SR;
    float cs[8], cq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cs[j] = 0.0f; cq[j] = 0.0f; }
    if (n < C) {
        for (int64_t m = m_base + rl; m < m_base + SR; m += 64) {
            float fa[8];
            const U4 va = ldg16(a + m * lda + n);
            unpack8<T>(va, fa);
            if (b) {
                float fb[8];
                unpack8<T>(ldg16(b + m * ldb + n), fb);
#pragma unroll
                for (int j = 0; j < 8; ++j) fa[j] += fb[j];
                stg16(out + m * ldo + n, pack8<T>(fa));
            } else {
                stg16(out + m * ldo + n, va);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { cs[j] += fa[j]; cq[j] += fa[j] * fa[j]; }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[rl][g][j] = cs[j]; red[rl][g][8 + j] = cq[j]; }
    __syncthreads();
    if (tid < 32 && blockIdx.x * 32 + tid < C) {
        const int gg = tid >> 3, j = tid & 7;
        float s = 0.0f, q = 0.0f;
        for (int r = 0; r < 64; ++r) { s += red[r][gg][j]; q += red[r][gg][8 + j]; }
        float* dst = gn_partial + ((int64_t)blockIdx.y * gn_ld + blockIdx.x * 32 + tid) * 2;
        dst[0] = s;
        dst[1] = q;
    }
}

// fp32 a (+ b) -> fp32 out, row-strided (high-precision activation stream)
__global__ void __launch_bounds__(256) add_f32_kernel(const float* a, int lda, const float* b, int ldb, float* out, int ldo,
                                                     int64_t rows, int CV4) {
    const int64_t total = rows * CV4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / CV4;
        const int cv = (int)(i - r * CV4);
        f32x4 va = *reinterpret_cast<const f32x4*>(a + r * lda + cv * 4);
        if (b) va += *reinterpret_cast<const f32x4*>(b + r * ldb + cv * 4);
        *reinterpret_cast<f32x4*>(out + r * ldo + cv * 4) = va;
    }
}

// fp32 a (+ b) -> fp32 out AND its fp16 mirror (the one-part GEMM operand of the mixed-precision mode), 8 columns per thread
__global__ void __launch_bounds__(256) add_f32_mirror_kernel(const float* a, int lda, const float* b, int ldb, float* out, int ldo,
                                                            uint16_t* out16, int ld16, int64_t rows, int CV) {
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / CV;
        const int cv = (int)(i - r * CV);
        f32x4 v0 = *reinterpret_cast<const f32x4*>(a + r * lda + cv * 8), v1 = *reinterpret_cast<const f32x4*>(a + r * lda + cv * 8 + 4);
        if (b) {
            v0 += *reinterpret_cast<const f32x4*>(b + r * ldb + cv * 8);
            v1 += *reinterpret_cast<const f32x4*>(b + r * ldb + cv * 8 + 4);
        }
        *reinterpret_cast<f32x4*>(out + r * ldo + cv * 8) = v0;
        *reinterpret_cast<f32x4*>(out + r * ldo + cv * 8 + 4) = v1;
        const float f[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        stg16(out16 + r * ld16 + cv * 8, pack8<F16>(f));
    }
}

// [rows][C] (fp32 or 16-bit) -> bf16 [rows][3C]: hi | lo | hi (pattern 0) or hi | hi | lo (pattern 1)
template <typename SRC>
__global__ void __launch_bounds__(256) split3_kernel(const void* src, int64_t rows, int CV, int C, int64_t ld_src, int pattern,
                                                    uint16_t* dst, int64_t ld_dst) {
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / CV;
        const int cv = (int)(i - r * CV);
        float f[8], back[8], lo[8];
        if constexpr (sizeof(typename SRC::elem) == 4) {
            const float* sp = static_cast<const float*>(src) + r * ld_src + cv * 8;
            const f32x4 a = *reinterpret_cast<const f32x4*>(sp), b = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[j + 4] = b[j]; }
        } else {
            unpack8<SRC>(ldg16(static_cast<const uint16_t*>(src) + r * ld_src + cv * 8), f);
        }
        const U4 hi = pack8<BF16>(f);
        unpack8<BF16>(hi, back);
#pragma unroll
        for (int j = 0; j < 8; ++j) lo[j] = f[j] - back[j];
        const U4 lov = pack8<BF16>(lo);
        uint16_t* dp = dst + r * ld_dst + cv * 8;
        stg16(dp, hi);
        if (pattern) { stg16(dp + C, hi); stg16(dp + 2 * C, lov); }      // (a select between two structs goes through scratch)
        else { stg16(dp + C, lov); stg16(dp + 2 * C, hi); }
    }
}

// [rows][C] (fp32 or 16-bit) -> PARTS-part operand of 16-bit type OT: [hi] / [hi | lo] / [hi | lo | hi]
template <typename SRC, typename OT, int PARTS>
__global__ void __launch_bounds__(256) split_operand_kernel(const void* src, int64_t rows, int CV, int C, int64_t ld_src,
                                                           uint16_t* dst, int64_t ld_dst) {
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / CV;
        const int cv = (int)(i - r * CV);
        float f[8];
        if constexpr (sizeof(typename SRC::elem) == 4) {
            const float* sp = static_cast<const float*>(src) + r * ld_src + cv * 8;
            const f32x4 a = *reinterpret_cast<const f32x4*>(sp), b = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[j + 4] = b[j]; }
        } else {
            unpack8<SRC>(ldg16(static_cast<const uint16_t*>(src) + r * ld_src + cv * 8), f);
        }
        const U4 hi = pack8<OT>(f);
        uint16_t* dp = dst + r * ld_dst + cv * 8;
        stg16(dp, hi);
        if constexpr (PARTS >= 2) {
            float back[8], lo[8];
            unpack8<OT>(hi, back);
#pragma unroll
            for (int j = 0; j < 8; ++j) lo[j] = f[j] - back[j];
            stg16(dp + C, pack8<OT>(lo));
        }
        if constexpr (PARTS == 3) stg16(dp + 2 * C, hi);
    }
}

// fp32 [rows][C] (row stride ld_src) -> 16-bit [rows][C] (row stride ld_dst)
template <typename T>
__global__ void __launch_bounds__(256) cast16_kernel(const float* src, int64_t rows, int CV, int64_t ld_src, uint16_t* dst,
                                                    int64_t ld_dst) {
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / CV;
        const int cv = (int)(i - r * CV);
        const float* sp = src + r * ld_src + cv * 8;
        const f32x4 a = *reinterpret_cast<const f32x4*>(sp), b = *reinterpret_cast<const f32x4*>(sp + 4);
        float f[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[j + 4] = b[j]; }
        stg16(dst + r * ld_dst + cv * 8, pack8<T>(f));
    }
}

template <typename T>
__global__ void temb_kernel(const int64_t* t, int dim, typename T::elem* out, int ld) {
    const int b = blockIdx.x, half = dim >> 1;
    const float tv = (float)t[b];
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
        // exp(-ln(10000) * i / half), fp32 like the reference
        const float freq = expf(-9.210340371976184f * (float)i / (float)half);
        const float arg = tv * freq;
        out[(int64_t)b * ld + i] = T::from_f32(cosf(arg));
        out[(int64_t)b * ld + half + i] = T::from_f32(sinf(arg));
    }
}

// (sampler_update_elem, q_sample_elem, gaussian_sample_elem: noise_elem.h, shared with the seeded forms of rng.hip)
__global__ void __launch_bounds__(256) sampler_update_kernel(const float* x, const float* eps, const float* noise,
                                                            float c_recip, float c_recipm1, float coef1, float coef2,
                                                            float sigma, float* x_prev, float* pred_x0, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float p0, xp;
        sampler_update_elem(x[i], eps[i], noise[i], c_recip, c_recipm1, coef1, coef2, sigma, p0, xp);
        if (pred_x0) pred_x0[i] = p0;
        x_prev[i] = xp;
    }
}

__global__ void __launch_bounds__(256) axpby_kernel(const float* x, const float* y, float a, float b, float* out,
                                                   int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = a * x[i] + b * y[i];
}

// q_sample with the timestep read on the device: out[b] = tab_a[t[b]] * x[b] + tab_b[t[b]] * noise[b]
__global__ void __launch_bounds__(256) q_sample_kernel(const float* x, const float* noise, const int64_t* t, const float* tab_a,
                                                      const float* tab_b, int n_tab, float* out, int64_t per_image, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int64_t ti = t[i / per_image];
        ti = ti < 0 ? 0 : (ti >= n_tab ? n_tab - 1 : ti);
        out[i] = q_sample_elem(tab_a[ti], x[i], tab_b[ti], noise[i]);
    }
}

// sampler update with the step index read on the device: coefs[n_steps][5] = (c_recip, c_recipm1, coef1, coef2, sigma)
__global__ void __launch_bounds__(256) sampler_update_indexed_kernel(const float* x, const float* eps, const float* noise,
                                                                    const int64_t* index, const float* coefs, int n_steps,
                                                                    float* x_prev, float* pred_x0, int64_t per_image, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int64_t k = index[i / per_image];
        k = k < 0 ? 0 : (k >= n_steps ? n_steps - 1 : k);
        const float* c = coefs + k * 5;
        float p0, xp;
        sampler_update_elem(x[i], eps[i], noise[i], c[0], c[1], c[2], c[3], c[4], p0, xp);
        if (pred_x0) pred_x0[i] = p0;
        x_prev[i] = xp;
    }
}

// VAE posterior: out (NCHW) = (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) * scale from NHWC fp32 moments rows
__global__ void __launch_bounds__(256) gaussian_sample_kernel(const float* moments, int ld, const float* noise, float* out, int C,
                                                             int64_t HW, float scale, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t px = i % HW, bc = i / HW;
        const int c = (int)(bc % C);
        const int64_t b = bc / C;
        const float* row = moments + (b * HW + px) * ld;
        out[i] = noise ? gaussian_sample_elem(row[c], row[C + c], noise[i], scale) : row[c] * scale;
    }
}

__global__ void __launch_bounds__(256) divide_kernel(const float* num, const float* den, float* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = num[i] / den[i];
}

__global__ void __launch_bounds__(256) tile_acc_kernel(const float* tile, const float* wts, float* out, float* count,
                                                      int BC, int H, int W, int th, int tw, int hi, int wi) {
    const int64_t n = (int64_t)BC * th * tw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % tw), y = (int)((i / tw) % th);
        const int64_t bc = i / ((int64_t)tw * th);
        const float w = wts[y * tw + x];
        const int64_t o = (bc * H + hi + y) * W + wi + x;
        out[o] += tile[i] * w;
        count[o] += w;
    }
}

}  // namespace

namespace {
__global__ void __launch_bounds__(256) zero_kernel(U4* dst, int64_t n16) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) dst[i] = zero16();
}
}  // namespace

extern "C" int edtr_zero_bytes(void* ptr, int64_t bytes, edtr_stream_t stream) {
    if (!ptr) return EDTR_E_NULL;
    if (bytes < 0) return EDTR_E_SHAPE;
    if ((bytes & 15) || !aligned16(ptr)) return EDTR_E_ALIGN;
    if (bytes == 0) return EDTR_OK;
    const int64_t n16 = bytes >> 4;
    int64_t blocks = (n16 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<U4*>(ptr), n16);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_abi_version(void) { return EDTR_ABI_VERSION; }

extern "C" const char* edtr_error_string(int code) {
    switch (code) {
        case EDTR_OK: return "ok";
        case EDTR_E_NULL: return "EDTR_E_NULL: required pointer is NULL";
        case EDTR_E_SHAPE: return "EDTR_E_SHAPE: non-positive or inconsistent extent";
        case EDTR_E_ALIGN: return "EDTR_E_ALIGN: pointer / leading dimension violates the 16-byte rule";
        case EDTR_E_DTYPE: return "EDTR_E_DTYPE: unknown dtype or flag value";
        case EDTR_E_UNSUPPORTED: return "EDTR_E_UNSUPPORTED: configuration not supported by this kernel";
        default: break;
    }
    if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
    return "unknown edtr error";
}

extern "C" int edtr_device_info(int* compute_units, int64_t* hbm_bytes, char* arch_name, int arch_name_len) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (arch_name && arch_name_len > 0) {
        strncpy(arch_name, prop.gcnArchName, arch_name_len - 1);
        arch_name[arch_name_len - 1] = 0;
    }
    return 1;
}

extern "C" int edtr_nchw_to_nhwc(int dtype, const float* src, int B, int C, int64_t HW, void* dst, int ld, int coff,
                                 int zero_pad_to, float scale, float shift, edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (dtype < EDTR_BF16 || dtype > EDTR_F32_H3) return EDTR_E_DTYPE;
    if (B <= 0 || C <= 0 || HW <= 0 || ld <= 0 || coff < 0) return EDTR_E_SHAPE;
    const int cpad = zero_pad_to > C ? zero_pad_to : C;
    if (coff + cpad > ld) return EDTR_E_SHAPE;
    dim3 grid((unsigned)((HW + 63) / 64), B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype >= EDTR_F32_SPLIT)       // high / mixed precision modes: the NHWC activation stays fp32
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<F32E>, grid, dim3(256), 0, s, src, C, HW, static_cast<float*>(dst), ld, coff,
                           cpad, scale, shift);
    else if (dtype == EDTR_BF16)
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<BF16>, grid, dim3(256), 0, s, src, C, HW, static_cast<uint16_t*>(dst), ld,
                           coff, cpad, scale, shift);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<F16>, grid, dim3(256), 0, s, src, C, HW, static_cast<uint16_t*>(dst), ld,
                           coff, cpad, scale, shift);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_nhwc_to_nchw(int dtype, const void* src, int src_f32, int B, int C, int64_t HW, int ld, float* dst,
                                 float scale, edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (dtype != EDTR_BF16 && dtype != EDTR_F16) return EDTR_E_DTYPE;
    if (B <= 0 || C <= 0 || HW <= 0 || ld < C) return EDTR_E_SHAPE;
    dim3 grid((unsigned)((HW + 63) / 64), B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == EDTR_BF16)
        hipLaunchKernelGGL(nhwc_to_nchw_kernel<BF16>, grid, dim3(256), 0, s, src, src_f32, C, HW, ld, dst, scale);
    else
        hipLaunchKernelGGL(nhwc_to_nchw_kernel<F16>, grid, dim3(256), 0, s, src, src_f32, C, HW, ld, dst, scale);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_add_mirror(const float* a, int lda, const float* b, int ldb, float* out, int ldo, void* out16, int ld16,
                               int64_t rows, int C, edtr_stream_t stream) {
    if (!a || !out || !out16) return EDTR_E_NULL;
    if (rows <= 0 || C <= 0) return EDTR_E_SHAPE;
    if ((C & 7) || (lda & 3) || (ldo & 3) || (ld16 & 7) || (b && (ldb & 3)) || !aligned16(a) || (b && !aligned16(b)) || !aligned16(out) ||
        !aligned16(out16))
        return EDTR_E_ALIGN;
    hipLaunchKernelGGL(add_f32_mirror_kernel, dim3(blocks_for(rows * (C >> 3))), dim3(256), 0, static_cast<hipStream_t>(stream), a, lda,
                       b, ldb, out, ldo, static_cast<uint16_t*>(out16), ld16, rows, C >> 3);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_add_stats(int dtype, const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows, int C,
                              float* gn_partial, int gn_ld, int slot_rows, edtr_stream_t stream) {
    if (!a || !out || !gn_partial) return EDTR_E_NULL;
    if (dtype != EDTR_BF16 && dtype != EDTR_F16) return EDTR_E_DTYPE;
    if (rows <= 0 || C <= 0 || (slot_rows != 64 && slot_rows != 128) || rows % slot_rows || gn_ld < C) return EDTR_E_SHAPE;
    if ((C & 31) || (lda & 7) || (ldo & 7) || (b && (ldb & 7)) || !aligned16(a) || (b && !aligned16(b)) || !aligned16(out) || !aligned_to(gn_partial, 8))
        return EDTR_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(C / 32), (unsigned)(rows / slot_rows));
    if (dtype == EDTR_BF16)
        hipLaunchKernelGGL(add_stats_kernel<BF16>, grid, dim3(256), 0, s, static_cast<const uint16_t*>(a), lda, static_cast<const uint16_t*>(b), ldb,
                           static_cast<uint16_t*>(out), ldo, C, gn_partial, gn_ld, slot_rows);
    else
        hipLaunchKernelGGL(add_stats_kernel<F16>, grid, dim3(256), 0, s, static_cast<const uint16_t*>(a), lda, static_cast<const uint16_t*>(b), ldb,
                           static_cast<uint16_t*>(out), ldo, C, gn_partial, gn_ld, slot_rows);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_add(int dtype, const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows,
                        int C, edtr_stream_t stream) {
    if (!a || !out) return EDTR_E_NULL;
    if (dtype < EDTR_BF16 || dtype > EDTR_F32_H3) return EDTR_E_DTYPE;
    if (rows <= 0 || C <= 0) return EDTR_E_SHAPE;
    if (dtype >= EDTR_F32_SPLIT) {     // fp32 in / out (every fp32-stream code)
        if ((C & 3) || (lda & 3) || (ldo & 3) || (b && (ldb & 3)) || !aligned16(a) || (b && !aligned16(b)) || !aligned16(out))
            return EDTR_E_ALIGN;
        hipLaunchKernelGGL(add_f32_kernel, dim3(blocks_for(rows * (C >> 2))), dim3(256), 0, static_cast<hipStream_t>(stream),
                           static_cast<const float*>(a), lda, static_cast<const float*>(b), ldb, static_cast<float*>(out), ldo,
                           rows, C >> 2);
        EDTR_LAUNCH_CHECK();
        return EDTR_OK;
    }
    if ((C & 7) || (lda & 7) || (ldo & 7) || (b && (ldb & 7)) || !aligned16(a) || (b && !aligned16(b)) || !aligned16(out))
        return EDTR_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int CV = C >> 3;
    const unsigned blocks = blocks_for(rows * CV);
    if (dtype == EDTR_BF16)
        hipLaunchKernelGGL(add_kernel<BF16>, dim3(blocks), dim3(256), 0, s, static_cast<const uint16_t*>(a), lda,
                           static_cast<const uint16_t*>(b), ldb, static_cast<uint16_t*>(out), ldo, rows, CV);
    else
        hipLaunchKernelGGL(add_kernel<F16>, dim3(blocks), dim3(256), 0, s, static_cast<const uint16_t*>(a), lda,
                           static_cast<const uint16_t*>(b), ldb, static_cast<uint16_t*>(out), ldo, rows, CV);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

namespace {
// out[row][d] = table[token[row]][d] + pos[row % L][d]   (16-bit out, 8 channels per thread)
template <typename T>
__global__ void __launch_bounds__(256) embed_tokens_kernel(const int64_t* tokens, const float* table, const float* pos, int rows,
                                                           int L, int D, int vocab, uint16_t* out, int ld) {
    const int dv = D >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)rows * dv; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i / dv), d0 = (int)(i - (int64_t)row * dv) * 8;
        int64_t tok = tokens[row];
        tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
        const float* tp = table + tok * D + d0;
        const float* pp = pos + (int64_t)(row % L) * D + d0;
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = tp[j] + pp[j];
        stg16(out + (int64_t)row * ld + d0, pack8<T>(f));
    }
}
}  // namespace

extern "C" int edtr_embed_tokens(int dtype, const int64_t* tokens, const float* table, const float* pos, int rows, int L,
                                 int D, int vocab, void* out, int ld, edtr_stream_t stream) {
    if (!tokens || !table || !pos || !out) return EDTR_E_NULL;
    if (dtype != EDTR_BF16 && dtype != EDTR_F16) return EDTR_E_DTYPE;
    if (rows <= 0 || L <= 0 || D <= 0 || vocab <= 0) return EDTR_E_SHAPE;
    if ((D & 7) || (ld & 7) || !aligned16(out)) return EDTR_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned blocks = blocks_for((int64_t)rows * (D >> 3));
    if (dtype == EDTR_BF16)
        hipLaunchKernelGGL(embed_tokens_kernel<BF16>, dim3(blocks), dim3(256), 0, s, tokens, table, pos, rows, L, D, vocab,
                           static_cast<uint16_t*>(out), ld);
    else
        hipLaunchKernelGGL(embed_tokens_kernel<F16>, dim3(blocks), dim3(256), 0, s, tokens, table, pos, rows, L, D, vocab,
                           static_cast<uint16_t*>(out), ld);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_timestep_embedding(int dtype, const int64_t* t, int B, int dim, void* out, int ld,
                                       edtr_stream_t stream) {
    if (!t || !out) return EDTR_E_NULL;
    if (dtype < EDTR_BF16 || dtype > EDTR_F32_H3) return EDTR_E_DTYPE;
    if (B <= 0 || dim <= 0 || (dim & 1) || ld < dim) return EDTR_E_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype >= EDTR_F32_SPLIT)
        hipLaunchKernelGGL(temb_kernel<F32E>, dim3(B), dim3(256), 0, s, t, dim, static_cast<float*>(out), ld);
    else if (dtype == EDTR_BF16)
        hipLaunchKernelGGL(temb_kernel<BF16>, dim3(B), dim3(256), 0, s, t, dim, static_cast<uint16_t*>(out), ld);
    else
        hipLaunchKernelGGL(temb_kernel<F16>, dim3(B), dim3(256), 0, s, t, dim, static_cast<uint16_t*>(out), ld);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_sampler_update(const float* x, const float* eps, const float* noise, float c_recip, float c_recipm1,
                                   float coef1, float coef2, float sigma, float* x_prev, float* pred_x0, int64_t n,
                                   edtr_stream_t stream) {
    if (!x || !eps || !noise || !x_prev) return EDTR_E_NULL;
    if (n <= 0) return EDTR_E_SHAPE;
    hipLaunchKernelGGL(sampler_update_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, eps,
                       noise, c_recip, c_recipm1, coef1, coef2, sigma, x_prev, pred_x0, n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_axpby(const float* x, const float* y, float a, float b, float* out, int64_t n, edtr_stream_t stream) {
    if (!x || !y || !out) return EDTR_E_NULL;
    if (n <= 0) return EDTR_E_SHAPE;
    hipLaunchKernelGGL(axpby_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, a, b, out,
                       n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_split3(int src_dtype, const void* src, int64_t rows, int C, int64_t ld_src, int pattern, void* dst,
                           int64_t ld_dst, edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (src_dtype < EDTR_BF16 || src_dtype > EDTR_F32_H3) return EDTR_E_DTYPE;
    if (rows <= 0 || C <= 0 || ld_dst < 3 * (int64_t)C || ld_src < C || (pattern != 0 && pattern != 1)) return EDTR_E_SHAPE;
    if ((C & 7) || (ld_src & 7) || (ld_dst & 7) || !aligned16(src) || !aligned16(dst)) return EDTR_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int CV = C >> 3;
    const unsigned blocks = blocks_for(rows * CV);
    uint16_t* d = static_cast<uint16_t*>(dst);
    if (src_dtype >= EDTR_F32_SPLIT) hipLaunchKernelGGL(split3_kernel<F32E>, dim3(blocks), dim3(256), 0, s, src, rows, CV, C, ld_src, pattern, d, ld_dst);
    else if (src_dtype == EDTR_BF16) hipLaunchKernelGGL(split3_kernel<BF16>, dim3(blocks), dim3(256), 0, s, src, rows, CV, C, ld_src, pattern, d, ld_dst);
    else hipLaunchKernelGGL(split3_kernel<F16>, dim3(blocks), dim3(256), 0, s, src, rows, CV, C, ld_src, pattern, d, ld_dst);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_split_operand(int src_dtype, const void* src, int64_t rows, int C, int64_t ld_src, int op_fmt, void* dst,
                                  int64_t ld_dst, edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (src_dtype < EDTR_BF16 || src_dtype > EDTR_F32_H3 || op_fmt < EDTR_F32_SPLIT || op_fmt > EDTR_F32_H3) return EDTR_E_DTYPE;
    const int parts = op_fmt == EDTR_F32_H1 ? 1 : (op_fmt == EDTR_F32_H2 ? 2 : 3);
    if (rows <= 0 || C <= 0 || ld_dst < parts * (int64_t)C || ld_src < C) return EDTR_E_SHAPE;
    const bool src32 = src_dtype >= EDTR_F32_SPLIT;
    if ((C & 7) || (ld_src & (src32 ? 3 : 7)) || (ld_dst & 7) || !aligned16(src) || !aligned16(dst)) return EDTR_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int CV = C >> 3;
    const dim3 grid(blocks_for(rows * CV)), block(256);
    uint16_t* d = static_cast<uint16_t*>(dst);
#define EDTR_SPLIT_LAUNCH(SRC, OT, PARTS) hipLaunchKernelGGL((split_operand_kernel<SRC, OT, PARTS>), grid, block, 0, s, src, rows, CV, C, ld_src, d, ld_dst)
#define EDTR_SPLIT_SRC(OT, PARTS)                                              \
    do {                                                                        \
        if (src32) EDTR_SPLIT_LAUNCH(F32E, OT, PARTS);                          \
        else if (src_dtype == EDTR_BF16) EDTR_SPLIT_LAUNCH(BF16, OT, PARTS);    \
        else EDTR_SPLIT_LAUNCH(F16, OT, PARTS);                                 \
    } while (0)
    if (op_fmt == EDTR_F32_SPLIT) EDTR_SPLIT_SRC(BF16, 3);
    else if (op_fmt == EDTR_F32_H1) EDTR_SPLIT_SRC(F16, 1);
    else if (op_fmt == EDTR_F32_H2) EDTR_SPLIT_SRC(F16, 2);
    else EDTR_SPLIT_SRC(F16, 3);
#undef EDTR_SPLIT_SRC
#undef EDTR_SPLIT_LAUNCH
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_sampler_update_indexed(const float* x, const float* eps, const float* noise, const int64_t* index,
                                           const float* coefs, int n_steps, float* x_prev, float* pred_x0, int B,
                                           int64_t per_image, edtr_stream_t stream) {
    if (!x || !eps || !noise || !index || !coefs || !x_prev) return EDTR_E_NULL;
    if (B <= 0 || per_image <= 0 || n_steps <= 0) return EDTR_E_SHAPE;
    const int64_t n = (int64_t)B * per_image;
    hipLaunchKernelGGL(sampler_update_indexed_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, eps,
                       noise, index, coefs, n_steps, x_prev, pred_x0, per_image, n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_gaussian_sample(const float* moments, int ld, const float* noise, float* out, int B, int C, int64_t HW,
                                    float scale, edtr_stream_t stream) {
    if (!moments || !out) return EDTR_E_NULL;
    if (B <= 0 || C <= 0 || HW <= 0 || ld < 2 * C) return EDTR_E_SHAPE;
    const int64_t n = (int64_t)B * C * HW;
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), moments, ld,
                       noise, out, C, HW, scale, n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_cast16(int dst_dtype, const float* src, int64_t rows, int C, int64_t ld_src, void* dst, int64_t ld_dst,
                           edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (dst_dtype != EDTR_BF16 && dst_dtype != EDTR_F16) return EDTR_E_DTYPE;
    if (rows <= 0 || C <= 0 || ld_src < C || ld_dst < C) return EDTR_E_SHAPE;
    if ((C & 7) || (ld_src & 3) || (ld_dst & 7) || !aligned16(src) || !aligned16(dst)) return EDTR_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int CV = C >> 3;
    if (dst_dtype == EDTR_BF16) hipLaunchKernelGGL(cast16_kernel<BF16>, dim3(blocks_for(rows * CV)), dim3(256), 0, s, src, rows, CV, ld_src, static_cast<uint16_t*>(dst), ld_dst);
    else hipLaunchKernelGGL(cast16_kernel<F16>, dim3(blocks_for(rows * CV)), dim3(256), 0, s, src, rows, CV, ld_src, static_cast<uint16_t*>(dst), ld_dst);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_q_sample(const float* x, const float* noise, const int64_t* t, const float* tab_a, const float* tab_b,
                             int n_tab, float* out, int B, int64_t per_image, edtr_stream_t stream) {
    if (!x || !noise || !t || !tab_a || !tab_b || !out) return EDTR_E_NULL;
    if (B <= 0 || per_image <= 0 || n_tab <= 0) return EDTR_E_SHAPE;
    const int64_t n = (int64_t)B * per_image;
    hipLaunchKernelGGL(q_sample_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, noise, t, tab_a,
                       tab_b, n_tab, out, per_image, n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_divide(const float* num, const float* den, float* out, int64_t n, edtr_stream_t stream) {
    if (!num || !den || !out) return EDTR_E_NULL;
    if (n <= 0) return EDTR_E_SHAPE;
    hipLaunchKernelGGL(divide_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), num, den, out,
                       n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_tile_accumulate(const float* tile, const float* wts, float* out, float* count, int B, int C, int H,
                                    int W, int th, int tw, int hi, int wi, edtr_stream_t stream) {
    if (!tile || !wts || !out || !count) return EDTR_E_NULL;
    if (B <= 0 || C <= 0 || th <= 0 || tw <= 0 || hi < 0 || wi < 0 || hi + th > H || wi + tw > W) return EDTR_E_SHAPE;
    const int64_t n = (int64_t)B * C * th * tw;
    hipLaunchKernelGGL(tile_acc_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), tile, wts, out,
                       count, B * C, H, W, th, tw, hi, wi);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

// ---- window table forms of the tiled path: every window cut in one launch, every window blended in one launch -----------------
namespace {
// unit = four consecutive elements of one window row (the last unit of a row is shorter when tw % 4 != 0).  `vec_ok`: tw % 4 == 0,
// W % 4 == 0 and both planes 16-byte aligned, so that a window moves as float4 exactly when its own wi % 4 == 0 (decided here).
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ src, const int32_t* __restrict__ table,
                                                         float* __restrict__ dst, int BC, int H, int W, int th, int tw, int n,
                                                         int vec_ok) {
    const int q = (tw + 3) >> 2;
    const int64_t units = (int64_t)n * BC * th * q;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
        const int x = (int)(u % q) << 2;
        int64_t r = u / q;
        const int y = (int)(r % th);
        r /= th;
        const int64_t bc = r % BC, k = r / BC;
        const int hi = table[2 * k], wi = table[2 * k + 1];
        const float* s = src + (bc * H + hi + y) * W + wi + x;
        float* d = dst + ((k * BC + bc) * th + y) * tw + x;
        if (vec_ok && (wi & 3) == 0) {
            *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(s);
        } else {
            const int m = tw - x < 4 ? tw - x : 4;
            for (int j = 0; j < m; ++j) d[j] = s[j];
        }
    }
}

// gather form of the overlap-add: one lane owns V adjacent pixels of one row, walks the windows in table order and writes the
// quotient once.  The numerator is __builtin_fmaf(tile, w, acc) from acc = 0 and the denominator cnt + w from cnt = 0: the very
// operations tile_acc_kernel performs per window on zeroed planes (its `out[o] += tile[i] * w` is contracted to one fma), and the
// division is divide_kernel's, so the bits are those of that sequence.  V = 4 needs every wi, tw and W to be multiples of 4: the
// four pixels of a lane are then inside or outside a window together.
template <int V>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ tiles, const float* __restrict__ wts,
                                                        const int32_t* __restrict__ table, float* __restrict__ out, int BC, int H,
                                                        int W, int th, int tw, int n) {
    const int q = W / V;
    const int64_t units = (int64_t)BC * H * q;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
        const int x = (int)(u % q) * V;
        const int64_t r = u / q;
        const int y = (int)(r % H);
        const int64_t bc = r / H;
        float acc[V], cnt[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.0f, cnt[j] = 0.0f;
        for (int k = 0; k < n; ++k) {
            const int ty = y - table[2 * k], tx = x - table[2 * k + 1];
            if ((unsigned)ty >= (unsigned)th || (unsigned)tx >= (unsigned)tw) continue;
            const float* t = tiles + (((int64_t)k * BC + bc) * th + ty) * tw + tx;
            const float* w = wts + ty * tw + tx;
            if (V == 4) {
                const f32x4 tv = *reinterpret_cast<const f32x4*>(t), wv = *reinterpret_cast<const f32x4*>(w);
#pragma unroll
                for (int j = 0; j < V; ++j) acc[j] = __builtin_fmaf(tv[j], wv[j], acc[j]), cnt[j] += wv[j];
            } else {
                acc[0] = __builtin_fmaf(t[0], w[0], acc[0]);
                cnt[0] += w[0];
            }
        }
        float* o = out + (bc * H + y) * W + x;
        if (V == 4) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = acc[j] / cnt[j];
            *reinterpret_cast<f32x4*>(o) = v;
        } else {
            o[0] = acc[0] / cnt[0];
        }
    }
}

// the table's host copy: n windows of th x tw inside the H x W plane.  *all_wi4: every wi is a multiple of 4.
int check_windows(const int32_t* t, int n, int th, int tw, int H, int W, bool* all_wi4) {
    bool a = true;
    for (int k = 0; k < n; ++k) {
        const int hi = t[2 * k], wi = t[2 * k + 1];
        if (hi < 0 || wi < 0 || hi > H - th || wi > W - tw) return EDTR_E_SHAPE;
        a = a && (wi & 3) == 0;
    }
    *all_wi4 = a;
    return EDTR_OK;
}

// every pixel of the plane lies in a window: per band of rows between two window edges, the columns [wi, wi + tw) of the windows
// over that band, sorted, must leave no gap in [0, W)
bool windows_cover(const int32_t* t, int n, int th, int tw, int H, int W) {
    std::vector<int> edges;
    edges.reserve(2 * (size_t)n + 2);
    edges.push_back(0);
    for (int k = 0; k < n; ++k) edges.push_back(t[2 * k]), edges.push_back(t[2 * k] + th);
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    if (edges.back() < H) return false;
    std::vector<int> cols;
    for (size_t e = 0; e + 1 < edges.size(); ++e) {
        const int y = edges[e];                      // no window starts or ends inside [y, edges[e + 1]): one row stands for the band
        cols.clear();
        for (int k = 0; k < n; ++k)
            if (t[2 * k] <= y && y < t[2 * k] + th) cols.push_back(t[2 * k + 1]);
        std::sort(cols.begin(), cols.end());
        int reach = 0;
        for (int wi : cols) {
            if (wi > reach) return false;
            reach = wi + tw > reach ? wi + tw : reach;
        }
        if (reach < W) return false;
    }
    return true;
}
}  // namespace

extern "C" int edtr_tile_gather(const float* src, int B, int C, int H, int W, const int32_t* table_host, const int32_t* table, int n,
                                int th, int tw, float* dst, edtr_stream_t stream) {
    if (!src || !table_host || !table || !dst) return EDTR_E_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || n <= 0 || n > EDTR_TILE_WINDOWS_MAX || th <= 0 || tw <= 0 || th > H || tw > W)
        return EDTR_E_SHAPE;
    if (!all_aligned_to(4, src, dst, table)) return EDTR_E_ALIGN;
    bool all_wi4 = false;
    const int rc = check_windows(table_host, n, th, tw, H, W, &all_wi4);
    if (rc != EDTR_OK) return rc;
    const int vec_ok = tw % 4 == 0 && W % 4 == 0 && aligned16(src) && aligned16(dst);
    const int64_t units = (int64_t)n * B * C * th * ((tw + 3) / 4);
    hipLaunchKernelGGL(tile_gather_kernel, dim3(blocks_for(units)), dim3(256), 0, static_cast<hipStream_t>(stream), src, table, dst,
                       B * C, H, W, th, tw, n, vec_ok);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_tile_blend(const float* tiles, const float* wts, const int32_t* table_host, const int32_t* table, int n, int th,
                               int tw, float* out, int B, int C, int H, int W, edtr_stream_t stream) {
    if (!tiles || !wts || !table_host || !table || !out) return EDTR_E_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || n <= 0 || n > EDTR_TILE_WINDOWS_MAX || th <= 0 || tw <= 0 || th > H || tw > W)
        return EDTR_E_SHAPE;
    if (!all_aligned_to(4, tiles, wts, out, table)) return EDTR_E_ALIGN;
    bool all_wi4 = false;
    const int rc = check_windows(table_host, n, th, tw, H, W, &all_wi4);
    if (rc != EDTR_OK) return rc;
    if (!windows_cover(table_host, n, th, tw, H, W)) return EDTR_E_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int BC = B * C;
    if (all_wi4 && tw % 4 == 0 && W % 4 == 0 && aligned16(tiles) && aligned16(wts) && aligned16(out))
        hipLaunchKernelGGL(tile_blend_kernel<4>, dim3(blocks_for((int64_t)BC * H * (W / 4))), dim3(256), 0, st, tiles, wts, table, out, BC,
                           H, W, th, tw, n);
    else
        hipLaunchKernelGGL(tile_blend_kernel<1>, dim3(blocks_for((int64_t)BC * H * W)), dim3(256), 0, st, tiles, wts, table, out, BC, H, W,
                           th, tw, n);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

// ---- hipGraph helpers -------------------------------------------------------------------------
extern "C" int edtr_graph_begin(edtr_stream_t stream) {
    return (int)hipStreamBeginCapture(static_cast<hipStream_t>(stream), hipStreamCaptureModeThreadLocal);
}

extern "C" int edtr_graph_end(edtr_stream_t stream, void** graph_exec_out) {
    if (!graph_exec_out) return EDTR_E_NULL;
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamEndCapture(static_cast<hipStream_t>(stream), &graph);
    if (e != hipSuccess) return (int)e;
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return (int)e;
    *graph_exec_out = exec;
    return EDTR_OK;
}

extern "C" int edtr_graph_launch(void* graph_exec, edtr_stream_t stream) {
    if (!graph_exec) return EDTR_E_NULL;
    return (int)hipGraphLaunch(static_cast<hipGraphExec_t>(graph_exec), static_cast<hipStream_t>(stream));
}

extern "C" int edtr_graph_destroy(void* graph_exec) {
    if (!graph_exec) return EDTR_E_NULL;
    return (int)hipGraphExecDestroy(static_cast<hipGraphExec_t>(graph_exec));
}

// ---- wavelet colour fix ------------------------------------------------------------------
// One level of the "wavelet blur": depthwise 3x3 binomial kernel with dilation r and replicate padding on fp32 NCHW
// planes (reference utils/common.py:99-118).  Optionally accumulates high += (in - low) in the same pass
// (utils/common.py:127-131), so a 5-level decomposition is 5 launches per image batch.
namespace {
__global__ void __launch_bounds__(256) wavelet_level_kernel(const float* in, float* low, float* high, int planes, int H,
                                                           int W, int r) {
    const int64_t n = (int64_t)planes * H * W;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const float* pl = in + (i - (int64_t)y * W - x);
        const int ym = max(y - r, 0), yp = min(y + r, H - 1), xm = max(x - r, 0), xp = min(x + r, W - 1);
        const float c = pl[(int64_t)y * W + x];
        const float v = 0.0625f * (pl[(int64_t)ym * W + xm] + pl[(int64_t)ym * W + xp] + pl[(int64_t)yp * W + xm] +
                                   pl[(int64_t)yp * W + xp]) +
                        0.125f * (pl[(int64_t)ym * W + x] + pl[(int64_t)yp * W + x] + pl[(int64_t)y * W + xm] +
                                  pl[(int64_t)y * W + xp]) +
                        0.25f * c;
        low[i] = v;
        if (high) high[i] += c - v;
    }
}
}  // namespace

extern "C" int edtr_wavelet_level(const float* in, float* low, float* high_accum, int planes, int H, int W, int radius,
                                  edtr_stream_t stream) {
    if (!in || !low) return EDTR_E_NULL;
    if (planes <= 0 || H <= 0 || W <= 0 || radius <= 0) return EDTR_E_SHAPE;
    if (in == low) return EDTR_E_UNSUPPORTED;   // not in-place: neighbours are read after the centre is written
    const int64_t n = (int64_t)planes * H * W;
    hipLaunchKernelGGL(wavelet_level_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), in, low,
                       high_accum, planes, H, W, radius);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

// ---- strided fp32 block copy (tile extraction / valid-region placement of the tiled VAE) -------------------------
namespace {
__global__ void __launch_bounds__(256) copy3d_kernel(const float* src, int64_t s_plane, int64_t s_row, float* dst,
                                                    int64_t d_plane, int64_t d_row, int planes, int rows, int cols) {
    const int64_t n = (int64_t)planes * rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % cols), y = (int)((i / cols) % rows);
        const int64_t pl = i / ((int64_t)cols * rows);
        dst[pl * d_plane + (int64_t)y * d_row + x] = src[pl * s_plane + (int64_t)y * s_row + x];
    }
}
}  // namespace

extern "C" int edtr_copy3d_f32(const float* src, int64_t src_plane_stride, int64_t src_row_stride, float* dst,
                               int64_t dst_plane_stride, int64_t dst_row_stride, int planes, int rows, int cols,
                               edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (planes <= 0 || rows <= 0 || cols <= 0) return EDTR_E_SHAPE;
    const int64_t n = (int64_t)planes * rows * cols;
    hipLaunchKernelGGL(copy3d_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), src,
                       src_plane_stride, src_row_stride, dst, dst_plane_stride, dst_row_stride, planes, rows, cols);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
