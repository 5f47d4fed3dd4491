// Seeded per-image Gaussian noise, drawn inside the kernels that consume it (edtr_hip.h "Reproducible noise"; the host
// restatement is edtr_amd/rng.py).  Philox4x32-10 keyed by the seed, counter (e >> 2, draw, purpose, image id): one lane owns
// one group of four consecutive elements of one image = one Philox call, two Box-Muller pairs, float4 loads and stores.
// The fused kernels form z in registers and hand it to the SAME element expressions the tensor-noise kernels use
// (noise_elem.h), so "edtr_normal_fill, then the existing kernel" and the fused launch give identical bits.
#include "common.h"
#include "noise_elem.h"
#include "philox.h"

namespace {

struct Stream {          // what does not depend on the element: passed by value to every kernel
    uint32_t k0, k1;
    const int64_t* ids;  // [B] global image ids, or NULL: id_base + b
    uint32_t id_base;
    int64_t groups;      // per_image / 4
};

// the normals of elements 4 * eg + 0..3 of image `id`
__device__ __forceinline__ f32x4 normal4(const Stream& s, uint32_t eg, uint32_t draw, uint32_t purpose, uint32_t id) {
    return philox_normal4(s.k0, s.k1, eg, draw, purpose, id);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }

__global__ void __launch_bounds__(256) normal_fill_kernel(float* out, Stream s, uint32_t purpose, uint32_t draw, int64_t n4) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / s.groups;
        st4(out + g * 4, normal4(s, (uint32_t)(g - b * s.groups), draw, purpose, EDTR_IMAGE_ID(s, b)));
    }
}

__global__ void __launch_bounds__(256) q_sample_rng_kernel(const float* x, const int64_t* t, const float* tab_a, const float* tab_b,
                                                          int n_tab, float* out, Stream s, int64_t n4) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / s.groups;
        int64_t ti = t[b];
        ti = ti < 0 ? 0 : (ti >= n_tab ? n_tab - 1 : ti);
        const float a = tab_a[ti], bb = tab_b[ti];
        const f32x4 z = normal4(s, (uint32_t)(g - b * s.groups), 0u, EDTR_NOISE_Q_SAMPLE, EDTR_IMAGE_ID(s, b));
        const f32x4 xv = ld4(x + g * 4);
        st4(out + g * 4, f32x4{q_sample_elem(a, xv.x, bb, z.x), q_sample_elem(a, xv.y, bb, z.y), q_sample_elem(a, xv.z, bb, z.z),
                               q_sample_elem(a, xv.w, bb, z.w)});
    }
}

// INDEXED: the coefficient row AND the draw are index[b], read on the device (clamped into the table like the tensor-noise form)
template <bool INDEXED>
__global__ void __launch_bounds__(256) sampler_update_rng_kernel(const float* x, const float* eps, const int64_t* index,
                                                                const float* coefs, int n_steps, float c_recip, float c_recipm1,
                                                                float coef1, float coef2, float sigma, uint32_t draw,
                                                                float* x_prev, float* pred_x0, Stream s, int64_t n4) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / s.groups;
        if (INDEXED) {
            int64_t k = index[b];
            k = k < 0 ? 0 : (k >= n_steps ? n_steps - 1 : k);
            const float* c = coefs + k * 5;
            c_recip = c[0], c_recipm1 = c[1], coef1 = c[2], coef2 = c[3], sigma = c[4];
            draw = (uint32_t)k;
        }
        const f32x4 z = normal4(s, (uint32_t)(g - b * s.groups), draw, EDTR_NOISE_STEP, EDTR_IMAGE_ID(s, b));
        const f32x4 xv = ld4(x + g * 4), ev = ld4(eps + g * 4);
        float p0[4], xp[4];
        sampler_update_elem(xv.x, ev.x, z.x, c_recip, c_recipm1, coef1, coef2, sigma, p0[0], xp[0]);
        sampler_update_elem(xv.y, ev.y, z.y, c_recip, c_recipm1, coef1, coef2, sigma, p0[1], xp[1]);
        sampler_update_elem(xv.z, ev.z, z.z, c_recip, c_recipm1, coef1, coef2, sigma, p0[2], xp[2]);
        sampler_update_elem(xv.w, ev.w, z.w, c_recip, c_recipm1, coef1, coef2, sigma, p0[3], xp[3]);
        if (pred_x0) st4(pred_x0 + g * 4, f32x4{p0[0], p0[1], p0[2], p0[3]});
        st4(x_prev + g * 4, f32x4{xp[0], xp[1], xp[2], xp[3]});
    }
}

// moments are NHWC rows (scalar loads, stride ld); out is NCHW, so a group is four consecutive elements of out and — when
// HW % 4 != 0 — may straddle two channels: the (channel, pixel) pair is worked out per element
__global__ void __launch_bounds__(256) gaussian_sample_rng_kernel(const float* moments, int ld, float* out, int C, int64_t HW,
                                                                 float scale, Stream s, int64_t n4) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (int64_t)gridDim.x * 256) {
        const int64_t b = g / s.groups;
        const uint32_t eg = (uint32_t)(g - b * s.groups);
        const f32x4 z = normal4(s, eg, 0u, EDTR_NOISE_VAE, EDTR_IMAGE_ID(s, b));
        const float zz[4] = {z.x, z.y, z.z, z.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t e = (int64_t)eg * 4 + j;
            const int64_t c = e / HW, px = e - c * HW;
            const float* row = moments + (b * HW + px) * ld;
            o[j] = gaussian_sample_elem(row[c], row[C + c], zz[j], scale);
        }
        st4(out + g * 4, f32x4{o[0], o[1], o[2], o[3]});
    }
}

// the checks every entry shares; fills `s`.  Nothing is launched unless this answers EDTR_OK.
int make_stream(int B, int64_t per_image, uint64_t seed, const int64_t* image_ids, int64_t image_id_base, Stream& s) {
    if (B <= 0 || per_image <= 0) return EDTR_E_SHAPE;
    if (per_image & 3) return EDTR_E_ALIGN;
    if (per_image > (int64_t)1 << 34) return EDTR_E_UNSUPPORTED;          // e >> 2 is one 32-bit counter word
    s.groups = per_image >> 2;
    return key_stream(s, B, seed, image_ids, image_id_base);
}

}  // namespace

extern "C" int edtr_normal_fill(float* out, int B, int64_t per_image, uint64_t seed, const int64_t* image_ids,
                                int64_t image_id_base, int purpose, int64_t draw, edtr_stream_t stream) {
    if (!out) return EDTR_E_NULL;
    if (purpose < EDTR_NOISE_Q_SAMPLE || purpose > EDTR_NOISE_VAE) return EDTR_E_DTYPE;
    if (!draw_ok(draw)) return EDTR_E_SHAPE;
    Stream s;
    if (int rc = make_stream(B, per_image, seed, image_ids, image_id_base, s)) return rc;
    if (!aligned16(out)) return EDTR_E_ALIGN;
    const int64_t n4 = (int64_t)B * s.groups;
    hipLaunchKernelGGL(normal_fill_kernel, dim3(blocks_for(n4)), dim3(256), 0, static_cast<hipStream_t>(stream), out, s,
                       (uint32_t)purpose, (uint32_t)draw, n4);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_q_sample_rng(const float* x, const int64_t* t, const float* tab_a, const float* tab_b, int n_tab, float* out,
                                 int B, int64_t per_image, uint64_t seed, const int64_t* image_ids, int64_t image_id_base,
                                 edtr_stream_t stream) {
    if (!x || !t || !tab_a || !tab_b || !out) return EDTR_E_NULL;
    if (n_tab <= 0) return EDTR_E_SHAPE;
    Stream s;
    if (int rc = make_stream(B, per_image, seed, image_ids, image_id_base, s)) return rc;
    if (!aligned16(x) || !aligned16(out)) return EDTR_E_ALIGN;
    const int64_t n4 = (int64_t)B * s.groups;
    hipLaunchKernelGGL(q_sample_rng_kernel, dim3(blocks_for(n4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, t, tab_a, tab_b,
                       n_tab, out, s, n4);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_sampler_update_rng(const float* x, const float* eps, float c_recip, float c_recipm1, float coef1, float coef2,
                                       float sigma, float* x_prev, float* pred_x0, int B, int64_t per_image, uint64_t seed,
                                       const int64_t* image_ids, int64_t image_id_base, int64_t draw, edtr_stream_t stream) {
    if (!x || !eps || !x_prev) return EDTR_E_NULL;
    if (!draw_ok(draw)) return EDTR_E_SHAPE;
    Stream s;
    if (int rc = make_stream(B, per_image, seed, image_ids, image_id_base, s)) return rc;
    if (!aligned16(x) || !aligned16(eps) || !aligned16(x_prev) || (pred_x0 && !aligned16(pred_x0))) return EDTR_E_ALIGN;
    const int64_t n4 = (int64_t)B * s.groups;
    hipLaunchKernelGGL(sampler_update_rng_kernel<false>, dim3(blocks_for(n4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, eps,
                       static_cast<const int64_t*>(nullptr), static_cast<const float*>(nullptr), 0, c_recip, c_recipm1, coef1, coef2,
                       sigma, (uint32_t)draw, x_prev, pred_x0, s, n4);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_sampler_update_indexed_rng(const float* x, const float* eps, const int64_t* index, const float* coefs,
                                               int n_steps, float* x_prev, float* pred_x0, int B, int64_t per_image, uint64_t seed,
                                               const int64_t* image_ids, int64_t image_id_base, edtr_stream_t stream) {
    if (!x || !eps || !index || !coefs || !x_prev) return EDTR_E_NULL;
    if (n_steps <= 0) return EDTR_E_SHAPE;
    Stream s;
    if (int rc = make_stream(B, per_image, seed, image_ids, image_id_base, s)) return rc;
    if (!aligned16(x) || !aligned16(eps) || !aligned16(x_prev) || (pred_x0 && !aligned16(pred_x0))) return EDTR_E_ALIGN;
    const int64_t n4 = (int64_t)B * s.groups;
    hipLaunchKernelGGL(sampler_update_rng_kernel<true>, dim3(blocks_for(n4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, eps,
                       index, coefs, n_steps, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u, x_prev, pred_x0, s, n4);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_gaussian_sample_rng(const float* moments, int ld, float* out, int B, int C, int64_t HW, float scale,
                                        uint64_t seed, const int64_t* image_ids, int64_t image_id_base, edtr_stream_t stream) {
    if (!moments || !out) return EDTR_E_NULL;
    if (C <= 0 || HW <= 0 || ld < 2 * C) return EDTR_E_SHAPE;
    Stream s;
    if (int rc = make_stream(B, (int64_t)C * HW, seed, image_ids, image_id_base, s)) return rc;
    if (!aligned16(out)) return EDTR_E_ALIGN;
    const int64_t n4 = (int64_t)B * s.groups;
    hipLaunchKernelGGL(gaussian_sample_rng_kernel, dim3(blocks_for(n4)), dim3(256), 0, static_cast<hipStream_t>(stream), moments, ld,
                       out, C, HW, scale, s, n4);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
