// The per-element expressions of the three kernels that consume Gaussian noise, shared by their tensor-noise form
// (elementwise.hip: noise read from memory) and their seeded form (rng.hip: noise formed in registers).  Every rounding point is
// pinned here — explicit fma where the operation is fused, contraction switched off where it is not — so that the two forms
// agree bit for bit whatever the surrounding code invites the compiler to contract.
#pragma once

// one element of the spaced-sampler update, with the rounding points fixed (explicit fma) so that the scalar-coefficient and
// the device-indexed kernels agree bit for bit
__device__ __forceinline__ void sampler_update_elem(float xv, float e, float nz, float c_recip, float c_recipm1, float coef1,
                                                    float coef2, float sigma, float& p0, float& xp) {
    p0 = __builtin_fmaf(c_recip, xv, -(c_recipm1 * e));
    const float mean = __builtin_fmaf(coef1, p0, coef2 * xv);
    xp = __builtin_fmaf(sigma, nz, mean);
}

// q_sample: a * x + b * noise as two rounded products and one rounded sum
__device__ __forceinline__ float q_sample_elem(float a, float xv, float b, float nz) {
#pragma clang fp contract(off)
    const float p = a * xv, q = b * nz;
    return p + q;
}

// VAE posterior sample: (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) * scale, the product fused into the sum
__device__ __forceinline__ float gaussian_sample_elem(float mean, float logvar, float nz, float scale) {
    const float lv = fminf(fmaxf(logvar, -30.0f), 20.0f);
    return __builtin_fmaf(expf(0.5f * lv), nz, mean) * scale;
}
