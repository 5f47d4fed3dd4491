// The seeded normal stream of edtr_hip.h "Reproducible noise", shared by the kernels that draw from it (rng.hip, degrade.hip):
// Philox4x32-10 on the counter (e >> 2, draw, purpose, image id) and the Box-Muller step that turns its four words into the
// normals of four consecutive elements.  One definition, so that every consumer gives the same bits for the same counter.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c.x), l0 = 0xD2511F53u * c.x;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c.z), l1 = 0xCD9E8D57u * c.z;
        c = u32x4{h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// two words -> two normals.  Both uniforms are exact in fp32 (24-bit integers times 2^-24), u1 in (0, 1]: no log(0), |z| <= 5.77.
// Accurate logf / sqrtf and an exactly reduced angle (sincospif of 2 u2, itself exact): the host reference has to agree to 1e-5.
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& za, float& zb) {
    const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(xb >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    za = r * c;
    zb = r * s;
}

// the normals of elements 4 * eg + 0..3 of image `id` under key (k0, k1)
__device__ __forceinline__ f32x4 philox_normal4(uint32_t k0, uint32_t k1, uint32_t eg, uint32_t draw, uint32_t purpose, uint32_t id) {
    const u32x4 w = philox4x32_10(u32x4{eg, draw, purpose, id}, k0, k1);
    float z0, z1, z2, z3;
    box_muller(w.x, w.y, z0, z1);
    box_muller(w.z, w.w, z2, z3);
    return f32x4{z0, z1, z2, z3};
}

}  // namespace
