// The seeded normal stream of edtr_hip.h "Reproducible noise", shared by the kernels that draw from it (rng.hip, degrade.hip,
// degrade2.hip, targets.hip): Philox4x32-10 on the counter (e >> 2, draw, purpose, image id) and the Box-Muller step that turns its four words
// into the normals of four consecutive elements; and how an entry point turns (seed, image_ids, image_id_base, draw) into the
// arguments of a launch.  One definition, so that every consumer gives the same bits, and the same answers, for the same stream.
#pragma once
#include "glue.h"

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

// The raw words of the stream (rng.uniform_words_reference): element e of image `id` receives word e & 3 of the call on the counter
// (e >> 2, draw, purpose, id); word_of picks it without indexing the vector.  edtr_targets_sample ranks boxes by these words under
// EDTR_NOISE_SAMPLE_RPN / EDTR_NOISE_SAMPLE_ROI, a lane owning the four boxes of one call.
__device__ __forceinline__ uint32_t word_of(u32x4 w, int j) { return j == 0 ? w.x : (j == 1 ? w.y : (j == 2 ? w.z : w.w)); }

// ---- a stream's launch arguments.  A struct with k0, k1, ids, id_base names the stream; rng.hip's has its own layout. ------------

// the global id of image b of stream s: ids[b], or id_base + b without ids.  (A macro: as an inlined function the expression is
// scheduled differently inside the degradation kernels, and their code is pinned.)
#define EDTR_IMAGE_ID(s, b) ((s).ids ? (uint32_t)(s).ids[b] : (s).id_base + (uint32_t)(b))

inline bool draw_ok(int64_t draw) { return draw >= 0 && draw < (int64_t)1 << 32; }       // one 32-bit counter word

// the checks on the image ids every seeded entry shares, then the key and the ids into `s`
template <class S>
inline int key_stream(S& s, int B, uint64_t seed, const int64_t* image_ids, int64_t image_id_base) {
    if (!aligned_to(image_ids, 8)) return EDTR_E_ALIGN;
    if (!image_ids && (image_id_base < 0 || image_id_base + B > (int64_t)1 << 32)) return EDTR_E_SHAPE;
    s.k0 = (uint32_t)(seed & 0xffffffffu);
    s.k1 = (uint32_t)(seed >> 32);
    s.ids = image_ids;
    s.id_base = (uint32_t)image_id_base;
    return EDTR_OK;
}

struct NoiseArgs {          // the seeded noise launches on an fp32 [B][3][H][W] batch (degrade.hip, degrade2.hip), passed by value
    uint32_t k0, k1;
    const int64_t* ids;     // [B] global image ids, or NULL: id_base + b
    uint32_t id_base, draw;
    int64_t plane4;         // H W / 4: groups of four elements per plane
    int rounds;
};

// What those two entries check between their NULL checks and the alignment of their own device arrays, in this order; fills `a`.
// amount_host: the per-image sigma / scale.  H W up to 2^32 (rng.hip's per_image goes to 2^34: its groups are of a whole image).
inline int make_noise_args(NoiseArgs& a, const float* x, const float* out, const float* noise_out, int B, int H, int W,
                           const float* amount_host, const int32_t* gray_host, uint64_t seed, const int64_t* image_ids,
                           int64_t image_id_base, int64_t draw, int rounds) {
    if (rounds != 0 && rounds != 1) return EDTR_E_DTYPE;
    if (!draw_ok(draw)) return EDTR_E_SHAPE;
    const int64_t hw = (int64_t)H * W;
    if (hw & 3) return EDTR_E_ALIGN;                                // per_image = 3 H W (colour) or H W (grey), both multiples of 4
    if (hw > (int64_t)1 << 32) return EDTR_E_UNSUPPORTED;           // e >> 2 is one 32-bit counter word
    for (int b = 0; b < B; ++b) {
        if (!(amount_host[b] >= 0.0f) || amount_host[b] > 3.0e38f) return EDTR_E_SHAPE;
        if (gray_host[b] != 0 && gray_host[b] != 1) return EDTR_E_DTYPE;
    }
    if (int rc = key_stream(a, B, seed, image_ids, image_id_base)) return rc;
    if (!all_aligned_to(16, x, out, noise_out)) return EDTR_E_ALIGN;
    a.draw = (uint32_t)draw;
    a.plane4 = hw >> 2;
    a.rounds = rounds;
    return EDTR_OK;
}

}  // namespace
