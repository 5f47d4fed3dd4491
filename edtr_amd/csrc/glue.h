// What the fp32 / uint8 glue kernels share (elementwise.hip, rng.hip, imageio.hip, degrade.hip, degrade2.hip, labels.hip, boxes.hip, coco.hip, coco_acc.hip, cls.hip, rois.hip, det_transform.hip, targets.hip, seg_loss.hip, losses.hip; no
// MFMA translation unit includes this file): the grid of a grid-stride launch, the alignment predicates and the batch check of the
// host side, and the device helpers whose roundings the numpy restatements repeat bit for bit.  ONE definition each: a rounding rule
// that lived in three files could be fixed in one and drift in the other two.
// Contraction: some of the including files switch it off at file scope and some must not, so this header carries NO file-scope
// `#pragma clang fp contract(off)`.  A function here that multiplies and adds holds the pragma in its own body (the operators
// mul_rn / add_rn below do), which travels with its instructions into whatever kernel inlines it.
#pragma once
#include "common.h"

namespace {

// ---- host side ---------------------------------------------------------------------------------------------------------------------

// the grid of every grid-stride launch of 256 lanes over n items
inline unsigned blocks_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// p is a multiple of a (a power of two; NULL is).  Also asked on the device, per image of a ragged batch.
__host__ __device__ inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// every one of p... is
template <class... P>
inline bool all_aligned_to(uintptr_t a, const P*... p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & (a - 1)) == 0;
}

// what every entry point on an fp32 [B][3][H][W] batch checks first, in this order
inline int check_batch(const void* x, const void* out, int B, int channels, int H, int W) {
    if (channels != 3) return EDTR_E_UNSUPPORTED;
    if (!x || !out) return EDTR_E_NULL;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return EDTR_E_SHAPE;
    if (H > (1 << 24) || W > (1 << 24)) return EDTR_E_UNSUPPORTED;
    if (!all_aligned_to(4, x, out)) return EDTR_E_ALIGN;
    return EDTR_OK;
}

// ---- device side -------------------------------------------------------------------------------------------------------------------

// The "no contraction" operators every bit-exact kernel is written in: a product and a sum written with them are two correctly
// rounded fp32 operations, never one FMA.  (HIP's own mul_rn-style intrinsics are plain operators compiled under the default
// -ffp-contract=fast, so a product and a sum written with them may still be fused; these three may not.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }     // IEEE: hipcc's fp32 division is correctly rounded

// v forced into [0, n): an index that no input can make stray
__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// F.pad(mode="reflect") index: the edge sample is not repeated.  One reflection is enough for k / 2 < n; the final clamp only serves
// halo positions that belong to outputs outside the image (partial tiles), which are never stored.
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// ATen's guard_index_and_lambda: idx = min(floor(src), n - 1), t = clamp(src - idx, 0, 1)
__device__ __forceinline__ void index_lambda(float src, int n, int& idx, float& t) {
    const int f = (int)floorf(src);
    idx = f < n - 1 ? f : n - 1;
    t = fminf(fmaxf(add_rn(src, -(float)idx), 0.0f), 1.0f);
}

// ATen's area_pixel_compute_source_index for align_corners = False: scale * (dst + 0.5) - 0.5, each step rounded to fp32
// (F.interpolate(size=) of degrade.hip and the coarse-logits launch of labels.hip; bilinear clamps the result at 0, bicubic does not)
__device__ __forceinline__ float source_index(float scale, int dst) {
    return add_rn(mul_rn(scale, add_rn((float)dst, 0.5f)), -0.5f);
}

// the bilinear blend of the four taps v[row][column] under the two lambdas, columns first: seven products and sums, each rounded
__device__ __forceinline__ float blend_taps(float v00, float v01, float v10, float v11, float ty, float tx) {
#pragma clang fp contract(off)
    const float wy0 = add_rn(1.0f, -ty), wx0 = add_rn(1.0f, -tx);
    const float top = add_rn(mul_rn(wx0, v00), mul_rn(tx, v01));
    const float bot = add_rn(mul_rn(wx0, v10), mul_rn(tx, v11));
    return add_rn(mul_rn(wy0, top), mul_rn(ty, bot));
}

// F.interpolate(mode="bilinear") from the point where the two index_lambda results are known: the four taps of plane `src` [ih][iw],
// columns blended first.  (How the source coordinate is formed differs between the callers and stays with them.)
__device__ __forceinline__ float bilinear_blend(const float* src, int ih, int iw, int y0, float ty, int x0, float tx) {
    const int y1 = y0 + (y0 < ih - 1 ? 1 : 0), x1 = x0 + (x0 < iw - 1 ? 1 : 0);
    const float* r0 = src + (int64_t)y0 * iw;
    const float* r1 = src + (int64_t)y1 * iw;
    return blend_taps(r0[x0], r0[x1], r1[x0], r1[x1], ty, tx);
}

// ---- coarse logits: what edtr_seg_confusion_coarse (labels.hip) and the segmentation loss (seg_loss.hip) blend alike ----------------

// element i of the coarse logits, widened exactly to fp32
template <int DT>
__device__ __forceinline__ float load1(const void* base, int64_t i) {
    if (DT == EDTR_LOGITS_F32) return static_cast<const float*>(base)[i];
    const uint16_t r = static_cast<const uint16_t*>(base)[i];
    return DT == EDTR_LOGITS_F16 ? F16::to_f32(r) : BF16::to_f32(r);
}

// an fp32 blend as F.interpolate hands it on in the input's type: rounded to nearest even to fp16 / bf16 (fp32: as it is)
template <int DT>
__device__ __forceinline__ float as_stored(float v) {
    if (DT == EDTR_LOGITS_F16) return F16::to_f32(F16::from_f32(v));
    if (DT == EDTR_LOGITS_BF16) return BF16::to_f32(BF16::from_f32(v));
    return v;
}

// one blended value as argmax sees it: the seven roundings of blend_taps, then the rounding to the input's type
template <int DT>
__device__ __forceinline__ float blended(float v00, float v01, float v10, float v11, float ty, float tx) {
    return as_stored<DT>(blend_taps(v00, v01, v10, v11, ty, tx));
}

// the lanes of a wave below `lane`, as a ballot mask: popcount(vote & lanes_below(lane)) is a lane's place in an ordered compaction
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }

// uint32 whose unsigned order is the order torch sorts fp32 scores in: every NaN is one largest key, -0.0 and 0.0 are one key
// (boxes.score_keys; the NMS rank and the per-label rank of the detection scores count with it)
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 0xffffffffu;
    if (s == 0.0f) return 0x80000000u;
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// BoxCoder.decode_single (model/util.py:702-743) for one box and one code, in the reference's operation order: the deltas divided by
// the weights, dw and dh cut at xform_clip, the centre moved and the side scaled by expf, the corners centre -/+ half a side.  Not
// clipped.  (boxes.decode_reference; the detector head's candidates and the RPN's both decode with it.)
__device__ __forceinline__ f32x4 decode_box(f32x4 pr, f32x4 r, float wx, float wy, float ww, float wh, float xform_clip) {
#pragma clang fp contract(off)
    const float width = add_rn(pr.z, -pr.x), height = add_rn(pr.w, -pr.y);
    const float ctr_x = add_rn(pr.x, mul_rn(0.5f, width)), ctr_y = add_rn(pr.y, mul_rn(0.5f, height));
    const float dx = div_rn(r.x, wx), dy = div_rn(r.y, wy);
    float dw = div_rn(r.z, ww), dh = div_rn(r.w, wh);
    dw = dw > xform_clip ? xform_clip : dw;
    dh = dh > xform_clip ? xform_clip : dh;
    const float pcx = add_rn(mul_rn(dx, width), ctr_x), pcy = add_rn(mul_rn(dy, height), ctr_y);
    const float hw = mul_rn(0.5f, mul_rn(expf(dw), width)), hh = mul_rn(0.5f, mul_rn(expf(dh), height));
    f32x4 o;
    o.x = add_rn(pcx, -hw), o.y = add_rn(pcy, -hh), o.z = add_rn(pcx, hw), o.w = add_rn(pcy, hh);
    return o;
}

// the 8-bit level of v in [0, 1] (round half to even, clamped), and v rounded to the levels and back
__device__ __forceinline__ float level8(float v) { return fminf(fmaxf(rintf(mul_rn(v, 255.0f)), 0.0f), 255.0f); }
__device__ __forceinline__ float round_to_levels(float v) { return div_rn(level8(v), 255.0f); }

}  // namespace
