// Detection boxes on the device (edtr_hip.h "Detection boxes"; the host restatements are edtr_amd/boxes.py): non-maximum suppression
// by a counting rank, a 64 x 64-blocked suppression mask and a one-workgroup scan; the candidate stage of the detector head's
// post-processing (softmax, box decoding, clip, the two filters, an ordered compaction); the per-window filter-and-shift of the tiled
// demo mode; a box transform; and the bilinear resize by a scale factor.  Boxes are fp32 [n][4] in xyxy.
// Every product, sum and quotient that decides a result bit is a correctly rounded fp32 operation in a stated order, compiled with
// contraction switched off, so numpy repeats the launches bit for bit — all but expf, which the softmax and the decoding call.
// No launch waits on another workgroup: dependent phases are separate launches, and nothing here uses an atomic.
#include "common.h"
#include "glue.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxBoxes = 32768;            // n of edtr_boxes_nms (EDTR_NMS_MAX_BOXES): 512 mask words per row, 4 KiB of LDS in the scan
constexpr int kLimit = 1 << 24;

__device__ __forceinline__ float larger(float a, float b) { return a > b ? a : b; }        // b where either is NaN
__device__ __forceinline__ float smaller(float a, float b) { return a < b ? a : b; }

// ---- non-maximum suppression -----------------------------------------------------------------------------------------------------

// order[rank(i)] = i with rank(i) = #{j : key j > key i} + #{j < i : key j == key i}: a stable descending sort by counting.
// A lane owns candidate i; the j side passes through LDS 256 keys at a time (every read is a broadcast).  Tiles are aligned with
// the workgroups, so "j < i" is decided per tile for all but the workgroup's own tile.  Keys past n are 0, which no test counts.
__global__ void __launch_bounds__(256) nms_rank_kernel(const float* scores, int n, int32_t* order) {
    __shared__ uint32_t tile[256];
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const uint32_t ki = i < n ? score_key(scores[i]) : 0xffffffffu;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        const int j = j0 + (int)threadIdx.x;
        tile[threadIdx.x] = j < n ? score_key(scores[j]) : 0u;
        __syncthreads();
        if (j0 < (int)blockIdx.x * 256) {
#pragma unroll 16
            for (int t = 0; t < 256; ++t) rank += tile[t] >= ki ? 1 : 0;
        } else if (j0 > (int)blockIdx.x * 256) {
#pragma unroll 16
            for (int t = 0; t < 256; ++t) rank += tile[t] > ki ? 1 : 0;
        } else {
#pragma unroll 16
            for (int t = 0; t < 256; ++t) rank += (tile[t] > ki || (tile[t] == ki && t < (int)threadIdx.x)) ? 1 : 0;
        }
    }
    if (i < n && rank < n) order[rank] = i;
}

__device__ __forceinline__ int64_t label_of(const void* labels, int labels_i64, int idx) {
    if (!labels) return 0;
    return labels_i64 ? static_cast<const int64_t*>(labels)[idx] : (int64_t) static_cast<const int32_t*>(labels)[idx];
}

// Workgroup (cb, rb), one wave: the block of rank-ordered rows 64 rb .. and rank-ordered columns 64 cb ..; blocks below the diagonal
// leave at once.  Lane r builds the 64-bit word of row 64 rb + r: bit c set iff column 64 cb + c comes later in the order, has the
// same label and inter / (area_r + area_c - inter) > thr.  (The rank launch writes a permutation of 0 .. n - 1; an index is forced inside
// all the same, clamp_index, so that no input can make a load stray.)
__global__ void __launch_bounds__(64) nms_mask_kernel(const float* boxes, const void* labels, int labels_i64, const int32_t* order, int n,
                                                      int words, float thr, uint64_t* mask) {
    const int cb = (int)blockIdx.x, rb = (int)blockIdx.y, lane = (int)threadIdx.x;
    if (cb < rb) return;
    __shared__ f32x4 cbox[64];
    __shared__ float carea[64];
    __shared__ int64_t clab[64];
    const int cj = cb * 64 + lane;
    f32x4 b = {0.0f, 0.0f, 0.0f, 0.0f};
    int64_t lab = 0;
    if (cj < n) {
        const int idx = clamp_index(order[cj], n);
        b = *reinterpret_cast<const f32x4*>(boxes + 4 * (int64_t)idx);
        lab = label_of(labels, labels_i64, idx);
    }
    cbox[lane] = b;
    carea[lane] = mul_rn(add_rn(b.z, -b.x), add_rn(b.w, -b.y));
    clab[lane] = lab;
    __syncthreads();
    const int ri = rb * 64 + lane;
    if (ri >= n) return;
    f32x4 rbx = b;
    int64_t rl = lab;
    if (rb != cb) {
        const int idx = clamp_index(order[ri], n);
        rbx = *reinterpret_cast<const f32x4*>(boxes + 4 * (int64_t)idx);
        rl = label_of(labels, labels_i64, idx);
    }
    const float rarea = mul_rn(add_rn(rbx.z, -rbx.x), add_rn(rbx.w, -rbx.y));
    const int ncols = n - cb * 64 < 64 ? n - cb * 64 : 64;
    const int first = rb == cb ? lane + 1 : 0;          // only later candidates are suppressed
    uint32_t half[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll 8
        for (int t = 0; t < 32; ++t) {
            const int c = 32 * h + t;
            const f32x4 q = cbox[c];
            const float w = add_rn(smaller(rbx.z, q.z), -larger(rbx.x, q.x));
            const float hh = add_rn(smaller(rbx.w, q.w), -larger(rbx.y, q.y));
            const float inter = mul_rn(w > 0.0f ? w : 0.0f, hh > 0.0f ? hh : 0.0f);
            const float iou = div_rn(inter, add_rn(add_rn(rarea, carea[c]), -inter));
            const bool hit = iou > thr && clab[c] == rl && c >= first && c < ncols;
            half[h] |= (hit ? 1u : 0u) << t;
        }
    }
    mask[(int64_t)ri * words + cb] = (uint64_t)half[0] | ((uint64_t)half[1] << 32);
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// One wave walks the candidates in rank order.  The removed-set lives in LDS, `words` words; the word of the current block of 64
// candidates is held in a register, so the walk inside a block touches neither LDS nor a barrier.  A kept candidate ORs its row into
// the words after the current one, lane by lane (a loop once there are more than 64 of them).  The walk ends when max_out candidates
// are kept; keep[kept ..] is filled with -1 and *count = kept.
__global__ void __launch_bounds__(64) nms_scan_kernel(const uint64_t* mask, const int32_t* order, int n, int words, int64_t* keep,
                                                      int max_out, int32_t* count) {
    __shared__ uint64_t removed[kMaxBoxes / 64];
    const int lane = (int)threadIdx.x;
    for (int k = lane; k < words; k += 64) removed[k] = 0ull;
    int kept = 0;
    for (int w = 0; w < words && kept < max_out; ++w) {
        __syncthreads();
        const uint64_t cur = uniform64(removed[w]);
        const int left = n - w * 64;
        const uint64_t valid = left >= 64 ? ~0ull : lanes_below(left);
        uint64_t todo = ~cur & valid;
        while (todo && kept < max_out) {
            const int i = w * 64 + __builtin_ctzll(todo);
            if (lane == 0) keep[kept] = (int64_t)order[i];
            ++kept;
            const uint64_t* row = mask + (int64_t)i * words;
            const uint64_t rw = uniform64(row[w]);
            for (int k = w + 1 + lane; k < words; k += 64) removed[k] |= row[k];
            todo &= todo - 1ull;
            todo &= ~rw;
        }
    }
    for (int k = kept + lane; k < max_out; k += 64) keep[k] = -1;
    if (lane == 0) *count = kept;
}

// ---- the candidate stage of RoIHeads.postprocess_detections ------------------------------------------------------------------------

struct CandParams {
    const float* logits;        // [P][C]
    const float* regression;    // [P][4 C]
    const float* proposals;     // [P][4]
    int P, C;
    float img_w, img_h, score_thresh, min_size, wx, wy, ww, wh, xform_clip;
    float* cand_boxes;          // [P (C - 1)][4]
    float* cand_scores;         // [P (C - 1)]
    uint8_t* flags;             // [P (C - 1)]
    int32_t* block_counts;      // [ceil(P / 4)]
};

__device__ __forceinline__ float clamp_to(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

// One wave per proposal row, four rows per workgroup: softmax over the row (maximum and sum by wave reduction), then for every
// class but the background BoxCoder.decode_single in the reference's operation order, the clip to the image and the flag
// score > score_thresh && width >= min_size && height >= min_size.  The workgroup's count of flagged candidates goes to block_counts.
__global__ void __launch_bounds__(256) det_candidates_kernel(CandParams a) {
    __shared__ int wcount[4];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int p = (int)blockIdx.x * 4 + wave;
    int cnt = 0;
    if (p < a.P) {
        const float* row = a.logits + (int64_t)p * a.C;
        float m = -INFINITY;
        for (int c = lane; c < a.C; c += 64) m = fmaxf(m, row[c]);
        m = wave_max(m);
        float s = 0.0f;
        for (int c = lane; c < a.C; c += 64) s = add_rn(s, expf(add_rn(row[c], -m)));
        s = wave_sum(s);
        const f32x4 pr = *reinterpret_cast<const f32x4*>(a.proposals + 4 * (int64_t)p);
        for (int c0 = 1; c0 < a.C; c0 += 64) {
            const int c = c0 + lane;
            bool flag = false;
            if (c < a.C) {
                const float score = div_rn(expf(add_rn(row[c], -m)), s);
                const f32x4 r = *reinterpret_cast<const f32x4*>(a.regression + ((int64_t)p * a.C + c) * 4);
                const f32x4 d = decode_box(pr, r, a.wx, a.wy, a.ww, a.wh, a.xform_clip);
                f32x4 o;
                o.x = clamp_to(d.x, a.img_w);
                o.y = clamp_to(d.y, a.img_h);
                o.z = clamp_to(d.z, a.img_w);
                o.w = clamp_to(d.w, a.img_h);
                const int64_t k = (int64_t)p * (a.C - 1) + (c - 1);
                *reinterpret_cast<f32x4*>(a.cand_boxes + 4 * k) = o;
                a.cand_scores[k] = score;
                flag = score > a.score_thresh && add_rn(o.z, -o.x) >= a.min_size && add_rn(o.w, -o.y) >= a.min_size;
                a.flags[k] = flag ? 1 : 0;
            }
            cnt += __popcll(__ballot(flag));
        }
    }
    if (lane == 0) wcount[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) a.block_counts[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
}

// counts [nb] -> offsets [nb] (exclusive prefix sums) and *total, by one workgroup: 256 counts at a time, a carry between the rounds
__global__ void __launch_bounds__(256) det_offsets_kernel(const int32_t* counts, int nb, int32_t* offsets, int32_t* total) {
    __shared__ int buf[256];
    const int tid = (int)threadIdx.x;
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int v = base + tid < nb ? counts[base + tid] : 0;
        buf[tid] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = tid >= o ? buf[tid - o] : 0;
            __syncthreads();
            buf[tid] += add;
            __syncthreads();
        }
        if (base + tid < nb) offsets[base + tid] = carry + buf[tid] - v;
        carry += buf[255];
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// the flagged candidates of det_candidates_kernel, in candidate-index order p (C - 1) + (c - 1), to out_* from offsets[workgroup] on
__global__ void __launch_bounds__(256) det_scatter_kernel(const float* cand_boxes, const float* cand_scores, const uint8_t* flags, int P,
                                                          int C, const int32_t* offsets, float* out_boxes, float* out_scores,
                                                          int32_t* out_labels, int64_t capacity) {
    __shared__ int wcount[4];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int p = (int)blockIdx.x * 4 + wave;
    int cnt = 0;
    if (p < P)
        for (int c0 = 1; c0 < C; c0 += 64) {
            const int c = c0 + lane;
            cnt += __popcll(__ballot(c < C && flags[(int64_t)p * (C - 1) + (c - 1)] != 0));
        }
    if (lane == 0) wcount[wave] = cnt;
    __syncthreads();
    if (p >= P) return;
    int64_t base = offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wcount[w];
    for (int c0 = 1; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const int64_t k = (int64_t)p * (C - 1) + (c - 1);
        const bool flag = c < C && flags[k] != 0;
        const uint64_t vote = __ballot(flag);
        const int64_t pos = base + __popcll(vote & lanes_below(lane));
        if (flag && pos < capacity) {
            *reinterpret_cast<f32x4*>(out_boxes + 4 * pos) = *reinterpret_cast<const f32x4*>(cand_boxes + 4 * k);
            out_scores[pos] = cand_scores[k];
            out_labels[pos] = c;
        }
        base += __popcll(vote);
    }
}

// ---- the tiled mode's per-window step, the box transform and the resize by a scale factor ------------------------------------------

// One workgroup: the boxes with score >= score_min, in their order, shifted by (dx, dy), appended to out_* at *offset, which is moved
// on.  Nothing is written at or past `capacity`.
__global__ void __launch_bounds__(256) filter_shift_kernel(const float* boxes, const float* scores, const int64_t* labels, int n,
                                                           float score_min, float dx, float dy, float* out_boxes, float* out_scores,
                                                           int32_t* out_labels, int32_t* offset, int capacity) {
    __shared__ int wsum[4];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int base = *offset;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool flag = i < n && scores[i] >= score_min;
        const uint64_t vote = __ballot(flag);
        __syncthreads();                        // the sums of the round before have been read
        if (lane == 0) wsum[wave] = __popcll(vote);
        __syncthreads();
        int pos = base + __popcll(vote & lanes_below(lane));
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        if (flag && pos < capacity) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(boxes + 4 * (int64_t)i);
            f32x4 o;
            o.x = add_rn(b.x, dx), o.y = add_rn(b.y, dy), o.z = add_rn(b.z, dx), o.w = add_rn(b.w, dy);
            *reinterpret_cast<f32x4*>(out_boxes + 4 * (int64_t)pos) = o;
            out_scores[pos] = scores[i];
            out_labels[pos] = (int32_t)labels[i];
        }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
    __syncthreads();                            // every lane has read *offset
    if (tid == 0) *offset = base < capacity ? base : capacity;
}

__device__ __forceinline__ float transform1(float v, int flags, float shift, float factor, float hi) {
    if (flags & EDTR_BOX_SHIFT) v = add_rn(v, shift);
    if (flags & EDTR_BOX_MUL) v = mul_rn(v, factor);
    if (flags & EDTR_BOX_DIV) v = div_rn(v, factor);
    if (flags & EDTR_BOX_CLIP) v = clamp_to(v, hi);
    return v;
}

__global__ void __launch_bounds__(256) box_transform_kernel(const float* src, float* dst, int n, int flags, float dx, float dy, float fx,
                                                            float fy, float clip_w, float clip_h) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(src + 4 * i);
        f32x4 o;
        o.x = transform1(b.x, flags, dx, fx, clip_w);
        o.y = transform1(b.y, flags, dy, fy, clip_h);
        o.z = transform1(b.z, flags, dx, fx, clip_w);
        o.w = transform1(b.w, flags, dy, fy, clip_h);
        *reinterpret_cast<f32x4*>(dst + 4 * i) = o;
    }
}

// F.interpolate(scale_factor=, mode="bilinear", align_corners=False): one lane per output element; the source coordinate is
// max(fma(rscale, dst + 0.5, -0.5), 0) with rscale = fp32(1 / scale_factor) handed in by the caller.  The fma is torch's: its
// builds contract area_pixel_compute_source_index, and with two roundings there the weights come out up to 2e-6 away from torch's.
__global__ void __launch_bounds__(256) bilinear_scale_kernel(const float* x, float* out, int planes, int ih, int iw, int oh, int ow,
                                                             float rh, float rw) {
    const int64_t total = (int64_t)planes * oh * ow;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t py = e / ow;
        const int ox = (int)(e - py * ow), p = (int)(py / oh), oy = (int)(py - (int64_t)p * oh);
        const float* src = x + (int64_t)p * ih * iw;
        int y0, x0;
        float ty, tx;
        index_lambda(fmaxf(__builtin_fmaf(rh, add_rn((float)oy, 0.5f), -0.5f), 0.0f), ih, y0, ty);
        index_lambda(fmaxf(__builtin_fmaf(rw, add_rn((float)ox, 0.5f), -0.5f), 0.0f), iw, x0, tx);
        y0 = y0 < 0 ? 0 : y0, x0 = x0 < 0 ? 0 : x0;
        out[e] = bilinear_blend(src, ih, iw, y0, ty, x0, tx);
    }
}

}  // namespace

extern "C" int edtr_boxes_rank(const float* scores, int n, int32_t* order, edtr_stream_t stream) {
    if (!scores || !order) return EDTR_E_NULL;
    if (n <= 0) return EDTR_E_SHAPE;
    if (n > kMaxBoxes) return EDTR_E_UNSUPPORTED;
    if (!aligned_to(scores, 4) || !aligned_to(order, 4)) return EDTR_E_ALIGN;
    hipLaunchKernelGGL(nms_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), scores, n, order);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_boxes_nms(const float* boxes, const float* scores, const void* labels, int labels_i64, int n, float iou_threshold,
                              int32_t* order, uint64_t* mask, int64_t* keep, int max_out, int32_t* count, edtr_stream_t stream) {
    static_assert(kMaxBoxes == EDTR_NMS_MAX_BOXES, "edtr_hip.h and boxes.hip disagree on the candidate limit");
    if (!boxes || !scores || !order || !mask || !keep || !count) return EDTR_E_NULL;
    if (n <= 0 || max_out <= 0) return EDTR_E_SHAPE;
    if (n > kMaxBoxes) return EDTR_E_UNSUPPORTED;
    if (labels_i64 != 0 && labels_i64 != 1) return EDTR_E_DTYPE;
    if (!aligned_to(boxes, 16) || !aligned_to(scores, 4) || !aligned_to(order, 4) || !aligned_to(mask, 8) || !aligned_to(keep, 8) ||
        !aligned_to(count, 4) || !aligned_to(labels, labels_i64 ? 8 : 4))
        return EDTR_E_ALIGN;
    const int words = (n + 63) / 64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nms_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scores, n, order);
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(nms_mask_kernel, dim3((unsigned)words, (unsigned)words), dim3(64), 0, st, boxes, labels, labels_i64, order, n, words,
                       iou_threshold, mask);
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(64), 0, st, mask, order, n, words, keep, max_out, count);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_boxes_candidates(const float* logits, const float* regression, const float* proposals, int P, int C, float img_h,
                                     float img_w, float score_thresh, float min_size, const float* weights, float xform_clip,
                                     float* cand_boxes, float* cand_scores, uint8_t* flags, int32_t* block_counts, float* out_boxes,
                                     float* out_scores, int32_t* out_labels, int32_t* count, edtr_stream_t stream) {
    if (!logits || !regression || !proposals || !weights || !cand_boxes || !cand_scores || !flags || !block_counts || !out_boxes ||
        !out_scores || !out_labels || !count)
        return EDTR_E_NULL;
    if (P <= 0 || C < 2) return EDTR_E_SHAPE;
    if (P > kLimit || C > kLimit || (int64_t)P * C > kLimit) return EDTR_E_UNSUPPORTED;
    for (int i = 0; i < 4; ++i)
        if (!(weights[i] == weights[i]) || weights[i] == 0.0f) return EDTR_E_SHAPE;
    if (!aligned_to(logits, 4) || !aligned_to(regression, 16) || !aligned_to(proposals, 16) || !aligned_to(cand_boxes, 16) ||
        !aligned_to(cand_scores, 4) || !aligned_to(block_counts, 4) || !aligned_to(out_boxes, 16) || !aligned_to(out_scores, 4) ||
        !aligned_to(out_labels, 4) || !aligned_to(count, 4))
        return EDTR_E_ALIGN;
    const int nb = (P + 3) / 4;
    CandParams a;
    a.logits = logits, a.regression = regression, a.proposals = proposals, a.P = P, a.C = C;
    a.img_w = img_w, a.img_h = img_h, a.score_thresh = score_thresh, a.min_size = min_size;
    a.wx = weights[0], a.wy = weights[1], a.ww = weights[2], a.wh = weights[3], a.xform_clip = xform_clip;
    a.cand_boxes = cand_boxes, a.cand_scores = cand_scores, a.flags = flags, a.block_counts = block_counts;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(det_candidates_kernel, dim3((unsigned)nb), dim3(256), 0, st, a);
    EDTR_LAUNCH_CHECK();
    // (the offsets overwrite the counts in place: a lane reads its count before the round's first barrier and writes after its last)
    hipLaunchKernelGGL(det_offsets_kernel, dim3(1), dim3(256), 0, st, block_counts, nb, block_counts, count);
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(det_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, st, cand_boxes, cand_scores, flags, P, C, block_counts, out_boxes,
                       out_scores, out_labels, (int64_t)P * (C - 1));
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_boxes_filter_shift(const float* boxes, const float* scores, const int64_t* labels, int n, float score_min, float dx,
                                       float dy, float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* offset, int capacity,
                                       edtr_stream_t stream) {
    if (!boxes || !scores || !labels || !out_boxes || !out_scores || !out_labels || !offset) return EDTR_E_NULL;
    if (n <= 0 || capacity <= 0) return EDTR_E_SHAPE;
    if (n > kLimit || capacity > kLimit) return EDTR_E_UNSUPPORTED;
    if (!aligned_to(boxes, 16) || !aligned_to(scores, 4) || !aligned_to(labels, 8) || !aligned_to(out_boxes, 16) || !aligned_to(out_scores, 4) ||
        !aligned_to(out_labels, 4) || !aligned_to(offset, 4))
        return EDTR_E_ALIGN;
    hipLaunchKernelGGL(filter_shift_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), boxes, scores, labels, n, score_min, dx, dy,
                       out_boxes, out_scores, out_labels, offset, capacity);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_boxes_transform(const float* src, float* dst, int n, int flags, float dx, float dy, float fx, float fy, float clip_w,
                                    float clip_h, edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (n <= 0) return EDTR_E_SHAPE;
    if (n > kLimit) return EDTR_E_UNSUPPORTED;
    if (flags & ~(EDTR_BOX_SHIFT | EDTR_BOX_MUL | EDTR_BOX_DIV | EDTR_BOX_CLIP)) return EDTR_E_DTYPE;
    if ((flags & EDTR_BOX_MUL) && (flags & EDTR_BOX_DIV)) return EDTR_E_DTYPE;
    if (!aligned_to(src, 16) || !aligned_to(dst, 16)) return EDTR_E_ALIGN;
    hipLaunchKernelGGL(box_transform_kernel, dim3(blocks_for(n)), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst, n, flags, dx, dy, fx,
                       fy, clip_w, clip_h);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_boxes_bilinear_scale(const float* src, float* dst, int planes, int ih, int iw, int oh, int ow, float rscale_h,
                                         float rscale_w, edtr_stream_t stream) {
    if (!src || !dst) return EDTR_E_NULL;
    if (planes <= 0 || ih <= 0 || iw <= 0 || oh <= 0 || ow <= 0) return EDTR_E_SHAPE;
    if (!(rscale_h > 0.0f) || !(rscale_w > 0.0f)) return EDTR_E_SHAPE;
    if (planes > kLimit || ih > kLimit || iw > kLimit || oh > kLimit || ow > kLimit) return EDTR_E_UNSUPPORTED;
    if (!aligned_to(src, 4) || !aligned_to(dst, 4)) return EDTR_E_ALIGN;
    hipLaunchKernelGGL(bilinear_scale_kernel, dim3(blocks_for((int64_t)planes * oh * ow)), dim3(256), 0, static_cast<hipStream_t>(stream), src,
                       dst, planes, ih, iw, oh, ow, rscale_h, rscale_w);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
