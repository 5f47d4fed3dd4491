// Detection scores on the device (edtr_hip.h "Detection scores"; the host restatement and the rule itself are edtr_amd/coco.py): one
// image's detections matched against its ground truth as COCOeval.evaluateImg does, for every label, IoU threshold and area range at
// once, appended to a running record whose two offsets stay on the device.
// Coordinates arrive as fp32 xyxy; w = x2 - x1 and h = y2 - y1 are fp32, everything after is fp64 with each operation rounded
// (contraction is off: (da + ga) - iw * ih must not become an FMA), so numpy repeats the launch bit for bit.
// Every record word has exactly one writer; no launch waits on another workgroup and nothing here uses an atomic: the offsets are
// moved on by a dependent one-workgroup launch.
#include "common.h"
#include "glue.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxDet = 1024;       // EDTR_COCO_MAX_DET: the detections of one image
constexpr int kMaxGt = 1024;        // EDTR_COCO_MAX_GT: the ground truths of one image
constexpr int kMaxLabels = 256;     // EDTR_COCO_MAX_LABELS
constexpr int kMaxThr = 10;         // EDTR_COCO_MAX_THRESHOLDS: with the four area ranges, 40 of a word's 64 bits
constexpr int kKeep = 100;          // EDTR_COCO_KEEP: the ranks of a label that are matched (the largest maxDets)
constexpr int kCrowd = 16;          // bit of a ground truth's flag byte beside the four ignore bits
constexpr int kMaxRows = 1 << 30;   // capacity, and where a running offset stops moving

struct MatchArgs {
    const float* det_boxes;         // [n][4]
    const float* det_scores;        // [n]
    const void* det_labels;         // [n]
    const int32_t* count;           // NULL or the number of rows that exist
    const float* gt_boxes;          // [g][4]
    const void* gt_labels;          // [g]
    const float* gt_area;           // [g]
    const uint8_t* gt_crowd;        // [g]
    const double* thresholds;       // [n_thr]
    const double* areas;            // [4][2]
    int n, g, labels_i64, n_labels, n_thr, image_id, capacity, gt_capacity;
    int32_t* rec_image;
    int32_t* rec_label;
    float* rec_score;
    int32_t* rec_rank;
    uint64_t* rec_match;
    uint64_t* rec_ignore;
    int32_t* gt_image;
    int32_t* gt_label;
    uint8_t* gt_ignore;
    const int32_t* det_offset;
    const int32_t* gt_offset;
};

__device__ __forceinline__ int64_t label_at(const void* labels, int labels_i64, int idx) {
    return labels_i64 ? static_cast<const int64_t*>(labels)[idx] : (int64_t) static_cast<const int32_t*>(labels)[idx];
}

__device__ __forceinline__ int rows_that_exist(const int32_t* count, int n) {
    if (!count) return n;
    const int c = *count;
    return c < 0 ? 0 : (c > n ? n : c);
}

// the ignore bits of one ground truth: bit a set iff it is a crowd or its area lies outside [lo_a, hi_a]
__device__ __forceinline__ int ignore_bits(float area, bool crowd, const double* areas) {
    const double ar = (double)area;
    int bits = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) bits |= (crowd || ar < areas[2 * a] || ar > areas[2 * a + 1]) ? (1 << a) : 0;
    return bits;
}

__device__ __forceinline__ double lesser(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double greater(double a, double b) { return a > b ? a : b; }

// One wave64 workgroup per label value k = blockIdx.x, and one more (k == n_labels) that writes what does not depend on the matching:
// image, label and score of every detection row, the whole record of a row whose label lies outside [0, n_labels) (rank -1, zero
// words), and the ground-truth records.  So every word of a row has one writer.
// A label's workgroup:
//   1  compacts the label's detections into LDS in input order (ballot + popcount) with their score keys;
//   2  ranks them by counting — rank(i) = #{j : key j > key i} + #{j before i : key j == key i}, the rule of edtr_boxes_rank — writes
//      the rank, zero words for rank >= 100, and the input index of every rank < 100 into `top`;
//   3  compacts the label's ground truths (x1, y1, w, h in fp32, a flag byte) and, per area range, their walking order: those not
//      ignored in input order, then the ignored in input order;
//   4  walks the kept detections in rank order.  Per detection the wave first fills one row of IoUs (fp64, lane p mod 64 owns ground
//      truth p); then lane 4 t + a owns the pair (threshold t, area range a) and walks the ground truths in the order of a with its own
//      matched-set bits (a column of `taken`).  The two ballots over the lanes are the row's two record words.
__global__ void __launch_bounds__(64) coco_match_kernel(MatchArgs a) {
    __shared__ f32x4 gbox[kMaxGt];
    __shared__ double iou[kMaxGt];
    __shared__ uint32_t dkey[kMaxDet];
    __shared__ uint32_t taken[kMaxGt / 32][64];
    __shared__ uint16_t gorder[4][kMaxGt];
    __shared__ uint16_t dlist[kMaxDet];
    __shared__ uint16_t top[kKeep];
    __shared__ uint8_t gflag[kMaxGt];

    const int lane = (int)threadIdx.x, k = (int)blockIdx.x;
    const int d = rows_that_exist(a.count, a.n);
    const int64_t doff = *a.det_offset, goff = *a.gt_offset;
    const bool det_room = doff >= 0, gt_room = goff >= 0;       // (an offset the caller broke writes nothing)

    if (k == a.n_labels) {
        for (int i = lane; i < d; i += 64) {
            const int64_t row = doff + i;
            if (!det_room || row >= a.capacity) continue;
            const int64_t lab = label_at(a.det_labels, a.labels_i64, i);
            const bool known = lab >= 0 && lab < a.n_labels;
            a.rec_image[row] = a.image_id;
            a.rec_label[row] = known ? (int32_t)lab : -1;
            a.rec_score[row] = a.det_scores[i];
            if (!known) {
                a.rec_rank[row] = -1;
                a.rec_match[row] = 0ull;
                a.rec_ignore[row] = 0ull;
            }
        }
        for (int j = lane; j < a.g; j += 64) {
            const int64_t row = goff + j;
            if (!gt_room || row >= a.gt_capacity) continue;
            const int64_t lab = label_at(a.gt_labels, a.labels_i64, j);
            a.gt_image[row] = a.image_id;
            a.gt_label[row] = (lab >= 0 && lab < a.n_labels) ? (int32_t)lab : -1;
            a.gt_ignore[row] = (uint8_t)ignore_bits(a.gt_area[j], a.gt_crowd[j] != 0, a.areas);
        }
        return;
    }

    // 1: this label's detections, in input order
    int nd = 0;
    for (int i0 = 0; i0 < d; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < d && label_at(a.det_labels, a.labels_i64, i) == (int64_t)k;
        const uint64_t vote = __ballot(mine);
        if (mine) {
            const int pos = nd + __popcll(vote & lanes_below(lane));
            dlist[pos] = (uint16_t)i;
            dkey[pos] = score_key(a.det_scores[i]);
        }
        nd += __popcll(vote);
    }
    if (nd == 0) return;            // (uniform: nothing of this label to record)
    __syncthreads();

    // 2: the counting rank; the j side is a broadcast read
    for (int m = lane; m < nd; m += 64) {
        const uint32_t km = dkey[m];
        int rank = 0;
        for (int j = 0; j < nd; ++j) {
            const uint32_t kj = dkey[j];
            rank += (kj > km || (kj == km && j < m)) ? 1 : 0;
        }
        const int i = (int)dlist[m];
        const int64_t row = doff + i;
        if (rank < kKeep) top[rank] = (uint16_t)i;
        if (det_room && row < a.capacity) {
            a.rec_rank[row] = rank;
            if (rank >= kKeep) {
                a.rec_match[row] = 0ull;
                a.rec_ignore[row] = 0ull;
            }
        }
    }

    // 3: this label's ground truths, in input order, and their walking order per area range
    int ng = 0;
    for (int j0 = 0; j0 < a.g; j0 += 64) {
        const int j = j0 + lane;
        const bool mine = j < a.g && label_at(a.gt_labels, a.labels_i64, j) == (int64_t)k;
        const uint64_t vote = __ballot(mine);
        if (mine) {
            const int pos = ng + __popcll(vote & lanes_below(lane));
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.gt_boxes + 4 * (int64_t)j);
            f32x4 o;
            o.x = b.x, o.y = b.y, o.z = add_rn(b.z, -b.x), o.w = add_rn(b.w, -b.y);
            const bool crowd = a.gt_crowd[j] != 0;
            gbox[pos] = o;
            gflag[pos] = (uint8_t)(ignore_bits(a.gt_area[j], crowd, a.areas) | (crowd ? kCrowd : 0));
        }
        ng += __popcll(vote);
    }
    __syncthreads();
    for (int ar = 0; ar < 4; ++ar) {
        int base = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int p0 = 0; p0 < ng; p0 += 64) {
                const int p = p0 + lane;
                const bool mine = p < ng && ((gflag[p] >> ar) & 1) == pass;
                const uint64_t vote = __ballot(mine);
                if (mine) gorder[ar][base + __popcll(vote & lanes_below(lane))] = (uint16_t)p;
                base += __popcll(vote);
            }
    }
    for (int w = 0; w < kMaxGt / 32; ++w) taken[w][lane] = 0u;
    __syncthreads();

    // 4: the walk
    const int t = lane >> 2, ar = lane & 3;
    const bool active = t < a.n_thr;
    const double thr = active ? a.thresholds[t] : 1.0;
    const double best0 = lesser(thr, 1.0 - 1e-10);
    const double lo = a.areas[2 * ar], hi = a.areas[2 * ar + 1];
    const int kept = nd < kKeep ? nd : kKeep;
    for (int r = 0; r < kept; ++r) {
        const int i = (int)top[r];
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.det_boxes + 4 * (int64_t)i);
        const double dx = (double)b.x, dy = (double)b.y, dw = (double)add_rn(b.z, -b.x), dh = (double)add_rn(b.w, -b.y);
        const double da = dw * dh;
        for (int p = lane; p < ng; p += 64) {
            const f32x4 q = gbox[p];
            const double gx = (double)q.x, gy = (double)q.y, gw = (double)q.z, gh = (double)q.w;
            const double ga = gw * gh;
            const double iw = lesser(dx + dw, gx + gw) - greater(dx, gx);
            const double ih = lesser(dy + dh, gy + gh) - greater(dy, gy);
            double v = 0.0;
            if (iw > 0.0 && ih > 0.0) {
                const double inter = iw * ih;
                const double uni = (gflag[p] & kCrowd) ? da : (da + ga) - inter;
                v = inter / uni;
            }
            iou[p] = v;
        }
        __syncthreads();
        int m = -1;
        bool m_ignored = false;
        if (active) {
            double best = best0;
            for (int s = 0; s < ng; ++s) {
                const int p = (int)gorder[ar][s];
                const int flag = (int)gflag[p];
                const bool ignored = (flag >> ar) & 1;
                if (((taken[s >> 5][lane] >> (s & 31)) & 1u) && !(flag & kCrowd)) continue;
                if (m >= 0 && !m_ignored && ignored) break;
                const double v = iou[p];
                if (v < best) continue;
                best = v, m = s, m_ignored = ignored;
            }
            if (m >= 0) taken[m >> 5][lane] |= 1u << (m & 31);
        }
        const bool matched = m >= 0;
        const bool row_ignored = active && (matched ? m_ignored : (da < lo || da > hi));
        const uint64_t match_word = __ballot(matched), ignore_word = __ballot(row_ignored);
        const int64_t row = doff + i;
        if (lane == 0 && det_room && row < a.capacity) {
            a.rec_match[row] = match_word;
            a.rec_ignore[row] = ignore_word;
        }
        __syncthreads();            // the row of IoUs is overwritten for the next detection
    }
}

__device__ __forceinline__ int32_t moved_on(int32_t offset, int by) { return offset < 0 || offset > kMaxRows ? offset : offset + by; }

// the dependent launch: both offsets moved on by what the image appended, whether or not it fitted (the host sees the overflow)
__global__ void __launch_bounds__(64) coco_advance_kernel(const int32_t* count, int n, int g, int32_t* det_offset, int32_t* gt_offset) {
    if (threadIdx.x != 0) return;
    *det_offset = moved_on(*det_offset, rows_that_exist(count, n));
    *gt_offset = moved_on(*gt_offset, g);
}

}  // namespace

extern "C" int edtr_coco_match(const float* det_boxes, const float* det_scores, const void* det_labels, int n, const int32_t* count,
                               const float* gt_boxes, const void* gt_labels, const float* gt_area, const uint8_t* gt_crowd, int g,
                               int labels_i64, int n_labels, int image_id, const double* thresholds, int n_thr, const double* areas,
                               int32_t* rec_image, int32_t* rec_label, float* rec_score, int32_t* rec_rank, uint64_t* rec_match,
                               uint64_t* rec_ignore, int32_t* det_offset, int capacity, int32_t* gt_image, int32_t* gt_label,
                               uint8_t* gt_ignore, int32_t* gt_offset, int gt_capacity, edtr_stream_t stream) {
    static_assert(kMaxDet == EDTR_COCO_MAX_DET && kMaxGt == EDTR_COCO_MAX_GT && kMaxLabels == EDTR_COCO_MAX_LABELS &&
                      kMaxThr == EDTR_COCO_MAX_THRESHOLDS && kKeep == EDTR_COCO_KEEP,
                  "edtr_hip.h and coco.hip disagree on a cap");
    static_assert(kMaxDet <= 65536 && kMaxGt <= 65536 && 4 * kMaxThr <= 64, "16-bit indices in LDS, one lane per (threshold, area range)");
    if (!thresholds || !areas || !rec_image || !rec_label || !rec_score || !rec_rank || !rec_match || !rec_ignore || !det_offset ||
        !gt_image || !gt_label || !gt_ignore || !gt_offset)
        return EDTR_E_NULL;
    if (n > 0 && (!det_boxes || !det_scores || !det_labels)) return EDTR_E_NULL;
    if (g > 0 && (!gt_boxes || !gt_labels || !gt_area || !gt_crowd)) return EDTR_E_NULL;
    if (n < 0 || g < 0 || n_labels <= 0 || n_thr <= 0 || capacity <= 0 || gt_capacity <= 0) return EDTR_E_SHAPE;
    if (n > kMaxDet || g > kMaxGt || n_labels > kMaxLabels || n_thr > kMaxThr || capacity > kMaxRows || gt_capacity > kMaxRows)
        return EDTR_E_UNSUPPORTED;
    if (labels_i64 != 0 && labels_i64 != 1) return EDTR_E_DTYPE;
    const uintptr_t la = labels_i64 ? 8 : 4;
    if (!aligned_to(det_boxes, 16) || !aligned_to(gt_boxes, 16) || !aligned_to(det_labels, la) || !aligned_to(gt_labels, la) ||
        !all_aligned_to(8, thresholds, areas) || !all_aligned_to(8, rec_match, rec_ignore) ||
        !all_aligned_to(4, det_scores, gt_area) || !all_aligned_to(4, count, rec_image, rec_label, rec_rank, det_offset, gt_image, gt_label, gt_offset) ||
        !aligned_to(rec_score, 4))
        return EDTR_E_ALIGN;
    if (n == 0 && g == 0) return EDTR_OK;       // an image with neither appends nothing
    MatchArgs a;
    a.det_boxes = det_boxes, a.det_scores = det_scores, a.det_labels = det_labels, a.count = count;
    a.gt_boxes = gt_boxes, a.gt_labels = gt_labels, a.gt_area = gt_area, a.gt_crowd = gt_crowd;
    a.thresholds = thresholds, a.areas = areas;
    a.n = n, a.g = g, a.labels_i64 = labels_i64, a.n_labels = n_labels, a.n_thr = n_thr, a.image_id = image_id;
    a.capacity = capacity, a.gt_capacity = gt_capacity;
    a.rec_image = rec_image, a.rec_label = rec_label, a.rec_score = rec_score, a.rec_rank = rec_rank;
    a.rec_match = rec_match, a.rec_ignore = rec_ignore;
    a.gt_image = gt_image, a.gt_label = gt_label, a.gt_ignore = gt_ignore;
    a.det_offset = det_offset, a.gt_offset = gt_offset;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)n_labels + 1u), dim3(64), 0, st, a);
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(coco_advance_kernel, dim3(1), dim3(64), 0, st, count, n, g, det_offset, gt_offset);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
