// Region proposals and RoI pooling on the device (edtr_hip.h "Region proposals and RoI pooling"; the host restatements and the rules
// themselves are edtr_amd/rois.py): the anchors of AnchorGenerator, the RPN's proposal filter up to its NMS — the per-level top-k as a
// radix select, an ordered compaction and a counting rank; then anchor, decoding, sigmoid, clip, the two filters and a second ordered
// compaction — and MultiScaleRoIAlign as one launch over every roi and level.
// The head's outputs are read where the head wrote them ([N][A][H][W] and [N][4 A][H][W]); no permuted copy and no anchor tensor is
// made on the proposal path.  Every output word has one writer, no launch waits on another workgroup, nothing uses a global or a
// floating-point atomic (the select's histogram is integer adds in LDS, whose result does not depend on their order), and every
// product, sum and quotient that decides a result bit is a correctly rounded fp32 operation in a stated order.
#include "common.h"
#include "glue.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxLevels = 8;           // EDTR_RPN_MAX_LEVELS
constexpr int kMaxPre = 4096;           // EDTR_RPN_MAX_PRE_NMS
constexpr int kMaxTaps = 64;            // EDTR_ROI_MAX_TAPS: output_size * sampling_ratio
constexpr int kLimit = 1 << 24;
constexpr int kSelectLanes = 1024;
constexpr int kSelectPeel = 4;          // bins of a wave that the select's histogram adds once per wave
constexpr int kSelectDepth = 8;         // loads a lane of the select has in flight: one workgroup walks a whole level, and latency is its cost
constexpr int kRoiChunk = 64;           // channels of one roi that a workgroup pools

template <int DT>
__device__ __forceinline__ float widen(const void* base, int64_t i) {
    if (DT == EDTR_LOGITS_F32) return static_cast<const float*>(base)[i];
    const uint16_t r = static_cast<const uint16_t*>(base)[i];
    return DT == EDTR_LOGITS_F16 ? F16::to_f32(r) : BF16::to_f32(r);
}

// One entry per feature level, by value in the kernel arguments.  n of a level = H W A; take = min(pre_nms_top_n, n).
struct RpnLevels {
    int n;
    int H[kMaxLevels], W[kMaxLevels], A[kMaxLevels], stride_h[kMaxLevels], stride_w[kMaxLevels];
    int take[kMaxLevels], sel_start[kMaxLevels], cell_start[kMaxLevels];
    int64_t anchor_start[kMaxLevels + 1];
    const void* obj[kMaxLevels];
    const void* deltas[kMaxLevels];
};

// anchor a of cell (y, x): float(x stride_w) + cell[a][0], float(y stride_h) + cell[a][1], and columns 2 and 3 alike (the shift is an
// integer below 2^24, so its conversion is exact and each value is one rounded sum)
__device__ __forceinline__ f32x4 anchor_of(f32x4 cell, int x, int y, int stride_w, int stride_h) {
    const float sx = (float)(x * stride_w), sy = (float)(y * stride_h);
    f32x4 o;
    o.x = add_rn(sx, cell.x), o.y = add_rn(sy, cell.y), o.z = add_rn(sx, cell.z), o.w = add_rn(sy, cell.w);
    return o;
}

__global__ void __launch_bounds__(256) rpn_anchors_kernel(RpnLevels t, const float* cells, float* anchors) {
    const int64_t total = t.anchor_start[t.n];
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        int l = 0;
        while (l + 1 < t.n && g >= t.anchor_start[l + 1]) ++l;
        const int i = (int)(g - t.anchor_start[l]);
        const int a = i % t.A[l], p = i / t.A[l], y = p / t.W[l], x = p - y * t.W[l];
        const f32x4 cell = *reinterpret_cast<const f32x4*>(cells + 4 * (int64_t)(t.cell_start[l] + a));
        *reinterpret_cast<f32x4*>(anchors + 4 * g) = anchor_of(cell, x, y, t.stride_w[l], t.stride_h[l]);
    }
}

// Workgroup (l, img) of 1024 lanes: the k = take[l] elements of level l of image img with the greatest key, equal keys by the smaller
// LOGICAL index i = (y W + x) A + a, written to selected[img][sel_start[l] ..] in that order.
//   select   four passes over the level in memory order (coalesced; a histogram does not care about order), 8 key bits each from the
//            top: a 256-bin histogram in LDS of the elements that match the prefix found so far, then the bin in which the k-th
//            greatest lies.  After the last pass the prefix is the threshold key T and `need` is
//            the number of elements with key == T to take.
//   compact  one pass in logical order (lane -> i, so a varies fastest: A runs of consecutive addresses per wave): every key > T and
//            the first `need` keys == T, by two ordered ballots per round, land in LDS in logical order.
//            Both walks fetch kSelectDepth rounds of keys before they use the first.
//   rank     place of selected e = #{key_j > key_e} + #{j < e : key_j == key_e} over the k selected: every read a broadcast.
template <int DT>
__global__ void __launch_bounds__(kSelectLanes) rpn_select_kernel(RpnLevels t, int total_take, int32_t* selected) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t found[2];
    __shared__ int wave_gt[kSelectLanes / 64], wave_eq[kSelectLanes / 64];
    __shared__ uint32_t sel_key[kMaxPre];
    __shared__ int32_t sel_idx[kMaxPre];
    const int l = (int)blockIdx.x, img = (int)blockIdx.y, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int A = t.A[l], HW = t.H[l] * t.W[l], n = HW * A, k = t.take[l];
    const void* obj = t.obj[l];
    const int64_t base = (int64_t)img * n;

    uint32_t prefix = 0u, himask = 0u;
    int need = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int m0 = 0; m0 < n; m0 += kSelectLanes * kSelectDepth) {
            uint32_t keys[kSelectDepth];
#pragma unroll
            for (int u = 0; u < kSelectDepth; ++u) {
                const int m = m0 + u * kSelectLanes + tid;
                keys[u] = m < n ? score_key(widen<DT>(obj, base + m)) : 0u;
            }
#pragma unroll
            for (int u = 0; u < kSelectDepth; ++u) {
                const uint32_t key = keys[u];
                const bool act = m0 + u * kSelectLanes + tid < n && (key & himask) == prefix;
                const uint32_t bin = (key >> shift) & 255u;
                // up to kSelectPeel bins of the wave are added once each, by one lane with the number of lanes that hold it; scores
                // of one sign and binade share their top bits, and 64 adds to one word would pass through the LDS one by one
                uint64_t rest = __ballot(act);
#pragma unroll
                for (int r = 0; r < kSelectPeel; ++r) {
                    if (!rest) break;
                    const int leader = __builtin_ctzll(rest);
                    const uint32_t b = __builtin_amdgcn_readlane(bin, leader);
                    const uint64_t same = __ballot(act && bin == b);
                    if (lane == leader) atomicAdd(&hist[b], (uint32_t)__popcll(same));
                    rest &= ~same;
                }
                if ((rest >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            // (the elements that match the prefix number at least `need`, so the walk ends at bin 0 at the latest)
            uint32_t above = 0u;
            int b = 255;
            for (; b > 0; --b) {
                if (above + hist[b] >= (uint32_t)need) break;
                above += hist[b];
            }
            found[0] = prefix | ((uint32_t)b << shift);
            found[1] = (uint32_t)need - above;
        }
        __syncthreads();
        prefix = found[0], need = (int)found[1], himask |= 0xffu << shift;
        __syncthreads();                        // found and hist are written again
    }

    const uint32_t T = prefix;
    int base_gt = 0, base_eq = 0;
    bool done = false;
    for (int i0 = 0; i0 < n && !done; i0 += kSelectLanes * kSelectDepth) {
        uint32_t keys[kSelectDepth];
#pragma unroll
        for (int u = 0; u < kSelectDepth; ++u) {
            const int i = i0 + u * kSelectLanes + tid;
            keys[u] = 0u;
            if (i < n) {
                const int p = i / A, a = i - p * A;
                keys[u] = score_key(widen<DT>(obj, base + (int64_t)a * HW + p));
            }
        }
#pragma unroll
        for (int u = 0; u < kSelectDepth; ++u) {
            if (done) continue;                 // uniform: everything to take has been seen
            const int i = i0 + u * kSelectLanes + tid;
            const uint32_t key = keys[u];
            const bool gt = i < n && key > T, eq = i < n && key == T;
            const uint64_t vg = __ballot(gt), ve = __ballot(eq);
            __syncthreads();                    // the sums of the round before have been read
            if (lane == 0) wave_gt[wave] = __popcll(vg), wave_eq[wave] = __popcll(ve);
            __syncthreads();
            int pg = base_gt + __popcll(vg & lanes_below(lane)), pe = base_eq + __popcll(ve & lanes_below(lane));
            for (int w = 0; w < kSelectLanes / 64; ++w) {
                const int g = wave_gt[w], e = wave_eq[w];
                pg += w < wave ? g : 0, pe += w < wave ? e : 0;
                base_gt += g, base_eq += e;
            }
            const int pos = pg + (pe < need ? pe : need);
            if ((gt || (eq && pe < need)) && pos < kMaxPre) sel_key[pos] = key, sel_idx[pos] = i;
            done = base_gt + (base_eq < need ? base_eq : need) >= k;
        }
    }
    __syncthreads();

    int32_t* out = selected + (int64_t)img * total_take + t.sel_start[l];
    for (int e = tid; e < k; e += kSelectLanes) {
        const uint32_t ke = sel_key[e];
        int rank = 0;
        for (int j = 0; j < k; ++j) {
            const uint32_t kj = sel_key[j];
            rank += (kj > ke || (kj == ke && j < e)) ? 1 : 0;
        }
        if (rank < k) out[rank] = sel_idx[e];
    }
}

struct RpnCandArgs {
    const int32_t* selected;    // [N][total_take]
    const float* cells;         // [sum A][4]
    const float* image_sizes;   // [N][2]: h, w
    float xform_clip, min_size, score_thresh;
    float* boxes;               // [N][total_take][4]
    float* probs;               // [N][total_take]
    int32_t* level;             // [N][total_take]
    int32_t* counts;            // [N]
    int total_take;
};

__device__ __forceinline__ float clip_to(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

// One workgroup per image walks the selected elements in level order and then selection order, 256 per round: anchor from the index,
// decode_box with weights 1, sigmoid, the clip to that image, width >= min_size && height >= min_size && prob >= score_thresh, and an
// ordered compaction by ballot; counts[img] = the number written.
template <int DT>
__global__ void __launch_bounds__(256) rpn_candidates_kernel(RpnLevels tv, RpnCandArgs a) {
    __shared__ RpnLevels t;
    __shared__ int wsum[4];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, img = (int)blockIdx.x;
    if (tid == 0) t = tv;
    __syncthreads();
    const float img_h = a.image_sizes[2 * img], img_w = a.image_sizes[2 * img + 1];
    const int M = a.total_take;
    const int64_t row = (int64_t)img * M;
    int base = 0;
    for (int e0 = 0; e0 < M; e0 += 256) {
        const int e = e0 + tid;
        bool flag = false;
        f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
        float prob = 0.0f;
        int l = 0;
        if (e < M) {
            while (l + 1 < t.n && e >= t.sel_start[l + 1]) ++l;
            const int A = t.A[l], W = t.W[l], HW = t.H[l] * W;
            const int idx = clamp_index(a.selected[row + e], HW * A);
            const int p = idx / A, ai = idx - p * A, y = p / W, x = p - y * W;
            const f32x4 cell = *reinterpret_cast<const f32x4*>(a.cells + 4 * (int64_t)(t.cell_start[l] + ai));
            const f32x4 anchor = anchor_of(cell, x, y, t.stride_w[l], t.stride_h[l]);
            const int64_t d0 = ((int64_t)img * 4 * A + 4 * ai) * HW + p;
            f32x4 r;
            r.x = widen<DT>(t.deltas[l], d0), r.y = widen<DT>(t.deltas[l], d0 + HW);
            r.z = widen<DT>(t.deltas[l], d0 + 2 * (int64_t)HW), r.w = widen<DT>(t.deltas[l], d0 + 3 * (int64_t)HW);
            const float logit = widen<DT>(t.obj[l], ((int64_t)img * A + ai) * HW + p);
            const f32x4 d = decode_box(anchor, r, 1.0f, 1.0f, 1.0f, 1.0f, a.xform_clip);
            prob = div_rn(1.0f, add_rn(1.0f, expf(-logit)));
            o.x = clip_to(d.x, img_w), o.y = clip_to(d.y, img_h), o.z = clip_to(d.z, img_w), o.w = clip_to(d.w, img_h);
            flag = add_rn(o.z, -o.x) >= a.min_size && add_rn(o.w, -o.y) >= a.min_size && prob >= a.score_thresh;
        }
        const uint64_t vote = __ballot(flag);
        __syncthreads();                        // the sums of the round before have been read
        if (lane == 0) wsum[wave] = __popcll(vote);
        __syncthreads();
        int pos = base + __popcll(vote & lanes_below(lane));
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        if (flag && pos < M) {
            *reinterpret_cast<f32x4*>(a.boxes + 4 * (row + pos)) = o;
            a.probs[row + pos] = prob;
            a.level[row + pos] = l;
        }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
    if (tid == 0) a.counts[img] = base < M ? base : M;
}

// ---- MultiScaleRoIAlign ------------------------------------------------------------------------------------------------------------

struct RoiLevels {
    int n, k_min, k_max;
    int H[kMaxLevels], W[kMaxLevels];
    float scale[kMaxLevels];
    const void* feat[kMaxLevels];
};

struct RoiArgs {
    const float* rois;          // [K][4]
    const int32_t* batch;       // [K]: the image of each roi
    float* out;                 // [K][C][P][P]
    int N, C, P, S;
    float canonical_scale, canonical_level;
};

// LevelMapper: the level of a roi, the ONE expression the forward and the backward's pre-pass both evaluate
__device__ __forceinline__ int roi_level(const RoiLevels& t, f32x4 box, float canonical_scale, float canonical_level) {
    if (t.n <= 1) return 0;
    const float s = sqrtf(mul_rn(add_rn(box.z, -box.x), add_rn(box.w, -box.y)));
    const float k = floorf(add_rn(add_rn(canonical_level, log2f(div_rn(s, canonical_scale))), 1e-6f));
    const float lo = (float)t.k_min, hi = (float)t.k_max;
    const int l = (int)(!(k >= lo) ? lo : (k > hi ? hi : k)) - t.k_min;   // (NaN and -inf: the finest level)
    return clamp_index(l, t.n);
}

// One tap position of one axis: start + ph bin and the offset of sample i inside the bin, then roi_align's bilinear_interpolate for
// that axis.  low < 0 marks a sample outside [-1, extent], which adds nothing (a NaN coordinate is outside).
__device__ __forceinline__ void roi_tap(float start, float bin, int ph, int i, int S, int extent, int& low, int& high, float& l, float& h) {
    float v = add_rn(add_rn(start, mul_rn((float)ph, bin)), div_rn(mul_rn(add_rn((float)i, 0.5f), bin), (float)S));
    if (!(v >= -1.0f && v <= (float)extent)) {
        low = high = -1, l = h = 0.0f;
        return;
    }
    v = v <= 0.0f ? 0.0f : v;
    low = (int)v;
    if (low >= extent - 1) {
        low = high = extent - 1;
        v = (float)low;
    } else {
        high = low + 1;
    }
    l = add_rn(v, -(float)low), h = add_rn(1.0f, -l);
}

// Workgroup (roi, chunk of 64 channels).  The level and the P S tap positions of each axis are the roi's alone: lanes 0 .. P S - 1
// work out the rows' and lanes 64 .. 64 + P S - 1 the columns' into LDS once.  Then lane -> output element (c, ph, pw) in the order
// the output is stored, so a wave stores 256 consecutive bytes and its taps fall into the same few rows of one or two planes.
template <int DT>
__global__ void __launch_bounds__(256) roi_align_kernel(RoiLevels t, RoiArgs a) {
    __shared__ int ylo[kMaxTaps], yhi[kMaxTaps], xlo[kMaxTaps], xhi[kMaxTaps];
    __shared__ float ly[kMaxTaps], hy[kMaxTaps], lx[kMaxTaps], hx[kMaxTaps];
    const int tid = (int)threadIdx.x, P = a.P, S = a.S, PS = P * S, PP = P * P;
    const int64_t roi = blockIdx.x;
    const f32x4 box = *reinterpret_cast<const f32x4*>(a.rois + 4 * roi);
    const int l = roi_level(t, box, a.canonical_scale, a.canonical_level);
    const int H = t.H[l], W = t.W[l];
    const float scale = t.scale[l];
    if (tid < PS) {
        const float y1 = mul_rn(box.y, scale), y2 = mul_rn(box.w, scale);
        const float ext = add_rn(y2, -y1), roi_h = ext < 1.0f ? 1.0f : ext;
        roi_tap(y1, div_rn(roi_h, (float)P), tid / S, tid % S, S, H, ylo[tid], yhi[tid], ly[tid], hy[tid]);
    } else if (tid >= 64 && tid < 64 + PS) {
        const int i = tid - 64;
        const float x1 = mul_rn(box.x, scale), x2 = mul_rn(box.z, scale);
        const float ext = add_rn(x2, -x1), roi_w = ext < 1.0f ? 1.0f : ext;
        roi_tap(x1, div_rn(roi_w, (float)P), i / S, i % S, S, W, xlo[i], xhi[i], lx[i], hx[i]);
    }
    __syncthreads();
    const int c0 = (int)blockIdx.y * kRoiChunk, cn = a.C - c0 < kRoiChunk ? a.C - c0 : kRoiChunk;
    const int b = clamp_index(a.batch[roi], a.N);
    const void* feat = t.feat[l];
    const int64_t plane0 = (int64_t)b * a.C + c0, HW = (int64_t)H * W;
    const float count = (float)(S * S);
    for (int e = tid; e < cn * PP; e += 256) {
        const int c = e / PP, r = e - c * PP, ph = r / P, pw = r - ph * P;
        const int64_t plane = (plane0 + c) * HW;
        float sum = 0.0f;
        for (int iy = 0; iy < S; ++iy) {
            const int yi = ph * S + iy, y0 = ylo[yi], y1 = yhi[yi];
            if (y0 < 0) continue;
            const float wly = ly[yi], why = hy[yi];
            for (int ix = 0; ix < S; ++ix) {
                const int xi = pw * S + ix, x0 = xlo[xi], x1 = xhi[xi];
                if (x0 < 0) continue;
                const float wlx = lx[xi], whx = hx[xi];
                const float v11 = widen<DT>(feat, plane + (int64_t)y0 * W + x0), v12 = widen<DT>(feat, plane + (int64_t)y0 * W + x1);
                const float v21 = widen<DT>(feat, plane + (int64_t)y1 * W + x0), v22 = widen<DT>(feat, plane + (int64_t)y1 * W + x1);
                const float val = add_rn(add_rn(add_rn(mul_rn(mul_rn(why, whx), v11), mul_rn(mul_rn(why, wlx), v12)),
                                                mul_rn(mul_rn(wly, whx), v21)), mul_rn(mul_rn(wly, wlx), v22));
                sum = add_rn(sum, val);
            }
        }
        a.out[(roi * a.C + c0 + c) * PP + r] = div_rn(sum, count);
    }
}

// ---- RoIAlign's backward -----------------------------------------------------------------------------------------------------------
// The gradient is GATHERED: a workgroup owns a 16 x 16 tile of one level of one image and kBwdChunk channels, and adds to it the
// contribution of every roi that reaches it in k order; no word has two writers and no sum depends on timing.

constexpr int kBwdMaxP = 16;            // EDTR_ROI_BWD_MAX_P
constexpr int kBwdChunk = 32;           // EDTR_ROI_BWD_CHUNK: channels whose sums a lane holds in registers
constexpr int kBwdStride = kBwdChunk + 4;   // floats between two bins of the staged g': 16-byte aligned rows; a staging wave writes 8 banks
constexpr int kRecHead = 8;             // words of a record before its taps: level, image, ymin, ymax, xmin, xmax, 0, 0

struct RoiBwdArgs {
    const float* rois;          // [K][4]
    const int32_t* batch;       // [K], not decreasing
    const float* grad;          // [K][C][P][P]
    int32_t* ws;                // image_start [N + 1] (padded to 4 words), then K records of kRecHead + 8 P S words
    void* out[kMaxLevels];      // [N][C][H_l][W_l]
    int64_t tile_start[kMaxLevels + 1];
    int tiles_x[kMaxLevels];
    int N, C, K, P, S, rec0;
    float canonical_scale, canonical_level;
};

inline int64_t bwd_image_words(int N) { return ((int64_t)N + 1 + 3) / 4 * 4; }
inline int64_t bwd_record_words(int P, int S) { return kRecHead + 8 * (int64_t)P * S; }

// Workgroup k of 128 lanes: lanes 0 .. P S - 1 the rows' taps and lanes 64 .. 64 + P S - 1 the columns', as the forward works them
// out; lane 0 then the footprint of the valid ones and image_start[n] = the first roi of image n (for the n that begin at k).
__global__ void __launch_bounds__(128) roi_backward_records_kernel(RoiLevels t, RoiBwdArgs a) {
    __shared__ int lo[2][kMaxTaps], hi[2][kMaxTaps];
    const int tid = (int)threadIdx.x, P = a.P, S = a.S, PS = P * S, k = (int)blockIdx.x;
    const f32x4 box = *reinterpret_cast<const f32x4*>(a.rois + 4 * (int64_t)k);
    const int l = roi_level(t, box, a.canonical_scale, a.canonical_level);
    int32_t* rec = a.ws + a.rec0 + (int64_t)k * (kRecHead + 8 * PS);
    const int axis = tid >> 6, i = tid & 63;            // axis 0: rows (y), axis 1: columns (x)
    if (i < PS) {
        const float scale = t.scale[l];
        const float p1 = mul_rn(axis ? box.x : box.y, scale), p2 = mul_rn(axis ? box.z : box.w, scale);
        const float ext = add_rn(p2, -p1), size = ext < 1.0f ? 1.0f : ext;
        int low, high;
        float wl, wh;
        roi_tap(p1, div_rn(size, (float)P), i / S, i % S, S, axis ? t.W[l] : t.H[l], low, high, wl, wh);
        lo[axis][i] = low, hi[axis][i] = high;
        int4 w;
        w.x = low, w.y = high, w.z = __float_as_int(wl), w.w = __float_as_int(wh);
        *reinterpret_cast<int4*>(rec + kRecHead + 4 * (axis * PS + i)) = w;
    }
    __syncthreads();
    if (tid == 0) {
        int ymin = kLimit, ymax = -1, xmin = kLimit, xmax = -1;
        for (int j = 0; j < PS; ++j) {
            if (lo[0][j] >= 0) ymin = lo[0][j] < ymin ? lo[0][j] : ymin, ymax = hi[0][j] > ymax ? hi[0][j] : ymax;
            if (lo[1][j] >= 0) xmin = lo[1][j] < xmin ? lo[1][j] : xmin, xmax = hi[1][j] > xmax ? hi[1][j] : xmax;
        }
        if (ymax < 0 || xmax < 0) ymin = xmin = 1, ymax = xmax = 0;     // no valid sample: the empty footprint
        const int b = clamp_index(a.batch[k], a.N);
        int4 h0, h1;
        h0.x = l, h0.y = b, h0.z = ymin, h0.w = ymax, h1.x = xmin, h1.y = xmax, h1.z = h1.w = 0;
        *reinterpret_cast<int4*>(rec) = h0, *reinterpret_cast<int4*>(rec + 4) = h1;
        const int prev = k > 0 ? clamp_index(a.batch[k - 1], a.N) : -1;
        for (int n = prev + 1; n <= b; ++n) a.ws[n] = k;
        if (k == a.K - 1)
            for (int n = b + 1; n <= a.N; ++n) a.ws[n] = a.K;
    }
}

template <int DT>
__device__ __forceinline__ void store_rounded(void* base, int64_t i, float v) {
    if (DT == EDTR_LOGITS_F32) static_cast<float*>(base)[i] = v;
    else static_cast<uint16_t*>(base)[i] = DT == EDTR_LOGITS_F16 ? F16::from_f32(v) : BF16::from_f32(v);
}

// Workgroup (tile of a level, chunk of channels, image) of 256 lanes, lane -> pixel (ty, tx) = (tid / 16, tid % 16) of the tile.
//   keep     the image's rois 256 per round: those of this level whose footprint meets the tile, by an ordered ballot compaction, so
//            `kept` holds them k ascending;
//   weights  per kept roi a[ph] of the tile's 16 rows and b[pw] of its 16 columns, one lane each, into LDS: a wave (4 rows) reads 4
//            consecutive words of `wa` and 16 of `wb`, each a broadcast within its lanes;
//   stage    g' = grad / (S S) of the chunk as gs[bin][channel]: the gather reads the 32 channels of a bin as eight 16-byte words at
//            ONE address for the whole wave (a broadcast, no bank conflict);
//   gather   t[c] over pw, contrib[c] over ph, acc[c] += contrib[c]: 3 x 32 sums in registers.  A zero weight skips its term: the
//            pixels of a tile that a roi does not reach cost a compare.
// The tile's 16 x 16 x chunk results are stored once at the end, per channel four 64-byte (fp32) row segments per wave.
template <int DT>
__global__ void __launch_bounds__(256) roi_backward_gather_kernel(RoiLevels t, RoiBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float gs[kBwdMaxP * kBwdMaxP * kBwdStride];
    __shared__ float wa[kBwdMaxP][16], wb[kBwdMaxP][16];
    __shared__ int kept[256];
    __shared__ int wsum[4];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, ty = tid >> 4, tx = tid & 15;
    const int P = a.P, S = a.S, PS = P * S, PP = P * P;
    int l = 0;
    while (l + 1 < t.n && (int64_t)blockIdx.x >= a.tile_start[l + 1]) ++l;
    const int tile = (int)((int64_t)blockIdx.x - a.tile_start[l]), tile_y = tile / a.tiles_x[l], tile_x = tile - tile_y * a.tiles_x[l];
    const int H = t.H[l], W = t.W[l], y0 = tile_y * 16, x0 = tile_x * 16;
    const int n = (int)blockIdx.z, c0 = (int)blockIdx.y * kBwdChunk, cn = a.C - c0 < kBwdChunk ? a.C - c0 : kBwdChunk;
    int kb = a.ws[n], ke = a.ws[n + 1];
    kb = kb < 0 ? 0 : (kb > a.K ? a.K : kb), ke = ke < kb ? kb : (ke > a.K ? a.K : ke);
    const int rec_words = kRecHead + 8 * PS;
    const int32_t* recs = a.ws + a.rec0;
    const float count = (float)(S * S);

    float acc[kBwdChunk];
#pragma unroll
    for (int c = 0; c < kBwdChunk; ++c) acc[c] = 0.0f;

    for (int k0 = kb; k0 < ke; k0 += 256) {
        const int k = k0 + tid;
        bool flag = false;
        if (k < ke) {
            const int32_t* rec = recs + (int64_t)k * rec_words;
            const int4 h0 = *reinterpret_cast<const int4*>(rec), h1 = *reinterpret_cast<const int4*>(rec + 4);
            flag = h0.x == l && h0.y == n && h0.z <= y0 + 15 && h0.w >= y0 && h1.x <= x0 + 15 && h1.y >= x0;
        }
        const uint64_t vote = __ballot(flag);
        __syncthreads();                        // the list and the sums of the round before have been read
        if (lane == 0) wsum[wave] = __popcll(vote);
        __syncthreads();
        int pos = __popcll(vote & lanes_below(lane));
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        if (flag) kept[pos] = k;
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        for (int j = 0; j < total; ++j) {
            __syncthreads();                    // the list is written; gs, wa and wb of the roi before have been read
            const int kk = kept[j];
            const int32_t* rec = recs + (int64_t)kk * rec_words;
            if (tid < 16 * P) {
                const int ph = tid >> 4, r = tid & 15;
                float wy = 0.0f, wx = 0.0f;
                for (int i = 0; i < S; ++i) {
                    const int4 yt = *reinterpret_cast<const int4*>(rec + kRecHead + 4 * (ph * S + i));
                    const int4 xt = *reinterpret_cast<const int4*>(rec + kRecHead + 4 * (PS + ph * S + i));
                    if (yt.x >= 0) {
                        if (yt.x == y0 + r) wy = add_rn(wy, __int_as_float(yt.w));
                        if (yt.y == y0 + r) wy = add_rn(wy, __int_as_float(yt.z));
                    }
                    if (xt.x >= 0) {
                        if (xt.x == x0 + r) wx = add_rn(wx, __int_as_float(xt.w));
                        if (xt.y == x0 + r) wx = add_rn(wx, __int_as_float(xt.z));
                    }
                }
                wa[ph][r] = wy, wb[ph][r] = wx;
            }
            const float* g = a.grad + ((int64_t)kk * a.C + c0) * PP;
            for (int e = tid; e < kBwdChunk * PP; e += 256) {
                const int c = e / PP, r = e - c * PP;
                gs[r * kBwdStride + c] = c < cn ? div_rn(g[e], count) : 0.0f;
            }
            __syncthreads();
            float contrib[kBwdChunk];
#pragma unroll
            for (int c = 0; c < kBwdChunk; ++c) contrib[c] = 0.0f;
            for (int ph = 0; ph < P; ++ph) {
                const float wy = wa[ph][ty];
                if (wy == 0.0f) continue;
                float ts[kBwdChunk];
#pragma unroll
                for (int c = 0; c < kBwdChunk; ++c) ts[c] = 0.0f;
                for (int pw = 0; pw < P; ++pw) {
                    const float wx = wb[pw][tx];
                    if (wx == 0.0f) continue;
                    const f32x4* g4 = reinterpret_cast<const f32x4*>(gs + (ph * P + pw) * kBwdStride);
#pragma unroll
                    for (int q = 0; q < kBwdChunk / 4; ++q) {
                        const f32x4 v = g4[q];
                        ts[4 * q] = add_rn(ts[4 * q], mul_rn(wx, v.x)), ts[4 * q + 1] = add_rn(ts[4 * q + 1], mul_rn(wx, v.y));
                        ts[4 * q + 2] = add_rn(ts[4 * q + 2], mul_rn(wx, v.z)), ts[4 * q + 3] = add_rn(ts[4 * q + 3], mul_rn(wx, v.w));
                    }
                }
#pragma unroll
                for (int c = 0; c < kBwdChunk; ++c) contrib[c] = add_rn(contrib[c], mul_rn(wy, ts[c]));
            }
#pragma unroll
            for (int c = 0; c < kBwdChunk; ++c) acc[c] = add_rn(acc[c], contrib[c]);
        }
    }

    const int y = y0 + ty, x = x0 + tx;
    if (y < H && x < W) {
        const int64_t HW = (int64_t)H * W, base = ((int64_t)n * a.C + c0) * HW + (int64_t)y * W + x;
        void* out = a.out[l];
#pragma unroll
        for (int c = 0; c < kBwdChunk; ++c)
            if (c < cn) store_rounded<DT>(out, base + c * HW, acc[c]);
    }
}

inline bool known_dtype(int dt) { return dt == EDTR_LOGITS_F32 || dt == EDTR_LOGITS_F16 || dt == EDTR_LOGITS_BF16; }

// levels_host [L][5] = H, W, A, stride_h, stride_w -> the table; what every RPN entry point checks first, in this order
inline int rpn_table(const int32_t* levels_host, int L, int pre_nms_top_n, RpnLevels& t) {
    if (!levels_host) return EDTR_E_NULL;
    if (L <= 0 || pre_nms_top_n <= 0) return EDTR_E_SHAPE;
    if (L > kMaxLevels || pre_nms_top_n > kMaxPre) return EDTR_E_UNSUPPORTED;
    t.n = L;
    int sel = 0, cell = 0;
    int64_t anchor = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        const bool have = l < L;
        const int H = have ? levels_host[5 * l] : 1, W = have ? levels_host[5 * l + 1] : 1, A = have ? levels_host[5 * l + 2] : 1;
        const int sh = have ? levels_host[5 * l + 3] : 0, sw = have ? levels_host[5 * l + 4] : 0;
        if (H <= 0 || W <= 0 || A <= 0 || sh < 0 || sw < 0) return EDTR_E_SHAPE;
        const int64_t n = (int64_t)H * W * A;
        if (n >= kLimit || (int64_t)H * sh >= kLimit || (int64_t)W * sw >= kLimit) return EDTR_E_UNSUPPORTED;
        t.H[l] = H, t.W[l] = W, t.A[l] = A, t.stride_h[l] = sh, t.stride_w[l] = sw;
        t.take[l] = have ? (int)(n < pre_nms_top_n ? n : pre_nms_top_n) : 0;
        t.sel_start[l] = sel, t.cell_start[l] = cell, t.anchor_start[l] = anchor;
        t.obj[l] = t.deltas[l] = nullptr;
        if (have) sel += t.take[l], cell += A, anchor += n;
    }
    t.anchor_start[kMaxLevels] = anchor;
    return EDTR_OK;
}

inline int total_take(const RpnLevels& t) { return t.sel_start[t.n - 1] + t.take[t.n - 1]; }

}  // namespace

extern "C" int edtr_rpn_anchors(const int32_t* levels_host, int L, const float* cells, float* anchors, edtr_stream_t stream) {
    static_assert(kMaxLevels == EDTR_RPN_MAX_LEVELS && kMaxPre == EDTR_RPN_MAX_PRE_NMS && kMaxTaps == EDTR_ROI_MAX_TAPS,
                  "edtr_hip.h and rois.hip disagree on a cap");
    static_assert(kMaxLevels * kMaxPre == EDTR_NMS_MAX_BOXES, "the NMS must take every level's selection");
    RpnLevels t;
    const int rc = rpn_table(levels_host, L, 1, t);
    if (rc != EDTR_OK) return rc;
    if (!cells || !anchors) return EDTR_E_NULL;
    if (!all_aligned_to(16, cells, anchors)) return EDTR_E_ALIGN;
    hipLaunchKernelGGL(rpn_anchors_kernel, dim3(blocks_for(t.anchor_start[L])), dim3(256), 0, static_cast<hipStream_t>(stream), t, cells, anchors);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_rpn_select(int dtype, const void* const* objectness_host, const int32_t* levels_host, int L, int N, int pre_nms_top_n,
                               int32_t* selected, edtr_stream_t stream) {
    RpnLevels t;
    const int rc = rpn_table(levels_host, L, pre_nms_top_n, t);
    if (rc != EDTR_OK) return rc;
    if (!objectness_host || !selected) return EDTR_E_NULL;
    if (N <= 0) return EDTR_E_SHAPE;
    if (N > 65535) return EDTR_E_UNSUPPORTED;
    if (!known_dtype(dtype)) return EDTR_E_DTYPE;
    for (int l = 0; l < L; ++l) {
        if (!objectness_host[l]) return EDTR_E_NULL;
        if (!aligned_to(objectness_host[l], dtype == EDTR_LOGITS_F32 ? 4 : 2)) return EDTR_E_ALIGN;
        t.obj[l] = objectness_host[l];
    }
    if (!aligned_to(selected, 4)) return EDTR_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)L, (unsigned)N), block(kSelectLanes);
    const int total = total_take(t);
    if (dtype == EDTR_LOGITS_F32) hipLaunchKernelGGL(rpn_select_kernel<EDTR_LOGITS_F32>, grid, block, 0, st, t, total, selected);
    else if (dtype == EDTR_LOGITS_F16) hipLaunchKernelGGL(rpn_select_kernel<EDTR_LOGITS_F16>, grid, block, 0, st, t, total, selected);
    else hipLaunchKernelGGL(rpn_select_kernel<EDTR_LOGITS_BF16>, grid, block, 0, st, t, total, selected);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_rpn_candidates(int dtype, const void* const* objectness_host, const void* const* deltas_host, const int32_t* levels_host,
                                   int L, int N, int pre_nms_top_n, const float* cells, const int32_t* selected, const float* image_sizes,
                                   float xform_clip, float min_size, float score_thresh, float* boxes, float* probs, int32_t* level,
                                   int32_t* counts, edtr_stream_t stream) {
    RpnLevels t;
    const int rc = rpn_table(levels_host, L, pre_nms_top_n, t);
    if (rc != EDTR_OK) return rc;
    if (!objectness_host || !deltas_host || !cells || !selected || !image_sizes || !boxes || !probs || !level || !counts) return EDTR_E_NULL;
    if (N <= 0) return EDTR_E_SHAPE;
    if (N > 65535) return EDTR_E_UNSUPPORTED;
    if (!known_dtype(dtype)) return EDTR_E_DTYPE;
    const uintptr_t elem = dtype == EDTR_LOGITS_F32 ? 4 : 2;
    for (int l = 0; l < L; ++l) {
        if (!objectness_host[l] || !deltas_host[l]) return EDTR_E_NULL;
        if (!aligned_to(objectness_host[l], elem) || !aligned_to(deltas_host[l], elem)) return EDTR_E_ALIGN;
        t.obj[l] = objectness_host[l], t.deltas[l] = deltas_host[l];
    }
    if (!all_aligned_to(16, cells, boxes) || !all_aligned_to(4, selected, level, counts) || !all_aligned_to(4, image_sizes, probs)) return EDTR_E_ALIGN;
    RpnCandArgs a;
    a.selected = selected, a.cells = cells, a.image_sizes = image_sizes;
    a.xform_clip = xform_clip, a.min_size = min_size, a.score_thresh = score_thresh;
    a.boxes = boxes, a.probs = probs, a.level = level, a.counts = counts, a.total_take = total_take(t);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)N), block(256);
    if (dtype == EDTR_LOGITS_F32) hipLaunchKernelGGL(rpn_candidates_kernel<EDTR_LOGITS_F32>, grid, block, 0, st, t, a);
    else if (dtype == EDTR_LOGITS_F16) hipLaunchKernelGGL(rpn_candidates_kernel<EDTR_LOGITS_F16>, grid, block, 0, st, t, a);
    else hipLaunchKernelGGL(rpn_candidates_kernel<EDTR_LOGITS_BF16>, grid, block, 0, st, t, a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_roi_align(int dtype, const void* const* features_host, const int32_t* level_hw_host, const float* scales_host, int L,
                              int N, int C, const float* rois, const int32_t* batch_index, int K, int P, int S, int k_min, int k_max,
                              float canonical_scale, float canonical_level, float* out, edtr_stream_t stream) {
    if (!features_host || !level_hw_host || !scales_host || !rois || !batch_index || !out) return EDTR_E_NULL;
    if (L <= 0 || N <= 0 || C <= 0 || K <= 0 || P <= 0 || S <= 0 || k_max < k_min || !(canonical_scale > 0.0f)) return EDTR_E_SHAPE;
    if (L > kMaxLevels || N > 65535 || (int64_t)P * S > kMaxTaps || (C + kRoiChunk - 1) / kRoiChunk > 65535 || C >= kLimit) return EDTR_E_UNSUPPORTED;
    if (L > 1 && k_max - k_min != L - 1) return EDTR_E_SHAPE;
    if (!known_dtype(dtype)) return EDTR_E_DTYPE;
    RoiLevels t;
    t.n = L, t.k_min = k_min, t.k_max = k_max;
    for (int l = 0; l < kMaxLevels; ++l) {
        const bool have = l < L;
        t.H[l] = have ? level_hw_host[2 * l] : 1, t.W[l] = have ? level_hw_host[2 * l + 1] : 1;
        t.scale[l] = have ? scales_host[l] : 1.0f, t.feat[l] = have ? features_host[l] : nullptr;
        if (!have) continue;
        if (!t.feat[l]) return EDTR_E_NULL;
        if (t.H[l] <= 0 || t.W[l] <= 0 || !(t.scale[l] > 0.0f)) return EDTR_E_SHAPE;
        if (t.H[l] >= kLimit || t.W[l] >= kLimit) return EDTR_E_UNSUPPORTED;
        if (!aligned_to(t.feat[l], dtype == EDTR_LOGITS_F32 ? 4 : 2)) return EDTR_E_ALIGN;
    }
    if (!aligned_to(rois, 16) || !aligned_to(batch_index, 4) || !aligned_to(out, 4)) return EDTR_E_ALIGN;
    RoiArgs a;
    a.rois = rois, a.batch = batch_index, a.out = out, a.N = N, a.C = C, a.P = P, a.S = S;
    a.canonical_scale = canonical_scale, a.canonical_level = canonical_level;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)K, (unsigned)((C + kRoiChunk - 1) / kRoiChunk)), block(256);
    if (dtype == EDTR_LOGITS_F32) hipLaunchKernelGGL(roi_align_kernel<EDTR_LOGITS_F32>, grid, block, 0, st, t, a);
    else if (dtype == EDTR_LOGITS_F16) hipLaunchKernelGGL(roi_align_kernel<EDTR_LOGITS_F16>, grid, block, 0, st, t, a);
    else hipLaunchKernelGGL(roi_align_kernel<EDTR_LOGITS_BF16>, grid, block, 0, st, t, a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int64_t edtr_roi_align_backward_workspace(int N, int K, int P, int S) {
    if (N <= 0 || K <= 0 || P <= 0 || S <= 0 || (int64_t)P * S > kMaxTaps) return 0;
    return 4 * (bwd_image_words(N) + (int64_t)K * bwd_record_words(P, S));
}

extern "C" int edtr_roi_align_backward(int dtype, void* const* grads_out_host, const int32_t* level_hw_host, const float* scales_host, int L,
                                       int N, int C, const float* rois, const int32_t* batch_index, int K, int P, int S, int k_min, int k_max,
                                       float canonical_scale, float canonical_level, const float* grad, void* workspace,
                                       int64_t workspace_bytes, edtr_stream_t stream) {
    static_assert(kBwdMaxP == EDTR_ROI_BWD_MAX_P && kBwdChunk == EDTR_ROI_BWD_CHUNK, "edtr_hip.h and rois.hip disagree on a cap");
    static_assert(kBwdMaxP * 16 <= 256 && kBwdChunk % 4 == 0, "one lane per (bin, row) of a tile; the staged channels are read four at a time");
    if (!grads_out_host || !level_hw_host || !scales_host || !rois || !batch_index || !grad || !workspace) return EDTR_E_NULL;
    if (L <= 0 || N <= 0 || C <= 0 || K <= 0 || P <= 0 || S <= 0 || k_max < k_min || !(canonical_scale > 0.0f)) return EDTR_E_SHAPE;
    if (L > kMaxLevels || N > 65535 || (int64_t)P * S > kMaxTaps || (C + kRoiChunk - 1) / kRoiChunk > 65535 || C >= kLimit) return EDTR_E_UNSUPPORTED;
    if (P > kBwdMaxP || (C + kBwdChunk - 1) / kBwdChunk > 65535) return EDTR_E_UNSUPPORTED;
    if (L > 1 && k_max - k_min != L - 1) return EDTR_E_SHAPE;
    if (!known_dtype(dtype)) return EDTR_E_DTYPE;
    RoiLevels t;
    RoiBwdArgs a;
    t.n = L, t.k_min = k_min, t.k_max = k_max;
    int64_t tiles = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        const bool have = l < L;
        t.H[l] = have ? level_hw_host[2 * l] : 1, t.W[l] = have ? level_hw_host[2 * l + 1] : 1;
        t.scale[l] = have ? scales_host[l] : 1.0f, t.feat[l] = nullptr;
        a.out[l] = have ? grads_out_host[l] : nullptr;
        a.tile_start[l] = tiles, a.tiles_x[l] = 1;
        if (!have) continue;
        if (!a.out[l]) return EDTR_E_NULL;
        if (t.H[l] <= 0 || t.W[l] <= 0 || !(t.scale[l] > 0.0f)) return EDTR_E_SHAPE;
        if (t.H[l] >= kLimit || t.W[l] >= kLimit) return EDTR_E_UNSUPPORTED;
        if (!aligned_to(a.out[l], dtype == EDTR_LOGITS_F32 ? 4 : 2)) return EDTR_E_ALIGN;
        a.tiles_x[l] = (t.W[l] + 15) / 16;
        tiles += (int64_t)a.tiles_x[l] * ((t.H[l] + 15) / 16);
        if (tiles >= ((int64_t)1 << 31)) return EDTR_E_UNSUPPORTED;
    }
    a.tile_start[kMaxLevels] = tiles;
    for (int l = L; l < kMaxLevels; ++l) a.tile_start[l] = tiles;
    if (!aligned_to(rois, 16) || !aligned_to(batch_index, 4) || !aligned_to(grad, 4) || !aligned_to(workspace, 16)) return EDTR_E_ALIGN;
    if (workspace_bytes < edtr_roi_align_backward_workspace(N, K, P, S)) return EDTR_E_SHAPE;
    a.rois = rois, a.batch = batch_index, a.grad = grad, a.ws = static_cast<int32_t*>(workspace);
    a.N = N, a.C = C, a.K = K, a.P = P, a.S = S, a.rec0 = (int)bwd_image_words(N);
    a.canonical_scale = canonical_scale, a.canonical_level = canonical_level;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(roi_backward_records_kernel, dim3((unsigned)K), dim3(128), 0, st, t, a);
    EDTR_LAUNCH_CHECK();
    const dim3 grid((unsigned)tiles, (unsigned)((C + kBwdChunk - 1) / kBwdChunk), (unsigned)N), block(256);
    if (dtype == EDTR_LOGITS_F32) hipLaunchKernelGGL(roi_backward_gather_kernel<EDTR_LOGITS_F32>, grid, block, 0, st, t, a);
    else if (dtype == EDTR_LOGITS_F16) hipLaunchKernelGGL(roi_backward_gather_kernel<EDTR_LOGITS_F16>, grid, block, 0, st, t, a);
    else hipLaunchKernelGGL(roi_backward_gather_kernel<EDTR_LOGITS_BF16>, grid, block, 0, st, t, a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
