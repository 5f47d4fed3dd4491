// Detector training targets on the device (edtr_hip.h "Detector training targets"; the host restatements and the rules themselves are
// edtr_amd/targets.py): Matcher over box_iou without the [G, P] matrix, BoxCoder.encode, and BalancedPositiveNegativeSampler on the
// seeded per-image Philox stream in place of torch.randperm.
//   match    two launches.  The scan keeps an image's ground truths in LDS, walks them for kTile boxes per workgroup, and writes each
//            box's best value and index and, per tile, the greatest IoU of every ground truth as an order-preserving 32-bit key.  The
//            assign pass folds those keys in LDS, applies the thresholds, recomputes the IoUs of a box below the high threshold with
//            the SAME device function (the same bits) to restore the low-quality matches, and writes labels and, for the RPN, the
//            regression target of every anchor.
//   sample   one 1024-lane workgroup per image: a radix select of the num_pos / num_neg smallest Philox words among the positives /
//            negatives (three passes of 11, 11 and 10 key bits, two histograms in LDS), then one pass in index order with ordered
//            ballots that writes the two masks and the sampled indices in ascending order.
//   gather   the sampled proposals, their labels, clamped matches and regression targets in one launch.
// Every output word has one writer, no launch waits on another workgroup, nothing uses a global or a floating-point atomic (the
// per-tile maxima and the histograms are integer atomics in LDS, whose result does not depend on their order), and every product,
// sum and quotient that decides a result bit is a correctly rounded fp32 operation in a stated order.
#include "common.h"
#include "glue.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxGt = 1024;            // EDTR_TARGETS_MAX_GT
constexpr int kMaxBatch = 4096;         // EDTR_TARGETS_MAX_BATCH
constexpr int kTile = 1024;             // EDTR_TARGETS_TILE: boxes of one workgroup of the scan and the assign pass
constexpr int kPerLane = kTile / 256;
constexpr int kLimit = 1 << 24;
constexpr int kSampleLanes = 1024;
constexpr uint32_t kNanKey = 0xffffffffu;       // score_key of every NaN

struct MatchArgs {
    const float* boxes;         // [sum P][4], or [P][4] shared by every image
    const float* gt;            // [sum G][4]
    const int64_t* gt_labels;   // [sum G] (RoI form)
    const int32_t* table;       // [N + 1][2]: box_start, gt_start
    int shared, tiles, gmax, allow_low;
    float high, low, wx, wy, ww, wh;
    float* best_val;            // [sum P]
    int32_t* best_idx;          // [sum P]
    uint32_t* partial;          // [N][tiles][gmax]: the key of the greatest IoU of ground truth g inside a tile
    int32_t* matched;           // [sum P]
    void* labels;               // [sum P] fp32 (RPN form) or int64 (RoI form)
    float* regression;          // [sum P][4] or NULL (RPN form)
};

// torch.max / torch.min of two elements: a NaN on either side is the result
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float clamp_min0(float v) { return v < 0.0f ? 0.0f : v; }             // clamp(min=0): a NaN stays
__device__ __forceinline__ float box_area(f32x4 b) { return mul_rn(add_rn(b.z, -b.x), add_rn(b.w, -b.y)); }

// torchvision's box_iou for one pair, each step one rounded fp32 operation: inter / ((area_g + area_p) - inter)
__device__ __forceinline__ float box_iou(f32x4 g, float area_g, f32x4 p, float area_p) {
    const float w = clamp_min0(add_rn(nan_min(g.z, p.z), -nan_max(g.x, p.x)));
    const float h = clamp_min0(add_rn(nan_min(g.w, p.w), -nan_max(g.y, p.y)));
    const float inter = mul_rn(w, h);
    return div_rn(inter, add_rn(add_rn(area_g, area_p), -inter));
}

// encode_boxes (model/util.py:594-638) for one pair in the reference's operation order: w (gcx - ecx) / ew, w log(gw / ew)
__device__ __forceinline__ f32x4 encode_box(f32x4 g, f32x4 p, float wx, float wy, float ww, float wh) {
    const float ew = add_rn(p.z, -p.x), eh = add_rn(p.w, -p.y);
    const float ecx = add_rn(p.x, mul_rn(0.5f, ew)), ecy = add_rn(p.y, mul_rn(0.5f, eh));
    const float gw = add_rn(g.z, -g.x), gh = add_rn(g.w, -g.y);
    const float gcx = add_rn(g.x, mul_rn(0.5f, gw)), gcy = add_rn(g.y, mul_rn(0.5f, gh));
    f32x4 o;
    o.x = div_rn(mul_rn(wx, add_rn(gcx, -ecx)), ew), o.y = div_rn(mul_rn(wy, add_rn(gcy, -ecy)), eh);
    o.z = mul_rn(ww, logf(div_rn(gw, ew))), o.w = mul_rn(wh, logf(div_rn(gh, eh)));
    return o;
}

__device__ __forceinline__ f32x4 load_box(const float* base, int64_t i) { return *reinterpret_cast<const f32x4*>(base + 4 * i); }

// Workgroup (tile, image).  Lane -> boxes tile kTile + u 256 + tid, u < kPerLane, so that a wave reads consecutive boxes.  For every
// ground truth in turn: the IoU with the lane's boxes, the running best by torch's max(dim=0) rule (the first maximal g; the first
// NaN wins outright), and the tile's maximum for that ground truth: the keys' maximum over the wave by shuffles, then one integer
// atomic maximum per wave in LDS (a NaN is the largest key, as torch's max(dim=1) propagates it).
__global__ void __launch_bounds__(256) match_scan_kernel(MatchArgs a) {
    __shared__ f32x4 gbox[kMaxGt];
    __shared__ float garea[kMaxGt];
    __shared__ uint32_t gkey[kMaxGt];
    const int tile = (int)blockIdx.x, n = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63;
    const int64_t b0 = a.table[2 * n], g0 = a.table[2 * n + 1];
    const int P = (int)(a.table[2 * n + 2] - b0);
    int G = (int)(a.table[2 * n + 3] - g0);
    G = G > kMaxGt ? kMaxGt : G;
    if (G <= 0 || (int64_t)tile * kTile >= P) return;       // (uniform) an image without ground truth needs no scan
    for (int g = tid; g < G; g += 256) {
        const f32x4 b = load_box(a.gt, g0 + g);
        gbox[g] = b, garea[g] = box_area(b), gkey[g] = 0u;
    }
    __syncthreads();
    f32x4 pb[kPerLane];
    float pa[kPerLane], best[kPerLane];
    int bi[kPerLane];
    bool have[kPerLane];
#pragma unroll
    for (int u = 0; u < kPerLane; ++u) {
        const int i = tile * kTile + u * 256 + tid;
        have[u] = i < P;
        pb[u] = have[u] ? load_box(a.boxes, a.shared ? (int64_t)i : b0 + i) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        pa[u] = box_area(pb[u]), best[u] = 0.0f, bi[u] = 0;
    }
    for (int g = 0; g < G; ++g) {
        const f32x4 gb = gbox[g];
        const float ga = garea[g];
        uint32_t k = 0u;                        // below every key
#pragma unroll
        for (int u = 0; u < kPerLane; ++u) {
            const float v = box_iou(gb, ga, pb[u], pa[u]);
            if (g == 0 || (!(best[u] != best[u]) && (v > best[u] || v != v))) best[u] = v, bi[u] = g;
            const uint32_t kv = have[u] ? score_key(v) : 0u;
            k = kv > k ? kv : k;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)k, off);
            k = o > k ? o : k;
        }
        if (lane == 0) atomicMax(&gkey[g], k);
    }
    __syncthreads();
    uint32_t* part = a.partial + ((int64_t)n * a.tiles + tile) * a.gmax;
    for (int g = tid; g < G; g += 256) part[g] = gkey[g];
#pragma unroll
    for (int u = 0; u < kPerLane; ++u) {
        const int i = tile * kTile + u * 256 + tid;
        if (have[u]) a.best_val[b0 + i] = best[u], a.best_idx[b0 + i] = bi[u];
    }
}

// Workgroup (tile, image).  highest[g] = the maximum over the image's tiles of the scan's keys, folded in LDS.  Then per box: the
// thresholds on the best value (-1 below low, -2 in [low, high); a NaN compares false both times and keeps its index); with
// allow_low, a box that lost its index gets it back iff its IoU with some ground truth equals that ground truth's highest (a NaN
// highest equals nothing) — set_low_quality_matches_, the all-zero row included.  Labels in the form's dtype; the RPN form encodes
// every box against gt[max(matched, 0)].  An image without ground truth: matched 0, label 0, encoded against the zero box.
template <int FORM>
__global__ void __launch_bounds__(256) match_assign_kernel(MatchArgs a) {
    __shared__ f32x4 gbox[kMaxGt];
    __shared__ float garea[kMaxGt];
    __shared__ uint32_t ghigh[kMaxGt];
    const int tile = (int)blockIdx.x, n = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int64_t b0 = a.table[2 * n], g0 = a.table[2 * n + 1];
    const int P = (int)(a.table[2 * n + 2] - b0);
    int G = (int)(a.table[2 * n + 3] - g0);
    G = G > kMaxGt ? kMaxGt : G;
    if ((int64_t)tile * kTile >= P) return;                 // (uniform)
    const int tiles_n = (P + kTile - 1) / kTile;
    for (int g = tid; g < G; g += 256) {
        const f32x4 b = load_box(a.gt, g0 + g);
        gbox[g] = b, garea[g] = box_area(b);
        const uint32_t* part = a.partial + (int64_t)n * a.tiles * a.gmax + g;
        uint32_t k = 0u;
        for (int t = 0; t < tiles_n; ++t) {
            const uint32_t o = part[(int64_t)t * a.gmax];
            k = o > k ? o : k;
        }
        ghigh[g] = k;
    }
    __syncthreads();
    for (int u = 0; u < kPerLane; ++u) {
        const int i = tile * kTile + u * 256 + tid;
        if (i >= P) continue;
        const f32x4 pb = load_box(a.boxes, a.shared ? (int64_t)i : b0 + i);
        int m = 0;
        if (G > 0) {
            const float val = a.best_val[b0 + i];
            const int idx = clamp_index(a.best_idx[b0 + i], G);
            m = val < a.low ? -1 : ((val >= a.low && val < a.high) ? -2 : idx);
            if (a.allow_low && m < 0) {
                const float pa = box_area(pb);
                bool restore = false;
                for (int g = 0; g < G; ++g) {
                    const uint32_t key = score_key(box_iou(gbox[g], garea[g], pb, pa));
                    restore = restore || (key == ghigh[g] && key != kNanKey);
                }
                m = restore ? idx : m;
            }
        }
        a.matched[b0 + i] = m;
        if (FORM == EDTR_TARGETS_RPN) {
            static_cast<float*>(a.labels)[b0 + i] = (G <= 0 || m == -1) ? 0.0f : (m >= 0 ? 1.0f : -1.0f);
            if (a.regression) {
                const f32x4 gb = G > 0 ? gbox[m < 0 ? 0 : m] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                *reinterpret_cast<f32x4*>(a.regression + 4 * (b0 + i)) = encode_box(gb, pb, a.wx, a.wy, a.ww, a.wh);
            }
        } else {
            static_cast<int64_t*>(a.labels)[b0 + i] = (G <= 0 || m == -1) ? (int64_t)0 : (m >= 0 ? a.gt_labels[g0 + m] : (int64_t)-1);
        }
    }
}

__global__ void __launch_bounds__(256) encode_kernel(const float* ref, const float* proposals, int64_t K, float wx, float wy, float ww, float wh,
                                                     float* out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < K; e += (int64_t)gridDim.x * 256)
        *reinterpret_cast<f32x4*>(out + 4 * e) = encode_box(load_box(ref, e), load_box(proposals, e), wx, wy, ww, wh);
}

struct SampleArgs {
    uint32_t k0, k1;
    const int64_t* ids;         // [N] global image ids, or NULL: id_base + n
    uint32_t id_base, draw, purpose;
    const void* labels;         // [sum P] fp32 (RPN form) or int64 (RoI form)
    const uint32_t* keys;       // [sum P] keys in place of the stream's words, or NULL
    const int32_t* table;       // [N + 1][2]: box_start, gt_start
    int batch, max_pos;
    uint8_t* mask_pos;          // [sum P]
    uint8_t* mask_neg;          // [sum P]
    int32_t* sampled;           // [N][batch]
    int32_t* counts;            // [N][2]: num_pos, num_neg
};

// 1 positive (label >= 1), 0 negative (label == 0), 2 neither
template <int FORM>
__device__ __forceinline__ int label_class(const void* labels, int64_t i) {
    if (FORM == EDTR_TARGETS_RPN) {
        const float v = static_cast<const float*>(labels)[i];
        return v >= 1.0f ? 1 : (v == 0.0f ? 0 : 2);
    }
    const int64_t v = static_cast<const int64_t*>(labels)[i];
    return v >= 1 ? 1 : (v == 0 ? 0 : 2);
}

constexpr int kBins = 2048;             // the select's digits are 11, 11 and 10 bits wide
constexpr int kBinsPerLane = kBins / 64;
constexpr int kHistWords = kBins + kBins / kBinsPerLane;

// where bin b lives in a histogram: one word of padding after every kBinsPerLane bins, so that the lanes of the scan, each walking
// its own kBinsPerLane consecutive bins, read kBinsPerLane + 1 words apart and never share an LDS bank
__device__ __forceinline__ int bin_slot(uint32_t b) { return (int)(b + b / kBinsPerLane); }

// Wave 0 only.  Lane l owns bins l kBinsPerLane .. of histogram h: s = their sum, incl = the sum over the lanes up to and including l.
__device__ __forceinline__ void scan_bins(const uint32_t* h, int lane, uint32_t& s, uint32_t& incl) {
    s = 0u;
    for (int k = 0; k < kBinsPerLane; ++k) s += h[lane * (kBinsPerLane + 1) + k];
    incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
        incl += lane >= off ? o : 0u;
    }
}

// Wave 0 only, after scan_bins: the bin of the digit at `shift` in which the need-th SMALLEST key lies among those that match
// `prefix`, and how many are still to take inside it.  (The keys that match the prefix number at least `need`, so some lane's
// inclusive sum reaches it; need == 0 gives bin 0 and nothing to take.)
__device__ __forceinline__ void locate_bin(const uint32_t* h, int lane, uint32_t s, uint32_t incl, uint32_t prefix, uint32_t need, int shift,
                                           uint32_t* found) {
    const uint64_t reach = __ballot(incl >= need);
    const int owner = reach ? __builtin_ctzll(reach) : 63;
    if (lane != owner) return;
    uint32_t below = incl - s;
    int b = lane * kBinsPerLane;
    for (int k = 0; k < kBinsPerLane - 1; ++k, ++b) {
        const uint32_t v = h[bin_slot((uint32_t)b)];
        if (below + v >= need) break;
        below += v;
    }
    found[0] = prefix | ((uint32_t)b << shift);
    found[1] = need - below;
}

// the classes (label_class, two bits each) of boxes i0 .. i0 + 3 of an image of P boxes; 2 past its end
template <int FORM>
__device__ __forceinline__ uint32_t classes4(const void* labels, int64_t b0, int64_t i0, int P) {
    uint32_t pc = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) pc |= (uint32_t)(i0 + j < P ? label_class<FORM>(labels, b0 + i0 + j) : 2) << (2 * j);
    return pc;
}

// the keys of boxes 4 q .. 4 q + 3 of image `id`: one Philox call, or the caller's own keys (0 past the image's end)
__device__ __forceinline__ u32x4 keys4(const SampleArgs& a, uint32_t id, int64_t b0, int q, int P) {
    if (!a.keys) return philox4x32_10(u32x4{(uint32_t)q, a.draw, a.purpose, id}, a.k0, a.k1);
    const int64_t i0 = 4 * (int64_t)q;
    u32x4 w;
    w.x = i0 < P ? a.keys[b0 + i0] : 0u, w.y = i0 + 1 < P ? a.keys[b0 + i0 + 1] : 0u;
    w.z = i0 + 2 < P ? a.keys[b0 + i0 + 2] : 0u, w.w = i0 + 3 < P ? a.keys[b0 + i0 + 3] : 0u;
    return w;
}

// One workgroup per image.  The key of box i is word i & 3 of Philox on the counter (i >> 2, draw, purpose, image id) — or keys[i], where
// the caller hands keys in (tests do, to reach equal keys) —; a lane owns the four boxes of one Philox call, in both phases.
//   select   three passes over the key's digits from the top (11, 11 and 10 bits; a histogram does not care about order): per class a
//            histogram in LDS of the boxes that match the prefix found so far, then — by a scan over wave 0 — the bin in which the k-th
//            SMALLEST key lies.  The first pass's histograms also count the classes, which gives num_pos = min(#positive, max_pos)
//            and num_neg = min(#negative, batch - num_pos).  After the last pass the prefix is the threshold key T of the class and
//            `need` the number of boxes with key == T to take (k = 0: T = 0 and need = 0, nothing is below or taken).
//   compact  one pass in index order, lane -> boxes 4 q .. 4 q + 3: a box is sampled iff its key < T, or == T with fewer than `need`
//            equal keys of its class before it, and its place among the sampled is the number sampled before it; both counts are
//            ordered ballots, one per box of the lane, summed over the lanes below, the waves below and the rounds before.
template <int FORM>
__global__ void __launch_bounds__(kSampleLanes) sample_kernel(SampleArgs a) {
    __shared__ uint32_t hist[2][kHistWords];
    __shared__ uint32_t found[2][2];
    __shared__ int take[2];
    __shared__ int wave_eq[kSampleLanes / 64][2], wave_sel[kSampleLanes / 64];
    const int n = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t b0 = a.table[2 * n];
    const int P = (int)(a.table[2 * n + 2] - b0);
    const uint32_t id = EDTR_IMAGE_ID(a, n);

    uint32_t t0 = 0u, t1 = 0u, himask = 0u;          // the prefix of the negatives' and the positives' threshold key
    uint32_t need0 = 0u, need1 = 0u;
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
        const uint32_t digit = pass == 2 ? 0x3ffu : 0x7ffu;
        for (int b = tid; b < 2 * kHistWords; b += kSampleLanes) (&hist[0][0])[b] = 0u;
        __syncthreads();
        for (int q = tid; 4 * (int64_t)q < P; q += kSampleLanes) {
            const uint32_t pc = classes4<FORM>(a.labels, b0, 4 * (int64_t)q, P);
            const u32x4 w = keys4(a, id, b0, q, P);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (int)((pc >> (2 * j)) & 3u);
                const uint32_t key = word_of(w, j);
                if (c < 2 && (key & himask) == (c ? t1 : t0)) atomicAdd(&hist[c][bin_slot((key >> shift) & digit)], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {
            uint32_t s0, i0, s1, i1;
            scan_bins(hist[0], lane, s0, i0);
            scan_bins(hist[1], lane, s1, i1);
            if (pass == 0) {
                const int neg = __shfl((int)i0, 63), pos = __shfl((int)i1, 63);
                const int np = pos < a.max_pos ? pos : a.max_pos;
                const int nn = neg < a.batch - np ? neg : a.batch - np;
                need1 = (uint32_t)np, need0 = (uint32_t)nn;
                if (lane == 0) take[0] = nn, take[1] = np;
            }
            locate_bin(hist[0], lane, s0, i0, t0, need0, shift, found[0]);
            locate_bin(hist[1], lane, s1, i1, t1, need1, shift, found[1]);
        }
        __syncthreads();
        t0 = found[0][0], need0 = found[0][1], t1 = found[1][0], need1 = found[1][1];
        himask |= digit << shift;
        __syncthreads();                        // found and hist are written again
    }

    int base_eq0 = 0, base_eq1 = 0, base_sel = 0;
    int32_t* out = a.sampled + (int64_t)n * a.batch;
    uint32_t pc_next = classes4<FORM>(a.labels, b0, 4 * (int64_t)tid, P);
    for (int q0 = 0; 4 * (int64_t)q0 < P; q0 += kSampleLanes) {
        const int q = q0 + tid;
        const int64_t i0 = 4 * (int64_t)q;
        const uint32_t pc = pc_next;
        pc_next = classes4<FORM>(a.labels, b0, i0 + 4 * kSampleLanes, P);      // the next round's, fetched under this round's barriers
        const u32x4 w = keys4(a, id, b0, q, P);
        int c[4];
        uint32_t key[4];
        bool eq0[4], eq1[4];
        int pe0 = 0, pe1 = 0, all0 = 0, all1 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = (int)((pc >> (2 * j)) & 3u), key[j] = word_of(w, j);
            eq0[j] = c[j] == 0 && key[j] == t0, eq1[j] = c[j] == 1 && key[j] == t1;
            const uint64_t v0 = __ballot(eq0[j]), v1 = __ballot(eq1[j]);
            pe0 += __popcll(v0 & lanes_below(lane)), pe1 += __popcll(v1 & lanes_below(lane));
            all0 += __popcll(v0), all1 += __popcll(v1);
        }
        if (lane == 0) wave_eq[wave][0] = all0, wave_eq[wave][1] = all1;
        __syncthreads();
        pe0 += base_eq0, pe1 += base_eq1;
        for (int w2 = 0; w2 < kSampleLanes / 64; ++w2) {
            const int e0 = wave_eq[w2][0], e1 = wave_eq[w2][1];
            pe0 += w2 < wave ? e0 : 0, pe1 += w2 < wave ? e1 : 0;
            base_eq0 += e0, base_eq1 += e1;
        }
        bool sel_pos[4], sel_neg[4];
        int pos = 0, all_sel = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sel_neg[j] = c[j] == 0 && (key[j] < t0 || (eq0[j] && (uint32_t)pe0 < need0));
            sel_pos[j] = c[j] == 1 && (key[j] < t1 || (eq1[j] && (uint32_t)pe1 < need1));
            pe0 += eq0[j] ? 1 : 0, pe1 += eq1[j] ? 1 : 0;
            const uint64_t vs = __ballot(sel_neg[j] || sel_pos[j]);
            pos += __popcll(vs & lanes_below(lane)), all_sel += __popcll(vs);
        }
        if (lane == 0) wave_sel[wave] = all_sel;
        __syncthreads();                        // (the next round writes wave_eq after this, when every lane has read it)
        pos += base_sel;
        for (int w2 = 0; w2 < kSampleLanes / 64; ++w2) {
            const int sw = wave_sel[w2];
            pos += w2 < wave ? sw : 0;
            base_sel += sw;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j >= P) continue;
            a.mask_pos[b0 + i0 + j] = sel_pos[j] ? 1 : 0, a.mask_neg[b0 + i0 + j] = sel_neg[j] ? 1 : 0;
            if (sel_neg[j] || sel_pos[j]) {
                if (pos < a.batch) out[pos] = (int32_t)(i0 + j);
                ++pos;
            }
        }
    }
    for (int j = base_sel + tid; j < a.batch; j += kSampleLanes) out[j] = -1;
    if (tid == 0) a.counts[2 * n] = take[1], a.counts[2 * n + 1] = take[0];
}

struct GatherArgs {
    const float* boxes;         // [sum P][4]
    const float* gt;            // [sum G][4]
    const int32_t* matched;     // [sum P]
    const int64_t* labels;      // [sum P]
    const int32_t* table;       // [N + 1][2]
    const int32_t* sampled;     // [N][batch]
    int batch;
    int64_t total;              // N batch
    float wx, wy, ww, wh;
    float* out_boxes;           // [N][batch][4]
    int64_t* out_labels;        // [N][batch]
    int64_t* out_matched;       // [N][batch]
    float* out_targets;         // [N][batch][4]
};

// slot (n, j): the sampled box, its label, max(matched, 0) and encode_box against that ground truth (the zero box for an image
// without any); a slot past the sampled count: zeros and label -1
__global__ void __launch_bounds__(256) gather_kernel(GatherArgs a) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * 256) {
        const int n = (int)(e / a.batch);
        const int64_t b0 = a.table[2 * n], g0 = a.table[2 * n + 1];
        const int P = (int)(a.table[2 * n + 2] - b0), G = (int)(a.table[2 * n + 3] - g0);
        const int idx = a.sampled[e];
        f32x4 pb = {0.0f, 0.0f, 0.0f, 0.0f}, t = {0.0f, 0.0f, 0.0f, 0.0f};
        int64_t label = -1, m = 0;
        if (idx >= 0 && idx < P) {
            pb = load_box(a.boxes, b0 + idx);
            label = a.labels[b0 + idx];
            m = G > 0 ? clamp_index(a.matched[b0 + idx], G) : 0;
            const f32x4 gb = G > 0 ? load_box(a.gt, g0 + m) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            t = encode_box(gb, pb, a.wx, a.wy, a.ww, a.wh);
        }
        *reinterpret_cast<f32x4*>(a.out_boxes + 4 * e) = pb;
        *reinterpret_cast<f32x4*>(a.out_targets + 4 * e) = t;
        a.out_labels[e] = label, a.out_matched[e] = m;
    }
}

// table_host [N + 1][2] = box_start, gt_start: what every entry point checks first, in this order.  tiles: of the longest image.
inline int check_table(const int32_t* table_host, const void* table, int N, int& tiles, int& gmax) {
    if (!table_host || !table) return EDTR_E_NULL;
    if (N <= 0) return EDTR_E_SHAPE;
    if (N > 65535) return EDTR_E_UNSUPPORTED;
    if (table_host[0] != 0 || table_host[1] != 0) return EDTR_E_SHAPE;
    int pmax = 1;
    gmax = 1;
    for (int n = 0; n < N; ++n) {
        const int64_t P = (int64_t)table_host[2 * n + 2] - table_host[2 * n], G = (int64_t)table_host[2 * n + 3] - table_host[2 * n + 1];
        if (P <= 0 || G < 0) return EDTR_E_SHAPE;
        if (P >= kLimit || G > kMaxGt) return EDTR_E_UNSUPPORTED;
        pmax = P > pmax ? (int)P : pmax, gmax = G > gmax ? (int)G : gmax;
    }
    tiles = (pmax + kTile - 1) / kTile;
    return EDTR_OK;
}

inline bool weights_ok(const float* w) {
    for (int c = 0; c < 4; ++c)
        if (!(w[c] == w[c])) return false;
    return true;
}

}  // namespace

extern "C" int edtr_targets_match(const float* boxes, int shared, const float* gt_boxes, const int64_t* gt_labels, const int32_t* table_host,
                                  const int32_t* table, int N, float high, float low, int allow_low_quality, int form,
                                  const float* weights_host, float* best_val, int32_t* best_idx, uint32_t* partial, int64_t partial_words,
                                  int32_t* matched, void* labels, float* regression, edtr_stream_t stream) {
    static_assert(kMaxGt == EDTR_TARGETS_MAX_GT && kMaxBatch == EDTR_TARGETS_MAX_BATCH && kTile == EDTR_TARGETS_TILE,
                  "edtr_hip.h and targets.hip disagree on a cap");
    int tiles = 0, gmax = 0;
    const int rc = check_table(table_host, table, N, tiles, gmax);
    if (rc != EDTR_OK) return rc;
    if (!boxes || !best_val || !best_idx || !partial || !matched || !labels) return EDTR_E_NULL;
    if (form != EDTR_TARGETS_RPN && form != EDTR_TARGETS_ROI) return EDTR_E_DTYPE;
    if ((shared != 0 && shared != 1) || (allow_low_quality != 0 && allow_low_quality != 1)) return EDTR_E_DTYPE;
    const int64_t total_gt = table_host[2 * N + 1];
    if (total_gt > 0 && (!gt_boxes || (form == EDTR_TARGETS_ROI && !gt_labels))) return EDTR_E_NULL;
    if (form == EDTR_TARGETS_RPN && regression && !weights_host) return EDTR_E_NULL;
    if (!(low <= high) || partial_words < (int64_t)N * tiles * gmax) return EDTR_E_SHAPE;
    if (shared)
        for (int n = 0; n < N; ++n)
            if (table_host[2 * n + 2] - table_host[2 * n] != table_host[2]) return EDTR_E_SHAPE;
    if (form == EDTR_TARGETS_RPN && regression && !weights_ok(weights_host)) return EDTR_E_SHAPE;
    if (!all_aligned_to(16, boxes, gt_boxes, regression) || !aligned_to(labels, form == EDTR_TARGETS_RPN ? 4 : 8) || !aligned_to(gt_labels, 8) ||
        !all_aligned_to(4, table, best_idx, matched) || !all_aligned_to(4, best_val) || !aligned_to(partial, 4))
        return EDTR_E_ALIGN;
    MatchArgs a;
    a.boxes = boxes, a.gt = gt_boxes, a.gt_labels = gt_labels, a.table = table;
    a.shared = shared, a.tiles = tiles, a.gmax = gmax, a.allow_low = allow_low_quality;
    a.high = high, a.low = low;
    const bool enc = form == EDTR_TARGETS_RPN && regression;
    a.wx = enc ? weights_host[0] : 1.0f, a.wy = enc ? weights_host[1] : 1.0f, a.ww = enc ? weights_host[2] : 1.0f, a.wh = enc ? weights_host[3] : 1.0f;
    a.best_val = best_val, a.best_idx = best_idx, a.partial = partial, a.matched = matched, a.labels = labels;
    a.regression = form == EDTR_TARGETS_RPN ? regression : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)tiles, (unsigned)N), block(256);
    if (total_gt > 0) {
        hipLaunchKernelGGL(match_scan_kernel, grid, block, 0, st, a);
        EDTR_LAUNCH_CHECK();
    }
    if (form == EDTR_TARGETS_RPN) hipLaunchKernelGGL(match_assign_kernel<EDTR_TARGETS_RPN>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(match_assign_kernel<EDTR_TARGETS_ROI>, grid, block, 0, st, a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_targets_encode(const float* reference_boxes, const float* proposals, int64_t K, const float* weights_host, float* out,
                                   edtr_stream_t stream) {
    if (!reference_boxes || !proposals || !weights_host || !out) return EDTR_E_NULL;
    if (K <= 0 || !weights_ok(weights_host)) return EDTR_E_SHAPE;
    if (K > (int64_t)1 << 30) return EDTR_E_UNSUPPORTED;
    if (!all_aligned_to(16, reference_boxes, proposals, out)) return EDTR_E_ALIGN;
    hipLaunchKernelGGL(encode_kernel, dim3(blocks_for(K)), dim3(256), 0, static_cast<hipStream_t>(stream), reference_boxes, proposals, K,
                       weights_host[0], weights_host[1], weights_host[2], weights_host[3], out);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_targets_sample(const void* labels, int form, const int32_t* table_host, const int32_t* table, int N, int batch, int max_pos,
                                   uint64_t seed, const int64_t* image_ids, int64_t image_id_base, int64_t draw, int purpose, const uint32_t* keys,
                                   uint8_t* mask_pos, uint8_t* mask_neg, int32_t* sampled, int32_t* counts, edtr_stream_t stream) {
    int tiles = 0, gmax = 0;
    const int rc = check_table(table_host, table, N, tiles, gmax);
    if (rc != EDTR_OK) return rc;
    if (!labels || !mask_pos || !mask_neg || !sampled || !counts) return EDTR_E_NULL;
    if (batch <= 0 || max_pos < 0 || max_pos > batch || !draw_ok(draw)) return EDTR_E_SHAPE;
    if (batch > kMaxBatch) return EDTR_E_UNSUPPORTED;
    if (form != EDTR_TARGETS_RPN && form != EDTR_TARGETS_ROI) return EDTR_E_DTYPE;
    if (purpose != EDTR_NOISE_SAMPLE_RPN && purpose != EDTR_NOISE_SAMPLE_ROI) return EDTR_E_DTYPE;
    SampleArgs a;
    if (int rk = key_stream(a, N, seed, image_ids, image_id_base)) return rk;
    if (!aligned_to(labels, form == EDTR_TARGETS_RPN ? 4 : 8) || !all_aligned_to(4, table, sampled, counts) || !aligned_to(keys, 4)) return EDTR_E_ALIGN;
    a.draw = (uint32_t)draw, a.purpose = (uint32_t)purpose;
    a.labels = labels, a.keys = keys, a.table = table, a.batch = batch, a.max_pos = max_pos;
    a.mask_pos = mask_pos, a.mask_neg = mask_neg, a.sampled = sampled, a.counts = counts;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (form == EDTR_TARGETS_RPN) hipLaunchKernelGGL(sample_kernel<EDTR_TARGETS_RPN>, dim3((unsigned)N), dim3(kSampleLanes), 0, st, a);
    else hipLaunchKernelGGL(sample_kernel<EDTR_TARGETS_ROI>, dim3((unsigned)N), dim3(kSampleLanes), 0, st, a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_targets_gather(const float* boxes, const float* gt_boxes, const int32_t* matched, const int64_t* labels,
                                   const int32_t* table_host, const int32_t* table, int N, const int32_t* sampled, int batch,
                                   const float* weights_host, float* out_boxes, int64_t* out_labels, int64_t* out_matched, float* out_targets,
                                   edtr_stream_t stream) {
    int tiles = 0, gmax = 0;
    const int rc = check_table(table_host, table, N, tiles, gmax);
    if (rc != EDTR_OK) return rc;
    if (!boxes || !matched || !labels || !sampled || !weights_host || !out_boxes || !out_labels || !out_matched || !out_targets) return EDTR_E_NULL;
    if (table_host[2 * N + 1] > 0 && !gt_boxes) return EDTR_E_NULL;
    if (batch <= 0 || !weights_ok(weights_host)) return EDTR_E_SHAPE;
    if (batch > kMaxBatch) return EDTR_E_UNSUPPORTED;
    if (!all_aligned_to(16, boxes, gt_boxes, out_boxes, out_targets) || !all_aligned_to(8, labels, out_labels, out_matched) ||
        !all_aligned_to(4, matched, table, sampled))
        return EDTR_E_ALIGN;
    GatherArgs a;
    a.boxes = boxes, a.gt = gt_boxes, a.matched = matched, a.labels = labels, a.table = table, a.sampled = sampled;
    a.batch = batch, a.total = (int64_t)N * batch;
    a.wx = weights_host[0], a.wy = weights_host[1], a.ww = weights_host[2], a.wh = weights_host[3];
    a.out_boxes = out_boxes, a.out_labels = out_labels, a.out_matched = out_matched, a.out_targets = out_targets;
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(a.total)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
