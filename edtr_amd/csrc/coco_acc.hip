// Detection scores, the second half (edtr_hip.h "Detection scores"; the host restatements and the rule are edtr_amd/coco.py):
// COCOeval.accumulate and _summarizeDets from the running record of coco.hip, with no host sync and no record copy.
//   edtr_coco_order       every record row sorted by the composite key (label, score class, image, rank) — ONE strict total order that
//                         serves every (area range, maxDets, threshold), because a stable sort of a filtered subsequence is the
//                         subsequence of the stable sort.  1024-row tiles sorted in LDS (bitonic), then merge passes that ping-pong
//                         two buffers of the workspace, one workgroup per 1024 outputs with a merge-path split.  The key is strict, so
//                         no pass has to be stable and nothing here uses an atomic on device memory.
//   edtr_coco_accumulate  precision fp64 [T][R][K][A][M] and recall fp64 [T][K][A][M], one wave64 workgroup per (label, area range,
//                         threshold) walking the label's segment ONCE for the three maxDets (see the kernel).
//   edtr_coco_summarize   the 12 statistics in a summation order that depends on the shape alone (see the kernel).
// The host never learns the row count: grids are sized by the capacity, and lanes and workgroups past min(count, capacity) leave.
// fp64 arithmetic is rounded per operation (contraction off) and `/` is correctly rounded, so numpy repeats it bit for bit.
#include "common.h"
#include "glue.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 1024;             // EDTR_COCO_ACC_TILE: rows of one LDS sort, outputs of one merge workgroup
constexpr int kMaxRows = 1 << 22;       // EDTR_COCO_ACC_MAX_ROWS
constexpr int kMaxLabels = 256;         // EDTR_COCO_MAX_LABELS
constexpr int kThr = 10;                // the IoU thresholds of a record word (EDTR_COCO_MAX_THRESHOLDS)
constexpr int kRec = 101;               // recall thresholds
constexpr int kKeep = 100;              // EDTR_COCO_KEEP
constexpr uint64_t kIdxMask = (1ull << 48) - 1ull;

// One sortable row, 128 bits, compared as (hi, lo) unsigned:
//   hi = label << 55 | score class << 23 | biased image >> 9          lo = (biased image & 511) << 55 | rank << 48 | row index
// i.e. label (9 bits) . score class (32) . image (32) . rank (7) . row (48).  A row that does not take part (label outside
// [0, n_labels), rank outside [0, 100), or past the counter) is hi = all ones: it sorts behind every row that does.
struct alignas(16) Key {
    uint64_t hi, lo;
};

__device__ __forceinline__ bool key_less(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl) { return ah < bh || (ah == bh && al < bl); }

// coco.order_keys: ascending in this uint32 is the order of numpy's stable argsort of the NEGATED fp64 score — a greater score
// first, -0.0 and 0.0 one class, +inf first, -inf last of the numbers, every NaN one last class
__device__ __forceinline__ uint32_t order_key(float s) {
    if (s != s) return 0xffffffffu;
    if (s == 0.0f) return 0x7fffffffu;
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? u : ~(u | 0x80000000u);
}

__device__ __forceinline__ int rows_counted(const int32_t* counter, int capacity) {
    const int c = *counter;
    return c < 0 ? 0 : (c > capacity ? capacity : c);
}

struct OrderArgs {
    const int32_t* image;
    const int32_t* label;
    const float* score;
    const int32_t* rank;
    const int32_t* counter;
    int capacity, n_labels;
    Key* buf0;
    Key* buf1;
};

// tile b of the rows, keyed and sorted ascending in LDS (bitonic, 256 lanes on 1024 rows), written to buf0.  A tile that begins at
// or past the counter leaves; the last one is filled up with rows that do not take part.
__global__ void __launch_bounds__(256) coco_tile_sort_kernel(OrderArgs a) {
    __shared__ uint64_t shi[kTile];
    __shared__ uint64_t slo[kTile];
    const int n = rows_counted(a.counter, a.capacity);
    const int base = (int)blockIdx.x * kTile, t = (int)threadIdx.x;
    if (base >= n) return;
    for (int e = t; e < kTile; e += 256) {
        const int i = base + e;
        uint64_t hi = ~0ull, lo = (~0ull & ~kIdxMask) | (uint64_t)i;
        if (i < n) {
            const int lab = a.label[i], rk = a.rank[i];
            if (lab >= 0 && lab < a.n_labels && rk >= 0 && rk < kKeep) {
                const uint64_t img = (uint64_t)((uint32_t)a.image[i] ^ 0x80000000u);
                hi = ((uint64_t)lab << 55) | ((uint64_t)order_key(a.score[i]) << 23) | (img >> 9);
                lo = ((img & 511ull) << 55) | ((uint64_t)rk << 48) | (uint64_t)i;
            }
        }
        shi[e] = hi, slo[e] = lo;
    }
    __syncthreads();
    for (int k = 2; k <= kTile; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int p = t + 256 * q;
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const uint64_t ih = shi[i], il = slo[i], lh = shi[l], ll = slo[l];
                const bool up = (i & k) == 0;
                if (key_less(lh, ll, ih, il) == up) {
                    shi[i] = lh, slo[i] = ll;
                    shi[l] = ih, slo[l] = il;
                }
            }
            __syncthreads();
        }
    for (int e = t; e < kTile; e += 256) {
        Key v;
        v.hi = shi[e], v.lo = slo[e];
        a.buf0[base + e] = v;
    }
}

// One merge pass: runs of `width` rows (a multiple of the tile) of src, pairwise, into dst.  Workgroup b makes outputs [1024 b,
// 1024 b + 1024): two lanes find where its first and its last diagonal cut the pair (merge path, a binary search in device memory),
// the 1024 rows between the cuts go to LDS, every lane places four of them — its own place in its run plus the rows of the other run
// below it, a binary search in LDS (the key is strict: no two rows compare equal) — and the tile leaves in order.  A run without a
// partner is a copy.  Rows at or past the padded count do not exist.
__global__ void __launch_bounds__(256) coco_merge_kernel(const Key* __restrict__ src, Key* __restrict__ dst, const int32_t* counter, int capacity, int width) {
    __shared__ uint64_t ihi[kTile];
    __shared__ uint64_t ilo[kTile];
    __shared__ uint64_t ohi[kTile];
    __shared__ uint64_t olo[kTile];
    __shared__ int cut[2];
    const int n = rows_counted(counter, capacity);
    const int n_pad = (n + kTile - 1) / kTile * kTile;
    const int out0 = (int)blockIdx.x * kTile, t = (int)threadIdx.x;
    if (out0 >= n_pad) return;
    const int pair = out0 / (2 * width) * (2 * width);
    const int a0 = pair, a1 = min(pair + width, n_pad), b1 = min(pair + 2 * width, n_pad);
    const int la = a1 - a0, lb = b1 - a1;
    const Key* A = src + a0;
    const Key* B = src + a1;
    if (t < 2) {
        const int D = out0 - pair + t * kTile;              // rows of the pair before this diagonal; D <= la + lb
        int lo = max(0, D - lb), hi = min(D, la);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;                 // mid < la, 0 <= D - 1 - mid < lb
            const Key x = A[mid], y = B[D - 1 - mid];
            if (key_less(x.hi, x.lo, y.hi, y.lo)) lo = mid + 1;
            else hi = mid;
        }
        cut[t] = lo;
    }
    __syncthreads();
    const int i0 = cut[0], na = cut[1] - cut[0], j0 = out0 - pair - i0;
    for (int e = t; e < kTile; e += 256) {
        const Key v = e < na ? A[i0 + e] : B[j0 + (e - na)];
        ihi[e] = v.hi, ilo[e] = v.lo;
    }
    __syncthreads();
    for (int e = t; e < kTile; e += 256) {
        const uint64_t xh = ihi[e], xl = ilo[e];
        const bool from_a = e < na;
        int lo = from_a ? na : 0, hi = from_a ? kTile : na;       // the other run's part of the tile
        const int other0 = lo;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key_less(ihi[mid], ilo[mid], xh, xl)) lo = mid + 1;
            else hi = mid;
        }
        const int pos = (from_a ? e : e - na) + (lo - other0);
        ohi[pos] = xh, olo[pos] = xl;
    }
    __syncthreads();
    for (int e = t; e < kTile; e += 256) {
        Key v;
        v.hi = ohi[e], v.lo = olo[e];
        dst[out0 + e] = v;
    }
}

// the sorted rows' indices into `order`, each label's first place into seg_start [n_labels + 1] (a binary search per label; the rows
// that do not take part lie behind all of them, so seg_start[n_labels] = n_kept), and the status word: bit 0, the counter does not
// lie in [0, capacity]
__global__ void __launch_bounds__(256) coco_order_finish_kernel(const Key* __restrict__ sorted, const int32_t* counter, int capacity, int n_labels,
                                                                 int32_t* order, int32_t* seg_start, int32_t* n_kept, int32_t* status) {
    const int n = rows_counted(counter, capacity);
    const int n_pad = (n + kTile - 1) / kTile * kTile;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < n) {
        const Key v = sorted[i];
        if (v.hi != ~0ull) order[i] = (int32_t)(v.lo & kIdxMask);      // at most n rows take part and they come first: i < capacity
    }
    if (blockIdx.x != 0) return;
    for (int k = (int)threadIdx.x; k <= n_labels; k += 256) {
        const uint64_t bound = k == n_labels ? ~0ull : (uint64_t)k << 55;    // (label n_labels = 256 would still fit the 9 bits; all ones covers it)
        int lo = 0, hi = n_pad;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sorted[mid].hi < bound) lo = mid + 1;
            else hi = mid;
        }
        seg_start[k] = lo;
        if (k == n_labels) *n_kept = lo;
    }
    if (threadIdx.x == 0) {
        const int c = *counter;
        *status = (c < 0 || c > capacity) ? 1 : 0;
    }
}

// npig[4 k + a] = the ground truths of label k = blockIdx.x that are not ignored in area range a, counted by ballot (order-free, so
// exact however it is reduced); status bit 1: the ground-truth counter does not lie in [0, gt_capacity]
__global__ void __launch_bounds__(256) coco_npig_kernel(const int32_t* gt_label, const uint8_t* gt_ignore, const int32_t* gt_counter, int gt_capacity,
                                                         int32_t* npig, int32_t* status) {
    __shared__ int part[4][4];
    const int k = (int)blockIdx.x, t = (int)threadIdx.x;
    const int g = rows_counted(gt_counter, gt_capacity);
    int c[4] = {0, 0, 0, 0};
    for (int j0 = 0; j0 < g; j0 += 256) {                   // (uniform bounds: every lane reaches every ballot)
        const int j = j0 + t;
        const bool mine = j < g && gt_label[j] == k;
        const int ign = mine ? (int)gt_ignore[j] : 15;
#pragma unroll
        for (int ar = 0; ar < 4; ++ar) c[ar] += __popcll(__ballot(!((ign >> ar) & 1)));
    }
    if ((t & 63) == 0)
        for (int ar = 0; ar < 4; ++ar) part[t >> 6][ar] = c[ar];
    __syncthreads();
    if (t < 4) npig[4 * k + t] = part[0][t] + part[1][t] + part[2][t] + part[3][t];
    if (k == 0 && t == 0) {
        const int cnt = *gt_counter;
        if (cnt < 0 || cnt > gt_capacity) *status = *status | 2;
    }
}

struct AccArgs {
    const int32_t* order;
    const int32_t* seg_start;
    const uint64_t* match;
    const uint64_t* ignore;
    const int32_t* rank;
    const int32_t* npig;
    const double* rec_thr;      // [101]
    double* precision;          // [T][101][K][4][3]
    double* recall;             // [T][K][4][3]
    int K, capacity;
};

// One wave64 workgroup per (label k, area range ar, threshold t), blockIdx.x = (k 4 + ar) 10 + t.  npig = 0 leaves the -1.
// Otherwise the label's segment of `order` is walked once, 64 rows at a time, for the three maxDets at once (rank < 1, 10, 100 are
// three masks over the same walk).  With tp = match & ~ignore and fp = ~match & ~ignore at bit 4 t + ar, the j-th true positive
// (counted by ballot and popcount on top of the carried totals) has fp_j false positives before it and
//     P_j = j / ((fp_j + j) + spacing(1)),     rc_j = j / npig                                      (all fp64).
// accumulate's precision[r] = pr[searchsorted(rc, recThr[r], "left")] after the envelope from the right is max{P_j : rc_j >= recThr[r]}:
// the search always lands on a true positive, and between true positives pr only falls.  recThr rises with r, so P_j counts for
// r < cnt_j = #{r : recThr[r] <= rc_j} and is folded (an LDS max on positive doubles, as uint64: order-free) into bin cnt_j - 1 of
// 101; a suffix maximum over the bins ends it, 0 where nothing reached.  cnt_j comes from the fp64 division itself, never from
// ceil(recThr npig).  recall = J / npig with J the true positives of the whole walk.
__global__ void __launch_bounds__(64) coco_accumulate_kernel(AccArgs a) {
    __shared__ unsigned long long bins[3][104];
    __shared__ double thr[kRec];
    const int lane = (int)threadIdx.x;
    const int t = (int)blockIdx.x % kThr, ar = ((int)blockIdx.x / kThr) & 3, k = (int)blockIdx.x / (4 * kThr);
    const int64_t K = a.K;
    const int npig = a.npig[4 * k + ar];
    const int64_t rec_at = ((int64_t)(t * K + k) * 4 + ar) * 3;
    if (npig == 0) {
        for (int r = lane; r < kRec; r += 64) {
            const int64_t at = (((int64_t)(t * kRec + r) * K + k) * 4 + ar) * 3;
            a.precision[at] = -1.0, a.precision[at + 1] = -1.0, a.precision[at + 2] = -1.0;
        }
        if (lane < 3) a.recall[rec_at + lane] = -1.0;
        return;
    }
    for (int r = lane; r < kRec; r += 64) {
        thr[r] = a.rec_thr[r];
        bins[0][r] = 0ull, bins[1][r] = 0ull, bins[2][r] = 0ull;
    }
    __syncthreads();
    const int s0 = clamp_index(a.seg_start[k], a.capacity + 1), s1 = clamp_index(a.seg_start[k + 1], a.capacity + 1);
    const int bit = 4 * t + ar;
    const double dn = (double)npig, eps = 2.220446049250313e-16;        // np.spacing(1)
    const int max_det[3] = {1, 10, kKeep};
    int tpc[3] = {0, 0, 0}, fpc[3] = {0, 0, 0};
    for (int c = s0; c < s1; c += 64) {                     // (uniform bounds: every lane reaches every ballot)
        const int i = c + lane;
        const bool live = i < s1;
        const int row = live ? clamp_index(a.order[i], a.capacity) : 0;
        const int rk = live ? a.rank[row] : kKeep;
        const bool mt = live && ((a.match[row] >> bit) & 1ull), ig = !live || ((a.ignore[row] >> bit) & 1ull);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const bool in = rk < max_det[m];
            const bool tp = in && mt && !ig, fp = in && !mt && !ig;
            const uint64_t tpm = __ballot(tp), fpm = __ballot(fp);
            if (tp) {
                const double dj = (double)(tpc[m] + __popcll(tpm & lanes_below(lane)) + 1);
                const double df = (double)(fpc[m] + __popcll(fpm & lanes_below(lane)));
                const double p = dj / ((df + dj) + eps), rc = dj / dn;
                int r0 = clamp_index((int)(rc * 100.0), kRec);
                while (r0 < kRec - 1 && thr[r0 + 1] <= rc) ++r0;
                while (r0 > 0 && thr[r0] > rc) --r0;           // (recThr[0] = 0 <= rc: bin 0 at the least)
                atomicMax(&bins[m][r0], (unsigned long long)__double_as_longlong(p));
            }
            tpc[m] += __popcll(tpm), fpc[m] += __popcll(fpm);
        }
    }
    __syncthreads();
    if (lane < 3) {
        unsigned long long best = 0ull;
        for (int r = kRec - 1; r >= 0; --r) {
            const unsigned long long v = bins[lane][r];
            best = v > best ? v : best;
            bins[lane][r] = best;
        }
        const int j = lane == 0 ? tpc[0] : (lane == 1 ? tpc[1] : tpc[2]);
        a.recall[rec_at + lane] = (double)j / dn;
    }
    __syncthreads();
    for (int r = lane; r < kRec; r += 64) {
        const int64_t at = (((int64_t)(t * kRec + r) * K + k) * 4 + ar) * 3;
#pragma unroll
        for (int m = 0; m < 3; ++m) a.precision[at + m] = __longlong_as_double((long long)bins[m][r]);
    }
}

// Statistic s = blockIdx.x of COCOeval._summarizeDets, in THIS order of summation (coco.summarize_ordered_reference), which the
// shape alone decides:
//   s_tk = the entries > -1 of (t, k) added over r in index order, from 0       (a recall statistic has one entry per (t, k))
//   s_k  = s_tk added over t in index order, from 0;      S = s_k added over k in index order, from 0
// with the count of the entries alongside; the statistic is S / count, or -1 where the count is 0.
// s: 0 AP, 1 AP at threshold 0 (0.5), 2 AP at threshold 5 (0.75), 3 .. 5 AP of area ranges 1 .. 3 (all with maxDets 100);
//    6 .. 8 AR at maxDets 1, 10, 100; 9 .. 11 AR of area ranges 1 .. 3 (maxDets 100).
// out[12] (the 13th word) takes the status word, so that one copy fetches both.
__global__ void __launch_bounds__(256) coco_summarize_kernel(const double* __restrict__ precision, const double* __restrict__ recall, int K,
                                                             const int32_t* status, double* out) {
    __shared__ double s_tk[kThr * kMaxLabels];
    __shared__ int c_tk[kThr * kMaxLabels];
    __shared__ double s_k[kMaxLabels];
    __shared__ int c_k[kMaxLabels];
    const int s = (int)blockIdx.x, t = (int)threadIdx.x;
    const bool ap = s < 6;
    const int ar = s < 3 ? 0 : (s < 6 ? s - 2 : (s < 9 ? 0 : s - 8));
    const int m = (s >= 6 && s < 9) ? s - 6 : 2;
    const int t0 = s == 2 ? 5 : 0, t1 = s == 1 ? 1 : (s == 2 ? 6 : kThr);
    for (int e = t; e < kThr * K; e += 256) {
        const int th = e / K, k = e % K;
        double sum = 0.0;
        int cnt = 0;
        if (th >= t0 && th < t1) {
            if (ap) {
                for (int r = 0; r < kRec; ++r) {
                    const double v = precision[(((int64_t)(th * kRec + r) * K + k) * 4 + ar) * 3 + m];
                    if (v > -1.0) sum = sum + v, ++cnt;
                }
            } else {
                const double v = recall[((int64_t)(th * K + k) * 4 + ar) * 3 + m];
                if (v > -1.0) sum = sum + v, ++cnt;
            }
        }
        s_tk[e] = sum, c_tk[e] = cnt;
    }
    __syncthreads();
    for (int k = t; k < K; k += 256) {
        double sum = 0.0;
        int cnt = 0;
        for (int th = t0; th < t1; ++th) sum = sum + s_tk[th * K + k], cnt += c_tk[th * K + k];
        s_k[k] = sum, c_k[k] = cnt;
    }
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        int64_t cnt = 0;
        for (int k = 0; k < K; ++k) sum = sum + s_k[k], cnt += c_k[k];
        out[s] = cnt ? sum / (double)cnt : -1.0;
        if (s == 0) reinterpret_cast<int64_t*>(out)[12] = (int64_t)*status;
    }
}

inline int64_t sort_bytes(int capacity) { return 2 * ((int64_t)(capacity + kTile - 1) / kTile * kTile) * (int64_t)sizeof(Key); }

}  // namespace

extern "C" int64_t edtr_coco_accumulate_workspace(int capacity, int n_labels) {
    if (capacity <= 0 || capacity > kMaxRows || n_labels <= 0 || n_labels > kMaxLabels) return 0;
    return sort_bytes(capacity) + 16 * (int64_t)n_labels;
}

extern "C" int edtr_coco_order(const int32_t* rec_image, const int32_t* rec_label, const float* rec_score, const int32_t* rec_rank,
                               const int32_t* det_offset, int capacity, int n_labels, void* workspace, int64_t workspace_bytes,
                               int32_t* order, int32_t* seg_start, int32_t* n_kept, int32_t* status, edtr_stream_t stream) {
    static_assert(kTile == EDTR_COCO_ACC_TILE && kMaxRows == EDTR_COCO_ACC_MAX_ROWS && kMaxLabels == EDTR_COCO_MAX_LABELS &&
                      kKeep == EDTR_COCO_KEEP && kThr == EDTR_COCO_MAX_THRESHOLDS,
                  "edtr_hip.h and coco_acc.hip disagree on a cap");
    static_assert(kKeep <= 128 && kMaxLabels < 511 && kMaxRows <= (1 << 30), "7 bits of rank, 9 of label, int row arithmetic");
    if (!rec_image || !rec_label || !rec_score || !rec_rank || !det_offset || !workspace || !order || !seg_start || !n_kept || !status)
        return EDTR_E_NULL;
    if (capacity <= 0 || n_labels <= 0) return EDTR_E_SHAPE;
    if (capacity > kMaxRows || n_labels > kMaxLabels) return EDTR_E_UNSUPPORTED;
    if (workspace_bytes < edtr_coco_accumulate_workspace(capacity, n_labels)) return EDTR_E_SHAPE;
    if (!aligned_to(workspace, 16) || !all_aligned_to(4, rec_image, rec_label, rec_rank, det_offset, order, seg_start, n_kept, status) ||
        !aligned_to(rec_score, 4))
        return EDTR_E_ALIGN;
    const int tiles = (capacity + kTile - 1) / kTile;
    OrderArgs a;
    a.image = rec_image, a.label = rec_label, a.score = rec_score, a.rank = rec_rank, a.counter = det_offset;
    a.capacity = capacity, a.n_labels = n_labels;
    a.buf0 = static_cast<Key*>(workspace), a.buf1 = a.buf0 + (int64_t)tiles * kTile;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(coco_tile_sort_kernel, dim3((unsigned)tiles), dim3(256), 0, st, a);
    EDTR_LAUNCH_CHECK();
    Key* src = a.buf0;
    Key* dst = a.buf1;
    for (int64_t width = kTile; width < (int64_t)tiles * kTile; width *= 2) {
        hipLaunchKernelGGL(coco_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, st, (const Key*)src, dst, det_offset, capacity, (int)width);
        EDTR_LAUNCH_CHECK();
        Key* s = src;
        src = dst, dst = s;
    }
    hipLaunchKernelGGL(coco_order_finish_kernel, dim3((unsigned)(tiles * (kTile / 256))), dim3(256), 0, st, (const Key*)src, det_offset, capacity,
                       n_labels, order, seg_start, n_kept, status);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_coco_accumulate(const int32_t* order, const int32_t* seg_start, const uint64_t* rec_match, const uint64_t* rec_ignore,
                                    const int32_t* rec_rank, int capacity, const int32_t* gt_label, const uint8_t* gt_ignore,
                                    const int32_t* gt_offset, int gt_capacity, int n_labels, const double* recall_thresholds,
                                    void* workspace, int64_t workspace_bytes, double* precision, double* recall, int32_t* status,
                                    edtr_stream_t stream) {
    if (!order || !seg_start || !rec_match || !rec_ignore || !rec_rank || !gt_label || !gt_ignore || !gt_offset || !recall_thresholds ||
        !workspace || !precision || !recall || !status)
        return EDTR_E_NULL;
    if (capacity <= 0 || gt_capacity <= 0 || n_labels <= 0) return EDTR_E_SHAPE;
    if (capacity > kMaxRows || gt_capacity > (1 << 30) || n_labels > kMaxLabels) return EDTR_E_UNSUPPORTED;
    if (workspace_bytes < edtr_coco_accumulate_workspace(capacity, n_labels)) return EDTR_E_SHAPE;
    if (!aligned_to(workspace, 16) || !all_aligned_to(8, rec_match, rec_ignore, recall_thresholds, precision, recall) ||
        !all_aligned_to(4, order, seg_start, rec_rank, gt_label, gt_offset, status))
        return EDTR_E_ALIGN;
    int32_t* npig = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + sort_bytes(capacity));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(coco_npig_kernel, dim3((unsigned)n_labels), dim3(256), 0, st, gt_label, gt_ignore, gt_offset, gt_capacity, npig, status);
    EDTR_LAUNCH_CHECK();
    AccArgs a;
    a.order = order, a.seg_start = seg_start, a.match = rec_match, a.ignore = rec_ignore, a.rank = rec_rank, a.npig = npig;
    a.rec_thr = recall_thresholds, a.precision = precision, a.recall = recall, a.K = n_labels, a.capacity = capacity;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(n_labels * 4 * kThr)), dim3(64), 0, st, a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_coco_summarize(const double* precision, const double* recall, int n_labels, const int32_t* status, double* out,
                                   edtr_stream_t stream) {
    if (!precision || !recall || !status || !out) return EDTR_E_NULL;
    if (n_labels <= 0) return EDTR_E_SHAPE;
    if (n_labels > kMaxLabels) return EDTR_E_UNSUPPORTED;
    if (!all_aligned_to(8, precision, recall, out) || !aligned_to(status, 4)) return EDTR_E_ALIGN;
    hipLaunchKernelGGL(coco_summarize_kernel, dim3(12), dim3(256), 0, static_cast<hipStream_t>(stream), precision, recall, n_labels, status, out);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
