// Classification on the device (edtr_hip.h "Classification"; the host restatements and the rules themselves are edtr_amd/cls.py): the
// order behind topk for every row of a batch of logits, the per-image feature distance as fp64 partial sums in an order that depends
// on the element count alone, the dependent one-workgroup launch that counts, finalises and moves the record's offsets on, the
// classifier's input normalisation, and the data set's crop / flip / transpose window on uint8 images.
// Every output word has exactly one writer, no launch waits on another workgroup and nothing here uses an atomic; every store into a
// record is guarded by the record's capacity.  No product feeds a sum anywhere, and contraction is off all the same.
#include "common.h"
#include "glue.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxClasses = 65536;      // EDTR_CLS_MAX_CLASSES
constexpr int kMaxKeep = 8;             // EDTR_CLS_MAX_KEEP
constexpr int kMaxTopk = 4;             // EDTR_CLS_MAX_TOPK
constexpr int kChunk = 4096;            // EDTR_CLS_FD_CHUNK: elements of one partial sum, 16 per lane of 256
constexpr int kMaxElems = 1 << 28;      // EDTR_CLS_FD_MAX_ELEMS
constexpr int kMaxRows = 1 << 30;       // capacity, and where a running offset stops moving
constexpr int kLimit = 1 << 24;         // extents and origins of the window stay below this: every index fits an int
constexpr int kTile = 32;               // pixels per side of the window's LDS tile

// element i of a row, widened exactly to fp32.  DT: EDTR_LOGITS_F32 / _F16 / _BF16
template <int DT>
__device__ __forceinline__ float widen(const void* base, int64_t i) {
    if (DT == EDTR_LOGITS_F32) return static_cast<const float*>(base)[i];
    const uint16_t r = static_cast<const uint16_t*>(base)[i];
    return DT == EDTR_LOGITS_F16 ? F16::to_f32(r) : BF16::to_f32(r);
}

// (key, index) as one word whose unsigned order is the rule's order: a greater key first, equal keys by the smaller index.
// The low half stays below 2^31, so no entry equals the all-ones word the selection starts from.
__device__ __forceinline__ uint64_t place_word(uint32_t key, int idx) { return (uint64_t)key << 32 | (uint64_t)(0x7fffffffu - (uint32_t)idx); }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

// One wave64 workgroup per row b = blockIdx.x; lane l owns classes l, l + 64, ...
//   rank   every class j with place_word(j) > place_word(label) precedes the label: one ballot and one popcount per 64 classes
//   top    K rounds; round m takes the greatest word below the one round m - 1 took (a per-lane maximum, then one wave-wide one)
template <int DT>
__global__ void __launch_bounds__(64) cls_rank_kernel(const void* logits, const int32_t* labels, int C, int K, int32_t* rec_label,
                                                      int32_t* rec_rank, int32_t* rec_top, const int32_t* offset, int capacity) {
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x;
    const int64_t off = offset ? (int64_t)*offset : 0;
    const int64_t row = off + b;
    const bool room = off >= 0 && row < capacity;       // (an offset the caller broke writes nothing)
    const int64_t base = (int64_t)b * C;

    if (labels) {
        const int label = labels[b];
        int rank = C;
        if (label >= 0 && label < C) {
            const uint64_t mine = place_word(score_key(widen<DT>(logits, base + label)), label);
            rank = 0;
            for (int j0 = 0; j0 < C; j0 += 64) {
                const int j = j0 + lane;
                const bool before = j < C && place_word(score_key(widen<DT>(logits, base + j)), j) > mine;
                rank += __popcll(__ballot(before));
            }
        }
        if (lane == 0 && room) {
            rec_rank[row] = rank;
            if (rec_label) rec_label[row] = label;
        }
    }

    uint64_t last = ~0ull;
    for (int m = 0; m < K; ++m) {
        uint64_t best = 0ull;                           // (no entry is 0: the least key, that of -inf, is 0x007fffff)
        for (int j = lane; j < C; j += 64) {
            const uint64_t w = place_word(score_key(widen<DT>(logits, base + j)), j);
            best = (w < last && w > best) ? w : best;
        }
        best = wave_max_u64(best);
        if (lane == 0 && room) rec_top[row * K + m] = best ? (int32_t)(0x7fffffffu - (uint32_t)best) : -1;       // -1: K > C
        last = best;                                    // (0 once the row is used up: nothing lies below it)
    }
}

// One 256-lane workgroup per (chunk, image) = (blockIdx.x, blockIdx.y): lane l adds |a - b| of elements l, l + 256, ... of the chunk
// in that order in fp64 (the difference and its absolute value in fp32), then the fixed-pairing tree s = 128, 64, ..., 1 with
// sum[l] += sum[l + s] gives the chunk's partial.
template <int DT>
__global__ void __launch_bounds__(256) cls_fdist_kernel(const void* a, const void* b, int n, int chunks, double* partials) {
    __shared__ double sums[256];
    const int lane = (int)threadIdx.x, chunk = (int)blockIdx.x, image = (int)blockIdx.y;
    const int64_t base = (int64_t)image * n;
    const int lo = chunk * kChunk, hi = n - lo < kChunk ? n : lo + kChunk;
    double s = 0.0;
    for (int i = lo + lane; i < hi; i += 256) s += (double)fabsf(add_rn(widen<DT>(a, base + i), -widen<DT>(b, base + i)));
    sums[lane] = s;
    __syncthreads();
#pragma unroll
    for (int step = 128; step > 0; step >>= 1) {
        if (lane < step) sums[lane] += sums[lane + step];
        __syncthreads();
    }
    if (lane == 0) partials[(int64_t)image * chunks + chunk] = sums[0];
}

struct CommitArgs {
    const int32_t* rec_rank;        // NULL with n_topk == 0
    float* rec_fd;
    int32_t* rec_batch;
    const double* partials;         // NULL: no features, fd = NaN
    int32_t* batch_n;
    int32_t* batch_correct;         // [batch_capacity][n_topk]
    int32_t* offsets;               // (images, batches)
    int B, n, chunks, n_topk, capacity, batch_capacity;
    int topk[kMaxTopk];
};

__device__ __forceinline__ int32_t moved_on(int32_t offset, int by) { return offset < 0 || offset > kMaxRows ? offset : offset + by; }

// The dependent launch, one workgroup: for the batch whose ranks lie at rows offsets[0] ..., count rank < k per k (integer sums: per
// lane, per wave by shuffles, the four waves through LDS), finalise every image's feature distance (its partials added in chunk
// order in fp64, divided by n in fp64, rounded once), write the batch row and move both offsets on.
__global__ void __launch_bounds__(256) cls_commit_kernel(CommitArgs a) {
    __shared__ int counts[4][kMaxTopk];
    const int lane = (int)threadIdx.x;
    const int64_t off = a.offsets[0], boff = a.offsets[1];
    int correct[kMaxTopk] = {0, 0, 0, 0};
    for (int i = lane; i < a.B; i += 256) {
        const int64_t row = off + i;
        if (off < 0 || row >= a.capacity) continue;
        if (a.n_topk > 0) {
            const int rank = a.rec_rank[row];
#pragma unroll
            for (int t = 0; t < kMaxTopk; ++t) correct[t] += (t < a.n_topk && rank < a.topk[t]) ? 1 : 0;
        }
        float fd = __uint_as_float(0x7fc00000u);
        if (a.partials) {
            double s = 0.0;
            for (int c = 0; c < a.chunks; ++c) s += a.partials[(int64_t)i * a.chunks + c];
            fd = (float)(s / (double)a.n);
        }
        a.rec_fd[row] = fd;
        a.rec_batch[row] = (int32_t)boff;
    }
#pragma unroll
    for (int t = 0; t < kMaxTopk; ++t) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) correct[t] += __shfl_xor(correct[t], o, 64);
        if ((lane & 63) == 0) counts[lane >> 6][t] = correct[t];
    }
    __syncthreads();            // (also: every lane has read both offsets)
    if (lane != 0) return;
    if (boff >= 0 && boff < a.batch_capacity) {
        a.batch_n[boff] = a.B;
        for (int t = 0; t < a.n_topk; ++t) a.batch_correct[boff * a.n_topk + t] = counts[0][t] + counts[1][t] + counts[2][t] + counts[3][t];
    }
    a.offsets[0] = moved_on((int32_t)off, a.B);
    a.offsets[1] = moved_on((int32_t)boff, 1);
}

struct NormArgs {
    float mean[3], std[3];
};

// out = (x - mean_c) / std_c, each operation rounded: torchvision's Normalize (sub_ then div_).  VEC: a lane owns four elements of
// one plane as a float4 (H W % 4 == 0, 16-byte aligned tensors).
template <bool VEC>
__global__ void __launch_bounds__(256) cls_normalize_kernel(const float* x, float* out, int64_t total, int64_t plane, NormArgs k) {
    const int64_t per = VEC ? plane >> 2 : plane, items = VEC ? total >> 2 : total;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < items; g += (int64_t)gridDim.x * 256) {
        const int c = (int)((g / per) % 3);
        const float m = -(c == 0 ? k.mean[0] : (c == 1 ? k.mean[1] : k.mean[2])), s = c == 0 ? k.std[0] : (c == 1 ? k.std[1] : k.std[2]);
        if (VEC) {
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[g];
            f32x4 o;
            o.x = div_rn(add_rn(v.x, m), s), o.y = div_rn(add_rn(v.y, m), s), o.z = div_rn(add_rn(v.z, m), s), o.w = div_rn(add_rn(v.w, m), s);
            reinterpret_cast<f32x4*>(out)[g] = o;
        } else {
            out[g] = div_rn(add_rn(x[g], m), s);
        }
    }
}

template <int C>
__device__ __forceinline__ uint32_t load_px(const uint8_t* s) {
    return C == 1 ? (uint32_t)s[0] : ((uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16);
}
template <int C>
__device__ __forceinline__ void store_px(uint8_t* o, uint32_t p) {
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)(p >> (8 * c));
}

// The crop [H][W] at (y0, x0) of src [h][w], `fill` outside the source, both flips on the crop's indices, then (TR) the transpose:
//   !TR  dst [H][W]:  dst (y, x) = crop (y', x'),  y' = H - 1 - y under vflip, x' = W - 1 - x under hflip
//    TR  dst [W][H]:  dst (y, x) = crop (x', y'),  x' = H - 1 - x under vflip, y' = W - 1 - y under hflip
// A workgroup walks 32 x 32 tiles of the flipped crop (r, c).  !TR: lane order c fastest for the read and the write alike.  TR: the
// tile is read c fastest (along a source row) into LDS and written r fastest (along a row of dst); the 33-word pitch keeps the
// column reads of the second phase on distinct banks.
template <int C, bool TR>
__global__ void __launch_bounds__(256) cls_window_kernel(const uint8_t* src, int h, int w, uint8_t* dst, int H, int W, int y0, int x0,
                                                         int hflip, int vflip, uint32_t fill_px) {
    __shared__ uint32_t tile[kTile][kTile + 1];
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    const int64_t tiles = (int64_t)tiles_x * tiles_y;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int r0 = (int)(t / tiles_x) * kTile, c0 = (int)(t % tiles_x) * kTile;
        for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
            const int lr = i >> 5, lc = i & 31, r = r0 + lr, c = c0 + lc;
            if (r >= H || c >= W) continue;
            const int sy = y0 + (vflip ? H - 1 - r : r), sx = x0 + (hflip ? W - 1 - c : c);
            const uint32_t p = (sy >= 0 && sy < h && sx >= 0 && sx < w) ? load_px<C>(src + ((int64_t)sy * w + sx) * C) : fill_px;
            if (TR) tile[lr][lc] = p;
            else store_px<C>(dst + ((int64_t)r * W + c) * C, p);
        }
        if (TR) {
            __syncthreads();
            for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
                const int lc = i >> 5, lr = i & 31, r = r0 + lr, c = c0 + lc;
                if (r < H && c < W) store_px<C>(dst + ((int64_t)c * H + r) * C, tile[lr][lc]);
            }
            __syncthreads();        // the tile is overwritten for the next one
        }
    }
}

inline bool known_dtype(int dt) { return dt == EDTR_LOGITS_F32 || dt == EDTR_LOGITS_F16 || dt == EDTR_LOGITS_BF16; }

}  // namespace

extern "C" int edtr_cls_rank(int logits_dtype, const void* logits, const int32_t* labels, int B, int C, int K, int32_t* rec_label,
                             int32_t* rec_rank, int32_t* rec_top, const int32_t* offset, int capacity, edtr_stream_t stream) {
    static_assert(kMaxClasses == EDTR_CLS_MAX_CLASSES && kMaxKeep == EDTR_CLS_MAX_KEEP && kMaxTopk == EDTR_CLS_MAX_TOPK &&
                      kChunk == EDTR_CLS_FD_CHUNK && kMaxElems == EDTR_CLS_FD_MAX_ELEMS,
                  "edtr_hip.h and cls.hip disagree on a cap");
    static_assert(kChunk % 256 == 0, "a chunk is a whole number of elements per lane");
    if (!logits || (labels && !rec_rank) || (K > 0 && !rec_top)) return EDTR_E_NULL;
    if (B <= 0 || C <= 0 || K < 0 || capacity <= 0 || (!labels && K == 0)) return EDTR_E_SHAPE;
    if (B > 65535 || C > kMaxClasses || K > kMaxKeep || capacity > kMaxRows) return EDTR_E_UNSUPPORTED;
    if (!known_dtype(logits_dtype)) return EDTR_E_DTYPE;
    if (!aligned_to(logits, logits_dtype == EDTR_LOGITS_F32 ? 4 : 2) || !all_aligned_to(4, labels, rec_label, rec_rank, rec_top, offset))
        return EDTR_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)B), block(64);
    if (logits_dtype == EDTR_LOGITS_F32)
        hipLaunchKernelGGL(cls_rank_kernel<EDTR_LOGITS_F32>, grid, block, 0, st, logits, labels, C, K, rec_label, rec_rank, rec_top, offset, capacity);
    else if (logits_dtype == EDTR_LOGITS_F16)
        hipLaunchKernelGGL(cls_rank_kernel<EDTR_LOGITS_F16>, grid, block, 0, st, logits, labels, C, K, rec_label, rec_rank, rec_top, offset, capacity);
    else
        hipLaunchKernelGGL(cls_rank_kernel<EDTR_LOGITS_BF16>, grid, block, 0, st, logits, labels, C, K, rec_label, rec_rank, rec_top, offset, capacity);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_cls_fdist(int dtype, const void* a, const void* b, int B, int n, double* partials, edtr_stream_t stream) {
    if (!a || !b || !partials) return EDTR_E_NULL;
    if (B <= 0 || n <= 0) return EDTR_E_SHAPE;
    if (B > 65535 || n > kMaxElems) return EDTR_E_UNSUPPORTED;
    if (!known_dtype(dtype)) return EDTR_E_DTYPE;
    const uintptr_t elem = dtype == EDTR_LOGITS_F32 ? 4 : 2;
    if (!aligned_to(a, elem) || !aligned_to(b, elem) || !aligned_to(partials, 8)) return EDTR_E_ALIGN;
    const int chunks = (n + kChunk - 1) / kChunk;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)chunks, (unsigned)B), block(256);
    if (dtype == EDTR_LOGITS_F32) hipLaunchKernelGGL(cls_fdist_kernel<EDTR_LOGITS_F32>, grid, block, 0, st, a, b, n, chunks, partials);
    else if (dtype == EDTR_LOGITS_F16) hipLaunchKernelGGL(cls_fdist_kernel<EDTR_LOGITS_F16>, grid, block, 0, st, a, b, n, chunks, partials);
    else hipLaunchKernelGGL(cls_fdist_kernel<EDTR_LOGITS_BF16>, grid, block, 0, st, a, b, n, chunks, partials);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_cls_commit(const int32_t* rec_rank, float* rec_fd, int32_t* rec_batch, int B, const double* partials, int n,
                               const int32_t* topk_host, int n_topk, int32_t* batch_n, int32_t* batch_correct, int32_t* offsets,
                               int capacity, int batch_capacity, edtr_stream_t stream) {
    if (!rec_fd || !rec_batch || !batch_n || !offsets) return EDTR_E_NULL;
    if (n_topk > 0 && (!rec_rank || !topk_host || !batch_correct)) return EDTR_E_NULL;
    if (B <= 0 || n_topk < 0 || capacity <= 0 || batch_capacity <= 0 || (partials && n <= 0)) return EDTR_E_SHAPE;
    if (B > 65535 || n_topk > kMaxTopk || capacity > kMaxRows || batch_capacity > kMaxRows || (partials && n > kMaxElems)) return EDTR_E_UNSUPPORTED;
    for (int t = 0; t < n_topk; ++t) {
        if (topk_host[t] <= 0) return EDTR_E_SHAPE;
        if (topk_host[t] > kMaxKeep) return EDTR_E_UNSUPPORTED;
    }
    if (!all_aligned_to(4, rec_rank, rec_batch, batch_n, batch_correct, offsets) || !aligned_to(rec_fd, 4) || !aligned_to(partials, 8))
        return EDTR_E_ALIGN;
    CommitArgs a;
    a.rec_rank = rec_rank, a.rec_fd = rec_fd, a.rec_batch = rec_batch, a.partials = partials;
    a.batch_n = batch_n, a.batch_correct = batch_correct, a.offsets = offsets;
    a.B = B, a.n = partials ? n : 1, a.chunks = partials ? (n + kChunk - 1) / kChunk : 0, a.n_topk = n_topk;
    a.capacity = capacity, a.batch_capacity = batch_capacity;
    for (int t = 0; t < kMaxTopk; ++t) a.topk[t] = t < n_topk ? topk_host[t] : 0;
    hipLaunchKernelGGL(cls_commit_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_cls_normalize(const float* x, float* out, int B, int channels, int H, int W, const float* mean_host,
                                  const float* std_host, edtr_stream_t stream) {
    const int rc = check_batch(x, out, B, channels, H, W);
    if (rc != EDTR_OK) return rc;
    if (!mean_host || !std_host) return EDTR_E_NULL;
    NormArgs k;
    for (int c = 0; c < 3; ++c) {
        k.mean[c] = mean_host[c], k.std[c] = std_host[c];
        if (!(k.mean[c] == k.mean[c]) || !(k.std[c] == k.std[c]) || k.std[c] == 0.0f) return EDTR_E_SHAPE;
    }
    const int64_t plane = (int64_t)H * W, total = (int64_t)B * 3 * plane;
    const bool vec = plane % 4 == 0 && all_aligned_to(16, x, out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(cls_normalize_kernel<true>, dim3(blocks_for(total / 4)), dim3(256), 0, st, x, out, total, plane, k);
    else hipLaunchKernelGGL(cls_normalize_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, st, x, out, total, plane, k);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_cls_window(const uint8_t* src, int h, int w, int channels, uint8_t* dst, int H, int W, int y0, int x0, int hflip,
                               int vflip, int transpose, int fill, edtr_stream_t stream) {
    if (channels != 1 && channels != 3) return EDTR_E_UNSUPPORTED;
    if (!src || !dst) return EDTR_E_NULL;
    if (h <= 0 || w <= 0 || H <= 0 || W <= 0) return EDTR_E_SHAPE;
    if (h > kLimit || w > kLimit || H > kLimit || W > kLimit || y0 < -kLimit || y0 > kLimit || x0 < -kLimit || x0 > kLimit) return EDTR_E_UNSUPPORTED;
    if ((hflip != 0 && hflip != 1) || (vflip != 0 && vflip != 1) || (transpose != 0 && transpose != 1) || fill < 0 || fill > 255) return EDTR_E_DTYPE;
    const uint32_t f = (uint32_t)fill, fill_px = channels == 1 ? f : (f | f << 8 | f << 16);
    const int64_t tiles = (int64_t)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
    const dim3 grid((unsigned)(tiles > 4096 ? 4096 : tiles)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define EDTR_CLS_WINDOW(CH, TR) hipLaunchKernelGGL((cls_window_kernel<CH, TR>), grid, block, 0, st, src, h, w, dst, H, W, y0, x0, hflip, vflip, fill_px)
    if (channels == 1) {
        if (transpose) EDTR_CLS_WINDOW(1, true);
        else EDTR_CLS_WINDOW(1, false);
    } else {
        if (transpose) EDTR_CLS_WINDOW(3, true);
        else EDTR_CLS_WINDOW(3, false);
    }
#undef EDTR_CLS_WINDOW
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
