// The training losses (edtr_hip.h "Training losses"; the host restatements are edtr_amd/losses.py): the weighted mean-L1 over a list of
// feature pairs, forward and backward, and the classifier's cross-entropy on rows of logits, forward and backward.  The L1 is a
// streaming path: the forward reads each operand once, the backward reads each operand once and writes each gradient once.  Every fp64
// sum runs in an order the element count alone decides; no atomics, no memset, one writer per word, nothing depends on the grid.
#include "common.h"
#include "glue.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxPairs = 8;                // EDTR_L1_MAX_PAIRS
constexpr int kChunk = 4096;                // EDTR_L1_CHUNK: elements of one partial sum, four quarters of 256 lanes x 4 elements
constexpr int kQuarter = kChunk / 4;
constexpr int64_t kMaxElems = 1 << 30;      // EDTR_L1_MAX_ELEMS
constexpr int kMaxClasses = 65536;          // EDTR_CLS_MAX_CLASSES
constexpr int kMaxRows = 65535;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// the pairs of one launch, by value in the kernel's arguments.  first[k]: the number of chunks before pair k (first[pairs]: all of them)
struct L1Pairs {
    const void* a[kMaxPairs];
    const void* b[kMaxPairs];
    void* ga[kMaxPairs];                    // the backward's outputs; either may be NULL
    void* gb[kMaxPairs];
    int64_t n[kMaxPairs];
    int64_t first[kMaxPairs + 1];
    float w[kMaxPairs];
    int dtype[kMaxPairs];
    int vec[kMaxPairs];                     // every pointer of the pair that the launch touches is aligned to a lane's vector
    int pairs;
};

// the pair that holds chunk g
__device__ __forceinline__ int pair_of(const L1Pairs& t, int64_t g) {
    int k = 0;
    while (k + 1 < t.pairs && g >= t.first[k + 1]) ++k;
    return k;
}

// elements i .. i + 3 of a pair's operand widened exactly to fp32; those at or past n are not read (and come back as 0).  VEC: i + 4 <= n
// is one load of 16 (fp32) or 8 bytes.
template <int DT>
__device__ __forceinline__ void load4(const void* base, int64_t i, int64_t n, bool vec, float v[4]) {
    if (vec && i + 4 <= n) {
        if (DT == EDTR_LOGITS_F32) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(static_cast<const float*>(base) + i);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            const u32x2 q = *reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(base) + i);
            const uint16_t r[4] = {(uint16_t)(q.x & 0xffffu), (uint16_t)(q.x >> 16), (uint16_t)(q.y & 0xffffu), (uint16_t)(q.y >> 16)};
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = DT == EDTR_LOGITS_F16 ? F16::to_f32(r[j]) : BF16::to_f32(r[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < n ? load1<DT>(base, i + j) : 0.0f;
    }
}

// a lane's share of one chunk of |a - b|: its four elements of each quarter, ascending, added in fp64 from +0
template <int DT>
__device__ __forceinline__ double l1_lane_sum(const void* a, const void* b, int64_t base, int64_t n, bool vec, int lane) {
    float va[4][4], vb[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {           // (all eight loads are in flight before the first is used)
        const int64_t i = base + q * kQuarter + 4 * lane;
        load4<DT>(a, i, n, vec, va[q]);
        load4<DT>(b, i, n, vec, vb[q]);
    }
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = base + q * kQuarter + 4 * lane;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < n) s += (double)fabsf(add_rn(va[q][j], -vb[q][j]));
    }
    return s;
}

// the tree s = 128, 64, ..., 1 with sum[l] += sum[l + s] over 256 lane sums, valid in lane 0.  The two upper levels through `buf` (256
// doubles that no lane reads or writes again before the workgroup's next barrier), the six lower ones by shuffles inside wave 0: lane l
// takes lane l + s's value exactly where the tree reads it, so the additions and their order are the tree's.
__device__ __forceinline__ double tree256(double s, double* buf, int lane) {
    buf[lane] = s;
    __syncthreads();
    double v = 0.0;
    if (lane < 64) {
        v = (buf[lane] + buf[lane + 128]) + (buf[lane + 64] + buf[lane + 192]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    }
    return v;
}

// part[g] = the fp64 sum of |a - b| over chunk g of the concatenated pairs.  Workgroups stride over the chunks; the two LDS buffers take
// turns, so that one barrier a chunk is enough (a lane that writes buffer g & 1 again has passed the barrier of chunk g + 1, which wave 0
// reaches only after it has read chunk g's sums).
__global__ void __launch_bounds__(256) l1_chunks_kernel(L1Pairs t, double* part) {
    __shared__ double sums[2][256];
    const int lane = (int)threadIdx.x;
    const int64_t total = t.first[t.pairs];
    int turn = 0;
    for (int64_t g = blockIdx.x; g < total; g += gridDim.x, turn ^= 1) {
        const int k = pair_of(t, g);
        const int64_t base = (g - t.first[k]) * kChunk, n = t.n[k];
        const bool vec = t.vec[k] != 0;
        double s;
        if (t.dtype[k] == EDTR_LOGITS_F32) s = l1_lane_sum<EDTR_LOGITS_F32>(t.a[k], t.b[k], base, n, vec, lane);
        else if (t.dtype[k] == EDTR_LOGITS_F16) s = l1_lane_sum<EDTR_LOGITS_F16>(t.a[k], t.b[k], base, n, vec, lane);
        else s = l1_lane_sum<EDTR_LOGITS_BF16>(t.a[k], t.b[k], base, n, vec, lane);
        s = tree256(s, sums[turn], lane);
        if (lane == 0) part[g] = s;
    }
}

// one workgroup: per pair, lane l adds partials l, l + 256, ... ascending, the tree, the division by n; then the weighted terms in pair order
__global__ void __launch_bounds__(256) l1_finalize_kernel(L1Pairs t, const double* part, float* loss, float* terms) {
    __shared__ double sums[2][256];
    const int lane = (int)threadIdx.x;
    double total = 0.0;
    for (int k = 0; k < t.pairs; ++k) {
        double s = 0.0;
        for (int64_t g = t.first[k] + lane; g < t.first[k + 1]; g += 256) s += part[g];
        s = tree256(s, sums[k & 1], lane);
        if (lane == 0) {
            const double term = s / (double)t.n[k];
            total += (double)t.w[k] * term;
            if (terms) terms[k] = (float)term;
        }
    }
    if (lane == 0) loss[0] = (float)total;
}

// four gradients of one sign pattern stored as the pair's type: fp32 words, or 16-bit values two to a word
template <int DT>
__device__ __forceinline__ void store4(void* base, int64_t i, int64_t n, bool vec, const uint32_t bits[4]) {
    if (vec && i + 4 <= n) {
        if (DT == EDTR_LOGITS_F32) {
            u32x4 q;
            q.x = bits[0], q.y = bits[1], q.z = bits[2], q.w = bits[3];
            *reinterpret_cast<u32x4*>(static_cast<uint32_t*>(base) + i) = q;
        } else {
            u32x2 q;
            q.x = bits[0] | bits[1] << 16, q.y = bits[2] | bits[3] << 16;
            *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(base) + i) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j >= n) continue;
            if (DT == EDTR_LOGITS_F32) static_cast<uint32_t*>(base)[i + j] = bits[j];
            else static_cast<uint16_t*>(base)[i + j] = (uint16_t)bits[j];
        }
    }
}

// one chunk of both gradients.  cbits: c_k in the pair's type (fp32 bits, or the 16-bit value in the low half); top: that type's sign bit
template <int DT>
__device__ __forceinline__ void l1_backward_chunk(const void* a, const void* b, void* ga, void* gb, int64_t base, int64_t n, bool vec, float c, int lane) {
    const uint32_t cbits = DT == EDTR_LOGITS_F32 ? __float_as_uint(c) : (uint32_t)(DT == EDTR_LOGITS_F16 ? F16::from_f32(c) : BF16::from_f32(c));
    const uint32_t top = DT == EDTR_LOGITS_F32 ? 0x80000000u : 0x8000u;
    float va[4][4], vb[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = base + q * kQuarter + 4 * lane;
        load4<DT>(a, i, n, vec, va[q]);
        load4<DT>(b, i, n, vec, vb[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = base + q * kQuarter + 4 * lane;
        if (i >= n) continue;
        uint32_t pa[4], pb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = add_rn(va[q][j], -vb[q][j]);
            pa[j] = d > 0.0f ? cbits : (d < 0.0f ? cbits ^ top : 0u);       // (zero and NaN: +0.0)
            pb[j] = pa[j] ^ top;
        }
        if (ga) store4<DT>(ga, i, n, vec, pa);
        if (gb) store4<DT>(gb, i, n, vec, pb);
    }
}

__global__ void __launch_bounds__(256) l1_backward_kernel(L1Pairs t, const float* grad_loss) {
    const int lane = (int)threadIdx.x;
    const int64_t total = t.first[t.pairs];
    const double g = (double)grad_loss[0];
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const int k = pair_of(t, item);
        if (!t.ga[k] && !t.gb[k]) continue;
        const int64_t base = (item - t.first[k]) * kChunk, n = t.n[k];
        const float c = (float)(g * (double)t.w[k] / (double)n);
        const bool vec = t.vec[k] != 0;
        if (t.dtype[k] == EDTR_LOGITS_F32) l1_backward_chunk<EDTR_LOGITS_F32>(t.a[k], t.b[k], t.ga[k], t.gb[k], base, n, vec, c, lane);
        else if (t.dtype[k] == EDTR_LOGITS_F16) l1_backward_chunk<EDTR_LOGITS_F16>(t.a[k], t.b[k], t.ga[k], t.gb[k], base, n, vec, c, lane);
        else l1_backward_chunk<EDTR_LOGITS_BF16>(t.a[k], t.b[k], t.ga[k], t.gb[k], base, n, vec, c, lane);
    }
}

// ---- the classifier's cross-entropy ------------------------------------------------------------------------------------------------

// One wave64 workgroup per row b = blockIdx.x; lane l owns classes l, l + 64, ...  lse[b] = m + logf(sum of expf(z_c - m)) and, for a row
// that counts, term[b] = (double)(lse - z_label).  (fmaxf drops a NaN; the sum then carries it into lse and the loss.)
template <int DT>
__global__ void __launch_bounds__(64) cls_ce_forward_kernel(const void* logits, const int32_t* labels, int C, int ignore, float* lse, double* term) {
    const int lane = (int)threadIdx.x, b = (int)blockIdx.x;
    const int64_t base = (int64_t)b * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, load1<DT>(logits, base + c));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s = add_rn(s, expf(add_rn(load1<DT>(logits, base + c), -m)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = add_rn(s, __shfl_down(s, o, 64));
    if (lane != 0) return;
    const float v = add_rn(m, logf(s));
    lse[b] = v;
    const int label = labels[b];
    term[b] = label != ignore && label >= 0 && label < C ? (double)add_rn(v, -load1<DT>(logits, base + label)) : 0.0;
}

// one workgroup: the counted rows' terms folded in row order by lane 0 (256 at a time through LDS) -> loss = float(sum / count), counts
__global__ void __launch_bounds__(256) cls_ce_finalize_kernel(const double* term, const int32_t* labels, int B, int C, int ignore, float* loss,
                                                              int64_t* counts) {
    __shared__ double st[256];
    __shared__ int sl[256];
    const int tid = (int)threadIdx.x;
    double sum = 0.0;
    int64_t count = 0, bad = 0;
    for (int base = 0; base < B; base += 256) {
        if (base + tid < B) st[tid] = term[base + tid], sl[tid] = labels[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int m = B - base < 256 ? B - base : 256;
            for (int k = 0; k < m; ++k) {
                const int label = sl[k];
                if (label == ignore) continue;
                if (label >= 0 && label < C) sum += st[k], ++count;
                else ++bad;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        loss[0] = (float)(sum / (double)count);         // no counted row: 0 / 0 = NaN, torch's answer
        counts[0] = count, counts[1] = bad;
    }
}

// grad [B][C]: a workgroup per row, lanes over the classes
template <int DT>
__global__ void __launch_bounds__(256) cls_ce_backward_kernel(const void* logits, const int32_t* labels, int C, int ignore, const float* lse,
                                                              const int64_t* counts, const float* grad_loss, void* grad) {
    const int b = (int)blockIdx.x;
    const int64_t base = (int64_t)b * C;
    const int64_t count = counts[0];
    const int label = labels[b];
    const bool live = count > 0 && label != ignore && label >= 0 && label < C;
    const float g = live ? div_rn(grad_loss[0], (float)count) : 0.0f;
    const float l = lse[b];
    for (int c = (int)threadIdx.x; c < C; c += 256) {
        float v = 0.0f;
        if (live) v = mul_rn(add_rn(expf(add_rn(load1<DT>(logits, base + c), -l)), c == label ? -1.0f : 0.0f), g);
        if (DT == EDTR_LOGITS_F32) static_cast<float*>(grad)[base + c] = v;
        else static_cast<uint16_t*>(grad)[base + c] = DT == EDTR_LOGITS_F16 ? F16::from_f32(v) : BF16::from_f32(v);
    }
}

inline bool known_dtype(int dt) { return dt == EDTR_LOGITS_F32 || dt == EDTR_LOGITS_F16 || dt == EDTR_LOGITS_BF16; }

// what the three L1 entry points check of the host arrays, in the header's order; fills the table's operands, counts and chunk starts
inline int check_pairs(const int32_t* dtype_host, const void* const* a_host, const void* const* b_host, const int64_t* n_host, const float* weight_host,
                       int pairs, int max_blocks, void* const* ga_host, void* const* gb_host, bool backward, L1Pairs& t) {
    if (!dtype_host || !a_host || !b_host || !n_host || !weight_host || (backward && (!ga_host || !gb_host))) return EDTR_E_NULL;
    if (pairs < 1 || pairs > kMaxPairs || max_blocks < 0) return EDTR_E_SHAPE;
    bool any = false;
    for (int k = 0; k < pairs; ++k) {
        if (!a_host[k] || !b_host[k]) return EDTR_E_NULL;
        any = any || (backward && (ga_host[k] || gb_host[k]));
    }
    if (backward && !any) return EDTR_E_NULL;
    for (int k = 0; k < pairs; ++k)
        if (!known_dtype(dtype_host[k])) return EDTR_E_DTYPE;
    for (int k = 0; k < pairs; ++k)
        if (n_host[k] <= 0) return EDTR_E_SHAPE;
    for (int k = 0; k < pairs; ++k)
        if (n_host[k] > kMaxElems) return EDTR_E_UNSUPPORTED;
    t = L1Pairs{};
    t.pairs = pairs;
    for (int k = 0; k < pairs; ++k) {
        t.a[k] = a_host[k], t.b[k] = b_host[k], t.n[k] = n_host[k], t.w[k] = weight_host[k], t.dtype[k] = dtype_host[k];
        t.ga[k] = backward ? ga_host[k] : nullptr, t.gb[k] = backward ? gb_host[k] : nullptr;
        t.first[k + 1] = t.first[k] + (n_host[k] + kChunk - 1) / kChunk;
    }
    return EDTR_OK;
}

// the pointers of every pair are aligned to their element (else EDTR_E_ALIGN); vec[k]: and to a lane's vector of four
inline int check_alignment(L1Pairs& t) {
    for (int k = 0; k < t.pairs; ++k) {
        const uintptr_t elem = t.dtype[k] == EDTR_LOGITS_F32 ? 4 : 2;
        if (!all_aligned_to(elem, t.a[k], t.b[k]) || !all_aligned_to(elem, t.ga[k], t.gb[k])) return EDTR_E_ALIGN;
        t.vec[k] = all_aligned_to(4 * elem, t.a[k], t.b[k]) && all_aligned_to(4 * elem, t.ga[k], t.gb[k]) ? 1 : 0;
    }
    return EDTR_OK;
}

inline unsigned l1_grid(int64_t chunks, int max_blocks) {
    const int64_t cap = max_blocks > 0 ? max_blocks : 8 * (int64_t)edtr_cu_count();
    return (unsigned)(chunks > cap ? cap : chunks);
}

inline int check_ce(int dt, const void* logits, const int32_t* labels, int B, int C) {
    if (!logits || !labels) return EDTR_E_NULL;
    if (!known_dtype(dt)) return EDTR_E_DTYPE;
    if (B <= 0 || C <= 0) return EDTR_E_SHAPE;
    if (B > kMaxRows || C > kMaxClasses) return EDTR_E_UNSUPPORTED;
    return EDTR_OK;
}

}  // namespace

extern "C" int64_t edtr_l1_workspace(const int64_t* n_host, int pairs) {
    if (!n_host || pairs < 1 || pairs > kMaxPairs) return 0;
    int64_t chunks = 0;
    for (int k = 0; k < pairs; ++k) {
        if (n_host[k] <= 0 || n_host[k] > kMaxElems) return 0;
        chunks += (n_host[k] + kChunk - 1) / kChunk;
    }
    return 8 * chunks;
}

extern "C" int edtr_l1_forward(const int32_t* dtype_host, const void* const* a_host, const void* const* b_host, const int64_t* n_host,
                               const float* weight_host, int pairs, void* workspace, int64_t workspace_bytes, float* loss, float* terms,
                               int max_blocks, edtr_stream_t stream) {
    static_assert(kMaxPairs == EDTR_L1_MAX_PAIRS && kChunk == EDTR_L1_CHUNK && kMaxElems == EDTR_L1_MAX_ELEMS,
                  "edtr_hip.h and losses.hip disagree on the L1 limits");
    if (!workspace || !loss) return EDTR_E_NULL;
    L1Pairs t;
    int bad = check_pairs(dtype_host, a_host, b_host, n_host, weight_host, pairs, max_blocks, nullptr, nullptr, false, t);
    if (bad != EDTR_OK) return bad;
    if (workspace_bytes < 8 * t.first[pairs]) return EDTR_E_SHAPE;
    if ((bad = check_alignment(t)) != EDTR_OK) return bad;
    if (!all_aligned_to(4, loss, terms) || !aligned_to(workspace, 8)) return EDTR_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(l1_chunks_kernel, dim3(l1_grid(t.first[pairs], max_blocks)), dim3(256), 0, st, t, part);
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(l1_finalize_kernel, dim3(1), dim3(256), 0, st, t, part, loss, terms);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_l1_backward(const int32_t* dtype_host, const void* const* a_host, const void* const* b_host, const int64_t* n_host,
                                const float* weight_host, int pairs, const float* grad_loss, void* const* grad_a_host, void* const* grad_b_host,
                                int max_blocks, edtr_stream_t stream) {
    if (!grad_loss) return EDTR_E_NULL;
    L1Pairs t;
    int bad = check_pairs(dtype_host, a_host, b_host, n_host, weight_host, pairs, max_blocks, grad_a_host, grad_b_host, true, t);
    if (bad != EDTR_OK) return bad;
    if ((bad = check_alignment(t)) != EDTR_OK) return bad;
    if (!aligned_to(grad_loss, 4)) return EDTR_E_ALIGN;
    hipLaunchKernelGGL(l1_backward_kernel, dim3(l1_grid(t.first[pairs], max_blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), t, grad_loss);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_cls_ce_forward(int logits_dtype, const void* logits, const int32_t* labels, int B, int C, int ignore_index, float* lse,
                                   void* workspace, int64_t workspace_bytes, float* loss, int64_t* counts, edtr_stream_t stream) {
    static_assert(kMaxClasses == EDTR_CLS_MAX_CLASSES, "edtr_hip.h and losses.hip disagree on the class limit");
    if (!lse || !workspace || !loss || !counts) return EDTR_E_NULL;
    const int bad = check_ce(logits_dtype, logits, labels, B, C);
    if (bad != EDTR_OK) return bad;
    if (workspace_bytes < 8 * (int64_t)B) return EDTR_E_SHAPE;
    if (!aligned_to(logits, logits_dtype == EDTR_LOGITS_F32 ? 4 : 2) || !all_aligned_to(4, labels, lse, loss) || !all_aligned_to(8, workspace, counts))
        return EDTR_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* term = static_cast<double*>(workspace);
#define EDTR_CLS_CE(DT) hipLaunchKernelGGL((cls_ce_forward_kernel<DT>), dim3(B), dim3(64), 0, st, logits, labels, C, ignore_index, lse, term)
    if (logits_dtype == EDTR_LOGITS_F32) EDTR_CLS_CE(EDTR_LOGITS_F32);
    else if (logits_dtype == EDTR_LOGITS_F16) EDTR_CLS_CE(EDTR_LOGITS_F16);
    else EDTR_CLS_CE(EDTR_LOGITS_BF16);
#undef EDTR_CLS_CE
    EDTR_LAUNCH_CHECK();
    hipLaunchKernelGGL(cls_ce_finalize_kernel, dim3(1), dim3(256), 0, st, term, labels, B, C, ignore_index, loss, counts);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

extern "C" int edtr_cls_ce_backward(int logits_dtype, const void* logits, const int32_t* labels, int B, int C, int ignore_index, const float* lse,
                                    const int64_t* counts, const float* grad_loss, void* grad, edtr_stream_t stream) {
    if (!lse || !counts || !grad_loss || !grad) return EDTR_E_NULL;
    const int bad = check_ce(logits_dtype, logits, labels, B, C);
    if (bad != EDTR_OK) return bad;
    const uintptr_t elem = logits_dtype == EDTR_LOGITS_F32 ? 4 : 2;
    if (!aligned_to(logits, elem) || !aligned_to(grad, elem) || !all_aligned_to(4, labels, lse, grad_loss) || !aligned_to(counts, 8)) return EDTR_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define EDTR_CLS_CE(DT) \
    hipLaunchKernelGGL((cls_ce_backward_kernel<DT>), dim3(B), dim3(256), 0, st, logits, labels, C, ignore_index, lse, counts, grad_loss, grad)
    if (logits_dtype == EDTR_LOGITS_F32) EDTR_CLS_CE(EDTR_LOGITS_F32);
    else if (logits_dtype == EDTR_LOGITS_F16) EDTR_CLS_CE(EDTR_LOGITS_F16);
    else EDTR_CLS_CE(EDTR_LOGITS_BF16);
#undef EDTR_CLS_CE
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
