// The detector's input transform on the device (edtr_hip.h "Detector input"; the host restatement and the extent rule are
// edtr_amd/detinput.py): GeneralizedRCNNTransform.forward in eval mode — (x - mean) / std, F.interpolate(bilinear) to the extent the
// caller worked out, and the zero-padded batch — for a ragged list of images in ONE launch.  No normalised or resized intermediate is
// written: the taps are normalised as they are read and blended with glue.h's source_index / index_lambda / blend_taps, so an
// element's bits are those of the three steps run one after the other.  Every word of the batch has exactly one writer, the
// padding included; nothing is read from the batch and nothing here uses an atomic.
#include "common.h"
#include "glue.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxChannels = 4;         // EDTR_DET_MAX_CHANNELS
constexpr int kMaxExtent = 32768;       // EDTR_DET_MAX_EXTENT
constexpr int kTileW = 256;             // EDTR_DET_TILE_W: columns of a workgroup's tile, four per lane of a wave
constexpr int kTileH = 16;              // EDTR_DET_TILE_H: rows of the tile, a quarter of them to each of the four waves
constexpr int kCols = kTileW / 64;

struct NormArgs {
    float mean[kMaxChannels], std[kMaxChannels];
};

// four values of one row, at columns col[0 .. 3], into the row that starts at element `row` of the batch.  VEC: the columns are
// consecutive, col[0] % 4 == 0 and the pitch and base keep the 16 bytes (8 for a 16-bit batch) aligned; else element by element.
template <int OT, bool VEC>
__device__ __forceinline__ void store_cols(void* batch, int64_t row, const int (&col)[kCols], int W, const float (&v)[kCols]) {
    if (OT == EDTR_LOGITS_F32) {
        float* o = static_cast<float*>(batch) + row;
        if (VEC) {
            if (col[0] < W) {
                f32x4 q;
                q.x = v[0], q.y = v[1], q.z = v[2], q.w = v[3];
                *reinterpret_cast<f32x4*>(o + col[0]) = q;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kCols; ++j)
                if (col[j] < W) o[col[j]] = v[j];
        }
    } else {
        uint16_t* o = static_cast<uint16_t*>(batch) + row;
        if (VEC) {
            if (col[0] < W) {
                uint2 q;
                q.x = OT == EDTR_LOGITS_F16 ? F16::pack2(v[0], v[1]) : BF16::pack2(v[0], v[1]);
                q.y = OT == EDTR_LOGITS_F16 ? F16::pack2(v[2], v[3]) : BF16::pack2(v[2], v[3]);
                *reinterpret_cast<uint2*>(o + col[0]) = q;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kCols; ++j)
                if (col[j] < W) o[col[j]] = OT == EDTR_LOGITS_F16 ? F16::from_f32(v[j]) : BF16::from_f32(v[j]);
        }
    }
}

// the two taps of every column of a lane in source row `row`, normalised: (v - mean) / std with m = -mean, each step rounded
__device__ __forceinline__ void load_row(const float* row, const int (&x0)[kCols], const int (&x1)[kCols], float m, float s,
                                         float (&at0)[kCols], float (&at1)[kCols]) {
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
        at0[j] = div_rn(add_rn(row[x0[j]], m), s);
        at1[j] = div_rn(add_rn(row[x1[j]], m), s);
    }
}

// Workgroup (blockIdx.x, blockIdx.y) = (tile, image): a kTileH x kTileW tile of the image's slot [C][H][W].  Lane l of every wave owns
// the columns 4 l .. 4 l + 3 of the tile (VEC) or l, l + 64, l + 128, l + 192 (element-wise stores, coalesced either way); their tap
// indices and lambdas are worked out once and serve every row and channel of the strip.  Wave w takes the kRows consecutive rows
// kRows w ... of the tile, channel by channel: a row's taps are the same in all 64 lanes, and the normalised taps of the two source
// rows it blends stay in registers for the next row, which when upscaling needs at most one new source row (the divisions are what
// the kernel spends its time on).  Outside [0, oh) x [0, ow) the value is +0.0; a tile wholly outside loads nothing, and a column
// outside reads the clamped tap of the last column, inside the source.
template <int OT, bool VEC>
__global__ void __launch_bounds__(256) det_transform_kernel(const edtr_det_image* descs, int C, void* batch, int H, int W, int tiles_x,
                                                            NormArgs k) {
    constexpr int kRows = kTileH / 4;
    const edtr_det_image d = descs[blockIdx.y];
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int tile_y = (int)blockIdx.x / tiles_x, tile_x = (int)blockIdx.x - tile_y * tiles_x;
    const float sh = div_rn((float)d.h, (float)d.oh), sw = div_rn((float)d.w, (float)d.ow);

    int col[kCols], x0[kCols], x1[kCols];
    float tx[kCols];
#pragma unroll
    for (int j = 0; j < kCols; ++j) {
        col[j] = tile_x * kTileW + (VEC ? 4 * lane + j : lane + 64 * j);
        index_lambda(fmaxf(source_index(sw, col[j]), 0.0f), d.w, x0[j], tx[j]);
        x1[j] = x0[j] + (x0[j] < d.w - 1 ? 1 : 0);
    }
    const bool tile_inside = tile_x * kTileW < d.ow;            // the same in every lane of the workgroup
    const int64_t plane = (int64_t)H * W, slot = (int64_t)blockIdx.y * C * plane;
    const int ybase = tile_y * kTileH + wave * kRows;

#pragma unroll
    for (int c = 0; c < kMaxChannels; ++c) {
        if (c >= C) break;
        const float m = -k.mean[c], s = k.std[c];
        const float* src = d.src + (int64_t)c * d.h * d.w;
        int held0 = -1, held1 = -1;                             // the source rows whose normalised taps top / bot hold
        float top0[kCols] = {}, top1[kCols] = {}, bot0[kCols] = {}, bot1[kCols] = {};
        for (int i = 0; i < kRows; ++i) {
            const int y = ybase + i;
            if (y >= H) break;
            float v[kCols] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (tile_inside && y < d.oh) {
                int y0;
                float ty;
                index_lambda(fmaxf(source_index(sh, y), 0.0f), d.h, y0, ty);
                const int y1 = y0 + (y0 < d.h - 1 ? 1 : 0);
                if (y0 != held0) {
                    if (y0 == held1) {
#pragma unroll
                        for (int j = 0; j < kCols; ++j) top0[j] = bot0[j], top1[j] = bot1[j];
                    } else {
                        load_row(src + (int64_t)y0 * d.w, x0, x1, m, s, top0, top1);
                    }
                    held0 = y0;
                }
                if (y1 != held1) {
                    if (y1 == held0) {
#pragma unroll
                        for (int j = 0; j < kCols; ++j) bot0[j] = top0[j], bot1[j] = top1[j];
                    } else {
                        load_row(src + (int64_t)y1 * d.w, x0, x1, m, s, bot0, bot1);
                    }
                    held1 = y1;
                }
#pragma unroll
                for (int j = 0; j < kCols; ++j) v[j] = col[j] < d.ow ? blend_taps(top0[j], top1[j], bot0[j], bot1[j], ty, tx[j]) : 0.0f;
            }
            store_cols<OT, VEC>(batch, slot + c * plane + (int64_t)y * W, col, W, v);
        }
    }
}

inline bool extent_ok(int v) { return v >= 1 && v <= kMaxExtent; }

}  // namespace

extern "C" int edtr_det_transform(const edtr_det_image* descs_host, const edtr_det_image* descs, int N, int channels,
                                  const float* mean_host, const float* std_host, int out_dtype, void* batch, int H, int W,
                                  edtr_stream_t stream) {
    static_assert(kMaxChannels == EDTR_DET_MAX_CHANNELS && kMaxExtent == EDTR_DET_MAX_EXTENT && kTileW == EDTR_DET_TILE_W &&
                      kTileH == EDTR_DET_TILE_H,
                  "edtr_hip.h and det_transform.hip disagree on a constant");
    static_assert(sizeof(edtr_det_image) == 24, "edtr_det_image is 24 bytes");
    if (!descs_host || !descs || !mean_host || !std_host || !batch) return EDTR_E_NULL;
    if (N < 1 || N > 65535 || channels < 1 || channels > kMaxChannels || !extent_ok(H) || !extent_ok(W)) return EDTR_E_SHAPE;
    if (out_dtype != EDTR_LOGITS_F32 && out_dtype != EDTR_LOGITS_F16 && out_dtype != EDTR_LOGITS_BF16) return EDTR_E_DTYPE;
    NormArgs k = {};
    for (int c = 0; c < channels; ++c) {
        k.mean[c] = mean_host[c], k.std[c] = std_host[c];
        if (!(k.mean[c] == k.mean[c]) || !(k.std[c] == k.std[c]) || k.std[c] == 0.0f) return EDTR_E_SHAPE;
    }
    for (int i = 0; i < N; ++i) {
        const edtr_det_image& d = descs_host[i];
        if (!d.src) return EDTR_E_NULL;
        if (!extent_ok(d.h) || !extent_ok(d.w) || !extent_ok(d.oh) || !extent_ok(d.ow) || d.oh > H || d.ow > W) return EDTR_E_SHAPE;
        if (!aligned_to(d.src, 4)) return EDTR_E_ALIGN;
    }
    const uintptr_t elem = out_dtype == EDTR_LOGITS_F32 ? 4 : 2;
    if (!aligned_to(batch, elem) || !aligned_to(descs, 8)) return EDTR_E_ALIGN;

    const bool vec = W % 4 == 0 && aligned_to(batch, 4 * elem);
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define EDTR_DET_LAUNCH(OT)                                                                                                            \
    do {                                                                                                                               \
        if (vec) hipLaunchKernelGGL((det_transform_kernel<OT, true>), grid, block, 0, st, descs, channels, batch, H, W, tiles_x, k);   \
        else hipLaunchKernelGGL((det_transform_kernel<OT, false>), grid, block, 0, st, descs, channels, batch, H, W, tiles_x, k);      \
    } while (0)
    if (out_dtype == EDTR_LOGITS_F32) EDTR_DET_LAUNCH(EDTR_LOGITS_F32);
    else if (out_dtype == EDTR_LOGITS_F16) EDTR_DET_LAUNCH(EDTR_LOGITS_F16);
    else EDTR_DET_LAUNCH(EDTR_LOGITS_BF16);
#undef EDTR_DET_LAUNCH
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}
