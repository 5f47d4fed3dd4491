// edtr_igemm's tile planner: which kernel runs for a set of parameters, or which error comes back.  Host code only — no HIP, nothing
// from common.h — so that edtr_igemm_plan answers without a device and tests/host/igemm_plan_main.cpp compiles it with a plain host
// compiler.  Three stages that run strictly one after another (plan(), at the end):
//   validate(p)        what depends on the parameters alone; normalises zdiv, splitk and an empty K tail
//   choose(p, ...)     the automatic tile for p.tile == 0; an explicit p.tile passes through
//   admit(p, tile, ..) the one place that says what each tile accepts: kTiles below, plus the rules that are no per-tile yes / no
// igemm.hip turns the resulting IgemmPlan into a launch and checks nothing more.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include "../../include/edtr_hip.h"

namespace igemm_plan {

constexpr int CK = 32;                          // channels per chunk of tiles 17 / 20 / 21 = K of one 16x16x32 MFMA
constexpr int64_t kBufferLimit = 0xF0000000LL;  // buffer-addressed operands: 32-bit byte offsets

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- environment switches (A/B measurements on ONE device: devices differ by several percent), all read once per process, on the
// first plan.  Three conventions: num = atoi of the value, else the stated default; off0 = on unless the value begins with '0';
// on1 = off unless it begins with '1'.
struct IgemmSwitches {
    int no_auto, halo512, halo512p, stagger_pct, debug_flags;
    bool halo, halo_ragged, skinny, halo160;
    static const IgemmSwitches& get() {
        static const IgemmSwitches sw = read();
        return sw;
    }
    static IgemmSwitches read() {
        auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
        auto off0 = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };
        auto on1 = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
        IgemmSwitches s;
        s.no_auto = num("EDTR_IGEMM_NO_AUTO", 0);           // bit i disables the automatic choice of tile i (6, 8); explicit p.tile requests are unaffected
        s.halo = off0("EDTR_IGEMM_HALO");                   // the automatic choice of tile 16 (and with it 17 / 21)
        s.halo_ragged = off0("EDTR_IGEMM_HALO_RAGGED");     // ... of tile 16 where 128-column tiles pad N
        s.skinny = off0("EDTR_IGEMM_SKINNY");               // ... of tile 14
        s.halo512 = num("EDTR_IGEMM_HALO512", 1);           // tile 17 replaces tile 16 from this many 512-pixel units per CU (<= 0: never)
        s.halo512p = num("EDTR_IGEMM_HALO512P", 0);         // tile 21 replaces tile 17 from this many units per CU (<= 0: never)
        s.halo160 = off0("EDTR_IGEMM_HALO160");             // the automatic choice of tile 20
        s.stagger_pct = num("EDTR_IGEMM_STAGGER", 0);       // percent of a workgroup's estimated half life (measured: no gain in isolation,
                                                            // the two workgroups of a CU are not slowed by their lockstep: off)
        s.debug_flags = (on1("EDTR_IGEMM_GENERAL_EPILOGUE") ? 1 : 0) | (on1("EDTR_IGEMM_N160_TWO_PASS") ? 2 : 0) |       // edtr_hip.h: debug_flags
                        (on1("EDTR_IGEMM_GEGLU_SERIAL") ? 4 : 0);
        return s;
    }
};

// ---- shape requirements of the halo tiles (buffer addressability is the planner's business: IgemmPlan::addressable)
// tile 16: four whole 8 x 8 images per workgroup (geometry 2 of the halo kernel)
static inline bool halo_img8(const edtr_igemm_params& p) {
    return !p.upsample2x && p.OH == 8 && p.OW == 8 && p.IH == 8 && p.IW == 8 && (p.M & 255) == 0;
}

static inline bool halo_ok(const edtr_igemm_params& p) {
    const int up = p.upsample2x ? 2 : 1;
    if (p.upsample2x == 2 && ((p.IH & 15) || (p.IW & 15) || p.w_phase_stride < (int64_t)p.N * p.ldw || p.ldw < 4 * p.C1)) return false;   // sub-pixel form: 16 x 16 source blocks
    return p.OH > 0 && p.taps == 9 && p.stride == 1 && p.pad_t == 1 && p.pad_l == 1 && p.C2 == 0 && (p.C1 & 63) == 0 &&
           p.OH == p.IH * up && p.OW == p.IW * up && (((p.OH & 15) == 0 && (p.OW & 15) == 0) || halo_img8(p)) && p.Z == 1 &&
           p.splitk <= p.C1 / 64 && p.act != EDTR_ACT_GEGLU && p.M == (p.M / (p.OH * p.OW)) * p.OH * p.OW;
}

// shape / option requirements of tile 17 (halo512.hip)
static inline bool edtr_halo512_ok(const edtr_igemm_params& p) {
    return p.OH > 0 && p.taps == 9 && p.stride == 1 && p.pad_t == 1 && p.pad_l == 1 && p.C2 == 0 && (p.C1 % CK) == 0 && !p.upsample2x &&
           p.OH == p.IH && p.OW == p.IW && (p.OH & 15) == 0 && (p.OW & 31) == 0 && p.Z == 1 && p.splitk <= 1 && p.act == EDTR_ACT_NONE &&
           !p.bias_m && (p.N & 127) == 0 && (p.n_valid == 0 || p.n_valid == p.N) && !p.vt_out && !p.row_stats && !p.ln_stats && !p.a_wrap &&
           p.M == (p.M / (p.OH * p.OW)) * p.OH * p.OW && (!p.rowvec || p.rows_per_image == p.OH * p.OW) &&
           (!p.residual || p.residual_f32 || (int64_t)p.M * p.ldr * 2 < 0xF0000000LL);      // (a 16-bit residual is fetched by buffer-addressed DMA)
}

// tile 21 = tile 17's shapes with a 16-bit output, no residual, no time-embedding row, an even number of 32-channel chunks
static inline bool edtr_halo512p_ok(const edtr_igemm_params& p) {
    return edtr_halo512_ok(p) && !p.out_f32 && !p.out16 && !p.residual && !p.rowvec && p.N <= 512 && ((p.C1 / CK) & 1) == 0 &&
           (int64_t)p.M * p.ldc * 2 < 0xF0000000LL;      // (the output is written by buffer-addressed stores)
}

// tile 20: 16 x 16-pixel units x 160 channels (no a_gn: the emitters fuse a GroupNorm input only into N <= 128 convolutions)
static inline bool edtr_halo160_ok(const edtr_igemm_params& p) {
    return p.OH > 0 && p.taps == 9 && p.stride == 1 && p.pad_t == 1 && p.pad_l == 1 && p.C2 == 0 && (p.C1 % CK) == 0 && !p.upsample2x &&
           p.OH == p.IH && p.OW == p.IW && (p.OH & 15) == 0 && (p.OW & 15) == 0 && p.Z == 1 && p.splitk <= 1 && p.act == EDTR_ACT_NONE &&
           !p.bias_m && p.N % 160 == 0 && (p.n_valid == 0 || p.n_valid == p.N) && !p.vt_out && !p.row_stats && !p.ln_stats && !p.a_wrap && !p.a_gn &&
           p.M == (p.M / (p.OH * p.OW)) * p.OH * p.OW && (!p.rowvec || p.rows_per_image == p.OH * p.OW);
}

// ---- the live tiles and what each accepts.  4, 5, 7, 9 - 13, 15, 18, 19 were experiments, measured (profiles/r01 - r03) and removed
// (15 = the 8-wave ping-pong 128x128 tile for small grids and 18 = the persistent halo tile were faster in isolation and neutral on
// the whole path: round 4 took them out): EDTR_E_DTYPE.
struct TileTraits {
    int tile, bn;                 // tile number; columns of N per workgroup
    bool chunk32;                 // the LDS-DMA main loop (every tile from 3 up has one) walks 32-channel chunks, not 64-wide K-tiles
    bool fast;                    // only the buffer-addressed fast path exists (32-bit byte offsets cover the A and W operands)
    bool splitk, geglu, vt_out, row_stats, ln_stats, a3, a_gn, a_wrap;
    bool gn_partial;              // the tile's epilogue writes the statistics (with split-K the reducer does: admit)
    bool (*shape_ok)(const edtr_igemm_params&);      // the halo tiles' own predicate
};
constexpr TileTraits kTiles[] = {
    //     bn  ck32 fast  splitk geglu vt  rowst lnst  a3  a_gn wrap gnp
    {1,   128, 0,   0,    1,     1,    1,  1,    1,    0,  0,   1,   1,  nullptr},            // 128x128 register-staged
    {2,    64, 0,   0,    1,     1,    0,  1,    0,    0,  0,   1,   0,  nullptr},            // 64x64 register-staged (GEGLU: runs as tile 1, plan())
    {3,   128, 0,   0,    1,     1,    1,  1,    1,    0,  0,   1,   1,  nullptr},            // 128x128 LDS-DMA
    {6,   256, 0,   1,    0,     0,    0,  0,    0,    0,  0,   0,   1,  nullptr},            // 256x256 ping-pong
    {8,   160, 0,   1,    1,     0,    1,  1,    0,    0,  0,   1,   1,  nullptr},            // 128x160 (row_stats: not with the two-pass epilogue, debug_flags bit 1)
    {14,   32, 0,   1,    1,     0,    0,  0,    0,    0,  0,   0,   0,  nullptr},            // 256x32 for skinny N
    {16,  128, 0,   0,    1,     0,    0,  0,    0,    1,  1,   0,   1,  halo_ok},            // halo, 16 x 16-pixel patches in five geometries (a3: not together with a_gn)
    {17,  128, 1,   0,    0,     0,    0,  0,    0,    1,  1,   0,   1,  edtr_halo512_ok},    // halo, 32 x 16-pixel units (halo512.hip)
    {20,  160, 1,   0,    0,     0,    0,  0,    0,    1,  0,   0,   1,  edtr_halo160_ok},    // halo, 16 x 16 pixels x 160 channels (halo512.hip)
    {21,  128, 1,   0,    0,     0,    0,  0,    0,    0,  1,   0,   1,  edtr_halo512p_ok},   // tile 17 as a persistent kernel with deferred stores (halo512.hip)
    // an unknown number: refused by every feature that names its tiles, else EDTR_E_DTYPE (behind gn_partial's own checks, as ever)
    {0,   128, 0,   0,    1,     1,    0,  0,    0,    0,  0,   0,   1,  nullptr},
};
constexpr int kTileRow[22] = {10, 0, 1, 2, 10, 10, 3, 10, 4, 10, 10, 10, 10, 10, 5, 10, 6, 7, 10, 10, 8, 9};      // tile number -> row of kTiles
static inline const TileTraits& traits(int tile) { return kTiles[(unsigned)tile < 22u ? kTileRow[tile] : 10]; }
constexpr bool tile_rows_match(int t = 0) { return t == 22 || (kTiles[kTileRow[t]].tile == (kTileRow[t] < 10 ? t : 0) && tile_rows_match(t + 1)); }
static_assert(tile_rows_match() && kTileRow[21] == 9, "kTileRow names the row of every live tile, and row 10 for every other number");

struct IgemmPlan {
    int rc;                 // > 0: the tile; < 0: the error
    bool spatial;           // OH > 0: A is an image, not a row-major matrix
    bool dma_ok;            // C2 == 0 and C1 % 64 == 0: every 64-wide K-tile lies inside one tap of one source
    bool addressable;       // igemm_fast_addressable, evaluated once
    bool fast;              // the chosen tile runs its buffer-addressed fast path (tiles 3 - 14)
    int halo_geo;           // tile 16: 0 plain, 1 nearest-2x gather, 2 four 8 x 8 images per workgroup, 3 sub-pixel upsample, 4 K tail
    edtr_igemm_params p;    // normalised, with stagger and debug_flags filled in
};
// the fast path of tiles 3 - 14 gathers a nearest-2x upsampled source at stride 1 only (tiles 3, 6, 8, 14)
static inline bool fast_path(const edtr_igemm_params& p, int tile, const IgemmPlan& f) {
    return (!p.upsample2x || (p.stride == 1 && (tile == 3 || tile >= 6))) && f.addressable;
}
// buffer-addressed fast path: 32-bit byte offsets must cover the A and W operands (per z slice).  Evaluated once per plan.
static inline bool igemm_fast_addressable(const edtr_igemm_params& p, bool spatial) {
    const int64_t a_rows = spatial ? (int64_t)(p.M / (p.OH * p.OW)) * p.IH * p.IW : p.M;
    const int64_t a_bytes = (a_rows + (spatial ? 3 * (int64_t)p.IW + 3 : 0)) * p.ld1 * 2 + (int64_t)p.K * 2;
    const int64_t w_bytes = (int64_t)p.N * p.ldw * 2 + (int64_t)p.K * 2;
    return a_bytes < kBufferLimit && w_bytes < kBufferLimit;
}
// tile 8 writes row statistics from its one-pass epilogue only (two passes: debug_flags bit 1)
static inline bool takes_row_stats(int tile, const IgemmPlan& f) { return traits(tile).row_stats && !(tile == 8 && (f.p.debug_flags & 2)); }

// ---- stage 1: the parameters alone.  The order of the checks is the error code of an input that breaks several rules.
static inline int validate(IgemmPlan& f) {
    edtr_igemm_params& p = f.p;
    if (!p.a1 || !p.w || !p.out) return EDTR_E_NULL;
    if (p.dtype != EDTR_BF16 && p.dtype != EDTR_F16) return EDTR_E_DTYPE;
    if (p.taps != 1 && p.taps != 9) return EDTR_E_UNSUPPORTED;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.Z <= 0) return EDTR_E_SHAPE;
    if (p.zdiv <= 0) p.zdiv = 1;
    if (p.C2 > 0 && !p.a2) return EDTR_E_NULL;
    if (p.C2 < 0 || p.C1 <= 0) return EDTR_E_SHAPE;
    if (!p.a3 || p.C3 == 0) { p.a3 = nullptr; p.C3 = 0; p.ld3 = 0; }     // no K tail
    if (p.C3 < 0) return EDTR_E_SHAPE;
    if (p.K != p.taps * (p.C1 + p.C2) + p.C3) return EDTR_E_SHAPE;
    const bool spatial = p.OH > 0;
    if (p.a3) {     // K tail: the halo tiles' plain 3x3 / stride 1 / pad 1 geometry only (which tile: admit)
        if (p.taps != 9 || !spatial || p.stride != 1 || p.pad_t != 1 || p.pad_l != 1 || p.upsample2x || p.C2 != 0 || (p.C3 & 63) ||
            (p.C1 & 63) || p.a_wrap != 0 || p.Z != 1 || p.act == EDTR_ACT_GEGLU)
            return EDTR_E_UNSUPPORTED;
        if (p.ld3 < p.C3 || p.ldw < p.K) return EDTR_E_SHAPE;
        if ((p.ld3 & 7) || !aligned16(p.a3)) return EDTR_E_ALIGN;
        if (((int64_t)p.M * p.ld3 + p.C3) * 2 >= kBufferLimit) return EDTR_E_UNSUPPORTED;    // 32-bit buffer offsets
    }
    if (p.taps == 9 && !spatial) return EDTR_E_SHAPE;
    if (spatial) {
        if (p.OW <= 0 || p.IH <= 0 || p.IW <= 0 || p.stride <= 0) return EDTR_E_SHAPE;
        if (p.M % (p.OH * p.OW) != 0) return EDTR_E_SHAPE;
    }
    if (p.upsample2x < 0 || p.upsample2x > 2) return EDTR_E_SHAPE;
    if (p.act < EDTR_ACT_NONE || p.act > EDTR_ACT_LRELU) return EDTR_E_DTYPE;
    if (p.act == EDTR_ACT_LRELU && !(p.act_slope >= 0.0f && p.act_slope <= 1.0f)) return EDTR_E_SHAPE;
    if (p.rowvec && p.rows_per_image <= 0) return EDTR_E_SHAPE;
    // 16-byte rule
    if ((p.K & 7) || (p.N & 7) || (p.C1 & 7) || (p.C2 & 7) || (p.ld1 & 7) || (p.C2 && (p.ld2 & 7)) || (p.ldw & 7))
        return EDTR_E_ALIGN;
    const int n_out = p.act == EDTR_ACT_GEGLU ? p.N / 2 : p.N;
    if (p.act == EDTR_ACT_GEGLU && (p.N & 63)) return EDTR_E_ALIGN;
    if ((n_out & 7) || (p.ldc & (p.out_f32 ? 3 : 7)) || (p.residual && (p.ldr & (p.residual_f32 ? 3 : 7)))) return EDTR_E_ALIGN;
    if (!aligned16(p.a1) || !aligned16(p.w) || !aligned16(p.out) || (p.a2 && !aligned16(p.a2)) ||
        (p.residual && !aligned16(p.residual)))
        return EDTR_E_ALIGN;
    if ((p.a_zs_outer & 7) || (p.a_zs_inner & 7) || (p.w_zs_outer & 7) || (p.w_zs_inner & 7) ||
        (p.o_zs_outer & 3) || (p.o_zs_inner & 3))
        return EDTR_E_ALIGN;
    // the epilogue reads bias / time-embedding rows as 16-byte vectors
    if ((p.bias_n && !aligned16(p.bias_n)) || (p.rowvec && (!aligned16(p.rowvec) || (p.rowvec_ld & 3)))) return EDTR_E_ALIGN;
    if (p.n_valid < 0 || p.n_valid > p.N) return EDTR_E_SHAPE;
    if (p.residual && p.Z != 1) return EDTR_E_UNSUPPORTED;  // residual / rowvec are not z-batched
    if (p.rowvec && p.Z != 1) return EDTR_E_UNSUPPORTED;
    if (p.splitk < 0) return EDTR_E_SHAPE;
    if (p.splitk <= 1) p.splitk = 1;
    if (p.splitk > 1) {
        if (p.Z != 1 || p.act == EDTR_ACT_GEGLU) return EDTR_E_UNSUPPORTED;
        if (!p.workspace) return EDTR_E_NULL;
        if (p.workspace_bytes < (int64_t)p.splitk * p.M * p.N * 4 || !aligned16(p.workspace)) return EDTR_E_SHAPE;
        if (p.splitk > (p.K + 63) / 64) return EDTR_E_SHAPE;
    }
    if (p.vt_out) {
        if (p.Z != 1 || p.splitk > 1 || p.act == EDTR_ACT_GEGLU || p.residual || p.rowvec || p.gn_partial || p.out_f32 || spatial)
            return EDTR_E_UNSUPPORTED;
        if (p.rows_per_image <= 0 || (p.rows_per_image & 7) || (p.M & 7) || p.vt_col0 <= 0 || p.vt_col0 >= p.N) return EDTR_E_SHAPE;
        if ((p.vt_ld & 7) || p.vt_ld < p.rows_per_image || !aligned16(p.vt_out)) return EDTR_E_ALIGN;
    }
    if (p.row_stats) {
        if (p.Z != 1 || p.splitk > 1 || p.act == EDTR_ACT_GEGLU || p.vt_out) return EDTR_E_UNSUPPORTED;
        if (p.N & 31) return EDTR_E_SHAPE;
        if (!aligned16(p.row_stats)) return EDTR_E_ALIGN;
    }
    if (p.ln_stats) {
        if (p.Z != 1 || p.splitk > 1 || p.taps != 1 || spatial || p.C2) return EDTR_E_UNSUPPORTED;
        if (!p.ln_c1 || !p.ln_c2) return EDTR_E_NULL;
        // ln_C = the number of REAL columns the statistics run over (SwinIR keeps 180 channels in rows of 192 whose pad columns are
        // exactly zero: they add nothing to the slots); the slots cover the K = ln_slots * 32 stored columns
        if (p.ln_slots <= 0 || p.ln_slots * 32 != p.K || p.ln_C <= 0 || p.ln_C > p.K) return EDTR_E_SHAPE;
        if (!aligned16(p.ln_stats) || !aligned16(p.ln_c1) || !aligned16(p.ln_c2)) return EDTR_E_ALIGN;
    }
    f.spatial = spatial;
    f.dma_ok = p.C2 == 0 && (p.C1 & 63) == 0;
    f.addressable = igemm_fast_addressable(p, spatial);
    return EDTR_OK;
}

// ---- stage 2: the automatic choice, a cascade in which a later rule overrides an earlier one.  `cus` = the CUs of the device the
// launch goes to (whole-round rules).  Refuses nothing: what the chosen tile cannot take, admit() refuses.
static inline int choose(const edtr_igemm_params& p, const IgemmPlan& f, int cus, const IgemmSwitches& sw) {
    if (p.tile != 0) return p.tile;
    const bool dma_ok = f.dma_ok, addr = f.addressable;
    const int ksel = p.K - p.C3;      // the 9-tap product: a K tail does not move a convolution to another tile
    // base: the LDS-DMA kernel wherever it applies
    const int64_t big = (int64_t)((p.M + 127) / 128) * ((p.N + 127) / 128) * p.Z;
    int tile = dma_ok ? 3 : (big >= 200 ? 1 : 2);
    const bool pp_ok = dma_ok && p.splitk <= 1 && p.act != EDTR_ACT_GEGLU && (!p.upsample2x || p.stride == 1) && addr;
    // 128x160 tile: the SD UNet widths 320 / 640 / 1280 are multiples of 160 (no padded columns; N = 320 at M = 32768 is
    // one resident round).  Measured faster than the 128-wide grid whenever >= 200 tiles exist, except the
    // short-K GEMMs whose N the 128-wide grid also divides (two-pass epilogue).
    const int64_t nb160 = (int64_t)((p.M + 127) / 128) * (p.N / 160) * p.Z;
    // 256x256 ping-pong kernel: large-K convolutions whose 256-column tiles are mostly full and fill >= half the CUs
    // (measured on MI355X: 1.17-1.32 PFLOP/s vs 0.98-1.05 for the 128x128 loop on the VAE convolutions)
    const int nbn256 = (p.N + 255) / 256;
    const int64_t nb256 = (int64_t)((p.M + 255) / 256) * nbn256 * p.Z;
    if (pp_ok && !(sw.no_auto & (1 << 8)) && p.N % 160 == 0 && nb160 >= 200 && (p.N % 128 != 0 || ksel >= 640))
        tile = 8;
    else if (pp_ok && !(sw.no_auto & (1 << 6)) && ksel >= 1024 && nb256 >= 120 && p.N * 5 >= nbn256 * 256 * 4)
        tile = 6;
    // Halo tile: 3x3 / stride 1 convolutions on 16-pixel-aligned images.  Measured on the MI355X against the tile chosen above
    // (profiles/r02/halo_tile_experiments.log): 1.16-1.27x over the 128x128 loop on the N = 128 convolutions of the VAE's 512x512
    // level, 1.03-1.13x over the 256x256 ping-pong on its 256 / 128 / 64-pixel levels, 1.39x over the 128x160 tile at 640
    // channels; NOT where 128-column tiles pad N (N = 320: the 160-column tile wins) or with fewer than 48 units
    // (16x16-pixel patches x 128-column tiles; measured: 1.3-1.4x over the 128x160 tile at 80 units, 1.04-1.29x at 64, equal at 32).
    if (sw.halo && dma_ok && addr && halo_ok(p)) {
        const int64_t units = (int64_t)(p.M >> 8) * ((p.N + 127) >> 7);
        if ((p.N & 127) == 0 && units * p.splitk >= 48) tile = 16;
        // ... and where they DO pad N (N = 320 = 2.5 tiles) as long as the padded grid is at most ONE round of workgroups: the
        // 64x64-latent convolutions at batch <= 4 (192 units), where the 128x160 tile's 256 workgroups crawl alone on their CUs.
        // Measured (profiles/r03/halo_n320.log, one device): 37.0 / 63.1 / 88.9 us against 51.8 / 92.6 / 133.8 (K = 2880 / 5760 /
        // 8640, batch 4: 1.40 - 1.50x), 33.1 against 48.7 at batch 2; at batch 8 (384 units = 1.5 rounds) the 128x160 tile wins by 8 %.
        if (sw.halo_ragged && (p.N & 127) != 0 && p.N > 128 && p.splitk <= 1 && units >= 48 && units <= 256) tile = 16;
    }
    // 256x32 tile for skinny-N convolutions (the VAE decoder's 3-channel output conv: 94 % of a 128-wide tile is padding);
    // validated against tile 3 on the MI355X (profiles/r02/ab_tiles_3_vs_14*.log)
    if (sw.skinny && tile == 3 && p.N <= 32 && p.M >= 65536 && p.splitk <= 1 && !p.gn_partial && p.act != EDTR_ACT_GEGLU &&
        (!p.upsample2x || p.stride == 1) && addr)
        tile = 14;
    // promotions.  16 -> 17: the plain 3x3 / stride-1 convolutions whose image is a multiple of 32 x 16 pixels (edtr_halo512_ok),
    // wherever there are `halo512` units of 512 pixels per CU; 17 -> 21 likewise from `halo512p` units per CU (A/B runs only)
    const int64_t units512 = (int64_t)(p.M >> 9) * (p.N >> 7);
    if (tile == 16 && sw.halo512 > 0 && units512 >= (int64_t)cus * sw.halo512 && edtr_halo512_ok(p)) tile = 17;
    if (tile == 17 && sw.halo512p > 0 && units512 >= (int64_t)cus * sw.halo512p && edtr_halo512p_ok(p)) tile = 21;
    // 8 -> 20: N % 160 == 0 convolutions whose 16 x 16-pixel x 160-channel units fill whole rounds of the chip (the 64 x 64-latent
    // ResBlock convolutions at batch 8: 256 units = one per CU)
    if (tile == 8 && sw.halo160 && addr && edtr_halo160_ok(p)) {
        const int64_t units = (int64_t)(p.M >> 8) * (p.N / 160), tail = units % cus, most = (int64_t)cus * 3 / 4;
        if (units >= most && (tail == 0 || tail >= most)) tile = 20;       // whole rounds of one unit per CU (the last one >= 3/4 full)
    }
    // features that only some tiles implement move the choice to one that does
    if (p.a_gn && tile != 17 && tile != 21) tile = 16;        // GroupNorm (+ SiLU) of the input in the halo tiles' patch staging
    if (p.a_wrap != 0 && !traits(tile).a_wrap) tile = 3;      // (an automatic 256x256 / ping-pong choice)
    if (p.upsample2x == 2) tile = 16;                         // sub-pixel form of the upsample convolution: phase-major pre-summed weights
    if (p.vt_out && !(traits(tile).vt_out && p.vt_col0 % traits(tile).bn == 0))      // the transposed V store needs whole column tiles of V
        tile = (dma_ok && p.N % 160 == 0 && p.vt_col0 % 160 == 0 && addr) ? 8 : (dma_ok ? 3 : 1);
    if (p.ln_stats && !traits(tile).ln_stats) tile = dma_ok ? 3 : 1;      // the folded LayerNorm's epilogue exists in the 128 x 128 tiles only
    if (p.row_stats && !takes_row_stats(tile, f)) tile = dma_ok ? 3 : 1;
    return tile;
}

// ---- stage 3: what the tile accepts.  Errors in the order they have always had: a_gn and out16 report a misaligned pointer only
// behind the refusals of the tile itself, gn_partial a bad slot stride before them.
// the LDS-DMA main loops (every tile from 3 up) need every 64-wide K-tile inside one tap of one source; tiles 17 / 20 / 21 walk 32-channel chunks
static inline bool chunks_ok(const edtr_igemm_params& p, int tile, const IgemmPlan& f) {
    return tile < 3 || f.dma_ok || (traits(tile).chunk32 && p.C2 == 0 && (p.C1 & 31) == 0);
}
// the main loop's own requirements
static inline bool loop_ok(const edtr_igemm_params& p, int tile, const IgemmPlan& f) {
    const TileTraits& t = traits(tile);
    return (!t.fast || fast_path(p, tile, f)) && (t.splitk || p.splitk <= 1) && (t.geglu || p.act != EDTR_ACT_GEGLU) &&
           (!t.shape_ok || (t.shape_ok(p) && f.addressable));
}

static inline int admit(const edtr_igemm_params& p, int tile, const IgemmPlan& f) {
    const TileTraits& t = traits(tile);
    const bool chunks = chunks_ok(p, tile, f), loop = loop_ok(p, tile, f);
    // Kept as found, not endorsed: on the automatic path the fallbacks of a_wrap and row_stats to tile 3 / 1 come AFTER a_gn or the
    // sub-pixel form has forced tile 16, and those two are judged on that tile 16.  a_wrap refuses a convolution anyway; with
    // row_stats the fallback tile runs and applies neither.  No emitter combines them; refusing changes an answer and belongs
    // in a change of its own.
    const int halo = (p.tile == 0 && (p.a_gn || p.upsample2x == 2) && tile < 16) ? 16 : tile;
    const bool halo_takes = halo == tile ? chunks && loop : chunks_ok(p, 16, f) && loop_ok(p, 16, f);
    if (p.a_gn) {           // 16 x 16 / 32 x 16-patch geometries only: not the upsampled or the 8 x 8-image form of tile 16
        if (!traits(halo).a_gn || !halo_takes || (halo == 16 && (p.upsample2x || halo_img8(p)))) return EDTR_E_UNSUPPORTED;
        if (!aligned16(p.a_gn)) return EDTR_E_ALIGN;
    }
    if (p.out16) {
        if (!p.out_f32 || p.Z != 1 || p.act == EDTR_ACT_GEGLU || p.vt_out) return EDTR_E_UNSUPPORTED;
        if ((p.ld16 & 7) || !aligned16(p.out16)) return EDTR_E_ALIGN;
    }
    if (p.a_wrap != 0) {    // weights-exact two-part product: A[m][k mod a_wrap] against [Wh | Wl]; plain GEMMs
        if (p.a_wrap < 0 || p.K != 2 * p.a_wrap || (p.a_wrap & 63) || f.spatial || p.taps != 1 || p.C2 || p.Z != 1 || p.ln_stats) return EDTR_E_UNSUPPORTED;
        if (!t.a_wrap) return EDTR_E_UNSUPPORTED;
    }
    if (p.upsample2x == 2 && (halo != 16 || !halo_takes)) return EDTR_E_UNSUPPORTED;       // sub-pixel form: the halo kernel only
    if (p.vt_out && (!t.vt_out || p.vt_col0 % t.bn != 0)) return EDTR_E_UNSUPPORTED;
    if (p.ln_stats && !t.ln_stats) return EDTR_E_UNSUPPORTED;
    if (p.row_stats && !takes_row_stats(tile, f)) return EDTR_E_UNSUPPORTED;
    if (!chunks) return EDTR_E_UNSUPPORTED;
    if (p.a3 && !(t.a3 && !(tile == 16 && p.a_gn))) return EDTR_E_UNSUPPORTED;       // (tile 16 normalises no tail operand apart)
    if (p.gn_partial) {
        const int sr = p.gn_slot_rows > 0 ? p.gn_slot_rows : 128;
        if (p.gn_ld < 0 || (p.gn_ld > 0 && p.gn_ld < p.N)) return EDTR_E_SHAPE;
        if (p.Z != 1 || p.act == EDTR_ACT_GEGLU) return EDTR_E_UNSUPPORTED;
        // with split-K the reducer writes the statistics, in slots of 128 rows or of 64 (the 8 x 8 images), behind every tile but 14;
        // without, the tile's epilogue does: whole 128-row tiles of the 128-row kernels
        if (p.splitk > 1 ? (tile == 14 || (sr != 64 && sr != 128) || p.M % sr || (p.N & 31)) : (!t.gn_partial || sr != 128 || (p.M & 127)))
            return EDTR_E_UNSUPPORTED;
    }
    if (t.tile == 0) return EDTR_E_DTYPE;
    return loop ? EDTR_OK : EDTR_E_UNSUPPORTED;
}

static inline IgemmPlan plan(const edtr_igemm_params* pp, int cus) {
    IgemmPlan pl;
    pl.spatial = pl.dma_ok = pl.addressable = pl.fast = false;
    pl.halo_geo = 0;
    if (!pp) { pl.p = {}; pl.rc = EDTR_E_NULL; return pl; }
    const IgemmSwitches& sw = IgemmSwitches::get();
    edtr_igemm_params& p = pl.p = *pp;
    p.debug_flags = sw.debug_flags;
    p.stagger = 0;
    if ((pl.rc = validate(pl)) != EDTR_OK) return pl;
    int tile = choose(p, pl, cus, sw);
    if ((pl.rc = admit(p, tile, pl)) != EDTR_OK) return pl;
    if (p.act == EDTR_ACT_GEGLU && tile == 2) tile = 1;       // value/gate pairing needs two 32-column MFMA tiles per wave
    pl.rc = tile;
    pl.fast = fast_path(p, tile, pl);
    pl.halo_geo = halo_img8(p) ? 2 : p.upsample2x == 2 ? 3 : p.a3 ? 4 : p.upsample2x ? 1 : 0;
    // lockstep breaker of the two-workgroups-per-CU kernels (stagger_second_slot): only when the grid has more than one round
    // (>= 768 workgroups: below that the second slot's blocks are the tail anyway) and the tile is short enough for the epilogue
    // to matter.  Off unless EDTR_IGEMM_STAGGER asks for it.
    const int nkt = (p.K + 63) / 64, bn = tile == 8 ? 160 : 128;
    if (sw.stagger_pct > 0 && (tile == 3 || tile == 8) && p.splitk <= 1 && nkt <= 48 &&
        (int64_t)((p.M + 127) / 128) * ((p.N + bn - 1) / bn) * p.Z >= 768) {
        const int life = 4000 + nkt * 1350 + (p.act == EDTR_ACT_GEGLU ? 11000 : 9000);      // cycles, from the in-kernel stamps
        p.stagger = (int)((int64_t)life * sw.stagger_pct / 200);
    }
    return pl;
}

}  // namespace igemm_plan
