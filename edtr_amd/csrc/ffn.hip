// edtr_ffn — the feed-forward half of a BasicTransformerBlock in ONE launch (see include/edtr_hip.h):
//     out = x + W2 . ( GEGLU( W1 . LayerNorm(x) + b1 ) ) + b2            reference model/attention.py:20-47, 232-233
// As two edtr_igemm launches (+ a LayerNorm launch at batch 8) the (rows, 4 d) hidden tensor makes a round trip through HBM —
// 84 MB written and read back at the 64 x 64 latent level, 34 us of memory time on its own — and both GEMMs are short-K launches
// whose prologue / GEGLU epilogue is as long as their loop (profiles/r05/stamps_short_linears.log).  Here a workgroup owns 128
// tokens for the whole hidden dimension and nothing but its tokens and the weights ever moves.
//
// Everything is computed TRANSPOSED so that the accumulator layout of one product is the operand layout of the next (the trick of
// attention.hip / swin.hip) and the token rows live in REGISTERS:
//   H^T[hidden][token] = W1 . X^T      A = W1 rows from LDS, B = this wave's 32 token rows (20 fragments, loaded once, normalised in place:
//                                       18 stay in registers, 2 are parked in LDS — the register file is full)
//   G = value * gelu(gate)              in the accumulators: lane = token, registers = hidden units; + the per-unit constant W1 beta + b1
//   O^T[out][token] += W2 . G^T        A = W2 rows from LDS, B = G packed to 16 bits — the accumulator registers 8 u .. 8 u + 7 of a
//                                       32 x 32 tile ARE the B fragment of k-step u once W2's columns are permuted inside every group
//                                       of 16 ([0-3, 8-11, 4-7, 12-15], done on the host: edtr_hip.h)
// Eight waves: wave (t, h) owns tokens 32 t .. 32 t + 31; in the first product it computes hidden half h of the chunk (32 gated
// units = a 32-row value tile and its gate tile: one lane holds a value and its gate), in the second product output half h (160
// columns = five 32 x 32 accumulators).  The two waves of a token tile swap their G fragments through 2 KiB of LDS per chunk.
// LDS holds only weights: 15 granules of 8 KiB (64 rows x 64 k, the XOR-swizzled tile of wave_prims.h) per 64-unit chunk — ten of
// W1 (k-tile kt, half h) and five of W2 (64 output rows each) — every granule type has a FIXED slot, refilled by LDS-DMA for the
// next chunk as soon as the step that read it is over (one dma per wave and granule: the counted vmcnt waits are uniform).
//
// Schedule of a chunk c (six steps, one barrier each; every wave issues the SAME sequence of DMAs, 16 per chunk):
//   step kt = 0 .. 4  first product, k-tile kt.  Refills issued between its MFMAs (their slots were freed by the barrier that opens the step):
//                       kt = 0: W2(c) x 5 (read five steps from now) + the constants of chunk c + 1;   kt >= 1: W1(c + 1, k-tile kt - 1) x 2
//   GEGLU             on the accumulators, G fragments to the exchange buffer
//   step B            second product (K = the chunk's 64 gated units); refill W1(c + 1, k-tile 4) x 2
// A step waits for the pieces it reads by counting what was issued AFTER them (loads complete in order):  kt = 0: vmcnt(8);
// kt = 1 .. 4: vmcnt(12);  B: vmcnt(9);  in the last chunk, where nothing is refilled: 8, 11, 9, 7, 5, 0.
#include "common.h"
#include "wave_prims.h"

namespace {

constexpr int FD = 320;                    // model width d
constexpr int FH = 1280;                   // gated hidden width 4 d
constexpr int FBM = 128;                   // tokens per workgroup
constexpr int FTHREADS = 512;
constexpr int FCH = 64;                    // gated hidden units per chunk (two halves of 32: a value tile + its gate tile per wave)
constexpr int FNCH = FH / FCH;             // 20 chunks
constexpr int GRAN = 8192;                 // one granule: 64 rows x 128 bytes
constexpr int NGRAN = 15;                  // per chunk: W1 (kt, h) at slot 2 kt + h, W2 rows 64 j .. at slot 10 + j
constexpr int RING = NGRAN * GRAN;
constexpr int XCH_OFF = RING;              // G fragments: [wave][k-step u] x 1 KiB (one buffer: a chunk's fragments are written behind the
constexpr int XCH = 8 * 2048;              //  barrier of its last k-tile, which every wave reaches after reading the previous chunk's)
constexpr int XFL = 2;                     // token fragments 20 - XFL .. 19 live in LDS, not in registers (the register file is full)
constexpr int XF_OFF = XCH_OFF + XCH;      // [wave][XFL] x 1 KiB
constexpr int CST_OFF = XF_OFF + 8 * XFL * 1024;     // per-unit constants of a chunk: [chunk parity][half][64 floats]
constexpr int CST = 2 * 2 * 256;
constexpr int FLDS = CST_OFF + CST;        // 156672 bytes
constexpr int OPITCH = 656;                // output tile row pitch in bytes (640 + 16: the 8-byte column writes of 32 rows spread over the banks)
static_assert(FLDS <= 160 * 1024 && FBM * OPITCH <= RING, "LDS budget");

// gelu from x / 2 over eight values as four PACKED fp32 pairs (v_pk_fma_f32 / v_pk_mul_f32: two values per instruction and lane): the
// GEGLU of a chunk is ~250 vector instructions per wave between two runs of MFMAs, with both waves of a SIMD in it at the same time —
// in the stamps it is as long as the chunk's matrix work.  Same arithmetic and order of operations as gelu_erf_lockstep<true>
// (common.h); v_exp / v_rcp stay per value.
__device__ __forceinline__ void pin4(f32x2 (&v)[4]) { asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])); }
__device__ __forceinline__ void gelu_half_in_pk(f32x2 (&h)[4]) {
    f32x2 d[4], u[4], poly[4], a[4];
    const f32x2 one = {1.0f, 1.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = f32x2{fabsf(h[i][0]), fabsf(h[i][1])};
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = a[i] * f32x2{0.3275911f * 1.41421356237309504880f, 0.3275911f * 1.41421356237309504880f} + one;
    pin4(d);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = f32x2{__builtin_amdgcn_rcpf(d[i][0]), __builtin_amdgcn_rcpf(d[i][1])};
    pin4(d);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = h[i] * h[i];
    pin4(u);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = u[i] * f32x2{-2.0f * 1.4426950408889634f, -2.0f * 1.4426950408889634f};
    pin4(u);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = f32x2{__builtin_amdgcn_exp2f(u[i][0]), __builtin_amdgcn_exp2f(u[i][1])};
    pin4(u);
#pragma unroll
    for (int i = 0; i < 4; ++i) poly[i] = d[i] * f32x2{1.061405429f, 1.061405429f} + f32x2{-1.453152027f, -1.453152027f};
    pin4(poly);
#pragma unroll
    for (int i = 0; i < 4; ++i) poly[i] = poly[i] * d[i] + f32x2{1.421413741f, 1.421413741f};
    pin4(poly);
#pragma unroll
    for (int i = 0; i < 4; ++i) poly[i] = poly[i] * d[i] + f32x2{-0.284496736f, -0.284496736f};
    pin4(poly);
#pragma unroll
    for (int i = 0; i < 4; ++i) poly[i] = poly[i] * d[i] + f32x2{0.254829592f, 0.254829592f};
    pin4(poly);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = u[i] * d[i];
    pin4(u);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = one - poly[i] * u[i];
    pin4(u);
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = a[i] * u[i] + h[i];
    pin4(h);
}

template <typename T, int HALF>
__device__ __forceinline__ void ffn_body(const edtr_ffn_params& p, char* smem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int t = wave & 3;
    constexpr int h = HALF;
    const int m0 = blockIdx.x * FBM;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));

    // ---- this wave's share of every granule: rows 8 wave .. 8 wave + 7, LDS slot (lane & 7) holds logical chunk slot ^ key(row)
    const int grow = 8 * wave + (lane >> 3);
    const int gchunk = (lane & 7) ^ ((grow >> 1) & 7);
    const uint32_t voff1 = (uint32_t)((grow * FD + 8 * gchunk) * 2);             // W1 [2 FH][FD]
    const uint32_t voff2 = (uint32_t)((grow * FH + 8 * gchunk) * 2);             // W2 [FD][FH]
    const u32x4 srd1 = make_srd(p.w1), srd2 = make_srd(p.w2);
    const uint32_t my_slot = lds0 + wave * 1024;
    auto issue_w1h = [&](int c, int kt, int hh) {          // half hh of k-tile kt of chunk c
        dma16_buf(voff1, srd1, (uint32_t)(((128 * c + 64 * hh) * FD + 64 * kt) * 2), my_slot + (2 * kt + hh) * GRAN);
    };
    auto issue_w1 = [&](int c, int kt) {
        issue_w1h(c, kt, 0);
        issue_w1h(c, kt, 1);
    };
    auto issue_w2j = [&](int c, int j) { dma16_buf(voff2, srd2, (uint32_t)((64 * j * FH + 64 * c) * 2), my_slot + (10 + j) * GRAN); };
    // constants of chunk c: 2 halves x 64 floats; every wave of half hw brings that half's 256 bytes (four waves bring the same
    // bytes: every wave issues ONE dma per chunk, which keeps the counted waits uniform)
    const u32x4 srdc = make_srd(p.cst);
    auto issue_cst = [&](int c) {
        int ln = lane;
        asm volatile("" : "+v"(ln));            // (re-derived per use: see the GEGLU section)
        dma4_buf((uint32_t)(ln * 4 + c * 512 + (wave >> 2) * 256), srdc, 0u, lds0 + CST_OFF + (c & 1) * 512 + (wave >> 2) * 256);
    };

    // ---- prologue: the token rows into registers (B fragments: lane = token l31, k = 16 s + 8 lh ..), first weights in flight
    U4 xf[20 - XFL];
    U4 xtail[XFL];
    {
        const uint16_t* xr = static_cast<const uint16_t*>(p.x) + (int64_t)(m0 + 32 * t + l31) * p.ldx + 8 * lh;
#pragma unroll
        for (int s = 0; s < 20 - XFL; ++s) xf[s] = ldg16(xr + 16 * s);
#pragma unroll
        for (int s = 0; s < XFL; ++s) xtail[s] = ldg16(xr + 16 * (20 - XFL + s));
    }
    issue_cst(0);
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) issue_w1(0, kt);

    // LayerNorm of this lane's token IN the registers (model/attention.py:224 norm3, eps 1e-5): two-pass statistics over the stored
    // 16-bit values, x <- (x - mean) rstd rounded to 16 bits — what the LayerNorm launch of the two-GEMM form hands its GEMM, minus
    // the affine part: gamma is folded into w1's columns, beta into the per-unit constants (edtr_hip.h).  The raw rows are read
    // again for the residual at the end.
    {
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 20; ++i) {
            float f[8];
            unpack8<T>(i < 20 - XFL ? xf[i < 20 - XFL ? i : 0] : xtail[i < 20 - XFL ? 0 : i - (20 - XFL)], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += f[j];
        }
        s += __shfl_xor(s, 32, 64);
        const float mean = s * (1.0f / FD);
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < 20; ++i) {
            float f[8];
            unpack8<T>(i < 20 - XFL ? xf[i < 20 - XFL ? i : 0] : xtail[i < 20 - XFL ? 0 : i - (20 - XFL)], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float dlt = f[j] - mean; q = __builtin_fmaf(dlt, dlt, q); }
        }
        q += __shfl_xor(q, 32, 64);
        const float rstd = __builtin_amdgcn_rsqf(q * (1.0f / FD) + p.eps);
        const float shift = -mean * rstd;
#pragma unroll
        for (int i = 0; i < 20; ++i) {
            float f[8];
            if (i < 20 - XFL) {
                unpack8<T>(xf[i < 20 - XFL ? i : 0], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = __builtin_fmaf(f[j], rstd, shift);
                xf[i < 20 - XFL ? i : 0] = pack8<T>(f);
            } else {
                unpack8<T>(xtail[i < 20 - XFL ? 0 : i - (20 - XFL)], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = __builtin_fmaf(f[j], rstd, shift);
                xtail[i < 20 - XFL ? 0 : i - (20 - XFL)] = pack8<T>(f);
            }
        }
#pragma unroll
        for (int i = 0; i < XFL; ++i) *reinterpret_cast<U4*>(smem + XF_OFF + (wave * XFL + i) * 1024 + lane * 16) = xtail[i];      // (own lanes only: no barrier needed)
    }

    f32x16 oacc[5];
#pragma unroll
    for (int b = 0; b < 5; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[b][r] = 0.0f;
#ifdef FFN_STAMPS       // diagnostic build (tools/exp/ffn_stamps.py): cycles per phase, written over the first output rows of the workgroup
    uint64_t st_t0 = __builtin_amdgcn_s_memtime(), st_last = st_t0, st_acc[6] = {0, 0, 0, 0, 0, 0};      // wait+barrier A | mfma A | geglu | wait+barrier B | mfma B | prologue
    st_acc[5] = 0;
#define FFN_STAMP(i) do { const uint64_t n__ = __builtin_amdgcn_s_memtime(); st_acc[i] += n__ - st_last; st_last = n__; } while (0)
#else
#define FFN_STAMP(i)
#endif

    const int arow = l31 * 128, akey = (l31 >> 1) & 7;        // fragment row l31 (and l31 + 32: same key) of a granule
    auto frag = [&](const char* gran, int row32, int c) {     // 16-byte chunk c of row row32 + l31
        return *reinterpret_cast<const U4*>(gran + row32 * 128 + arow + ((c ^ akey) << 4));
    };

    FFN_STAMP(5);
#pragma unroll 1
    for (int c = 0; c < FNCH; ++c) {
        const bool more = c + 1 < FNCH;
        f32x16 hv, hg;
#pragma unroll
        for (int r = 0; r < 16; ++r) { hv[r] = 0.0f; hg[r] = 0.0f; }

        // ---- first product: five k-tiles of 64
#pragma unroll
        for (int kt = 0; kt < 5; ++kt) {
            // this wave's pieces of k-tile kt have landed (counts: the DMAs issued after them — the schedule in the header comment)
            if (kt == 0) wait_vm<8>();
            else if (more) wait_vm<12>();
            else if (kt == 1) wait_vm<11>();
            else if (kt == 2) wait_vm<9>();
            else if (kt == 3) wait_vm<7>();
            else wait_vm<5>();
            block_sync();                                       // ... everyone's; the step before is over: its slots are free
            FFN_STAMP(0);
            const char* gran = smem + (2 * kt + h) * GRAN;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const U4 av = frag(gran, 0, 2 * ks + lh), ag = frag(gran, 32, 2 * ks + lh);
                constexpr int NR = 20 - XFL;
                const int si = 4 * kt + ks;
                U4 xb_;
                if (si < NR) {
                    xb_ = xf[si < NR ? si : 0];
                } else {
                    int ln = lane;
                    asm volatile("" : "+v"(ln));
                    xb_ = *reinterpret_cast<const U4*>(smem + XF_OFF + (wave * XFL + (si < NR ? 0 : si - NR)) * 1024 + ln * 16);
                }
                hv = T::mfma(av, xb_, hv);
                hg = T::mfma(ag, xb_, hg);
                // refills, spread between the MFMAs (a DMA issued behind queued matrix work costs the wave ~60 cycles of issue, six
                // in a row right behind the barrier held the matrix pipe empty): at k-tile 0 the chunk's W2 (needed five steps from now:
                // its slots are free since the barrier above) and the next chunk's constants, later the next chunk's W1 k-tile kt - 1
                if (kt == 0) {
                    if (ks < 2) { issue_w2j(c, 2 * ks); issue_w2j(c, 2 * ks + 1); }
                    else if (ks == 2) { issue_w2j(c, 4); if (more) issue_cst(c + 1); }
                } else if (more && ks < 2) {
                    issue_w1h(c + 1, kt - 1, ks);
                }
            }
            FFN_STAMP(1);
        }

        // ---- GEGLU: register r = 4 q + e is hidden unit e + 8 q + 4 lh of this wave's 32; + (W1 beta + b1), the gate's halved
        {
            int ln = lane;
            asm volatile("" : "+v"(ln));        // (addresses re-derived here: carried through the loop they spill, and a scratch reload drains the DMA queue)
            const float* cst = reinterpret_cast<const float*>(smem + CST_OFF + (c & 1) * 512 + h * 256) + 4 * (ln >> 5);
            char* mine = smem + XCH_OFF + wave * 2048 + ln * 16;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                f32x2 val[4], gate[4];
#pragma unroll
                for (int qq = 0; qq < 2; ++qq) {
                    const int q = 2 * u + qq;
                    const f32x4 c2v = *reinterpret_cast<const f32x4*>(cst + (q * 2 + 0) * 8);
                    const f32x4 c2g = *reinterpret_cast<const f32x4*>(cst + (q * 2 + 1) * 8);
#pragma unroll
                    for (int e2 = 0; e2 < 2; ++e2) {
                        val[2 * qq + e2] = f32x2{hv[4 * q + 2 * e2], hv[4 * q + 2 * e2 + 1]} + f32x2{c2v[2 * e2], c2v[2 * e2 + 1]};
                        gate[2 * qq + e2] = f32x2{hg[4 * q + 2 * e2], hg[4 * q + 2 * e2 + 1]} * f32x2{0.5f, 0.5f} + f32x2{c2g[2 * e2], c2g[2 * e2 + 1]};      // gate / 2
                    }
                }
                gelu_half_in_pk(gate);
                float out8[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x2 pr = val[e] * gate[e];
                    out8[2 * e] = pr[0];
                    out8[2 * e + 1] = pr[1];
                }
                *reinterpret_cast<U4*>(mine + u * 1024) = pack8<T>(out8);
            }
        }

        FFN_STAMP(2);
        // ---- second product: K = this chunk's 64 gated units (k-step 2 h' + u: half h', u = 0 / 1), five output tiles
        if (more) wait_vm<9>(); else wait_vm<0>();
        block_sync();                                           // W2 of the chunk everyone's; both halves' G fragments published
        FFN_STAMP(3);
        {
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const char* xb = smem + XCH_OFF + (wave & 3) * 2048 + ln * 16;      // wave t of half 0; + 8192: half 1
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const U4 g = *reinterpret_cast<const U4*>(xb + (ks >> 1) * 8192 + (ks & 1) * 1024);
#pragma unroll
                for (int b = 0; b < 5; ++b) {
                    const int gb = 5 * h + b;
                    const U4 a = frag(smem + (10 + (gb >> 1)) * GRAN, 32 * (gb & 1), 2 * ks + lh);
                    oacc[b] = T::mfma(a, g, oacc[b]);
                }
                if (more && ks < 2) issue_w1h(c + 1, 4, ks);
            }
        }
        FFN_STAMP(4);
    }

    // ---- epilogue: + bias + residual (the raw rows) in fp32, one rounding, through an LDS tile so that whole rows leave coalesced
    block_sync();                                               // every wave is done with the ring
    FFN_STAMP(3);
    {
        const uint16_t* xr = static_cast<const uint16_t*>(p.x) + (int64_t)(m0 + 32 * t + l31) * p.ldx;
        char* trow = smem + (32 * t + l31) * OPITCH;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            uint2 res[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) res[q] = *reinterpret_cast<const uint2*>(xr + 160 * h + 32 * b + 8 * q + 4 * lh);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = 160 * h + 32 * b + 8 * q + 4 * lh;
                const f32x4 bias = *reinterpret_cast<const f32x4*>(p.b2 + n);
                const float r0 = T::to_f32((uint16_t)(res[q].x & 0xffff)), r1 = T::to_f32((uint16_t)(res[q].x >> 16));
                const float r2 = T::to_f32((uint16_t)(res[q].y & 0xffff)), r3 = T::to_f32((uint16_t)(res[q].y >> 16));
                uint2 o;
                o.x = pack2<T>(oacc[b][4 * q + 0] + bias[0] + r0, oacc[b][4 * q + 1] + bias[1] + r1);
                o.y = pack2<T>(oacc[b][4 * q + 2] + bias[2] + r2, oacc[b][4 * q + 3] + bias[3] + r3);
                *reinterpret_cast<uint2*>(trow + n * 2) = o;
            }
        }
    }
    __syncthreads();
    {
        uint16_t* og = static_cast<uint16_t*>(p.out);
#pragma unroll
        for (int i = 0; i < (FBM * 40) / FTHREADS; ++i) {
            const int idx = tid + FTHREADS * i, row = idx / 40, ch = idx - row * 40;
            const U4 v = *reinterpret_cast<const U4*>(smem + row * OPITCH + ch * 16);
            stg16(og + (int64_t)(m0 + row) * p.ldo + ch * 8, v);
        }
    }
#ifdef FFN_STAMPS
    __syncthreads();
    if (lane == 0) {
        const uint64_t end = __builtin_amdgcn_s_memtime();
        uint64_t* dst = reinterpret_cast<uint64_t*>(static_cast<uint16_t*>(p.out) + (int64_t)(m0 + wave) * p.ldo);
        for (int i = 0; i < 6; ++i) dst[i] = st_acc[i];
        dst[6] = end - st_last;       // epilogue
        dst[7] = end - st_t0;
    }
#endif
}

template <typename T>
__global__ void __launch_bounds__(FTHREADS, 1) ffn320_kernel(const edtr_ffn_params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (threadIdx.x < 256) ffn_body<T, 0>(p, smem);
    else ffn_body<T, 1>(p, smem);
}

template <typename T>
int launch_ffn(const edtr_ffn_params& p, hipStream_t stream) {
    static EdtrLdsOnce attr_set;
    if (int rc_ = edtr_lds_attr(reinterpret_cast<const void*>(&ffn320_kernel<T>), FLDS, attr_set)) return rc_;
    hipLaunchKernelGGL((ffn320_kernel<T>), dim3(p.M / FBM), dim3(FTHREADS), FLDS, stream, p);
    EDTR_LAUNCH_CHECK();
    return EDTR_OK;
}

}  // namespace

static int ffn_check(const edtr_ffn_params* p) {
    if (!p) return EDTR_E_NULL;
    if (!p->x || !p->w1 || !p->w2 || !p->cst || !p->b2 || !p->out) return EDTR_E_NULL;
    if (p->dtype != EDTR_BF16 && p->dtype != EDTR_F16) return EDTR_E_DTYPE;
    if (p->M <= 0 || p->D <= 0 || p->H <= 0) return EDTR_E_SHAPE;
    if (p->D != FD || p->H != FH || p->M % FBM != 0) return EDTR_E_UNSUPPORTED;      // the caller issues the two edtr_igemm launches
    if ((p->ldx & 7) || (p->ldo & 7) || p->ldx < FD || p->ldo < FD) return EDTR_E_ALIGN;
    if (!aligned16(p->x) || !aligned16(p->w1) || !aligned16(p->w2) || !aligned16(p->cst) || !aligned16(p->b2) || !aligned16(p->out))
        return EDTR_E_ALIGN;
    if (p->x == p->out) return EDTR_E_UNSUPPORTED;              // (rows are re-read as the residual after other rows were stored)
    return EDTR_OK;
}

extern "C" int edtr_ffn(const edtr_ffn_params* p, edtr_stream_t stream) {
    if (int rc = ffn_check(p)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return p->dtype == EDTR_BF16 ? launch_ffn<BF16>(*p, s) : launch_ffn<F16>(*p, s);
}

// HIP-free: would edtr_ffn take these parameters?  (EDTR_OK or the error edtr_ffn would return)
extern "C" int edtr_ffn_plan(const edtr_ffn_params* p) { return ffn_check(p); }
