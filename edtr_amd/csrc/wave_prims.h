// Inline-asm and LDS-layout primitives of the hand-written MFMA kernels (igemm, halo512, attention, attn512, swin, ffn, lin320):
// LDS-DMA, buffer descriptors, counted waits, the barrier triple, swizzle keys.  Each is defined here once; the glue units
// (glue.h -> common.h) never see them.
#pragma once
#include "common.h"

// Byte offset of 16-byte chunk `c` of row `r` in a [rows][64 x 16-bit] LDS tile (128-byte rows).
// XOR swizzle so that the 16 lanes of every ds_read_b128 lane group (rows r..r+15 pattern of the
// MFMA operand read, chunk fixed) hit 16 distinct 16-byte bank slots of the 256-byte bank row.
__device__ __forceinline__ int tile_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

// 2-bit XOR key of a 64-byte LDS row (a patch pixel or a weight row), by row index mod 8: {3, 3, 0, 1, 0, 1, 3, 2}
// (halo512.hip: conflict-free ds_read_b128 of 16 consecutive 64-byte rows)
__device__ __forceinline__ int key8(int x) {
    constexpr uint32_t kKey = 3u | (3u << 2) | (0u << 4) | (1u << 6) | (0u << 8) | (1u << 10) | (3u << 12) | (2u << 14);
    return (int)((kKey >> (2 * (x & 7))) & 3u);
}

// bits 2,3 of a row index swapped (attention.hip: the row order that makes a score accumulator the next MFMA's B operand)
__device__ __forceinline__ int swap23(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }

// sum over the 16 lanes of a DPP row (lanes that share lane >> 4), result in every lane: four v_add_f32 with DPP operands
// (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror) instead of four ds_bpermute round trips
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

// One global_load_lds_dwordx4: lane i's 16 bytes land at LDS byte address lds_addr + 16*i (lds_addr wave-uniform, in
// M0).  Inline asm on purpose: hipcc neither counts it in its own vmcnt bookkeeping nor serialises later ds_reads
// behind it with a vmcnt(0), so the prefetch can stay in flight across the barrier; completion is waited for by
// the hand-placed counted s_waitcnt in the main loop.
__device__ __forceinline__ void dma16(const void* gsrc, uint32_t lds_addr) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_addr)
                 : "memory");
}

__device__ __forceinline__ uint32_t lds_addr_of(const char* p) {
    return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) char*)p);
}

// Buffer-addressed LDS-DMA: address = SRD base + voff (per lane) + soff (wave uniform); lanes whose voff fails the
// descriptor's range check write zeros.
constexpr uint32_t kOobOffset = 0xFFFFFF00u;     // >= num_records - 15 -> always out of range
constexpr uint32_t kNumRecords = 0xFFFFFF00u;

__device__ __forceinline__ u32x4 make_srd(const void* base) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    u32x4 srd;
    srd.x = __builtin_amdgcn_readfirstlane((uint32_t)b);
    srd.y = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32) & 0xffffu);   // stride 0 (raw buffer)
    srd.z = kNumRecords;
    srd.w = 0x00020000u;
    return srd;
}

// lane i's 16 bytes (SRD base + voff + soff) land at LDS byte lds_addr + 16 i
__device__ __forceinline__ void dma16_buf(uint32_t voff, const u32x4& srd, uint32_t soff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 :
                 : "v"(voff), "s"(srd), "s"(lds_addr), "s"(soff)
                 : "memory");   // M0 is free here: hipcc keeps no value in it across statements on gfx950
}
// dma16_buf that saves and restores M0 (attention.hip): two more scalar moves, kept because the change that gathered these
// helpers alters no kernel
__device__ __forceinline__ void dma16_buf_keep_m0(uint32_t voff, const u32x4& srd, uint32_t soff, uint32_t lds_addr) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(srd), "s"(lds_addr), "s"(soff)
                 : "memory");
}
// one buffer_load_dword ... lds: lane i's 4 bytes land at lds_addr + 4 i (buffer-addressed like dma16_buf: one 32-bit offset per lane,
// the chunk moves the scalar offset — no 64-bit pointer to carry through the loop)
__device__ __forceinline__ void dma4_buf(uint32_t voff, const u32x4& srd, uint32_t soff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dword %0, %1, %3 offen lds"
                 :
                 : "v"(voff), "s"(srd), "s"(lds_addr), "s"(soff)
                 : "memory");
}

// Counted wait: at most N of this wave's vector-memory operations (loads, LDS-DMAs, stores) are still in flight.
// -DEDTR_DRAIN_WAITS, diagnostic build only (tools/exp/ffn_debug.py): every counted wait drains the queue.  The generated
// loop of attn_v3_loop.inc carries its waits inside whole asm strings and is not covered.
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field on gfx9");
#ifdef EDTR_DRAIN_WAITS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}
__device__ __forceinline__ void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void wait_vm_lds() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }   // one instruction
__device__ __forceinline__ void block_sync() {
    wait_lds();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
