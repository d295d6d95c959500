// scanline.hpp -- what the two scanline sources, unfilter.hip (reconstruction) and encode.hip (filter selection), both use:
// the 16-byte vector and its unaligned form, PNG.paeth on one byte, and the move that brings a value from the lane above.
#pragma once
#include "common.hpp"

namespace spng {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));     // the two 16-bit halves of a dword, for the packed-i16 VALU ops
struct __attribute__((packed)) U128u { u32x4 v; };           // 16 bytes, alignment 1

// keeps a value out of the optimiser's sight: sign masks stay bit masks (v_bfi) instead of per-half compares
__device__ __forceinline__ uint32_t opaque(uint32_t v) { asm volatile("" : "+v"(v)); return v; }

// PNG.paeth (PNG.swift:124-147): a if pa <= pb && pa <= pc, else b if pb <= pc, else c.
__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// value of lane-1 (lane 0 receives `first`)
__device__ __forceinline__ uint32_t lane_above(uint32_t mine, uint32_t first)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)mine, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

}  // namespace spng
