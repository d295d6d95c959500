// indexing.hpp -- what the kernels of indexing.hip and colour_tables.hip share: the key of a pixel, four pixels per lane, and the hash of
// a key.  (The key: the pixel's components after the optional premultiplication, reduced to UInt8 -- >> 8 for T = UInt16,
// Sources/PNG/PNG.swift:829-852 --, r | g << 8 | b << 16 | a << 24, v | a << 8, or v.)
#pragma once
#include "alpha.hpp"

namespace spng {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t index_hash(uint32_t key) { return key * 0x9E3779B1u; }   // (the TOP bits are the slot)

// The keys of the (up to four) pixels i0 .. i0 + m of an array of RGBA<T> (LAYOUT 0), VA<T> (1) or T (2).  vec: the array is aligned
// to a whole quad (at most 16 bytes): one or two vector loads.  Keys behind m are 0 and not to be used.
template <typename T, int LAYOUT>
__device__ __forceinline__ void quad_keys(const T *in, uint64_t i0, uint32_t m, bool vec, uint32_t premultiply, uint32_t (&key)[4])
{
    constexpr uint32_t TB = sizeof(T) * 8, NC1 = LAYOUT == 0 ? 4 : LAYOUT == 1 ? 2 : 1, ND = NC1 * sizeof(T);   // dwords per quad
    constexpr uint32_t MASK = TB == 8 ? 0xffu : 0xffffu;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};                   // the quad's bytes in memory order
    const T *p = in + i0 * NC1;
    if (vec && m == 4) {
        if (ND == 1) w[0] = *(const uint32_t *)p;
        else if (ND == 2) { const v2u v = *(const v2u *)p; w[0] = v[0]; w[1] = v[1]; }
        else {
#pragma unroll
            for (uint32_t d = 0; d < ND; d += 4) {
                const v4u v = *(const v4u *)((const uint32_t *)p + d);
                w[d] = v[0]; w[d + 1] = v[1]; w[d + 2] = v[2]; w[d + 3] = v[3];
            }
        }
    } else {
#pragma unroll
        for (uint32_t e = 0; e < 4 * NC1; ++e)
            if (e < m * NC1) w[(e * sizeof(T)) >> 2] |= (uint32_t)p[e] << 8 * ((e * sizeof(T)) & 3);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        uint32_t c[4];
#pragma unroll
        for (uint32_t z = 0; z < NC1; ++z) {
            const uint32_t off = (k * NC1 + z) * sizeof(T);
            c[z] = (w[off >> 2] >> 8 * (off & 3)) & MASK;
        }
        uint32_t none = 0;
        if (LAYOUT == 0) {
            if (premultiply) { uint32_t rgb[3] = {c[0], c[1], c[2]}; alpha_pixel_op<TB, 3>(premultiply, rgb, c[3], none); c[0] = rgb[0]; c[1] = rgb[1]; c[2] = rgb[2]; }
            key[k] = (c[0] >> (TB - 8)) | (c[1] >> (TB - 8)) << 8 | (c[2] >> (TB - 8)) << 16 | (c[3] >> (TB - 8)) << 24;
        } else if (LAYOUT == 1) {
            if (premultiply) { uint32_t v[1] = {c[0]}; alpha_pixel_op<TB, 1>(premultiply, v, c[1], none); c[0] = v[0]; }
            key[k] = (c[0] >> (TB - 8)) | (c[1] >> (TB - 8)) << 8;
        } else {
            key[k] = c[0] >> (TB - 8);
        }
    }
}

template <typename T, int LAYOUT>
__device__ __forceinline__ bool quad_aligned(const void *pixels)
{
    constexpr uint32_t QB = 4 * (LAYOUT == 0 ? 4 : LAYOUT == 1 ? 2 : 1) * sizeof(T);
    return ((uintptr_t)pixels & ((QB < 16 ? QB : 16) - 1)) == 0;
}

}  // namespace spng
