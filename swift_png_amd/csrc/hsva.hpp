// hsva.hpp -- the reference's custom colour target (Snippets/PNG/CustomColor.swift:4-78: struct HSVA { h: UInt32, s: UInt16,
// v: UInt8, a: UInt8 }) in integers, without an integer division: what hsva_kernel (hsva.hip) and its emulation share.
//
//   HSVA.init(r:g:b:a:)   CustomColor.swift:19-49    RGBA<UInt8> -> HSVA
//   HSVA.rgba             CustomColor.swift:51-78    HSVA -> RGBA<UInt8>
//
// A pixel in memory is Swift's and C's struct: {uint32 h; uint16 s; uint8 v; uint8 a}, 8 bytes, host byte order -- here two
// dwords, h and s | v << 16 | a << 24.
#pragma once
#include "common.hpp"

namespace spng {

// n / d for n < 2^24 and 1 <= d <= 255 (both exact as floats) where the quotient is below 2^17 -- the two divisions of
// HSVA.init(r:g:b:a:): at most 65536 and 65535.  v_rcp_f32 is good to 1 ulp and the product rounds once more, a relative error
// below 2^-22, so n * (1 / d) is less than 2^-5 away from n / d: the truncation is the quotient or one beside it, and one step
// of the remainder in either direction makes it exact.  The argument is not the proof: tests/test_gpu_hsva.py runs all 2^24
// colours through the real v_rcp_f32, tests/test_emu_hsva.py through a correctly rounded 1.0f / x.
__device__ __forceinline__ uint32_t hsva_div(uint32_t n, uint32_t d)
{
    uint32_t q = (uint32_t)((float)n * __builtin_amdgcn_rcpf((float)d));
    const int32_t r = (int32_t)(n - (q & 0x3ffffu) * d);         // (q < 2^17 + 2, d < 2^8: a 24-bit multiplication)
    q = r < 0 ? q - 1 : r >= (int32_t)d ? q + 1 : q;
    return q;
}

// HSVA.init(r:g:b:a:): -> h; sva = s | v << 16 | a << 24.  Nothing here can trap in the reference: max - min and mid - min do not
// underflow (the switch sorts, ties included), f <= 65537 because mid - min <= d, and s <= 65535 because d <= max.
__device__ __forceinline__ void hsva_from_rgba(uint32_t rgba, uint32_t &h, uint32_t &sva)
{
    const uint32_t r = rgba & 0xff, g = (rgba >> 8) & 0xff, b = (rgba >> 16) & 0xff;
    // the switch over (r < g, g < b, r < b), CustomColor.swift:23-31: its six cases as a table of eight nibbles; every case names
    // the components in ascending order, so the three sorted values are the plain minimum, median and maximum
    const uint32_t idx = (uint32_t)(r < g) << 2 | (uint32_t)(g < b) << 1 | (uint32_t)(r < b);
    const uint32_t sector = (0x33214500u >> (idx * 4)) & 7u;
    const uint32_t lo_rg = r < g ? r : g, hi_rg = r < g ? g : r;
    const uint32_t lo = lo_rg < b ? lo_rg : b, hi = hi_rg < b ? b : hi_rg, mid = hi_rg < b ? hi_rg : lo_rg < b ? b : lo_rg;
    const uint32_t d = hi - lo;
    h = 0;
    uint32_t s = 0;
    if (d) {
        const uint32_t f = hsva_div((mid - lo) << 16, d) + 1;
        h = 65537u * sector + ((sector & 1) ? 65537u - f : f);
        s = hsva_div((d << 16) - 1, hi);
    }
    sva = s | hi << 16 | (rgba & 0xff000000u);
}

// HSVA.rgba: -> r | g << 8 | b << 16 | a << 24.  The reference traps in one place only, fatalError("unreachable") for a sector
// above 5 with s > 0 and v > 0: the pixel becomes (v, v, v, a) then and `trapped` is counted up.  Nothing else can: s v < 2^24,
// so d = (s v >> 16) + 1 <= v (s v / 65536 < v) and y = v - d >= 0; f <= 65537, so f d < 2^24 and (f d) >> 16 <= d, z <= y + d = v
// <= 255.  h divmod 65537 from h = q 65536 + l = q 65537 + (l - q): (q, l - q) when l >= q, else (q - 1, l - q + 65537) with
// 2 <= l - q + 65537 <= 65536.
__device__ __forceinline__ uint32_t hsva_to_rgba(uint32_t h, uint32_t sva, uint32_t &trapped)
{
    const uint32_t s = sva & 0xffff, v = (sva >> 16) & 0xff, a = sva & 0xff000000u;
    const uint32_t grey = v * 0x010101u | a;
    if (s == 0 || v == 0) return grey;
    const uint32_t q = h >> 16, l = h & 0xffff;
    const uint32_t sector = l < q ? q - 1 : q, rem = l < q ? l - q + 65537u : l - q;
    if (sector > 5) { ++trapped; return grey; }
    const uint32_t f = (sector & 1) ? 65537u - rem : rem;
    const uint32_t d = ((s * v) >> 16) + 1;
    const uint32_t x = v, y = x - d, z = ((f * d) >> 16) + y;
    // CustomColor.swift:68-76: (x, z, y), (z, x, y), (y, x, z), (y, z, x), (z, y, x), (x, y, z)
    const uint32_t r = (sector == 0 || sector == 5) ? x : (sector == 1 || sector == 4) ? z : y;
    const uint32_t g = (sector == 1 || sector == 2) ? x : (sector == 0 || sector == 3) ? z : y;
    const uint32_t b = (sector == 3 || sector == 4) ? x : (sector == 2 || sector == 5) ? z : y;
    return r | g << 8 | b << 16 | a;
}

// what the tutorial's pack stores for the grey formats (kernel: \.v; (c.v, c.a) for va8 / va16, CustomColor.swift:232-251):
// v | a << 8.  Not .rgba.r.
__device__ __forceinline__ uint32_t hsva_to_va(uint32_t sva) { return sva >> 16; }

}  // namespace spng
