// alpha.hpp -- premultiplied <-> straight alpha for one component, without an integer division: what alpha_kernel (alpha.hip) and
// the fused forms of unpack_kernel / pack_kernel (unpack.hip) share.
//
//   PNG.premultiply  Sources/PNG/PNG.swift:55-66     (c * a + (M >> 1)) / M                          M = T.max
//   PNG.straighten   Sources/PNG/PNG.swift:101-117   a == 0 ? p : (M * p + (a >> 1)) / a             traps when the quotient > M
//
// RGBA8 in and out at the copy ceiling leaves about 23 lane operations per component; the compiler's expansion of a 32-bit `/` by
// a run-time value is longer than that (profiles/r09_alpha.md).  K = 8 or 16 is the width of T; components and alpha are < 2^K.
#pragma once
#include "common.hpp"

namespace spng {

// x / (2^K - 1) for 0 <= x <= (2^K - 1)^2 + (2^K - 1) / 2: x = q M + r = q 2^K + (r - q) with r - q > -2^K, so x >> K is q or
// q - 1, and x + 1 + (x >> K) = q 2^K + (r + 1 or r), below (q + 1) 2^K since r < M.  (tests/test_emu_alpha.py walks the whole
// range for both K.)
template <uint32_t K>
__device__ __forceinline__ uint32_t div_tmax(uint32_t x) { return (x + 1u + (x >> K)) >> K; }

template <uint32_t K>
__device__ __forceinline__ uint32_t premultiply_c(uint32_t c, uint32_t a) { return div_tmax<K>(c * a + (((1u << K) - 1) >> 1)); }

// PNG.straighten for the components of one pixel: set up once per pixel (one v_rcp_f32), applied to every component.  `trapped` is
// counted up where the reference traps (a > 0 and p > a: the quotient does not fit T); the component is T.max then.
//   K = 8:  n = 255 p + (a >> 1) <= 65152; (n + 0.5) / a = p * (255 / a) + ((a >> 1) + 0.5) / a is one fused multiply-add on the byte
//           converted to float.  The exact value is at least 0.5 / 255 away from every integer, and above 256.4 exactly where the
//           reference traps (below 255.8 otherwise); the roundings of v_rcp_f32 (1 ulp), of the two constants and of the fma move
//           it by less than 2^-13 while it matters: the truncation is the quotient, and "> 255" is the trap.  a == 0 turns the
//           constants into the identity (p + 0.5).
//   K = 16: n < 2^32 is rounded to 24 bits and the estimate n * (1 / a) is off by less than 65535 * 2^-21 < 1: one step of the
//           remainder in either direction makes it exact (p is clamped to a so that the estimate stays inside T).
template <uint32_t K>
struct Straighten {
    float k1, k0;                                               // K = 8: the fma's constants;  K = 16: k1 = 1 / max(a, 1)
    uint32_t a;
    __device__ __forceinline__ explicit Straighten(uint32_t alpha) : a(alpha)
    {
        const float r = __builtin_amdgcn_rcpf((float)(a ? a : 1u));
        if (K == 8) { k1 = a ? 255.0f * r : 1.0f; k0 = a ? ((float)(a >> 1) + 0.5f) * r : 0.5f; }
        else { k1 = r; k0 = 0.0f; }
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t p, uint32_t &trapped) const
    {
        constexpr uint32_t M = (1u << K) - 1;
        if (K == 8) {
            const uint32_t q = (uint32_t)__builtin_fmaf((float)p, k1, k0);
            trapped += q > M;
            return q < M ? q : M;
        }
        const bool trap = p > a && a;
        const uint32_t pc = p < a ? p : a;
        const uint32_t n = (pc << K) - pc + (a >> 1);
        uint32_t q = (uint32_t)((float)n * k1);
        const int32_t r = (int32_t)(n - q * a);
        q = r < 0 ? q - 1 : r >= (int32_t)a ? q + 1 : q;
        trapped += trap;
        return trap ? M : a ? q : p;
    }
};

// One pixel of `NC` colour components (3: RGBA, 1: VA) and its alpha, in registers.  OP: SPNG_PREMULTIPLY, _AS_U8, SPNG_STRAIGHTEN,
// _AS_U8; the _AS_U8 forms (K = 16 only) run in eight bits and scale every component, alpha included, back by 257
// (PNG.RGBA.swift:146-158, 192-206).
template <uint32_t K, int OP, int NC>
__device__ __forceinline__ void alpha_pixel(uint32_t (&c)[NC], uint32_t &a, uint32_t &trapped)
{
    if (OP == 1) {
#pragma unroll
        for (int z = 0; z < NC; ++z) c[z] = premultiply_c<K>(c[z], a);
    } else if (OP == 2) {
        const uint32_t a8 = a >> 8;
#pragma unroll
        for (int z = 0; z < NC; ++z) c[z] = premultiply_c<8>(c[z] >> 8, a8) * 257u;
        a = a8 * 257u;
    } else if (OP == 3) {
        const Straighten<K> st(a);
#pragma unroll
        for (int z = 0; z < NC; ++z) c[z] = st(c[z], trapped);
    } else {
        const uint32_t a8 = a >> 8;
        const Straighten<8> st(a8);
#pragma unroll
        for (int z = 0; z < NC; ++z) c[z] = st(c[z] >> 8, trapped) * 257u;
        a = a8 * 257u;
    }
}

// the same with the operation in a register (the fused forms: one branch per pixel, uniform over the launch's job)
template <uint32_t K, int NC>
__device__ __forceinline__ void alpha_pixel_op(uint32_t op, uint32_t (&c)[NC], uint32_t &a, uint32_t &trapped)
{
    if (op == 1) alpha_pixel<K, 1, NC>(c, a, trapped);
    else if (op == 3) alpha_pixel<K, 3, NC>(c, a, trapped);
    else if (K == 16 && op == 2) alpha_pixel<K, 2, NC>(c, a, trapped);
    else if (K == 16 && op == 4) alpha_pixel<K, 4, NC>(c, a, trapped);
}

}  // namespace spng
