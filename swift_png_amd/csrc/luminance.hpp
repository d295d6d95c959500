// luminance.hpp -- COMPUTE_LUMINANCE of the reference's tutorial (Snippets/PNG/BasicEncoding.swift:63-71) for one pixel: what
// luminance_kernel (luminance.hip) and its emulation share.
//
//   let l:Double = (0.299 * r * r + 0.587 * g * g + 0.114 * b * b).squareRoot()
//   return .init(max(0, min(l.rounded(), 255)))
//
// The arithmetic is the contract: IEEE-754 binary64, every product and sum rounded on its own, in Swift's association
// x = ((0.299 r) r + (0.587 g) g) + (0.114 b) b; the correctly rounded root; halves away from zero.  Of the 2^24 colours 38 land on
// an exact half, 97 change when this is evaluated in float, 2 when the products are taken as 0.299 (r r).
#pragma once
#include "common.hpp"

namespace spng {

// x.  Neither compiler may fuse a product into the sum behind it (hipcc does by default: 4 v_mul_f64 + 2 v_fma_f64 without the
// pragma, the 6 v_mul_f64 + 2 v_add_f64 of the reference with it).
__device__ __forceinline__ double luminance_square(uint32_t rgba)
{
#pragma clang fp contract(off)
    const double r = (double)(rgba & 0xff), g = (double)((rgba >> 8) & 0xff), b = (double)((rgba >> 16) & 0xff);
    return ((0.299 * r) * r + (0.587 * g) * g) + (0.114 * b) * b;
}

// LUMINANCE_STEP[k], k = 0 ... 255: the smallest double whose correctly rounded root rounds (halves away from zero) to k or more:
// (k - 0.5)^2, or the double in front of it where its root still rounds up to k - 0.5.  [256]: +infinity, so that 255 is the
// clamp.  Written by tools/make_luminance_table.py (bisection over the bit patterns); tools/emu/emu_luminance.cpp checks every
// entry and its predecessor against sqrt.
#define SPNG_LUMINANCE_STEPS 257
static __device__ const double LUMINANCE_STEP[SPNG_LUMINANCE_STEPS] = {
    0x0.0p+0, 0x1.0000000000000p-2, 0x1.2000000000000p+1, 0x1.8ffffffffffffp+2,
    0x1.8800000000000p+3, 0x1.43fffffffffffp+4, 0x1.e3fffffffffffp+4, 0x1.5200000000000p+5,
    0x1.c200000000000p+5, 0x1.20fffffffffffp+6, 0x1.68fffffffffffp+6, 0x1.b8fffffffffffp+6,
    0x1.0880000000000p+7, 0x1.3880000000000p+7, 0x1.6c80000000000p+7, 0x1.a480000000000p+7,
    0x1.e080000000000p+7, 0x1.103ffffffffffp+8, 0x1.323ffffffffffp+8, 0x1.563ffffffffffp+8,
    0x1.7c3ffffffffffp+8, 0x1.a43ffffffffffp+8, 0x1.ce3ffffffffffp+8, 0x1.fa3ffffffffffp+8,
    0x1.1420000000000p+9, 0x1.2c20000000000p+9, 0x1.4520000000000p+9, 0x1.5f20000000000p+9,
    0x1.7a20000000000p+9, 0x1.9620000000000p+9, 0x1.b320000000000p+9, 0x1.d120000000000p+9,
    0x1.f020000000000p+9, 0x1.080ffffffffffp+10, 0x1.188ffffffffffp+10, 0x1.298ffffffffffp+10,
    0x1.3b0ffffffffffp+10, 0x1.4d0ffffffffffp+10, 0x1.5f8ffffffffffp+10, 0x1.728ffffffffffp+10,
    0x1.860ffffffffffp+10, 0x1.9a0ffffffffffp+10, 0x1.ae8ffffffffffp+10, 0x1.c38ffffffffffp+10,
    0x1.d90ffffffffffp+10, 0x1.ef0ffffffffffp+10, 0x1.02c8000000000p+11, 0x1.0e48000000000p+11,
    0x1.1a08000000000p+11, 0x1.2608000000000p+11, 0x1.3248000000000p+11, 0x1.3ec8000000000p+11,
    0x1.4b88000000000p+11, 0x1.5888000000000p+11, 0x1.65c8000000000p+11, 0x1.7348000000000p+11,
    0x1.8108000000000p+11, 0x1.8f08000000000p+11, 0x1.9d48000000000p+11, 0x1.abc8000000000p+11,
    0x1.ba88000000000p+11, 0x1.c988000000000p+11, 0x1.d8c8000000000p+11, 0x1.e848000000000p+11,
    0x1.f808000000000p+11, 0x1.0403fffffffffp+12, 0x1.0c23fffffffffp+12, 0x1.1463fffffffffp+12,
    0x1.1cc3fffffffffp+12, 0x1.2543fffffffffp+12, 0x1.2de3fffffffffp+12, 0x1.36a3fffffffffp+12,
    0x1.3f83fffffffffp+12, 0x1.4883fffffffffp+12, 0x1.51a3fffffffffp+12, 0x1.5ae3fffffffffp+12,
    0x1.6443fffffffffp+12, 0x1.6dc3fffffffffp+12, 0x1.7763fffffffffp+12, 0x1.8123fffffffffp+12,
    0x1.8b03fffffffffp+12, 0x1.9503fffffffffp+12, 0x1.9f23fffffffffp+12, 0x1.a963fffffffffp+12,
    0x1.b3c3fffffffffp+12, 0x1.be43fffffffffp+12, 0x1.c8e3fffffffffp+12, 0x1.d3a3fffffffffp+12,
    0x1.de83fffffffffp+12, 0x1.e983fffffffffp+12, 0x1.f4a3fffffffffp+12, 0x1.ffe3fffffffffp+12,
    0x1.05a2000000000p+13, 0x1.0b62000000000p+13, 0x1.1132000000000p+13, 0x1.1712000000000p+13,
    0x1.1d02000000000p+13, 0x1.2302000000000p+13, 0x1.2912000000000p+13, 0x1.2f32000000000p+13,
    0x1.3562000000000p+13, 0x1.3ba2000000000p+13, 0x1.41f2000000000p+13, 0x1.4852000000000p+13,
    0x1.4ec2000000000p+13, 0x1.5542000000000p+13, 0x1.5bd2000000000p+13, 0x1.6272000000000p+13,
    0x1.6922000000000p+13, 0x1.6fe2000000000p+13, 0x1.76b2000000000p+13, 0x1.7d92000000000p+13,
    0x1.8482000000000p+13, 0x1.8b82000000000p+13, 0x1.9292000000000p+13, 0x1.99b2000000000p+13,
    0x1.a0e2000000000p+13, 0x1.a822000000000p+13, 0x1.af72000000000p+13, 0x1.b6d2000000000p+13,
    0x1.be42000000000p+13, 0x1.c5c2000000000p+13, 0x1.cd52000000000p+13, 0x1.d4f2000000000p+13,
    0x1.dca2000000000p+13, 0x1.e462000000000p+13, 0x1.ec32000000000p+13, 0x1.f412000000000p+13,
    0x1.fc02000000000p+13, 0x1.0200fffffffffp+14, 0x1.0608fffffffffp+14, 0x1.0a18fffffffffp+14,
    0x1.0e30fffffffffp+14, 0x1.1250fffffffffp+14, 0x1.1678fffffffffp+14, 0x1.1aa8fffffffffp+14,
    0x1.1ee0fffffffffp+14, 0x1.2320fffffffffp+14, 0x1.2768fffffffffp+14, 0x1.2bb8fffffffffp+14,
    0x1.3010fffffffffp+14, 0x1.3470fffffffffp+14, 0x1.38d8fffffffffp+14, 0x1.3d48fffffffffp+14,
    0x1.41c0fffffffffp+14, 0x1.4640fffffffffp+14, 0x1.4ac8fffffffffp+14, 0x1.4f58fffffffffp+14,
    0x1.53f0fffffffffp+14, 0x1.5890fffffffffp+14, 0x1.5d38fffffffffp+14, 0x1.61e8fffffffffp+14,
    0x1.66a0fffffffffp+14, 0x1.6b60fffffffffp+14, 0x1.7028fffffffffp+14, 0x1.74f8fffffffffp+14,
    0x1.79d0fffffffffp+14, 0x1.7eb0fffffffffp+14, 0x1.8398fffffffffp+14, 0x1.8888fffffffffp+14,
    0x1.8d80fffffffffp+14, 0x1.9280fffffffffp+14, 0x1.9788fffffffffp+14, 0x1.9c98fffffffffp+14,
    0x1.a1b0fffffffffp+14, 0x1.a6d0fffffffffp+14, 0x1.abf8fffffffffp+14, 0x1.b128fffffffffp+14,
    0x1.b660fffffffffp+14, 0x1.bba0fffffffffp+14, 0x1.c0e8fffffffffp+14, 0x1.c638fffffffffp+14,
    0x1.cb90fffffffffp+14, 0x1.d0f0fffffffffp+14, 0x1.d658fffffffffp+14, 0x1.dbc8fffffffffp+14,
    0x1.e140fffffffffp+14, 0x1.e6c0fffffffffp+14, 0x1.ec48fffffffffp+14, 0x1.f1d8fffffffffp+14,
    0x1.f770fffffffffp+14, 0x1.fd10fffffffffp+14, 0x1.015c800000000p+15, 0x1.0434800000000p+15,
    0x1.0710800000000p+15, 0x1.09f0800000000p+15, 0x1.0cd4800000000p+15, 0x1.0fbc800000000p+15,
    0x1.12a8800000000p+15, 0x1.1598800000000p+15, 0x1.188c800000000p+15, 0x1.1b84800000000p+15,
    0x1.1e80800000000p+15, 0x1.2180800000000p+15, 0x1.2484800000000p+15, 0x1.278c800000000p+15,
    0x1.2a98800000000p+15, 0x1.2da8800000000p+15, 0x1.30bc800000000p+15, 0x1.33d4800000000p+15,
    0x1.36f0800000000p+15, 0x1.3a10800000000p+15, 0x1.3d34800000000p+15, 0x1.405c800000000p+15,
    0x1.4388800000000p+15, 0x1.46b8800000000p+15, 0x1.49ec800000000p+15, 0x1.4d24800000000p+15,
    0x1.5060800000000p+15, 0x1.53a0800000000p+15, 0x1.56e4800000000p+15, 0x1.5a2c800000000p+15,
    0x1.5d78800000000p+15, 0x1.60c8800000000p+15, 0x1.641c800000000p+15, 0x1.6774800000000p+15,
    0x1.6ad0800000000p+15, 0x1.6e30800000000p+15, 0x1.7194800000000p+15, 0x1.74fc800000000p+15,
    0x1.7868800000000p+15, 0x1.7bd8800000000p+15, 0x1.7f4c800000000p+15, 0x1.82c4800000000p+15,
    0x1.8640800000000p+15, 0x1.89c0800000000p+15, 0x1.8d44800000000p+15, 0x1.90cc800000000p+15,
    0x1.9458800000000p+15, 0x1.97e8800000000p+15, 0x1.9b7c800000000p+15, 0x1.9f14800000000p+15,
    0x1.a2b0800000000p+15, 0x1.a650800000000p+15, 0x1.a9f4800000000p+15, 0x1.ad9c800000000p+15,
    0x1.b148800000000p+15, 0x1.b4f8800000000p+15, 0x1.b8ac800000000p+15, 0x1.bc64800000000p+15,
    0x1.c020800000000p+15, 0x1.c3e0800000000p+15, 0x1.c7a4800000000p+15, 0x1.cb6c800000000p+15,
    0x1.cf38800000000p+15, 0x1.d308800000000p+15, 0x1.d6dc800000000p+15, 0x1.dab4800000000p+15,
    0x1.de90800000000p+15, 0x1.e270800000000p+15, 0x1.e654800000000p+15, 0x1.ea3c800000000p+15,
    0x1.ee28800000000p+15, 0x1.f218800000000p+15, 0x1.f60c800000000p+15, 0x1.fa04800000000p+15,
    __builtin_inf()
};

// max(0, min(sqrt(x).rounded(), 255)) without the binary64 root: the answer is the largest k with x >= step[k].  A float root of
// the float of x (v_sqrt_f32, 1 ulp) is within 255 * 2^-21 of the root, so its rounding is that k or one beside it, and one
// comparison on either side settles it -- in binary64, against the table: nothing here depends on how the device rounds a root.
// `step`: LUMINANCE_STEP where the caller keeps it (LDS in the kernel).  -DSPNG_LUMINANCE_SQRT builds the form this one was measured
// against (profiles/r12_luminance.md): the compiler's own binary64 root, v_rsq_f64 and a refinement in some ten f64 operations.
__device__ __forceinline__ uint32_t luminance_of_square(double x, const double *step)
{
#ifdef SPNG_LUMINANCE_SQRT
    const double l = __builtin_round(__builtin_sqrt(x));
    return (uint32_t)(l > 255.0 ? 255.0 : l);
#else
    const uint32_t k = (uint32_t)(__builtin_amdgcn_sqrtf((float)x) + 0.5f);     // 0 ... 255: x <= 65025.000000000015
    return x < step[k] ? k - 1 : x >= step[k + 1] ? k + 1 : k;                  // (step[0] = 0 <= x < step[256])
#endif
}

__device__ __forceinline__ uint32_t luminance(uint32_t rgba, const double *step) { return luminance_of_square(luminance_square(rgba), step); }

}  // namespace spng
