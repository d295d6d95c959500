// alpha.hip -- premultiplied <-> straight alpha on arrays of colour-target pixels for gfx950 (spng_alpha_batch).
//
// Replaces, for T = UInt8 / UInt16,
//   PNG.RGBA<T>.premultiplied, .premultiplied(as: UInt8.self)   Sources/PNG/ColorTargets/PNG.RGBA.swift:121-158
//   PNG.RGBA<T>.straightened,  .straightened(as: UInt8.self)    PNG.RGBA.swift:167-206
//   PNG.VA<T>, the same four                                    PNG.VA.swift:57-131
//   PNG.premultiply / PNG.straighten                            Sources/PNG/PNG.swift:55-66, 101-117
// the two halves of the reference's iPhone-optimized tutorial (Snippets/PNG/iPhoneOptimized.swift) that spng_unpack_batch and
// spng_pack_batch do not cover when the caller already holds the pixels.  HBM-bound by design: 16 bytes per lane each way, no
// integer division (alpha.hpp), and a wave whose pixels are all opaque (or all clear) only copies.
#include "alpha.hpp"

namespace spng {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// the alpha bits of dword d of a lane's 16 bytes
template <typename T, int LAYOUT>
__device__ __forceinline__ constexpr uint32_t alpha_mask(int d)
{
    return sizeof(T) == 1 ? (LAYOUT == 0 ? 0xff000000u : 0xff00ff00u) : (LAYOUT == 0 && !(d & 1) ? 0u : 0xffff0000u);
}

// a lane's 16 bytes: four RGBA8, two RGBA16, eight VA8 or four VA16 pixels
template <typename T, int LAYOUT, int OP>
__device__ __forceinline__ void alpha_vec(v4u &v, uint32_t &trapped)
{
    constexpr uint32_t K = sizeof(T) * 8;
    if (K == 8 && LAYOUT == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = v[k];
            uint32_t c[3] = {w & 0xff, (w >> 8) & 0xff, (w >> 16) & 0xff}, a = w >> 24;
            alpha_pixel<8, OP, 3>(c, a, trapped);
            v[k] = c[0] | c[1] << 8 | c[2] << 16 | a << 24;
        }
    } else if (K == 8) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = v[k];
            uint32_t c0[1] = {w & 0xff}, a0 = (w >> 8) & 0xff, c1[1] = {(w >> 16) & 0xff}, a1 = w >> 24;
            alpha_pixel<8, OP, 1>(c0, a0, trapped);
            alpha_pixel<8, OP, 1>(c1, a1, trapped);
            v[k] = c0[0] | a0 << 8 | c1[0] << 16 | a1 << 24;
        }
    } else if (LAYOUT == 0) {
#pragma unroll
        for (int k = 0; k < 4; k += 2) {
            const uint32_t lo = v[k], hi = v[k + 1];
            uint32_t c[3] = {lo & 0xffff, lo >> 16, hi & 0xffff}, a = hi >> 16;
            alpha_pixel<16, OP, 3>(c, a, trapped);
            v[k] = c[0] | c[1] << 16; v[k + 1] = c[2] | a << 16;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = v[k];
            uint32_t c[1] = {w & 0xffff}, a = w >> 16;
            alpha_pixel<16, OP, 1>(c, a, trapped);
            v[k] = c[0] | a << 16;
        }
    }
}

// One job with the layout and the operation known to the compiler.  Both loops are walked wave by wave (every lane of a wave
// makes the same number of rounds), so the ballots below see the whole wave.
template <typename T, int LAYOUT, int OP>
__device__ __forceinline__ void alpha_run(const AlphaJob &job, uint32_t &trapped)
{
    constexpr uint32_t K = sizeof(T) * 8, NC = LAYOUT == 0 ? 3 : 1, PPV = 16 / ((NC + 1) * sizeof(T));   // pixels per 16 bytes
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const bool in_place = job.in == job.out;
    // arrays that are aligned to T but not to 16 bytes go pixel by pixel, like the tail
    const uint64_t nvec = (((uintptr_t)job.in | (uintptr_t)job.out) & 15) == 0 ? job.count / PPV : 0;
    const v4u *vin = (const v4u *)job.in;
    v4u *vout = (v4u *)job.out;
    for (uint64_t base = wave * 64; base < nvec; base += waves * 64) {
        const uint64_t i = base + lane;
        const bool live = i < nvec;
        v4u v = {0, 0, 0, 0};
        if (live) v = vin[i];
        bool work = true, changed = true;
        if (OP == SPNG_PREMULTIPLY || OP == SPNG_STRAIGHTEN) {
            // most pixels of real images are opaque: a == T.max is the identity for both operations; a == 0 is the identity
            // when straightening and gives zeros when premultiplying
            uint32_t all = ~0u, any = 0u;
#pragma unroll
            for (int d = 0; d < 4; ++d) { all &= v[d] | ~alpha_mask<T, LAYOUT>(d); any |= v[d] & alpha_mask<T, LAYOUT>(d); }
            if (__ballot(live && all != ~0u) == 0) { work = false; changed = false; }
            else if (__ballot(live && any != 0u) == 0) { work = false; changed = OP == SPNG_PREMULTIPLY; if (changed) v = (v4u){0, 0, 0, 0}; }
        }
        if (work) alpha_vec<T, LAYOUT, OP>(v, trapped);
        if (live && (changed || !in_place)) vout[i] = v;
    }
    const T *pin = (const T *)job.in;
    T *pout = (T *)job.out;
    for (uint64_t base = nvec * PPV + wave * 64; base < job.count; base += waves * 64) {
        const uint64_t i = base + lane;
        if (i < job.count) {
            uint32_t c[NC], a = pin[i * (NC + 1) + NC];
#pragma unroll
            for (uint32_t z = 0; z < NC; ++z) c[z] = pin[i * (NC + 1) + z];
            alpha_pixel<K, OP, (int)NC>(c, a, trapped);
#pragma unroll
            for (uint32_t z = 0; z < NC; ++z) pout[i * (NC + 1) + z] = (T)c[z];
            pout[i * (NC + 1) + NC] = (T)a;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void alpha_kernel(const AlphaJob *__restrict__ jobs)
{
    const AlphaJob job = jobs[blockIdx.y];
    uint32_t trapped = 0;                                       // components of this lane the reference would have trapped on
    switch (job.layout << 3 | job.op) {
    case 0 << 3 | SPNG_PREMULTIPLY: alpha_run<T, 0, SPNG_PREMULTIPLY>(job, trapped); break;
    case 0 << 3 | SPNG_STRAIGHTEN: alpha_run<T, 0, SPNG_STRAIGHTEN>(job, trapped); break;
    case 1 << 3 | SPNG_PREMULTIPLY: alpha_run<T, 1, SPNG_PREMULTIPLY>(job, trapped); break;
    case 1 << 3 | SPNG_STRAIGHTEN: alpha_run<T, 1, SPNG_STRAIGHTEN>(job, trapped); break;
    default:
        if constexpr (sizeof(T) == 2) {                         // the (as: UInt8.self) forms exist for T = UInt16 only
            switch (job.layout << 3 | job.op) {
            case 0 << 3 | SPNG_PREMULTIPLY_AS_U8: alpha_run<uint16_t, 0, SPNG_PREMULTIPLY_AS_U8>(job, trapped); break;
            case 0 << 3 | SPNG_STRAIGHTEN_AS_U8: alpha_run<uint16_t, 0, SPNG_STRAIGHTEN_AS_U8>(job, trapped); break;
            case 1 << 3 | SPNG_PREMULTIPLY_AS_U8: alpha_run<uint16_t, 1, SPNG_PREMULTIPLY_AS_U8>(job, trapped); break;
            case 1 << 3 | SPNG_STRAIGHTEN_AS_U8: alpha_run<uint16_t, 1, SPNG_STRAIGHTEN_AS_U8>(job, trapped); break;
            }
        }
    }
    add_wave_count(job.result, trapped);
}

hipError_t launch_alpha(const AlphaJob *d_jobs, uint32_t count, uint32_t blocks_x, int bits, hipStream_t stream)
{
    if (!count) return hipSuccess;
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        const dim3 grid(blocks_x ? blocks_x : 1, ny);
        if (bits == 8) alpha_kernel<uint8_t><<<grid, 256, 0, stream>>>(d_jobs + y0);
        else alpha_kernel<uint16_t><<<grid, 256, 0, stream>>>(d_jobs + y0);
    });
}

}  // namespace spng
