// luminance.hip -- the pixel step of the reference's tutorial Snippets/PNG/BasicEncoding.swift on arrays of pixels for gfx950
// (spng_luminance_batch).
//
// Replaces, mapped over an array,
//   COMPUTE_LUMINANCE                       Snippets/PNG/BasicEncoding.swift:63-71   SPNG_LUMINANCE_V8
//   the same with the pixel's alpha beside it                                        SPNG_LUMINANCE_VA8
// hsva_kernel's shape: a job table over grid rows, 16-byte accesses on both sides -- so a lane takes 64 bytes of RGBA8 for 16 of V8
// and 32 for 16 of VA8 per step: its store is always a whole dwordx4 --, a pixel-by-pixel path for tails and unaligned arrays.  The
// arithmetic (luminance.hpp) is binary64 up to x; the root is a float estimate settled against a table of 257 doubles in LDS.
#include "luminance.hpp"

namespace spng {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// One job with the operation known to the compiler.  Both loops are walked wave by wave, as hsva_run's are.
template <int OP>
__device__ __forceinline__ void luminance_run(const LuminanceJob &job, const double *step)
{
    constexpr uint32_t PPV = OP == SPNG_LUMINANCE_V8 ? 16 : 8;  // pixels of a lane and step: 16 bytes of output
    constexpr uint32_t NIN = PPV / 4;                           // ... from so many 16-byte loads
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    // arrays that are not aligned to 16 bytes go pixel by pixel, like the tail
    const uint64_t nvec = (((uintptr_t)job.in | (uintptr_t)job.out) & 15) == 0 ? job.count / PPV : 0;
    const v4u *vin = (const v4u *)job.in;
    v4u *vout = (v4u *)job.out;
    for (uint64_t base = wave * 64; base < nvec; base += waves * 64) {
        const uint64_t i = base + lane;
        if (i < nvec) {
            v4u v[NIN], o;
#pragma unroll
            for (uint32_t k = 0; k < NIN; ++k) v[k] = vin[NIN * i + k];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                if (OP == SPNG_LUMINANCE_V8) {
                    o[k] = luminance(v[k][0], step) | luminance(v[k][1], step) << 8 | luminance(v[k][2], step) << 16 |
                           luminance(v[k][3], step) << 24;
                } else {
                    const uint32_t p = v[k / 2][2 * (k & 1)], q = v[k / 2][2 * (k & 1) + 1];
                    o[k] = luminance(p, step) | (p >> 24) << 8 | luminance(q, step) << 16 | (q & 0xff000000u);
                }
            }
            vout[i] = o;
        }
    }
    for (uint64_t base = nvec * PPV + wave * 64; base < job.count; base += waves * 64) {
        const uint64_t i = base + lane;
        if (i < job.count) {
            const uint8_t *p = (const uint8_t *)job.in + 4 * i;
            const uint32_t l = luminance(p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16, step);
            if (OP == SPNG_LUMINANCE_V8) {
                ((uint8_t *)job.out)[i] = (uint8_t)l;
            } else {
                uint8_t *o = (uint8_t *)job.out + 2 * i;
                o[0] = (uint8_t)l; o[1] = p[3];
            }
        }
    }
}

__global__ __launch_bounds__(256) void luminance_kernel(const LuminanceJob *__restrict__ jobs)
{
    __shared__ double step[SPNG_LUMINANCE_STEPS];
    for (uint32_t k = threadIdx.x; k < SPNG_LUMINANCE_STEPS; k += blockDim.x) step[k] = LUMINANCE_STEP[k];
    __syncthreads();
    const LuminanceJob job = jobs[blockIdx.y];
    if (job.op == SPNG_LUMINANCE_V8) luminance_run<SPNG_LUMINANCE_V8>(job, step);
    else luminance_run<SPNG_LUMINANCE_VA8>(job, step);
}

hipError_t launch_luminance(const LuminanceJob *d_jobs, uint32_t count, uint32_t blocks_x, hipStream_t stream)
{
    if (!count) return hipSuccess;
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) { luminance_kernel<<<dim3(blocks_x ? blocks_x : 1, ny), 256, 0, stream>>>(d_jobs + y0); });
}

}  // namespace spng
