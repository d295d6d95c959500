// hsva.hip -- the custom colour target of the reference's tutorial (Snippets/PNG/CustomColor.swift) on arrays of pixels for gfx950
// (spng_hsva_batch).
//
// Replaces, mapped over an array,
//   HSVA.init(r:g:b:a:)                     Snippets/PNG/CustomColor.swift:19-49     SPNG_HSVA_FROM_RGBA8
//   HSVA.rgba                               CustomColor.swift:51-78                  SPNG_HSVA_TO_RGBA8
//   (c.v, c.a), kernel: \.v                 CustomColor.swift:232-251                SPNG_HSVA_TO_VA8
// the halves of HSVA.unpack / HSVA.pack (CustomColor.swift:86-299) that spng_unpack_batch and spng_pack_batch do not cover.
// HBM-bound by design: 16-byte accesses on both sides (16 bytes of RGBA8 and 32 bytes of HSVA per lane and step; 64 bytes of
// HSVA for 16 of VA8), no integer division (hsva.hpp), no LDS.
#include "hsva.hpp"

namespace spng {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// One job with the operation known to the compiler.  Both loops are walked wave by wave, as alpha_run's are.
template <int OP>
__device__ __forceinline__ void hsva_run(const HsvaJob &job, uint32_t &trapped)
{
    constexpr uint32_t PPV = OP == SPNG_HSVA_TO_VA8 ? 8 : 4;    // pixels of a lane and step: 16 bytes of the narrower side
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    // arrays that are not aligned to 16 bytes go pixel by pixel, like the tail
    const uint64_t nvec = (((uintptr_t)job.in | (uintptr_t)job.out) & 15) == 0 ? job.count / PPV : 0;
    const v4u *vin = (const v4u *)job.in;
    v4u *vout = (v4u *)job.out;
    for (uint64_t base = wave * 64; base < nvec; base += waves * 64) {
        const uint64_t i = base + lane;
        if (i < nvec) {
            if (OP == SPNG_HSVA_FROM_RGBA8) {
                const v4u v = vin[i];
                uint32_t h[4], sva[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) hsva_from_rgba(v[k], h[k], sva[k]);
                vout[2 * i] = (v4u){h[0], sva[0], h[1], sva[1]};
                vout[2 * i + 1] = (v4u){h[2], sva[2], h[3], sva[3]};
            } else if (OP == SPNG_HSVA_TO_RGBA8) {
                const v4u a = vin[2 * i], b = vin[2 * i + 1];
                v4u o;
                o[0] = hsva_to_rgba(a[0], a[1], trapped); o[1] = hsva_to_rgba(a[2], a[3], trapped);
                o[2] = hsva_to_rgba(b[0], b[1], trapped); o[3] = hsva_to_rgba(b[2], b[3], trapped);
                vout[i] = o;
            } else {
                v4u o;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const v4u a = vin[4 * i + k];
                    o[k] = hsva_to_va(a[1]) | hsva_to_va(a[3]) << 16;
                }
                vout[i] = o;
            }
        }
    }
    // the HSVA side is aligned to 4 (the host checks), the RGBA8 / VA8 side to nothing
    for (uint64_t base = nvec * PPV + wave * 64; base < job.count; base += waves * 64) {
        const uint64_t i = base + lane;
        if (i < job.count) {
            if (OP == SPNG_HSVA_FROM_RGBA8) {
                const uint8_t *p = (const uint8_t *)job.in + 4 * i;
                uint32_t *o = (uint32_t *)job.out + 2 * i;
                hsva_from_rgba(p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24, o[0], o[1]);
            } else {
                const uint32_t *p = (const uint32_t *)job.in + 2 * i;
                if (OP == SPNG_HSVA_TO_RGBA8) {
                    uint8_t *o = (uint8_t *)job.out + 4 * i;
                    const uint32_t c = hsva_to_rgba(p[0], p[1], trapped);
                    o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16); o[3] = (uint8_t)(c >> 24);
                } else {
                    uint8_t *o = (uint8_t *)job.out + 2 * i;
                    const uint32_t c = hsva_to_va(p[1]);
                    o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void hsva_kernel(const HsvaJob *__restrict__ jobs)
{
    const HsvaJob job = jobs[blockIdx.y];
    uint32_t trapped = 0;                                       // pixels of this lane the reference would have trapped on
    switch (job.op) {
    case SPNG_HSVA_FROM_RGBA8: hsva_run<SPNG_HSVA_FROM_RGBA8>(job, trapped); break;
    case SPNG_HSVA_TO_RGBA8: hsva_run<SPNG_HSVA_TO_RGBA8>(job, trapped); break;
    case SPNG_HSVA_TO_VA8: hsva_run<SPNG_HSVA_TO_VA8>(job, trapped); break;
    }
    add_wave_count(job.result, trapped);
}

hipError_t launch_hsva(const HsvaJob *d_jobs, uint32_t count, uint32_t blocks_x, hipStream_t stream)
{
    if (!count) return hipSuccess;
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) { hsva_kernel<<<dim3(blocks_x ? blocks_x : 1, ny), 256, 0, stream>>>(d_jobs + y0); });
}

}  // namespace spng
