// text.hip -- the byte work between a text chunk's body and a String, for gfx950 (spng_text_batch).
//
// Replaces, for texts resident in HBM:
//   SPNG_TEXT_LATIN1_TO_UTF8   String(uncompressed.map{ Character(Unicode.Scalar($0)) }) and its .utf8 view: what PNG.Text.init(parsing:
//                              unicode: false) makes of a tEXt / zTXt body and PNG.Text.serialized writes back
//                              (Sources/PNG/Parsing/PNG.Text.swift:198, 309-349): a byte >= 0x80 becomes two
//   SPNG_TEXT_CHECK_UTF8       the question String(decoding:as: Unicode.UTF8.self) (:146, :173) answers silently by repairing: is the
//                              body well-formed UTF-8 (Unicode 15, table 3-7), and if not, where first and how often
// A text is cut into tiles of TEXT_TILE bytes, a workgroup each, 16 bytes per lane.  `text_count_kernel`: the bytes >= 0x80 of a tile
// (the ill-formed sequences that begin in it, and the first).  `text_scan_kernel`, a workgroup per text: the tiles' places in the
// output, the result.  `text_write_kernel`: a tile's output put together in LDS -- a lane's place from a scan over the workgroup -- and
// stored as dwords aligned on the destination.  Whether a byte begins an ill-formed sequence is decided from the three bytes in front
// of it and the three behind it (utf8_bad), read from memory, so lanes, 16-byte units and tiles are all the same boundary.
#include "common.hpp"

namespace spng {

static constexpr uint32_t TEXT_TILE = 4096, TEXT_THREADS = TEXT_TILE / 16, TEXT_NONE = 0xffffffffu;
static constexpr uint32_t TEXT_END = 0x100;                    // what lies outside the text: no continuation byte, no lead

// the up to 16 bytes at p[pos ...) of a text of len bytes, little-endian in w; -> how many there are
__device__ __forceinline__ uint32_t text_load16(const gbyte *p, uint64_t pos, uint64_t len, uint32_t w[4])
{
    typedef uint32_t c4 __attribute__((vector_size(16)));
    struct __attribute__((packed)) P16 { c4 v; };
#ifndef SPNG_EMU
    typedef P16 __attribute__((address_space(1))) gP16;
#else
    typedef P16 gP16;
#endif
    w[0] = w[1] = w[2] = w[3] = 0;
    if (pos >= len) return 0;
    if (len - pos >= 16) {
        const c4 v = ((const gP16 *)(p + pos))->v;
        w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
        return 16;
    }
    const uint32_t n = (uint32_t)(len - pos);
    for (uint32_t i = 0; i < n; ++i) w[i >> 2] |= (uint32_t)p[pos + i] << (8 * (i & 3));
    return n;
}

__device__ __forceinline__ bool utf8_cont(uint32_t c) { return (c & 0x1c0) == 0x80; }
// the length a lead byte announces; 0: no lead (a continuation byte, 0xc0, 0xc1, 0xf5 ... 0xff, the end)
__device__ __forceinline__ uint32_t utf8_len(uint32_t c) { return c < 0x80 ? 1 : c < 0xc2 ? 0 : c < 0xe0 ? 2 : c < 0xf0 ? 3 : c < 0xf5 ? 4 : 0; }
// may c follow the lead directly?  (table 3-7: no overlong forms, no surrogates, nothing above U+10FFFF)
__device__ __forceinline__ bool utf8_second(uint32_t lead, uint32_t c)
{
    const uint32_t lo = lead == 0xe0 ? 0xa0 : lead == 0xf0 ? 0x90 : 0x80, hi = lead == 0xed ? 0x9f : lead == 0xf4 ? 0x8f : 0xbf;
    return c >= lo && c <= hi;
}
// Does the byte b[3] begin an ill-formed sequence?  b[0 .. 2] lie in front of it, b[4 .. 6] behind it (TEXT_END outside the text).  A
// decoder that replaces maximal subparts restarts at every byte that is no continuation byte, and a continuation byte belongs to the
// sequence in front of it exactly when a lead byte within three bytes announces enough length and its own second byte is in range.
__device__ __forceinline__ bool utf8_bad(const uint32_t *b)
{
    const uint32_t c = b[3];
    if (c < 0x80) return false;
    if (utf8_cont(c)) {
#pragma unroll
        for (int d = 1; d <= 3; ++d) {
            const uint32_t lead = b[3 - d];
            if (!utf8_cont(lead)) return !(utf8_len(lead) > (uint32_t)d && utf8_second(lead, b[4 - d]));
        }
        return true;
    }
    const uint32_t n = utf8_len(c);
    return !(n && utf8_second(c, b[4]) && (n < 3 || utf8_cont(b[5])) && (n < 4 || utf8_cont(b[6])));
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *slots)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    __syncthreads();                                           // (the slots' last readers)
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    return slots[0] + slots[1] + slots[2] + slots[3];
}
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t *slots)
{
#pragma unroll
    for (int m = 32; m; m >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, m); v = o < v ? o : v; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t a = slots[0] < slots[1] ? slots[0] : slots[1], b = slots[2] < slots[3] ? slots[2] : slots[3];
    return a < b ? a : b;
}
static_assert(TEXT_THREADS == 256, "block_sum and block_min fold four waves");

__global__ __launch_bounds__(TEXT_THREADS) void text_count_kernel(const TextJob *__restrict__ jobs)
{
    __shared__ uint32_t slots[4];
    const TextJob job = jobs[blockIdx.y];
    const gbyte *in = (const gbyte *)job.in;
    for (uint64_t t = blockIdx.x; t < job.tiles; t += gridDim.x) {
        const uint64_t pos = t * TEXT_TILE + threadIdx.x * 16;
        uint32_t w[4];
        const uint32_t n = text_load16(in, pos, job.len, w);
        if (job.op == SPNG_TEXT_LATIN1_TO_UTF8) {
            const uint32_t high = __popc(w[0] & 0x80808080u) + __popc(w[1] & 0x80808080u) + __popc(w[2] & 0x80808080u) + __popc(w[3] & 0x80808080u);
            const uint32_t total = block_sum(high, slots);
            if (threadIdx.x == 0) job.counts[t] = total;
            continue;
        }
        // the lane's bytes with three on either side
        uint32_t b[22], bad = 0, first = TEXT_NONE;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            b[i] = n && pos + i >= 3 ? in[pos + i - 3] : TEXT_END;
            b[19 + i] = n == 16 && pos + 16 + i < job.len ? in[pos + 16 + i] : TEXT_END;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) b[3 + i] = (uint32_t)i < n ? (w[i >> 2] >> (8 * (i & 3))) & 0xff : TEXT_END;
        if ((w[0] | w[1] | w[2] | w[3]) & 0x80808080u) {
#pragma unroll
            for (int i = 15; i >= 0; --i)
                if ((uint32_t)i < n && utf8_bad(b + i)) { bad += 1; first = threadIdx.x * 16 + i; }
        }
        const uint32_t total = block_sum(bad, slots), lowest = block_min(first, slots);
        if (threadIdx.x == 0) { job.counts[t] = total; job.firsts[t] = lowest; }
    }
}

// a workgroup per text: the tiles' places in the output (job.offs), the result
__global__ __launch_bounds__(TEXT_THREADS) void text_scan_kernel(const TextJob *__restrict__ jobs, spng_result *__restrict__ results)
{
    __shared__ uint64_t sums[TEXT_THREADS];
    __shared__ uint64_t firsts[TEXT_THREADS];
    const TextJob job = jobs[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (job.tiles + TEXT_THREADS - 1) / TEXT_THREADS;
    const uint64_t lo = tid * per < job.tiles ? tid * per : job.tiles, hi = lo + per < job.tiles ? lo + per : job.tiles;
    uint64_t sum = 0, first = ~0ull;
    for (uint64_t t = lo; t < hi; ++t) {
        sum += job.counts[t];
        if (job.op == SPNG_TEXT_CHECK_UTF8 && first == ~0ull && job.firsts[t] != TEXT_NONE) first = t * TEXT_TILE + job.firsts[t];
    }
    sums[tid] = sum; firsts[tid] = first;
    __syncthreads();
    uint64_t before = 0, total = 0, lowest = ~0ull;
    for (uint32_t k = 0; k < TEXT_THREADS; ++k) {
        before += k < tid ? sums[k] : 0; total += sums[k];
        lowest = firsts[k] < lowest ? firsts[k] : lowest;
    }
    if (job.op == SPNG_TEXT_LATIN1_TO_UTF8)
        for (uint64_t t = lo; t < hi; ++t) { job.offs[t] = t * TEXT_TILE + before; before += job.counts[t]; }
    if (tid == 0) {
        spng_result r;
        r.reserved = 0; r.consumed = job.len; r.aux[0] = r.aux[1] = 0;
        if (job.op == SPNG_TEXT_LATIN1_TO_UTF8) {
            r.written = job.len + total;
            r.status = r.written > job.out_cap ? SPNG_E_OUTPUT_CAPACITY : SPNG_DONE;
        } else {
            r.written = 0;
            r.status = total ? SPNG_E_TEXT_ENCODING : SPNG_DONE;
            if (total) { r.aux[0] = lowest; r.aux[1] = total; }
        }
        results[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(TEXT_THREADS) void text_write_kernel(const TextJob *__restrict__ jobs, const spng_result *__restrict__ results)
{
    __shared__ uint32_t slots[4];
    __shared__ uint8_t obuf[2 * TEXT_TILE];
    const TextJob job = jobs[blockIdx.y];
    if (job.op != SPNG_TEXT_LATIN1_TO_UTF8 || results[blockIdx.y].status != SPNG_DONE) return;
    const gbyte *in = (const gbyte *)job.in;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t t = blockIdx.x; t < job.tiles; t += gridDim.x) {
        const uint64_t pos = t * TEXT_TILE + tid * 16;
        uint32_t w[4];
        const uint32_t n = text_load16(in, pos, job.len, w);
        const uint32_t high = __popc(w[0] & 0x80808080u) + __popc(w[1] & 0x80808080u) + __popc(w[2] & 0x80808080u) + __popc(w[3] & 0x80808080u);
        // the bytes >= 0x80 in front of the lane's, in its tile
        uint32_t incl = high;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)incl, d); incl += lane >= (uint32_t)d ? o : 0; }
        __syncthreads();                                       // (the previous tile's readers of slots and obuf)
        if (lane == 63) slots[wave] = incl;
        __syncthreads();
        uint32_t o = tid * 16 + incl - high;
        for (uint32_t k = 0; k < wave; ++k) o += slots[k];
        const uint64_t tile_len = job.len - t * TEXT_TILE < TEXT_TILE ? job.len - t * TEXT_TILE : TEXT_TILE;
        const uint32_t olen = (uint32_t)tile_len + slots[0] + slots[1] + slots[2] + slots[3];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xff;
            if ((uint32_t)i < n) {
                if (c < 0x80) obuf[o++] = (uint8_t)c;
                else { obuf[o] = (uint8_t)(0xc0 | c >> 6); obuf[o + 1] = (uint8_t)(0x80 | (c & 0x3f)); o += 2; }
            }
        }
        __syncthreads();
        // out of LDS: the bytes in front of the first aligned dword, the dwords, the bytes behind the last
        gbyte *out = (gbyte *)job.out + job.offs[t];
        const uint32_t lead = (uint32_t)((4 - ((uint64_t)out & 3)) & 3), head = lead < olen ? lead : olen;
        if (tid < head) out[tid] = obuf[tid];
        const uint32_t words = (olen - head) / 4;
        for (uint32_t k = tid; k < words; k += TEXT_THREADS) {
            const uint8_t *s = obuf + head + 4 * k;
#ifndef SPNG_EMU
            typedef uint32_t __attribute__((address_space(1))) gword;
#else
            typedef uint32_t gword;
#endif
            *(gword *)(out + head + 4 * k) = s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
        }
        const uint32_t done = head + 4 * words;
        if (tid < olen - done) out[done + tid] = obuf[done + tid];
    }
}

size_t text_tiles(uint64_t len) { return (size_t)((len + TEXT_TILE - 1) / TEXT_TILE); }
hipError_t launch_text(const TextJob *d_jobs, uint32_t count, uint32_t blocks_x, bool writes, spng_result *d_results, hipStream_t stream)
{
    if (!count) return hipSuccess;
    if (blocks_x) {
        const hipError_t e = launch_rows(count, [&](uint32_t y0, uint32_t ny) {
            text_count_kernel<<<dim3(blocks_x, ny), TEXT_THREADS, 0, stream>>>(d_jobs + y0);
        });
        if (e != hipSuccess) return e;
    }
    text_scan_kernel<<<count, TEXT_THREADS, 0, stream>>>(d_jobs, d_results);
    if (!blocks_x || !writes) return hipGetLastError();
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        text_write_kernel<<<dim3(blocks_x, ny), TEXT_THREADS, 0, stream>>>(d_jobs + y0, d_results + y0);
    });
}

}  // namespace spng
