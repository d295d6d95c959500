// indexing.hip -- indexed colour with any pure indexer, on the device, for gfx950 (spng_census_batch, spng_pack_indexed_batch).
//
// Replaces, for T = UInt8 / UInt16, the indexer half of
//   PNG.RGBA<T>.pack(_:as:indexer:)                     Sources/PNG/ColorTargets/PNG.RGBA.swift:409-423
//   PNG.VA<T>.pack(_:as:indexer:)                       PNG.VA.swift:334-350
//   the scalar PNG.Image.pack<T>(_:as:indexer:)         Sources/PNG/PNG.Image.swift:767-782
//   PNG.Image.init(packing:size:layout:metadata:indexer:)   PNG.Image.swift:935-996
//   PNG.deconvolve(_:_:dereference:)                    Sources/PNG/PNG.swift:747-854
// An indexer is a closure over a UInt8 aggregate, so it is a table: the CENSUS reports the distinct aggregates ("keys") of a pixel
// array with their frequencies (what PNG.Histogram and sPLT entries hold), the host evaluates the closure once per key, and the
// MAPPED PACK stores the resulting index of every pixel.  The key of a pixel: its components after the optional
// premultiplication, reduced to UInt8 (>> 8 for T = UInt16, PNG.swift:829-852), r | g << 8 | b << 16 | a << 24, v | a << 8, or v.
//
// Both kernels are HBM-bound by design: four pixels per lane, 16-byte loads where the pixels are aligned, one dword of four indices
// out where the storage is.
#include "indexing.hpp"                                        // (the key of a pixel: quad_keys, index_hash)

namespace spng {

// ---- thresholds (mirrored in swift_png_amd/__init__.py; tests/test_indexing_host.py compares the two) -----------------------------
static constexpr uint32_t CENSUS_LDS_SLOTS = 2048;              // a workgroup's private table: 64-bit slots, open addressing
static constexpr uint32_t CENSUS_LDS_LIMIT = 512;               // keys in it above which it is merged into the image's table: a round
                                                                // adds at most 1024 keys (256 lanes x 4 pixels), so it never fills
static constexpr uint32_t CENSUS_MIN_SLOTS = 64;                // the image's table: max(this, 2 x cap rounded up to a power of two)
static constexpr uint32_t CENSUS_FINISH_LDS_KEYS = 4096;        // up to so many keys (rounded up to a power of two) are sorted in LDS
static constexpr uint32_t PACK_INDEXED_LDS_KEYS = 512;          // maps of up to so many keys are looked up in an LDS hash table,
static constexpr uint32_t PACK_INDEXED_LDS_SLOTS = 2048;        // (of so many slots), larger ones by binary search over d_keys

// ---- census -------------------------------------------------------------------------------------------------------------------
// The image's table (context scratch, zeroed by the host in front of every call): `slots` tags -- 0: empty, else key << 32 | 1, so
// that no key value, 0x00000000 and 0xFFFFFFFF included, can look like an empty slot -- claimed by compare-and-swap, and as many
// 64-bit counts.  ctrl[0]: the distinct keys claimed so far; ctrl[1]: the overflow flag, raised when ctrl[0] passes `cap` (or, never
// seen, when the table is full): workgroups that see it stop reading.  Global atomics only (no workgroup waits for another);
// census_finish_kernel runs in a launch of its own.  Every probe loop is bounded by the table's size.
__device__ __forceinline__ uint32_t census_overflowed(const CensusJob &job)
{
    return __hip_atomic_load(job.ctrl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void census_global_add(const CensusJob &job, uint32_t key, uint64_t n)
{
    const unsigned long long tag = (unsigned long long)key << 32 | 1u;
    const uint32_t mask = job.slots - 1;
    uint32_t h = (index_hash(key) >> (32 - job.slot_bits)) & mask;
    for (uint32_t step = 0; step < job.slots; ++step, h = (h + 1) & mask) {
        // (a slot never changes once it is claimed: a plain load that sees a tag is right, one that sees a stale 0 costs the CAS)
        unsigned long long old = job.tags[h];
        if (old == 0ull) {
            old = atomicCAS(job.tags + h, 0ull, tag);
            if (old == 0ull) {
                old = tag;
                if (atomicAdd(job.ctrl, 1u) + 1u > job.cap) atomicOr(job.ctrl + 1, 1u);
            }
        }
        if (old == tag) { atomicAdd(job.counts + h, (unsigned long long)n); return; }
        // (long probe sequences exist only in a table that overflows: the result is decided, nobody needs this key)
        if ((step & 31u) == 31u && census_overflowed(job)) return;
    }
    atomicOr(job.ctrl + 1, 1u);                                 // full: more than cap keys
}

// A workgroup's table: 0: empty, else key << 32 | 1 << 31 | count (count < 2^31: the table is merged at least every 2^20 rounds)
__device__ __forceinline__ void census_lds_add(unsigned long long *table, uint32_t *used, const CensusJob &job, uint32_t key, uint32_t n)
{
    const unsigned long long tag = (unsigned long long)key << 32 | 0x80000000u;
    uint32_t h = index_hash(key) >> 21;                         // (CENSUS_LDS_SLOTS == 2^11)
    static_assert(CENSUS_LDS_SLOTS == 1u << 11, "the shift above");
    for (uint32_t step = 0; step < CENSUS_LDS_SLOTS; ++step, h = (h + 1) & (CENSUS_LDS_SLOTS - 1)) {
        unsigned long long e = table[h];
        if (e == 0ull) {
            e = atomicCAS(table + h, 0ull, tag);
            if (e == 0ull) { atomicAdd(used, 1u); e = tag; }
        }
        if ((uint32_t)(e >> 32) == key) { atomicAdd(table + h, (unsigned long long)n); return; }
    }
    census_global_add(job, key, n);                             // (a full table: not reached below the load limit)
}

template <typename T, int LAYOUT>
__device__ __forceinline__ void census_run(const CensusJob &job, unsigned long long *table, uint32_t *used, uint32_t *stop)
{
    const T *in = (const T *)job.pixels;
    const uint64_t n = job.count, quads = (n + 3) / 4;
    const bool vec = quad_aligned<T, LAYOUT>(job.pixels);
    const uint32_t lane = threadIdx.x & 63;
    uint32_t rounds = 0;
    // walked workgroup by workgroup: every thread makes the same number of rounds (ballots and barriers below)
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < quads; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = base + threadIdx.x;
        const bool live = q < quads;
        const uint32_t m = !live ? 0u : n - q * 4 < 4 ? (uint32_t)(n - q * 4) : 4u;
        uint32_t key[4] = {0, 0, 0, 0}, cnt[4];
        if (live) quad_keys<T, LAYOUT>(in, q * 4, m, vec, job.premultiply, key);
        // equal pixels of a lane are counted once
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) cnt[k] = k < m ? 1u : 0u;
#pragma unroll
        for (uint32_t k = 1; k < 4; ++k) {
            bool merged = false;
#pragma unroll
            for (uint32_t j = 0; j < k; ++j)
                if (!merged && cnt[k] && cnt[j] && key[j] == key[k]) { cnt[j] += cnt[k]; cnt[k] = 0; merged = true; }
        }
        // ... and a wave whose pixels are all one colour (flat areas) adds once: the live lanes are lanes 0 .. of the wave
        const uint32_t first = UNI(key[0]);
        const unsigned long long lives = __ballot(live), same = __ballot(live && cnt[0] == m && key[0] == first);
        if (lives != 0ull && same == lives) {
            uint32_t total = m;
#pragma unroll
            for (int s = 32; s; s >>= 1) total += (uint32_t)__shfl_xor((int)total, s);
            if (lane == 0) census_lds_add(table, used, job, first, total);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) if (cnt[k]) census_lds_add(table, used, job, key[k], cnt[k]);
        }
        ++rounds;
        // `used` only grows during a round, and the thread that took it over the limit looks at it afterwards: all or none merge
        if (__syncthreads_or(*used > CENSUS_LDS_LIMIT || (rounds & 0xfffffu) == 0u)) {
            for (uint32_t i = threadIdx.x; i < CENSUS_LDS_SLOTS; i += blockDim.x) {
                const unsigned long long e = table[i];
                if (e == 0ull) continue;
                if (census_overflowed(job)) break;              // (one request per wave; the counts of an overflow are nobody's)
                census_global_add(job, (uint32_t)(e >> 32), (uint32_t)e & 0x7fffffffu);
                table[i] = 0ull;
            }
            if (threadIdx.x == 0) { *used = 0; *stop = census_overflowed(job); }
            __syncthreads();
            if (*stop) return;                                  // (more than cap keys: the rest of the pixels cannot change that)
        }
    }
    // what is left
    for (uint32_t i = threadIdx.x; i < CENSUS_LDS_SLOTS; i += blockDim.x) {
        const unsigned long long e = table[i];
        if (e != 0ull) census_global_add(job, (uint32_t)(e >> 32), (uint32_t)e & 0x7fffffffu);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void census_kernel(const CensusJob *__restrict__ jobs)
{
    const CensusJob job = jobs[blockIdx.y];
    if ((uint64_t)blockIdx.x * blockDim.x >= (job.count + 3) / 4) return;      // (the grid is sized for the largest array)
    __shared__ unsigned long long table[CENSUS_LDS_SLOTS];
    __shared__ uint32_t used, stop;
    for (uint32_t i = threadIdx.x; i < CENSUS_LDS_SLOTS; i += blockDim.x) table[i] = 0ull;
    if (threadIdx.x == 0) { used = 0; stop = census_overflowed(job); }
    __syncthreads();
    if (stop) return;
    if (job.layout == 0) census_run<T, 0>(job, table, &used, &stop);
    else if (job.layout == 1) census_run<T, 1>(job, table, &used, &stop);
    else census_run<T, 2>(job, table, &used, &stop);
}

// One workgroup per image, behind census_kernel: the claimed slots are gathered as key << 32 | slot, sorted ascending (a bitonic
// network over the next power of two, in LDS up to CENSUS_FINISH_LDS_KEYS elements and in the context's scratch above), and written
// out with their counts.  The order of the gather is arbitrary, the keys are distinct: the output is a function of the pixels alone.
__global__ __launch_bounds__(1024) void census_finish_kernel(const CensusJob *__restrict__ jobs)
{
    const CensusJob job = jobs[blockIdx.x];
    __shared__ unsigned long long lds[CENSUS_FINISH_LDS_KEYS];
    __shared__ uint32_t gathered;
    const uint32_t n = job.ctrl[0];
    if (job.ctrl[1] != 0u || n > job.cap) {
        if (threadIdx.x == 0) {
            spng_result r;
            r.status = SPNG_E_OUTPUT_CAPACITY; r.reserved = 0; r.written = 0; r.consumed = 0; r.aux[0] = 0; r.aux[1] = 0;
            *job.result = r;
        }
        return;
    }
    uint32_t np = 1;
    while (np < n) np <<= 1;                                    // n <= cap <= 65536: np <= the scratch's pow2(cap) elements
    unsigned long long *buf = np <= CENSUS_FINISH_LDS_KEYS ? lds : job.sort;
    if (threadIdx.x == 0) gathered = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < job.slots; i += blockDim.x) {
        const unsigned long long tag = job.tags[i];
        if (tag != 0ull) {
            const uint32_t at = atomicAdd(&gathered, 1u);
            if (at < np) buf[at] = (tag & 0xffffffff00000000ull) | i;
        }
    }
    for (uint32_t i = n + threadIdx.x; i < np; i += blockDim.x) buf[i] = ~0ull;   // (above every element: slot numbers are < 2^18)
    __syncthreads();
    for (uint32_t k = 2; k <= np; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < np / 2; i += blockDim.x) {
                const uint32_t a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a + j;
                const unsigned long long x = buf[a], y = buf[b];
                if ((x > y) == ((a & k) == 0u)) { buf[a] = y; buf[b] = x; }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned long long e = buf[i];
        job.keys[i] = (uint32_t)(e >> 32);
        if (job.out_counts) job.out_counts[i] = job.counts[(uint32_t)e & (job.slots - 1)];
    }
    if (threadIdx.x == 0) {
        spng_result r;
        r.status = SPNG_DONE; r.reserved = 0; r.written = n; r.consumed = job.count; r.aux[0] = 0; r.aux[1] = 0;
        *job.result = r;
    }
}

// ---- mapped pack --------------------------------------------------------------------------------------------------------------
// Every pixel stores indices[j] where keys[j] is its key, `miss` where none is.  Maps of up to PACK_INDEXED_LDS_KEYS keys sit in an
// LDS hash table (0: empty, else key << 32 | 0x100 | index; load <= 1/4), larger ones are searched in d_keys (ascending), which the
// L2 holds: 64 K keys are 256 KiB.  A lane looks a run of equal pixels up once.
struct IndexMap {
    const unsigned long long *table;                            // null: binary search
    const uint32_t *keys;
    const uint8_t *indices;
    uint32_t count, miss;
    __device__ __forceinline__ uint32_t operator()(uint32_t key, uint32_t &missed) const
    {
        if (table) {
            uint32_t h = index_hash(key) >> 21;
            static_assert(PACK_INDEXED_LDS_SLOTS == 1u << 11, "the shift above");
            for (uint32_t step = 0; step < PACK_INDEXED_LDS_SLOTS; ++step, h = (h + 1) & (PACK_INDEXED_LDS_SLOTS - 1)) {
                const unsigned long long e = table[h];
                if (e == 0ull) break;
                if ((uint32_t)(e >> 32) == key) return (uint32_t)e & 0xffu;
            }
        } else {
            uint32_t lo = 0, hi = count;                        // (at most 17 rounds)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (keys[mid] < key) lo = mid + 1; else hi = mid;
            }
            if (lo < count && keys[lo] == key) return indices[lo];
        }
        ++missed;
        return miss;
    }
};

template <typename T, int LAYOUT>
__device__ __forceinline__ void pack_indexed_run(const PackIndexedJob &job, const IndexMap &map, uint32_t &missed)
{
    const T *in = (const T *)job.pixels;
    const uint64_t n = (uint64_t)job.width * job.height, quads = (n + 3) / 4;
    const bool vec = quad_aligned<T, LAYOUT>(job.pixels), words = ((uintptr_t)job.storage & 3) == 0;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i0 = q * 4;
        const uint32_t m = n - i0 < 4 ? (uint32_t)(n - i0) : 4u;
        uint32_t key[4], idx[4] = {0, 0, 0, 0};
        quad_keys<T, LAYOUT>(in, i0, m, vec, job.premultiply, key);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (k >= m) continue;
            if (k && key[k] == key[k - 1]) { idx[k] = idx[k - 1]; missed += idx[k] >> 8; }
            else { uint32_t mine = 0; idx[k] = map(key[k], mine); idx[k] |= mine << 8; missed += mine; }   // (bit 8: this one missed)
        }
        uint8_t *dst = job.storage + i0;
        if (m == 4 && words) *(uint32_t *)dst = (idx[0] & 0xff) | (idx[1] & 0xff) << 8 | (idx[2] & 0xff) << 16 | (idx[3] & 0xff) << 24;
        else for (uint32_t k = 0; k < m; ++k) dst[k] = (uint8_t)idx[k];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_indexed_kernel(const PackIndexedJob *__restrict__ jobs)
{
    const PackIndexedJob job = jobs[blockIdx.y];
    const uint64_t n = (uint64_t)job.width * job.height;
    if ((uint64_t)blockIdx.x * blockDim.x >= (n + 3) / 4) return;
    __shared__ unsigned long long table[PACK_INDEXED_LDS_SLOTS];
    __shared__ uint32_t block_missed;
    const bool in_lds = job.map_count <= PACK_INDEXED_LDS_KEYS;
    if (threadIdx.x == 0) block_missed = 0;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < PACK_INDEXED_LDS_SLOTS; i += blockDim.x) table[i] = 0ull;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < job.map_count; i += blockDim.x) {
            const uint32_t key = job.keys[i];
            const unsigned long long mine = (unsigned long long)key << 32 | 0x100u | job.indices[i];
            uint32_t h = index_hash(key) >> 21;
            for (uint32_t step = 0; step < PACK_INDEXED_LDS_SLOTS; ++step, h = (h + 1) & (PACK_INDEXED_LDS_SLOTS - 1)) {
                const unsigned long long old = atomicCAS(table + h, 0ull, mine);
                if (old == 0ull || (uint32_t)(old >> 32) == key) break;      // (a repeated key: whichever came first)
            }
        }
    }
    __syncthreads();
    IndexMap map;
    map.table = in_lds ? table : nullptr; map.keys = job.keys; map.indices = job.indices; map.count = job.map_count; map.miss = job.miss;
    uint32_t missed = 0;
    if (job.layout == 0) pack_indexed_run<T, 0>(job, map, missed);
    else if (job.layout == 1) pack_indexed_run<T, 1>(job, map, missed);
    else pack_indexed_run<T, 2>(job, map, missed);
    // the misses: summed per wave, added once per workgroup
#pragma unroll
    for (int s = 32; s; s >>= 1) missed += (uint32_t)__shfl_xor((int)missed, s);
    if ((threadIdx.x & 63) == 0 && missed) atomicAdd(&block_missed, missed);
    __syncthreads();
    if (threadIdx.x == 0 && block_missed) atomicAdd((unsigned long long *)&job.result->aux[0], (unsigned long long)block_missed);
}

uint32_t census_slots(uint32_t cap)
{
    uint32_t s = CENSUS_MIN_SLOTS;
    while (s < 2 * (uint64_t)cap) s <<= 1;
    return s;
}
uint32_t census_sort_elems(uint32_t cap)
{
    uint32_t s = 1;
    while (s < cap) s <<= 1;
    return s;
}

// the counting stage alone (spng_census_wide_batch finishes with the launches of colour_tables.hip)
hipError_t launch_census_count(const CensusJob *d_jobs, uint32_t count, uint32_t blocks_x, int bits, hipStream_t stream)
{
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        const dim3 grid(blocks_x ? blocks_x : 1, ny);
        if (bits == 8) census_kernel<uint8_t><<<grid, 256, 0, stream>>>(d_jobs + y0);
        else census_kernel<uint16_t><<<grid, 256, 0, stream>>>(d_jobs + y0);
    });
}

hipError_t launch_census(const CensusJob *d_jobs, uint32_t count, uint32_t blocks_x, int bits, hipStream_t stream)
{
    if (!count) return hipSuccess;
    const hipError_t e = launch_census_count(d_jobs, count, blocks_x, bits, stream);
    if (e != hipSuccess) return e;
    census_finish_kernel<<<count, 1024, 0, stream>>>(d_jobs);
    return hipGetLastError();
}

hipError_t launch_pack_indexed(const PackIndexedJob *d_jobs, uint32_t count, uint32_t blocks_x, int source, hipStream_t stream)
{
    if (!count) return hipSuccess;
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        const dim3 grid(blocks_x ? blocks_x : 1, ny);
        if (source == 8) pack_indexed_kernel<uint8_t><<<grid, 256, 0, stream>>>(d_jobs + y0);
        else pack_indexed_kernel<uint16_t><<<grid, 256, 0, stream>>>(d_jobs + y0);
    });
}

}  // namespace spng
