// colour_tables.hip -- colour tables without a ceiling, on the device, for gfx950 (spng_census_wide_batch, spng_map_batch).
//
// The reference lets a caller put any pure function between pixels and storage: the indexer closures of
//   PNG.RGBA<T>.pack(_:as:indexer:)                     Sources/PNG/ColorTargets/PNG.RGBA.swift:409-423
//   PNG.VA<T>.pack(_:as:indexer:)                       PNG.VA.swift:334-350
//   PNG.Image.pack<T>(_:as:indexer:) / init(packing:size:layout:metadata:indexer:)   Sources/PNG/PNG.Image.swift:767-782, 935-996
// and whole colour targets of the caller's own (Snippets/PNG/CustomColor.swift).  A pure function of a UInt8 aggregate is a table
// (indexing.hip); this file takes the table's two limits away: the WIDE CENSUS sorts up to 2^24 distinct keys on many workgroups
// -- the counting stage is census_kernel of indexing.hip itself --, and the MAP stores a value of 1, 2, 4 or 8 bytes per pixel
// through a hash table in the context's scratch.
//
// No workgroup waits for another inside a kernel: whatever needs a whole stage to have finished is a launch of its own on the
// context's stream, and every loop over a table is bounded by the table's size.
#include "indexing.hpp"

namespace spng {

// ---- thresholds (mirrored in swift_png_amd/__init__.py; tests/test_colour_tables_host.py compares the two) ------------------------
static constexpr uint32_t CENSUS_WIDE_TILE = 4096;              // elements a workgroup sorts in LDS: every stride below is fused there,
                                                                // every stride from here on is a launch over the whole buffer
static constexpr uint32_t MAP_LDS_KEYS = 512;                   // maps of up to so many keys are looked up in an LDS hash table
static constexpr uint32_t MAP_LDS_SLOTS = 2048;                 // (of so many slots), larger ones in a table in the context's scratch:
static constexpr uint32_t MAP_MIN_SLOTS = 64;                   // max(this, 2 x map_count rounded up to a power of two) slots

// ---- wide census: the stages behind census_kernel -------------------------------------------------------------------------------
// ctrl[0]: the distinct keys census_kernel claimed, ctrl[1]: its overflow flag, ctrl[2]: the cursor of the gather below (zeroed with
// the table).  -> false: more than cap keys, nothing to sort.  n: the keys; np: the next power of two, what the network sorts.
__device__ __forceinline__ bool census_wide_sizes(const CensusJob &job, uint32_t &n, uint32_t &np)
{
    n = job.ctrl[0];
    np = 1;
    if (job.ctrl[1] != 0u || n > job.cap) return false;
    while (np < n) np <<= 1;                                    // n <= min(cap, count): np <= the scratch's pow2(min(cap, count)) elements
    return true;
}

// The claimed slots gathered as key << 32 | slot (slots stay below 2^25), in whatever order the waves arrive -- the keys are
// distinct, so the sorted order does not depend on it --, and the elements [n, np) padded with ~0, which sorts above key
// 0xFFFFFFFF in any slot.  One atomic per wave: the table's size is a multiple of the wave's.
__global__ __launch_bounds__(256) void census_gather_kernel(const CensusJob *__restrict__ jobs)
{
    const CensusJob job = jobs[blockIdx.y];
    uint32_t n, np;
    if (!census_wide_sizes(job, n, np)) return;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * blockDim.x; base < job.slots; base += gridDim.x * blockDim.x) {
        const uint32_t i = base + threadIdx.x;                  // (a wave is inside the table or behind it: slots is a multiple of 64)
        const unsigned long long tag = i < job.slots ? job.tags[i] : 0ull;
        const unsigned long long claimed = __ballot(tag != 0ull);
        uint32_t at = 0;
        if (lane == 0 && claimed != 0ull) at = atomicAdd(job.ctrl + 2, (uint32_t)__popcll(claimed));
        at = (uint32_t)__shfl((int)at, 0) + (uint32_t)__popcll(claimed & ((1ull << lane) - 1ull));
        if (tag != 0ull && at < np) job.sort[at] = (tag & 0xffffffff00000000ull) | i;
        if (i >= n && i < np) job.sort[i] = ~0ull;              // (np <= 2 n <= slots)
    }
}

// The strides of the bitonic network that fit a tile, fused in LDS: the steps j = min(k / 2, tile / 2) ... 1 of every stage
// k = k_lo, 2 k_lo, ... k_hi (k_lo == 2: a tile sorted from scratch; k_lo == k_hi > CENSUS_WIDE_TILE: the tail of stage k behind
// its global steps).  An element's direction is decided by its index in the whole buffer.
__global__ __launch_bounds__(1024) void census_sort_tile_kernel(const CensusJob *__restrict__ jobs, uint32_t k_lo, uint32_t k_hi)
{
    const CensusJob job = jobs[blockIdx.y];
    uint32_t n, np;
    if (!census_wide_sizes(job, n, np) || np < k_lo) return;
    __shared__ unsigned long long lds[CENSUS_WIDE_TILE];
    const uint32_t tile = np < CENSUS_WIDE_TILE ? np : CENSUS_WIDE_TILE;
    for (uint32_t t0 = blockIdx.x * tile; t0 < np; t0 += gridDim.x * tile) {     // (np <= 2^24 and the grid has at most np / tile workgroups)
        for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) lds[i] = job.sort[t0 + i];
        __syncthreads();
        for (uint32_t k = k_lo; k <= k_hi && k <= np; k <<= 1) {
            for (uint32_t j = (k >> 1) < (tile >> 1) ? (k >> 1) : (tile >> 1); j > 0; j >>= 1) {
                for (uint32_t i = threadIdx.x; i < tile / 2; i += blockDim.x) {
                    const uint32_t a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a + j;
                    const unsigned long long x = lds[a], y = lds[b];
                    if ((x > y) == (((t0 + a) & k) == 0u)) { lds[a] = y; lds[b] = x; }
                }
                __syncthreads();
            }
        }
        for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) job.sort[t0 + i] = lds[i];
        __syncthreads();
    }
}

// One step (stage k, stride j >= CENSUS_WIDE_TILE) over the whole buffer: every pair belongs to one thread of one launch.
__global__ __launch_bounds__(256) void census_sort_step_kernel(const CensusJob *__restrict__ jobs, uint32_t k, uint32_t j)
{
    const CensusJob job = jobs[blockIdx.y];
    uint32_t n, np;
    if (!census_wide_sizes(job, n, np) || np < k) return;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < np / 2; i += gridDim.x * blockDim.x) {
        const uint32_t a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a + j;
        const unsigned long long x = job.sort[a], y = job.sort[b];
        if ((x > y) == ((a & k) == 0u)) { job.sort[a] = y; job.sort[b] = x; }
    }
}

// The keys, their counts and the result.
__global__ __launch_bounds__(256) void census_write_kernel(const CensusJob *__restrict__ jobs)
{
    const CensusJob job = jobs[blockIdx.y];
    uint32_t n, np;
    const bool fits = census_wide_sizes(job, n, np);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        spng_result r;
        r.status = fits ? SPNG_DONE : SPNG_E_OUTPUT_CAPACITY; r.reserved = 0; r.written = fits ? n : 0; r.consumed = fits ? job.count : 0;
        r.aux[0] = 0; r.aux[1] = 0;
        *job.result = r;
    }
    if (!fits) return;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long e = job.sort[i];
        job.keys[i] = (uint32_t)(e >> 32);
        if (job.out_counts) job.out_counts[i] = job.counts[(uint32_t)e & (job.slots - 1)];
    }
}

// ---- map ------------------------------------------------------------------------------------------------------------------------
// A table of key -> position in d_keys, open addressing, load <= 1/2.  A slot: 0: empty, else key << 32 | 1 << 31 | position
// (positions stay below 2^24), so that neither key 0x00000000 nor key 0xFFFFFFFF looks empty.  A key that d_keys holds twice takes
// one slot -- every insertion of it walks the same slots, and a slot never becomes empty again -- and keeps its lowest position.
__device__ __forceinline__ void map_insert(unsigned long long *table, uint32_t slots, uint32_t h, uint32_t key, uint32_t position)
{
    const unsigned long long mine = (unsigned long long)key << 32 | 0x80000000u | position;
    for (uint32_t step = 0; step < slots; ++step, h = (h + 1) & (slots - 1)) {
        const unsigned long long old = atomicCAS(table + h, 0ull, mine);
        if (old == 0ull) return;
        if ((uint32_t)(old >> 32) == key) { atomicMin(table + h, mine); return; }
    }
}

// -> the position of `key`, or ~0u
__device__ __forceinline__ uint32_t map_find(const unsigned long long *table, uint32_t slots, uint32_t h, uint32_t key)
{
    for (uint32_t step = 0; step < slots; ++step, h = (h + 1) & (slots - 1)) {
        const unsigned long long e = table[h];
        if (e == 0ull) break;
        if ((uint32_t)(e >> 32) == key) return (uint32_t)e & 0x7fffffffu;
    }
    return ~0u;
}

// The tables of the maps above MAP_LDS_KEYS keys (job.slots != 0), in scratch the host zeroed; the lookups are the next launch.
__global__ __launch_bounds__(256) void map_build_kernel(const MapJob *__restrict__ jobs, unsigned long long *__restrict__ scratch)
{
    const MapJob job = jobs[blockIdx.y];
    if (!job.slots) return;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < job.map_count; i += gridDim.x * blockDim.x) {
        const uint32_t key = job.keys[i];
        map_insert(scratch + job.table_off, job.slots, index_hash(key) >> (32 - job.slot_bits), key, i);
    }
}

__device__ __forceinline__ unsigned long long map_value(const void *values, uint32_t position, uint32_t value_bytes)
{
    switch (value_bytes) {
    case 1: return ((const uint8_t *)values)[position];
    case 2: return ((const uint16_t *)values)[position];
    case 4: return ((const uint32_t *)values)[position];
    default: return ((const unsigned long long *)values)[position];
    }
}

// The values of the quad at pixel i0 (m of them), as wide as the output's alignment allows (`wide`: d_out is aligned to a quad of
// values, 16 bytes at most; it always is to one value).
__device__ __forceinline__ void map_store(void *out, uint64_t i0, uint32_t m, bool wide, uint32_t value_bytes, const unsigned long long (&v)[4])
{
    if (m == 4 && wide) {
        switch (value_bytes) {
        case 1: *((uint32_t *)out + i0 / 4) = (uint32_t)(v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24); break;
        case 2: { v2u w; w[0] = (uint32_t)(v[0] | v[1] << 16); w[1] = (uint32_t)(v[2] | v[3] << 16); *((v2u *)out + i0 / 4) = w; break; }
        case 4: { v4u w; w[0] = (uint32_t)v[0]; w[1] = (uint32_t)v[1]; w[2] = (uint32_t)v[2]; w[3] = (uint32_t)v[3]; *((v4u *)out + i0 / 4) = w; break; }
        default: {
            v4u w;
            w[0] = (uint32_t)v[0]; w[1] = (uint32_t)(v[0] >> 32); w[2] = (uint32_t)v[1]; w[3] = (uint32_t)(v[1] >> 32); *((v4u *)out + i0 / 2) = w;
            w[0] = (uint32_t)v[2]; w[1] = (uint32_t)(v[2] >> 32); w[2] = (uint32_t)v[3]; w[3] = (uint32_t)(v[3] >> 32); *((v4u *)out + i0 / 2 + 1) = w;
        }
        }
        return;
    }
    for (uint32_t k = 0; k < m; ++k) {
        switch (value_bytes) {
        case 1: ((uint8_t *)out)[i0 + k] = (uint8_t)v[k]; break;
        case 2: ((uint16_t *)out)[i0 + k] = (uint16_t)v[k]; break;
        case 4: ((uint32_t *)out)[i0 + k] = (uint32_t)v[k]; break;
        default: ((unsigned long long *)out)[i0 + k] = v[k];
        }
    }
}

template <typename T, int LAYOUT>
__device__ __forceinline__ void map_run(const MapJob &job, const unsigned long long *table, uint32_t slots, uint32_t slot_bits, uint32_t &missed)
{
    const T *in = (const T *)job.pixels;
    const uint64_t n = job.count, quads = (n + 3) / 4;
    const uint32_t quad_bytes = 4u * job.value_bytes;
    const bool vec = quad_aligned<T, LAYOUT>(job.pixels), wide = ((uintptr_t)job.out & ((quad_bytes < 16 ? quad_bytes : 16) - 1)) == 0;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i0 = q * 4;
        const uint32_t m = n - i0 < 4 ? (uint32_t)(n - i0) : 4u;
        uint32_t key[4], miss[4] = {0, 0, 0, 0};
        unsigned long long v[4] = {0, 0, 0, 0};
        quad_keys<T, LAYOUT>(in, i0, m, vec, job.premultiply, key);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (k >= m) continue;
            if (k && key[k] == key[k - 1]) { v[k] = v[k - 1]; miss[k] = miss[k - 1]; }    // a run of equal pixels is looked up once
            else {
                const uint32_t at = map_find(table, slots, index_hash(key[k]) >> (32 - slot_bits), key[k]);
                miss[k] = at >= job.map_count;                  // (~0u; a position read from the table is below map_count)
                v[k] = miss[k] ? job.miss : map_value(job.values, at, job.value_bytes);
            }
            missed += miss[k];
        }
        map_store(job.out, i0, m, wide, job.value_bytes, v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void map_kernel(const MapJob *__restrict__ jobs, const unsigned long long *__restrict__ scratch)
{
    const MapJob job = jobs[blockIdx.y];
    if ((uint64_t)blockIdx.x * blockDim.x >= (job.count + 3) / 4) return;       // (the grid is sized for the longest array)
    __shared__ unsigned long long lds[MAP_LDS_SLOTS];
    __shared__ uint32_t block_missed;
    const bool in_lds = job.slots == 0;
    static_assert(MAP_LDS_SLOTS == 1u << 11 && MAP_LDS_SLOTS >= 4 * MAP_LDS_KEYS, "the shifts below; the load of the LDS table");
    if (threadIdx.x == 0) block_missed = 0;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < MAP_LDS_SLOTS; i += blockDim.x) lds[i] = 0ull;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < job.map_count; i += blockDim.x) {
            const uint32_t key = job.keys[i];
            map_insert(lds, MAP_LDS_SLOTS, index_hash(key) >> 21, key, i);
        }
    }
    __syncthreads();
    const unsigned long long *table = in_lds ? lds : scratch + job.table_off;
    const uint32_t slots = in_lds ? MAP_LDS_SLOTS : job.slots, slot_bits = in_lds ? 11u : job.slot_bits;
    uint32_t missed = 0;
    if (job.layout == 0) map_run<T, 0>(job, table, slots, slot_bits, missed);
    else if (job.layout == 1) map_run<T, 1>(job, table, slots, slot_bits, missed);
    else map_run<T, 2>(job, table, slots, slot_bits, missed);
    // the misses: summed per wave, added once per workgroup
#pragma unroll
    for (int s = 32; s; s >>= 1) missed += (uint32_t)__shfl_xor((int)missed, s);
    if ((threadIdx.x & 63) == 0 && missed) atomicAdd(&block_missed, missed);
    __syncthreads();
    if (threadIdx.x == 0 && block_missed) atomicAdd((unsigned long long *)&job.result->aux[0], (unsigned long long)block_missed);
}

// slots of the scratch table of a map of map_count keys; 0: the map sits in LDS
uint32_t map_slots(uint32_t map_count)
{
    if (map_count <= MAP_LDS_KEYS) return 0;
    uint32_t s = MAP_MIN_SLOTS;
    while (s < 2 * (uint64_t)map_count) s <<= 1;
    return s;
}

// Behind census_kernel (launch_census_count) and the host's look at the counters: gather, sort, write.  most_slots: the largest
// table; most_keys: the most keys found in an array that did not overflow (0: none did not).
hipError_t launch_census_wide_finish(const CensusJob *d_jobs, uint32_t count, uint32_t most_slots, uint32_t most_keys, hipStream_t stream)
{
    if (!count) return hipSuccess;
    uint32_t np = 1;
    while (np < most_keys) np <<= 1;
    const uint32_t tiles = np <= CENSUS_WIDE_TILE ? 1 : np / CENSUS_WIDE_TILE;
    const uint32_t gx_gather = (most_slots + 4095) / 4096 < 4096 ? (most_slots + 4095) / 4096 : 4096;   // (16 slots per thread at least)
    const uint32_t gx_tiles = tiles < 4096 ? tiles : 4096, gx_step = np / 2048 < 4096 ? (np / 2048 ? np / 2048 : 1) : 4096;   // (4 pairs per thread at least)
    const uint32_t gx_write = (most_keys + 1023) / 1024 < 4096 ? (most_keys + 1023) / 1024 : 4096;
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        if (most_keys) {
            census_gather_kernel<<<dim3(gx_gather ? gx_gather : 1, ny), 256, 0, stream>>>(d_jobs + y0);
            census_sort_tile_kernel<<<dim3(gx_tiles, ny), 1024, 0, stream>>>(d_jobs + y0, 2u, CENSUS_WIDE_TILE);
            for (uint32_t k = 2 * CENSUS_WIDE_TILE; k <= np && k; k <<= 1) {
                for (uint32_t j = k >> 1; j >= CENSUS_WIDE_TILE; j >>= 1)
                    census_sort_step_kernel<<<dim3(gx_step, ny), 256, 0, stream>>>(d_jobs + y0, k, j);
                census_sort_tile_kernel<<<dim3(gx_tiles, ny), 1024, 0, stream>>>(d_jobs + y0, k, k);
            }
        }
        census_write_kernel<<<dim3(gx_write ? gx_write : 1, ny), 256, 0, stream>>>(d_jobs + y0);
    });
}

// build_blocks_x: 0: every map of the call sits in LDS, no build launch
hipError_t launch_map(const MapJob *d_jobs, uint32_t count, unsigned long long *d_scratch, uint32_t build_blocks_x, uint32_t blocks_x,
                      int source, hipStream_t stream)
{
    if (!count) return hipSuccess;
    return launch_rows(count, [&](uint32_t y0, uint32_t ny) {
        const dim3 grid(blocks_x ? blocks_x : 1, ny);
        if (build_blocks_x) map_build_kernel<<<dim3(build_blocks_x, ny), 256, 0, stream>>>(d_jobs + y0, d_scratch);
        if (source == 8) map_kernel<uint8_t><<<grid, 256, 0, stream>>>(d_jobs + y0, d_scratch);
        else map_kernel<uint16_t><<<grid, 256, 0, stream>>>(d_jobs + y0, d_scratch);
    });
}

}  // namespace spng
