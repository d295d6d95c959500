// emu_indexing.cpp -- TEST INFRASTRUCTURE: runs census_kernel, census_finish_kernel and pack_indexed_kernel of csrc/indexing.hip on
// the CPU (tools/emu/hip/hip_runtime.h; host compiler clang++) against std::map over keys computed with the reference's formulas
// restated with plain `/` (PNG.premultiply, Sources/PNG/PNG.swift:55-66; PNG.deconvolve's reduction to UInt8, :829-852).  From a
// prepared copy of the source (EMU_INDEXING_SRC); never part of the product.
//
//   emu_indexing census   sizes around the quad and the workgroup, flat and skewed arrays, exactly cap and cap + 1 keys, the keys 0 and
//                         0xFFFFFFFF, keys that differ in one byte only, more keys in a workgroup than its table may hold, the sort
//                         on both sides of its LDS limit, premultiplication, no counts, unaligned arrays
//   emu_indexing pack     sizes, storage offsets 0 .. 3, map sizes around every threshold, misses, many-to-one maps, premultiplication
#include EMU_INDEXING_SRC

#include <map>
#include <random>
#include <string>
#include <vector>

using namespace spng;

static uint32_t ref_premultiply(uint32_t c, uint32_t a, uint32_t M) { return (uint32_t)(((uint64_t)c * a + (M >> 1)) / M); }

// the key of one pixel of nc1 components of T (bits wide)
static uint32_t ref_key(const uint32_t *px, int layout, int bits, int premultiply)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    uint32_t c[4];
    for (int z = 0; z < nc1; ++z) c[z] = px[z];
    if (premultiply == SPNG_PREMULTIPLY) {
        for (int z = 0; z < nc1 - 1; ++z) c[z] = ref_premultiply(c[z], c[nc1 - 1], bits == 8 ? 255u : 65535u);
    } else if (premultiply == SPNG_PREMULTIPLY_AS_U8) {
        const uint32_t a8 = c[nc1 - 1] >> 8;
        for (int z = 0; z < nc1 - 1; ++z) c[z] = 257u * ref_premultiply(c[z] >> 8, a8, 255u);
        c[nc1 - 1] = 257u * a8;
    }
    uint32_t key = 0;
    for (int z = 0; z < nc1; ++z) key |= (c[z] >> (bits - 8)) << 8 * z;
    return key;
}

// pixels of T whose keys (without premultiplication) are `keys`; T = UInt16: random low bytes
template <typename T>
static std::vector<T> pixels_of(const std::vector<uint32_t> &keys, int layout, std::mt19937 &rng)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    std::vector<T> px;
    for (uint32_t k : keys)
        for (int z = 0; z < nc1; ++z) {
            const uint32_t c = (k >> 8 * z) & 255;
            px.push_back(sizeof(T) == 1 ? (T)c : (T)(c << 8 | (rng() & 255)));
        }
    return px;
}

static uint32_t layout_mask(int layout) { return layout == 0 ? 0xffffffffu : layout == 1 ? 0xffffu : 0xffu; }

template <typename T>
static std::vector<uint32_t> ref_keys(const std::vector<T> &px, int layout, int premultiply)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    std::vector<uint32_t> keys;
    for (size_t i = 0; i + nc1 <= px.size(); i += nc1) {
        uint32_t c[4] = {0, 0, 0, 0};
        for (int z = 0; z < nc1; ++z) c[z] = px[i + z];
        keys.push_back(ref_key(c, layout, (int)sizeof(T) * 8, premultiply));
    }
    return keys;
}

template <typename T>
static bool census(const char *what, const std::vector<T> &px, int layout, int premultiply, uint32_t cap, unsigned grid, bool with_counts = true,
                   size_t offset = 0)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    const size_t count = px.size() / nc1;
    std::vector<uint8_t> raw(px.size() * sizeof(T) + 64 + offset);
    uint8_t *in = raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15) + offset;
    memcpy(in, px.data(), px.size() * sizeof(T));
    CensusJob job;
    memset(&job, 0, sizeof job);
    job.cap = cap; job.slots = census_slots(cap);
    for (job.slot_bits = 0; (1u << job.slot_bits) < job.slots; ++job.slot_bits) {}
    std::vector<unsigned long long> tags(job.slots, 0), counts(job.slots, 0), sort(census_sort_elems(cap), 0xABABABABABABABABull);
    std::vector<uint32_t> keys(cap + 8, 0xEEEEEEEEu);
    std::vector<uint64_t> outc(cap + 8, 0xEEEEEEEEEEEEEEEEull);
    uint32_t ctrl[2] = {0, 0};
    spng_result res;
    memset(&res, 0xCC, sizeof res);
    job.pixels = in; job.count = count; job.keys = keys.data(); job.out_counts = with_counts ? outc.data() : nullptr;
    job.tags = tags.data(); job.counts = counts.data(); job.ctrl = ctrl; job.sort = sort.data(); job.result = &res;
    job.layout = (uint8_t)layout; job.premultiply = (uint8_t)premultiply;
    emu::launch(grid, 256, [&] { census_kernel<T>(&job); }, 1);
    emu::launch(1, 1024, [&] { census_finish_kernel(&job); }, 1);
    std::map<uint32_t, uint64_t> want;
    for (uint32_t k : ref_keys(px, layout, premultiply)) ++want[k];
    if (want.size() > cap) {
        if (res.status != SPNG_E_OUTPUT_CAPACITY || res.written != 0) {
            printf("%s: %zu keys at cap %u: status %d, written %llu\n", what, want.size(), cap, res.status, (unsigned long long)res.written);
            return false;
        }
        return true;
    }
    if (res.status != SPNG_DONE || res.written != want.size() || res.consumed != count) {
        printf("%s: layout %d: status %d, written %llu (want %zu), consumed %llu\n", what, layout, res.status, (unsigned long long)res.written,
               want.size(), (unsigned long long)res.consumed);
        return false;
    }
    size_t i = 0;
    for (auto &kv : want) {
        if (keys[i] != kv.first || (with_counts && outc[i] != kv.second)) {
            printf("%s: layout %d: entry %zu is (%08x, %llu), want (%08x, %llu)\n", what, layout, i, keys[i], (unsigned long long)outc[i], kv.first,
                   (unsigned long long)kv.second);
            return false;
        }
        ++i;
    }
    for (; i < keys.size(); ++i)
        if (keys[i] != 0xEEEEEEEEu || outc[i] != 0xEEEEEEEEEEEEEEEEull) { printf("%s: entry %zu behind the result was written\n", what, i); return false; }
    if (!with_counts) for (uint64_t c : outc) if (c != 0xEEEEEEEEEEEEEEEEull) { printf("%s: counts written though none were asked for\n", what); return false; }
    return true;
}

// n keys drawn from `set` (skew: the square of a uniform number picks the entry)
static std::vector<uint32_t> draw(const std::vector<uint32_t> &set, size_t n, std::mt19937 &rng, bool skew = false)
{
    std::vector<uint32_t> out(n);
    for (auto &k : out) {
        const double u = (rng() & 0xffffff) / (double)0x1000000;
        k = set[(size_t)((skew ? u * u : u) * set.size())];
    }
    return out;
}

static std::vector<uint32_t> distinct(size_t n, uint32_t mask, std::mt19937 &rng)
{
    std::map<uint32_t, int> seen;
    std::vector<uint32_t> out;
    while (out.size() < n) {
        const uint32_t k = (uint32_t)rng() & mask;
        if (!seen[k]++) out.push_back(k);
    }
    return out;
}

template <typename T>
static bool census_cases()
{
    std::mt19937 rng(sizeof(T));
    for (int layout = 0; layout < 3; ++layout) {
        const uint32_t mask = layout_mask(layout);
        const std::vector<uint32_t> few = distinct(layout == 2 ? 40 : 100, mask, rng);
        for (size_t n : {0, 1, 3, 4, 5, 259, 2051})
            for (unsigned grid : {1u, 3u})
                if (!census<T>("sizes", pixels_of<T>(draw(few, n, rng), layout, rng), layout, 0, 256, grid)) return false;
        if (!census<T>("unaligned", pixels_of<T>(draw(few, 777, rng), layout, rng), layout, 0, 256, 2, true, sizeof(T) * (layout == 0 ? 4 : layout == 1 ? 2 : 1))) return false;
        if (!census<T>("flat", pixels_of<T>(std::vector<uint32_t>(20000, 0x80FF8040u & mask), layout, rng), layout, 0, 4, 4)) return false;
        if (!census<T>("no counts", pixels_of<T>(draw(few, 3000, rng), layout, rng), layout, 0, 256, 2, false)) return false;
        // the keys nothing may be reserved for, and keys that differ in one byte only
        {
            std::vector<uint32_t> set = {0u, mask, 1u, mask - 1};
            if (!census<T>("0 and ~0", pixels_of<T>(draw(set, 1500, rng), layout, rng), layout, 0, 4, 2)) return false;
            if (!census<T>("only ~0", pixels_of<T>(std::vector<uint32_t>(300, mask), layout, rng), layout, 0, 1, 1)) return false;
            if (!census<T>("only 0", pixels_of<T>(std::vector<uint32_t>(300, 0u), layout, rng), layout, 0, 1, 1)) return false;
        }
        for (int s = 0; s < (layout == 0 ? 32 : layout == 1 ? 16 : 8); s += 8) {
            std::vector<uint32_t> set;
            for (uint32_t k = 0; k < 256; ++k) set.push_back(k << s);
            std::vector<uint32_t> ks = set;
            for (uint32_t k : draw(set, 1000, rng)) ks.push_back(k);
            if (!census<T>("k << s", pixels_of<T>(ks, layout, rng), layout, 0, 256, 2)) return false;
        }
        // exactly cap and cap + 1 keys
        for (uint32_t cap : {1u, 200u, 256u}) {
            if (cap + 1 > (uint64_t)mask + 1) continue;
            for (uint32_t extra : {0u, 1u}) {
                std::vector<uint32_t> set = distinct(cap + extra, mask, rng), ks = set;
                for (uint32_t k : draw(set, 700, rng)) ks.push_back(k);
                if (!census<T>("cap", pixels_of<T>(ks, layout, rng), layout, 0, cap, 2)) return false;
            }
        }
        if (layout == 2) continue;
        // more keys in one workgroup than its table may hold, then the same keys again (the merge into the image's table); the sort
        // on both sides of its LDS limit; an overflow that workgroups see while they read
        for (uint32_t nk : {CENSUS_LDS_LIMIT + 1, 3000u, CENSUS_FINISH_LDS_KEYS, CENSUS_FINISH_LDS_KEYS + 1, 5000u}) {
            std::vector<uint32_t> set = distinct(nk, mask, rng), ks = set;
            for (uint32_t k : set) ks.push_back(k);
            for (uint32_t k : draw(set, 2000, rng, true)) ks.push_back(k);
            for (unsigned grid : {1u, 3u})
                if (!census<T>("merge", pixels_of<T>(ks, layout, rng), layout, 0, 8192, grid)) return false;
            if (!census<T>("overflow", pixels_of<T>(ks, layout, rng), layout, 0, nk - 1, 2)) return false;
            if (!census<T>("overflow far", pixels_of<T>(ks, layout, rng), layout, 0, 16, 3)) return false;
        }
        // premultiplied keys
        {
            std::vector<T> px(4000 * (layout == 0 ? 4 : 2));
            for (auto &c : px) c = (T)rng();
            if (!census<T>("premultiply", px, layout, SPNG_PREMULTIPLY, 8192, 2)) return false;
            if (sizeof(T) == 2 && !census<T>("premultiply as u8", px, layout, SPNG_PREMULTIPLY_AS_U8, 8192, 2)) return false;
        }
    }
    return true;
}

template <typename T>
static bool pack(const char *what, const std::vector<T> &px, int layout, int premultiply, std::vector<uint32_t> keys, const std::vector<uint8_t> &indices_of_unsorted,
                 uint32_t miss, unsigned grid, size_t storage_offset)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    const size_t count = px.size() / nc1;
    std::map<uint32_t, uint8_t> map;
    for (size_t j = 0; j < keys.size(); ++j) map[keys[j]] = indices_of_unsorted[j];
    std::vector<uint32_t> skeys;
    std::vector<uint8_t> sidx;
    for (auto &kv : map) { skeys.push_back(kv.first); sidx.push_back(kv.second); }
    std::vector<uint8_t> raw(px.size() * sizeof(T) + 64), sto(count + 64 + 8, 0xEE);
    uint8_t *in = raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15);
    uint8_t *out = sto.data() + ((4 - ((uintptr_t)sto.data() & 3)) & 3) + 4 + storage_offset;
    memcpy(in, px.data(), px.size() * sizeof(T));
    spng_result res;
    memset(&res, 0, sizeof res);
    PackIndexedJob job;
    memset(&job, 0, sizeof job);
    job.pixels = in; job.storage = out; job.keys = skeys.data(); job.indices = sidx.data(); job.result = &res;
    job.width = (uint32_t)count; job.height = 1; job.map_count = (uint32_t)skeys.size();
    job.layout = (uint8_t)layout; job.premultiply = (uint8_t)premultiply; job.miss = (uint8_t)miss;
    emu::launch(grid, 256, [&] { pack_indexed_kernel<T>(&job); }, 1);
    uint64_t missed = 0;
    const std::vector<uint32_t> pk = ref_keys(px, layout, premultiply);
    for (size_t i = 0; i < count; ++i) {
        auto it = map.find(pk[i]);
        const uint8_t want = it == map.end() ? (uint8_t)miss : it->second;
        missed += it == map.end();
        if (out[i] != want) { printf("%s: layout %d, %zu keys: pixel %zu (key %08x) stored %u, want %u\n", what, layout, skeys.size(), i, pk[i], out[i], want); return false; }
    }
    for (int k = 1; k <= 4; ++k)
        if (out[-k] != 0xEE || out[count + k - 1] != 0xEE) { printf("%s: a byte beside the storage was written\n", what); return false; }
    if (res.aux[0] != missed) { printf("%s: %llu misses counted, %llu expected\n", what, (unsigned long long)res.aux[0], (unsigned long long)missed); return false; }
    return true;
}

template <typename T>
static bool pack_cases()
{
    std::mt19937 rng(40 + sizeof(T));
    for (int layout = 0; layout < 3; ++layout) {
        const uint32_t mask = layout_mask(layout);
        auto indices = [&](size_t n, uint32_t modulo) { std::vector<uint8_t> v(n); for (auto &b : v) b = (uint8_t)(rng() % modulo); return v; };
        const std::vector<uint32_t> few = distinct(layout == 2 ? 40 : 100, mask, rng);
        for (size_t n : {0, 1, 3, 4, 5, 259, 2051})
            for (size_t off = 0; off < 4; ++off) {
                // half of the map's keys occur, half of the pixels' keys are in the map
                std::vector<uint32_t> keys(few.begin(), few.begin() + few.size() / 2);
                for (uint32_t k : distinct(20, mask, rng)) keys.push_back(k);
                if (!pack<T>("sizes", pixels_of<T>(draw(few, n, rng), layout, rng), layout, 0, keys, indices(keys.size(), 256), 7, n > 1024 ? 3 : 1, off)) return false;
            }
        // map sizes around every threshold
        for (uint32_t mc : {0u, 1u, 255u, 256u, 257u, PACK_INDEXED_LDS_KEYS - 1, PACK_INDEXED_LDS_KEYS, PACK_INDEXED_LDS_KEYS + 1, 65536u}) {
            if (mc > (uint64_t)mask + 1) continue;
            std::vector<uint32_t> keys = distinct(mc, mask, rng), ks = keys;
            for (uint32_t k : distinct(50, mask, rng)) ks.push_back(k);
            if (!pack<T>("map sizes", pixels_of<T>(draw(ks, 3000, rng), layout, rng), layout, 0, keys, indices(mc, 5), 200, 2, 1)) return false;
        }
        // the keys 0 and ~0, in the map and not
        for (int present = 0; present < 2; ++present)
            for (uint32_t extra : {10u, PACK_INDEXED_LDS_KEYS + 10}) {
                if (extra > mask) continue;
                std::vector<uint32_t> keys = distinct(extra, mask - 2, rng), ks;
                for (auto &k : keys) k += 1;
                ks = keys; ks.push_back(0u); ks.push_back(mask);
                if (present) { keys.push_back(0u); keys.push_back(mask); }
                if (!pack<T>("0 and ~0", pixels_of<T>(draw(ks, 1200, rng), layout, rng), layout, 0, keys, indices(keys.size(), 256), 99, 1, 0)) return false;
            }
        if (layout == 2) {
            // the tutorial's indexer: Int.init
            std::vector<uint32_t> keys(256);
            std::vector<uint8_t> idx(256);
            for (uint32_t k = 0; k < 256; ++k) { keys[k] = k; idx[k] = (uint8_t)k; }
            if (!pack<T>("identity", pixels_of<T>(draw(keys, 2000, rng), layout, rng), layout, 0, keys, idx, 0, 2, 0)) return false;
            continue;
        }
        std::vector<T> px(3000 * (layout == 0 ? 4 : 2));
        for (auto &c : px) c = (T)rng();
        for (int premultiply : {SPNG_PREMULTIPLY, SPNG_PREMULTIPLY_AS_U8}) {
            if (premultiply == SPNG_PREMULTIPLY_AS_U8 && sizeof(T) == 1) continue;
            std::vector<uint32_t> all = ref_keys(px, layout, premultiply), keys;
            std::map<uint32_t, int> seen;
            for (size_t i = 0; i < all.size(); i += 2) if (!seen[all[i]]++) keys.push_back(all[i]);
            if (!pack<T>("premultiply", px, layout, premultiply, keys, indices(keys.size(), 256), 3, 2, 2)) return false;
        }
    }
    return true;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "census") {
        if (!census_cases<uint8_t>() || !census_cases<uint16_t>()) return 1;
        printf("ok\n");
        return 0;
    }
    if (mode == "pack") {
        if (!pack_cases<uint8_t>() || !pack_cases<uint16_t>()) return 1;
        printf("ok\n");
        return 0;
    }
    fprintf(stderr, "usage: emu_indexing census | pack\n");
    return 2;
}
