// emu_colour_tables.cpp -- TEST INFRASTRUCTURE: runs the kernels of csrc/colour_tables.hip (census_gather_kernel, census_sort_tile_kernel,
// census_sort_step_kernel, census_write_kernel behind census_kernel of csrc/indexing.hip; map_build_kernel, map_kernel) on the CPU
// (tools/emu/hip/hip_runtime.h; host compiler clang++) against std::map, over the rules of tests/colour_table_cases.py up to 131 073
// keys.  Every launch of a multi-launch stage is an emulated launch of its own, in the order launch_census_wide_finish / launch_map
// enqueue them; every output lies between guard bytes, and every scratch array has exactly the size the host gives it, so that the
// sanitizer build (tests/test_emu_colour_tables.py) sees a step beyond it.  From prepared copies of the sources (EMU_INDEXING_SRC,
// EMU_COLOUR_TABLES_SRC); never part of the product.
//
//   emu_colour_tables census   key counts around the tile and the old ceiling up to 131 073, exactly cap and cap + 1 on both sides of 65 536 with
//                              the overflow seen early and late, the keys 0 and 0xFFFFFFFF, keys that differ in one byte, a count above 2^16,
//                              heavy duplication, unaligned arrays, a count of 0, a cap far above the count, layouts and premultiplications
//   emu_colour_tables map      map sizes around every threshold up to 131 073, values of 1 / 2 / 4 / 8 bytes, the keys 0 and 0xFFFFFFFF
//                              present and absent, every pixel missing, output offsets, runs of equal pixels, a duplicated key
#include EMU_INDEXING_SRC
#include EMU_COLOUR_TABLES_SRC

#include <map>
#include <random>
#include <string>
#include <vector>

using namespace spng;

static uint32_t ref_premultiply(uint32_t c, uint32_t a, uint32_t M) { return (uint32_t)(((uint64_t)c * a + (M >> 1)) / M); }

// the key of one pixel of nc1 components of T (bits wide): PNG.premultiply, Sources/PNG/PNG.swift:55-66, PNG.deconvolve's reduction, :829-852
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

template <typename T>
static std::vector<T> pixels_of(const std::vector<uint32_t> &keys, int layout, std::mt19937 &rng)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    std::vector<T> px;
    px.reserve(keys.size() * nc1);
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
    keys.reserve(px.size() / nc1);
    for (size_t i = 0; i + nc1 <= px.size(); i += nc1) {
        uint32_t c[4] = {0, 0, 0, 0};
        for (int z = 0; z < nc1; ++z) c[z] = px[i + z];
        keys.push_back(ref_key(c, layout, (int)sizeof(T) * 8, premultiply));
    }
    return keys;
}

static std::vector<uint32_t> distinct(size_t n, uint32_t mask, std::mt19937 &rng, uint32_t lo = 0, uint32_t span = 0)
{
    std::map<uint32_t, int> seen;
    std::vector<uint32_t> out;
    while (out.size() < n) {
        const uint32_t k = span ? lo + (uint32_t)(rng() % span) : (uint32_t)rng() & mask;
        if (!seen[k]++) out.push_back(k);
    }
    return out;
}

static std::vector<uint32_t> draw(const std::vector<uint32_t> &set, size_t n, std::mt19937 &rng)
{
    std::vector<uint32_t> out(n);
    for (auto &k : out) k = set[rng() % set.size()];
    return out;
}

static uint32_t pow2(uint32_t n) { uint32_t p = 1; while (p < n) p <<= 1; return p; }

// ---- wide census -----------------------------------------------------------------------------------------------------------------
template <typename T>
static bool census(const char *what, const std::vector<T> &px, int layout, int premultiply, uint32_t cap, unsigned grid, bool with_counts = true,
                   size_t offset = 0)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    const size_t count = px.size() / nc1;
    std::vector<uint8_t> raw(px.size() * sizeof(T) + 32 + offset);
    uint8_t *in = raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15) + offset;
    if (!px.empty()) memcpy(in, px.data(), px.size() * sizeof(T));
    // the scratch spng_census_wide_batch gives an array: sized by min(cap, count), not by cap
    const uint32_t most = (uint32_t)std::min<uint64_t>(cap, count ? count : 1);
    CensusJob job;
    memset(&job, 0, sizeof job);
    job.cap = cap; job.slots = census_slots(most);
    for (job.slot_bits = 0; (1u << job.slot_bits) < job.slots; ++job.slot_bits) {}
    std::vector<unsigned long long> tags(job.slots, 0), counts(job.slots, 0), sort(census_sort_elems(most), 0xABABABABABABABABull);
    std::vector<uint32_t> keys(most + 8, 0xEEEEEEEEu);
    std::vector<uint64_t> outc(most + 8, 0xEEEEEEEEEEEEEEEEull);
    std::vector<uint32_t> ctrl(64, 0);
    spng_result res;
    memset(&res, 0xCC, sizeof res);
    job.pixels = in; job.count = count; job.keys = keys.data(); job.out_counts = with_counts ? outc.data() : nullptr;
    job.tags = tags.data(); job.counts = counts.data(); job.ctrl = ctrl.data(); job.sort = sort.data(); job.result = &res;
    job.layout = (uint8_t)layout; job.premultiply = (uint8_t)premultiply;
    emu::launch(grid, 256, [&] { census_kernel<T>(&job); }, 1);
    // what the host does behind its one wait (launch_census_wide_finish)
    const bool fits = !ctrl[1] && ctrl[0] <= cap;
    const uint32_t found = fits ? ctrl[0] : 0, np = pow2(found);
    unsigned launches = 0;
    if (found) {
        const unsigned tiles = np <= CENSUS_WIDE_TILE ? 1 : np / CENSUS_WIDE_TILE;
        emu::launch(std::min<unsigned>((job.slots + 4095) / 4096, 3), 256, [&] { census_gather_kernel(&job); }, 1);
        emu::launch(std::min(tiles, 3u), 1024, [&] { census_sort_tile_kernel(&job, 2u, CENSUS_WIDE_TILE); }, 1); ++launches;
        for (uint32_t k = 2 * CENSUS_WIDE_TILE; k <= np; k <<= 1) {
            for (uint32_t j = k >> 1; j >= CENSUS_WIDE_TILE; j >>= 1) { emu::launch(2, 256, [&] { census_sort_step_kernel(&job, k, j); }, 1); ++launches; }
            emu::launch(std::min(tiles, 5u), 1024, [&] { census_sort_tile_kernel(&job, k, k); }, 1); ++launches;
        }
    }
    emu::launch(found > 3000 ? 3 : 1, 256, [&] { census_write_kernel(&job); }, 1);
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
    // the launches the binding's census_wide_sort_launches promises
    unsigned promised = 1;
    for (uint32_t k = 2 * CENSUS_WIDE_TILE; k <= np; k <<= 1) { for (uint32_t j = k >> 1; j >= CENSUS_WIDE_TILE; j >>= 1) ++promised; ++promised; }
    if (found && launches != promised) { printf("%s: %u sort launches, %u promised\n", what, launches, promised); return false; }
    return true;
}

// nk distinct keys and `extra` repeats: the distinct ones first, or pixels of one colour first and the keys last
template <typename T>
static std::vector<T> spread(size_t nk, size_t extra, bool front, int layout, std::mt19937 &rng)
{
    std::vector<uint32_t> set = distinct(nk, layout_mask(layout), rng), ks;
    if (front) { ks = set; for (uint32_t k : draw(set, extra, rng)) ks.push_back(k); }
    else { ks.assign(extra, set[0]); for (uint32_t k : set) ks.push_back(k); }
    return pixels_of<T>(ks, layout, rng);
}

template <typename T>
static bool census_cases(bool large, bool brief)
{
    std::mt19937 rng(100 + sizeof(T));
    for (int layout = 0; layout < 3; ++layout) {
        const uint32_t mask = layout_mask(layout);
        const std::vector<uint32_t> few = distinct(layout == 2 ? 40 : 100, mask, rng);
        if (!census<T>("empty", std::vector<T>(), layout, 0, 16, 1)) return false;
        for (size_t n : {1, 3, 5, 259, 2051})
            if (!census<T>("sizes", pixels_of<T>(draw(few, n, rng), layout, rng), layout, 0, 256, n > 1024 ? 3 : 1)) return false;
        if (!census<T>("cap far above", pixels_of<T>(draw(few, 5, rng), layout, rng), layout, 0, SPNG_CENSUS_WIDE_CAP, 1)) return false;
        for (size_t off = sizeof(T); off < 16; off += (sizeof(T) == 1 && layout == 0 ? 1 : 5 * sizeof(T)))
            if (!census<T>("unaligned", pixels_of<T>(draw(few, 777, rng), layout, rng), layout, 0, 256, 2, true, off)) return false;
        if (!census<T>("no counts", pixels_of<T>(draw(few, 3000, rng), layout, rng), layout, 0, 3000, 2, false)) return false;
        {
            std::vector<uint32_t> set = {0u, mask};
            if (!census<T>("0 and ~0", pixels_of<T>(draw(set, 700, rng), layout, rng), layout, 0, 2, 2)) return false;
            if (!census<T>("only ~0", pixels_of<T>(std::vector<uint32_t>(300, mask), layout, rng), layout, 0, 3, 1)) return false;
            if (!census<T>("only 0", pixels_of<T>(std::vector<uint32_t>(300, 0u), layout, rng), layout, 0, 1, 1)) return false;
        }
        for (int s = 0; s < (layout == 0 ? 32 : layout == 1 ? 16 : 8); s += (layout == 0 ? 24 : 8)) {
            std::vector<uint32_t> set;
            for (uint32_t k = 0; k < 256; ++k) set.push_back(k << s);
            std::vector<uint32_t> ks = set;
            for (uint32_t k : draw(set, 1000, rng)) ks.push_back(k);
            if (!census<T>("k << s", pixels_of<T>(ks, layout, rng), layout, 0, 300, 2)) return false;
        }
        if (layout == 2) continue;
        {
            std::vector<T> px(3001 * (layout == 0 ? 4 : 2));
            for (auto &c : px) c = (T)rng();
            if (!census<T>("premultiply", px, layout, SPNG_PREMULTIPLY, 3001, 2)) return false;
            if (sizeof(T) == 2 && !census<T>("premultiply as u8", px, layout, SPNG_PREMULTIPLY_AS_U8, 3001, 2)) return false;
        }
        // the tile: one tile, two tiles and the first global stride
        for (uint32_t nk : {CENSUS_WIDE_TILE - 1, CENSUS_WIDE_TILE, CENSUS_WIDE_TILE + 1})
            if (!census<T>("tile", spread<T>(nk, 1500, true, layout, rng), layout, 0, nk + 7, 3)) return false;
    }
    if (!large) return true;
    // RGBA<T> only from here on: the sizes are about keys, not about layouts
    if (brief)                                                  // (the sanitizer build: one count above the old ceiling, its overflow seen late)
        return census<T>("distinct", spread<T>(65537, 1500, true, 0, rng), 0, 0, 65544, 4) &&
               census<T>("cap, seen late", spread<T>(65538, 3000, false, 0, rng), 0, 0, 65537, 4);
    if (!census<T>("flat 70000", pixels_of<T>(std::vector<uint32_t>(70000, 0x80FF8040u), 0, rng), 0, 0, 1, 4)) return false;
    for (uint32_t nk : {65535u, 65536u, 65537u, 131073u})
        if (!census<T>("distinct", spread<T>(nk, 1500, true, 0, rng), 0, 0, nk + 7, 4)) return false;
    for (uint32_t cap : {65535u, 65537u})
        for (uint32_t extra : {0u, 1u})
            for (bool front : {true, false})
                if (!census<T>(front ? "cap, seen early" : "cap, seen late", spread<T>(cap + extra, 3000, front, 0, rng), 0, 0, cap, 4)) return false;
    if (!census<T>("duplication", spread<T>(70000, 130000, true, 0, rng), 0, 0, 200000, 4)) return false;
    return true;
}

// ---- map -------------------------------------------------------------------------------------------------------------------------
static const uint64_t MISS = 0xF1E2D3C4B5A69788ull;            // (its bytes all differ)

// keys: ascending (one may be there twice); values: one per key, the low vb bytes count
template <typename T>
static bool map_case(const char *what, const std::vector<T> &px, int layout, int premultiply, const std::vector<uint32_t> &keys,
                     const std::vector<uint64_t> &values, int vb, unsigned grid, size_t out_offset)
{
    const int nc1 = layout == 0 ? 4 : layout == 1 ? 2 : 1;
    const size_t count = px.size() / nc1;
    const uint64_t vmask = vb == 8 ? ~0ull : (1ull << 8 * vb) - 1;
    std::vector<uint8_t> raw(px.size() * sizeof(T) + 32), vals(keys.size() * vb + 1), sto((count + out_offset) * vb + 96, 0xEE);
    uint8_t *in = raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15);
    uint8_t *out = sto.data() + ((16 - ((uintptr_t)sto.data() & 15)) & 15) + 32 + out_offset * vb;   // out_offset values behind a 16-byte boundary
    if (!px.empty()) memcpy(in, px.data(), px.size() * sizeof(T));
    for (size_t j = 0; j < keys.size(); ++j) memcpy(vals.data() + j * vb, &values[j], vb);
    std::vector<uint32_t> dkeys(keys);                          // (exactly map_count keys: a read beyond them is seen)
    spng_result res;
    memset(&res, 0, sizeof res);
    MapJob job;
    memset(&job, 0, sizeof job);
    job.pixels = in; job.out = out; job.keys = dkeys.data(); job.values = vals.data(); job.result = &res;
    job.count = count; job.miss = MISS & vmask; job.map_count = (uint32_t)keys.size();
    job.layout = (uint8_t)layout; job.premultiply = (uint8_t)premultiply; job.value_bytes = (uint8_t)vb;
    job.slots = map_slots(job.map_count);
    for (job.slot_bits = 0; job.slots && (1u << job.slot_bits) < job.slots; ++job.slot_bits) {}
    const size_t lead = 24;                                     // (another map's table in front of this one)
    job.table_off = job.slots ? lead : 0;
    std::vector<unsigned long long> scratch(job.slots ? lead + job.slots : 0, 0);
    for (size_t i = 0; i < lead && job.slots; ++i) scratch[i] = 0x7777777777777777ull;
    if (job.slots) emu::launch(2, 256, [&] { map_build_kernel(&job, scratch.data()); }, 1);
    emu::launch(grid, 256, [&] { map_kernel<T>(&job, scratch.data()); }, 1);
    for (size_t i = 0; i < lead && job.slots; ++i) if (scratch[i] != 0x7777777777777777ull) { printf("%s: the table in front was written\n", what); return false; }
    std::map<uint32_t, uint64_t> want;
    for (size_t j = keys.size(); j-- > 0;) want[keys[j]] = values[j] & vmask;      // (the lowest position last: it wins)
    uint64_t missed = 0;
    const std::vector<uint32_t> pk = ref_keys(px, layout, premultiply);
    for (size_t i = 0; i < count; ++i) {
        auto it = want.find(pk[i]);
        const uint64_t w = it == want.end() ? MISS & vmask : it->second;
        missed += it == want.end();
        uint64_t got = 0;
        memcpy(&got, out + i * vb, vb);
        if (got != w) { printf("%s: layout %d, %zu keys, %d bytes: pixel %zu (key %08x) stored %llx, want %llx\n", what, layout, keys.size(), vb, i, pk[i],
                               (unsigned long long)got, (unsigned long long)w); return false; }
    }
    for (int k = 1; k <= 16; ++k)
        if (out[-k] != 0xEE || out[count * vb + k - 1] != 0xEE) { printf("%s: a byte beside the output was written\n", what); return false; }
    if (res.aux[0] != missed) { printf("%s: %llu misses counted, %llu expected\n", what, (unsigned long long)res.aux[0], (unsigned long long)missed); return false; }
    return true;
}

static std::vector<uint64_t> values_for(const std::vector<uint32_t> &keys)
{
    std::vector<uint64_t> v;
    for (size_t j = 0; j < keys.size(); ++j) v.push_back((keys[j] + j + 1) * 0x9E3779B97F4A7C15ull ^ 0xA5A5A5A5A5A5A5A5ull);
    return v;
}

static std::vector<uint32_t> sorted(std::vector<uint32_t> k) { std::sort(k.begin(), k.end()); return k; }

template <typename T>
static bool map_cases(bool large, bool brief)
{
    std::mt19937 rng(140 + sizeof(T));
    int turn = 0;
    for (int layout = 0; layout < 3; ++layout) {
        const uint32_t mask = layout_mask(layout);
        const std::vector<uint32_t> few = distinct(layout == 2 ? 40 : 100, mask, rng);
        for (size_t n : {0, 1, 3, 4, 5, 259, 2051})
            for (int vb : {1, 2, 4, 8}) {
                std::vector<uint32_t> keys(few.begin(), few.begin() + few.size() / 2);
                keys = sorted(keys);
                if (!map_case<T>("sizes", pixels_of<T>(draw(few, n, rng), layout, rng), layout, 0, keys, values_for(keys), vb, n > 1024 ? 3 : 1, (n + vb) % 4)) return false;
            }
        // map sizes around the LDS threshold, every value size; a quarter of the pixels miss
        for (uint32_t mc : {0u, 1u, MAP_LDS_KEYS - 1, MAP_LDS_KEYS, MAP_LDS_KEYS + 1}) {
            if (mc > (uint64_t)mask + 1) continue;
            for (int vb : {1, 2, 4, 8}) {
                std::vector<uint32_t> keys = distinct(mc, mask, rng), ks = keys;
                for (size_t i = 0; i < mc / 3 + 17; ++i) ks.push_back((uint32_t)rng() & mask);
                if (!map_case<T>("map sizes", pixels_of<T>(draw(ks, 3001, rng), layout, rng), layout, 0, sorted(keys), values_for(sorted(keys)), vb, 2, 1)) return false;
            }
        }
        // the keys 0 and ~0, in the map and not, on both sides of the threshold
        for (int present = 0; present < 2; ++present)
            for (uint32_t extra : {10u, MAP_LDS_KEYS + 10}) {
                if (extra + 2 > mask) continue;
                std::vector<uint32_t> keys = distinct(extra, mask, rng, 1, mask - 1), ks = keys;
                ks.push_back(0u); ks.push_back(mask);
                if (present) { keys.push_back(0u); keys.push_back(mask); }
                if (!map_case<T>("0 and ~0", pixels_of<T>(draw(ks, 1500, rng), layout, rng), layout, 0, sorted(keys), values_for(sorted(keys)), 4, 1, 0)) return false;
            }
        if (layout == 2) continue;
        for (uint32_t mc : {40u, MAP_LDS_KEYS + 40}) {
            const int vb = 1 << (turn++ & 3);
            std::vector<uint32_t> keys = sorted(distinct(mc, mask, rng, 0, mask / 2)), absent = distinct(50, mask, rng, mask / 2 + 1, mask / 2);
            // every pixel misses
            if (!map_case<T>("all miss", pixels_of<T>(draw(absent, 2051, rng), layout, rng), layout, 0, keys, values_for(keys), vb, 3, 3)) return false;
            // runs of equal pixels across a lane's quad and a workgroup's tile
            std::vector<uint32_t> ks = draw(keys, 4100, rng);
            for (auto r : {std::pair<size_t, size_t>(3, 5), {1022, 7}, {2046, 1030}}) for (size_t i = 0; i < r.second; ++i) ks[r.first + i] = ks[r.first];
            if (!map_case<T>("runs", pixels_of<T>(ks, layout, rng), layout, 0, keys, values_for(keys), vb, 2, 0)) return false;
            // a key twice: the lowest position wins
            std::vector<uint32_t> twice = keys;
            twice[mc / 2 + 1] = twice[mc / 2];
            ks = draw(twice, 1500, rng);
            for (size_t i = 0; i < 64; ++i) ks[i] = twice[mc / 2];
            if (!map_case<T>("duplicate", pixels_of<T>(ks, layout, rng), layout, 0, twice, values_for(twice), vb, 2, 1)) return false;
        }
        std::vector<T> px(3001 * (layout == 0 ? 4 : 2));
        for (auto &c : px) c = (T)rng();
        for (int premultiply : {SPNG_PREMULTIPLY, SPNG_PREMULTIPLY_AS_U8}) {
            if (premultiply == SPNG_PREMULTIPLY_AS_U8 && sizeof(T) == 1) continue;
            std::vector<uint32_t> all = ref_keys(px, layout, premultiply), keys;
            std::map<uint32_t, int> seen;
            for (size_t i = 0; i < all.size(); i += 2) if (!seen[all[i]]++) keys.push_back(all[i]);
            if (!map_case<T>("premultiply", px, layout, premultiply, sorted(keys), values_for(sorted(keys)), 2, 2, 3)) return false;
        }
    }
    if (!large) return true;
    for (uint32_t mc : {65536u, 65537u, 131073u}) {
        if (brief && mc != 65537u) continue;
        const int vb = 1 << (turn++ & 3);
        std::vector<uint32_t> keys = distinct(mc, 0xffffffffu, rng), ks = keys;
        for (size_t i = 0; i < mc / 3; ++i) ks.push_back((uint32_t)rng());
        if (!map_case<T>("large maps", pixels_of<T>(draw(ks, 5000, rng), 0, rng), 0, 0, sorted(keys), values_for(sorted(keys)), vb, 3, 1)) return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    const bool brief = argc > 2 && std::string(argv[2]) == "brief";      // the sanitizer build's share of the large cases
    // T = UInt16 differs from UInt8 in quad_keys alone: the sizes that are about keys run once
    if (mode == "census") {
        if (!census_cases<uint8_t>(true, brief) || !census_cases<uint16_t>(false, brief)) return 1;
        printf("ok\n");
        return 0;
    }
    if (mode == "map") {
        if (!map_cases<uint8_t>(true, brief) || !map_cases<uint16_t>(false, brief)) return 1;
        printf("ok\n");
        return 0;
    }
    fprintf(stderr, "usage: emu_colour_tables census | map [brief]\n");
    return 2;
}
