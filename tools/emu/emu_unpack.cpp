// emu_unpack.cpp -- TEST INFRASTRUCTURE: runs unpack_kernel<uint8_t / uint16_t> and pack_kernel<uint8_t / uint16_t> of csrc/unpack.hip on
// the CPU (tools/emu/hip/hip_runtime.h; host compiler clang++) over the case table of tests/unpack_cases.py and compares every output,
// byte for byte, with the oracle's (oracle/pixels.py).  From a prepared copy of the source (EMU_UNPACK_SRC); never part of the product.
// Nothing of the table is restated here: tests/test_emu_unpack.py dumps it (unpack_cases.dump) and the oracle's bytes beside it.
//
//   emu_unpack <table> <want>
//
// Cases that follow one another with the same kernel and T share a launch, one job per grid row, as a call of spng_unpack_batch /
// spng_pack_batch with several descs does: blocks_x comes from the largest (blocks_for(most, 4096), csrc/geometry.hpp), so small
// jobs run under a large job's grid, and an indexed job's LDS table meets the next job's.
// Every input ends where its heap block ends and the palette is a block of its own (a build with -fsanitize=address sees a read one
// quad too far); every output lies between 64 guard bytes of 0xEE that must come back untouched, the bytes of the case's offset
// behind the 16-byte boundary in front of it too.
// The build with -fsanitize=address,undefined takes -fno-sanitize=alignment: unpack_kernel writes a pixel, or the four scalars of a
// quad, with one store, and at an output that is only a multiple of T (which include/spng_mi355.h allows and the device takes) C++
// calls that store misaligned.  Every other check stays on for every case.
#include EMU_UNPACK_SRC
#include "geometry.hpp"

#include <memory>
#include <string>
#include <vector>

using namespace spng;

struct Case {
    std::string name;
    uint32_t kind, width, height, depth, channels, bits, layout, indexed, bgr, premultiply, has_key, key[3], palette_count, in_off, out_off;
    uint64_t in_len, out_len;
    std::vector<uint8_t> palette, input, want;
};

static bool read(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static bool load(const char *table, const char *want, std::vector<Case> &cases)
{
    FILE *f = fopen(table, "rb"), *g = fopen(want, "rb");
    if (!f || !g) { fprintf(stderr, "cannot open the table\n"); return false; }
    char magic[4];
    uint32_t count = 0;
    if (!read(f, magic, 4) || memcmp(magic, "UPK1", 4) || !read(f, &count, 4)) return false;
    cases.resize(count);
    for (Case &c : cases) {
        uint32_t len = 0, v[17];
        if (!read(f, &len, 4) || len > 4096) return false;
        c.name.resize(len);
        if (!read(f, &c.name[0], len) || !read(f, v, sizeof v) || !read(f, &c.in_len, 8) || !read(f, &c.out_len, 8)) return false;
        c.kind = v[0]; c.width = v[1]; c.height = v[2]; c.depth = v[3]; c.channels = v[4]; c.bits = v[5]; c.layout = v[6]; c.indexed = v[7];
        c.bgr = v[8]; c.premultiply = v[9]; c.has_key = v[10]; c.key[0] = v[11]; c.key[1] = v[12]; c.key[2] = v[13];
        c.palette_count = v[14]; c.in_off = v[15]; c.out_off = v[16];
        c.palette.resize((size_t)c.palette_count * 4); c.input.resize(c.in_len);
        if (!read(f, c.palette.data(), c.palette.size()) || !read(f, c.input.data(), c.in_len)) return false;
        uint64_t wl = 0;
        if (!read(g, &wl, 8) || wl != c.out_len) return false;
        c.want.resize(wl);
        if (!read(g, c.want.data(), wl)) return false;
    }
    fclose(f); fclose(g);
    return true;
}

struct Freed { void operator()(void *p) const { free(p); } };
typedef std::unique_ptr<uint8_t, Freed> Block;

// a heap block of exactly off + len bytes on a 16-byte boundary: the bytes at [off, off + len) are the last of it
static Block block(size_t off, const uint8_t *src, size_t len)
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, off + len ? off + len : 1)) abort();
    memset(p, 0xEE, off);
    if (len) memcpy((uint8_t *)p + off, src, len);
    return Block((uint8_t *)p);
}

static const size_t GUARD = 64;

// the cases [a, b): one launch.  -> the cases that failed
static int run(const std::vector<Case> &cases, size_t a, size_t b)
{
    const size_t count = b - a;
    std::vector<Block> inputs, palettes, outputs;
    std::vector<UnpackJob> ujobs(count);
    std::vector<PackJob> pjobs(count);
    uint64_t most = 1;
    const bool pack = cases[a].kind == 1;
    for (size_t i = a; i < b; ++i) {
        const Case &c = cases[i];
        inputs.push_back(block(c.in_off, c.input.data(), c.in_len));
        palettes.push_back(block(0, c.palette.data(), c.palette.size()));
        std::vector<uint8_t> poison(GUARD + c.out_off + c.out_len + GUARD, 0xEE);
        outputs.push_back(block(0, poison.data(), poison.size()));
        uint8_t *in = inputs.back().get() + c.in_off, *out = outputs.back().get() + GUARD + c.out_off;
        const uint8_t *pal = c.palette_count ? palettes.back().get() : nullptr;
        if (((uintptr_t)outputs.back().get() | (uintptr_t)inputs.back().get()) & 15) abort();
        if (pack) {
            PackJob &j = pjobs[i - a];
            memset(&j, 0, sizeof j);
            j.pixels = in; j.storage = out; j.palette = pal; j.width = c.width; j.height = c.height; j.palette_count = c.palette_count;
            j.depth = (uint8_t)c.depth; j.channels = (uint8_t)c.channels; j.indexed = (uint8_t)c.indexed; j.bgr = (uint8_t)c.bgr;
            j.layout = (uint8_t)c.layout; j.premultiply = (uint8_t)c.premultiply;
        } else {
            UnpackJob &j = ujobs[i - a];
            memset(&j, 0, sizeof j);
            j.storage = in; j.out = out; j.palette = pal; j.width = c.width; j.height = c.height; j.palette_count = c.palette_count;
            j.key[0] = (uint16_t)c.key[0]; j.key[1] = (uint16_t)c.key[1]; j.key[2] = (uint16_t)c.key[2];
            j.depth = (uint8_t)c.depth; j.channels = (uint8_t)c.channels; j.indexed = (uint8_t)c.indexed; j.bgr = (uint8_t)c.bgr;
            j.has_key = (uint8_t)c.has_key; j.layout = (uint8_t)c.layout; j.premultiply = (uint8_t)c.premultiply;
        }
        const uint64_t px = (uint64_t)c.width * c.height;
        most = px > most ? px : most;
    }
    const unsigned blocks_x = blocks_for(most, 4096);           // (as spng_unpack_batch / spng_pack_batch size the grid)
    const int bits = (int)cases[a].bits;
    emu::launch(blocks_x, 256, [&] {
        if (pack) { if (bits == 8) pack_kernel<uint8_t>(pjobs.data()); else pack_kernel<uint16_t>(pjobs.data()); }
        else { if (bits == 8) unpack_kernel<uint8_t>(ujobs.data()); else unpack_kernel<uint16_t>(ujobs.data()); }
    }, (unsigned)count);
    int failed = 0;
    for (size_t i = a; i < b; ++i) {
        const Case &c = cases[i];
        const uint8_t *base = outputs[i - a].get(), *out = base + GUARD + c.out_off;
        bool ok = true;
        for (size_t k = 0; k < GUARD + c.out_off && ok; ++k)
            if (base[k] != 0xEE) { printf("%s: byte %zu in front of the output was written\n", c.name.c_str(), GUARD + c.out_off - k); ok = false; }
        for (size_t k = 0; k < GUARD && ok; ++k)
            if (out[c.out_len + k] != 0xEE) { printf("%s: byte %zu behind the output was written\n", c.name.c_str(), k); ok = false; }
        for (size_t k = 0; k < c.out_len && ok; ++k)
            if (out[k] != c.want[k]) {
                printf("%s: byte %zu of %llu: got %02x, want %02x\n", c.name.c_str(), k, (unsigned long long)c.out_len, out[k], c.want[k]);
                ok = false;
            }
        failed += !ok;
    }
    return failed;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: emu_unpack <table> <want>\n"); return 2; }
    std::vector<Case> cases;
    if (!load(argv[1], argv[2], cases)) { fprintf(stderr, "the table does not read\n"); return 2; }
    int failed = 0;
    size_t launches = 0;
    for (size_t a = 0; a < cases.size();) {
        size_t b = a + 1;
        while (b < cases.size() && b - a < 40 && cases[b].kind == cases[a].kind && cases[b].bits == cases[a].bits) ++b;
        failed += run(cases, a, b);
        a = b;
        ++launches;
    }
    printf("%zu cases in %zu launches, %d failed\n", cases.size(), launches, failed);
    return failed ? 1 : 0;
}
