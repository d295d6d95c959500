// emu_alpha.cpp -- TEST INFRASTRUCTURE: runs alpha_kernel of csrc/alpha.hip (premultiplied <-> straight alpha without an integer
// division) on the CPU (tools/emu/hip/hip_runtime.h; host compiler clang++) against the reference's formulas restated with plain
// `/` (PNG.premultiply / PNG.straighten, Sources/PNG/PNG.swift:55-117).  From a prepared copy of the source (EMU_ALPHA_SRC); never
// part of the product.
//
//   emu_alpha grid8     all 65536 (c, a) pairs: T = UInt8 with both operations, T = UInt16 with the two (as: UInt8.self) forms (high
//                       bytes through all pairs, low bytes random); RGBA and VA; aligned and offset by a pixel; in and out of place
//   emu_alpha sweep16   T = UInt16, all four operations: every alpha with the components 0, 1, a - 1, a, a + 1, 65535 and 64 random
//   emu_alpha divmax    x / (2^k - 1) == (x + 1 + (x >> k)) >> k over the whole range of c * a + (M >> 1), k = 8 and 16
#include EMU_ALPHA_SRC

#include <random>
#include <string>
#include <vector>

using namespace spng;

static uint32_t ref_premultiply(uint32_t c, uint32_t a, uint32_t M) { return (uint32_t)(((uint64_t)c * a + (M >> 1)) / M); }
static uint32_t ref_straighten(uint32_t p, uint32_t a, uint32_t M, uint64_t &trapped)
{
    if (!a) return p;
    const uint64_t q = ((uint64_t)M * p + (a >> 1)) / a;
    if (q > M) { ++trapped; return M; }                         // (the reference traps: T(q) does not fit)
    return (uint32_t)q;
}

// one pixel of nc colour components + alpha, T of `bits` bits
static void ref_pixel(uint32_t *px, int nc, int bits, int op, uint64_t &trapped)
{
    const uint32_t M = bits == 8 ? 0xffu : 0xffffu;
    if (op == SPNG_PREMULTIPLY) for (int z = 0; z < nc; ++z) px[z] = ref_premultiply(px[z], px[nc], M);
    else if (op == SPNG_STRAIGHTEN) for (int z = 0; z < nc; ++z) px[z] = ref_straighten(px[z], px[nc], M, trapped);
    else {
        const uint32_t a8 = px[nc] >> 8;
        for (int z = 0; z < nc; ++z)
            px[z] = 257u * (op == SPNG_PREMULTIPLY_AS_U8 ? ref_premultiply(px[z] >> 8, a8, 255) : ref_straighten(px[z] >> 8, a8, 255, trapped));
        px[nc] = 257u * a8;
    }
}

// the kernel over `pixels` (components in memory order); offset: bytes the arrays start behind a 16-byte boundary.  Returns false
// (and says why) when a pixel, the trap count or the poison behind the output is wrong.
template <typename T>
static bool run(const char *what, const std::vector<T> &pixels, int layout, int op, size_t offset, bool in_place)
{
    const int nc = layout == SPNG_TARGET_VA ? 1 : 3, bits = (int)sizeof(T) * 8;
    const size_t count = pixels.size() / (nc + 1), bytes = pixels.size() * sizeof(T);
    std::vector<uint8_t> a(bytes + 256, 0xEE), b(bytes + 256, 0xEE);
    uint8_t *in = a.data() + ((16 - ((uintptr_t)a.data() & 15)) & 15) + offset;
    uint8_t *out = in_place ? in : b.data() + ((16 - ((uintptr_t)b.data() & 15)) & 15) + offset;
    memcpy(in, pixels.data(), bytes);
    spng_result res;
    memset(&res, 0, sizeof res);
    AlphaJob job;
    memset(&job, 0, sizeof job);
    job.in = in; job.out = out; job.count = count; job.result = &res; job.layout = (uint8_t)layout; job.op = (uint8_t)op;
    emu::launch(3, 256, [&] { alpha_kernel<T>(&job); }, 1);
    uint64_t want_trapped = 0;
    for (size_t i = 0; i < count; ++i) {
        uint32_t px[4];
        for (int z = 0; z <= nc; ++z) px[z] = pixels[i * (nc + 1) + z];
        const uint32_t a0 = px[nc], c0 = px[0];
        ref_pixel(px, nc, bits, op, want_trapped);
        for (int z = 0; z <= nc; ++z) {
            const uint32_t got = ((const T *)out)[i * (nc + 1) + z];
            if (got != px[z]) {
                printf("%s: layout %d op %d offset %zu %s: pixel %zu component %d (c = %u, a = %u): got %u, want %u\n", what, layout, op,
                       offset, in_place ? "in place" : "out of place", i, z, c0, a0, got, px[z]);
                return false;
            }
        }
    }
    for (size_t k = 0; k < 64; ++k)
        if (out[bytes + k] != 0xEE) { printf("%s: layout %d op %d: byte %zu behind the output was written\n", what, layout, op, k); return false; }
    if (res.aux[0] != want_trapped) {
        printf("%s: layout %d op %d: %llu trapped components counted, %llu expected\n", what, layout, op, (unsigned long long)res.aux[0],
               (unsigned long long)want_trapped);
        return false;
    }
    return true;
}

static int grid8()
{
    std::mt19937 rng(8);
    uint64_t runs = 0;
    for (int layout = 0; layout < 2; ++layout) {
        const int nc = layout ? 1 : 3;
        // pixel i: alpha = i / 256 and the first colour = i % 256 (whole waves of one alpha: both shortcuts are taken); the other
        // colours of an RGBA pixel walk the grid from elsewhere
        std::vector<uint8_t> p8;
        std::vector<uint16_t> p16;
        for (uint32_t i = 0; i < 65536; ++i) {
            const uint32_t a = i >> 8;
            for (int z = 0; z < nc; ++z) {
                const uint32_t c = (i + 85 * z) & 255;
                p8.push_back((uint8_t)c);
                p16.push_back((uint16_t)(c << 8 | (rng() & 255)));
            }
            p8.push_back((uint8_t)a);
            p16.push_back((uint16_t)(a << 8 | (rng() & 255)));
        }
        for (size_t offset : {(size_t)0, (size_t)(nc + 1)})
            for (int in_place = 0; in_place < 2; ++in_place) {
                for (int op : {SPNG_PREMULTIPLY, SPNG_STRAIGHTEN}) { if (!run<uint8_t>("grid8", p8, layout, op, offset, in_place)) return 1; ++runs; }
                for (int op : {SPNG_PREMULTIPLY_AS_U8, SPNG_STRAIGHTEN_AS_U8}) { if (!run<uint16_t>("grid8 as u8", p16, layout, op, 2 * offset, in_place)) return 1; ++runs; }
            }
    }
    printf("ok: %llu runs over all 65536 pairs\n", (unsigned long long)runs);
    return 0;
}

static int sweep16()
{
    std::mt19937 rng(16);
    for (int layout = 0; layout < 2; ++layout) {
        const int nc = layout ? 1 : 3;
        std::vector<uint16_t> px;
        for (uint32_t a = 0; a < 65536; ++a) {
            uint32_t comps[72];
            const uint32_t edge[6] = {0, 1, (a - 1) & 0xffff, a, (a + 1) & 0xffff, 65535};
            for (int k = 0; k < 72; ++k) comps[k] = k < 6 ? edge[k] : (k & 1) && a ? rng() % (a + 1) : rng() & 0xffff;   // (half of them below alpha)
            for (int k = 0; k < 72; k += nc) {
                for (int z = 0; z < nc; ++z) px.push_back((uint16_t)comps[k + z]);
                px.push_back((uint16_t)a);
            }
        }
        // a stretch of opaque pixels, a few in between, a stretch of clear ones: the shortcuts from both sides
        for (uint32_t i = 0; i < 1024 + 3 + 1024; ++i) {
            for (int z = 0; z < nc; ++z) px.push_back((uint16_t)rng());
            px.push_back(i < 1024 ? 65535 : i < 1027 ? (uint16_t)(rng() | 1) : 0);
        }
        for (int op = SPNG_PREMULTIPLY; op <= SPNG_STRAIGHTEN_AS_U8; ++op)
            if (!run<uint16_t>("sweep16", px, layout, op, 0, op & 1)) return 1;
    }
    printf("ok: every alpha of 16 bits, 72 components each, four operations, two layouts\n");
    return 0;
}

template <uint32_t K>
static bool divmax_range()
{
    const uint64_t M = (1ull << K) - 1, last = M * M + (M >> 1);
    uint64_t bad = 0;
    for (uint64_t x = 0; x <= last; ++x) bad += div_tmax<K>((uint32_t)x) != (uint32_t)(x / M);
    printf("divmax: k = %u: %llu of the numerators 0 ... %llu differ\n", K, (unsigned long long)bad, (unsigned long long)last);
    return !bad;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "grid8") return grid8();
    if (mode == "sweep16") return sweep16();
    if (mode == "divmax") {
        if (!divmax_range<8>() || !divmax_range<16>()) return 1;
        printf("ok\n");
        return 0;
    }
    fprintf(stderr, "usage: emu_alpha grid8 | sweep16 | divmax\n");
    return 2;
}
