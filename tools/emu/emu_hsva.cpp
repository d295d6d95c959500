// emu_hsva.cpp -- TEST INFRASTRUCTURE: runs hsva_kernel of csrc/hsva.hip (the HSVA colour target of Snippets/PNG/CustomColor.swift
// without an integer division) on the CPU (tools/emu/hip/hip_runtime.h; host compiler clang++) against the tutorial's formulas
// restated with plain `/` and `%` (CustomColor.swift:19-78).  From a prepared copy of the source (EMU_HSVA_SRC); never part of the
// product.  The emulator's reciprocal is a correctly rounded 1.0f / x: this proves the scheme, the GPU test proves the device.
//
//   emu_hsva forward     SPNG_HSVA_FROM_RGBA8 over all 2^24 colours (alpha a byte of the index), on the 16-byte path; a stride of
//                        them again pixel by pixel (input 4 bytes, output 8 bytes behind a 16-byte boundary, and an odd input)
//   emu_hsva roundtrip   SPNG_HSVA_TO_RGBA8 of SPNG_HSVA_FROM_RGBA8 over all 2^24 colours is the input, nothing trapped
//   emu_hsva grid        SPNG_HSVA_TO_RGBA8 and SPNG_HSVA_TO_VA8: h in k 65537 + {0, 1, 32768, 65535, 65536}, k = 0 ... 7, and 2^32 - 1;
//                        s in {0, 1, 255, 256, 32767, 32768, 65534, 65535}; every v; and 2^20 random pixels with h below 6 * 65537
#include EMU_HSVA_SRC

#include <random>
#include <string>
#include <vector>

using namespace spng;

struct Hsva { uint32_t h; uint16_t s; uint8_t v, a; };
static_assert(sizeof(Hsva) == 8, "the struct of the tutorial");

static Hsva ref_from(const uint8_t *p)
{
    const uint32_t r = p[0], g = p[1], b = p[2];
    uint32_t lo, mid, hi, sector;
    if (r < g && g < b) { lo = r; mid = g; hi = b; sector = 3; }
    else if (!(r < g) && g < b && r < b) { lo = g; mid = r; hi = b; sector = 4; }
    else if (!(r < g) && g < b) { lo = g; mid = b; hi = r; sector = 5; }
    else if (r < g && r < b) { lo = r; mid = b; hi = g; sector = 2; }
    else if (r < g) { lo = b; mid = r; hi = g; sector = 1; }
    else { lo = b; mid = g; hi = r; sector = 0; }
    const uint32_t d = hi - lo;
    Hsva o = {0, 0, (uint8_t)hi, p[3]};
    if (d > 0) {
        const uint32_t f = ((mid - lo) << 16) / d + 1, rem = (sector & 1) == 0 ? f : 65537 - f;
        o.h = 65537 * sector + rem;
        o.s = (uint16_t)(((d << 16) - 1) / hi);
    }
    return o;
}

static void ref_to_rgba(const Hsva &c, uint8_t *o, uint64_t &trapped)
{
    o[0] = o[1] = o[2] = c.v; o[3] = c.a;
    if (!(c.s > 0 && c.v > 0)) return;
    const uint32_t sector = c.h / 65537, rem = c.h % 65537, f = (sector & 1) == 0 ? rem : 65537 - rem;
    const uint32_t d = (((uint32_t)c.s * c.v) >> 16) + 1;
    const uint32_t x = c.v, y = x - d, z = ((f * d) >> 16) + y;
    switch (sector) {
    case 0: o[0] = x; o[1] = z; o[2] = y; break;
    case 1: o[0] = z; o[1] = x; o[2] = y; break;
    case 2: o[0] = y; o[1] = x; o[2] = z; break;
    case 3: o[0] = y; o[1] = z; o[2] = x; break;
    case 4: o[0] = z; o[1] = y; o[2] = x; break;
    case 5: o[0] = x; o[1] = y; o[2] = z; break;
    default: ++trapped;                                         // fatalError("unreachable"): (v, v, v, a)
    }
}

static size_t in_bytes(int op) { return op == SPNG_HSVA_FROM_RGBA8 ? 4 : 8; }
static size_t out_bytes(int op) { return op == SPNG_HSVA_FROM_RGBA8 ? 8 : op == SPNG_HSVA_TO_RGBA8 ? 4 : 2; }

// the kernel over `count` pixels at `src`, input and output `in_off` / `out_off` bytes behind a 16-byte boundary: -> the output, or
// nothing (and says why) when the poison behind it was written; *trapped: aux[0]
static std::vector<uint8_t> kernel(int op, const void *src, size_t count, size_t in_off, size_t out_off, uint64_t *trapped, unsigned blocks = 3)
{
    const size_t ib = count * in_bytes(op), ob = count * out_bytes(op);
    std::vector<uint8_t> a(ib + 256, 0xEE), b(ob + 256, 0xEE);
    uint8_t *in = a.data() + ((16 - ((uintptr_t)a.data() & 15)) & 15) + in_off;
    uint8_t *out = b.data() + ((16 - ((uintptr_t)b.data() & 15)) & 15) + out_off;
    memcpy(in, src, ib);
    spng_result res;
    memset(&res, 0, sizeof res);
    HsvaJob job;
    memset(&job, 0, sizeof job);
    job.in = in; job.out = out; job.count = count; job.result = &res; job.op = (uint8_t)op;
    emu::launch(blocks, 256, [&] { hsva_kernel(&job); }, 1);
    for (size_t k = 0; k < 64; ++k)
        if (out[ob + k] != 0xEE) { printf("op %d: byte %zu behind the output was written\n", op, k); return {}; }
    for (uint8_t *p = b.data(); p < out; ++p)
        if (*p != 0xEE) { printf("op %d: a byte in front of the output was written\n", op); return {}; }
    *trapped = res.aux[0];
    std::vector<uint8_t> o(out, out + ob);
    o.push_back(0);                                             // (never empty: empty means failure)
    return o;
}

static std::vector<uint8_t> all_colours()
{
    std::vector<uint8_t> px((size_t)4 << 24);
    for (uint32_t c = 0; c < 1u << 24; ++c) {
        px[4 * (size_t)c] = (uint8_t)c; px[4 * (size_t)c + 1] = (uint8_t)(c >> 8); px[4 * (size_t)c + 2] = (uint8_t)(c >> 16);
        px[4 * (size_t)c + 3] = (uint8_t)((c * 7 + 3) >> 5);
    }
    return px;
}

static bool check_from(const char *what, const std::vector<uint8_t> &px, size_t in_off, size_t out_off)
{
    const size_t count = px.size() / 4;
    uint64_t trapped = 0;
    const std::vector<uint8_t> got = kernel(SPNG_HSVA_FROM_RGBA8, px.data(), count, in_off, out_off, &trapped, 64);
    if (got.empty()) return false;
    for (size_t i = 0; i < count; ++i) {
        const Hsva want = ref_from(&px[4 * i]);
        if (memcmp(&got[8 * i], &want, 8)) {
            Hsva g; memcpy(&g, &got[8 * i], 8);
            printf("%s: (%u, %u, %u, %u): got h %u s %u v %u a %u, want h %u s %u v %u a %u\n", what, px[4 * i], px[4 * i + 1], px[4 * i + 2],
                   px[4 * i + 3], g.h, g.s, g.v, g.a, want.h, want.s, want.v, want.a);
            return false;
        }
    }
    if (trapped) { printf("%s: %llu pixels counted as trapped\n", what, (unsigned long long)trapped); return false; }
    return true;
}

static int forward()
{
    const std::vector<uint8_t> px = all_colours();
    if (!check_from("forward", px, 0, 0)) return 1;
    std::vector<uint8_t> some;
    for (size_t c = 0; c < (size_t)1 << 24; c += 61) some.insert(some.end(), &px[4 * c], &px[4 * c] + 4);
    if (!check_from("forward, pixel by pixel", some, 4, 8) || !check_from("forward, odd input", some, 3, 0)) return 1;
    printf("ok: all 2^24 colours\n");
    return 0;
}

static int roundtrip()
{
    const std::vector<uint8_t> px = all_colours();
    uint64_t t0 = 0, t1 = 0;
    std::vector<uint8_t> mid = kernel(SPNG_HSVA_FROM_RGBA8, px.data(), px.size() / 4, 0, 0, &t0, 64);
    if (mid.empty()) return 1;
    const std::vector<uint8_t> back = kernel(SPNG_HSVA_TO_RGBA8, mid.data(), px.size() / 4, 0, 0, &t1, 64);
    if (back.empty()) return 1;
    if (t0 || t1) { printf("roundtrip: %llu + %llu pixels trapped\n", (unsigned long long)t0, (unsigned long long)t1); return 1; }
    for (size_t i = 0; i < px.size(); ++i)
        if (back[i] != px[i]) { printf("roundtrip: colour %zu: byte %zu is %u\n", i / 4, i % 4, back[i]); return 1; }
    printf("ok: all 2^24 colours and back\n");
    return 0;
}

static bool check_to(const char *what, const std::vector<Hsva> &px, size_t in_off, size_t out_off)
{
    uint64_t want_trapped = 0, trapped = 0;
    std::vector<uint8_t> want(px.size() * 4);
    for (size_t i = 0; i < px.size(); ++i) ref_to_rgba(px[i], &want[4 * i], want_trapped);
    std::vector<uint8_t> got = kernel(SPNG_HSVA_TO_RGBA8, px.data(), px.size(), in_off, out_off, &trapped, 16);
    if (got.empty()) return false;
    for (size_t i = 0; i < want.size(); ++i)
        if (got[i] != want[i]) {
            const Hsva &c = px[i / 4];
            printf("%s: to rgba: h %u s %u v %u a %u: component %zu is %u, want %u\n", what, c.h, c.s, c.v, c.a, i % 4, got[i], want[i]);
            return false;
        }
    if (trapped != want_trapped) {
        printf("%s: to rgba: %llu trapped pixels counted, %llu expected\n", what, (unsigned long long)trapped, (unsigned long long)want_trapped);
        return false;
    }
    got = kernel(SPNG_HSVA_TO_VA8, px.data(), px.size(), in_off, out_off, &trapped, 16);
    if (got.empty()) return false;
    for (size_t i = 0; i < px.size(); ++i)
        if (got[2 * i] != px[i].v || got[2 * i + 1] != px[i].a) { printf("%s: to va: pixel %zu\n", what, i); return false; }
    if (trapped) { printf("%s: to va: %llu pixels counted as trapped\n", what, (unsigned long long)trapped); return false; }
    return true;
}

static int grid()
{
    std::vector<Hsva> px;
    std::vector<uint32_t> hs;
    for (uint32_t k = 0; k < 8; ++k)
        for (uint32_t off : {0u, 1u, 32768u, 65535u, 65536u}) hs.push_back(k * 65537u + off);
    hs.push_back(0xffffffffu);
    for (uint32_t h : hs)
        for (uint32_t s : {0u, 1u, 255u, 256u, 32767u, 32768u, 65534u, 65535u})
            for (uint32_t v = 0; v < 256; ++v) px.push_back({h, (uint16_t)s, (uint8_t)v, (uint8_t)(v * 5 + s + h)});
    px.resize(px.size() + 3, Hsva{70000, 40000, 200, 9});      // (a tail behind the 16-byte path)
    if (!check_to("grid", px, 0, 0) || !check_to("grid, pixel by pixel", px, 4, 8) || !check_to("grid, odd output", px, 0, 1)) return 1;
    std::mt19937 rng(11);
    std::vector<Hsva> rnd(1u << 20);
    for (Hsva &c : rnd) c = {(uint32_t)(rng() % (6 * 65537u)), (uint16_t)rng(), (uint8_t)rng(), (uint8_t)rng()};
    for (size_t i = 0; i < rnd.size(); i += 16) rnd[i].h = rng();   // (one in sixteen over all 32 bits)
    if (!check_to("random", rnd, 0, 0)) return 1;
    printf("ok: %zu grid pixels, %zu random ones\n", px.size(), rnd.size());
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "forward") return forward();
    if (mode == "roundtrip") return roundtrip();
    if (mode == "grid") return grid();
    fprintf(stderr, "usage: emu_hsva forward | roundtrip | grid\n");
    return 2;
}
