// emu_luminance.cpp -- TEST INFRASTRUCTURE: runs luminance_kernel of csrc/luminance.hip (COMPUTE_LUMINANCE of Snippets/PNG/BasicEncoding.swift
// :63-71 without the binary64 root) on the CPU (tools/emu/hip/hip_runtime.h; host compiler clang++) against the formula written
// plainly with sqrt and round.  From a prepared copy of the source (EMU_LUMINANCE_SRC); never part of the product.  The emulator's
// float root is correctly rounded: this proves the scheme and the table, the GPU test proves the device's v_sqrt_f32.
//
//   emu_luminance table  every entry of LUMINANCE_STEP is the smallest double whose rounded root reaches its index
//   emu_luminance v8     SPNG_LUMINANCE_V8 over all 2^24 colours (alpha a byte of the index) on the 16-byte path; a stride of them again
//                        pixel by pixel (input 4 bytes, output 1 byte behind a 16-byte boundary, and an odd input)
//   emu_luminance va8    the same for SPNG_LUMINANCE_VA8
#include EMU_LUMINANCE_SRC

#include <cmath>
#include <string>
#include <vector>

using namespace spng;

// the tutorial, plainly.  (volatile: the compiler may not fuse a product into a sum here either)
static uint8_t ref_luminance(const uint8_t *p)
{
    const double r = p[0], g = p[1], b = p[2];
    volatile double rr = 0.299 * r, gg = 0.587 * g, bb = 0.114 * b;
    volatile double r2 = rr * r, g2 = gg * g, b2 = bb * b;
    volatile double rg = r2 + g2;
    const double l = sqrt(rg + b2);
    return (uint8_t)fmax(0.0, fmin(round(l), 255.0));
}

// the kernel over `count` pixels at `src`, input and output `in_off` / `out_off` bytes behind a 16-byte boundary: -> the output, or
// nothing (and says why) when a byte around it was written or the result was touched
static std::vector<uint8_t> kernel(int op, const uint8_t *src, size_t count, size_t in_off, size_t out_off, unsigned blocks)
{
    const size_t ib = count * 4, ob = count * (size_t)(op == SPNG_LUMINANCE_V8 ? 1 : 2);
    std::vector<uint8_t> a(ib + 256, 0xEE), b(ob + 256, 0xEE);
    uint8_t *in = a.data() + ((16 - ((uintptr_t)a.data() & 15)) & 15) + in_off;
    uint8_t *out = b.data() + ((16 - ((uintptr_t)b.data() & 15)) & 15) + out_off;
    memcpy(in, src, ib);
    spng_result res;
    memset(&res, 0x5A, sizeof res);
    const spng_result before = res;
    LuminanceJob job;
    memset(&job, 0, sizeof job);
    job.in = in; job.out = out; job.count = count; job.result = &res; job.op = (uint8_t)op;
    emu::launch(blocks, 256, [&] { luminance_kernel(&job); }, 1);
    for (size_t k = 0; k < 64; ++k)
        if (out[ob + k] != 0xEE) { printf("op %d: byte %zu behind the output was written\n", op, k); return {}; }
    for (uint8_t *p = b.data(); p < out; ++p)
        if (*p != 0xEE) { printf("op %d: a byte in front of the output was written\n", op); return {}; }
    if (memcmp(&res, &before, sizeof res)) { printf("op %d: the result was written\n", op); return {}; }
    std::vector<uint8_t> o(out, out + ob);
    o.push_back(0);                                             // (never empty: empty means failure)
    return o;
}

static bool check(const char *what, int op, const std::vector<uint8_t> &px, size_t in_off, size_t out_off, unsigned blocks)
{
    const size_t count = px.size() / 4, per = op == SPNG_LUMINANCE_V8 ? 1 : 2;
    const std::vector<uint8_t> got = kernel(op, px.data(), count, in_off, out_off, blocks);
    if (got.empty()) return false;
    for (size_t i = 0; i < count; ++i) {
        const uint8_t want = ref_luminance(&px[4 * i]);
        if (got[per * i] != want || (per == 2 && got[2 * i + 1] != px[4 * i + 3])) {
            printf("%s: (%u, %u, %u, %u): got %u", what, px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3], got[per * i]);
            if (per == 2) printf(", %u", got[2 * i + 1]);
            printf(", want %u\n", want);
            return false;
        }
    }
    return true;
}

static int colours(int op)
{
    std::vector<uint8_t> px((size_t)4 << 24);
    for (uint32_t c = 0; c < 1u << 24; ++c) {
        px[4 * (size_t)c] = (uint8_t)c; px[4 * (size_t)c + 1] = (uint8_t)(c >> 8); px[4 * (size_t)c + 2] = (uint8_t)(c >> 16);
        px[4 * (size_t)c + 3] = (uint8_t)((c * 7 + 3) >> 5);
    }
    if (!check("every colour", op, px, 0, 0, 64)) return 1;
    std::vector<uint8_t> some;
    for (size_t c = 0; c < (size_t)1 << 24; c += 61) some.insert(some.end(), &px[4 * c], &px[4 * c] + 4);
    some.resize(some.size() / 64 * 64 + 4 * 13);               // (a tail behind the 16-byte path)
    if (!check("a stride, 16-byte path and tail", op, some, 0, 0, 3) || !check("a stride, pixel by pixel", op, some, 4, 1, 3) ||
        !check("a stride, odd input", op, some, 3, 0, 3)) return 1;
    printf("ok: all 2^24 colours\n");
    return 0;
}

static int rounded_root(double x) { return (int)round(sqrt(x)); }

static int table()
{
    if (LUMINANCE_STEP[0] != 0.0 || !std::isinf(LUMINANCE_STEP[256])) { printf("the ends of the table\n"); return 1; }
    for (int k = 1; k < 256; ++k) {
        const double t = LUMINANCE_STEP[k];
        if (rounded_root(t) != k || rounded_root(std::nextafter(t, 0.0)) != k - 1) { printf("entry %d: %a\n", k, t); return 1; }
    }
    // and the function over the neighbourhood of every entry, where the float estimate is at its worst
    for (int k = 1; k < 256; ++k)
        for (int d = -3; d <= 3; ++d) {
            double x = LUMINANCE_STEP[k];
            for (int s = 0; s < (d < 0 ? -d : d); ++s) x = std::nextafter(x, d < 0 ? 0.0 : 1e9);
            const int want = rounded_root(x) > 255 ? 255 : rounded_root(x);
            if ((int)luminance_of_square(x, LUMINANCE_STEP) != want) { printf("x = %a: got %u, want %d\n", x, luminance_of_square(x, LUMINANCE_STEP), want); return 1; }
        }
    printf("ok: 255 steps\n");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "table") return table();
    if (mode == "v8") return colours(SPNG_LUMINANCE_V8);
    if (mode == "va8") return colours(SPNG_LUMINANCE_VA8);
    fprintf(stderr, "usage: emu_luminance table | v8 | va8\n");
    return 2;
}
