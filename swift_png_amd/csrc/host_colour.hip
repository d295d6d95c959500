// host_colour.hip -- host side of the colour targets: the entries of the C ABI for unpack, pack, alpha, hsva, luminance, census and
// pack_indexed, the checks their descs share and the skeleton of the entries whose results the host fills in.
#include "host.hpp"
#include "geometry.hpp"

// ---- colour targets ------------------------------------------------------------------------------
// What a batch entry and its host-pointer form both need to know about a desc.

static uint32_t pixel_bytes(int layout, int bits)              // one RGBA<T> / VA<T> / T pixel, T of `bits` bits
{
    return (layout == SPNG_TARGET_VA ? 2u : layout == SPNG_TARGET_SCALAR ? 1u : 4u) * (bits / 8);
}
static uint32_t hsva_in_bytes(int op) { return op == SPNG_HSVA_FROM_RGBA8 ? 4u : 8u; }
static uint32_t hsva_out_bytes(int op) { return op == SPNG_HSVA_FROM_RGBA8 ? 8u : op == SPNG_HSVA_TO_RGBA8 ? 4u : 2u; }
static uint32_t luminance_out_bytes(int op) { return op == SPNG_LUMINANCE_V8 ? 1u : 2u; }     // (in: RGBA<UInt8>, 4)

// A desc's `premultiply` (spng_alpha_desc.op too): 0 ... highest, the (as: UInt8.self) forms for T = UInt16 only, none for scalars.
static bool valid_premultiply(int value, int bits, int layout, int highest)
{
    return value <= highest && !((value == SPNG_PREMULTIPLY_AS_U8 || value == SPNG_STRAIGHTEN_AS_U8) && bits != 16) &&
           !(layout == SPNG_TARGET_SCALAR && value);
}

template <size_t N> static bool all_zero(const uint8_t (&reserved)[N]) { return std::all_of(reserved, reserved + N, [](uint8_t r) { return !r; }); }

// [a, a + an) and [b, b + bn) share a byte.  (Equal ranges do: an entry that works in place allows a == b itself.)
static bool overlap(uintptr_t a, uint64_t an, uintptr_t b, uint64_t bn) { return a < b + bn && b < a + an; }

// The call of an entry whose results the host fills in (alpha, hsva, luminance, pack_indexed): one Job and one result per desc, written into
// the arena and uploaded; the results go to d_results by a copy of their own when the caller gave one.
//   fill(desc, job, result, extent) -> bool: checks one desc and fills its zeroed job, its result (status SPNG_DONE so far) and
//     the extent its launch is sized by; false refuses the call (SPNG_E_ARGUMENT) with nothing enqueued.
//   launch(d_jobs, count, most) -> hipError_t: the entry's kernels; most: the largest extent (1 at least).
template <class Job, class Desc, class Fill, class Launch>
static int32_t result_batch(spng_ctx *c, const Desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results,
                            Fill fill, Launch launch)
{
    if (!c || (!descs && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    if (int32_t st = c->reserve(count * (sizeof(Job) + sizeof(spng_result)) + 1024)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(Job)), rslot = a.take(count * sizeof(spng_result));
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(rslot);
    uint64_t most = 1;
    for (uint32_t i = 0; i < count; ++i) {
        Job j;
        memset(&j, 0, sizeof j);
        j.result = dr + i;
        spng_result r{};
        r.status = SPNG_DONE;
        uint64_t extent = 0;
        if (!fill(descs[i], j, r, extent)) return SPNG_E_ARGUMENT;
        a.host<Job>(jslot)[i] = j;
        a.host<spng_result>(rslot)[i] = r;
        most = extent > most ? extent : most;
    }
    if (d_results)
        HIP_TRY(hipMemcpyAsync(d_results, a.host<spng_result>(rslot), count * sizeof(spng_result), hipMemcpyHostToDevice, c->stream));
    if (int32_t st = c->upload(0, a.off)) return st;
    HIP_TRY(launch(a.dev<Job>(jslot), count, most));
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

extern "C" {

int32_t spng_unpack_batch(spng_ctx *c, const spng_unpack_desc *descs, uint32_t count)
{
    if (!c || (!descs && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    const int target = descs[0].target;
    if (target != 8 && target != 16) return SPNG_E_ARGUMENT;
    if (int32_t st = c->reserve(count * sizeof(UnpackJob) + 1024)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(UnpackJob));
    uint64_t maxpix = 1;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_unpack_desc &d = descs[i];
        if (!valid_format(d.depth, d.channels) || !d.d_storage || !d.d_out || d.target != target ||
            (d.indexed && (d.channels != 1 || d.depth > 8 || (!d.d_palette && d.palette_count))) ||
            d.layout > SPNG_TARGET_SCALAR || ((uintptr_t)d.d_out & (target / 8 - 1)) ||
            !valid_premultiply(d.premultiply, target, d.layout, SPNG_STRAIGHTEN_AS_U8))
            return SPNG_E_ARGUMENT;
        UnpackJob j;
        memset(&j, 0, sizeof j);
        j.storage = (const uint8_t *)d.d_storage; j.out = d.d_out; j.palette = (const uint8_t *)d.d_palette;
        j.width = d.width; j.height = d.height; j.palette_count = d.palette_count;
        j.key[0] = d.key[0]; j.key[1] = d.key[1]; j.key[2] = d.key[2];
        j.depth = d.depth; j.channels = d.channels; j.indexed = d.indexed; j.bgr = d.bgr; j.has_key = d.has_key;
        j.layout = d.layout; j.premultiply = d.premultiply;
        a.host<UnpackJob>(jslot)[i] = j;
        const uint64_t px = (uint64_t)d.width * d.height;
        maxpix = px > maxpix ? px : maxpix;
    }
    if (int32_t st = c->upload(0, a.off)) return st;
    Timed t(c, SPNG_K_UNPACK);
    HIP_TRY(launch_unpack(a.dev<UnpackJob>(jslot), count, blocks_for(maxpix, 4096), target, c->stream));   // (four pixels per thread)
    return SPNG_DONE;
}

int32_t spng_unpack_as(spng_ctx *c, const void *storage, uint32_t w, uint32_t h, int depth, int channels,
                       int indexed, int bgr, int target, int layout, int premultiply, const void *palette,
                       uint32_t palette_count, const uint16_t *key, void *out)
{
    if (!c || !storage || !out || !valid_format(depth, channels) || (target != 8 && target != 16)) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t o = (uint64_t)w * h * pixel_bytes(layout, target);
    DevBuf ds, dout, dp;
    HIP_TRY(ds.alloc_from(storage, spng_storage_size(w, h, depth, channels), c->stream)); HIP_TRY(dout.alloc(o));
    HIP_TRY(dp.alloc_from(palette, (size_t)palette_count * 4, c->stream));
    spng_unpack_desc d{};
    d.d_storage = ds.p; d.d_out = dout.p; d.d_palette = palette_count ? dp.p : nullptr;
    d.width = w; d.height = h; d.palette_count = palette_count;
    if (key) { d.key[0] = key[0]; d.key[1] = key[1]; d.key[2] = key[2]; d.has_key = 1; }
    d.depth = (uint8_t)depth; d.channels = (uint8_t)channels; d.indexed = (uint8_t)(indexed != 0); d.bgr = (uint8_t)(bgr != 0);
    d.target = (uint8_t)target; d.layout = (uint8_t)layout; d.premultiply = (uint8_t)premultiply;
    if (int32_t st = spng_unpack_batch(c, &d, 1)) return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(dout.copy_to(out, o));
    return SPNG_DONE;
}

int32_t spng_unpack(spng_ctx *c, const void *storage, uint32_t w, uint32_t h, int depth, int channels,
                    int indexed, int bgr, int target, const void *palette, uint32_t palette_count,
                    const uint16_t *key, void *out)
{
    return spng_unpack_as(c, storage, w, h, depth, channels, indexed, bgr, target, SPNG_TARGET_RGBA, 0, palette, palette_count, key, out);
}

int32_t spng_pack_batch(spng_ctx *c, const spng_pack_desc *descs, uint32_t count)
{
    if (!c || (!descs && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    const int source = descs[0].source;
    if (source != 8 && source != 16) return SPNG_E_ARGUMENT;
    if (int32_t st = c->reserve(count * sizeof(PackJob) + 1024)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(PackJob));
    uint64_t maxpix = 1;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_pack_desc &d = descs[i];
        if (!valid_format(d.depth, d.channels) || !d.d_storage || !d.d_pixels || d.source != source ||
            (d.indexed && (d.channels != 1 || d.depth > 8 || (!d.d_palette && d.palette_count) || d.palette_count > 256)) ||
            d.layout > SPNG_TARGET_SCALAR || ((uintptr_t)d.d_pixels & (source / 8 - 1)) ||
            !valid_premultiply(d.premultiply, source, d.layout, SPNG_PREMULTIPLY_AS_U8))
            return SPNG_E_ARGUMENT;
        PackJob j;
        memset(&j, 0, sizeof j);
        j.pixels = d.d_pixels; j.storage = (uint8_t *)d.d_storage; j.palette = (const uint8_t *)d.d_palette;
        j.width = d.width; j.height = d.height; j.palette_count = d.palette_count;
        j.depth = d.depth; j.channels = d.channels; j.indexed = d.indexed; j.bgr = d.bgr; j.layout = d.layout;
        j.premultiply = d.premultiply;
        a.host<PackJob>(jslot)[i] = j;
        const uint64_t px = (uint64_t)d.width * d.height;
        maxpix = px > maxpix ? px : maxpix;
    }
    if (int32_t st = c->upload(0, a.off)) return st;
    Timed t(c, SPNG_K_PACK);
    HIP_TRY(launch_pack(a.dev<PackJob>(jslot), count, blocks_for(maxpix, 4096), source, c->stream));       // (four pixels per thread)
    return SPNG_DONE;
}

int32_t spng_pack_as(spng_ctx *c, const void *pixels, uint32_t w, uint32_t h, int depth, int channels,
                     int indexed, int bgr, int source, int layout, const void *palette, uint32_t palette_count, void *storage)
{
    if (!c || !storage || !pixels || !valid_format(depth, channels) || (source != 8 && source != 16) || layout < 0 ||
        layout > SPNG_TARGET_SCALAR) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t s = spng_storage_size(w, h, depth, channels);
    DevBuf ds, dpx, dp;
    HIP_TRY(ds.alloc(s)); HIP_TRY(dpx.alloc_from(pixels, (uint64_t)w * h * pixel_bytes(layout, source), c->stream));
    HIP_TRY(dp.alloc_from(palette, (size_t)palette_count * 4, c->stream));
    spng_pack_desc d{};
    d.d_pixels = dpx.p; d.d_storage = ds.p; d.d_palette = palette_count ? dp.p : nullptr;
    d.width = w; d.height = h; d.palette_count = palette_count;
    d.depth = (uint8_t)depth; d.channels = (uint8_t)channels; d.indexed = (uint8_t)(indexed != 0); d.bgr = (uint8_t)(bgr != 0);
    d.source = (uint8_t)source; d.layout = (uint8_t)layout;
    if (int32_t st = spng_pack_batch(c, &d, 1)) return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(ds.copy_to(storage, s));
    return SPNG_DONE;
}

int32_t spng_alpha_batch(spng_ctx *c, const spng_alpha_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    return result_batch<AlphaJob>(c, descs, count, d_results, h_results,
        [=](const spng_alpha_desc &d, AlphaJob &j, spng_result &r, uint64_t &extent) {
            const int bits = descs[0].bits;
            const uint64_t bytes = d.count * pixel_bytes(d.layout, bits);
            const uintptr_t in = (uintptr_t)d.d_in, out = (uintptr_t)d.d_out;
            if ((bits != 8 && bits != 16) || d.bits != bits || d.layout > SPNG_TARGET_VA || d.op < SPNG_PREMULTIPLY ||
                !valid_premultiply(d.op, bits, d.layout, SPNG_STRAIGHTEN_AS_U8) || d.count > (~0ull >> 4) ||
                ((in | out) & (bits / 8 - 1)) || (d.count && (!in || !out)) || (in != out && overlap(in, bytes, out, bytes)) ||
                !all_zero(d.reserved)) return false;
            j.in = d.d_in; j.out = d.d_out; j.count = d.count; j.layout = d.layout; j.op = d.op;
            r.written = r.consumed = extent = bytes;            // (aux[0]: the kernel adds the trapped components)
            return true;
        },
        [=](const AlphaJob *d_jobs, uint32_t n, uint64_t most) {
            Timed t(c, SPNG_K_ALPHA);                           // (16 bytes per thread)
            return launch_alpha(d_jobs, n, blocks_for(most, 16384), descs[0].bits, c->stream);
        });
}

int32_t spng_alpha(spng_ctx *c, const void *pixels, uint64_t n, int bits, int layout, int op, void *out, spng_result *result)
{
    if (!c || (n && (!pixels || !out)) || !result || (bits != 8 && bits != 16) || layout < 0 || layout > SPNG_TARGET_VA ||
        op < 0 || op > 255 || n > (~0ull >> 4)) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t bytes = n * pixel_bytes(layout, bits);
    DevBuf dpx;
    HIP_TRY(dpx.alloc_from(pixels, bytes, c->stream));
    spng_alpha_desc d{};
    d.d_in = dpx.p; d.d_out = dpx.p; d.count = n; d.bits = (uint8_t)bits; d.layout = (uint8_t)layout; d.op = (uint8_t)op;
    if (int32_t st = spng_alpha_batch(c, &d, 1, nullptr, result)) return st;
    HIP_TRY(dpx.copy_to(out, bytes));
    return SPNG_DONE;
}

int32_t spng_hsva_batch(spng_ctx *c, const spng_hsva_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    return result_batch<HsvaJob>(c, descs, count, d_results, h_results,
        [](const spng_hsva_desc &d, HsvaJob &j, spng_result &r, uint64_t &extent) {
            if (d.op < SPNG_HSVA_FROM_RGBA8 || d.op > SPNG_HSVA_TO_VA8 || d.count > (~0ull >> 4)) return false;
            const uint64_t ibytes = d.count * hsva_in_bytes(d.op), obytes = d.count * hsva_out_bytes(d.op);
            const uintptr_t in = (uintptr_t)d.d_in, out = (uintptr_t)d.d_out, hsva = d.op == SPNG_HSVA_FROM_RGBA8 ? out : in;
            // the element sizes differ: nothing runs in place, and no other overlap is allowed either
            if ((hsva & 3) || (d.count && (!in || !out)) || (in && in == out) || overlap(in, ibytes, out, obytes) ||
                !all_zero(d.reserved)) return false;
            j.in = d.d_in; j.out = d.d_out; j.count = d.count; j.op = d.op;
            r.written = obytes; r.consumed = ibytes; extent = d.count;   // (aux[0]: the kernel adds the trapped pixels)
            return true;
        },
        [=](const HsvaJob *d_jobs, uint32_t n, uint64_t most) {
            Timed t(c, SPNG_K_HSVA);                            // (four pixels per thread)
            return launch_hsva(d_jobs, n, blocks_for(most, 4096), c->stream);
        });
}

int32_t spng_hsva(spng_ctx *c, const void *pixels, uint64_t n, int op, void *out, spng_result *result)
{
    if (!c || (n && (!pixels || !out)) || !result || op < SPNG_HSVA_FROM_RGBA8 || op > SPNG_HSVA_TO_VA8 || n > (~0ull >> 4))
        return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t obytes = n * hsva_out_bytes(op);
    DevBuf din, dout;
    HIP_TRY(din.alloc_from(pixels, n * hsva_in_bytes(op), c->stream)); HIP_TRY(dout.alloc(obytes));
    spng_hsva_desc d{};
    d.d_in = din.p; d.d_out = dout.p; d.count = n; d.op = (uint8_t)op;
    if (int32_t st = spng_hsva_batch(c, &d, 1, nullptr, result)) return st;
    HIP_TRY(dout.copy_to(out, obytes));
    return SPNG_DONE;
}

int32_t spng_luminance_batch(spng_ctx *c, const spng_luminance_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    return result_batch<LuminanceJob>(c, descs, count, d_results, h_results,
        [](const spng_luminance_desc &d, LuminanceJob &j, spng_result &r, uint64_t &extent) {
            if (d.op < SPNG_LUMINANCE_V8 || d.op > SPNG_LUMINANCE_VA8 || d.count > (~0ull >> 4)) return false;
            const uint64_t ibytes = d.count * 4, obytes = d.count * luminance_out_bytes(d.op);
            const uintptr_t in = (uintptr_t)d.d_in, out = (uintptr_t)d.d_out;
            // the element sizes differ: nothing runs in place, and no other overlap is allowed either
            if ((d.count && (!in || !out)) || (in && in == out) || overlap(in, ibytes, out, obytes) || !all_zero(d.reserved))
                return false;
            j.in = d.d_in; j.out = d.d_out; j.count = d.count; j.op = d.op;
            r.written = obytes; r.consumed = ibytes; extent = d.count;   // (aux[0] stays 0: nothing traps)
            return true;
        },
        [=](const LuminanceJob *d_jobs, uint32_t n, uint64_t most) {
            Timed t(c, SPNG_K_LUMINANCE);                       // (16 pixels per thread and step at most)
            return launch_luminance(d_jobs, n, blocks_for(most, 16384), c->stream);
        });
}

int32_t spng_luminance(spng_ctx *c, const void *pixels, uint64_t n, int op, void *out, spng_result *result)
{
    if (!c || (n && (!pixels || !out)) || !result || op < SPNG_LUMINANCE_V8 || op > SPNG_LUMINANCE_VA8 || n > (~0ull >> 4))
        return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t obytes = n * luminance_out_bytes(op);
    DevBuf din, dout;
    HIP_TRY(din.alloc_from(pixels, n * 4, c->stream)); HIP_TRY(dout.alloc(obytes));
    spng_luminance_desc d{};
    d.d_in = din.p; d.d_out = dout.p; d.count = n; d.op = (uint8_t)op;
    if (int32_t st = spng_luminance_batch(c, &d, 1, nullptr, result)) return st;
    HIP_TRY(dout.copy_to(out, obytes));
    return SPNG_DONE;
}

int32_t spng_census_batch(spng_ctx *c, const spng_census_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    const int bits = descs[0].bits;
    if (bits != 8 && bits != 16) return SPNG_E_ARGUMENT;
    // the scratch: {ctrl, tags, counts} of every array first -- one block to zero --, the sort buffers behind it
    uint64_t zeroed = 0, sorts = 0, most = 1;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_census_desc &d = descs[i];
        if (d.bits != bits || d.layout > SPNG_TARGET_SCALAR || !valid_premultiply(d.premultiply, bits, d.layout, SPNG_PREMULTIPLY_AS_U8) ||
            d.cap < 1 || d.cap > 65536 || !d.d_keys || ((uintptr_t)d.d_keys & 3) || ((uintptr_t)d.d_counts & 7) ||
            (d.count && !d.d_pixels) || ((uintptr_t)d.d_pixels & (bits / 8 - 1)) || d.count > (~0ull >> 4) || !all_zero(d.reserved))
            return SPNG_E_ARGUMENT;
        zeroed += 256 + 16ull * census_slots(d.cap);
        sorts += 8ull * census_sort_elems(d.cap);
        most = d.count > most ? d.count : most;
    }
    if (int32_t st = c->grow(c->d_census, c->census_cap, zeroed + sorts, 0)) return st;
    if (int32_t st = c->reserve(count * (sizeof(CensusJob) + sizeof(spng_result)) + 1024)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(CensusJob)), rslot = a.take(count * sizeof(spng_result));
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(rslot);
    char *z = (char *)c->d_census, *srt = z + zeroed;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_census_desc &d = descs[i];
        CensusJob j;
        memset(&j, 0, sizeof j);
        j.pixels = d.d_pixels; j.count = d.count; j.keys = (uint32_t *)d.d_keys; j.out_counts = (uint64_t *)d.d_counts;
        j.cap = d.cap; j.slots = census_slots(d.cap);
        for (j.slot_bits = 0; (1u << j.slot_bits) < j.slots; ++j.slot_bits) {}
        j.ctrl = (uint32_t *)z; j.tags = (unsigned long long *)(z + 256); j.counts = j.tags + j.slots;
        z += 256 + 16ull * j.slots;
        j.sort = (unsigned long long *)srt; srt += 8ull * census_sort_elems(d.cap);
        j.result = dr + i; j.layout = d.layout; j.premultiply = d.premultiply;
        a.host<CensusJob>(jslot)[i] = j;
    }
    HIP_TRY(hipMemsetAsync(c->d_census, 0, zeroed, c->stream));
    if (int32_t st = c->upload(0, a.off)) return st;
    { Timed t(c, SPNG_K_CENSUS); HIP_TRY(launch_census(a.dev<CensusJob>(jslot), count, census_blocks_x(count, most), bits, c->stream)); }
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

int32_t spng_census(spng_ctx *c, const void *pixels, uint64_t n, int bits, int layout, int premultiply, uint32_t cap,
                    uint32_t *keys, uint64_t *counts, spng_result *result)
{
    if (!c || (n && !pixels) || !keys || !result || (bits != 8 && bits != 16) || layout < 0 || layout > SPNG_TARGET_SCALAR ||
        premultiply < 0 || premultiply > 255 || cap < 1 || cap > 65536 || n > (~0ull >> 4)) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf dpx, dk, dc;
    HIP_TRY(dpx.alloc_from(pixels, n * pixel_bytes(layout, bits), c->stream));
    HIP_TRY(dk.alloc((size_t)cap * 4)); HIP_TRY(dc.alloc((size_t)cap * 8));
    spng_census_desc d{};
    d.d_pixels = dpx.p; d.count = n; d.d_keys = dk.p; d.d_counts = counts ? dc.p : nullptr; d.cap = cap;
    d.bits = (uint8_t)bits; d.layout = (uint8_t)layout; d.premultiply = (uint8_t)premultiply;
    if (int32_t st = spng_census_batch(c, &d, 1, nullptr, result)) return st;
    if (result->status == SPNG_DONE) {
        HIP_TRY(dk.copy_to(keys, result->written * 4));
        if (counts) HIP_TRY(dc.copy_to(counts, result->written * 8));
    }
    return SPNG_DONE;
}

int32_t spng_pack_indexed_batch(spng_ctx *c, const spng_pack_indexed_desc *descs, uint32_t count, spng_result *d_results,
                                spng_result *h_results)
{
    return result_batch<PackIndexedJob>(c, descs, count, d_results, h_results,
        [=](const spng_pack_indexed_desc &d, PackIndexedJob &j, spng_result &r, uint64_t &extent) {
            const int source = descs[0].source;
            const uint64_t px = (uint64_t)d.width * d.height;
            if ((source != 8 && source != 16) || d.source != source || d.layout > SPNG_TARGET_SCALAR ||
                !valid_premultiply(d.premultiply, source, d.layout, SPNG_PREMULTIPLY_AS_U8) || d.map_count > 65536 ||
                (d.map_count && (!d.d_keys || !d.d_indices)) || ((uintptr_t)d.d_keys & 3) || (px && (!d.d_pixels || !d.d_storage)) ||
                ((uintptr_t)d.d_pixels & (source / 8 - 1)) || !all_zero(d.reserved)) return false;
            j.pixels = d.d_pixels; j.storage = (uint8_t *)d.d_storage; j.keys = (const uint32_t *)d.d_keys; j.indices = (const uint8_t *)d.d_indices;
            j.width = d.width; j.height = d.height; j.map_count = d.map_count;
            j.layout = d.layout; j.premultiply = d.premultiply; j.miss = d.miss;
            r.written = r.consumed = extent = px;               // (aux[0]: the kernel adds the pixels that missed)
            return true;
        },
        [=](const PackIndexedJob *d_jobs, uint32_t n, uint64_t most) {
            Timed t(c, SPNG_K_PACK_INDEXED);                    // (four pixels per thread)
            return launch_pack_indexed(d_jobs, n, blocks_for(most, 4096), descs[0].source, c->stream);
        });
}

int32_t spng_pack_indexed(spng_ctx *c, const void *pixels, uint32_t w, uint32_t h, int source, int layout, int premultiply,
                          const uint32_t *keys, const uint8_t *indices, uint32_t map_count, int miss, void *storage, spng_result *result)
{
    const uint64_t px = (uint64_t)w * h;
    if (!c || !result || (px && (!pixels || !storage)) || (source != 8 && source != 16) || layout < 0 || layout > SPNG_TARGET_SCALAR ||
        premultiply < 0 || premultiply > 255 || miss < 0 || miss > 255 || map_count > 65536 || (map_count && (!keys || !indices)))
        return SPNG_E_ARGUMENT;
    for (uint32_t i = 1; i < map_count; ++i) if (keys[i] <= keys[i - 1]) return SPNG_E_ARGUMENT;   // ascending and distinct
    HIP_TRY(hipSetDevice(c->device));
    DevBuf dpx, ds, dk, di;
    HIP_TRY(dpx.alloc_from(pixels, px * pixel_bytes(layout, source), c->stream)); HIP_TRY(ds.alloc(px));
    HIP_TRY(dk.alloc_from(keys, (size_t)map_count * 4, c->stream)); HIP_TRY(di.alloc_from(indices, map_count, c->stream));
    spng_pack_indexed_desc d{};
    d.d_pixels = dpx.p; d.d_storage = ds.p; d.d_keys = map_count ? dk.p : nullptr; d.d_indices = map_count ? di.p : nullptr;
    d.width = w; d.height = h; d.map_count = map_count;
    d.source = (uint8_t)source; d.layout = (uint8_t)layout; d.premultiply = (uint8_t)premultiply; d.miss = (uint8_t)miss;
    if (int32_t st = spng_pack_indexed_batch(c, &d, 1, nullptr, result)) return st;
    HIP_TRY(ds.copy_to(storage, px));
    return SPNG_DONE;
}

// ---- colour tables without a ceiling (colour_tables.hip) -----------------------------------------

// what a census of `count` pixels at `cap` can find at most: its table and its sort buffer are sized by this, not by cap
static uint32_t census_wide_keys(const spng_census_desc &d) { return (uint32_t)std::min<uint64_t>(d.cap, d.count ? d.count : 1); }

int32_t spng_census_wide_batch(spng_ctx *c, const spng_census_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    const int bits = descs[0].bits;
    if (bits != 8 && bits != 16) return SPNG_E_ARGUMENT;
    // the scratch: the ctrl blocks of all arrays first -- one copy brings them to the host --, their {tags, counts} behind them
    // -- one block to zero --, the sort buffers last
    uint64_t zeroed = 256ull * count, sorts = 0, most = 1;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_census_desc &d = descs[i];
        if (d.bits != bits || d.layout > SPNG_TARGET_SCALAR || !valid_premultiply(d.premultiply, bits, d.layout, SPNG_PREMULTIPLY_AS_U8) ||
            d.cap < 1 || d.cap > SPNG_CENSUS_WIDE_CAP || !d.d_keys || ((uintptr_t)d.d_keys & 3) || ((uintptr_t)d.d_counts & 7) ||
            (d.count && !d.d_pixels) || ((uintptr_t)d.d_pixels & (bits / 8 - 1)) || d.count > (~0ull >> 4) || !all_zero(d.reserved))
            return SPNG_E_ARGUMENT;
        zeroed += 16ull * census_slots(census_wide_keys(d));
        sorts += 8ull * census_sort_elems(census_wide_keys(d));
        most = d.count > most ? d.count : most;
    }
    if (int32_t st = c->grow(c->d_census, c->census_cap, zeroed + sorts, 0)) return st;
    if (int32_t st = c->reserve(count * (sizeof(CensusJob) + sizeof(spng_result)) + 1024)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(CensusJob)), rslot = a.take(count * sizeof(spng_result));
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(rslot);
    char *z = (char *)c->d_census + 256ull * count, *srt = (char *)c->d_census + zeroed;
    uint32_t most_slots = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_census_desc &d = descs[i];
        CensusJob j;
        memset(&j, 0, sizeof j);
        j.pixels = d.d_pixels; j.count = d.count; j.keys = (uint32_t *)d.d_keys; j.out_counts = (uint64_t *)d.d_counts;
        j.cap = d.cap; j.slots = census_slots(census_wide_keys(d));
        for (j.slot_bits = 0; (1u << j.slot_bits) < j.slots; ++j.slot_bits) {}
        j.ctrl = (uint32_t *)((char *)c->d_census + 256ull * i); j.tags = (unsigned long long *)z; j.counts = j.tags + j.slots;
        z += 16ull * j.slots;
        j.sort = (unsigned long long *)srt; srt += 8ull * census_sort_elems(census_wide_keys(d));
        j.result = dr + i; j.layout = d.layout; j.premultiply = d.premultiply;
        a.host<CensusJob>(jslot)[i] = j;
        most_slots = j.slots > most_slots ? j.slots : most_slots;
    }
    HIP_TRY(hipMemsetAsync(c->d_census, 0, zeroed, c->stream));
    if (int32_t st = c->upload(0, a.off)) return st;
    { Timed t(c, SPNG_K_CENSUS); HIP_TRY(launch_census_count(a.dev<CensusJob>(jslot), count, census_blocks_x(count, most), bits, c->stream)); }
    // the one wait: the stages behind are sized by the keys found, not by cap
    std::vector<uint32_t> ctrl(64ull * count);
    HIP_TRY(hipMemcpyAsync(ctrl.data(), c->d_census, 256ull * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t most_keys = 0;
    for (uint32_t i = 0; i < count; ++i)
        if (!ctrl[64ull * i + 1] && ctrl[64ull * i] <= descs[i].cap) most_keys = std::max(most_keys, ctrl[64ull * i]);
    { Timed t(c, SPNG_K_CENSUS); HIP_TRY(launch_census_wide_finish(a.dev<CensusJob>(jslot), count, most_slots, most_keys, c->stream)); }
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

int32_t spng_census_wide(spng_ctx *c, const void *pixels, uint64_t n, int bits, int layout, int premultiply, uint32_t cap,
                         uint32_t *keys, uint64_t *counts, spng_result *result)
{
    if (!c || (n && !pixels) || !keys || !result || (bits != 8 && bits != 16) || layout < 0 || layout > SPNG_TARGET_SCALAR ||
        premultiply < 0 || premultiply > 255 || cap < 1 || cap > SPNG_CENSUS_WIDE_CAP || n > (~0ull >> 4)) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const size_t most = (size_t)std::min<uint64_t>(cap, n ? n : 1);           // (no more keys than pixels)
    DevBuf dpx, dk, dc;
    HIP_TRY(dpx.alloc_from(pixels, n * pixel_bytes(layout, bits), c->stream));
    HIP_TRY(dk.alloc(most * 4)); HIP_TRY(dc.alloc(most * 8));
    spng_census_desc d{};
    d.d_pixels = dpx.p; d.count = n; d.d_keys = dk.p; d.d_counts = counts ? dc.p : nullptr; d.cap = cap;
    d.bits = (uint8_t)bits; d.layout = (uint8_t)layout; d.premultiply = (uint8_t)premultiply;
    if (int32_t st = spng_census_wide_batch(c, &d, 1, nullptr, result)) return st;
    if (result->status == SPNG_DONE) {
        HIP_TRY(dk.copy_to(keys, result->written * 4));
        if (counts) HIP_TRY(dc.copy_to(counts, result->written * 8));
    }
    return SPNG_DONE;
}

static bool valid_value_bytes(int v) { return v == 1 || v == 2 || v == 4 || v == 8; }

int32_t spng_map_batch(spng_ctx *c, const spng_map_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    uint64_t table_slots = 0;                                   // of the maps that do not sit in LDS, one behind the other
    uint32_t most_keys = 0;
    return result_batch<MapJob>(c, descs, count, d_results, h_results,
        [&](const spng_map_desc &d, MapJob &j, spng_result &r, uint64_t &extent) {
            const int source = descs[0].source;
            const uintptr_t align = (uintptr_t)d.value_bytes - 1;
            if ((source != 8 && source != 16) || d.source != source || d.layout > SPNG_TARGET_SCALAR ||
                !valid_premultiply(d.premultiply, source, d.layout, SPNG_PREMULTIPLY_AS_U8) || !valid_value_bytes(d.value_bytes) ||
                d.map_count > SPNG_CENSUS_WIDE_CAP || (d.map_count && (!d.d_keys || !d.d_values)) || ((uintptr_t)d.d_keys & 3) ||
                ((uintptr_t)d.d_values & align) || ((uintptr_t)d.d_out & align) || (d.count && (!d.d_pixels || !d.d_out)) ||
                ((uintptr_t)d.d_pixels & (source / 8 - 1)) || d.count > (~0ull >> 4) || !all_zero(d.reserved)) return false;
            j.pixels = d.d_pixels; j.out = d.d_out; j.keys = (const uint32_t *)d.d_keys; j.values = d.d_values;
            j.count = d.count; j.map_count = d.map_count; j.layout = d.layout; j.premultiply = d.premultiply; j.value_bytes = d.value_bytes;
            memcpy(&j.miss, d.miss, d.value_bytes);             // (little-endian, like the values)
            j.slots = map_slots(d.map_count);
            if (j.slots) {
                for (j.slot_bits = 0; (1u << j.slot_bits) < j.slots; ++j.slot_bits) {}
                j.table_off = table_slots; table_slots += j.slots;
                most_keys = d.map_count > most_keys ? d.map_count : most_keys;
            }
            r.written = d.count * d.value_bytes; r.consumed = extent = d.count;   // (aux[0]: the kernel adds the pixels that missed)
            return true;
        },
        [&](const MapJob *d_jobs, uint32_t n, uint64_t most) {
            if (table_slots) {
                if (c->grow(c->d_census, c->census_cap, 8 * table_slots, 0)) return hipErrorOutOfMemory;     // (the text: spng_last_error_string)
                const hipError_t e = hipMemsetAsync(c->d_census, 0, 8 * table_slots, c->stream);
                if (e != hipSuccess) return e;
            }
            Timed t(c, SPNG_K_PACK_INDEXED);                    // (four pixels per thread, four keys per thread of the build)
            return launch_map(d_jobs, n, (unsigned long long *)c->d_census, table_slots ? blocks_for(most_keys, 1024) : 0,
                              blocks_for(most, 4096), descs[0].source, c->stream);
        });
}

int32_t spng_map(spng_ctx *c, const void *pixels, uint64_t n, int source, int layout, int premultiply, const uint32_t *keys,
                 const void *values, uint32_t map_count, int value_bytes, const void *miss, void *out, spng_result *result)
{
    if (!c || !result || (n && (!pixels || !out)) || (source != 8 && source != 16) || layout < 0 || layout > SPNG_TARGET_SCALAR ||
        premultiply < 0 || premultiply > 255 || !valid_value_bytes(value_bytes) || !miss || map_count > SPNG_CENSUS_WIDE_CAP ||
        (map_count && (!keys || !values)) || n > (~0ull >> 4)) return SPNG_E_ARGUMENT;
    for (uint32_t i = 1; i < map_count; ++i) if (keys[i] <= keys[i - 1]) return SPNG_E_ARGUMENT;   // ascending and distinct
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t obytes = n * (uint64_t)value_bytes;
    DevBuf dpx, dout, dk, dv;
    HIP_TRY(dpx.alloc_from(pixels, n * pixel_bytes(layout, source), c->stream)); HIP_TRY(dout.alloc(obytes));
    HIP_TRY(dk.alloc_from(keys, (size_t)map_count * 4, c->stream)); HIP_TRY(dv.alloc_from(values, (size_t)map_count * value_bytes, c->stream));
    spng_map_desc d{};
    d.d_pixels = dpx.p; d.d_out = dout.p; d.d_keys = map_count ? dk.p : nullptr; d.d_values = map_count ? dv.p : nullptr;
    d.count = n; d.map_count = map_count;
    d.source = (uint8_t)source; d.layout = (uint8_t)layout; d.premultiply = (uint8_t)premultiply; d.value_bytes = (uint8_t)value_bytes;
    memcpy(d.miss, miss, value_bytes);
    if (int32_t st = spng_map_batch(c, &d, 1, nullptr, result)) return st;
    HIP_TRY(dout.copy_to(out, obytes));
    return SPNG_DONE;
}

}  // extern "C"
