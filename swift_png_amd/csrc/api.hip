// api.hip -- the context of libspng_mi355.so and what is not a stage of its own: the part of the C ABI declared in
// include/spng_mi355.h that creates, configures, profiles and trims a context, and the sizes and status strings.  The stages
// have their entries in host_decode.hip, host_encode.hip, host_colour.hip and host_files.hip; the launch arithmetic is geometry.hpp.
//
// Everything here is plumbing: argument checks, job tables (the Adam7 / row geometry of
// PNG.Decoder.push, Sources/PNG/Decoding/PNG.Decoder.swift:59-140, and of PNG.Encoder.pull,
// Sources/PNG/Encoding/PNG.Encoder.swift:33-129), one pinned->device upload per call, kernel
// launches on the context's stream and optional HIP-event timing around each launch.  There is
// no CPU implementation of any hot-path function in this library.
#include "host.hpp"

namespace spng {

thread_local char g_err[512] = "";

// PNG.adam7 (PNG.Decoder.swift:6-15) and the sub-image geometry of :63-82
int passes(uint32_t w, uint32_t h, int volume, int interlaced, Pass out[7])
{
    static const uint32_t A7[7][4] = {{0, 0, 3, 3}, {4, 0, 3, 3}, {0, 4, 2, 3}, {2, 0, 2, 2},
                                      {0, 2, 1, 2}, {1, 0, 1, 1}, {0, 1, 0, 1}};
    int n = 0;
    if (!interlaced) {
        if (w && h) out[n++] = Pass{0, 0, 1, 1, w, h, ((uint64_t)w * volume + 7) >> 3};
        return n;
    }
    for (int z = 0; z < 7; ++z) {
        const uint32_t bx = A7[z][0], by = A7[z][1], ex = A7[z][2], ey = A7[z][3];
        const uint32_t sx = 1u << ex, sy = 1u << ey;
        if (w + sx - bx - 1 < sx || h + sy - by - 1 < sy) continue;   // empty pass (:76-80)
        const uint32_t sw = (w + sx - bx - 1) >> ex, sh = (h + sy - by - 1) >> ey;
        if (!sw || !sh) continue;
        out[n++] = Pass{bx, by, sx, sy, sw, sh, ((uint64_t)sw * volume + 7) >> 3};
    }
    return n;
}

}  // namespace spng

extern "C" {

int32_t spng_version(void) { return SPNG_VERSION; }

const char *spng_status_string(int32_t s)
{
    switch (s) {
    case SPNG_DONE: return "done";
    case SPNG_NEED_MORE_INPUT: return "need more input";
    case SPNG_E_COMPRESSION_METHOD: return "invalid rfc-1950 compression method code";
    case SPNG_E_WINDOW_SIZE: return "invalid rfc-1950 window size";
    case SPNG_E_CHECK_BITS: return "invalid rfc-1950 header check bits";
    case SPNG_E_DICTIONARY: return "unexpected rfc-1950 stream dictionary";
    case SPNG_E_STREAM_CHECKSUM: return "invalid rfc-1950 checksum";
    case SPNG_E_BLOCK_TYPE: return "invalid rfc-1951 block type code";
    case SPNG_E_BLOCK_COUNT_PARITY: return "invalid rfc-1951 block element count parity";
    case SPNG_E_RUNLITERAL_COUNT: return "invalid rfc-1951 run-literal symbol count";
    case SPNG_E_CODELENGTH_TABLE: return "malformed rfc-1951 codelength huffman table";
    case SPNG_E_CODELENGTH_SEQUENCE: return "invalid rfc-1951 codelength sequence";
    case SPNG_E_HUFFMAN_TABLE: return "malformed rfc-1951 huffman table";
    case SPNG_E_STRING_REFERENCE: return "invalid rfc-1951 string reference";
    case SPNG_E_EXTRANEOUS_IMAGE_DATA: return "image data buffer not empty after decoding final scanline";
    case SPNG_E_EXTRANEOUS_COMPRESSED_DATA: return "extraneous compressed image data after end of compressed stream";
    case SPNG_E_INCOMPLETE_DATASTREAM: return "reached end-of-image chunk while compressed image data stream is incomplete";
    case SPNG_E_TRUNCATED_SIGNATURE: return "signature truncated";
    case SPNG_E_SIGNATURE: return "invalid png signature bytes";
    case SPNG_E_TRUNCATED_CHUNK_HEADER: return "chunk header truncated";
    case SPNG_E_TRUNCATED_CHUNK_BODY: return "chunk body truncated";
    case SPNG_E_CHUNK_TYPE: return "invalid chunk type code";
    case SPNG_E_CHUNK_CHECKSUM: return "invalid chunk checksum";
    case SPNG_E_OUTPUT_CAPACITY: return "destination buffer too small";
    case SPNG_E_ARGUMENT: return "invalid argument";
    case SPNG_E_DEVICE: return "device error";
    case SPNG_E_REFERENCE_UNDEFINED: return "stream uses a distance code the reference leaves undefined";
    case SPNG_E_TEXT_KEYWORD: return "invalid english keyword in text chunk";
    case SPNG_E_TEXT_CHUNK_LENGTH: return "text chunk shorter than its head";
    case SPNG_E_TEXT_LANGUAGE: return "invalid language tag in text chunk";
    case SPNG_E_TEXT_LOCALIZED_KEYWORD: return "localized keyword of text chunk has no terminator";
    case SPNG_E_TEXT_COMPRESSION_METHOD: return "invalid compression method code in text chunk";
    case SPNG_E_TEXT_COMPRESSION: return "invalid compression code in text chunk";
    case SPNG_E_TEXT_INCOMPLETE: return "compressed datastream of text chunk is incomplete";
    case SPNG_E_PROFILE_NAME: return "invalid color profile name";
    case SPNG_E_PROFILE_CHUNK_LENGTH: return "color profile chunk shorter than its head";
    case SPNG_E_PROFILE_COMPRESSION_METHOD: return "invalid compression method code in color profile chunk";
    case SPNG_E_PROFILE_INCOMPLETE: return "compressed datastream of color profile chunk is incomplete";
    case SPNG_E_TEXT_ENCODING: return "text is not well-formed utf-8";
    // PNG.ParsingError.message without its scope (PNG.ParsingError.swift:397-473): the status names the chunk
    case SPNG_E_PARSE_HEADER_CHUNK_LENGTH: case SPNG_E_PARSE_PALETTE_CHUNK_LENGTH: case SPNG_E_PARSE_TRANSPARENCY_CHUNK_LENGTH:
    case SPNG_E_PARSE_BACKGROUND_CHUNK_LENGTH: case SPNG_E_PARSE_HISTOGRAM_CHUNK_LENGTH: case SPNG_E_PARSE_GAMMA_CHUNK_LENGTH:
    case SPNG_E_PARSE_CHROMATICITY_CHUNK_LENGTH: case SPNG_E_PARSE_RENDERING_CHUNK_LENGTH: case SPNG_E_PARSE_SIGNIFICANT_BITS_CHUNK_LENGTH:
    case SPNG_E_PARSE_PHYSICAL_CHUNK_LENGTH: case SPNG_E_PARSE_SUGGESTED_PALETTE_CHUNK_LENGTH: case SPNG_E_PARSE_SUGGESTED_PALETTE_DATA_LENGTH:
    case SPNG_E_PARSE_TIME_CHUNK_LENGTH: return "invalid chunk length";
    case SPNG_E_PARSE_HEADER_PIXEL_FORMAT_CODE: case SPNG_E_PARSE_HEADER_COMPRESSION_METHOD: case SPNG_E_PARSE_HEADER_FILTER:
    case SPNG_E_PARSE_HEADER_INTERLACING: case SPNG_E_PARSE_RENDERING_CODE: case SPNG_E_PARSE_PHYSICAL_UNIT:
    case SPNG_E_PARSE_SUGGESTED_PALETTE_DEPTH: return "invalid flag code";
    case SPNG_E_PARSE_HEADER_PIXEL_FORMAT: return "invalid pixel format";
    case SPNG_E_PARSE_HEADER_SIZE: return "invalid image size";
    case SPNG_E_PARSE_UNEXPECTED_PALETTE: case SPNG_E_PARSE_UNEXPECTED_TRANSPARENCY: return "unexpected chunk";
    case SPNG_E_PARSE_PALETTE_COUNT: case SPNG_E_PARSE_TRANSPARENCY_COUNT: return "invalid count";
    case SPNG_E_PARSE_TRANSPARENCY_SAMPLE: case SPNG_E_PARSE_BACKGROUND_SAMPLE: return "invalid sample";
    case SPNG_E_PARSE_BACKGROUND_INDEX: return "invalid index";
    case SPNG_E_PARSE_SIGNIFICANT_BITS_PRECISION: return "invalid precision";
    case SPNG_E_PARSE_SUGGESTED_PALETTE_NAME: return "invalid name";
    case SPNG_E_PARSE_SUGGESTED_PALETTE_FREQUENCY: return "invalid frequency";
    case SPNG_E_PARSE_TIME: return "invalid time";
    case SPNG_E_GZIP_SIGIL: return "invalid gzip sigil";
    case SPNG_E_GZIP_METHOD: return "invalid gzip compression method";
    case SPNG_E_GZIP_FLAG_BITS: return "invalid gzip flag bits";
    case SPNG_E_GZIP_HEADER_CHECKSUM: return "gzip header checksum unsupported";
    default: return "unknown status";
    }
}

const char *spng_last_error_string(void) { return g_err; }

uint64_t spng_inflated_size(uint32_t w, uint32_t h, int depth, int channels, int interlaced)
{
    Pass p[7];
    const int n = passes(w, h, depth * channels, interlaced, p);
    uint64_t u = 0;
    for (int i = 0; i < n; ++i) u += (p[i].pitch + 1) * (uint64_t)p[i].h;
    return u;
}

uint64_t spng_storage_size(uint32_t w, uint32_t h, int depth, int channels)
{
    return (uint64_t)w * h * (uint64_t)((depth * channels + 7) >> 3);
}

int32_t spng_create(int device, void *stream, spng_ctx **out)
{
    if (!out) return SPNG_E_ARGUMENT;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || device < 0 || device >= count)
        return fail_hip(e == hipSuccess ? hipErrorInvalidDevice : e, "spng_create: no such HIP device");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(g_err, sizeof g_err, "spng_create: device %d is %s; this library contains gfx950 code only",
                 device, prop.gcnArchName);
        return SPNG_E_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    spng_ctx *c = new spng_ctx;
    c->device = device;
    if (stream) c->stream = (hipStream_t)stream;
    else {
        hipError_t e2 = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e2 != hipSuccess) { delete c; return fail_hip(e2, "hipStreamCreateWithFlags"); }
        c->owns_stream = true;
    }
    // (the deflater's match search asks the device once how its LDS orders the lanes of an atomic exchange: deflate.hip)
    if (hipError_t e3 = launch_deflate3_probe(c->stream); e3 != hipSuccess) { (void)hipGetLastError(); }
    *out = c;
    return SPNG_DONE;
}

void spng_destroy(spng_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &s : c->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto e : c->pool) (void)hipEventDestroy(e);
    if (c->d_ws) (void)hipFree(c->d_ws);
    for (auto &sl : c->slabs) { if (sl.h) (void)hipHostFree(sl.h); if (sl.ev) (void)hipEventDestroy(sl.ev); }
    for (auto b : c->batch_buffers()) if (*b.p) (void)hipFree(*b.p);
    if (c->h_pool_used) (void)hipHostFree(c->h_pool_used);
    if (c->h_lex_stats) (void)hipHostFree(c->h_lex_stats);
    if (c->pool_ev) (void)hipEventDestroy(c->pool_ev);
    if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
    if (c->stream_out) { (void)hipStreamSynchronize(c->stream_out); (void)hipStreamDestroy(c->stream_out); }
    for (hipEvent_t e : c->ev_out) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->ev_fork, c->ev_join}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_dfl) if (e) (void)hipEventDestroy(e);
    if (c->owns_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void *spng_stream(spng_ctx *c) { return c ? (void *)c->stream : nullptr; }

int32_t spng_sync(spng_ctx *c)
{
    if (!c) return SPNG_E_ARGUMENT;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SPNG_DONE;
}

int32_t spng_configure(spng_ctx *c, int key, int64_t value)
{
    if (!c || key < 0 || key >= SPNG_CFG_COUNT || key == 4 || key == 6 /* reserved */ || value < 0) return SPNG_E_ARGUMENT;
    std::lock_guard<std::mutex> g(c->mu);
    c->cfg[key] = value;
    return SPNG_DONE;
}

int32_t spng_profile(spng_ctx *c, int enable)
{
    if (!c) return SPNG_E_ARGUMENT;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (auto &s : c->spans) { c->pool.push_back(s.a); c->pool.push_back(s.b); }
    c->spans.clear();
    c->profiling = enable != 0;
    return SPNG_DONE;
}

int32_t spng_token_stats(spng_ctx *c, uint64_t *page_bytes, uint64_t *blocks, int32_t *ran_dry)
{
    if (!c) return SPNG_E_ARGUMENT;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t *h = c->h_pool_used;                          // {pages, ran dry, blocks} of the last batch read back
    if (page_bytes) *page_bytes = h ? (uint64_t)h[0] << 16 : 0;
    if (ran_dry) *ran_dry = h ? (int32_t)h[1] : 0;
    if (blocks) *blocks = h ? h[2] : 0;
    return SPNG_DONE;
}

int32_t spng_cut_stats(spng_ctx *c, uint64_t *tried, uint64_t *joined, uint64_t *streams_redone)
{
    if (!c) return SPNG_E_ARGUMENT;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t *h = c->h_pool_used && c->cut_stats_valid ? c->h_pool_used + 8 : nullptr;
    if (tried) *tried = h ? h[0] : 0;
    if (joined) *joined = h ? h[1] : 0;
    if (streams_redone) *streams_redone = h ? h[2] : 0;
    return SPNG_DONE;
}

int32_t spng_profile_get(spng_ctx *c, int kernel, double *total_ms, uint64_t *launches)
{
    if (!c || kernel < 0 || kernel >= SPNG_K_COUNT) return SPNG_E_ARGUMENT;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    double t = 0; uint64_t n = 0;
    for (auto &s : c->spans) if (s.kernel == kernel) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
        t += ms; ++n;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = n;
    return SPNG_DONE;
}

}  // extern "C"

extern "C" {

// ---- measurement and housekeeping --------------------------------------------------------------------------------
int32_t spng_copy_ceiling(spng_ctx *c, void *d_dst, const void *d_src, uint64_t bytes, int32_t pattern, int32_t repeats, double *ms_per_copy)
{
    if (!c || !d_dst || !d_src || bytes < 65536 || pattern < 0 || pattern > 1 || repeats < 1 || !ms_per_copy) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    hipEvent_t e0 = c->event(), e1 = c->event();
    HIP_TRY(launch_copy_probe(d_src, d_dst, bytes, pattern, c->stream));      // (first touch)
    HIP_TRY(hipEventRecord(e0, c->stream));
    for (int32_t i = 0; i < repeats; ++i) HIP_TRY(launch_copy_probe(d_src, d_dst, bytes, pattern, c->stream));
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    c->pool.push_back(e0); c->pool.push_back(e1);
    *ms_per_copy = (double)ms / repeats;
    return SPNG_DONE;
}

int32_t spng_lds_exchange_ordered(spng_ctx *c, int32_t *ordered)
{
    if (!c || !ordered) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t v = 0;
    HIP_TRY(deflate3_probe_result(&v));
    *ordered = (int32_t)v;
    return SPNG_DONE;
}

int32_t spng_trim(spng_ctx *c)
{
    if (!c) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
    if (c->stream_out) HIP_TRY(hipStreamSynchronize(c->stream_out));
    for (auto b : c->batch_buffers()) {
        if (*b.p) HIP_TRY(hipFree(*b.p));
        *b.p = nullptr; *b.cap = 0;
    }
    c->pool_ratio = 0; c->block_bytes = 0; c->sym_failed = 0;  // (what the token pool had learned went with it)
    return SPNG_DONE;
}

int32_t spng_shard(uint32_t count, uint32_t parts, uint32_t index, uint32_t *first, uint32_t *n)
{
    if (!parts || index >= parts || !first || !n) return SPNG_E_ARGUMENT;
    const uint32_t per = (count + parts - 1) / parts;
    const uint64_t lo = (uint64_t)per * index;
    *first = lo < count ? (uint32_t)lo : count;
    *n = lo >= count ? 0u : (count - lo < per ? count - (uint32_t)lo : per);
    return SPNG_DONE;
}

}  // extern "C"
