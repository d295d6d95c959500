// host_files.hip -- host side of the file stages: the entries of the C ABI that lex PNG files into chunks, write IDAT chunks and
// compute CRC-32.
#include "host.hpp"
#include "geometry.hpp"

// Both lexer entries.  d_states: a state per file (files that arrive in pieces: the call's counters go to c->h_lex_stats), or null:
// whole files
static int32_t lex_batch(spng_ctx *c, const spng_file_desc *files, void *const *d_states, uint32_t count, spng_lexed *d_infos, spng_lexed *h_infos)
{
    if (!c || (!files && count) || (!d_infos && !h_infos && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    if (d_states && !c->h_lex_stats) {
        HIP_TRY(hipHostMalloc((void **)&c->h_lex_stats, 32, hipHostMallocDefault));
        memset(c->h_lex_stats, 0, 32);
    }
    std::vector<uint64_t> at(count + 1, 0);                    // the chunk lists / piece lists (geometry.hpp: lex_listed, lex_resume_listed)
    uint32_t max_listed = 1;
    for (uint32_t i = 0; i < count; ++i) {
        if ((!files[i].d_png && files[i].len) || (!files[i].d_idat && files[i].idat_cap)) return SPNG_E_ARGUMENT;
        const uint64_t k = d_states ? lex_resume_listed(files[i].len) : lex_listed(files[i].len);
        at[i + 1] = at[i] + k;
        max_listed = k > max_listed ? (uint32_t)k : max_listed;
    }
    const size_t walk_bytes = d_states ? lex_rwalk_bytes() : lex_walk_bytes();
    const size_t table_bytes = (size_t)at[count] * (d_states ? lex_piece_bytes() : lex_chunk_bytes());
    if (int32_t st = c->reserve(count * (sizeof(spng_file_desc) + sizeof(spng_lexed) + 16 + walk_bytes) + table_bytes + 4096)) return st;
    Arena a{c};
    const size_t fslot = a.take(count * sizeof(spng_file_desc));
    for (uint32_t i = 0; i < count; ++i) a.host<spng_file_desc>(fslot)[i] = files[i];
    const size_t atslot = a.take((count + 1) * 8);
    memcpy(a.host<uint64_t>(atslot), at.data(), (count + 1) * 8);
    size_t sslot = 0, cslot = 0;
    if (d_states) {
        sslot = a.take(count * sizeof(void *));                // (a null state is that file's SPNG_E_ARGUMENT: the walk sees it)
        memcpy(a.host<void *>(sslot), d_states, count * sizeof(void *));
        cslot = a.take(32);                                    // the call's counters, zeroed by the upload
        memset(a.host<uint64_t>(cslot), 0, 32);
    }
    const size_t upload = a.off;
    const size_t oslot = a.take(count * sizeof(spng_lexed));
    const size_t wslot = a.take(count * walk_bytes);
    const size_t tslot = a.take(table_bytes);
    if (int32_t st = c->upload(0, upload)) return st;
    spng_lexed *dout = d_infos ? d_infos : a.dev<spng_lexed>(oslot);
    {
        Timed t(c, SPNG_K_LEX);
        if (d_states)
            HIP_TRY(launch_lex_resume(a.dev<spng_file_desc>(fslot), a.dev<void *>(sslot), count, dout, a.dev<uint8_t>(tslot), a.dev<uint64_t>(atslot),
                                      a.dev<uint8_t>(wslot), max_listed, a.dev<uint64_t>(cslot), c->stream));
        else
            HIP_TRY(launch_lex(a.dev<spng_file_desc>(fslot), count, dout, a.dev<uint8_t>(tslot), a.dev<uint64_t>(atslot), a.dev<uint8_t>(wslot),
                               max_listed, c->stream));
    }
    if (d_states) HIP_TRY(hipMemcpyAsync(c->h_lex_stats, a.dev<uint64_t>(cslot), 24, hipMemcpyDeviceToHost, c->stream));
    return read_back(c, h_infos, dout, count * sizeof(spng_lexed));
}

extern "C" {

int32_t spng_lex_batch(spng_ctx *c, const spng_file_desc *files, uint32_t count, spng_lexed *d_infos, spng_lexed *h_infos)
{
    return lex_batch(c, files, nullptr, count, d_infos, h_infos);
}

uint64_t spng_lex_state_bytes(void) { return lex_state_bytes(); }

int32_t spng_lex_resume_batch(spng_ctx *c, const spng_file_desc *files, void *const *d_states, uint32_t count, spng_lexed *d_infos,
                              spng_lexed *h_infos)
{
    if (!d_states && count) return SPNG_E_ARGUMENT;
    return lex_batch(c, files, d_states, count, d_infos, h_infos);
}

int32_t spng_lex_resume_stats(spng_ctx *c, uint64_t *summed, uint64_t *copied, uint64_t *headers)
{
    if (!c) return SPNG_E_ARGUMENT;
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t *h = c->h_lex_stats;
    if (summed) *summed = h ? h[0] : 0;
    if (copied) *copied = h ? h[1] : 0;
    if (headers) *headers = h ? h[2] : 0;
    return SPNG_DONE;
}

int32_t spng_write_idat_batch(spng_ctx *c, const spng_chunking_desc *descs, uint32_t count,
                              spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    if (int32_t st = c->reserve(count * (sizeof(spng_chunking_desc) + sizeof(spng_result)) + 1024)) return st;
    Arena a{c};
    const size_t dslot = a.take(count * sizeof(spng_chunking_desc));
    uint64_t most = 1;
    for (uint32_t i = 0; i < count; ++i) {
        if ((!descs[i].d_stream && descs[i].len) || !descs[i].d_out || !descs[i].chunk_bytes ||
            descs[i].chunk_bytes > 0x7fffffffull) return SPNG_E_ARGUMENT;
        a.host<spng_chunking_desc>(dslot)[i] = descs[i];
        const uint64_t pieces = (descs[i].len + descs[i].chunk_bytes - 1) / descs[i].chunk_bytes;
        most = pieces > most ? pieces : most;
    }
    const size_t upload = a.off;
    const size_t rslot = a.take(count * sizeof(spng_result));
    if (int32_t st = c->upload(0, upload)) return st;
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(rslot);
    { Timed t(c, SPNG_K_LEX); HIP_TRY(launch_write_idat(a.dev<spng_chunking_desc>(dslot), count, write_idat_blocks_x(most), dr, c->stream)); }
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

int32_t spng_crc32(spng_ctx *c, const void *data, uint64_t n, uint32_t *out)
{
    if (!c || (!data && n) || !out) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t piece = 1u << 20;
    const uint32_t pieces = (uint32_t)((n + piece - 1) / piece);
    std::vector<uint32_t> part(pieces ? pieces : 1);
    if (pieces) {
        DevBuf dd, dp;
        HIP_TRY(dd.alloc(n)); HIP_TRY(dp.alloc((size_t)pieces * 4));
        HIP_TRY(hipMemcpyAsync(dd.p, data, n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_crc_partial((const uint8_t *)dd.p, n, piece, (uint32_t *)dp.p, pieces, c->stream));
        if (int32_t st = read_back(c, part.data(), dp.p, (size_t)pieces * 4)) return st;
    }
    *out = crc32_fold(part.data(), pieces, n, piece);
    return SPNG_DONE;
}

}  // extern "C"
