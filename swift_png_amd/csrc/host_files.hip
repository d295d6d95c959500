// host_files.hip -- host side of the file stages: the entries of the C ABI that lex PNG files into chunks, write IDAT chunks and whole
// files, and compute CRC-32.
#include "host.hpp"
#include "geometry.hpp"
#include "file_head.hpp"

// The writer over descs[0, count): heads built on the host (file_head.hpp) and uploaded through the call's arena with the job table.
// The caller holds the context's lock.
static int32_t write_files(spng_ctx *c, const spng_png_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    std::vector<uint8_t> heads;
    std::vector<uint64_t> head_at(count, 0), head_len(count, 0), part_at(count + 1, 0);
    uint64_t most_units = 1, finish_chunks = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_png_desc &d = descs[i];
        if (!d.d_stream || !d.d_out || (!d.d_stream_result && d.stream_cap && d.stream_cap < d.stream_len)) return SPNG_E_ARGUMENT;
        while (heads.size() % 16) heads.push_back(0);          // (every head at a multiple of 16 of the arena)
        head_at[i] = heads.size();
        if (int32_t st = file_head(d, heads)) return st;
        head_len[i] = heads.size() - head_at[i];
        const uint64_t cap = d.d_stream_result || d.stream_cap ? d.stream_cap : d.stream_len;
        const uint64_t units = file_units(cap, d.chunk_bytes);
        most_units = units > most_units ? units : most_units;
        // raw sums for the chunks of several pieces: a word per unit the capacity allows
        part_at[i + 1] = part_at[i] + (d.chunk_bytes > FILE_PIECE_BYTES && cap > FILE_PIECE_BYTES ? units : 0);
        if (part_at[i + 1] > part_at[i]) finish_chunks = std::max(finish_chunks, file_chunks(cap, d.chunk_bytes));
    }
    if (int32_t st = c->reserve(count * (sizeof(FileJob) + sizeof(spng_result)) + heads.size() + 4 * part_at[count] + 4096)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(FileJob));
    const size_t hslot = a.take(heads.size());
    const size_t upload = a.off;
    const size_t rslot = a.take(count * sizeof(spng_result));
    const size_t pslot = a.take(4 * part_at[count]);
    if (!heads.empty()) memcpy(a.host<uint8_t>(hslot), heads.data(), heads.size());
    for (uint32_t i = 0; i < count; ++i) {
        const spng_png_desc &d = descs[i];
        FileJob j{};
        j.head = a.dev<uint8_t>(hslot) + head_at[i]; j.head_len = head_len[i];
        j.stream = (const uint8_t *)d.d_stream; j.src_result = d.d_stream_result; j.len = d.d_stream_result ? 0 : d.stream_len;
        j.stream_cap = d.d_stream_result || d.stream_cap ? d.stream_cap : d.stream_len;
        j.out = (uint8_t *)d.d_out; j.out_cap = d.out_cap; j.chunk_bytes = d.chunk_bytes;
        j.partial = part_at[i + 1] > part_at[i] ? a.dev<uint32_t>(pslot) + part_at[i] : nullptr;
        a.host<FileJob>(jslot)[i] = j;
    }
    if (int32_t st = c->upload(0, upload)) return st;
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(rslot);
    {
        Timed t(c, SPNG_K_LEX);
        HIP_TRY(launch_write_file(a.dev<FileJob>(jslot), count, file_blocks_x(count, most_units), finish_chunks, dr, c->stream));
    }
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

// The lexer entries.  d_states: a state per file (files that arrive in pieces: the call's counters go to c->h_lex_stats), or null:
// whole files -- with `dirs`, a chunk directory per file behind the lexer's own kernels
static int32_t lex_batch(spng_ctx *c, const spng_file_desc *files, void *const *d_states, uint32_t count, spng_lexed *d_infos, spng_lexed *h_infos,
                         const spng_chunk_dir *dirs = nullptr)
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
    uint32_t most_entries = 0;                                 // (no chunk is shorter than 12 bytes)
    for (uint32_t i = 0; dirs && i < count; ++i) {
        if ((!dirs[i].d_entries && dirs[i].cap) || ((uintptr_t)dirs[i].d_entries & 7) || dirs[i].reserved) return SPNG_E_ARGUMENT;
        most_entries = std::max(most_entries, (uint32_t)std::min<uint64_t>(dirs[i].cap, files[i].len / 12));
    }
    const size_t walk_bytes = d_states ? lex_rwalk_bytes() : lex_walk_bytes();
    const size_t table_bytes = (size_t)at[count] * (d_states ? lex_piece_bytes() : lex_chunk_bytes());
    if (int32_t st = c->reserve(count * (sizeof(spng_file_desc) + sizeof(spng_lexed) + 16 + walk_bytes + (dirs ? sizeof(spng_chunk_dir) : 0)) + table_bytes + 4096))
        return st;
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
    const size_t dslot = dirs ? a.take(count * sizeof(spng_chunk_dir)) : 0;
    if (dirs) memcpy(a.host<spng_chunk_dir>(dslot), dirs, count * sizeof(spng_chunk_dir));
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
        if (dirs)
            HIP_TRY(launch_lex_dir(a.dev<spng_file_desc>(fslot), a.dev<spng_chunk_dir>(dslot), count, dout, a.dev<uint8_t>(tslot),
                                   a.dev<uint64_t>(atslot), a.dev<uint8_t>(wslot), most_entries, c->stream));
    }
    if (d_states) HIP_TRY(hipMemcpyAsync(c->h_lex_stats, a.dev<uint64_t>(cslot), 24, hipMemcpyDeviceToHost, c->stream));
    return read_back(c, h_infos, dout, count * sizeof(spng_lexed));
}

extern "C" {

int32_t spng_lex_batch(spng_ctx *c, const spng_file_desc *files, uint32_t count, spng_lexed *d_infos, spng_lexed *h_infos)
{
    return lex_batch(c, files, nullptr, count, d_infos, h_infos);
}

int32_t spng_lex_dir_batch(spng_ctx *c, const spng_file_desc *files, const spng_chunk_dir *dirs, uint32_t count, spng_lexed *d_infos,
                           spng_lexed *h_infos)
{
    if (!dirs && count) return SPNG_E_ARGUMENT;
    return lex_batch(c, files, nullptr, count, d_infos, h_infos, dirs);
}

int32_t spng_parse_dir_batch(spng_ctx *c, const spng_file_desc *files, const spng_chunk_dir *dirs, const spng_lexed *d_infos,
                             spng_chunk_value *const *d_values, uint32_t count, spng_parsed *d_parsed, spng_parsed *h_parsed)
{
    if (!c || ((!files || !dirs || !d_infos || !d_values) && count) || (!d_parsed && !h_parsed && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    uint32_t most_entries = 0;                                 // (as the directory's: no chunk is shorter than 12 bytes)
    for (uint32_t i = 0; i < count; ++i) {
        if ((!files[i].d_png && files[i].len) || (dirs[i].cap && (!dirs[i].d_entries || !d_values[i])) || ((uintptr_t)d_values[i] & 7) ||
            dirs[i].reserved)
            return SPNG_E_ARGUMENT;
        most_entries = std::max(most_entries, (uint32_t)std::min<uint64_t>(dirs[i].cap, files[i].len / 12));
    }
    // the tables go up behind whatever the stream still holds -- the directory's kernels, as a rule --: nothing here waits for them
    if (int32_t st = c->reserve(count * (sizeof(spng_file_desc) + sizeof(spng_chunk_dir) + sizeof(void *) + sizeof(spng_parsed)) + 4096)) return st;
    Arena a{c};
    const size_t fslot = a.take(count * sizeof(spng_file_desc));
    memcpy(a.host<spng_file_desc>(fslot), files, count * sizeof(spng_file_desc));
    const size_t dslot = a.take(count * sizeof(spng_chunk_dir));
    memcpy(a.host<spng_chunk_dir>(dslot), dirs, count * sizeof(spng_chunk_dir));
    const size_t vslot = a.take(count * sizeof(void *));
    memcpy(a.host<void *>(vslot), d_values, count * sizeof(void *));
    const size_t upload = a.off;
    const size_t pslot = a.take(count * sizeof(spng_parsed));
    if (int32_t st = c->upload(0, upload)) return st;
    spng_parsed *dp = d_parsed ? d_parsed : a.dev<spng_parsed>(pslot);
    {
        Timed t(c, SPNG_K_LEX);
        HIP_TRY(launch_parse_dir(a.dev<spng_file_desc>(fslot), a.dev<spng_chunk_dir>(dslot), count, d_infos, a.dev<spng_chunk_value *>(vslot),
                                 most_entries, dp, c->stream));
    }
    return read_back(c, h_parsed, dp, count * sizeof(spng_parsed));
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

uint64_t spng_file_bound(const spng_png_desc *desc, uint64_t stream_len) { return desc ? file_bound(*desc, stream_len) : 0; }

int32_t spng_write_file_batch(spng_ctx *c, const spng_png_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    return write_files(c, descs, count, d_results, h_results);
}

int32_t spng_compress_batch(spng_ctx *c, const spng_image_desc *images, const spng_png_desc *files, int32_t level, uint32_t count,
                            spng_result *d_results, spng_result *h_results)
{
    if (!c || ((!images || !files) && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    // the files with the stream fields and the header fields of their images; refused before anything is launched
    std::vector<spng_png_desc> fd(files, files + count);
    std::vector<uint8_t> scratch;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_image_desc &im = images[i];
        spng_png_desc &d = fd[i];
        if ((im.format == SPNG_FORMAT_IOS) != (d.bgr != 0) || im.format > SPNG_FORMAT_IOS || !im.d_idat || !d.d_out) return SPNG_E_ARGUMENT;
        d.width = im.width; d.height = im.height; d.depth = im.depth; d.channels = im.channels; d.interlaced = im.interlaced;
        d.d_stream = im.d_idat; d.stream_len = 0; d.stream_cap = im.idat_len;
        scratch.clear();
        if (int32_t st = file_head(d, scratch)) return st;
    }
    // the encoder's results stay on the device, in a buffer of the context (the job tables of the calls below take the arena in turn)
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (int32_t st = c->grow(c->d_file, c->file_cap, count * sizeof(spng_result), 4096)) return st;
    }
    spng_result *enc = (spng_result *)c->d_file;
    for (uint32_t i = 0; i < count; ++i) fd[i].d_stream_result = enc + i;
    // PNG.Encoder.pull end to end, then the chunks around its stream: one launch chain, no host wait in between
    if (int32_t st = spng_encode_batch(c, images, level, count, enc, nullptr)) return st;
    std::lock_guard<std::mutex> g(c->mu);
    return write_files(c, fd.data(), count, d_results, h_results);
}

int32_t spng_text_batch(spng_ctx *c, const spng_text_desc *descs, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t tiles = 0, most = 0;
    bool writes = false;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_text_desc &d = descs[i];
        const bool transcode = d.op == SPNG_TEXT_LATIN1_TO_UTF8;
        if ((!transcode && d.op != SPNG_TEXT_CHECK_UTF8) || (d.len && !d.d_in) || d.len > (~0ull >> 2)) return SPNG_E_ARGUMENT;
        for (uint8_t r : d.reserved) if (r) return SPNG_E_ARGUMENT;
        if (transcode && d.len) {
            const uintptr_t in = (uintptr_t)d.d_in, out = (uintptr_t)d.d_out;
            if ((!out && d.out_cap) || (in < out + d.out_cap && out < in + d.len)) return SPNG_E_ARGUMENT;   // (no room at all: the bytes needed come back)
        }
        writes = writes || transcode;
        tiles += text_tiles(d.len);
        most = std::max<uint64_t>(most, text_tiles(d.len));
    }
    if (int32_t st = c->reserve(count * (sizeof(TextJob) + sizeof(spng_result)) + 16 * tiles + 4096)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(TextJob));
    const size_t upload = a.off;
    const size_t rslot = a.take(count * sizeof(spng_result));
    const size_t oslot = a.take(8 * tiles), cslot = a.take(4 * tiles), fslot = a.take(4 * tiles);
    uint64_t at = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_text_desc &d = descs[i];
        TextJob j{};
        j.in = (const uint8_t *)d.d_in; j.out = (uint8_t *)d.d_out; j.len = d.len; j.out_cap = d.out_cap; j.op = d.op;
        j.tiles = text_tiles(d.len);
        j.offs = a.dev<uint64_t>(oslot) + at; j.counts = a.dev<uint32_t>(cslot) + at; j.firsts = a.dev<uint32_t>(fslot) + at;
        at += j.tiles;
        a.host<TextJob>(jslot)[i] = j;
    }
    if (int32_t st = c->upload(0, upload)) return st;
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(rslot);
    {
        Timed t(c, SPNG_K_LEX);
        HIP_TRY(launch_text(a.dev<TextJob>(jslot), count, most ? lex_piece_blocks_x(count, (uint32_t)std::min<uint64_t>(most, 1u << 20)) : 0, writes, dr,
                            c->stream));
    }
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
