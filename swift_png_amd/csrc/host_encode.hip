// host_encode.hip -- host side of the encode stages: the entries of the C ABI for filter selection, Adler-32, deflate (levels 0-7 in
// rounds, the full search of levels 8 and up, one-shot and resumed) and encode, with the slab layout and the round pipeline of the deflate search.
#include "host.hpp"
#include "geometry.hpp"

extern "C" {

int32_t spng_adler32(spng_ctx *c, const void *data, uint64_t n, uint32_t *out)
{
    if (!c || (!data && n) || !out) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t chunk = 1u << 16;
    const uint32_t blocks = (uint32_t)((n + chunk - 1) / chunk);
    uint32_t s1 = 1, s2 = 0;
    if (blocks) {
        DevBuf dd, dp;
        HIP_TRY(dd.alloc(n)); HIP_TRY(dp.alloc((size_t)blocks * 16));
        HIP_TRY(hipMemcpyAsync(dd.p, data, n, hipMemcpyHostToDevice, c->stream));
        {
            Timed t(c, SPNG_K_ADLER);
            HIP_TRY(launch_adler_partial((const uint8_t *)dd.p, n, chunk, (uint64_t *)dp.p, blocks, c->stream));
        }
        std::vector<uint64_t> part((size_t)blocks * 2);
        if (int32_t st = read_back(c, part.data(), dp.p, (size_t)blocks * 16)) return st;
        for (uint32_t i = 0; i < blocks; ++i) {
            const uint64_t len = n - (uint64_t)i * chunk < chunk ? n - (uint64_t)i * chunk : chunk;
            s2 = (uint32_t)((s2 + (len % 65521) * s1 + part[2 * i + 1] % 65521) % 65521);
            s1 = (uint32_t)((s1 + part[2 * i] % 65521) % 65521);
        }
    }
    *out = s2 << 16 | s1;
    return SPNG_DONE;
}

int32_t spng_filter_batch(spng_ctx *c, const spng_image_desc *descs, uint32_t count,
                          spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    std::vector<FilterJob> jobs;
    std::vector<uint64_t> sizes(count);
    uint32_t max_rows = 1;
    for (uint32_t i = 0; i < count; ++i) {
        const spng_image_desc &d = descs[i];
        if (!valid_format(d.depth, d.channels) || !d.d_rows || !d.d_storage) return SPNG_E_ARGUMENT;
        const int volume = d.depth * d.channels;
        sizes[i] = spng_inflated_size(d.width, d.height, d.depth, d.channels, d.interlaced);
        if (d.rows_cap < sizes[i]) return SPNG_E_ARGUMENT;
        Pass p[7];
        const int np = passes(d.width, d.height, volume, d.interlaced, p);
        uint64_t off = 0;
        for (int z = 0; z < np; ++z) {
            FilterJob j;
            j.storage = (const uint8_t *)d.d_storage;
            j.rows = (uint8_t *)d.d_rows + off;
            j.row_stride = p[z].pitch + 1;
            j.sub_w = p[z].w; j.sub_h = p[z].h; j.width = d.width;
            j.bx = p[z].bx; j.by = p[z].by; j.sx = p[z].sx; j.sy = p[z].sy;
            j.depth = d.depth; j.channels = d.channels; j.pitch = (uint32_t)p[z].pitch;
            jobs.push_back(j);
            if (p[z].h > max_rows) max_rows = p[z].h;
            off += (p[z].pitch + 1) * (uint64_t)p[z].h;
        }
    }
    const size_t need = jobs.size() * sizeof(FilterJob) + count * (sizeof(spng_result) + 8) + 2048;
    if (int32_t st = c->reserve(need)) return st;
    Arena a{c};
    const size_t jslot = a.take(jobs.size() * sizeof(FilterJob));
    const size_t wslot = a.take(count * 8);
    if (!jobs.empty()) memcpy(a.host<FilterJob>(jslot), jobs.data(), jobs.size() * sizeof(FilterJob));
    memcpy(a.host<uint64_t>(wslot), sizes.data(), count * 8);
    const size_t upload = a.off;
    const size_t res = a.take(count * sizeof(spng_result));
    if (int32_t st = c->upload(0, upload)) return st;
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(res);
    {
        Timed t(c, SPNG_K_FILTER);
        HIP_TRY(launch_filter(a.dev<FilterJob>(jslot), (uint32_t)jobs.size(), max_rows, c->stream));
    }
    init_results_kernel<<<(count + 255) / 256, 256, 0, c->stream>>>(dr, a.dev<uint64_t>(wslot), count);
    HIP_TRY(hipGetLastError());
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

int32_t spng_filter(spng_ctx *c, const void *storage,
                    uint32_t w, uint32_t h, int depth, int channels, int interlaced,
                    void *rows, spng_result *result)
{
    if (!c || !storage || !rows || !result || !valid_format(depth, channels)) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t u = spng_inflated_size(w, h, depth, channels, interlaced);
    const uint64_t s = spng_storage_size(w, h, depth, channels);
    DevBuf dr, dst;
    HIP_TRY(dr.alloc(u)); HIP_TRY(dst.alloc_from(storage, s, c->stream));
    spng_image_desc d{};
    d.d_rows = dr.p; d.rows_cap = u; d.d_storage = dst.p; d.width = w; d.height = h;
    d.depth = (uint8_t)depth; d.channels = (uint8_t)channels; d.interlaced = (uint8_t)(interlaced != 0);
    if (int32_t st = spng_filter_batch(c, &d, 1, nullptr, result)) return st;
    HIP_TRY(dr.copy_to(rows, u));
    return SPNG_DONE;
}

uint64_t spng_deflate_bound(uint64_t n) { return n + n / 4 + 4096; }   // (covers the 18 bytes of a gzip wrapper too)

// The context's deflate slab (c->d_graph) for a plan of stream groups: plan(budget, single) cuts the groups for a budget and
// returns the bytes they need (single: every group is one stream).  The budget is SPNG_CFG_DEFLATE_BYTES, or half of the free
// memory, and at least `floor`.  When hipMalloc cannot give that much, the budget is halved and the groups cut again, down to
// one stream per group.  (A launch of this call may still read the slab: it is waited for before the slab moves.)
static int32_t deflate_slab(spng_ctx *c, uint64_t floor, const std::function<uint64_t(uint64_t, bool &)> &plan)
{
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    uint64_t budget = c->cfg[SPNG_CFG_DEFLATE_BYTES] ? (uint64_t)c->cfg[SPNG_CFG_DEFLATE_BYTES] : (uint64_t)(free_b + c->graph_cap) / 2;
    if (budget < floor) budget = floor;
    for (;;) {
        bool single = false;
        const uint64_t slab = plan(budget, single);
        bool failed = false;
        if (int32_t st = c->grow(c->d_graph, c->graph_cap, slab, 0, &failed)) return st;
        if (!failed) return SPNG_DONE;
        if (single) return fail_text("deflate: no device memory for the search scratch of a single stream");
        budget /= 2;
    }
}

// The rounds of one group of deflate streams: the search of round r + 1 beside the parse of round r, on a stream of its own
// (candidates are a function of the input alone; the parse is a wave or two per stream and leaves most of the chip idle): two
// sets of records, by round parity.  searched[p] / parsed[p] (c->ev_dfl[p] / [2 + p]): the last search into / parse out of the
// records of parity p.  search(parity) launches on c->stream2, parse(parity) on c->stream.
static int32_t deflate_round_pipeline(spng_ctx *c, uint32_t rounds, const std::function<hipError_t(uint32_t)> &search,
                                      const std::function<hipError_t(uint32_t)> &parse)
{
    if (int32_t st = second_stream(c)) return st;
    if (!c->ev_dfl[0]) for (hipEvent_t &e : c->ev_dfl) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t par = r & 1;
        if (r >= 2) HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_dfl[2 + par], 0));     // the parse of round r - 2 is done with these records
        { Timed t(c, SPNG_K_DFL_SEARCH, c->stream2); HIP_TRY(search(par)); }
        HIP_TRY(hipEventRecord(c->ev_dfl[par], c->stream2));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_dfl[par], 0));
        { Timed t(c, SPNG_K_DFL_PARSE); HIP_TRY(parse(par)); }
        HIP_TRY(hipEventRecord(c->ev_dfl[2 + par], c->stream));
    }
    return SPNG_DONE;
}

// One pass of the two-kernel full search (deflate.hip, "round 4") over jobs[0, n): per stream 11 bytes of scratch per vertex of
// a round (<= 2^21 vertices), rings for the search workgroups and, per group of streams, two pools of candidate words (one per
// round parity) -- all from the context's slab; streams whose scratch does not fit side by side go in groups.  The pools take
// what the budget leaves (at least 64 MiB) or, `worst`, their group's worst case: a position leaves at most min(attempts, 30)
// words and a pool starts empty at every search launch, so that no stream of the group can run dry.  The stream table and the
// states are the arena's slots sslot / tslot.
static int32_t deflate_full_pass(spng_ctx *c, const DeflateJob *jobs, size_t n, bool worst, spng_result *dr, Arena &a, size_t sslot, size_t tslot)
{
    auto scratch_of = [](uint64_t len) -> uint64_t {
        const uint64_t V = deflate2_vertices(len), B = V / 64 + 2;
        // (the candidate records twice: round r + 1 is searched while round r is parsed)
        return 2 * (((2 * V + 255) & ~255ull) + ((8 * B + 255) & ~255ull) + ((4 * B + 255) & ~255ull)) + ((8 * B + 255) & ~255ull) +
               2 * ((4 * (V + 2) + 255) & ~255ull) + ((V + 2 + 255) & ~255ull) + ((B + 255) & ~255ull);
    };
    auto pool_of = [](const DeflateJob &j) -> uint64_t {      // (14 words per position at level 8, 20 at level 9, 30 from level 10 on)
        const uint64_t per = j.level <= 8 ? 14 : j.level == 9 ? 20 : 30;
        return (j.src_len < (1u << 21) ? j.src_len : (1u << 21)) * per * 4;
    };
    uint64_t largest = 0, worst_pool = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t sc = scratch_of(jobs[i].src_len);
        largest = sc > largest ? sc : largest;
        worst_pool += pool_of(jobs[i]);
    }
    const uint64_t min_pool = 64ull << 20;
    struct Lay { size_t first, last; uint64_t scratch, rings, pool; uint32_t cps, chunk; };
    std::vector<Lay> lay;
    auto plan = [&](uint64_t budget, bool &single) -> uint64_t {
        lay.clear(); single = true;
        uint64_t slab = 0;
        for (size_t i = 0; i < n;) {
            // the group: streams whose scratch takes at most 2 / 3 of the budget (the rest is rings and pool) -- or, worst, whose
            // scratch, rings and worst-case pools fit it
            Lay l{i, i, 0, 0, 0, 0, 0};
            uint64_t wp = 0;
            while (l.last < n) {
                const uint64_t sc = l.scratch + scratch_of(jobs[l.last].src_len), p = wp + pool_of(jobs[l.last]);
                const uint64_t need = worst ? sc + deflate2_temp_bytes((uint32_t)(l.last + 1 - i) * search_chunks(l.last + 1 - i).cps) + 2 * (p + 512) + 4096 : sc;
                if (l.last > i && need > (worst ? budget : budget * 2 / 3)) break;
                l.scratch = sc; wp = p; ++l.last;
            }
            const uint32_t cnt = (uint32_t)(l.last - i);
            const SearchChunks chunks = search_chunks(cnt);
            l.cps = chunks.cps; l.chunk = chunks.chunk_len;
            l.rings = deflate2_temp_bytes(cnt * l.cps);           // (the searchers' word scratch; round 4: a 256 KiB link ring per workgroup)
            if (worst) l.pool = (wp + 255) & ~255ull;
            else {
                const uint64_t room = budget > l.scratch + l.rings ? budget - l.scratch - l.rings : 0;
                l.pool = worst_pool < room / 2 ? worst_pool : room / 2;
                if (l.pool < min_pool) l.pool = min_pool;
                l.pool &= ~255ull;
            }
            const uint64_t tot = l.scratch + l.rings + 2 * (l.pool + 256) + 4096;
            slab = tot > slab ? tot : slab;
            single = single && cnt == 1;
            lay.push_back(l);
            i = l.last;
        }
        return slab;
    };
    if (int32_t st = deflate_slab(c, worst ? 0 : largest + min_pool + (64ull << 20), plan)) return st;
    D2Stream *hs = a.host<D2Stream>(sslot);
    D2State *ht = a.host<D2State>(tslot);
    memset(ht, 0, n * sizeof(D2State));                        // (a zeroed state = a stream's beginning: dfl2_begin_kernel)
    std::vector<uint32_t> rounds_of(n, 1);
    for (const Lay &l : lay) {
        char *base = (char *)c->d_graph;
        uint64_t at = 0;
        auto take = [&](uint64_t bytes) { char *p = base + at; at += (bytes + 255) & ~255ull; return p; };
        for (size_t i = l.first; i < l.last; ++i) {
            const DeflateJob &j = jobs[i];
            D2Stream &s = hs[i];
            const uint64_t V = deflate2_vertices(j.src_len), B = V / 64 + 2;
            s.src = j.src; s.dst = j.dst; s.src_len = j.src_len; s.dst_cap = j.dst_cap; s.format = j.format; s.level = j.level;
            s.image = j.image; s.exponent = j.exponent; s.more = j.more; s.pad = 0;
            // (spng_deflate_resume_batch: the caller's state, kept from push to push; else the call's own)
            s.state = j.state ? (D2State *)j.state : a.dev<D2State>(tslot) + i;
            s.vinfo = (uint16_t *)take(2 * V); s.bbase = (uint64_t *)take(8 * B); s.bwords = (uint32_t *)take(4 * B); s.emask = (uint64_t *)take(8 * B);
            s.vinfo2 = (uint16_t *)take(2 * V); s.bbase2 = (uint64_t *)take(8 * B); s.bwords2 = (uint32_t *)take(4 * B);
            s.up = (uint32_t *)take(4 * (V + 2)); s.step = (uint32_t *)take(4 * (V + 2)); s.pathb = (uint8_t *)take(V + 2); s.litb = (uint8_t *)take(B);
            uint64_t pos = j.state ? j.plan_pos : 0;
            uint32_t lim = j.state && j.plan_limit ? j.plan_limit : 2048;
            rounds_of[i] = deflate2_plan(j.src_len, j.more != 0, pos, lim);
        }
    }
    if (int32_t st = c->upload(sslot, tslot + n * sizeof(D2State))) return st;
    for (const Lay &l : lay) {
        const uint32_t cnt = (uint32_t)(l.last - l.first);
        char *rings = (char *)c->d_graph + ((l.scratch + 255) & ~255ull);
        char *pools[2] = {rings + l.rings, rings + l.rings + l.pool + 256};       // (each followed by its bump counter)
        uint32_t rounds = 0;
        for (size_t i = l.first; i < l.last; ++i) rounds = rounds_of[i] > rounds ? rounds_of[i] : rounds;
        const D2Stream *ds = a.dev<D2Stream>(sslot) + l.first;
        HIP_TRY(launch_deflate2_begin(ds, cnt, c->stream));
        // (two pools too, by round parity)
        auto search = [&](uint32_t par) {
            return launch_deflate2_search(ds, cnt, l.cps, l.chunk, (uint32_t *)pools[par], (unsigned long long *)(pools[par] + l.pool), l.pool / 4,
                                          (uint32_t *)rings, par, c->stream2);
        };
        auto parse = [&](uint32_t par) { return launch_deflate2_parse(ds, cnt, (uint32_t *)pools[par], dr, par, c->stream); };
        if (int32_t st = deflate_round_pipeline(c, rounds, search, parse)) return st;
    }
    return SPNG_DONE;
}

// The full search for sorted[first, last).  Streams the pool could not serve (a batch of very compressible streams on little
// memory) come back unfinished and go through the rounds once more, with pools of their worst case.
static int32_t deflate_full_rounds(spng_ctx *c, std::vector<DeflateJob> &sorted, size_t first, size_t last, spng_result *dr, Arena &a)
{
    if (first >= last) return SPNG_DONE;
    const size_t nfull = last - first;
    // the stream table, the device-side states, who is not finished: in the arena, once (the second pass takes the same slots)
    const size_t sslot = a.take(nfull * sizeof(D2Stream)), tslot = a.take(nfull * sizeof(D2State)), fslot = a.take((nfull + 1) * 4);
    std::vector<uint32_t> failed;
    auto unfinished = [&](size_t n) -> int32_t {
        HIP_TRY(launch_deflate2_failed(a.dev<D2Stream>(sslot), (uint32_t)n, a.dev<uint32_t>(fslot), c->stream));
        failed.assign(n + 1, 0);
        return read_back(c, failed.data(), a.dev<uint32_t>(fslot), (n + 1) * 4);
    };
    if (int32_t st = deflate_full_pass(c, sorted.data() + first, nfull, false, dr, a, sslot, tslot)) return st;
    if (int32_t st = unfinished(nfull)) return st;
    for (size_t i = 0; i < nfull; ++i) if (failed[1 + i] == 1 && sorted[first + i].more) { failed[1 + i] = 0; failed[0] -= 1; }   // (a push that is not the last is never "finished")
    for (size_t i = 0; i < nfull; ++i)
        if (failed[1 + i] && sorted[first + i].state) {
            snprintf(g_err, sizeof g_err, "spng_deflate_resume_batch: the candidate pool ran dry under stream %u (raise SPNG_CFG_DEFLATE_BYTES)", sorted[first + i].image);
            return SPNG_E_DEVICE;
        }
    if (!failed[0]) return SPNG_DONE;
    std::vector<DeflateJob> again;
    for (size_t i = 0; i < nfull; ++i) if (failed[1 + i]) again.push_back(sorted[first + i]);
    if (int32_t st = deflate_full_pass(c, again.data(), again.size(), true, dr, a, sslot, tslot)) return st;
    if (int32_t st = unfinished(again.size())) return st;
    if (failed[0]) return fail_text("deflate: a stream is unfinished after a pass with pools of its worst case");
    return SPNG_DONE;
}

// Levels 0-7 in rounds (deflate.hip, "round 5"): the chip-wide search leaves one word per position, a parse wave per stream walks
// them.  Per stream two sets of 4 bytes per position of a round (<= 2^21 positions; the search of round r + 1 beside the parse of
// round r) from the context's slab, streams that do not fit side by side in groups.
static int32_t deflate_fast_rounds(spng_ctx *c, std::vector<DeflateJob> &sorted, size_t first, size_t last, spng_result *dr, Arena &a)
{
    if (first >= last) return SPNG_DONE;
    const size_t nfast = last - first;
    const uint64_t RV = deflate3_round_positions();
    // one-shot streams first: their blocks are written side by side (dfl4_*); streams that arrive in pieces keep their state
    // between calls and take the two-wave parse (dfl3_parse_kernel)
    std::stable_partition(sorted.begin() + first, sorted.begin() + last, [](const DeflateJob &j) { return !j.state && !j.more; });
    size_t mid = first;
    while (mid < last && !sorted[mid].state && !sorted[mid].more) ++mid;
    // what a call searches: from where the previous push left the search (plan_aux) to the end the input allows
    auto span_of = [&](const DeflateJob &j) -> uint64_t {
        const uint64_t from = j.state ? j.plan_aux : 0, E = deflate3_end(j.src_len, j.more != 0);
        return E > from ? E - from : 0;
    };
    auto round_of = [&](const DeflateJob &j) -> uint64_t { const uint64_t sp = span_of(j); return sp < RV ? sp : RV; };
    auto al = [](uint64_t b) -> uint64_t { return (b + 255) & ~255ull; };
    // (dfl4_scan / dfl4_place find a block's first bit at bbits[launch's max_blocks + k]: every stream's bbits is sized by the
    // largest block count of the call, not by its own -- ADVICE r5: a short stream beside a long one had its staged bits overwritten)
    uint64_t mb_all = 0;
    for (size_t i = first; i < mid; ++i) { const uint64_t mb = deflate4_max_blocks(round_of(sorted[i])); mb_all = mb > mb_all ? mb : mb_all; }
    auto scratch_of = [&](const DeflateJob &j, bool blocks) -> uint64_t {
        const uint64_t V = round_of(j) + 64;
        uint64_t b = 2 * al(4 * V);
        if (blocks) {
            const uint64_t mb = deflate4_max_blocks(round_of(j));
            b += al(4 * (V + 4096)) + al(4 * (4 + 2 * mb)) + al(16 * mb_all) + al(mb * deflate4_block_bytes() + 64);
        }
        return b;
    };
    struct Group { size_t first, last; bool blocks; };
    std::vector<Group> groups;
    auto plan = [&](uint64_t budget, bool &single) -> uint64_t {
        groups.clear(); single = true;
        uint64_t slab = 0;
        for (size_t i = first; i < last;) {
            const bool blocks = i < mid;
            const size_t stop = blocks ? mid : last;
            uint64_t used = 0;
            size_t k = i;
            while (k < stop) {
                const uint64_t sc = scratch_of(sorted[k], blocks);
                if (used + sc > budget && k > i) break;
                used += sc; ++k;
            }
            slab = used > slab ? used : slab;
            single = single && k == i + 1;
            groups.push_back({i, k, blocks});
            i = k;
        }
        return slab + 4096;
    };
    if (int32_t st = deflate_slab(c, 0, plan)) return st;
    const size_t sslot = a.take(nfast * sizeof(D3Stream)), tslot = a.take(nfast * sizeof(D1State));
    D3Stream *hs = a.host<D3Stream>(sslot);
    // (a zeroed state = a stream's beginning: dfl3_begin_kernel)
    for (size_t i = 0; i < nfast; ++i) memset(a.host<D1State>(tslot) + i, 0, sizeof(D1State));
    std::vector<uint32_t> rounds_of(nfast, 1), maxb_of(nfast, 0);
    for (auto &gr : groups) {
        char *base = (char *)c->d_graph;
        uint64_t at = 0;
        auto take = [&](uint64_t bytes) { char *p = base + at; at += al(bytes); return p; };
        for (size_t i = gr.first; i < gr.last; ++i) {
            const DeflateJob &j = sorted[i];
            D3Stream &s = hs[i - first];
            memset(&s, 0, sizeof s);
            const uint64_t V = round_of(j) + 64;
            s.src = j.src; s.dst = j.dst; s.src_len = j.src_len; s.dst_cap = j.dst_cap; s.format = j.format; s.level = j.level;
            s.image = j.image; s.exponent = j.exponent; s.more = j.more; s.pad = 0;
            s.state = j.state ? j.state : a.dev<D1State>(tslot) + (i - first);
            s.match[0] = (uint32_t *)take(4 * V); s.match[1] = (uint32_t *)take(4 * V);
            if (gr.blocks) {
                const uint64_t mb = deflate4_max_blocks(round_of(j));
                s.terms = (uint32_t *)take(4 * (V + 4096)); s.bdesc = (uint32_t *)take(4 * (4 + 2 * mb));
                s.bbits = (uint64_t *)take(16 * mb_all); s.scratch = (uint8_t *)take(mb * deflate4_block_bytes() + 64);
                maxb_of[i - first] = (uint32_t)mb;
            }
            const uint64_t sp = span_of(j);
            rounds_of[i - first] = sp ? (uint32_t)((sp + RV - 1) / RV) : 1u;   // (one launch at least: it reports where the stream stands)
        }
    }
    if (int32_t st = c->upload(sslot, tslot + nfast * sizeof(D1State))) return st;
    for (auto &gr : groups) {
        const uint32_t cnt = (uint32_t)(gr.last - gr.first);
        const SearchChunks chunks = search_chunks(cnt);
        uint32_t rounds = 0, maxb = 0;
        for (size_t i = gr.first; i < gr.last; ++i) {
            rounds = rounds_of[i - first] > rounds ? rounds_of[i - first] : rounds;
            maxb = maxb_of[i - first] > maxb ? maxb_of[i - first] : maxb;
        }
        const D3Stream *ds = a.dev<D3Stream>(sslot) + (gr.first - first);
        HIP_TRY(launch_deflate3_begin(ds, cnt, c->stream));
        auto search = [&](uint32_t par) { return launch_deflate3_search(ds, cnt, chunks.cps, chunks.chunk_len, par, c->stream2); };
        auto parse = [&](uint32_t par) {
            return gr.blocks ? launch_deflate4_round(ds, cnt, maxb, dr, par, c->stream) : launch_deflate3_parse(ds, cnt, dr, par, c->stream);
        };
        if (int32_t st = deflate_round_pipeline(c, rounds, search, parse)) return st;
    }
    return SPNG_DONE;
}

// shared by spng_deflate_batch / spng_encode_batch
static int32_t deflate_launch(spng_ctx *c, std::vector<DeflateJob> &jobs, spng_result *dr, Arena &a, size_t jslot,
                              size_t gzparts = (size_t)-1)
{
    // greedy / lazy streams first, then the full-search ones: two contiguous job tables
    std::vector<DeflateJob> sorted;
    sorted.reserve(jobs.size());
    for (auto &j : jobs) if (j.level < 8) sorted.push_back(j);
    const size_t nfast = sorted.size();
    for (auto &j : jobs) if (j.level >= 8) sorted.push_back(j);
    if (nfast) {
        Timed t(c, SPNG_K_DEFLATE);
        if (int32_t st = deflate_fast_rounds(c, sorted, 0, nfast, dr, a)) return st;
    }
    memcpy(a.host<DeflateJob>(jslot), sorted.data(), sorted.size() * sizeof(DeflateJob));
    if (int32_t st = c->upload(jslot, jslot + sorted.size() * sizeof(DeflateJob))) return st;
    {
        Timed t(c, SPNG_K_DEFLATE);
        if (int32_t st = deflate_full_rounds(c, sorted, nfast, sorted.size(), dr, a)) return st;
    }
    // gzip members: CRC-32 and byte count of the input behind the stream (DeflatorBuffers.swift:96-135)
    if (gzparts != (size_t)-1)
        HIP_TRY(launch_gzip_deflate_post(a.dev<DeflateJob>(jslot), dr, a.dev<uint32_t>(gzparts), (uint32_t)sorted.size(), c->stream));
    return SPNG_DONE;
}

// One-shot streams (d_states == NULL) and streams that arrive in pieces (spng_deflate_resume_batch: d_states, last, h_state).
static int32_t deflate_batch(spng_ctx *c, const spng_stream_desc *descs, const int32_t *levels, void *const *d_states, const uint8_t *last,
                             const uint64_t *h_state, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || !levels) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    std::vector<DeflateJob> jobs(count);
    bool gzip = false;
    for (uint32_t i = 0; i < count; ++i) {
        // spng_stream_desc.reserved: window exponent 8 ... 15 (0 = 15, as PNG always uses)
        const int32_t e = descs[i].reserved ? descs[i].reserved : 15;
        if ((!descs[i].d_src && descs[i].src_len) || !descs[i].d_dst || (d_states && !d_states[i]) || e < 8 || e > 15 ||
            descs[i].format < SPNG_FORMAT_ZLIB || descs[i].format > SPNG_FORMAT_GZIP) return SPNG_E_ARGUMENT;
        gzip = gzip || descs[i].format == SPNG_FORMAT_GZIP;
        DeflateJob j{};
        j.src = (const uint8_t *)descs[i].d_src; j.dst = (uint8_t *)descs[i].d_dst; j.src_len = descs[i].src_len; j.dst_cap = descs[i].dst_cap;
        j.format = descs[i].format; j.level = levels[i]; j.image = i; j.exponent = descs[i].format == SPNG_FORMAT_IOS ? 15u : (uint32_t)e;
        if (d_states) {
            j.more = last[i] ? 0u : 1u; j.state = (D1State *)d_states[i];
            if (h_state) { j.plan_pos = h_state[2 * i]; j.plan_limit = (uint32_t)h_state[2 * i + 1]; j.plan_aux = h_state[2 * i + 1]; }
            // (a state is only ever what an earlier call handed out: the search position it names lies inside what the input allows --
            // the match arrays and the round count of levels 0-7 are sized from it)
            if (j.plan_pos > j.src_len || (levels[i] < 8 && j.plan_aux > deflate3_end(j.src_len, j.more != 0))) return SPNG_E_ARGUMENT;
        }
        jobs[i] = j;
    }
    if (int32_t st = c->reserve(count * (sizeof(DeflateJob) + sizeof(spng_result) + sizeof(D2Stream) + sizeof(D2State) + sizeof(D3Stream) + sizeof(D1State) + 1024 + (gzip ? 4 * (size_t)gzip_pieces() : 0)) + 8192)) return st;
    Arena a{c};
    const size_t jslot = a.take(count * sizeof(DeflateJob));
    const size_t res = a.take(count * sizeof(spng_result));
    const size_t gzparts = gzip ? a.take((size_t)count * 4 * gzip_pieces()) : (size_t)-1;
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(res);
    if (int32_t st = deflate_launch(c, jobs, dr, a, jslot, gzparts)) return st;
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

int32_t spng_deflate_batch(spng_ctx *c, const spng_stream_desc *descs, const int32_t *levels, uint32_t count,
                           spng_result *d_results, spng_result *h_results)
{
    return deflate_batch(c, descs, levels, nullptr, nullptr, nullptr, count, d_results, h_results);
}

uint64_t spng_deflate_state_bytes(void) { return deflate_state_bytes(); }

int32_t spng_deflate_resume_batch(spng_ctx *c, const spng_stream_desc *descs, const int32_t *levels, void *const *d_states, const uint8_t *last,
                                  const uint64_t *h_state, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    if (!d_states || !last) return SPNG_E_ARGUMENT;
    return deflate_batch(c, descs, levels, d_states, last, h_state, count, d_results, h_results);
}

int32_t spng_deflate(spng_ctx *c, const void *src, uint64_t n, int32_t format, int32_t level,
                     void *dst, uint64_t cap, spng_result *result)
{
    return spng_deflate_window(c, src, n, format, level, 15, dst, cap, result);
}

int32_t spng_deflate_window(spng_ctx *c, const void *src, uint64_t n, int32_t format, int32_t level, int32_t exponent,
                            void *dst, uint64_t cap, spng_result *result)
{
    if (!c || (!src && n) || !dst || !result || exponent < 8 || exponent > 15) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf ds, dd;
    HIP_TRY(ds.alloc(n + 8)); HIP_TRY(dd.alloc(cap));
    HIP_TRY(hipMemcpyAsync(ds.p, src, n, hipMemcpyHostToDevice, c->stream));
    spng_stream_desc d{ds.p, n, dd.p, cap, format, exponent};
    if (int32_t st = spng_deflate_batch(c, &d, &level, 1, nullptr, result)) return st;
    const uint64_t w = result->written < cap ? result->written : cap;
    HIP_TRY(dd.copy_to(dst, w));
    return SPNG_DONE;
}

int32_t spng_encode_batch(spng_ctx *c, const spng_image_desc *descs, int32_t level, uint32_t count,
                          spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    // filter-select (own lock), then deflate of the filtered scanlines
    if (int32_t st = spng_filter_batch(c, descs, count, d_results, nullptr)) return st;
    std::vector<spng_stream_desc> sd(count);
    std::vector<int32_t> lv(count, level);
    for (uint32_t i = 0; i < count; ++i) {
        const spng_image_desc &d = descs[i];
        if (!d.d_idat) return SPNG_E_ARGUMENT;
        sd[i] = spng_stream_desc{d.d_rows, spng_inflated_size(d.width, d.height, d.depth, d.channels, d.interlaced),
                                 (void *)d.d_idat, d.idat_len, d.format, 0};
    }
    return spng_deflate_batch(c, sd.data(), lv.data(), count, d_results, h_results);
}

}  // extern "C"
