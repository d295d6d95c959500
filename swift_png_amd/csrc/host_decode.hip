// host_decode.hip -- host side of the decode stages: the entries of the C ABI for inflate, unfilter and decode (one-shot, resumed,
// host-pointer forms, several devices), with the plans they stage -- the unfilter jobs of a batch, the segments, token pool and parts
// of the parallel inflate pipeline -- and the kernels that initialise and finish a batch's results.
#include "host.hpp"
#include "geometry.hpp"

// ------------------------------------------------------------------------------------------------
namespace spng {

__global__ void finish_decode_kernel(spng_result *results, const uint64_t *expected, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int32_t st = results[i].status;
    // PNG.Decoder.swift:142-147: anything left in the inflator after the last row
    if (st == SPNG_E_OUTPUT_CAPACITY ||
        ((st == SPNG_DONE || st == SPNG_NEED_MORE_INPUT) && results[i].written > expected[i]))
        results[i].status = SPNG_E_EXTRANEOUS_IMAGE_DATA;
}

// A stream whose waves gave up on each other (inflate.hip: SPIN_LIMIT) never writes its result: such
// a slot must read as a device error that wrote and consumed nothing.
__global__ void poison_results_kernel(spng_result *results, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    results[i].status = SPNG_E_DEVICE; results[i].reserved = 0;
    results[i].written = 0; results[i].consumed = 0;
    results[i].aux[0] = results[i].aux[1] = 0;
}

__global__ void init_results_kernel(spng_result *results, const uint64_t *written, uint32_t count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    results[i].status = SPNG_DONE; results[i].reserved = 0;
    results[i].written = written[i]; results[i].consumed = 0;
    results[i].aux[0] = results[i].aux[1] = 0;
}

// Plans and launches the unfilter (+ scatter) stage for a batch.  rows_len_of(i) gives the device
// address holding the number of valid inflated bytes of image i (or null).
struct UnfilterPlan {
    std::vector<UnfJob> unf[9];          // indexed by bpp
    std::vector<ScatterJob> scat;
    std::vector<uint32_t> scat_image;
    std::vector<OverdrawJob> over;       // spng_unfilter_resume_batch with SPNG_IMAGE_OVERDRAW
};

static int32_t plan_unfilter(const spng_image_desc *descs, uint32_t count, UnfilterPlan &plan,
                             const uint64_t *(*rows_len_of)(void *, uint32_t), void *user)
{
    for (uint32_t i = 0; i < count; ++i) {
        const spng_image_desc &d = descs[i];
        if (!valid_format(d.depth, d.channels) || !d.d_rows || !d.d_storage) return SPNG_E_ARGUMENT;
        const int volume = d.depth * d.channels;
        const uint32_t bpp = (uint32_t)(volume + 7) >> 3;
        const uint64_t u = spng_inflated_size(d.width, d.height, d.depth, d.channels, d.interlaced);
        if (d.rows_cap < u) return SPNG_E_ARGUMENT;
        Pass p[7];
        const int np = passes(d.width, d.height, volume, d.interlaced, p);
        const bool direct = !d.interlaced && volume >= 8;   // rows land in storage as they are
        uint64_t off = 0;
        for (int z = 0; z < np; ++z) {
            UnfJob j;
            j.in = (const uint8_t *)d.d_rows + off;
            j.in_stride = p[z].pitch + 1;
            if (direct) { j.out = (uint8_t *)d.d_storage; j.out_stride = p[z].pitch; }
            else        { j.out = (uint8_t *)d.d_rows + off + 1; j.out_stride = p[z].pitch + 1; }
            j.stream_off = off;
            j.rows_len = rows_len_of(user, i);
            j.pitch = (uint32_t)p[z].pitch; j.rows = p[z].h; j.image = i; j.bpp = bpp; j.has_prev = 0; j.pad = 0;
            plan.unf[bpp].push_back(j);
            if (!direct) {
                ScatterJob s;
                s.rows = (const uint8_t *)d.d_rows + off + 1;
                s.storage = (uint8_t *)d.d_storage;
                s.row_stride = p[z].pitch + 1; s.stream_off = off; s.rows_len = j.rows_len;
                s.sub_w = p[z].w; s.sub_h = p[z].h; s.width = d.width;
                s.bx = p[z].bx; s.by = p[z].by; s.sx = p[z].sx; s.sy = p[z].sy;
                s.depth = d.depth; s.channels = d.channels;
                plan.scat.push_back(s);
                plan.scat_image.push_back(i);
            }
            off += (p[z].pitch + 1) * (uint64_t)p[z].h;
        }
    }
    return SPNG_DONE;
}

static size_t plan_bytes(const UnfilterPlan &plan)
{
    size_t b = 0;
    for (int k = 1; k <= 8; ++k) b += plan.unf[k].size() * sizeof(UnfJob) + 256;
    b += plan.scat.size() * (sizeof(ScatterJob) + 4) + 512;
    b += plan.over.size() * sizeof(OverdrawJob) + 256;
    return b;
}

// copies the plan into the arena (host side) and launches after the caller's upload
struct PlanSlots { size_t unf[9]; size_t scat, scat_image, over; };

static void stage_plan(const UnfilterPlan &plan, Arena &a, PlanSlots &slots)
{
    for (int k = 1; k <= 8; ++k) {
        slots.unf[k] = a.take(plan.unf[k].size() * sizeof(UnfJob));
        if (!plan.unf[k].empty())
            memcpy(a.host<UnfJob>(slots.unf[k]), plan.unf[k].data(), plan.unf[k].size() * sizeof(UnfJob));
    }
    slots.scat = a.take(plan.scat.size() * sizeof(ScatterJob));
    slots.scat_image = a.take(plan.scat.size() * 4);
    if (!plan.scat.empty()) {
        memcpy(a.host<ScatterJob>(slots.scat), plan.scat.data(), plan.scat.size() * sizeof(ScatterJob));
        memcpy(a.host<uint32_t>(slots.scat_image), plan.scat_image.data(), plan.scat.size() * 4);
    }
    slots.over = a.take(plan.over.size() * sizeof(OverdrawJob));
    if (!plan.over.empty()) memcpy(a.host<OverdrawJob>(slots.over), plan.over.data(), plan.over.size() * sizeof(OverdrawJob));
}

static int32_t launch_plan(spng_ctx *c, const UnfilterPlan &plan, Arena &a, const PlanSlots &slots,
                           spng_result *d_results)
{
    {
        Timed t(c, SPNG_K_UNFILTER);
        for (int k = 1; k <= 8; ++k)
            if (!plan.unf[k].empty()) {
                // (chains are cut into pieces when there are few of them: geometry.hpp)
                uint64_t total_rows = 0; uint32_t max_rows = 1;
                for (auto &j : plan.unf[k]) { total_rows += j.rows; max_rows = j.rows > max_rows ? j.rows : max_rows; }
                uint64_t widest = 0;
                for (auto &j : plan.unf[k]) widest = (uint64_t)j.pitch > widest ? (uint64_t)j.pitch : widest;
                const UnfilterPieces cut = unfilter_pieces((uint32_t)k, total_rows, max_rows, widest, (uint32_t)c->cfg[SPNG_CFG_UNFILTER_PIECE_ROWS]);
                HIP_TRY(launch_unfilter(a.dev<UnfJob>(slots.unf[k]), (uint32_t)plan.unf[k].size(), k,
                                        d_results, cut.pieces, cut.piece_rows, c->stream, (uint32_t)(widest > 0xffffffffull ? 0xffffffffull : widest)));
            }
    }
    if (!plan.scat.empty()) {
        Timed t(c, SPNG_K_SCATTER);
        uint64_t maxpix = 1;
        for (auto &s : plan.scat) { uint64_t px = (uint64_t)s.sub_w * s.sub_h; if (px > maxpix) maxpix = px; }
        HIP_TRY(launch_scatter(a.dev<ScatterJob>(slots.scat), (uint32_t)plan.scat.size(),
                               a.dev<uint32_t>(slots.scat_image), d_results, plane_blocks_x(maxpix, SCATTER_BLOCKS_MAX), c->stream));
    }
    if (!plan.over.empty()) {
        Timed t(c, SPNG_K_SCATTER);
        uint64_t maxpix = 1;
        for (auto &o : plan.over) { uint64_t px = (uint64_t)o.width * (o.y1 - o.y0); if (px > maxpix) maxpix = px; }
        HIP_TRY(launch_overdraw(a.dev<OverdrawJob>(slots.over), (uint32_t)plan.over.size(), plane_blocks_x(maxpix, OVERDRAW_BLOCKS_MAX), c->stream));
    }
    return SPNG_DONE;
}

// ---- inflate stage: the parallel pipeline (pinflate2.hip) in front of the serial kernel (inflate.hip) ----
struct InflatePlan {
    std::vector<InflateJob> jobs;
    std::vector<PStream> streams;
    std::vector<PSeg> segs;
    size_t log_bytes = 0;
    bool parallel = false;
    // pinflate2: the token pool and the groups of streams that share it, one after the other
    uint32_t pool_pages = 0;
    struct Group { uint32_t s0, s1, g0, g1; };                 // streams, segments
    std::vector<Group> groups;
    std::vector<uint64_t> est;       // token bytes every stream is expected to take (planning only)
    uint32_t pmax = 0;               // several workgroups per stream: part slots per stream (0: one workgroup per stream)
    size_t parts_at = 0;
    size_t next_at = 0;
    bool gzip = false;               // some stream is SPNG_FORMAT_GZIP: header kernel in front, CRC-32 check behind
    std::vector<uint64_t> state;     // {bit, written} per stream: spng_inflate_resume_batch's, else the library's own zeros
    bool internal = true;            // (the latter)
    size_t jobs_at = 0, streams_at = 0, segs_at = 0, done_at = 0, gz_at = 0, gzparts_at = 0, state_at = 0, sumparts_at = 0;
    bool cuts = false;               // block cuts may be tried for some stream: a PCut per segment, device side only, behind everything
    size_t cuts_at = 0;              // else in the arena (take_cuts)
    size_t take_cuts(Arena &a) { if (cuts) cuts_at = a.take(segs.size() * sizeof(PCut)); return cuts_at; }
    size_t bytes() const
    {
        return jobs.size() * (sizeof(InflateJob) + sizeof(PStream) + 4 + (size_t)pmax * sizeof(PPart) + 256 + (gzip ? 8 + 4 * (size_t)gzip_pieces() : 0) +
                              (state.empty() ? 0 : 32 + 8 * (size_t)gzip_pieces())) +
               segs.size() * (sizeof(PSeg) + (cuts ? sizeof(PCut) : 0)) + 8192 + 1024;
    }
};

#ifndef SPNG_PARTS_MAX
#define SPNG_PARTS_MAX 128        // parts a stream's chain is cut into at most (round 5: 64 -- one to four images left half the chip idle)
#endif

// What the last batch taught about token volume (its page count comes back behind its kernels: when the planning
// figure would cut THIS batch into groups, waiting for that number is cheaper than not knowing it).
static int32_t learn_from_last_batch(spng_ctx *c, uint64_t total)
{
    if (c->pool_pending && c->pool_ratio == 0 && hipEventQuery(c->pool_ev) != hipSuccess) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        uint64_t room = c->cfg[SPNG_CFG_TOKEN_BYTES] ? (uint64_t)c->cfg[SPNG_CFG_TOKEN_BYTES] : (uint64_t)(free_b + c->tok_cap) / 2;
        if ((double)total * 3.2 > (double)room) HIP_TRY(hipEventSynchronize(c->pool_ev));
    }
    if (c->pool_pending && hipEventQuery(c->pool_ev) == hipSuccess) {
        c->pool_pending = false;
        const uint64_t used = c->h_pool_used[0], blocks = c->h_pool_used[2];
        if (c->h_pool_used[1]) c->pool_ratio = 0;                                   // it ran dry: back to the default
        else if (c->pool_src_pending > (1u << 20)) c->pool_ratio = (double)used * 65536.0 / (double)c->pool_src_pending;
        c->block_bytes = (blocks && c->pool_src_pending > (1u << 20)) ? (double)c->pool_src_pending / (double)blocks : 0;
    }
    return SPNG_DONE;
}

// Cuts every stream into segments of seg_bytes (p.streams, p.segs, the page-table entries they may take: p.log_bytes) and
// estimates the token bytes each stream will need (p.est).
static int32_t cut_into_segments(spng_ctx *c, InflatePlan &p, uint64_t seg_bytes)
{
    p.streams.resize(p.jobs.size());
    const double per_byte = c->pool_ratio > 0 ? (c->pool_ratio * 1.25 < 1.0 ? 1.0 : c->pool_ratio * 1.25) : 3.2;
    p.est.assign(p.jobs.size(), 0);
    size_t log = 0;
    for (size_t i = 0; i < p.jobs.size(); ++i) {
        const InflateJob &j = p.jobs[i];
        PStream &st = p.streams[i];
        memset(&st, 0, sizeof st);
        st.src = j.src; st.dst = j.dst; st.src_len = j.src_len; st.dst_cap = j.dst_cap;
        st.format = j.format; st.image = j.image;
        // Block cuts (pinflate2.hip).  A one-shot call: a stream long enough to hold a run of segments without a start.  A resumed call:
        // a state that is not all zero with that much input behind its resume point -- the token it stands at, else the block header --;
        // its segments are counted from there (seg_origin), and a state inside a block goes on at its token (tok_bit) instead of taking
        // the serial kernel or the block's header again.  A call with an all-zero state is a whole stream, for which
        // spng_inflate_batch is the entry: it keeps the plan it always had.
        const int64_t cb = c->cfg[SPNG_CFG_BLOCK_CUT_BYTES];
        const uint64_t cut_bytes = cb == 0 ? RESUME_SERIAL_BITS / 8 : (uint64_t)cb;
        uint64_t origin = 0;
        bool cut = p.internal && cb != SPNG_BLOCK_CUT_NEVER && j.src_len >= cut_bytes;
        if (!p.internal && cb != SPNG_BLOCK_CUT_NEVER) {
            const uint64_t *s4 = &p.state[4 * i];
            const uint64_t at = (s4[2] ? s4[2] : s4[0]) / 8;
            if ((s4[0] | s4[1] | s4[2] | s4[3]) && j.src_len >= at && j.src_len - at >= cut_bytes) {
                cut = true; st.cut_resumed = 1;
                origin = at & ~(uint64_t)255;
            }
        }
        if (!p.state.empty()) {
            st.start_bit = p.state[4 * i]; st.out_pos = p.state[4 * i + 1]; st.blk_out = st.out_pos;
            if (st.cut_resumed && p.state[4 * i + 2]) { st.tok_bit = p.state[4 * i + 2]; st.out_pos = p.state[4 * i + 3]; }
            // The caller's state stands inside a block.  A block of ordinary size is simply decoded again from its header by the
            // pipeline (cheaper than the serial kernel for everything behind it); one that has already taken more than
            // RESUME_SERIAL_BITS of input would make every push cost what all pushes before it did -- a stream that is ONE block
            // pushed in k pieces O(n k) --: the serial kernel goes on at the token the last push stopped in front of.
            // (Not with cuts: the pipeline goes on at that token itself.)
            if (!p.internal && !st.cut_resumed && p.state[4 * i + 2] && p.state[4 * i + 2] - p.state[4 * i] > RESUME_SERIAL_BITS) st.serial_only = 1;
        }
        st.seg_first = (uint32_t)p.segs.size();
        st.seg_origin = origin;
        const uint64_t span = j.src_len - origin;                  // (what the segments cover)
        uint64_t k = (span + seg_bytes - 1) / seg_bytes;
        if (k < 1) k = 1;
        if (p.segs.size() + k > 0x7fffffffu) return SPNG_E_ARGUMENT;
        st.seg_count = (uint32_t)k; st.seg_bytes = seg_bytes;
        if (cut) {
            // (whole segments: rounded up -- a resumed call down, so that what passed the gate above is not refused by the plan, which
            // counts the run of such a call from its first segment's start, at or in front of the resume point)
            const uint64_t cs = st.cut_resumed ? cut_bytes / seg_bytes : (cut_bytes + seg_bytes - 1) / seg_bytes;
            st.cut_segs = (uint32_t)(cs > 0x7fffffffu ? 0x7fffffffu : cs < 1 ? 1 : cs);
            p.cuts = true;
        }
        for (uint64_t q = 0; q < k; ++q) {
            PSeg sg;
            memset(&sg, 0, sizeof sg);
            sg.stream = (uint32_t)i; sg.index = (uint32_t)q;
            const uint64_t len = q + 1 < k ? seg_bytes : span - q * seg_bytes;
            // page-table entries: 16 token bytes per compressed byte at most, and never more than two per output byte
            uint64_t most = 16 * len;
            if (most > 2 * (j.dst_cap + 64)) most = 2 * (j.dst_cap + 64);
            sg.log_cap = (most >> 16) + 2;
            sg.log_off = log; log += sg.log_cap;
            sg.start_bit = ~0ull;
            p.segs.push_back(sg);
        }
        uint64_t e = (uint64_t)(per_byte * (double)span);
        if (e > 2 * (j.dst_cap + 64)) e = 2 * (j.dst_cap + 64);
        p.est[i] = e + k * 65536 + 65536;                                          // (every segment ends inside a page)
        // (block cuts: a cut segment's first chunks -- tokens nobody reads --, the padding of its records and its join's bridge take room
        // too, and EVERY segment of the stream ends inside a page, not only those with a start: a second page per segment.
        // Not for a stream whose like the last batch showed to be made of ordinary blocks: there nothing will be cut, and a batch of
        // 1024 images would ask for 10 GiB it never touches.  A wrong guess costs the stream the retry pass, not its result.)
        if (st.cut_segs && !(c->block_bytes > 0 && c->block_bytes < 262144)) p.est[i] += k * 65536;
    }
    p.log_bytes = log * 4;
    return SPNG_DONE;
}

// The page tables (c->d_log) and the token pool (c->d_tok), sized by the estimates within the budget.  No room for the pool:
// the plan is not parallel any more.
static int32_t size_token_pool(spng_ctx *c, InflatePlan &p)
{
    if (int32_t st = c->grow(c->d_log, c->log_cap, p.log_bytes, p.log_bytes / 8)) return st;
    uint64_t want = 0, largest = 0;
    for (auto e : p.est) { want += e; if (e > largest) largest = e; }
    uint64_t budget = (uint64_t)c->cfg[SPNG_CFG_TOKEN_BYTES];
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = (uint64_t)(free_b + c->tok_cap) / 2;
        if (budget < (64ull << 20)) budget = 64ull << 20;
    }
    if (budget < 2 * largest && !c->cfg[SPNG_CFG_TOKEN_BYTES]) budget = 2 * largest;
    uint64_t need = want < budget ? want : budget;
    if (need < largest) need = largest;                                            // (a stream is never split over groups)
    need = (need + 65535) & ~(uint64_t)65535;
    bool failed = false;
    if (int32_t st = c->grow(c->d_tok, c->tok_cap, need, 0, &failed)) return st;
    if (failed) {
        // no room for the pipeline: the serial kernel takes the batch
        p.parallel = false; p.streams.clear(); p.segs.clear();
    }
    return SPNG_DONE;
}

// Groups of consecutive streams whose estimates fit the pool together.
static void group_streams(const spng_ctx *c, InflatePlan &p)
{
    uint64_t want = 0, largest = 0;
    for (auto e : p.est) { want += e; if (e > largest) largest = e; }
    const uint64_t pool = c->tok_cap & ~(uint64_t)65535;
    p.pool_pages = (uint32_t)(pool >> 16 > 0xfffffff0ull ? 0xfffffff0ull : pool >> 16);
    // (as many groups as the estimates need, of equal share: 730 + 294 streams cost resolve three rounds of resident
    // workgroups where 512 + 512 cost two)
    uint64_t share = pool;
    if (want > pool) {
        const uint64_t ng = (want + pool - 1) / pool;
        share = (want + ng - 1) / ng;
        if (share < largest) share = largest;
        if (share > pool) share = pool;
    }
    uint64_t run = 0;
    InflatePlan::Group g{0, 0, 0, 0};
    for (size_t i = 0; i < p.jobs.size(); ++i) {
        if (run + p.est[i] > share && g.s1 > g.s0) {
            p.groups.push_back(g);
            g.s0 = g.s1; g.g0 = g.g1; run = 0;
        }
        run += p.est[i];
        g.s1 = (uint32_t)i + 1; g.g1 = p.streams[i].seg_first + p.streams[i].seg_count;
    }
    p.groups.push_back(g);
}

// Few streams: a workgroup per stream would leave most of the chip idle while each resolves its stream at ~0.9 GB/s
// (one 4K image: 77 ms of an 89 ms decode).  Then a stream's chain is cut into parts that resolve side by side
// (pinflate2.hip, "Several workgroups per stream"): 16-bit symbols in c->d_sym, the windows in c->d_win.
static int32_t plan_parts(spng_ctx *c, InflatePlan &p)
{
    p.pmax = 0;
    if (p.internal && p.jobs.size() <= 384 && c->cfg[SPNG_CFG_RESOLVE_PARTS] != 1) {
        // (512 workgroups in all: the marker parts run two to a CU -- pinflate2.hip, RGeo --, so that is one round of resident
        // workgroups; 768 left half a round behind: 128 images 41.6 ms of resolve against 33.5, 1024 parts 34.2)
        uint32_t pm = (uint32_t)(512 / p.jobs.size());
        if (pm < 2) pm = 2;
        if (c->cfg[SPNG_CFG_RESOLVE_PARTS] > 1) pm = (uint32_t)c->cfg[SPNG_CFG_RESOLVE_PARTS];
        if (pm > SPNG_PARTS_MAX) pm = SPNG_PARTS_MAX;
        if (c->cfg[SPNG_CFG_RESOLVE_PARTS] <= 1) {
            // (a part has fixed costs -- its first window, the hand-over of the windows part by part, the symbols' second pass --: not
            // below ~1 MiB of output each.  One 4K image: 64 parts 2.94 ms, 128 parts 3.81; the 8192^2 RGBA16 image of configs[4]:
            // 64 parts 11.1 ms, 128 parts 8.3: profiles/archive/r06x_probe_parts128.log)
            uint64_t most = 0;
            for (auto &j : p.jobs) most = j.dst_cap > most ? j.dst_cap : most;
            const uint64_t by_size = most >> 20 < 2 ? 2 : most >> 20;
            if (pm > by_size) pm = (uint32_t)by_size;
        }
        uint64_t syms = 0;
        for (size_t i = 0; i < p.jobs.size(); ++i) {
            p.streams[i].sym_off = syms;
            syms += (p.jobs[i].dst_cap + 15) & ~(uint64_t)7;
        }
        const uint64_t win = (uint64_t)p.jobs.size() * pm * 32768;
        // (the symbol scratch is two bytes per output byte: only when it fits a quarter of what is free, and not again after an
        // allocation of that size has failed -- a failed hipMalloc of gigabytes per call costs more than the parts save)
        bool afford = syms * 2 <= c->sym_cap;
        if (!afford && !(c->sym_failed && syms * 2 >= c->sym_failed)) {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            afford = syms * 2 + win <= (uint64_t)(free_b + c->sym_cap + c->win_cap) / 4;
        }
        if (pm >= 2 && afford) {
            bool failed = false;
            if (syms * 2 > c->sym_cap) {
                if (int32_t st = c->grow(c->d_sym, c->sym_cap, syms * 2, 0, &failed)) return st;
                c->sym_failed = failed ? syms * 2 : 0;
            }
            if (!failed)
                if (int32_t st = c->grow(c->d_win, c->win_cap, win, 0, &failed)) return st;
            if (!failed) {
                p.pmax = pm;
                for (auto &st : p.streams) st.parts_max = pm;
            }
        }
    }
    if (!p.pmax && c->d_sym && p.jobs.size() > 384) {
        // (a large batch after small ones: the symbol scratch -- two bytes per output byte -- goes back to the device)
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(c->d_sym)); c->d_sym = nullptr; c->sym_cap = 0;
    }
    return SPNG_DONE;
}

// Cuts every stream into segments and makes sure the context owns what the pipeline needs.  Segment length: long
// enough that the search for a block header (which costs more per bit than decoding) stays a small part of a
// segment's work, short enough that the batch yields several thousand segments, i.e. a few waves per SIMD.
//
// pinflate2 (the default): a page table per segment (c->d_log) and the token pool (c->d_tok, 64 KiB pages).  A
// compressed byte becomes at most 8 token halfwords and a stream at most one per output byte; what a batch really
// needs is far less (0.8 per byte for zlib-made PNG streams, 1.4 for swift-png's own), so the pool is sized by the
// ratio the previous batch showed (3.2 bytes per byte before there is one), capped by SPNG_CFG_TOKEN_BYTES or half of
// the free memory, and the streams take it in as many groups as that needs.  A segment that finds the pool empty
// gives its stream to the serial kernel.
static int32_t plan_inflate(spng_ctx *c, InflatePlan &p)
{
    p.internal = p.state.empty();
    if (p.internal) p.state.assign(p.jobs.size() * 4, 0);
    for (auto &j : p.jobs) j.internal = p.internal ? 1 : 0;
    p.parallel = c->cfg[SPNG_CFG_INFLATE_MODE] != SPNG_INFLATE_SERIAL && !p.jobs.empty();
    for (auto &j : p.jobs) p.gzip = p.gzip || j.format == SPNG_FORMAT_GZIP;
    if (!p.parallel) return SPNG_DONE;
    uint64_t total = 0;
    for (auto &j : p.jobs) total += j.src_len;
    if (int32_t st = learn_from_last_batch(c, total)) return st;
    if (int32_t st = cut_into_segments(c, p, inflate_segment_bytes((uint64_t)c->cfg[SPNG_CFG_SEGMENT_BYTES], total, c->block_bytes))) return st;
    if (int32_t st = size_token_pool(c, p)) return st;
    if (!p.parallel) return SPNG_DONE;
    group_streams(c, p);
    if (int32_t st = plan_parts(c, p)) return st;
    // what the next batch will learn from: this one's pool and source bytes, and where its counters come back to
    c->pool_pages_planned = p.pool_pages;
    c->pool_src_bytes = total;
    if (!c->h_pool_used) {
        HIP_TRY(hipHostMalloc((void **)&c->h_pool_used, 64, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&c->pool_ev, hipEventDisableTiming));
    }
    return SPNG_DONE;
}

static void stage_inflate(InflatePlan &p, Arena &a)
{
    const size_t n = p.jobs.size();
    p.jobs_at = a.take(n * sizeof(InflateJob));
    if (!p.state.empty()) {
        p.state_at = a.take(n * 32);
        memcpy(a.host<uint64_t>(p.state_at), p.state.data(), n * 32);
        for (size_t i = 0; i < n; ++i) {
            p.jobs[i].state = a.dev<uint64_t>(p.state_at) + 4 * i;
            if (p.parallel) p.streams[i].state = p.jobs[i].state;
        }
    }
    if (p.parallel) {
        p.streams_at = a.take(n * sizeof(PStream));
        p.segs_at = a.take(p.segs.size() * sizeof(PSeg));
        memcpy(a.host<PStream>(p.streams_at), p.streams.data(), n * sizeof(PStream));
        memcpy(a.host<PSeg>(p.segs_at), p.segs.data(), p.segs.size() * sizeof(PSeg));
    }
    if (p.parallel) {
        p.next_at = a.take(64);
        memset(a.host<uint32_t>(p.next_at), 0, 64);
        if (p.pmax) {
            p.parts_at = a.take(n * p.pmax * sizeof(PPart));
            memset(a.host<PPart>(p.parts_at), 0, n * p.pmax * sizeof(PPart));
        }
    }
    if (p.parallel || p.gzip) {
        p.done_at = a.take(n * 4);
        memset(a.host<int32_t>(p.done_at), 0, n * 4);
        for (size_t i = 0; i < n; ++i) p.jobs[i].skip = a.dev<int32_t>(p.done_at) + i;
    }
    memcpy(a.host<InflateJob>(p.jobs_at), p.jobs.data(), n * sizeof(InflateJob));
}

// SPNG_TRACE_PINFLATE -- diagnostic: how far every stream got in the pipeline (synchronises; never on by default)
static int32_t trace_inflate_plan(spng_ctx *c, const InflatePlan &p, Arena &a)
{
    const uint32_t n = (uint32_t)p.jobs.size();
    std::vector<PStream> hs(n);
    std::vector<PSeg> hg(p.segs.size());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(hs.data(), a.dev<PStream>(p.streams_at), n * sizeof(PStream), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hg.data(), a.dev<PSeg>(p.segs_at), hg.size() * sizeof(PSeg), hipMemcpyDeviceToHost));
    {
        // anomalies over the whole batch: segments without a start, segments that did not end on the next one
        uint64_t nostart = 0, fail = 0, skipped = 0; uint32_t shown = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const PStream &st = hs[i];
            for (uint32_t k = 0; k < st.seg_count; ++k) {
                const PSeg &sg = hg[st.seg_first + k];
                const bool a = sg.start_bit == ~0ull, b = !a && sg.status != PSEG_CONT && sg.status != PSEG_FINAL, cskip = !a && !b && sg.status == PSEG_CONT && sg.next != k + 1;
                nostart += a; fail += b; skipped += cskip;
                if ((a || b || cskip) && shown < 12) {
                    ++shown;
                    fprintf(stderr, "[pinflate] anomaly: stream %u seg %u/%u start %lld end %lld status %d next %u ntok %llu\n", i, k, st.seg_count,
                            (long long)sg.start_bit, (long long)sg.end_bit, sg.status, sg.next, (unsigned long long)sg.ntok);
                }
            }
        }
        fprintf(stderr, "[pinflate] %u streams, %zu segments in %zu groups, pool %u pages: %llu without a start, %llu failed, %llu ran past the next start\n", n,
                hg.size(), p.groups.size(), p.pool_pages, (unsigned long long)nostart, (unsigned long long)fail, (unsigned long long)skipped);
    }
    for (uint32_t i = 0; i < n && i < 4; ++i) {
        const PStream &st = hs[i];
        // (parts: how many the chain was cut into, of the slots plan_parts gave the stream -- 0 of 0: one workgroup)
        fprintf(stderr, "[pinflate] stream %u: len %llu segs %u seg_bytes %llu ok %d pass %u ntok %llu end_bit %llu parts %u of %u\n", i,
                (unsigned long long)st.src_len, st.seg_count, (unsigned long long)st.seg_bytes, st.ok, st.pass,
                (unsigned long long)st.ntok, (unsigned long long)st.end_bit, st.parts, st.parts_max);
        for (uint32_t k = 0; k < st.seg_count && k < 12; ++k) {
            const PSeg &sg = hg[st.seg_first + k];
            fprintf(stderr, "   seg %u: start %lld end %lld status %d used %u ntok %llu tok_base %llu next %u", k,
                    (long long)sg.start_bit, (long long)sg.end_bit, sg.status, sg.used, (unsigned long long)sg.ntok,
                    (unsigned long long)sg.tok_base, sg.next);
            if (sg.head) fprintf(stderr, " head %u", sg.head);
            fprintf(stderr, "\n");
        }
    }
    return SPNG_DONE;
}

static int32_t launch_inflate_plan(spng_ctx *c, InflatePlan &p, Arena &a, spng_result *dr)
{
    const uint32_t n = (uint32_t)p.jobs.size();
    if (p.gzip)   // (slots behind the uploaded part of the arena: the header kernel fills them)
        HIP_TRY(launch_gzip_pre(a.dev<InflateJob>(p.jobs_at), p.parallel ? a.dev<PStream>(p.streams_at) : nullptr, dr,
                                a.dev<uint64_t>(p.gz_at), a.dev<int32_t>(p.done_at), n, c->stream));
    if (p.parallel) {
        Timed whole(c, SPNG_K_PINFLATE);
        PStream *ds = a.dev<PStream>(p.streams_at);
        PSeg *dg = a.dev<PSeg>(p.segs_at);
        int32_t *dd = a.dev<int32_t>(p.done_at);
        uint32_t *dnext = a.dev<uint32_t>(p.next_at);      // {page counter, blocks} of the pass; dnext[8 ..] = the batch's totals
        uint32_t *dlog = (uint32_t *)c->d_log;
        uint8_t *pool = (uint8_t *)c->d_tok;
        const uint32_t pages = p.pool_pages;
        const hipStream_t q = c->stream;
        // every group of streams in turn, each with the whole pool, then once more those whose segments found the pool empty
        // (a batch unlike the one the pool was sized by): they get a second pass instead of the serial kernel
        c->cut_stats_valid = false;
        for (size_t gi = 0; gi <= p.groups.size(); ++gi) {
            const bool retry = gi == p.groups.size();
            const InflatePlan::Group g = retry ? InflatePlan::Group{0, n, 0, (uint32_t)p.segs.size()} : p.groups[gi];
            if (gi) HIP_TRY(hipMemsetAsync(dnext, 0, 4, q));
            { Timed t(c, SPNG_K_PINF_FIND, q); HIP_TRY(launch_pinf2_find(ds, dg, g.g0, g.g1 - g.g0, retry, q)); }
            // block cuts: only a group with a stream they may be tried for takes the kernels that know them (the plan in front of
            // the decode, the join behind it, their instantiations of decode and scan); dnext[12 ..] = {tried, joined, streams redone}
            bool cuts = false;
            if (!retry) for (uint32_t i = g.s0; i < g.s1 && !cuts; ++i) cuts = p.streams[i].cut_segs != 0;
            PCut *dc = p.cuts ? a.dev<PCut>(p.cuts_at) : nullptr;
            if (cuts) {
                c->cut_stats_valid = true;
                Timed t(c, SPNG_K_PINF_DECODE, q);
                HIP_TRY(hipMemsetAsync(dc + g.g0, 0, (size_t)(g.g1 - g.g0) * sizeof(PCut), q));
                HIP_TRY(launch_pinf2_cutplan(ds + g.s0, g.s1 - g.s0, dg, dc, dnext + 12, q));
                HIP_TRY(launch_pinf2_cutdecode(ds, dg, dc, g.g0, g.g1 - g.g0, dlog, pool, dnext, pages, q));
                HIP_TRY(launch_pinf2_cutjoin(ds, dg, dc, g.g0, g.g1 - g.g0, dlog, pool, dnext, pages, dnext + 12, q));
            } else
            { Timed t(c, SPNG_K_PINF_DECODE, q); HIP_TRY(launch_pinf2_decode(ds, dg, g.g0, g.g1 - g.g0, dlog, pool, dnext, pages, retry, q)); }
            PPart *dparts = p.pmax ? a.dev<PPart>(p.parts_at) + (size_t)g.s0 * p.pmax : nullptr;
            const uint32_t pm = retry ? 0u : p.pmax;                 // (the retry pass: one workgroup per stream)
            if (cuts) HIP_TRY(launch_pinf2_cutscan(ds + g.s0, g.s1 - g.s0, dg, dc, dparts, dnext + 12, q));
            else HIP_TRY(launch_pinf2_scan(ds + g.s0, g.s1 - g.s0, dg, dparts, retry, q));
            {
                Timed t(c, SPNG_K_PINF_RESOLVE, q);
                if (pm) {
                    // (the parts behind the first on the second stream, beside the first parts: 79 KB -- 93 KB when they have a CU each -- and 61 KB of LDS share a CU)
                    if (int32_t st = second_stream(c)) return st;
                    HIP_TRY(hipEventRecord(c->ev_fork, q));
                    HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
                    HIP_TRY(launch_pinf2_parts(ds + g.s0, g.s1 - g.s0, dg, dlog, pool, pages, dr, dd + g.s0, dparts, pm, (uint16_t *)c->d_sym, c->stream2));
                }
                HIP_TRY(launch_pinf2_resolve(ds + g.s0, g.s1 - g.s0, dg, dlog, pool, pages, dr, dd + g.s0, dparts, pm, retry, q));
                if (pm) {
                    HIP_TRY(hipEventRecord(c->ev_join, c->stream2));
                    HIP_TRY(hipStreamWaitEvent(q, c->ev_join, 0));
                    HIP_TRY(launch_pinf2_join(ds + g.s0, g.s1 - g.s0, dr, dd + g.s0, dparts, pm, (uint16_t *)c->d_sym,
                                              (uint8_t *)c->d_win + (size_t)g.s0 * pm * 32768, q));
                }
            }
            HIP_TRY(launch_pinf2_account(dnext, dnext + 8, pages, q));
        }
        if (c->cut_stats_valid) HIP_TRY(hipMemcpyAsync(c->h_pool_used + 8, dnext + 12, 12, hipMemcpyDeviceToHost, c->stream));
        if (!c->pool_pending) {
            // pages this batch took: read at the start of the next one (never waited for)
            HIP_TRY(hipMemcpyAsync(c->h_pool_used, dnext + 8, 16, hipMemcpyDeviceToHost, c->stream));
            c->pool_src_pending = c->pool_src_bytes;
            HIP_TRY(hipEventRecord(c->pool_ev, c->stream));
            c->pool_pending = true;
        }
    }
    if (p.parallel && getenv("SPNG_TRACE_PINFLATE"))
        if (int32_t st = trace_inflate_plan(c, p, a)) return st;
    {
        Timed t(c, SPNG_K_INFLATE);
        HIP_TRY(launch_inflate(a.dev<InflateJob>(p.jobs_at), n, dr, c->stream));
    }
    if (p.gzip)
        HIP_TRY(launch_gzip_inflate_post(a.dev<InflateJob>(p.jobs_at), dr, a.dev<uint64_t>(p.gz_at), a.dev<uint32_t>(p.gzparts_at), n,
                                         c->stream));
    if (!p.state.empty())   // the zlib checksum of a stream that finished in this call, over all of its bytes
        HIP_TRY(launch_resume_post(a.dev<InflateJob>(p.jobs_at), dr, a.dev<uint64_t>(p.sumparts_at), n, c->stream));
    return SPNG_DONE;
}

static const uint64_t *rows_len_in_results(void *user, uint32_t i)
{
    return &((spng_result *)user)[i].written;
}
static const uint64_t *rows_len_in_array(void *user, uint32_t i)
{
    return user ? (const uint64_t *)user + i : nullptr;
}

}  // namespace spng

extern "C" {

static int32_t inflate_batch(spng_ctx *c, const spng_stream_desc *descs, const uint64_t *h_state, bool resume, uint32_t count,
                             spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || (!d_results && !h_results && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    InflatePlan plan;
    plan.jobs.resize(count);
    if (resume) plan.state.assign((size_t)count * 4, 0);
    for (uint32_t i = 0; i < count; ++i) {
        if ((!descs[i].d_src && descs[i].src_len) || (!descs[i].d_dst && descs[i].dst_cap) || descs[i].format < SPNG_FORMAT_ZLIB ||
            descs[i].format > SPNG_FORMAT_GZIP) return SPNG_E_ARGUMENT;
        plan.jobs[i] = InflateJob{(const uint8_t *)descs[i].d_src, (uint8_t *)descs[i].d_dst,
                                  descs[i].src_len, descs[i].dst_cap, descs[i].format, i, nullptr, nullptr, 0, 0};
        if (resume && h_state) {
            const uint64_t *hs = h_state + 4 * (size_t)i;
            for (int k = 0; k < 4; ++k) plan.state[4 * (size_t)i + k] = hs[k];
            // (a state is only ever what an earlier call handed out: inside the input and the output, the token behind its block's
            // header, its bytes behind the block's)
            if (hs[0] > descs[i].src_len * 8 || hs[1] > descs[i].dst_cap || hs[2] > descs[i].src_len * 8 || hs[3] > descs[i].dst_cap ||
                (hs[2] && (hs[2] <= hs[0] || hs[3] < hs[1])) || (!hs[2] && hs[3])) return SPNG_E_ARGUMENT;
        }
    }
    if (int32_t st = plan_inflate(c, plan)) return st;
    if (int32_t st = c->reserve(plan.bytes() + count * sizeof(spng_result) + 1024)) return st;
    Arena a{c};
    stage_inflate(plan, a);
    const size_t upload = a.off;
    const size_t res = a.take(count * sizeof(spng_result));
    if (plan.gzip) { plan.gz_at = a.take(count * 8); plan.gzparts_at = a.take((size_t)count * 4 * gzip_pieces()); }
    plan.sumparts_at = a.take((size_t)count * 8 * gzip_pieces());
    plan.take_cuts(a);
    if (int32_t st = c->upload(0, upload)) return st;
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(res);
    poison_results_kernel<<<(count + 255) / 256, 256, 0, c->stream>>>(dr, count);
    HIP_TRY(hipGetLastError());
    if (int32_t st = launch_inflate_plan(c, plan, a, dr)) return st;
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

int32_t spng_inflate_batch(spng_ctx *c, const spng_stream_desc *descs, uint32_t count,
                           spng_result *d_results, spng_result *h_results)
{
    return inflate_batch(c, descs, nullptr, false, count, d_results, h_results);
}

int32_t spng_inflate_resume_batch(spng_ctx *c, const spng_stream_desc *descs, const uint64_t *h_state, uint32_t count,
                                  spng_result *d_results, spng_result *h_results)
{
    return inflate_batch(c, descs, h_state, true, count, d_results, h_results);
}

int32_t spng_unfilter_batch(spng_ctx *c, const spng_image_desc *descs, uint32_t count,
                            const uint64_t *d_rows_len,
                            spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    UnfilterPlan plan;
    if (int32_t st = plan_unfilter(descs, count, plan, rows_len_in_array, (void *)d_rows_len)) return st;
    const size_t need = plan_bytes(plan) + count * (sizeof(spng_result) + 16) + 1024;
    if (int32_t st = c->reserve(need)) return st;
    Arena a{c};
    PlanSlots slots;
    stage_plan(plan, a, slots);
    const size_t expected = a.take(count * 8);
    for (uint32_t i = 0; i < count; ++i)
        a.host<uint64_t>(expected)[i] = spng_inflated_size(descs[i].width, descs[i].height, descs[i].depth,
                                                           descs[i].channels, descs[i].interlaced);
    const size_t upload = a.off;
    const size_t res = a.take(count * sizeof(spng_result));
    if (int32_t st = c->upload(0, upload)) return st;
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(res);
    // results: status DONE, written = rows_len (or U); then extraneous check
    init_results_kernel<<<(count + 255) / 256, 256, 0, c->stream>>>(
        dr, d_rows_len ? d_rows_len : a.dev<uint64_t>(expected), count);
    HIP_TRY(hipGetLastError());
    if (int32_t st = launch_plan(c, plan, a, slots, nullptr)) return st;
    finish_decode_kernel<<<(count + 255) / 256, 256, 0, c->stream>>>(dr, a.dev<uint64_t>(expected), count);
    HIP_TRY(hipGetLastError());
    return read_back(c, h_results, dr, count * sizeof(spng_result));
}

int32_t spng_unfilter_resume_batch(spng_ctx *c, const spng_image_desc *descs, void *const *d_work, const uint64_t *h_prev_len,
                                   const uint64_t *h_now_len, uint32_t count, spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count) || !h_prev_len || !h_now_len) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    UnfilterPlan plan;
    std::vector<spng_result> res(count);
    for (uint32_t i = 0; i < count; ++i) {
        const spng_image_desc &d = descs[i];
        if (!valid_format(d.depth, d.channels) || !d.d_rows || !d.d_storage || h_prev_len[i] > h_now_len[i] ||
            (d.reserved & ~(uint32_t)SPNG_IMAGE_OVERDRAW)) return SPNG_E_ARGUMENT;   // (unknown flag bits: an uninitialised desc)
        const int volume = d.depth * d.channels;
        const uint32_t bpp = (uint32_t)(volume + 7) >> 3;
        const uint64_t u = spng_inflated_size(d.width, d.height, d.depth, d.channels, d.interlaced);
        if (d.rows_cap < u) return SPNG_E_ARGUMENT;
        const bool direct = !d.interlaced && volume >= 8;       // rows land in storage as they are
        if (!direct && (!d_work || !d_work[i])) return SPNG_E_ARGUMENT;
        Pass p[7];
        const int np = passes(d.width, d.height, volume, d.interlaced, p);
        uint64_t off = 0, fresh = 0, upto = 0;
        OverdrawJob ov;
        memset(&ov, 0, sizeof ov);
        ov.y0 = d.height; ov.y1 = 0;
        for (int z = 0; z < np; ++z) {
            const uint64_t stride = p[z].pitch + 1, end = off + stride * p[z].h;
            // rows of this sub-image complete before / with this push (PNG.Decoder.row / pass, PNG.Decoder.swift:20-21, 88-94)
            const uint64_t r0 = h_prev_len[i] <= off ? 0 : (h_prev_len[i] >= end ? p[z].h : (h_prev_len[i] - off) / stride);
            const uint64_t r1 = h_now_len[i] <= off ? 0 : (h_now_len[i] >= end ? p[z].h : (h_now_len[i] - off) / stride);
            upto = off + r1 * stride > upto && r1 ? off + r1 * stride : upto;
            if (r1 > r0) {
                UnfJob j;
                j.in = (const uint8_t *)d.d_rows + off + r0 * stride;
                j.in_stride = stride;
                if (direct) { j.out = (uint8_t *)d.d_storage + r0 * p[z].pitch; j.out_stride = p[z].pitch; }
                else        { j.out = (uint8_t *)d_work[i] + off + r0 * stride + 1; j.out_stride = stride; }
                j.stream_off = off; j.rows_len = nullptr;
                j.pitch = (uint32_t)p[z].pitch; j.rows = (uint32_t)(r1 - r0); j.image = i; j.bpp = bpp;
                j.has_prev = r0 ? 1 : 0; j.pad = 0;
                plan.unf[bpp].push_back(j);
                if (!direct) {
                    ScatterJob s;
                    s.rows = (const uint8_t *)d_work[i] + off + r0 * stride + 1;
                    s.storage = (uint8_t *)d.d_storage;
                    s.row_stride = stride; s.stream_off = off; s.rows_len = nullptr;
                    s.sub_w = p[z].w; s.sub_h = (uint32_t)(r1 - r0); s.width = d.width;
                    s.bx = p[z].bx; s.by = p[z].by + (uint32_t)r0 * p[z].sy; s.sx = p[z].sx; s.sy = p[z].sy;
                    s.depth = d.depth; s.channels = d.channels;
                    plan.scat.push_back(s);
                    plan.scat_image.push_back(i);
                }
                fresh += (r1 - r0) * stride;
            }
            if (d.interlaced && (d.reserved & SPNG_IMAGE_OVERDRAW)) {
                // (the pass index of PNG.adam7 from the pass's base; rows [first new scanline, last new scanline + its stride))
                const int q = p[z].sy == 8 ? (p[z].by ? 2 : p[z].bx ? 1 : 0) : p[z].sy == 4 ? (p[z].by ? 4 : 3) : (p[z].by ? 6 : 5);
                ov.done[q] = (uint32_t)r1;
                if (r1 > r0) {
                    const uint32_t a0 = p[z].by + (uint32_t)r0 * p[z].sy, a1 = p[z].by + (uint32_t)r1 * p[z].sy;
                    ov.y0 = a0 < ov.y0 ? a0 : ov.y0;
                    ov.y1 = a1 > ov.y1 ? a1 : ov.y1;
                }
            }
            off = end;
        }
        if (ov.y1 > ov.y0) {
            ov.storage = (uint8_t *)d.d_storage; ov.width = d.width; ov.height = d.height;
            ov.elem = volume < 8 ? 1u : (uint32_t)volume >> 3;
            if (ov.y1 > d.height) ov.y1 = d.height;
            plan.over.push_back(ov);
        }
        res[i].status = SPNG_DONE; res[i].reserved = 0;
        res[i].written = fresh;                                // scanline bytes defiltered by THIS call
        res[i].consumed = upto;                                // inflated bytes that are whole rows by now
        res[i].aux[0] = res[i].aux[1] = 0;
    }
    const size_t need = plan_bytes(plan) + count * sizeof(spng_result) + 1024;
    if (int32_t st = c->reserve(need)) return st;
    Arena a{c};
    PlanSlots slots;
    stage_plan(plan, a, slots);
    const size_t rslot = a.take(count * sizeof(spng_result));
    memcpy(a.host<spng_result>(rslot), res.data(), count * sizeof(spng_result));
    if (int32_t st = c->upload(0, a.off)) return st;
    if (int32_t st = launch_plan(c, plan, a, slots, nullptr)) return st;
    if (d_results) HIP_TRY(hipMemcpyAsync(d_results, a.dev<spng_result>(rslot), count * sizeof(spng_result), hipMemcpyDeviceToDevice, c->stream));
    if (h_results) {
        memcpy(h_results, res.data(), count * sizeof(spng_result));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return SPNG_DONE;
}

int32_t spng_decode_batch(spng_ctx *c, const spng_image_desc *descs, uint32_t count,
                          spng_result *d_results, spng_result *h_results)
{
    if (!c || (!descs && count)) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    HIP_TRY(hipSetDevice(c->device));
    std::lock_guard<std::mutex> g(c->mu);
    // results live on the device from the start: the unfilter jobs read `written` from them
    const size_t res_bytes = count * sizeof(spng_result);
    UnfilterPlan plan;
    InflatePlan ip;
    ip.jobs.resize(count);
    for (uint32_t i = 0; i < count; ++i) {
        const spng_image_desc &d = descs[i];
        if ((!d.d_idat && d.idat_len) || (d.format != SPNG_FORMAT_ZLIB && d.format != SPNG_FORMAT_IOS)) return SPNG_E_ARGUMENT;
        ip.jobs[i] = InflateJob{(const uint8_t *)d.d_idat, (uint8_t *)d.d_rows, d.idat_len, d.rows_cap, d.format, i, nullptr, nullptr, 0, 0};
    }
    if (int32_t st = plan_inflate(c, ip)) return st;
    // two-phase: we need the device address of the results before planning
    const size_t fixed = ip.bytes() + count * 8 + res_bytes + 2048;
    // conservative upper bound on plan size: 7 passes per image
    if (int32_t st = c->reserve(fixed + (size_t)count * 7 * (sizeof(UnfJob) + sizeof(ScatterJob) + 4) + 8192)) return st;
    Arena a{c};
    const size_t res = a.take(res_bytes);                      // first, so its device address is stable
    spng_result *dr = d_results ? d_results : a.dev<spng_result>(res);
    if (int32_t st = plan_unfilter(descs, count, plan, rows_len_in_results, (void *)dr)) return st;
    stage_inflate(ip, a);
    const size_t expected = a.take(count * 8);
    for (uint32_t i = 0; i < count; ++i) {
        const spng_image_desc &d = descs[i];
        a.host<uint64_t>(expected)[i] = spng_inflated_size(d.width, d.height, d.depth, d.channels, d.interlaced);
    }
    PlanSlots slots;
    stage_plan(plan, a, slots);
    // upload everything except the results region at the front
    const size_t first = (res_bytes + 255) & ~(size_t)255;
    const size_t staged = a.off;
    ip.sumparts_at = a.take((size_t)count * 8 * gzip_pieces());
    ip.take_cuts(a);
    if (int32_t st = c->upload(first, staged)) return st;
    poison_results_kernel<<<(count + 255) / 256, 256, 0, c->stream>>>(dr, count);
    HIP_TRY(hipGetLastError());
    if (int32_t st = launch_inflate_plan(c, ip, a, dr)) return st;
    if (int32_t st = launch_plan(c, plan, a, slots, dr)) return st;
    finish_decode_kernel<<<(count + 255) / 256, 256, 0, c->stream>>>(dr, a.dev<uint64_t>(expected), count);
    HIP_TRY(hipGetLastError());
    return read_back(c, h_results, dr, res_bytes);
}

// ---- host-pointer convenience wrappers ---------------------------------------------------------

int32_t spng_inflate(spng_ctx *c, const void *src, uint64_t n, int32_t format,
                     void *dst, uint64_t cap, spng_result *result)
{
    if (!c || (!src && n) || (!dst && cap) || !result) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf ds, dd;
    HIP_TRY(ds.alloc_from(src, n, c->stream)); HIP_TRY(dd.alloc(cap));
    spng_stream_desc d{ds.p, n, dd.p, cap, format, 0};
    if (int32_t st = spng_inflate_batch(c, &d, 1, nullptr, result)) return st;
    const uint64_t w = result->written < cap ? result->written : cap;
    HIP_TRY(dd.copy_to(dst, w));
    return SPNG_DONE;
}

int32_t spng_unfilter(spng_ctx *c, const void *rows, uint64_t rows_len,
                      uint32_t w, uint32_t h, int depth, int channels, int interlaced,
                      void *storage, spng_result *result)
{
    if (!c || (!rows && rows_len) || !storage || !result || !valid_format(depth, channels)) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t u = spng_inflated_size(w, h, depth, channels, interlaced);
    const uint64_t s = spng_storage_size(w, h, depth, channels);
    const uint64_t take = rows_len < u ? rows_len : u;
    DevBuf dr, dst, dl;
    HIP_TRY(dr.alloc(u));
    HIP_TRY(hipMemcpyAsync(dr.p, rows, take, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(dst.alloc_from(storage, s, c->stream));             // keep undecoded rows
    HIP_TRY(dl.alloc_from(&rows_len, 8, c->stream));
    spng_image_desc d{};
    d.d_rows = dr.p; d.rows_cap = u; d.d_storage = dst.p; d.width = w; d.height = h;
    d.depth = (uint8_t)depth; d.channels = (uint8_t)channels; d.interlaced = (uint8_t)(interlaced != 0);
    if (int32_t st = spng_unfilter_batch(c, &d, 1, (const uint64_t *)dl.p, nullptr, result)) return st;
    HIP_TRY(dst.copy_to(storage, s));
    return SPNG_DONE;
}

int32_t spng_decode(spng_ctx *c, const void *idat, uint64_t n, int32_t format,
                    uint32_t w, uint32_t h, int depth, int channels, int interlaced,
                    void *storage, spng_result *result)
{
    if (!c || (!idat && n) || !storage || !result || !valid_format(depth, channels)) return SPNG_E_ARGUMENT;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t u = spng_inflated_size(w, h, depth, channels, interlaced);
    const uint64_t s = spng_storage_size(w, h, depth, channels);
    DevBuf di, dr, dst;
    HIP_TRY(di.alloc_from(idat, n, c->stream)); HIP_TRY(dr.alloc(u + 4096)); HIP_TRY(dst.alloc_from(storage, s, c->stream));
    spng_image_desc d{};
    d.d_idat = di.p; d.idat_len = n; d.d_rows = dr.p; d.rows_cap = u + 4096; d.d_storage = dst.p;
    d.width = w; d.height = h; d.depth = (uint8_t)depth; d.channels = (uint8_t)channels;
    d.interlaced = (uint8_t)(interlaced != 0); d.format = (uint8_t)format;
    if (int32_t st = spng_decode_batch(c, &d, 1, nullptr, result)) return st;
    HIP_TRY(dst.copy_to(storage, s));
    return SPNG_DONE;
}

// spng_decode_batch over several devices: contiguous blocks of ceil(count / n_ctx) images per context,
// no communication while decoding; then, where d_gather names a destination on the FIRST context's device, every raster of the
// other contexts leaves for it as a peer-to-peer copy behind its context's decode (xGMI: one link per peer, all at once).
int32_t spng_decode_batch_multi(spng_ctx *const *ctxs, uint32_t n_ctx, const spng_image_desc *descs, uint32_t count, void *const *d_gather,
                                spng_result *h_results)
{
    if (!ctxs || !n_ctx || (!descs && count) || !h_results) return SPNG_E_ARGUMENT;
    for (uint32_t k = 0; k < n_ctx; ++k) if (!ctxs[k]) return SPNG_E_ARGUMENT;
    if (!count) return SPNG_DONE;
    // (the caller's current device is the caller's: put back on every way out -- ADVICE r4)
    struct Restore { int dev = -1; Restore() { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
                     ~Restore() { if (dev >= 0) (void)hipSetDevice(dev); } } restore;
    spng_ctx *root = ctxs[0];
    // Every context's shard is enqueued -- asynchronous calls, results stay on the devices -- in SPNG_CFG_MULTI_GROUPS groups
    // (2 by default when rasters leave for another device): a group's rasters leave on the context's second stream behind an
    // event, while the next group decodes on the first.
    int32_t status = SPNG_DONE;
    std::vector<uint32_t> sent(n_ctx, 0);
    for (uint32_t k = 0; k < n_ctx && status == SPNG_DONE; ++k) {
        uint32_t first = 0, n = 0;
        (void)spng_shard(count, n_ctx, k, &first, &n);
        if (!n) continue;
        spng_ctx *c = ctxs[k];
        if (hipError_t e = hipSetDevice(c->device); e != hipSuccess) { status = fail_hip(e, "hipSetDevice"); break; }
        bool leaves = false;                                   // any raster of this shard wanted on another device?
        if (d_gather)
            for (uint32_t i = first; i < first + n && !leaves; ++i) leaves = d_gather[i] && d_gather[i] != descs[i].d_storage;
        uint32_t groups = 1;
        {
            std::lock_guard<std::mutex> g(c->mu);
            const size_t need = (size_t)n * sizeof(spng_result);
            if ((status = c->grow(c->d_multi, c->multi_cap, need, need / 2)) != SPNG_DONE) break;
            if (leaves) {
                if (!c->stream_out) {
                    if (hipError_t e = hipStreamCreateWithFlags(&c->stream_out, hipStreamNonBlocking); e != hipSuccess) { status = fail_hip(e, "hipStreamCreateWithFlags"); break; }
                    for (hipEvent_t &ev : c->ev_out)
                        if (hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); e != hipSuccess) { status = fail_hip(e, "hipEventCreateWithFlags"); break; }
                    if (status != SPNG_DONE) break;
                }
                // peer access, once per pair of devices: with it the copies ride xGMI directly; without it the runtime stages them
                // through the host -- slower, not wrong, and said so in spng_last_error_string
                const int rd = root->device;
                if (c->device != rd && rd < 64 && !((c->peers | c->peers_refused) >> rd & 1)) {
                    int can = 0;
                    if (hipDeviceCanAccessPeer(&can, c->device, rd) != hipSuccess) { can = 0; (void)hipGetLastError(); }
                    hipError_t e = can ? hipDeviceEnablePeerAccess(rd, 0) : hipErrorPeerAccessUnsupported;
                    if (e == hipErrorPeerAccessAlreadyEnabled) { e = hipSuccess; (void)hipGetLastError(); }
                    if (e == hipSuccess) c->peers |= 1ull << rd;
                    else {
                        (void)hipGetLastError();
                        c->peers_refused |= 1ull << rd;
                        snprintf(g_err, sizeof g_err, "spng_decode_batch_multi: no peer access from device %d to device %d (%s): copies are staged",
                                 c->device, rd, hipGetErrorString(e));
                    }
                }
                const int64_t want = c->cfg[SPNG_CFG_MULTI_GROUPS];
                groups = want > 0 ? (uint32_t)want : 2u;
                if (groups > n) groups = n;
                if (groups > 2) groups = 2;                    // (two events per context; more groups cost more than they hide)
            }
        }
        spng_result *d_res = (spng_result *)c->d_multi;
        for (uint32_t g = 0; g < groups && status == SPNG_DONE; ++g) {
            const uint32_t g0 = (uint32_t)((uint64_t)n * g / groups), g1 = (uint32_t)((uint64_t)n * (g + 1) / groups);
            status = spng_decode_batch(c, descs + first + g0, g1 - g0, d_res + g0, nullptr);
            if (status != SPNG_DONE || !leaves) continue;
            sent[k] = 1;                                       // (before the first copy is enqueued: a failure half way still waits for stream_out below)
            if (hipError_t e = hipEventRecord(c->ev_out[g & 1], c->stream); e != hipSuccess) { status = fail_hip(e, "hipEventRecord"); break; }
            if (hipError_t e = hipStreamWaitEvent(c->stream_out, c->ev_out[g & 1], 0); e != hipSuccess) { status = fail_hip(e, "hipStreamWaitEvent"); break; }
            for (uint32_t i = first + g0; i < first + g1; ++i) {
                if (!d_gather[i] || d_gather[i] == descs[i].d_storage) continue;
                const uint64_t s = spng_storage_size(descs[i].width, descs[i].height, descs[i].depth, descs[i].channels);
                const hipError_t e = hipMemcpyPeerAsync(d_gather[i], root->device, descs[i].d_storage, c->device, s, c->stream_out);
                if (e != hipSuccess) { status = fail_hip(e, "hipMemcpyPeerAsync"); break; }
            }
        }
    }
    // wait for everything that was enqueued (also on the way out of a failure), results to the host
    for (uint32_t k = 0; k < n_ctx; ++k) {
        uint32_t first = 0, n = 0;
        (void)spng_shard(count, n_ctx, k, &first, &n);
        if (!n) continue;
        spng_ctx *c = ctxs[k];
        (void)hipSetDevice(c->device);
        if (status == SPNG_DONE && c->d_multi) {
            const hipError_t e = hipMemcpyAsync(h_results + first, c->d_multi, (size_t)n * sizeof(spng_result), hipMemcpyDeviceToHost, c->stream);
            if (e != hipSuccess) status = fail_hip(e, "hipMemcpyAsync");
        }
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess && status == SPNG_DONE) status = fail_hip(e, "hipStreamSynchronize");
        if (sent[k] && c->stream_out) {
            e = hipStreamSynchronize(c->stream_out);
            if (e != hipSuccess && status == SPNG_DONE) status = fail_hip(e, "hipStreamSynchronize");
        }
    }
    return status;
}

}  // extern "C"