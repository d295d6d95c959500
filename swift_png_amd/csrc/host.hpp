// host.hpp -- what the host-side sources of libspng_mi355.so share (api.hip and the host_*.hip of the stages): error text, the
// context with its workspaces, the arena over them, launch timing, and a device buffer for the host-pointer forms of the entries.
#pragma once
#include "common.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <functional>
#include <mutex>
#include <vector>

namespace spng {

extern thread_local char g_err[512];                           // spng_last_error_string (api.hip)

static int32_t fail_hip(hipError_t e, const char *what)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return SPNG_E_DEVICE;
}
static int32_t fail_text(const char *what)
{
    snprintf(g_err, sizeof g_err, "%s", what);
    return SPNG_E_DEVICE;
}
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail_hip(e_, #expr); } while (0)

static bool valid_format(int depth, int channels)
{
    if (channels < 1 || channels > 4) return false;
    if (depth == 8 || depth == 16) return true;
    return channels == 1 && (depth == 1 || depth == 2 || depth == 4);
}

__global__ void init_results_kernel(spng_result *results, const uint64_t *written, uint32_t count);   // (host_decode.hip)

}  // namespace spng

using namespace spng;

struct spng_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    // device + pinned workspaces for job tables
    void *d_ws = nullptr;  size_t d_ws_cap = 0;
    // Pinned staging for the job tables.  An entry point fills a slab on the host, enqueues its
    // upload and may return before the copy engine has read it (h_results == NULL), so the next
    // call must not scribble over the same pinned bytes: slabs are used round-robin and each is
    // guarded by an event recorded behind its upload.  (The device copy d_ws needs no such care: the
    // next upload is ordered behind the kernels that read the previous tables by the stream itself.)
    static constexpr int SLABS = 4;
    struct Slab { void *h = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; };
    Slab slabs[SLABS];
    int slab_next = 0;
    void *h_ws = nullptr;                 // the slab of the call in progress
    Slab *cur = nullptr;
    // parallel inflate (pinflate2.hip): chunk-record slab, token buffer, knobs (spng_configure)
    void *d_graph = nullptr; size_t graph_cap = 0;   // deflate: the search's records and pools, the parse's vertex arrays
    void *d_log = nullptr;  size_t log_cap = 0;
    void *d_tok = nullptr;  size_t tok_cap = 0;      // bytes
    void *d_sym = nullptr;  size_t sym_cap = 0;      // several workgroups per stream: 16-bit symbols, windows (bytes)
    uint64_t sym_failed = 0;                        // a symbol scratch of this size could not be had (forgotten by spng_trim)
    void *d_win = nullptr;  size_t win_cap = 0;
    void *d_census = nullptr; size_t census_cap = 0; // spng_census_batch: the images' hash tables and sort buffers
    void *d_file = nullptr;  size_t file_cap = 0;    // spng_compress_batch: the encoder's results, which the writer reads on the device
    // token pool of the pipeline (pinflate2.hip): halfwords a compressed byte turned into in the last batch (learned,
    // so that the next batch of the same kind takes one pass), and the pinned word the page counter is read back into
    double   pool_ratio = 0;
    uint32_t *h_pool_used = nullptr;                 // ([8 .. 10]: block cuts tried, joined, streams redone of the last call that could try any)
    bool cut_stats_valid = false;                    // (the last parallel-inflate call could)
    uint64_t pool_pages_planned = 0, pool_src_bytes = 0, pool_src_pending = 0;   // (source bytes of the batch planned / of the one whose counters are on their way)
    double   block_bytes = 0;        // compressed bytes per DEFLATE block in the last batch (0: not known)
    hipEvent_t pool_ev = nullptr; bool pool_pending = false;
    uint64_t *h_lex_stats = nullptr;                 // pinned: {bytes summed, IDAT bytes copied, headers walked} of the last spng_lex_resume_batch
    hipEvent_t ev_dfl[4] = {nullptr, nullptr, nullptr, nullptr};    // level >= 8 rounds: searched[parity], parsed[parity]
    // second stream (second_stream()): the parts of a stream's resolve beside its first, a deflate round's search beside the parse
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // spng_decode_batch_multi: the stream a context's rasters leave on (so that a group's copies run beside the next group's
    // decode), the events between the two, its part of the results, the peers it has been given access to
    hipStream_t stream_out = nullptr;
    hipEvent_t ev_out[2] = {nullptr, nullptr};
    void *d_multi = nullptr; size_t multi_cap = 0;
    uint64_t peers = 0, peers_refused = 0;
    int64_t cfg[SPNG_CFG_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // profiling
    bool profiling = false;
    struct Span { int kernel; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> pool;
    std::mutex mu;

    // the buffers a batch sizes (spng_trim gives them back to the device; d_ws, the job tables', stays)
    struct Buf { void **p; size_t *cap; };
    std::array<Buf, 8> batch_buffers()
    {
        return {{{&d_graph, &graph_cap}, {&d_log, &log_cap}, {&d_tok, &tok_cap}, {&d_sym, &sym_cap}, {&d_win, &win_cap}, {&d_multi, &multi_cap},
                 {&d_census, &census_cap}, {&d_file, &file_cap}}};
    }
    // Makes a device buffer of the context hold `need` bytes.  Only when it has to grow: waits for the stream (kernels in
    // flight may still read the old one), frees it and allocates need + slack.  A failed allocation is an error -- or, `failed`
    // given, reported there: the sticky HIP error cleared, the pointer null, the capacity 0.
    int32_t grow(void *&buf, size_t &cap, size_t need, size_t slack, bool *failed = nullptr)
    {
        if (failed) *failed = false;
        if (need <= cap) return SPNG_DONE;
        HIP_TRY(hipStreamSynchronize(stream));
        if (buf) { HIP_TRY(hipFree(buf)); buf = nullptr; }
        cap = 0;
        const hipError_t e = hipMalloc(&buf, need + slack);
        if (e != hipSuccess) {
            buf = nullptr;
            if (!failed) return fail_hip(e, "hipMalloc");
            (void)hipGetLastError();
            *failed = true;
            return SPNG_DONE;
        }
        cap = need + slack;
        return SPNG_DONE;
    }
    // Starts a call: device table space for `bytes`, and a pinned slab nobody is reading any more.
    int32_t reserve(size_t bytes)
    {
        if (int32_t st = grow(d_ws, d_ws_cap, bytes, bytes / 2 + 4096)) return st;
        Slab &sl = slabs[slab_next];
        slab_next = (slab_next + 1) % SLABS;
        if (sl.pending) { HIP_TRY(hipEventSynchronize(sl.ev)); sl.pending = false; }
        if (bytes > sl.cap) {
            if (sl.h) { HIP_TRY(hipHostFree(sl.h)); sl.h = nullptr; sl.cap = 0; }
            const size_t cap = bytes + bytes / 2 + 4096;
            HIP_TRY(hipHostMalloc(&sl.h, cap, hipHostMallocDefault));
            sl.cap = cap;
        }
        if (!sl.ev) HIP_TRY(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
        cur = &sl; h_ws = sl.h;
        return SPNG_DONE;
    }
    // Enqueues the upload of slab bytes [from, to) to the same offsets of d_ws and marks the slab busy
    // until the copy has executed.
    int32_t upload(size_t from, size_t to)
    {
        if (to > from)
            HIP_TRY(hipMemcpyAsync((char *)d_ws + from, (char *)h_ws + from, to - from, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(cur->ev, stream));
        cur->pending = true;
        return SPNG_DONE;
    }
    hipEvent_t event()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};

// The second stream and the events that fork to it and join from it, on first use.
static int32_t second_stream(spng_ctx *c)
{
    if (c->stream2) return SPNG_DONE;
    HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    for (hipEvent_t *e : {&c->ev_fork, &c->ev_join}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return SPNG_DONE;
}

// The tail of a call that hands something back: `bytes` from the device to the host behind everything the call enqueued, and
// the wait for them.  No host pointer: nothing -- the call stays asynchronous.
static int32_t read_back(spng_ctx *c, void *h, const void *d, size_t bytes)
{
    if (!h) return SPNG_DONE;
    HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SPNG_DONE;
}

struct Timed {            // records a pair of events around a launch when profiling is on
    spng_ctx *c; int k; hipEvent_t a = nullptr; hipStream_t s;
    Timed(spng_ctx *c_, int k_, hipStream_t s_ = nullptr) : c(c_), k(k_), s(s_ ? s_ : c_->stream) { if (c->profiling) { a = c->event(); (void)hipEventRecord(a, s); } }
    ~Timed() { if (a) { hipEvent_t b = c->event(); (void)hipEventRecord(b, s); c->spans.push_back({k, a, b}); } }
};

// simple bump allocator over the paired pinned/device workspaces
struct Arena {
    spng_ctx *c; size_t off = 0;
    template <class T> T *host(size_t at) { return (T *)((char *)c->h_ws + at); }
    template <class T> T *dev(size_t at) { return (T *)((char *)c->d_ws + at); }
    size_t take(size_t bytes) { size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; }
};

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 16); }
    // alloc, and the n bytes at `host` copied in behind what the stream holds (n == 0: no copy)
    hipError_t alloc_from(const void *host, size_t n, hipStream_t stream)
    { const hipError_t e = alloc(n); return e != hipSuccess || !n ? e : hipMemcpyAsync(p, host, n, hipMemcpyHostToDevice, stream); }
    hipError_t copy_to(void *host, size_t n) const { return n ? hipMemcpy(host, p, n, hipMemcpyDeviceToHost) : hipSuccess; }
};
