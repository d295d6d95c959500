// common.hpp -- shared host/device declarations for libspng_mi355.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/spng_mi355.h"

namespace spng {

// ---- device-side vocabulary shared by every kernel file --------------------------------------------------------
// Wave-uniform values loaded through the vector path are pinned to scalar registers (the bit readers and
// symbol-boundary chains then run on the scalar unit).
#define UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)UNI(v >> 32) << 32 | UNI((uint32_t)v); }
// A wave-uniform condition, said so to the compiler: its divergence analysis is conservative at control-flow joins,
// and one branch it takes for lane-dependent turns every loop around it into exec-mask bookkeeping.
#define UB(c) (UNI((c) ? 1u : 0u) != 0u)
#ifndef SPNG_EMU
typedef uint8_t __attribute__((address_space(1))) gbyte;      // a byte in global memory (global_load, not flat_load)
#else
typedef uint8_t gbyte;
#endif

// A bound on the spin waits of the wave-to-wave protocols (unfilter bands, the search kernel's inserter and searchers): a
// protocol bug must fault, not hang the GPU -- but a wave held up from outside (a profiler serialising the kernel, a debugger)
// is not a bug, so the bound is wall time (s_memrealtime, 100 MHz), looked at every 4096 spins: 20 s.
struct SpinGuard {
    uint32_t spins = 0;
    uint64_t t0 = 0;
    __device__ __forceinline__ void tick()
    {
        if ((++spins & 0xfffu) != 0) return;
#ifndef SPNG_EMU
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (!t0) t0 = now;
        else if (now - t0 > 2000000000ull) __builtin_trap();
#else
        if (spins > (1u << 28)) __builtin_trap();
#endif
    }
};

// The epilogue of a kernel whose lanes counted what the reference would have trapped on: the counts of a wave are added to
// result->aux[0] by one atomic per wave, and only from waves that counted anything.  Every lane of the wave arrives here.
__device__ __forceinline__ void add_wave_count(spng_result *result, uint32_t n)
{
    if (__ballot(n != 0) == 0) return;
#pragma unroll
    for (int m = 32; m; m >>= 1) n += (uint32_t)__shfl_xor((int)n, m);
    if ((threadIdx.x & 63) == 0) atomicAdd((unsigned long long *)&result->aux[0], (unsigned long long)n);
}

// One unfilter job = one dependency chain of scanlines: a whole non-interlaced image or one
// Adam7 sub-image (PNG.Decoder.swift:59-140).  Rows are `in_stride` apart starting at `in`
// (which points at the first row's filter byte); defiltered bytes of row y go to
// out + y*out_stride.  For 8/16-bit non-interlaced images `out` is PNG.Image.storage itself;
// otherwise the rows are defiltered in place (out = in + 1) and a scatter kernel follows.
struct UnfJob {
    const uint8_t *in;
    uint8_t       *out;
    uint64_t       in_stride;     // pitch + 1
    uint64_t       out_stride;
    uint64_t       stream_off;    // offset of `in` inside the image's inflated stream
    const uint64_t *rows_len;     // device pointer to the number of valid inflated bytes, or null
    uint32_t       pitch;         // bytes per row without the filter byte
    uint32_t       rows;
    uint32_t       image;         // index into the result array
    uint32_t       bpp;           // "delay": ceil(volume / 8)
    uint32_t       has_prev;      // spng_unfilter_resume_batch: the defiltered row above row 0 is at out - out_stride
    uint32_t       pad;
};

// One scatter job: defiltered rows of one (sub-)image -> PNG.Image.storage (PNG.Image.assign,
// PNG.Image.swift:186-285), including MSB-first expansion of 1/2/4-bit samples.
struct ScatterJob {
    const uint8_t *rows;          // first row's first data byte
    uint8_t       *storage;
    uint64_t       row_stride;    // pitch + 1
    uint64_t       stream_off;
    const uint64_t *rows_len;
    uint32_t       sub_w, sub_h;  // sub-image size in pixels
    uint32_t       width;         // full image width
    uint32_t       bx, by, sx, sy;
    uint32_t       depth, channels;
};

// One image whose unfinished Adam7 cells are filled in for progressive display (PNG.Image.overdraw, PNG.Image.swift:134-183, as
// PNG.Context.push(data:overdraw: true) calls it after every scanline, PNG.Context.swift:88-102).
struct OverdrawJob {
    uint8_t *storage;
    uint32_t width, height;
    uint32_t elem;                // storage bytes per pixel (1, 2, 3, 4, 6, 8)
    uint32_t y0, y1;              // storage rows this call may have changed
    uint32_t done[7];             // scanlines of each Adam7 pass assigned so far
};

// One filter job (encode): storage -> filtered rows of one (sub-)image
// (PNG.Encoder.pull + PNG.Image.collect + PNG.Encoder.filter).
struct FilterJob {
    const uint8_t *storage;
    uint8_t       *rows;          // first row's filter byte
    uint64_t       row_stride;    // pitch + 1
    uint32_t       sub_w, sub_h;
    uint32_t       width;
    uint32_t       bx, by, sx, sy;
    uint32_t       depth, channels;
    uint32_t       pitch;
};

// One image to unpack: PNG.Image.storage -> RGBA<UInt8 / UInt16> (unpack.hip)
struct UnpackJob {
    const uint8_t *storage;
    void          *out;
    const uint8_t *palette;       // indexed formats: palette_count x (r, g, b, a)
    uint32_t       width, height;
    uint32_t       palette_count;
    uint16_t       key[3];        // tRNS chroma key, at the source depth
    uint8_t        depth, channels, indexed, bgr, has_key, pad;
    uint8_t        layout, premultiply;      // spng_unpack_desc.layout / .premultiply
};

// One image to pack: RGBA<T> / VA<T> / T pixels -> PNG.Image.storage (unpack.hip, pack_kernel)
struct PackJob {
    const void    *pixels;
    uint8_t       *storage;
    const uint8_t *palette;       // indexed formats: palette_count x (r, g, b, a)
    uint32_t       width, height;
    uint32_t       palette_count;
    uint8_t        depth, channels, indexed, bgr;
    uint8_t        layout, premultiply, pad[2];   // spng_pack_desc.layout / .premultiply
};

// One array of colour-target pixels to premultiply or straighten (alpha.hip, alpha_kernel)
struct AlphaJob {
    const void    *in;
    void          *out;           // == in: in place
    uint64_t       count;         // pixels
    spng_result   *result;        // filled in by the host; the kernel adds the trapped components to aux[0]
    uint8_t        layout, op, pad[6];       // spng_alpha_desc.layout / .op
};

// One array of pixels converted to or from the tutorial's HSVA colour target (hsva.hip, hsva_kernel)
struct HsvaJob {
    const void    *in;
    void          *out;
    uint64_t       count;         // pixels
    spng_result   *result;        // filled in by the host; the kernel adds the trapped pixels to aux[0]
    uint8_t        op, pad[7];    // spng_hsva_desc.op
};

// One array of RGBA<UInt8> pixels reduced to the luminance of the BasicEncoding tutorial (luminance.hip, luminance_kernel)
struct LuminanceJob {
    const void    *in;
    void          *out;
    uint64_t       count;         // pixels
    spng_result   *result;        // filled in by the host; the kernel leaves it alone (nothing traps)
    uint8_t        op, pad[7];    // spng_luminance_desc.op
};

// One array of colour-target pixels whose distinct keys are counted (indexing.hip, census_kernel + census_finish_kernel)
struct CensusJob {
    const void    *pixels;
    uint64_t       count;         // pixels
    uint32_t      *keys;          // out: the distinct keys, ascending
    uint64_t      *out_counts;    // out: their frequencies, or null
    unsigned long long *tags;     // context scratch, zeroed in front of the call: the image's hash table (slots tags, slots counts),
    unsigned long long *counts;
    uint32_t      *ctrl;          // ... {distinct keys claimed, overflow flag},
    unsigned long long *sort;     // ... and pow2(cap) elements for the sort (not zeroed)
    spng_result   *result;        // written by census_finish_kernel
    uint32_t       cap, slots, slot_bits;
    uint8_t        layout, premultiply, pad[2];
};

// One image to pack through a map from keys to indices (indexing.hip, pack_indexed_kernel)
struct PackIndexedJob {
    const void    *pixels;
    uint8_t       *storage;       // one byte per pixel
    const uint32_t *keys;         // map_count keys, ascending and distinct
    const uint8_t *indices;
    spng_result   *result;        // filled in by the host; the kernel adds the pixels that missed to aux[0]
    uint32_t       width, height;
    uint32_t       map_count;
    uint8_t        layout, premultiply, miss, pad;
};

// One array of pixels mapped through a table from keys to values of 1, 2, 4 or 8 bytes (colour_tables.hip, map_build_kernel + map_kernel)
struct MapJob {
    const void    *pixels;
    void          *out;           // one value per pixel
    const uint32_t *keys;         // map_count keys, ascending and distinct
    const void    *values;
    spng_result   *result;        // filled in by the host; the kernel adds the pixels that missed to aux[0]
    uint64_t       count;         // pixels
    uint64_t       miss;          // the value of a pixel whose key is not in the map (its low value_bytes bytes)
    uint64_t       table_off;     // slots != 0: where the map's hash table starts in the call's scratch, in slots
    uint32_t       map_count, slots, slot_bits;      // slots == 0: the table is built in LDS by every workgroup
    uint8_t        layout, premultiply, value_bytes, pad;
};

// One PNG file to write (chunks.hip, wfile_body_kernel + wfile_finish_kernel)
struct FileJob {
    const uint8_t *head;          // device copy of the bytes between the signature and the first IDAT (file_head.hpp)
    const uint8_t *stream;
    const spng_result *src_result;    // device: the stream's status and length (written), or null: len
    uint8_t       *out;
    uint32_t      *partial;       // chunks of several pieces: a raw CRC per unit of the file (null when chunk_bytes allows none)
    uint64_t       head_len, len, stream_cap, out_cap, chunk_bytes;
};

// One text to transcode or check (text.hip)
struct TextJob {
    const uint8_t *in;
    uint8_t       *out;
    uint64_t       len, out_cap;
    uint64_t       tiles;         // of TEXT_TILE bytes
    uint32_t      *counts;        // call scratch, per tile: bytes >= 0x80 / ill-formed sequences that begin in it,
    uint32_t      *firsts;        // ... the first of those in the tile (check only),
    uint64_t      *offs;          // ... where its output starts (transcode only)
    uint8_t        op, pad[7];    // spng_text_desc.op
};

struct InflateJob {
    const uint8_t *src;
    uint8_t       *dst;
    uint64_t       src_len;
    uint64_t       dst_cap;
    int32_t        format;
    uint32_t       image;
    const int32_t *skip;          // device flag: non-zero = the parallel pipeline already produced this stream
    // FOUR words: {first bit of the first block not decoded completely yet, inflated bytes in front of it, first bit INSIDE that block
    // that is still to decode (0: its header), inflated bytes in front of that}: the pipeline moves the first pair forward (and
    // clears the second), the serial kernel starts there.  spng_inflate_resume_batch: what the previous call returned; every other
    // call: the library's own slot, {0, 0} (`internal`), so that a stream the pipeline cannot finish -- truncated,
    // corrupt -- costs the serial kernel one block, not the whole stream.
    uint64_t      *state;
    uint32_t       internal, pad;
};

// ---- the parallel inflate pipeline (pinflate2.hip) -----------------------------------------------
// One stream of a batch.  The host fills the first group of fields, the kernels the second.
struct PStream {
    const uint8_t *src;
    uint8_t       *dst;
    uint64_t       src_len, dst_cap;
    int32_t        format;
    uint32_t       image;
    uint32_t       seg_first, seg_count;   // its segments in the PSeg table
    uint64_t       seg_bytes;              // nominal segment length (multiple of 256)
    // device side
    uint64_t       tok_base, ntok;         // its tokens in the token buffer (of its pass)
    uint64_t       end_bit;                // first bit after the final block
    int32_t        ok;                     // 1: the segment chain holds from the first bit to a final block; 2 (resumable
                                           // streams): up to the first block the input does not hold completely; 3 (resumed calls
                                           // with cuts): up to a token inside a block, the input ends within two segments of it
    uint32_t       pass;
    // resumable streams (spng_inflate_resume_batch): where to start, and where to note how far the chain got
    uint64_t       start_bit, out_pos;
    uint64_t      *state;
    uint32_t       serial_only, cut_segs;  // cut_segs (host): block cuts are tried for runs of at least so many segments without a start (0: never).  serial_only: the caller's state stands deep inside a huge block: the serial kernel goes on THERE (the pipeline would decode the block again)
    // several workgroups per stream: parts_max slots in the part table (0: one workgroup), how many the chain was cut into
    uint32_t       parts_max, parts;
    uint64_t       out_total;              // scan: bytes of the whole chain
    uint64_t       sym_off;                // its 16-bit symbols in the symbol scratch (in symbols)
    uint32_t       cut_on, cut_resumed;    // plan (device side): some of its segments are cut.  cut_resumed (host): a call of
                                           // spng_inflate_resume_batch with a state for which cuts may be tried ("resumed calls", pinflate2.hip)
    // resumed calls with cuts: segment 0 starts seg_origin bytes into the input (a multiple of 256; 0 in every other stream);
    // tok_bit != 0: the state stands INSIDE the block whose header is start_bit -- the first token still to decode, out_pos bytes
    // in the output, blk_out of them in front of the block (the plan or scan clear tok_bit, on the device, when the call falls back
    // to the block's header)
    uint64_t       seg_origin, tok_bit, blk_out;
    uint64_t       ho_hdr, ho_out;         // scan, ok == 3: the block the hand-over token (end_bit) lies in: its header, the bytes in front of it
};
enum { PSEG_FAIL = 0, PSEG_CONT = 1, PSEG_FINAL = 2, PSEG_PARTIAL = 3, PSEG_NOPAGE = 4,
       PSEG_CUT = 5 };                     // stopped INSIDE a block, in front of a cut segment (block cuts: pinflate2.hip)
static constexpr uint64_t RESUME_SERIAL_BITS = 8ull << 20;      // 1 MiB of input inside one block: a resumed call goes on there, not at its header
                                                                // (and the default of SPNG_CFG_BLOCK_CUT_BYTES)
static constexpr uint32_t PCUT_RECS = 4;   // chunk ends a cut segment's wave records of its chain's head
// One segment: the blocks that start in [index * seg_bytes, (index + 1) * seg_bytes).
struct PSeg {
    uint32_t stream, index;
    uint64_t log_off, log_cap;             // its page table in the slab (first entry, entries)
    // device side
    uint64_t start_bit;                    // find: first block header at or after the nominal start (~0: none)
    uint64_t end_bit;                      // count: where decoding stopped (start of the next block)
    uint64_t ntok;                         // decode: token halfwords
    uint64_t tok_base;                     // scan: first token, relative to the stream's
    int32_t  status;                       // count: PSEG_*
    uint32_t used;                         // scan: part of the chain
    uint32_t next, head;                   // count: index of the segment that starts where this one stopped; scan: token halfwords at
                                           // its front that are not on the chain (a multiple of 8; 0 in every segment that is not cut)
    uint64_t nbytes;                       // decode: bytes its tokens stand for
    uint64_t out_base;                     // scan: its first byte, counted from the stream's first byte of this call
};
// What block cuts (pinflate2.hip) keep per segment: a table beside the PSeg table, same index, device side only -- it exists, zeroed,
// only in a batch in which cuts may be tried, so that every other batch stages and uploads what it always did.
struct PCut {
    uint32_t cut, anchor;                  // plan: decoded from a guessed bit with the tables of the block at segment `anchor`'s start
    uint32_t nrec, joined;                 // decode: records below; join (PSEG_CUT): this segment's chain provably runs into segment `next`'s ...
    uint32_t next_head, tbl_here;          // ... behind that one's first next_head halfwords, which stand for next_sub bytes.  tbl_here (decode,
                                           // PSEG_CUT): the block end_bit lies in began in this segment, tbl_bytes of its bytes in front of it
    uint64_t tbl, tbl_id;                  // decode, PSEG_CUT: the header of the block end_bit lies in, and which tables that makes (table_id)
    uint64_t head_tbl;                     // decode, cut segments: the tables its records were decoded with
    uint64_t add_tok, add_bytes;           // join: bridge tokens it appended behind ntok on the way there, their bytes
    uint64_t next_sub;
    uint64_t tbl_bytes;
    uint64_t next_bit;                     // join: the bit at which the two chains are one (a token start: a record of segment `next`)
    uint64_t join_tbl, join_tbl_bytes;     // join: the bridge crossed into another block: its header (0: it did not), bridge bytes in front of it
    struct { uint64_t bit; uint32_t hw, bytes; } rec[PCUT_RECS];   // decode: a chunk end of its first block: the token start there,
                                                                   // halfwords (padded to 8) and bytes emitted in front of it
};
// A part of a stream's segment chain that one workgroup resolves (pinflate2.hip, "Several workgroups per stream").
struct PPart {
    uint32_t seg, seg_end;                 // first chain segment (index in the stream), the next part's (~0: to the chain's end)
    uint64_t out_pos;                      // first byte, counted from the stream's first byte of this call
    uint64_t out_len;                      // bytes
    unsigned long long sumS, sumI;         // Adler-32 partial sums over its bytes (not reduced)
    uint32_t present, failed;
};

struct DeflateJob {
    const uint8_t *src;
    uint8_t       *dst;
    uint64_t       src_len;
    uint64_t       dst_cap;
    int32_t        format, level;
    uint32_t       image;
    uint32_t       exponent;      // window = 2^exponent (LZ77.Deflator(exponent:); PNG: 15)
    uint32_t       more;          // spng_deflate_resume_batch: more input will follow (src_len is what arrived so far)
    struct D1State *state;        // ... and where the stream keeps itself between pushes (levels 0-7: a D1State, 8 and up: a D2State; null: one-shot)
    uint64_t       plan_pos;      // (host side: where the previous push left the parse; levels >= 8: its block limit, 0-7: how far
    uint32_t       plan_limit, pad2;   //  the input has been searched -- what the previous call returned in aux[0], aux[1])
    uint64_t       plan_aux;
};

// A stream of levels 0-7 between two pushes (spng_deflate_resume_batch): the parse position, the terms queued for the
// block being filled, the bit writer, the Adler sums.  The hash window is not kept: the next push enters the last 32 KiB again.
struct D1State {
    uint64_t w, inserted;         // first unparsed position; (not read any more: a free word)
    uint64_t acc, total;          // the bit writer: pending bits, bytes produced
    uint32_t nacc, overflow, count, started;
    uint32_t adlerS, adlerI, pad[2];
    uint32_t terms[2048];
    // the two-kernel form (round 5: dfl3_search_kernel + dfl3_parse_kernel): the positions of the round the parse is at, the
    // search's own cursor (it runs a round ahead) and how far the input has been searched -- rounds partition the positions, so the
    // Adler sums the search workgroups add up (unreduced, adlerS / adlerI) count every byte once whatever the pushes were.
    // LIMIT: the two sums are 32-bit and grow by up to 65 520 per search chunk and push (deflate.hip: atomicAdd(adlerS, S % 65521)): a
    // stream of more than 65 536 chunks or pushes could wrap them (include/spng_mi355.h, spng_deflate_resume_batch, says so too).
    uint64_t rb, re, srb, sre, spos;
    uint32_t done, pad3;
};
// One stream of the greedy / lazy levels in the two-kernel form
struct D3Stream {
    const uint8_t *src; uint8_t *dst;
    uint64_t src_len, dst_cap;
    int32_t  format, level;
    uint32_t image, exponent;
    uint32_t more, pad;
    D1State *state;
    uint32_t *match[2];           // by round parity: per position of the round (and one behind it) run << 16 | distance, 0: no run > 5
    // the block-parallel form (one-shot streams: dfl4_walk / dfl4_block / dfl4_scan / dfl4_place), null otherwise
    uint32_t *terms;              // the round's terms, block after block
    uint32_t *bdesc;              // [0] blocks of the round, [1] the stream's last round, [2..3] the bit the round starts at; then per block {first term, terms | final << 31}
    uint64_t *bbits;              // per block: the bits it takes (dfl4_block), its first bit in the stream (dfl4_scan) at [max blocks + k]
    uint8_t  *scratch;            // per block D4_BCAP bytes: its bits from bit 0 on
};

// levels >= 8, the two-kernel form (deflate.hip, "round 4"): what the search and the parse kernel share per stream.
struct D2State {                  // device side, kept from round to round; arrives zeroed except rb / re / limit / generic
    uint64_t rb, re;              // the positions of the current round
    uint64_t pos;                 // first position not parsed yet
    uint32_t limit, generic;      // block limit of the next block; the first block of a stream iterates twice as often
    uint64_t acc, total;          // the bit writer: pending bits, bytes produced
    uint32_t nacc, overflow;
    uint32_t adlerS, adlerI;      // Adler-32 partial sums of the chunks searched so far (mod 65521 each time)
    uint32_t fail, done;          // the pool ran dry under this stream (the one-kernel search takes it afterwards); finished
    uint8_t  depths[544];         // LZ77.DeflatorMatches.Depths between blocks
    uint32_t started, pad;        // (a state arrives zeroed: the first round of the first call sets the block limit)
    // the search kernel's own cursor: it runs a round ahead of the parse (block boundaries are a function of the positions alone)
    uint64_t srb, sre, spos;
    uint32_t slimit, spad;
};
struct D2Stream {
    const uint8_t *src; uint8_t *dst;
    uint64_t src_len, dst_cap;
    int32_t  format, level;
    uint32_t image, exponent;
    uint32_t more, pad;           // spng_deflate_resume_batch: more input will follow -- only blocks whose every vertex has its whole
                                  // look-ahead (258 bytes, + 3 for the key) are taken now
    D2State *state;
    // scratch, round coordinates (vertex = position - rb): per vertex candidates << 9 | longest run; per batch of 64 the first
    // word of its list in the pool and words | longest run << 16; block coordinates: which vertices keep their edges, the
    // ways in, the path
    uint16_t *vinfo; uint64_t *bbase; uint32_t *bwords; uint64_t *emask;
    uint16_t *vinfo2; uint64_t *bbase2; uint32_t *bwords2;   // (the candidate records of the odd rounds: round r + 1 is searched while round r is parsed)
    uint32_t *up, *step; uint8_t *pathb, *litb;   // (litb: per batch of the block, nothing but literal ways in)
};

// PNG.adam7, PNG.Decoder.swift:6-15
struct Pass { uint32_t bx, by, sx, sy, w, h; uint64_t pitch; };
int passes(uint32_t w, uint32_t h, int volume, int interlaced, Pass out[7]);

// A job per grid row.  The grid's y stops at 65535, so `count` jobs take one launch per 65535 of them: launch(y0, ny) launches
// rows [y0, y0 + ny) -- every per-job pointer it passes moves on by y0 --; -> hipGetLastError() behind the last launch.
template <class Launch> inline hipError_t launch_rows(uint32_t count, Launch launch)
{
    for (uint32_t y0 = 0; y0 < count; y0 += 65535u) launch(y0, count - y0 < 65535u ? count - y0 : 65535u);
    return hipGetLastError();
}

// kernel launchers (each returns the hipError_t of the launch)
hipError_t launch_unfilter(const UnfJob *d_jobs, uint32_t count, uint32_t bpp, spng_result *d_results,
                           uint32_t pieces, uint32_t piece_rows, hipStream_t stream, uint32_t widest = 0);   // widest: the longest row of the batch in bytes
hipError_t launch_copy_probe(const void *d_src, void *d_dst, uint64_t bytes, int pattern, hipStream_t stream);
hipError_t launch_scatter(const ScatterJob *d_jobs, uint32_t count, const uint32_t *d_job_image,
                          const spng_result *d_results, uint32_t blocks_x, hipStream_t stream);
hipError_t launch_overdraw(const OverdrawJob *d_jobs, uint32_t count, uint32_t blocks_x, hipStream_t stream);
hipError_t launch_inflate(const InflateJob *d_jobs, uint32_t count, spng_result *d_results,
                          hipStream_t stream);
// pinflate2.hip: the parallel inflate pipeline
hipError_t launch_pinf2_find(PStream *d_streams, PSeg *d_segs, uint32_t seg0, uint32_t nsegs, uint32_t retry, hipStream_t stream);
hipError_t launch_pinf2_decode(PStream *d_streams, PSeg *d_segs, uint32_t seg0, uint32_t nsegs, uint32_t *d_pt, uint8_t *d_pool, uint32_t *d_next,
                               uint32_t pages, uint32_t retry, hipStream_t stream);
hipError_t launch_pinf2_scan(PStream *d_streams, uint32_t nstreams, PSeg *d_segs, PPart *d_parts, uint32_t retry, hipStream_t stream);
hipError_t launch_pinf2_resolve(PStream *d_streams, uint32_t nstreams, PSeg *d_segs, uint32_t *d_pt, uint8_t *d_pool, uint32_t pages,
                                spng_result *d_results, int32_t *d_done, PPart *d_parts, uint32_t pmax, uint32_t retry, hipStream_t stream);
hipError_t launch_pinf2_parts(PStream *d_streams, uint32_t nstreams, PSeg *d_segs, uint32_t *d_pt, uint8_t *d_pool, uint32_t pages,
                              spng_result *d_results, int32_t *d_done, PPart *d_parts, uint32_t pmax, uint16_t *d_sym, hipStream_t stream);
hipError_t launch_pinf2_join(PStream *d_streams, uint32_t nstreams, spng_result *d_results, int32_t *d_done, PPart *d_parts, uint32_t pmax,
                             uint16_t *d_sym, uint8_t *d_win, hipStream_t stream);
hipError_t launch_pinf2_cutplan(PStream *d_streams, uint32_t nstreams, PSeg *d_segs, PCut *d_cuts, uint32_t *d_stats, hipStream_t stream);
hipError_t launch_pinf2_cutdecode(PStream *d_streams, PSeg *d_segs, PCut *d_cuts, uint32_t seg0, uint32_t nsegs, uint32_t *d_pt, uint8_t *d_pool,
                                  uint32_t *d_next, uint32_t pages, hipStream_t stream);
hipError_t launch_pinf2_cutjoin(PStream *d_streams, PSeg *d_segs, PCut *d_cuts, uint32_t seg0, uint32_t nsegs, uint32_t *d_pt, uint8_t *d_pool,
                                uint32_t *d_next, uint32_t pages, uint32_t *d_stats, hipStream_t stream);
hipError_t launch_pinf2_cutscan(PStream *d_streams, uint32_t nstreams, PSeg *d_segs, PCut *d_cuts, PPart *d_parts, uint32_t *d_stats, hipStream_t stream);
hipError_t launch_pinf2_account(uint32_t *d_ctr, uint32_t *d_totals, uint32_t pages, hipStream_t stream);
// gzip.hip
static constexpr uint64_t GZ_NONE = ~0ull;
uint32_t   gzip_pieces();
hipError_t launch_gzip_pre(InflateJob *d_jobs, PStream *d_streams, spng_result *d_results, uint64_t *d_gz, int32_t *d_done,
                           uint32_t count, hipStream_t stream);
hipError_t launch_gzip_inflate_post(const InflateJob *d_jobs, spng_result *d_results, const uint64_t *d_gz, uint32_t *d_parts,
                                    uint32_t count, hipStream_t stream);
hipError_t launch_gzip_deflate_post(const DeflateJob *d_jobs, spng_result *d_results, uint32_t *d_parts, uint32_t count,
                                    hipStream_t stream);
hipError_t launch_resume_post(const InflateJob *d_jobs, spng_result *d_results, uint64_t *d_parts, uint32_t count, hipStream_t stream);
uint64_t deflate_state_bytes();
uint32_t deflate2_plan(uint64_t n, bool more, uint64_t &pos, uint32_t &lim);
hipError_t launch_deflate2_begin(const D2Stream *d_streams, uint32_t count, hipStream_t stream);
uint64_t deflate2_vertices(uint64_t n);
hipError_t launch_deflate2_search(const D2Stream *d_streams, uint32_t count, uint32_t cps, uint32_t chunk_len, uint32_t *d_pool, unsigned long long *d_pool_next,
                                  uint64_t pool_words, uint32_t *d_temp, uint32_t parity, hipStream_t stream);
uint64_t deflate2_temp_bytes(uint32_t workgroups);
// levels 0-7 in rounds (deflate.hip, "round 5")
uint64_t deflate3_round_positions();
uint64_t deflate3_end(uint64_t n, bool more);
hipError_t launch_deflate3_begin(const D3Stream *d_streams, uint32_t count, hipStream_t stream);
hipError_t launch_deflate3_search(const D3Stream *d_streams, uint32_t count, uint32_t cps, uint32_t chunk_len, uint32_t parity, hipStream_t stream);
hipError_t launch_deflate3_probe(hipStream_t stream);
hipError_t deflate3_probe_result(uint32_t *ordered);      // once per context: may the match search's inserter use the one-exchange form?
hipError_t launch_deflate3_parse(const D3Stream *d_streams, uint32_t count, spng_result *d_results, uint32_t parity, hipStream_t stream);
// ... with the blocks written side by side (one-shot streams)
uint64_t deflate4_max_blocks(uint64_t positions);
uint64_t deflate4_block_bytes();
hipError_t launch_deflate4_round(const D3Stream *d_streams, uint32_t count, uint32_t max_blocks, spng_result *d_results, uint32_t parity, hipStream_t stream);
hipError_t launch_deflate2_parse(const D2Stream *d_streams, uint32_t count, const uint32_t *d_pool, spng_result *d_results, uint32_t parity, hipStream_t stream);
hipError_t launch_deflate2_failed(const D2Stream *d_streams, uint32_t count, uint32_t *d_failed, hipStream_t stream);
hipError_t launch_unpack(const UnpackJob *d_jobs, uint32_t count, uint32_t blocks_x, int target, hipStream_t stream);
hipError_t launch_pack(const PackJob *d_jobs, uint32_t count, uint32_t blocks_x, int source, hipStream_t stream);
hipError_t launch_alpha(const AlphaJob *d_jobs, uint32_t count, uint32_t blocks_x, int bits, hipStream_t stream);
hipError_t launch_hsva(const HsvaJob *d_jobs, uint32_t count, uint32_t blocks_x, hipStream_t stream);
hipError_t launch_luminance(const LuminanceJob *d_jobs, uint32_t count, uint32_t blocks_x, hipStream_t stream);
uint32_t census_slots(uint32_t cap);                       // slots of an image's table
uint32_t census_sort_elems(uint32_t cap);
hipError_t launch_census(const CensusJob *d_jobs, uint32_t count, uint32_t blocks_x, int bits, hipStream_t stream);
hipError_t launch_pack_indexed(const PackIndexedJob *d_jobs, uint32_t count, uint32_t blocks_x, int source, hipStream_t stream);
// colour_tables.hip (the counting stage of the wide census is census_kernel: launch_census_count, indexing.hip)
hipError_t launch_census_count(const CensusJob *d_jobs, uint32_t count, uint32_t blocks_x, int bits, hipStream_t stream);
hipError_t launch_census_wide_finish(const CensusJob *d_jobs, uint32_t count, uint32_t most_slots, uint32_t most_keys, hipStream_t stream);
uint32_t map_slots(uint32_t map_count);                    // slots of a map's table in scratch; 0: it sits in LDS
hipError_t launch_map(const MapJob *d_jobs, uint32_t count, unsigned long long *d_scratch, uint32_t build_blocks_x, uint32_t blocks_x,
                      int source, hipStream_t stream);
size_t lex_chunk_bytes();
size_t lex_walk_bytes();
hipError_t launch_lex(const spng_file_desc *d_files, uint32_t count, spng_lexed *d_out, void *d_table, const uint64_t *d_table_at,
                      void *d_walks, uint32_t max_listed, hipStream_t stream);
hipError_t launch_lex_dir(const spng_file_desc *d_files, const spng_chunk_dir *d_dirs, uint32_t count, const spng_lexed *d_out, const void *d_table,
                          const uint64_t *d_table_at, const void *d_walks, uint32_t most_entries, hipStream_t stream);
// behind launch_lex_dir on the same stream, over its files, directories and infos; most_entries as there
hipError_t launch_parse_dir(const spng_file_desc *d_files, const spng_chunk_dir *d_dirs, uint32_t count, const spng_lexed *d_infos,
                            spng_chunk_value *const *d_values, uint32_t most_entries, spng_parsed *d_parsed, hipStream_t stream);
size_t text_tiles(uint64_t len);
// blocks_x: workgroups along x of the per-tile kernels (0: no text of the call has a tile); writes: some text is transcoded
hipError_t launch_text(const TextJob *d_jobs, uint32_t count, uint32_t blocks_x, bool writes, spng_result *d_results, hipStream_t stream);
size_t lex_state_bytes();
size_t lex_piece_bytes();
size_t lex_rwalk_bytes();
hipError_t launch_lex_resume(const spng_file_desc *d_files, void *const *d_states, uint32_t count, spng_lexed *d_out, void *d_table,
                             const uint64_t *d_table_at, void *d_walks, uint32_t max_listed, uint64_t *d_stats, hipStream_t stream);
hipError_t launch_write_idat(const spng_chunking_desc *d_descs, uint32_t count, uint32_t blocks_x, spng_result *d_results, hipStream_t stream);
// finish_chunks: the most chunks of several pieces a file of the launch can have (0: none can, nothing to fold)
hipError_t launch_write_file(const FileJob *d_jobs, uint32_t count, uint32_t blocks_x, uint64_t finish_chunks, spng_result *d_results,
                             hipStream_t stream);
hipError_t launch_crc_partial(const uint8_t *d, uint64_t n, uint64_t piece, uint32_t *d_partial, uint32_t pieces, hipStream_t stream);
uint32_t crc32_fold(const uint32_t *partial, uint64_t pieces, uint64_t n, uint64_t piece);
hipError_t launch_filter(const FilterJob *d_jobs, uint32_t count, uint32_t max_rows, hipStream_t stream);
hipError_t launch_adler_partial(const uint8_t *d, uint64_t n, uint32_t chunk, uint64_t *d_out, uint32_t blocks,
                                hipStream_t stream);

}  // namespace spng
