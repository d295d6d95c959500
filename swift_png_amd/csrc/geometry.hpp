// geometry.hpp -- the launch arithmetic of libspng_mi355.so: every rule that turns a batch into a grid, as plain functions of
// numbers.  Plain C++17 without a HIP header, so that the tests call the very functions the library runs (tools/geometry_c.cpp
// forwards to them, tests/geometry.py loads that) instead of restating them.
#ifndef SPNG_GEOMETRY_HPP     // (not #pragma once: the header also compiles alone, as the main file)
#define SPNG_GEOMETRY_HPP
#include <algorithm>
#include <cstdint>

namespace spng {

// ---- unfilter: rows per piece -----------------------------------------------------------------------------------
// Enough workgroups to fill the chip: chains are cut into pieces of piece_rows rows (unfilter.hip: at rows filtered with
// None / Sub) when there are few of them.
constexpr uint32_t PIECE_SCALE_ROWS = 4096;      // rows of the call per row of a piece, rounded up to bands of 64 rows
constexpr uint32_t PIECE_FLOOR = 128;
// (round 6: a piece of 128 rows is two bands of 64 -- two of the workgroup's four waves have nothing to do.  Rows of
//  2 KiB and more take four bands at least: 128 x 4096^2 RGB16 15.2 -> 10.0 ms, 256 x RGB8 10.5 -> 10.0; rows of a
//  1-bit image, 512 bytes, want the workgroups more than the waves: profiles/r06_tuning.md 15)
constexpr uint32_t WIDE_ROW = 2048;              // bytes of the call's widest row from which on the wide rules hold
constexpr uint32_t WIDE_SCALE_ROWS = 2048, WIDE_FLOOR = 256, WIDE_CEIL = 1024;
// (the line-aligned kernel, pixels of 4 and 8 bytes: bands of 128 / bpp rows, 64 / that many chains per wave -- pieces may be
//  shorter, and a few images still fill the chip)
constexpr uint32_t PK_BAND_BYTES = 128, PK_SCALE_ROWS = 8192;
// (a piece of fewer than four bands leaves waves of its 4-wave workgroup idle and pays a pipeline fill per
//  band: while two rounds of resident workgroups -- 3 per CU -- are there anyway, pieces are not cut below
//  four bands.  128 images: 64-row pieces, 9.4 ms -> 128-row pieces; VERDICT r4 "what's weak" 6)
constexpr uint32_t PK_FILL_ROWS = 1536, PK_FLOOR_BANDS = 4;
// (round 6, measured per batch size -- profiles/r06_tuning.md 16: 128 x 4096^2 RGBA8 want pieces of 256 rows
//  (7.1 -> 5.9 ms), 32 images 128 (3.0 -> 2.3), 8 images 64 (1.8 -> 1.5): total rows / 1024, between 64 and 256)
//  -- for 4-byte pixels in images of 1024 rows and more, what was measured: the 8192^2 RGBA16 image of configs[4], whose
//  rows are 64 KiB, wants its 16-row bands one to a piece (3.9 ms; 64-row pieces 5.5), and images of 240 rows
//  two pieces each)
constexpr uint32_t PK_FEW_HEIGHT = 1024, PK_FEW_ROWS = 1024, PK_FEW_MIN = 64, PK_FEW_MAX = 256;

enum class PieceRule { configured, scaled, floor128, wide, rr, floor4, few };    // the clause that set the length
struct UnfilterPieces { uint32_t piece_rows, pieces; PieceRule rule; };

// The pieces of one unfilter launch.  k: bytes per pixel; total_rows, max_rows, widest: over the jobs of the launch (rows in all,
// of the tallest job, bytes of the longest row); configured: SPNG_CFG_UNFILTER_PIECE_ROWS (0: by the rules above).
inline UnfilterPieces unfilter_pieces(uint32_t k, uint64_t total_rows, uint32_t max_rows, uint64_t widest, uint32_t configured)
{
    uint32_t piece_rows = configured;
    PieceRule rule = PieceRule::configured;
    if (!piece_rows) {
        piece_rows = (uint32_t)((total_rows / PIECE_SCALE_ROWS + 63) & ~(uint64_t)63);
        rule = PieceRule::scaled;
        if (piece_rows < PIECE_FLOOR) { piece_rows = PIECE_FLOOR; rule = PieceRule::floor128; }
        if (widest >= WIDE_ROW && k != 4 && k != 8) {
            piece_rows = (uint32_t)((total_rows / WIDE_SCALE_ROWS + 63) & ~(uint64_t)63);
            if (piece_rows < WIDE_FLOOR) piece_rows = WIDE_FLOOR;
            if (piece_rows > WIDE_CEIL) piece_rows = WIDE_CEIL;
            rule = PieceRule::wide;
        }
        if (k == 4 || k == 8) {
            const uint32_t rr = PK_BAND_BYTES / k;
            piece_rows = (uint32_t)((total_rows / PK_SCALE_ROWS + rr - 1) / rr * rr);
            if (piece_rows < rr) piece_rows = rr;
            rule = PieceRule::rr;
            const uint32_t fill = (uint32_t)(total_rows / PK_FILL_ROWS / rr * rr);
            const uint32_t floor4 = fill < PK_FLOOR_BANDS * rr ? fill : PK_FLOOR_BANDS * rr;
            if (piece_rows < floor4) { piece_rows = floor4; rule = PieceRule::floor4; }
            if (k == 4 && max_rows >= PK_FEW_HEIGHT) {
                uint32_t few = (uint32_t)((total_rows / PK_FEW_ROWS + rr - 1) / rr * rr);
                few = few < PK_FEW_MIN ? PK_FEW_MIN : few > PK_FEW_MAX ? PK_FEW_MAX : few;
                if (piece_rows < few) { piece_rows = few; rule = PieceRule::few; }
            }
        }
    }
    return {piece_rows, (max_rows + piece_rows - 1) / piece_rows, rule};
}

// unfilter_kernel for pixels of 1 and 2 bytes: tiles of 32 dword units for rows of 2 KiB and more, of SPNG_UNF_PSUB = 16 for
// narrower ones -- wide tiles cost rows of 512 bytes a third and save rows of 4 KiB a sixth: profiles/r06_tuning.md 14
inline bool unfilter_wide_tiles(uint32_t k, uint64_t widest) { return (k == 1 || k == 2) && widest >= WIDE_ROW; }

// ---- unfilter: the hand-over between the bands of a piece --------------------------------------------------------------
// The nw waves of a workgroup take the bands of a piece in turn (band j: wave j % nw) and each counts the steps it has completed,
// over all of its bands, per_band to a band.  Step `step` of a band reads the last row of the band above as the steps
// step .. step + reach of that band left it (reach: how many producer steps a consumer step reaches into -- Cfg::K tiles of
// unfilter_kernel's skewed windows, one phase of unfilter_pk_kernel, whose tile T is stored at the end of phase T + 1).
// -> the count the producing wave must have published before step `step` of `band` (>= 1) may be loaded.
constexpr uint32_t band_steps_needed(uint32_t band, uint32_t step, uint32_t nw, uint32_t per_band, uint32_t reach)
{
    return (band - 1) / nw * per_band + (step + reach < per_band ? step + reach : per_band - 1) + 1;
}
// A wave in the last step of a band may WAIT for the first step of its next band only if that wait cannot close a circle.
// Every wave in between may itself be waiting, in front of its staged step with only the steps before it published, so each hop
// from band to band reaches back reach + 1 steps, and nw hops end at step nw * (reach + 1) - 1 of the waiting wave's own current
// band: that step must lie in front of the last one, which is the one it has not published.  (The first form of this bound,
// nw * reach + 1 < per_band, hung a workgroup for good: tests/test_emu_unfilter.py "one long piece".)  Shorter rows do not
// prefetch across the band; what that costs them has not been measured.
// By that count alone nw * (reach + 1) < per_band would do: the bound asks for one step more, as both kernels' own bounds did
// before they became this one.  Nothing in the tests tells the two apart -- the cases at the very edge ("9 phases" / "10 phases",
// "13 tiles" / "14 tiles") pass even with the first form, and only the "one long piece" and "pieces only where None / Sub
// allow" cases catch a bound that is too loose -- so the edge cases are no licence to take the step of slack away.
constexpr bool band_may_wait(uint32_t nw, uint32_t reach, uint32_t per_band) { return nw * (reach + 1) + 1 < per_band; }

// ---- workgroups along x ------------------------------------------------------------------------------------------
// filter_kernel: a workgroup is four waves, a row per wave; images taller than the grid loop.
constexpr uint32_t FILTER_ROWS_PER_BLOCK = 4, FILTER_BLOCKS_MAX = 4096;
inline uint32_t filter_blocks_x(uint32_t max_rows)
{
    const uint32_t bx = std::min((max_rows + FILTER_ROWS_PER_BLOCK - 1) / FILTER_ROWS_PER_BLOCK, FILTER_BLOCKS_MAX);
    return bx ? bx : 1;
}

// scatter (cap SCATTER_BLOCKS_MAX) and overdraw (cap OVERDRAW_BLOCKS_MAX): a thread per pixel of the largest plane, grid-stride
constexpr uint32_t SCATTER_BLOCKS_MAX = 1024, OVERDRAW_BLOCKS_MAX = 4096;
inline uint32_t plane_blocks_x(uint64_t max_pixels, uint32_t cap) { return std::min((uint32_t)((max_pixels + 255) / 256), cap); }

// Workgroups for the longest array of a call: `per_block` of its elements each (256 threads, a few rounds), 4096 at most.
inline uint32_t blocks_for(uint64_t most, uint32_t per_block) { return (uint32_t)std::min<uint64_t>((most + per_block - 1) / per_block, 4096); }

// census_kernel: about 4096 workgroups over the call (twice what is resident), at least 16 per array: a workgroup that counts
// many pixels merges its table into the image's seldom.  count: arrays of the call; most: pixels of the longest.
inline uint32_t census_blocks_x(uint32_t count, uint64_t most)
{
    const uint64_t bx = 4096 / count < 16 ? 16 : 4096 / count;
    const uint64_t full = (most + 1023) / 1024;                 // (four pixels per thread, 256 threads)
    return (uint32_t)std::min(bx, full);
}

// write_idat_kernel: a workgroup per IDAT chunk of the stream with the most
inline uint32_t write_idat_blocks_x(uint64_t most_pieces) { return (uint32_t)std::min<uint64_t>(most_pieces, 4096); }

// lex_chunk_kernel's chunk list of a file of `len` bytes: it holds at most len / 12 chunks; 64 KiB IDATs are the usual case, so a
// list of len / 2048 + 64 entries (at most 8192) is plenty, and a file with more is finished by its own wave
inline uint64_t lex_listed(uint64_t len) { return std::min<uint64_t>(std::min(len / 2048 + 64, len / 12 + 1), 8192); }

// lexr_piece_kernel (files that arrive in pieces): the bytes of a chunk's type + data that are new with a push are summed in pieces of
// LEX_PIECE_BYTES, a wave each -- a file that is one huge IDAT pushed in large parts must not wait for one wave.  A chunk that became
// complete takes a piece even when nothing of it is left to sum (only its checksum field arrived): somebody has to compare.
constexpr uint64_t LEX_PIECE_BYTES = 1u << 20;
constexpr uint64_t lex_resume_pieces(uint64_t new_bytes, bool complete)
{
    return new_bytes ? (new_bytes + LEX_PIECE_BYTES - 1) / LEX_PIECE_BYTES : complete ? 1 : 0;
}
// its list for a file of which `len` bytes have arrived: an entry per piece.  The host does not look into the device-side state, so
// the list is sized as if every byte were new: the chunks lex_listed allows and a piece more per LEX_PIECE_BYTES.  Chunks whose
// pieces do not fit are summed by the walking wave itself.
inline uint64_t lex_resume_listed(uint64_t len) { return lex_listed(len) + len / LEX_PIECE_BYTES; }
// lex_chunk_kernel's and lexr_piece_kernel's workgroups along x (y: the files): enough waves to fill the chip; a wave strides over its
// file's list -- four waves per file at least: a batch of small files is as slow as its file with the most chunks.  max_listed: the
// longest list of the call
inline uint32_t lex_piece_blocks_x(uint32_t count, uint32_t max_listed)
{
    const uint32_t want = std::max((8192 + count - 1) / count, 4u);
    return std::min(std::max(max_listed, 1u), want);
}

// wfile_body_kernel (whole files written on the device): a stream of n bytes is cut into IDAT chunks of c bytes, the last one shorter,
// and every chunk into pieces of FILE_PIECE_BYTES that a wave each copies and sums -- a file written as one IDAT must not sit on one
// wave.  A unit is a piece: the units of a stream are those of its full chunks, chunk after chunk, then those of the last.
constexpr uint64_t FILE_PIECE_BYTES = LEX_PIECE_BYTES;
constexpr uint64_t file_pieces(uint64_t chunk_len) { return (chunk_len + FILE_PIECE_BYTES - 1) / FILE_PIECE_BYTES; }
constexpr uint64_t file_chunks(uint64_t n, uint64_t c) { return n ? (n + c - 1) / c : 0; }
constexpr uint64_t file_units(uint64_t n, uint64_t c)
{
    return n ? (file_chunks(n, c) - 1) * file_pieces(c) + file_pieces(n - (file_chunks(n, c) - 1) * c) : 0;
}
// The length may exist on the device only, so the grid is sized by the host-known capacity of the stream (file_units is monotonic in
// n) and surplus workgroups leave; a wave strides over its file's units, as lex_piece_blocks_x has it.  count: files of the launch;
// most_units: the most units any of them can have
inline uint32_t file_blocks_x(uint32_t count, uint64_t most_units)
{
    return lex_piece_blocks_x(count, (uint32_t)std::min<uint64_t>(most_units, 1u << 20));
}

// ---- inflate: segment length -------------------------------------------------------------------------------------
// configured: SPNG_CFG_SEGMENT_BYTES, or (0) by the batch's compressed bytes `total` and the compressed bytes per DEFLATE block
// the last batch showed (block_bytes; 0: not known).
constexpr uint64_t SMALL_BLOCK_BYTES = 8192;
inline uint64_t inflate_segment_bytes(uint64_t configured, uint64_t total, double block_bytes)
{
    uint64_t seg_bytes = configured;
    if (!seg_bytes) {
        const bool small_blocks = block_bytes > 0 && block_bytes < SMALL_BLOCK_BYTES;
        // (~9 rounds of resident waves, so that the last, partly filled one costs little; the search costs 7 ms per 10^4 segments)
        // (small batches: >= 4096 segments if that leaves them 64 KiB -- a zlib block is ~40 KB, and a segment without a block
        // start is a wave without work; one 4K image: 15.1 ms per decode with 256 KiB segments, 10.3 with 64 KiB)
        // (streams of small blocks -- swift-png closes one every 2047 terms, ~2 KB -- as the last batch showed them: their
        // search is nearly free, and twice the segments halve what the last round of resident waves leaves idle:
        // 1024 x 4K images, decode 317 -> 301 ms)
        // (round 6: the search is 2-3 x cheaper -- pinf2_find's bit-parallel screen --, so streams of small blocks take 2.5 x the
        // segments again: 1024 x 4K images, swift-png-made: 418 KB segments 503.4 ms per step, 180 KB 494.5, 140 KB 494.0, 100 KB
        // 500.1; zlib-made streams, whose search still costs 2.4 ms per 10^4 segments, stay: profiles/archive/r06m_probe_segments.log)
        seg_bytes = total / (small_blocks ? 163840 : 32768);
        // (streams of small blocks, whose search is nearly free: 32 .. 64 KiB in small batches -- one 4K image 7.6 -> 6.65 ms per
        // call, 32 images 26.1 -> 22.7; zlib-made streams pay the search of every added segment -- 32 images 23.1 -> 27.0 at 32 KiB --
        // and stay at 64 .. 256 KiB: profiles/archive/r06r_probe_small_segments_*.log)
        uint64_t least = total / 4096;
        const uint64_t lo = small_blocks ? 32u << 10 : 64u << 10, hi = small_blocks ? 64u << 10 : 256u << 10;
        if (least < lo) least = lo;
        if (least > hi) least = hi;
        if (seg_bytes < least) seg_bytes = least;
    }
    return (seg_bytes + 255) & ~(uint64_t)255;
}

// ---- deflate: the match search's chunks ----------------------------------------------------------------------------
// A search workgroup is a CU: one round of them where the streams are few, chunks of 2^20 positions -- 3 % of warm-up -- where
// they are many.  cps: chunks per stream of a round (SEARCH_ROUND_POSITIONS positions at most); chunk_len: positions, whole
// batches of 64.  Every level's search is cut this way.
constexpr uint32_t SEARCH_ROUND_POSITIONS = 1u << 21;
struct SearchChunks { uint32_t cps, chunk_len; };
inline SearchChunks search_chunks(uint64_t streams)
{
    const uint64_t per = (256 + streams - 1) / streams;
    const uint32_t cps = per < 2 ? 2u : per > 64 ? 64u : (uint32_t)per;
    return {cps, ((SEARCH_ROUND_POSITIONS / cps + 63) / 64) * 64};
}

}  // namespace spng

#endif
