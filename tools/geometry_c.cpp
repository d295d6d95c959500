// geometry_c.cpp -- test infrastructure: the launch arithmetic of csrc/geometry.hpp behind a C ABI, so that the tests call what
// the library runs (tests/geometry.py compiles this with the host compiler and loads it with ctypes).  Nothing here computes.
#include <string.h>
#include "geometry.hpp"

using namespace spng;

extern "C" {

void geo_unfilter_pieces(uint32_t k, uint64_t total_rows, uint32_t max_rows, uint64_t widest, uint32_t configured, uint32_t out[3])
{
    const UnfilterPieces p = unfilter_pieces(k, total_rows, max_rows, widest, configured);
    out[0] = p.piece_rows; out[1] = p.pieces; out[2] = (uint32_t)p.rule;
}
int32_t geo_unfilter_wide_tiles(uint32_t k, uint64_t widest) { return unfilter_wide_tiles(k, widest); }
uint32_t geo_band_steps_needed(uint32_t band, uint32_t step, uint32_t nw, uint32_t per_band, uint32_t reach) { return band_steps_needed(band, step, nw, per_band, reach); }
int32_t geo_band_may_wait(uint32_t nw, uint32_t reach, uint32_t per_band) { return band_may_wait(nw, reach, per_band); }
uint32_t geo_filter_blocks_x(uint32_t max_rows) { return filter_blocks_x(max_rows); }
uint32_t geo_plane_blocks_x(uint64_t max_pixels, uint32_t cap) { return plane_blocks_x(max_pixels, cap); }
uint32_t geo_blocks_for(uint64_t most, uint32_t per_block) { return blocks_for(most, per_block); }
uint32_t geo_census_blocks_x(uint32_t count, uint64_t most) { return census_blocks_x(count, most); }
uint32_t geo_write_idat_blocks_x(uint64_t most_pieces) { return write_idat_blocks_x(most_pieces); }
uint64_t geo_lex_listed(uint64_t len) { return lex_listed(len); }
uint64_t geo_lex_resume_pieces(uint64_t new_bytes, int32_t complete) { return lex_resume_pieces(new_bytes, complete != 0); }
uint64_t geo_lex_resume_listed(uint64_t len) { return lex_resume_listed(len); }
uint32_t geo_lex_piece_blocks_x(uint32_t count, uint32_t max_listed) { return lex_piece_blocks_x(count, max_listed); }
uint64_t geo_inflate_segment_bytes(uint64_t configured, uint64_t total, double block_bytes) { return inflate_segment_bytes(configured, total, block_bytes); }
void geo_search_chunks(uint64_t streams, uint32_t out[2])
{
    const SearchChunks s = search_chunks(streams);
    out[0] = s.cps; out[1] = s.chunk_len;
}

// a named constant of geometry.hpp (the names of enum PieceRule: their values), -1: no such name
int64_t geo_constant(const char *name)
{
#define C(x) if (!strcmp(name, #x)) return (int64_t)(x)
    C(PIECE_SCALE_ROWS); C(PIECE_FLOOR); C(WIDE_ROW); C(WIDE_SCALE_ROWS); C(WIDE_FLOOR); C(WIDE_CEIL);
    C(PK_BAND_BYTES); C(PK_SCALE_ROWS); C(PK_FILL_ROWS); C(PK_FLOOR_BANDS); C(PK_FEW_HEIGHT); C(PK_FEW_ROWS); C(PK_FEW_MIN); C(PK_FEW_MAX);
    C(FILTER_ROWS_PER_BLOCK); C(FILTER_BLOCKS_MAX); C(SCATTER_BLOCKS_MAX); C(OVERDRAW_BLOCKS_MAX); C(SMALL_BLOCK_BYTES);
    C(SEARCH_ROUND_POSITIONS); C(LEX_PIECE_BYTES);
    C(PieceRule::configured); C(PieceRule::scaled); C(PieceRule::floor128); C(PieceRule::wide); C(PieceRule::rr); C(PieceRule::floor4);
    C(PieceRule::few);
#undef C
    return -1;
}

}  // extern "C"
