"""The launch arithmetic the library runs (csrc/geometry.hpp through tests/geometry.py) still computes what the host layer computed
when the rules were written inline in its launch functions: tests/golden/launch_geometry.json, made by
tests/golden/make_launch_geometry.py before they moved.  And bench_one_block.py's own segment count is the library's.  No GPU needed."""
import json
import os
import sys

import geometry as geo
import pnghelp as ph

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_geometry.json")))


def test_the_arithmetic_is_what_it_was_written_inline():
    for k, total, max_rows, widest, configured, kernel, rule, piece, pieces in GOLDEN["unfilter_pieces"]:
        assert geo.unfilter_pieces(k, total, max_rows, widest, configured) == (piece, pieces, rule), (k, total, max_rows, widest, configured)
        assert geo.unfilter_wide_tiles(k, widest) == kernel.endswith(",32>"), (k, widest, kernel)
    for name in ("filter_blocks_x", "plane_blocks_x", "blocks_for", "census_blocks_x", "write_idat_blocks_x", "lex_listed",
                 "inflate_segment_bytes"):
        assert len(GOLDEN[name]) >= 180, name
        for *args, want in GOLDEN[name]:
            assert getattr(geo, name)(*args) == want, (name, args)
    for streams, cps, chunk_len in GOLDEN["search_chunks"]:
        assert geo.search_chunks(streams) == (cps, chunk_len), streams
    assert len(GOLDEN["unfilter_pieces"]) >= 180 and len(GOLDEN["search_chunks"]) >= 180
    assert {r[6] for r in GOLDEN["unfilter_pieces"]} == set(geo.RULES)


def test_the_grid_of_the_lexer_sum_and_copy_launch():
    """8192 / count waves per file, rounded up, four at least, and no more than the longest list (one where there is none): the values
    the rule gave when it stood inline in the launchers of both lexer entries"""
    want = {1: (1, 1, 3, 5000), 4: (1, 1, 3, 2048), 2048: (1, 1, 3, 4), 8192: (1, 1, 3, 4), 8193: (1, 1, 3, 4)}
    for count, row in want.items():
        assert tuple(geo.lex_piece_blocks_x(count, m) for m in (0, 1, 3, 5000)) == row, count


def test_bench_one_block_counts_the_segments_the_library_cuts():
    sys.path.insert(0, str(ph.ROOT))
    import bench_one_block as bob
    # the compressed bytes of its legs (fixed_32MiB, dynamic_64MiB, fpnge_4k: "in_bytes" in profiles/r07_one_block.md), and a sweep
    # from 1 byte to 1 GiB
    lengths = [33554440, 12040423, 37026127]
    n = 1
    while n <= 1 << 30:
        lengths += [m for m in (n - 1, n, n + 1, n + n // 3) if 1 <= m <= 1 << 30]
        n *= 2
    for n in lengths:
        seg = geo.inflate_segment_bytes(0, n, 0.0)
        assert bob.segments(n) == (n + seg - 1) // seg, n
