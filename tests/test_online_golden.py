"""tests/golden/online.json -- the 35 images the reference's OnlineDecoding tutorial wrote, one after every IDAT chunk of its three runs,
as SHA-256 of their storage (tests/golden/make_online.py) -- held to the checker under oracle/: every snapshot is what the oracle
decodes from the IDAT chunks up to it, and with overdraw what oracle/pixels.py `overdrawn` makes of the final image after the
scanlines those chunks complete.  Where the reference checkout is there, the table is derived again from its files.  And the launch
arithmetic of the resumable lexer (csrc/geometry.hpp) against its stated rule."""
import ctypes
import hashlib
import json
import sys
import zlib

import pytest

import geometry
import pnghelp as ph

sys.path.insert(0, str(ph.ROOT / "oracle"))
sys.path.insert(0, str(ph.GOLDEN))
import make_online  # noqa: E402
import pixels as orc_pixels  # noqa: E402

TABLE = json.loads((ph.GOLDEN / "online.json").read_text())


def scanline_ends(png):
    """inflated bytes after which each scanline is complete, in the order of PNG.Decoder.push"""
    volume, ends, off = png.depth * png.channels, [], 0
    passes = orc_pixels.ADAM7 if png.interlaced else [((0, 0), (0, 0))]
    for (bx, by), (ex, ey) in passes:
        sw, sh = (png.width + (1 << ex) - bx - 1) >> ex, (png.height + (1 << ey) - by - 1) >> ey
        if sw <= 0 or sh <= 0:
            continue
        for _ in range(sh):
            off += ((sw * volume + 7) >> 3) + 1
            ends.append(off)
    return ends


def expected_snapshots(run):
    """-> per IDAT chunk of the run's file the SHA-256 of the storage the oracle gives after it"""
    entry = TABLE[run]
    data = (ph.GOLDEN / "tutorials" / entry["file"]).read_bytes()
    assert (len(data), hashlib.sha256(data).hexdigest()) == (entry["file_len"], entry["file_sha256"])
    png = ph.parse_png(data)
    assert png.idat_chunks == entry["idat_chunks"]
    st, final, _ = ph.orc_decode(png)
    assert st == 0
    elem = len(final) // (png.width * png.height)
    ends, out, pos = scanline_ends(png), [], 0
    for n in png.idat_chunks:
        pos += n
        if entry["overdraw"]:
            inflated = len(zlib.decompressobj().decompress(png.idat[:pos]))
            k = sum(1 for e in ends if e <= inflated)
            storage = orc_pixels.overdrawn(final.reshape(png.height, png.width, elem), k)
        else:
            _, storage, _ = ph.orc_decode(png, png.idat[:pos])
        out.append(hashlib.sha256(storage.tobytes()).hexdigest())
    return out


@pytest.mark.parametrize("run", sorted(make_online.RUNS))
def test_every_snapshot_is_what_the_oracle_gives_for_the_chunks_up_to_it(run):
    name, overdraw, count, _ = make_online.RUNS[run]
    entry = TABLE[run]
    assert (entry["file"], entry["overdraw"], len(entry["snapshots"]), len(entry["idat_chunks"])) == (name, overdraw, count, count)
    assert expected_snapshots(run) == entry["snapshots"]
    assert len(set(entry["snapshots"])) == count                       # (every chunk shows)


def test_the_table_is_what_the_reference_files_give():
    if not (ph.REFERENCE / "Sources" / "PNG" / "docs.docc" / make_online.FOLDER).is_dir():
        pytest.skip("no reference checkout")
    assert make_online.derive(ph.REFERENCE / "Sources" / "PNG" / "docs.docc") == TABLE


def test_pieces_and_list_of_the_resumable_lexer():
    """csrc/geometry.hpp: the new bytes of a chunk go in pieces of 1 MiB, a chunk that became complete takes one even with nothing left
    to sum; the list of a file holds what lex_listed allows and a piece more per MiB that has arrived"""
    lib = geometry._lib                                                 # (tools/geometry_c.cpp, built by tests/geometry.py)
    lib.geo_lex_resume_pieces.restype, lib.geo_lex_resume_pieces.argtypes = ctypes.c_uint64, (ctypes.c_uint64, ctypes.c_int32)
    lib.geo_lex_resume_listed.restype, lib.geo_lex_resume_listed.argtypes = ctypes.c_uint64, (ctypes.c_uint64,)
    piece = geometry.constant("LEX_PIECE_BYTES")
    assert piece == 1 << 20
    for n in (0, 1, 4, piece - 1, piece, piece + 1, 5 * piece // 2, 3 * piece, (1 << 32) + 3, (1 << 40) + 1):
        for complete in (0, 1):
            want = -(-n // piece) if n else complete
            assert lib.geo_lex_resume_pieces(n, complete) == want, (n, complete)
    for n in (0, 11, 12, 164, 4096, piece - 1, piece, 30 << 20, 5 << 30):
        assert lib.geo_lex_resume_listed(n) == geometry.lex_listed(n) + n // piece, n
    # every chunk of a file of n bytes takes at most a piece more than its MiBs: with lex_listed's chunks the pieces fit
    for n, chunks in ((5 * piece // 2 + 45, [13, 5 * piece // 2, 0]), (164, [13, 4, 91, 0])):
        assert sum(lib.geo_lex_resume_pieces(c + 4, 1) for c in chunks) <= lib.geo_lex_resume_listed(n)
