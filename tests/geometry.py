"""The library's launch arithmetic (swift_png_amd/csrc/geometry.hpp), callable from the tests: tools/geometry_c.cpp forwards to it
behind a C ABI; this module compiles that once per process with the host compiler into a temporary directory (nothing is left in
the tree) and loads it with ctypes.  Importable without a GPU, and needed on a machine with one too: the case table of the scanline
tests is built on it.  It never skips: where the shim cannot be built, the table is wrong to trust."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift_png_amd", "csrc")
CLANG = os.environ.get("SPNG_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")       # (the host compiler beside hipcc, as tests/emu_build.py)
RULES = ("configured", "scaled", "floor128", "wide", "rr", "floor4", "few")     # enum PieceRule

_u32, _u64 = ctypes.c_uint32, ctypes.c_uint64


def _load():
    d = tempfile.mkdtemp(prefix="spng_geometry_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "geometry_c.so")
    run = subprocess.run([CLANG, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I" + CSRC, "-o", so,
                          os.path.join(ROOT, "tools", "geometry_c.cpp")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lib = ctypes.CDLL(so)
    for name, res, args in (("geo_unfilter_pieces", None, (_u32, _u64, _u32, _u64, _u32, ctypes.POINTER(_u32))),
                            ("geo_unfilter_wide_tiles", ctypes.c_int32, (_u32, _u64)),
                            ("geo_band_steps_needed", _u32, (_u32, _u32, _u32, _u32, _u32)),
                            ("geo_band_may_wait", ctypes.c_int32, (_u32, _u32, _u32)),
                            ("geo_filter_blocks_x", _u32, (_u32,)),
                            ("geo_plane_blocks_x", _u32, (_u64, _u32)),
                            ("geo_blocks_for", _u32, (_u64, _u32)),
                            ("geo_census_blocks_x", _u32, (_u32, _u64)),
                            ("geo_write_idat_blocks_x", _u32, (_u64,)),
                            ("geo_lex_listed", _u64, (_u64,)),
                            ("geo_lex_piece_blocks_x", _u32, (_u32, _u32)),
                            ("geo_inflate_segment_bytes", _u64, (_u64, _u64, ctypes.c_double)),
                            ("geo_search_chunks", None, (_u64, ctypes.POINTER(_u32))),
                            ("geo_constant", ctypes.c_int64, (ctypes.c_char_p,))):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


_lib = _load()


def constant(name: str) -> int:
    """a named constant of geometry.hpp"""
    v = _lib.geo_constant(name.encode())
    assert v >= 0, name
    return v


assert [constant("PieceRule::" + r) for r in RULES] == list(range(len(RULES)))


def unfilter_pieces(k, total_rows, max_rows, widest, configured=0):
    """-> (rows per piece, pieces, the rule that set the length: one of RULES)"""
    out = (_u32 * 3)()
    _lib.geo_unfilter_pieces(k, total_rows, max_rows, widest, configured, out)
    return out[0], out[1], RULES[out[2]]


def unfilter_wide_tiles(k, widest) -> bool:
    return bool(_lib.geo_unfilter_wide_tiles(k, widest))


def band_may_wait(nw, reach, per_band) -> bool:
    return bool(_lib.geo_band_may_wait(nw, reach, per_band))


def search_chunks(streams):
    """-> (chunks per stream, positions per chunk)"""
    out = (_u32 * 2)()
    _lib.geo_search_chunks(streams, out)
    return out[0], out[1]


band_steps_needed = _lib.geo_band_steps_needed
filter_blocks_x = _lib.geo_filter_blocks_x
plane_blocks_x = _lib.geo_plane_blocks_x
blocks_for = _lib.geo_blocks_for
census_blocks_x = _lib.geo_census_blocks_x
write_idat_blocks_x = _lib.geo_write_idat_blocks_x
lex_listed = _lib.geo_lex_listed
lex_piece_blocks_x = _lib.geo_lex_piece_blocks_x
inflate_segment_bytes = _lib.geo_inflate_segment_bytes
