"""The geometry / content table of the scanline tests at production size, and its input generators: shared by the CPU check of the
table (tests/test_scanline_cases.py) and the GPU parity tests (tests/test_gpu_scanlines.py), so both speak of one definition.
Importable without a GPU.  Everything is generated, seeded by a stable function of the case name; nothing is read from disk.

A case names width, height, depth, channels, interlaced, a content kind and a filter-type regime, plus what it CLAIMS about the
dispatch (which kernel, which piece-length rule of `unfilter_pieces`): tests/test_scanline_cases.py holds the claims against the
dispatch itself -- csrc/geometry.hpp, the arithmetic `launch_plan` (csrc/host_decode.hip), `launch_unfilter` (csrc/unfilter.hip) and
`launch_filter` (csrc/encode.hip) run, reached through tests/geometry.py -- and against mirrors of the kernels' internals below,
which restate csrc/unfilter.hip and csrc/encode.hip `filter_kernel` as plain numbers, and checks that the lines those restate
are still in the sources."""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass, replace

import numpy as np

import geometry as geo
import pnghelp as ph

SENTINEL = 0xA5                      # what storage holds before a call: rows that were not decoded must still hold it

# ---- the dispatch constants: the library's own (csrc/geometry.hpp) ---------------------------------------------------------------
WIDE_ROW = geo.constant("WIDE_ROW")  # launch_unfilter: 32-unit tiles for 1- and 2-byte pixels; unfilter_pieces: the 256..1024-row rule
PIECE_FLOOR, WIDE_FLOOR, WIDE_CEIL = (geo.constant(n) for n in ("PIECE_FLOOR", "WIDE_FLOOR", "WIDE_CEIL"))
SCALE_ROWS, WIDE_SCALE_ROWS = geo.constant("PIECE_SCALE_ROWS"), geo.constant("WIDE_SCALE_ROWS")
PK_SCALE_ROWS, PK_FILL_ROWS, PK_FEW_ROWS, PK_FEW_HEIGHT = (geo.constant(n) for n in ("PK_SCALE_ROWS", "PK_FILL_ROWS", "PK_FEW_ROWS", "PK_FEW_HEIGHT"))
PK_FEW_MIN, PK_FEW_MAX = geo.constant("PK_FEW_MIN"), geo.constant("PK_FEW_MAX")
# launch_filter: at most so many workgroups of 4 waves, a row per wave: taller images loop
FILTER_GRID_ROWS = geo.constant("FILTER_ROWS_PER_BLOCK") * geo.constant("FILTER_BLOCKS_MAX")
# ---- the kernels' internals, as plain numbers (where they live: see SOURCE_LINES) ------------------------------------------------
PK_NW, PK_TILE_BYTES = 4, 128        # unfilter_pk_kernel: waves per workgroup, bytes of a row per phase
U_NW = 4                             # unfilter_kernel: waves per workgroup
BAND = 64                            # rows per band of unfilter_kernel; the ballot of `piece_start` looks at 64 rows per round
PACKED_ROW = 2048                    # filter_kernel: longest sub-byte scanline that goes through LDS
FAST_STEP = 1024                     # filter_row_fast: bytes of a row per step of the wave (64 lanes x 16)

# (file, line that must still be there): the table fails, instead of silently losing coverage, when one of them moves
SOURCE_LINES = [
    ("unfilter.hip", "#define SPNG_UNF_PK_NW 4"),
    ("unfilter.hip", "static constexpr int TB = 128, RING = 256;"),
    ("unfilter.hip", "return NW > 1 && next && (next == band || band_may_wait(NW, reach, per_band));"),    # the one pipeline of both kernels
    ("unfilter.hip", "band_pipeline<NW>(BandProgress<NW>{done, nph, 1u, wave, lane}, maxb, nta, begin, issue, commit, compute, store);"),
    ("unfilter.hip", "band_pipeline<NW>(BandProgress<NW>{done, ntiles, (uint32_t)C::K, wave, lane}, nbands, ntiles, begin, issue, commit, compute, store);"),
    ("unfilter.hip", "#define SPNG_UNF_NW 4"),
    ("unfilter.hip", "#define SPNG_UNF_P4 64"),
    ("unfilter.hip", "#define SPNG_UNF_PSUB 16"),
    ("unfilter.hip", "#define SPNG_UNF_P8 32"),
    ("unfilter.hip", "const uint32_t ntiles = (W + 63 + C::P - 1) / C::P;"),
    ("unfilter.hip", "__device__ __forceinline__ uint32_t piece_start(const UnfJob &job, uint32_t rows, int lane, uint64_t x)"),
    ("unfilter.hip", "for (uint64_t r0 = x; r0 < rows; r0 += 64) {"),
    ("unfilter.hip", "const unsigned long long m = __ballot(r < rows && ft <= 1);"),
    ("encode.hip", "static constexpr uint32_t PACKED_ROW = 2048;"),
    ("encode.hip", "if (volume < 8 && job.pitch <= PACKED_ROW) {"),
    ("encode.hip", "const bool fast = direct && (job.pitch & 15) == 0 && bpp != 5 && bpp != 7;"),
    ("encode.hip", "const uint32_t steps = pitch / 1024 + (pitch % 1024 ? 1 : 0);"),
    ("encode.hip", "for (uint32_t y = blockIdx.x * 4 + wave; y < job.sub_h; y += gridDim.x * 4) {"),
]

FORMATS = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (8, 2), (16, 2), (8, 3), (16, 3), (8, 4), (16, 4)]
REGIMES = ("mixed", "up", "average", "paeth", "rare", "nocut")
ADAM7 = [(0, 0, 3, 3), (4, 0, 3, 3), (0, 4, 2, 3), (2, 0, 2, 2), (0, 2, 1, 2), (1, 0, 1, 1), (0, 1, 0, 1)]


@dataclass(frozen=True)
class Case:
    name: str
    width: int
    height: int
    depth: int
    channels: int
    interlaced: bool = False
    content: str = "noise"           # noise | synth | zebra (noise rows alternating with all-zero rows)
    regime: str = "mixed"            # unfilter cases: how the filter-type bytes are chosen (REGIMES)
    kernel: str = ""                 # claimed: the kernel `launch_unfilter` picks / the path of `filter_kernel`
    branch: str = ""                 # claimed: the rule of `unfilter_pieces` that sets the piece length

    @property
    def volume(self):
        return self.depth * self.channels

    @property
    def bpp(self):
        return (self.volume + 7) >> 3

    @property
    def fmt(self):
        return (self.width, self.height, self.depth, self.channels, self.interlaced)


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


def passes(c: Case):
    """[(scanline bytes without the filter byte, rows, pixels per row)] of the image or of its Adam7 sub-images that are not empty"""
    if not c.interlaced:
        return [((c.width * c.volume + 7) >> 3, c.height, c.width)]
    out = []
    for bx, by, ex, ey in ADAM7:
        sw, sh = (c.width + (1 << ex) - bx - 1) >> ex, (c.height + (1 << ey) - by - 1) >> ey
        if sw > 0 and sh > 0:
            out.append(((sw * c.volume + 7) >> 3, sh, sw))
    return out


def inflated_size(c: Case) -> int:
    return sum((p + 1) * h for p, h, _ in passes(c))


def storage_size(c: Case) -> int:
    return c.width * c.height * (1 if c.volume < 8 else c.volume >> 3)


def storage_row_bytes(c: Case) -> int:
    return c.width * (1 if c.volume < 8 else c.volume >> 3)


# ---- the dispatch, and mirrors of the kernels' internals -------------------------------------------------------------------------
def unfilter_plan(k: int, jobs, configured: int = 0):
    """`launch_plan` (csrc/host_decode.hip) + `launch_unfilter` (csrc/unfilter.hip) for the jobs [(pitch, rows)] of pixel size k of
    ONE call, by the functions of csrc/geometry.hpp those two call: -> (kernel, branch, rows per piece, pieces)"""
    widest = max(p for p, _ in jobs)
    piece, pieces, branch = geo.unfilter_pieces(k, sum(r for _, r in jobs), max([1] + [r for _, r in jobs]), widest, configured)
    if k in (4, 8):
        kernel = f"pk<{k}>"
    elif k in (1, 2):
        kernel = f"u<4,{k},32>" if geo.unfilter_wide_tiles(k, widest) else f"u<4,{k}>"
    else:
        kernel = f"u<{k}>"
    return kernel, branch, piece, pieces


def pk_may_block(pitch: int) -> bool:
    """unfilter_pk_kernel, nph phases per band and a reach of one: a wave that finishes a band may wait for the next band's first
    tile (`band_may_wait` of csrc/geometry.hpp, as the kernels' pipeline calls it)"""
    nph = (pitch + PK_TILE_BYTES - 1) // PK_TILE_BYTES + 1
    return geo.band_may_wait(PK_NW, 1, nph)


def u_tiles(k: int, pitch: int, wide: bool):
    """unfilter_kernel<...>: (K, tiles per row) -- `Cfg::P`, `Cfg::K`, `ntiles`.  k: pixel bytes (1, 2, 3, 6); wide: the batch's
    widest row has WIDE_ROW bytes or more (32-unit tiles for pixels of one and two bytes)"""
    unit = 4 if k in (1, 2) else k
    p = (32 if wide else 16) if k in (1, 2) else 64 if k == 3 else 32
    return (63 + p - 1) // p, ((pitch + unit - 1) // unit + 63 + p - 1) // p


def u_may_block(k: int, pitch: int, wide: bool) -> str:
    """unfilter_kernel, ntiles steps per band and a reach of K: a wave in its band's last tile may wait for the first tile of its next
    band (`band_may_wait` of csrc/geometry.hpp, as the kernels' pipeline calls it).
    -> "blocks", "gap" (the bound this one replaced, `NW * K + 1 < ntiles`, let it wait: rows on which the waves of a piece of more
    than NW bands waited for each other for good) or "never" """
    kk, nt = u_tiles(k, pitch, wide)
    if geo.band_may_wait(U_NW, kk, nt):
        return "blocks"
    return "gap" if U_NW * kk + 1 < nt else "never"


def filter_path(c: Case, pitch: int, whole: bool) -> str:
    """csrc/encode.hip `filter_kernel`: fast (16 bytes per lane), packed (sub-byte rows through LDS) or generic (`raw_byte`)"""
    if c.volume >= 8 and whole and pitch % 16 == 0:
        return "fast"
    if c.volume < 8 and pitch <= PACKED_ROW:
        return "packed"
    return "generic"


# ---- the filter-type bytes of the unfilter inputs ----------------------------------------------------------------------------------
def filter_types(regime: str, rows: int, rng) -> np.ndarray:
    if regime == "mixed":                               # all five, and a few invalid bytes (taken as None, PNG.Decoder.swift:193-194)
        t = rng.integers(0, 5, rows).astype(np.uint8)
        bad = rng.random(rows) < 0.02
        t[bad] = rng.integers(5, 256, int(bad.sum()))
        return t
    if regime in ("up", "average", "paeth"):            # one type alone under a Sub row: an error anywhere reaches the last row
        t = np.full(rows, {"up": 2, "average": 3, "paeth": 4}[regime], np.uint8)
        t[0] = 1
        return t
    t = rng.integers(2, 5, rows).astype(np.uint8)       # nocut: nothing after row 0 lets a piece start
    t[0] = 0
    if regime == "rare":                                # None / Sub rows more than 64 rows apart: `piece_start` takes several ballots
        r = int(rng.integers(70, 200))
        while r < rows:
            t[r] = rng.integers(0, 2)
            r += int(rng.integers(90, 400))
    else:
        assert regime == "nocut", regime
    return t


def unfilter_input(c: Case) -> np.ndarray:
    """the scanline stream of the case: noise under the regime's filter-type bytes (any payload is a valid input of the defilter)"""
    rng = np.random.default_rng(seed_of(c.name))
    rows = rng.integers(0, 256, inflated_size(c), dtype=np.uint8)
    off = 0
    for pitch, h, _ in passes(c):
        rows[off:off + (pitch + 1) * h:pitch + 1] = filter_types(c.regime, h, rng)
        off += (pitch + 1) * h
    return rows


def types_of(c: Case, rows) -> list:
    """the filter-type bytes of a scanline stream, one array per (sub-)image"""
    rows = np.frombuffer(rows, np.uint8) if isinstance(rows, (bytes, bytearray)) else rows
    out, off = [], 0
    for pitch, h, _ in passes(c):
        out.append(rows[off:off + (pitch + 1) * h:pitch + 1].copy())
        off += (pitch + 1) * h
    return out


def oracle_unfilter(c: Case, rows: np.ndarray, rows_len: int | None = None, into: np.ndarray | None = None):
    """-> (status, storage): the oracle's raster over a storage that held SENTINEL (or `into`, which is updated): the oracle
    assigns the pixels of the rows it has and touches nothing else (oracle/png_rows.c orc_unfilter)"""
    lib = ph.oracle()
    storage = into if into is not None else np.full(max(storage_size(c), 1), SENTINEL, np.uint8)
    rows = np.ascontiguousarray(rows)
    n = len(rows) if rows_len is None else rows_len
    st = lib.orc_unfilter(rows.ctypes.data_as(ctypes.c_void_p), n, c.width, c.height, c.depth, c.channels, int(c.interlaced),
                          storage.ctypes.data_as(ctypes.c_void_p))
    return st, storage[:storage_size(c)]


# ---- the rasters of the filter-select inputs ---------------------------------------------------------------------------------------
def filter_source(c: Case) -> np.ndarray:
    """PNG.Image.storage of the case (sub-byte samples one to a byte, unscaled), by content kind"""
    from swift_png_amd import synth
    rng = np.random.default_rng(seed_of(c.name))
    n, rowb = storage_size(c), storage_row_bytes(c)
    hi = (1 << c.depth) if c.depth < 8 else 256
    if c.content == "synth":
        if c.depth < 8:                                      # (synth.image makes whole bytes: the top bits of an 8-bit grey image)
            return (synth.image(seed_of(c.name) & 0xffff, c.width, c.height, 1, 8, tile=64) >> (8 - c.depth)).reshape(-1)
        return synth.image(seed_of(c.name) & 0xffff, c.width, c.height, c.channels, c.depth, tile=64).reshape(-1)
    img = rng.integers(0, hi, n, dtype=np.uint8).reshape(c.height, rowb)
    if c.content == "zebra":        # a noise row under a zero row: None ties with Up, Sub with Paeth, exactly (the first minimum wins)
        img[0::2] = 0
    else:
        assert c.content == "noise", c.content
    return img.reshape(-1)


def diff_report(name: str, got: np.ndarray, want: np.ndarray, row_bytes: int) -> str:
    """image, row and byte of the first and last difference"""
    if len(got) != len(want):
        return f"{name}: {len(got)} bytes, want {len(want)}"
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return ""
    a, b = int(bad[0]), int(bad[-1])
    return (f"{name}: {len(bad)} bytes differ; first row {a // row_bytes} byte {a % row_bytes} (got {got[a]:#x}, want {want[a]:#x}), "
            f"last row {b // row_bytes} byte {b % row_bytes}")


# ---- a. unfilter, one large image per launch path ----------------------------------------------------------------------------------
def _g(name, w, h, depth, ch, kernel, branch, interlaced=False):
    return Case(name, w, h, depth, ch, interlaced, "noise", "mixed", kernel, branch)


# every path of `launch_unfilter` x `unfilter_pieces` that one image can reach: these take all six regimes
PRIMARY = [
    _g("gray8 1500x1300", 1500, 1300, 8, 1, "u<4,1>", "floor128"),
    _g("indexed8 4096x2500", 4096, 2500, 8, 1, "u<4,1,32>", "wide"),
    _g("bit1 20000x1100", 20000, 1100, 1, 1, "u<4,1,32>", "wide"),
    _g("va8 900x1300", 900, 1300, 8, 2, "u<4,2>", "floor128"),
    _g("gray16 3000x1500", 3000, 1500, 16, 1, "u<4,2,32>", "wide"),
    _g("rgb8 600x2200", 600, 2200, 8, 3, "u<3>", "floor128"),
    _g("rgb8 1400x2200", 1400, 2200, 8, 3, "u<3>", "wide"),
    _g("rgb16 300x1300", 300, 1300, 16, 3, "u<6>", "floor128"),
    _g("rgb16 700x1300", 700, 1300, 16, 3, "u<6>", "wide"),
    _g("rgba8 200x900", 200, 900, 8, 4, "pk<4>", "rr"),
    _g("rgba8 200x1500", 200, 1500, 8, 4, "pk<4>", "few"),
    _g("rgba8 1000x900", 1000, 900, 8, 4, "pk<4>", "rr"),
    _g("rgba8 1000x2048", 1000, 2048, 8, 4, "pk<4>", "few"),
    _g("rgba16 500x1200", 500, 1200, 16, 4, "pk<8>", "rr"),
]
# the edges: rows of 2047 / 2048 / 2049 bytes for pixels of one byte and less (2046 / 2048 / 2050 for two-byte pixels, whose rows
# are even), sub-byte rows on both sides, the `2 NW + 1 < nph` edge of the line-aligned kernel: mixed and Paeth-only
SECONDARY = [
    _g("gray8 2047x600", 2047, 600, 8, 1, "u<4,1>", "floor128"),
    _g("gray8 2048x600", 2048, 600, 8, 1, "u<4,1,32>", "wide"),
    _g("gray8 2049x600", 2049, 600, 8, 1, "u<4,1,32>", "wide"),
    _g("bit1 8000x1100", 8000, 1100, 1, 1, "u<4,1>", "floor128"),
    _g("bit2 8192x700", 8192, 700, 2, 1, "u<4,1,32>", "wide"),
    _g("bit2 8193x700", 8193, 700, 2, 1, "u<4,1,32>", "wide"),
    _g("bit4 4094x700", 4094, 700, 4, 1, "u<4,1>", "floor128"),
    _g("va8 1023x600", 1023, 600, 8, 2, "u<4,2>", "floor128"),
    _g("va8 1024x600", 1024, 600, 8, 2, "u<4,2,32>", "wide"),
    _g("va8 1025x600", 1025, 600, 8, 2, "u<4,2,32>", "wide"),
    _g("va8 480x1300", 480, 1300, 8, 2, "u<4,2>", "floor128"),       # rows of the old `may_block` gap (u_may_block), with rgb16 300 and bit1 8000
    _g("rgb8 300x1300", 300, 1300, 8, 3, "u<3>", "floor128"),
    _g("gray8 1000x1300", 1000, 1300, 8, 1, "u<4,1>", "floor128"),
    _g("rgb8 200x700", 200, 700, 8, 3, "u<3>", "floor128"),          # and rows too short to wait on either bound
    _g("rgb16 100x700", 100, 700, 16, 3, "u<6>", "floor128"),
    _g("gray8 500x700", 500, 700, 8, 1, "u<4,1>", "floor128"),
    _g("va8 250x700", 250, 700, 8, 2, "u<4,2>", "floor128"),
    _g("va16 256x1100", 256, 1100, 16, 2, "pk<4>", "few"),
    _g("va16 257x1100", 257, 1100, 16, 2, "pk<4>", "few"),
    _g("rgba16 100x700", 100, 700, 16, 4, "pk<8>", "rr"),
]
# Adam7 at size: a sub-byte, a 3-byte and an 8-byte format (claims: of the largest sub-image's call -- one call holds all seven)
ADAM7_CASES = [
    _g("adam7 bit4 5000x1500", 5000, 1500, 4, 1, "u<4,1,32>", "wide", True),
    _g("adam7 rgb8 1500x1200", 1500, 1200, 8, 3, "u<3>", "wide", True),
    _g("adam7 rgba16 900x1100", 900, 1100, 16, 4, "pk<8>", "rr", True),
]


# the edge of `band_may_wait` for every kernel family, as tests/test_emu_unfilter.py has it ("N tiles", "N phases"): one type under a
# Sub row, so the image is one long piece of more bands than the workgroup has waves -- the last step count per band at which a wave
# never waits for its next band, and the first at which it may.  (name, steps per band, case)
def _e(name, steps, w, depth, ch, regime, kernel, branch):
    return steps, Case(f"edge {name} {w}x330 {regime}", w, 330, depth, ch, False, "noise", regime, kernel, branch)


BOUND_EDGE_CASES = [
    _e("rgb16", 13, 330, 16, 3, "paeth", "u<6>", "floor128"), _e("rgb16", 14, 360, 16, 3, "paeth", "u<6>", "wide"),
    _e("rgb8", 9, 460, 8, 3, "average", "u<3>", "floor128"), _e("rgb8", 10, 520, 8, 3, "up", "u<3>", "floor128"),
    _e("gray8", 21, 1040, 8, 1, "paeth", "u<4,1>", "floor128"), _e("va8", 22, 550, 8, 2, "paeth", "u<4,2>", "floor128"),
    _e("rgba8", 9, 256, 8, 4, "paeth", "pk<4>", "rr"), _e("rgba8", 10, 257, 8, 4, "paeth", "pk<4>", "rr"),
    _e("rgba16", 9, 128, 16, 4, "paeth", "pk<8>", "rr"), _e("rgba16", 10, 129, 16, 4, "paeth", "pk<8>", "rr"),
]


def band_steps(c: Case):
    """(waves, reach, steps per band) of the kernel that defilters the non-interlaced case: what `band_pipeline` is called with"""
    pitch = passes(c)[0][0]
    if c.bpp in (4, 8):
        return PK_NW, 1, (pitch + PK_TILE_BYTES - 1) // PK_TILE_BYTES + 1
    kk, nt = u_tiles(c.bpp, pitch, pitch >= WIDE_ROW)
    return U_NW, kk, nt


def unfilter_cases():
    out = []
    for g in PRIMARY:
        out += [replace(g, name=f"{g.name} {r}", regime=r) for r in REGIMES]
    for g in SECONDARY:
        out += [replace(g, name=f"{g.name} {r}", regime=r) for r in ("mixed", "paeth")]
    for g in ADAM7_CASES:
        out += [replace(g, name=f"{g.name} {r}", regime=r) for r in ("mixed", "rare")]
    return out


def case_plan(c: Case):
    """the plan of the call that defilters this image alone"""
    return unfilter_plan(c.bpp, [(p, h) for p, h, _ in passes(c)])


# short input at size (`rows_len`): a cut inside a row, exactly at a row's end, inside the last piece
SHORT_CASES = [g for g in PRIMARY if g.name in ("indexed8 4096x2500", "rgb8 1400x2200", "rgba8 1000x2048", "bit1 20000x1100")]


def short_lengths(c: Case):
    stride = passes(c)[0][0] + 1
    _, _, piece, pieces = case_plan(c)
    last_piece = (pieces - 1) * piece
    assert last_piece + 10 < c.height
    return [stride * 777 + stride // 3, stride * 1000, stride * (last_piece + 9) + 5, stride * c.height - 1]


# ---- b. one call, mixed batch ------------------------------------------------------------------------------------------------------
BATCH_WIDTHS_BYTES = [1, 2, 3, 5, 16, 17, 63, 64, 65, 127, 200, 257, 511, 777, 1000, 1024, 1500, 2047, 2048, 2100, 4100, 31]
BATCH_HEIGHTS = [1, 2, 63, 64, 65, 129, 300, 1025, 5, 1300, 33, 127, 1, 7, 500, 1100, 90, 64, 200, 3, 70, 1500]
BATCH_FORMATS = {1: [(8, 1), (8, 1), (8, 1), (1, 1), (2, 1), (4, 1)], 2: [(8, 2), (16, 1)], 3: [(8, 3)], 4: [(8, 4), (16, 2)],
                 6: [(16, 3)], 8: [(16, 4)]}


def batch_cases(k: int):
    """images of pixel size k for ONE unfilter_batch: rows of 1 byte ... more than 2048, 1 row ... more than 1024"""
    out = []
    fmts = BATCH_FORMATS[k]
    for i, (wb, h) in enumerate(zip(BATCH_WIDTHS_BYTES, BATCH_HEIGHTS)):
        depth, ch = fmts[i % len(fmts)]
        w = max(1, wb * 8 // (depth * ch))
        regime = ("mixed", "mixed", "rare", "paeth", "nocut")[i % 5]
        out.append(Case(f"batch k={k} #{i} {w}x{h} d{depth}c{ch} {regime}", w, h, depth, ch, False, "noise", regime))
    return out


def batch_plan(k: int, cases):
    return unfilter_plan(k, [(p, h) for c in cases for p, h, _ in passes(c)])


# total rows > 128 * 4096: the `total_rows / PIECE_SCALE_ROWS` term of `unfilter_pieces` exceeds the 128-row floor.  Many narrow tall images.
def scaled_batch_cases():
    return [Case(f"scaled #{i} 16x1800 gray8", 16, 1800, 8, 1, False, "noise", ("mixed", "rare", "average")[i % 3]) for i in range(300)]


# the 256 .. 1024-row branch beyond its floor: `widest` is taken over the call, so ONE row of 2048 bytes puts many narrow tall
# images on it -- more than 256 * 2048 rows for the `total_rows / 2048` term, more than 1024 * 2048 for the ceiling
def wide_batch_cases(ceiling: bool):
    n = 1200 if ceiling else 300
    tag = "ceiling" if ceiling else "term"
    out = [Case(f"wide {tag} #{i} 16x1800 gray8", 16, 1800, 8, 1, False, "noise", ("mixed", "rare", "paeth")[i % 3]) for i in range(n)]
    return out + [Case(f"wide {tag} the wide one 2048x1300 gray8", 2048, 1300, 8, 1, False, "noise", "rare")]


# the two-rounds-of-workgroups floor of the line-aligned kernels (`floor4`): many images below 1024 rows
def floor4_batch_cases(k: int):
    depth, ch, w = ((8, 4, 64) if k == 4 else (16, 4, 32))
    return [Case(f"floor4 k={k} #{i} {w}x800", w, 800, depth, ch, False, "noise", ("mixed", "rare", "paeth")[i % 3]) for i in range(128)]


# ---- c. the piece-rows knob --------------------------------------------------------------------------------------------------------
KNOB_CASES = [g for g in PRIMARY if g.name in ("indexed8 4096x2500", "va8 900x1300", "rgb8 1400x2200", "rgb16 700x1300",
                                               "rgba8 1000x2048", "rgba16 500x1200")]
KNOB_VALUES = [8, 24, 100, 512, 5000]               # 24 and 100: no multiple of a band; 5000: more rows than any of the images has


# ---- d. rows that arrive in pieces -------------------------------------------------------------------------------------------------
RESUME_CASES = [
    _g("resume indexed8 4096x2500", 4096, 2500, 8, 1, "u<4,1,32>", "wide"),
    _g("resume rgb8 1400x2200", 1400, 2200, 8, 3, "u<3>", "wide"),
    _g("resume rgba8 1000x2048", 1000, 2048, 8, 4, "pk<4>", "few"),
    _g("resume rgba16 500x1200", 500, 1200, 16, 4, "pk<8>", "rr"),
    _g("resume adam7 rgb8 1500x1200", 1500, 1200, 8, 3, "u<3>", "wide", True),
    _g("resume bit2 8193x1300", 8193, 1300, 2, 1, "u<4,1,32>", "wide"),
]


def resume_pushes(c: Case):
    """the inflated byte counts after each push: less than a row, exactly one row, thousands of rows, ends inside rows"""
    stride = passes(c)[0][0] + 1
    u = inflated_size(c)
    marks = [stride // 3, stride, stride + 7, stride * 3 + stride // 2, stride * 130, stride * 131 + 1, stride * 131 + stride - 1,
             stride * 1150 + 11, u - stride - 1, u - 1, u]
    out = []
    for m in marks:
        if m <= u and (not out or m > out[-1]):
            out.append(m)
    return out


# ---- e. filter-select --------------------------------------------------------------------------------------------------------------
FAST_PITCH = 2064                    # a multiple of 16 and of every pixel size, three 1 KiB steps
CONTENTS = ("noise", "synth", "zebra")


def filter_cases():
    out = []
    for depth, ch in FORMATS:
        vol = depth * ch
        if vol >= 8:
            widths = [(FAST_PITCH * 8 // vol, "fast"), (FAST_PITCH * 8 // vol + 1, "generic")]
        else:                           # sub-byte: a row of exactly PACKED_ROW bytes (LDS) and one of PACKED_ROW + 1 (`raw_byte`)
            widths = [(PACKED_ROW * 8 // vol, "packed"), (PACKED_ROW * 8 // vol + 1, "generic")]
        for w, path in widths:
            for content in CONTENTS:
                out.append(Case(f"filter d{depth}c{ch} {w}x260 {content}", w, 260, depth, ch, False, content, "", path))
    # taller than the grid of `launch_filter`: the rows from FILTER_GRID_ROWS on come in the second round of the grid-stride loop
    out.append(Case("filter tall rgba8 16x16500 synth", 16, 16500, 8, 4, False, "synth", "", "fast"))
    out.append(Case("filter tall bit1 100x16500 noise", 100, 16500, 1, 1, False, "noise", "", "packed"))
    out.append(Case("filter tall rgb8 21x16400 zebra", 21, 16400, 8, 3, False, "zebra", "", "generic"))
    # Adam7 at size: the sub-images are gathered pixel by pixel (`raw_byte`), the sub-byte ones of short rows through LDS
    out.append(Case("filter adam7 bit2 3000x600 synth", 3000, 600, 2, 1, True, "synth", "", "packed"))
    out.append(Case("filter adam7 rgb8 700x500 synth", 700, 500, 8, 3, True, "synth", "", "generic"))
    out.append(Case("filter adam7 rgba16 400x400 noise", 400, 400, 16, 4, True, "noise", "", "generic"))
    out.append(Case("filter adam7 bit1 40000x64 zebra", 40000, 64, 1, 1, True, "zebra", "", "generic"))
    return out


def filter_batch_cases():
    """mixed formats for ONE filter_batch: every format at a row that is a multiple of 16 bytes and at one that is not"""
    out = []
    for i, (depth, ch) in enumerate(FORMATS):
        vol = depth * ch
        for j, pitch in enumerate((1040, 333)):
            w = pitch * 8 // vol + j
            h = 40 + 7 * i + j
            out.append(Case(f"fbatch #{2 * i + j} d{depth}c{ch} {w}x{h}", w, h, depth, ch, (2 * i + j) % 5 == 4,
                            CONTENTS[(i + j) % 3], ""))
    return out


# ---- the size of it all ------------------------------------------------------------------------------------------------------------
# Scanline plus storage bytes over every case of the table, each counted once.  The GPU tests hold one case (or one batch) on
# the device at a time: the largest is bit1 20000x1100 (22 MB of storage), the batches stay below 64 MB, so the device footprint
# of the whole file is far below a GiB.
TOTAL_BYTES_CAP = 3 << 30


def all_cases():
    out = unfilter_cases() + [c for _, c in BOUND_EDGE_CASES] + RESUME_CASES + filter_cases() + filter_batch_cases() + scaled_batch_cases()
    out += wide_batch_cases(False) + wide_batch_cases(True)
    for k in BATCH_FORMATS:
        out += batch_cases(k)
    for k in (4, 8):
        out += floor4_batch_cases(k)
    return out
