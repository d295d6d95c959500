"""Checksums at their arithmetic limits: the table shared by its own CPU check (tests/test_checksum_cases.py), the emulators
(tests/test_checksum_cases.py, tests/test_emu_gzip.py) and the device tests (tests/test_gpu_checksum_cases.py).  Importable without a
GPU; nothing is read from disk; every random byte comes from a seed that is a stable function of the case's name (seed_of).

Adler-32 is computed in nine places, each in the closed form s1 = 1 + S, s2 = N + N S - I (mod 65521) with S = sum b_i and
I = sum i b_i, each with 32-bit partial sums of its own.  Only byte VALUES and POSITIONS reach the bounds of those sums, so the payloads
here are all-0xFF, near-0xFF noise, a single 0xFF on the positions around a multiple of 65521, lengths that are 0 and +-1 modulo 65521,
and sums whose halves are 0.  What a stream must answer comes from Python's zlib / gzip, the oracle and oracle/gzip_wrap.py, never from
the code under test; every comparison is exact.

The MIRRORS restate, in unbounded Python integers, the additions and products an accumulator sees between two reductions and return
the PEAK a payload drives it to; tests/test_checksum_cases.py compares each peak with the worst case the source's comment names and with
2^32.  SOURCE_LINES pins the lines the mirrors restate.

The gzip header table (header_rows) is at the end: its expectation is oracle/gzip_wrap.py's read_header."""
from __future__ import annotations

import functools
import gzip
import zlib
from dataclasses import dataclass

import numpy as np

import pnghelp as ph
from test_oracle_gzip import gw, raw_deflate

ZLIB, RAW, GZIP = 0, 1, 2              # spng.FORMAT_ZLIB, FORMAT_IOS, FORMAT_GZIP
DONE, NEED_MORE_INPUT, E_STREAM_CHECKSUM = 0, 1, 32
MOD = 65521
BASE_N = 4 * MOD + 37                  # 262121: four turns of the modulus and a ragged end
TOTAL_BYTES_CAP = 8 << 20              # payload bytes of the whole table
GZ_PIECES = 256                        # csrc/gzip.hip
CRC_WAVE_THRESHOLD = 1024              # csrc/crc32.hpp, wave_crc32: `if (n > 1024)` picks the piece length of a lane

# (file, line that must still be there): the table fails, instead of silently losing coverage, when one of them moves
SOURCE_LINES = [
    ("inflate.hip", "uint32_t g = o.base + off;                         // < 65521 + 4096"),
    ("inflate.hip", "g = g >= 65521 ? g - 65521 : g;"),
    ("inflate.hip", "o.accS += A;                                       // <= 4080 per piece"),
    ("inflate.hip", "o.accI = (o.accI + g * A + J) % 65521;             // 65520*4080 + 30600 + 65520 < 2^32"),
    ("inflate.hip", "o.accS %= 65521;"),
    ("inflate.hip", "static constexpr int FLUSH = 4096;           // flush granularity"),
    ("pinflate2.hip", "// (position of the unit mod 65521, from the tile's: 32-bit arithmetic; g * A < 2^29)"),
    ("pinflate2.hip", "const uint32_t g = (pmod + 65521u - ((uint32_t)pos & 15u) + 16u * (uint32_t)(u - u0)) % 65521u;"),
    ("pinflate2.hip", "accS = (accS + A) % 65521u;"),
    ("pinflate2.hip", "accI = (accI + g * A + J) % 65521u;"),
    ("pinflate2.hip", "accI = (uint32_t)((accI + (uint64_t)g * b) % 65521);"),
    ("pinflate2.hip", "// (64-bit sums without reduction: a part is far below 2^40 bytes)"),
    ("deflate.hip", "accI += pm * byte;"),
    ("deflate.hip", "pm = pm + 64 >= 65521 ? pm + 64 - 65521 : pm + 64;"),
    ("deflate.hip", "accI %= 65521;                                     // (four products < 2^24 each on top of a reduced sum)"),
    ("deflate.hip", "for (uint32_t k = 0; k < n; ++k) { const uint32_t v = in[k]; emit(v); S += v; I += k * v; }"),
    ("deflate.hip", "if (lane == 0) { atomicAdd(adlerS, S % 65521); atomicAdd(adlerI, I % 65521); }"),
    ("gzip.hip", "static constexpr uint32_t GZ_PIECES = 256;"),
    ("gzip.hip", "__device__ __forceinline__ uint64_t piece_len(uint64_t n) { return (n + GZ_PIECES - 1) / GZ_PIECES; }"),
    ("gzip.hip", "I = (I + g * b) % 65521;"),
    ("gzip.hip", "g += 64; g = g >= 65521 ? g - 65521 : g;"),
    ("gzip.hip", "acc = multmodp(m == len ? whole : xpow8(m), acc) ^ part[k];"),
    ("gzip.hip", "for (int k = 0; k < 2 && status == SPNG_DONE; ++k) {   // FNAME, FCOMMENT"),
    ("gzip.hip", "if (!(flags & (k ? 0x10 : 0x08))) continue;"),
    ("crc32.hpp", "if (n > 1024) k = 64 - (uint32_t)__builtin_clzll((unsigned long long)((n - 1) >> 6));     // smallest k with 2^k * 64 >= n"),
]


def seed_of(name: str) -> int:
    return zlib.crc32(("checksum_cases/" + name).encode())


# ---- payloads ------------------------------------------------------------------------------------------------------------------------

ONEHOT_P = [0, 15, 16, 65519, 65520, 65521, 65522, 131041, 131042, 131043, BASE_N - 1]
N_ZERO = [65520, 65521, 65522, 131042]
GZ_N = [1, 255, 256, 257, 511, 512, 513, 256 * 16 - 1, 256 * 16, 256 * 16 + 1, 65535, 65537,
        256 * CRC_WAVE_THRESHOLD + 1]   # (added: the only length whose pieces, 1025 bytes, lie behind wave_crc32's threshold)
S2_ZERO_LEN = 600
S2_ZERO_FOUND = (64, 114)               # the first (byte 0, byte 1), in that order of search, that makes the high half 0: see _s2_zero


def high(name: str, n: int) -> bytes:
    """uniform random in 0xF0 .. 0xFF: near the maximum of every sum, and no single run"""
    return np.random.default_rng(seed_of(name)).integers(0xF0, 0x100, n, dtype=np.uint8).tobytes()


def adler_parts(data: bytes):
    """(S, I) of the closed form, in unbounded integers"""
    a = np.frombuffer(data, np.uint8).astype(object)
    return int(a.sum()) if len(data) else 0, int((a * np.arange(len(data), dtype=object)).sum()) if len(data) else 0


def closed_form(S: int, I: int, n: int) -> int:
    return ((n + n * S - I) % MOD) << 16 | (1 + S) % MOD


def _s2_zero():
    """600 bytes of `high` whose first two bytes are replaced by the first pair (a, b), a ascending then b, for which
    s2 = N + N S - I is 0 modulo 65521: byte 0 weighs N in s2 and byte 1 weighs N - 1.  Deterministic: the seed is seed_of("s2-zero")."""
    d = bytearray(high("s2-zero", S2_ZERO_LEN))
    d[0] = d[1] = 0
    base = zlib.adler32(bytes(d)) >> 16
    for a in range(256):
        for b in range(256):
            if (base + S2_ZERO_LEN * a + (S2_ZERO_LEN - 1) * b) % MOD == 0:
                d[0], d[1] = a, b
                return bytes(d), (a, b)
    raise AssertionError("no pair")


@functools.lru_cache(maxsize=None)
def payload(name: str) -> bytes:
    if name == "ff":
        return b"\xff" * BASE_N
    if name == "high":
        return high(name, BASE_N)
    kind, _, arg = name.partition("-")
    if name == PARTS7:
        return high(name, PARTS7_N)
    if kind == "onehot":
        d = bytearray(BASE_N)
        d[int(arg)] = 0xFF
        return bytes(d)
    if kind == "n" and arg.startswith("zero-"):
        return high(name, int(arg[5:]))
    if name == "s1-zero":
        return b"\xff" * 256 + bytes([240])
    if name == "s2-zero":
        return _s2_zero()[0]
    if kind == "tiny":
        return b"\xff" * int(arg)
    if kind == "gz":
        return high(name, int(arg))
    raise KeyError(name)


# Seven parts.  pinf2_scan_kernel (scan_stream, "the parts") begins part t at the first chain segment that starts a block, lies behind the
# first 32 KiB and at or behind t / pmax of the output: seven parts need a block start in every seventh of the output.  zlib's level-6
# blocks of `high` hold about 43.7 KB of output and the oracle's greedy / lazy levels cap a block at 32767 terms, so a seventh must be
# about 44 KB: 262121 bytes give six parts at most, the next length of the table's form, five turns + 37, gives seven.  (The oracle's
# level 9 doubles its blocks up to 2^21 terms -- the last block is half the stream, and no length of megabytes gives it seven
# parts --, so this payload's swift-png-shaped stream is the oracle's level 7.)  Not in PAYLOADS: it exists for the part counts alone.
PARTS7_N = 5 * MOD + 37
PARTS7 = "high-%d" % PARTS7_N

ONEHOTS = ["onehot-%d" % p for p in ONEHOT_P]
N_ZEROS = ["n-zero-%d" % n for n in N_ZERO]
TINY = ["tiny-%d" % n for n in range(4)]
GZ = ["gz-%d" % n for n in GZ_N]
ADLER_PAYLOADS = ["ff", "high"] + ONEHOTS + N_ZEROS + ["s1-zero", "s2-zero"] + TINY     # what the deflate side takes, and inflate
PAYLOADS = ADLER_PAYLOADS + GZ


def onehot_expected(p: int, n: int = BASE_N) -> int:
    """Adler-32 of n zeros with one 0xFF at p, in two lines of integer arithmetic: every byte from p on adds 255 to s2"""
    s1 = (1 + 255) % MOD
    return ((n + 255 * (n - p)) % MOD) << 16 | s1


# ---- gzip's 256 pieces ---------------------------------------------------------------------------------------------------------------

def piece_len(n: int) -> int:
    """csrc/gzip.hip, restated"""
    return (n + GZ_PIECES - 1) // GZ_PIECES


def piece_shape(n: int):
    """-> (piece length, full pieces, bytes of the short piece or 0, empty pieces behind the end)"""
    ln = piece_len(n)
    if not ln:
        return 0, 0, 0, GZ_PIECES
    full, short = divmod(n, ln)
    return ln, full, short, GZ_PIECES - full - (1 if short else 0)


# ---- mirrors: the peak of each 32-bit accumulation between two reductions -------------------------------------------------------------

def _units(data: bytes):
    """A = sum b_j and J = sum j b_j of every 16-byte unit of the stream (the last one padded with zeros), and g = 16 k mod 65521"""
    a = np.frombuffer(data + bytes(-len(data) % 16), np.uint8).astype(np.int64).reshape(-1, 16)
    return a.sum(1), (a * np.arange(16)).sum(1), (np.arange(len(a), dtype=np.int64) * 16) % MOD


def unit_peak(data: bytes) -> int:
    """inflate.hip `flush` and pinflate2.hip's tile loop: `accI + g * A + J` per 16-byte unit at stream offset g (mod 65521), accI
    reduced in front of it.  Units lie on multiples of 16 of the STREAM position in both (flush: `flushed` starts at out_pos & ~15
    and grows by whole flushes; resolve: u << 4), whatever the destination's alignment.  -> the peak of g * A + J; on top of it stands
    a reduced accI of at most 65520."""
    if not data:
        return 0
    A, J, g = _units(data)
    return int((g * A + J).max())


UNIT_WORST = 65520 * 4080 + 30600      # the comment of `flush`: g = 65520, sixteen 0xFF
UNIT_RESOLVE_CLAIM = 1 << 29           # pinflate2.hip: "g * A < 2^29"


def flush_accS_peak(data: bytes) -> int:
    """inflate.hip: `o.accS += A` for every unit of a lane within one flush of FLUSH = 4096 bytes -- 64 lanes x 16 bytes x 4 rounds --,
    reduced behind the flush: at most 4 units on top of 65520"""
    if not data:
        return 0
    A = _units(data)[0]
    return 65520 + int(np.sort(A)[-4:].sum())


def tail_peak(data: bytes) -> int:
    """pinflate2.hip, the bytes behind the last whole unit: `(uint64_t)g * b` in 64 bits, reduced to 32: the peak of accI + g * b"""
    n = len(data)
    return max([65520 + (i % MOD) * data[i] for i in range(n - n % 16, n)], default=0)


def insert_peak(data: bytes, warm: int = 0) -> int:
    """deflate.hip, d3_insert / d3_insert_quad: a lane adds pm * byte for its position in each of the four batches of a quad of 256
    positions (pm: the position mod 65521), and the caller reduces accI once per quad.  Quads count from the chunk's first position
    `warm`.  -> the peak of the four products; on top of them stands a reduced accI of at most 65520."""
    if not data:
        return 0
    n = len(data)
    pos = np.arange(warm, warm + n, dtype=np.int64)
    prod = (pos % MOD) * np.frombuffer(data, np.uint8).astype(np.int64)
    prod = np.concatenate([prod, np.zeros(-n % 256, np.int64)]).reshape(-1, 4, 64)
    return int(prod.sum(1).max())


INSERT_CLAIM = 4 * ((1 << 24) - 1)      # "four products < 2^24 each"
# what four consecutive batches of one lane can reach: positions 64 apart, the last on 65520, every byte 0xFF
INSERT_WORST = 255 * (65520 + 65456 + 65392 + 65328)


def insert_accS_bound(positions_per_chunk: int) -> int:
    """deflate.hip: accS += byte is reduced only behind the chunk: a lane sees a 64th of its positions (+ one quad of slack)"""
    return (positions_per_chunk // 64 + 4) * 255


def resume_peak(data: bytes):
    """gzip.hip resume_adler_kernel: 256 pieces, a wave each, lane l takes the bytes from + l + 64 j; `I = (I + g * b) % 65521` per byte and
    `S += b` unreduced over the piece.  -> (peak of g * b, peak of a lane's S)"""
    n = len(data)
    if not n:
        return 0, 0
    a = np.frombuffer(data, np.uint8).astype(np.int64)
    peak_I = int(((np.arange(n, dtype=np.int64) % MOD) * a).max())
    ln, peak_S = piece_len(n), 0
    for k in range(GZ_PIECES):
        piece = a[k * ln:(k + 1) * ln]
        if len(piece):
            lanes = np.concatenate([piece, np.zeros(-len(piece) % 64, np.int64)]).reshape(-1, 64).sum(0)
            peak_S = max(peak_S, int(lanes.max()))
    return peak_I, peak_S


RESUME_WORST_I = 65520 * 255            # a 0xFF on a position that is 65520 modulo 65521
# `S += b` stays below 2^32 while a lane sees at most (2^32 - 1) / 255 bytes: pieces of up to 64 x that, 2^30 bytes and more
RESUME_PIECE_LIMIT = ((1 << 32) - 1) // 255 * 64


def stored_tail_peak(data: bytes):
    """deflate.hip stored_tail (n < 3): S += v, I += k * v, unreduced"""
    assert len(data) < 3
    return sum(data), sum(k * v for k, v in enumerate(data))


# ---- streams -------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Stream:
    name: str                          # <payload>/<encoder>/<format>[/flip]
    payload: str
    z: bytes
    fmt: int
    status: int                        # DONE or E_STREAM_CHECKSUM
    aux: tuple                         # (declared, computed) of a twin, else (0, 0)

    @property
    def data(self):
        return payload(self.payload)


def _raw6(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


ENCODERS = ("zlib6", "orc9")


def _flip(z: bytes, at: int, name: str) -> bytes:
    """one bit of the four checksum bytes at z[at:at + 4], chosen by the name"""
    bit = seed_of(name) % 32
    b = bytearray(z)
    b[at + bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def streams(pname: str):
    """every stream of a payload: zlib / raw / gzip from Python's zlib and gzip at level 6 and from the oracle's deflate at level 9 (a
    swift-png-shaped stream; PARTS7: level 7), and for every zlib and gzip stream a twin with one flipped bit in the checksum"""
    data = payload(pname)
    out = []
    lv = 7 if pname == PARTS7 else 9
    made = {"zlib6": {ZLIB: zlib.compress(data, 6), RAW: _raw6(data), GZIP: gzip.compress(data, 6, mtime=0)},
            "orc%d" % lv: {ZLIB: ph.orc_deflate(data, lv, ZLIB), RAW: ph.orc_deflate(data, lv, RAW), GZIP: gw.deflate(data, raw_deflate(lv))}}
    for enc, by_fmt in made.items():
        for fmt, z in by_fmt.items():
            name = "%s/%s/%s" % (pname, enc, ("zlib", "raw", "gzip")[fmt])
            out.append(Stream(name, pname, z, fmt, DONE, (0, 0)))
            if fmt == ZLIB:
                bad = _flip(z, len(z) - 4, name)
                out.append(Stream(name + "/flip", pname, bad, fmt, E_STREAM_CHECKSUM, (int.from_bytes(bad[-4:], "big"), zlib.adler32(data))))
            elif fmt == GZIP:
                bad = _flip(z, len(z) - 8, name)
                out.append(Stream(name + "/flip", pname, bad, fmt, E_STREAM_CHECKSUM, (int.from_bytes(bad[-8:-4], "little"), zlib.crc32(data))))
    return out


def splits(st: Stream) -> bool:
    """a stream the part plan must cut in two or more at segments of 256 bytes: 65520 bytes or more, compressed to 1024 or more"""
    return len(st.data) >= 65520 and len(st.z) >= 1024


def all_streams(names=None):
    return [s for p in (PAYLOADS if names is None else names) for s in streams(p)]


def body(st: Stream):
    """-> (the raw DEFLATE of a stream with the trailer behind it, as the kernels behind gzip.hip's header kernel see a gzip member;
    the format they see)"""
    if st.fmt == GZIP:
        status, _, off = gw.read_header(st.z)
        assert status == DONE
        return st.z[off:], RAW
    return st.z, st.fmt


# ---- deflate: what the device must write ---------------------------------------------------------------------------------------------

DEFLATE_LEVELS = [0, 1, 4, 7, 8, 9, 13]
DEFLATE_SHAPES = [(ZLIB, 15), (ZLIB, 8), (GZIP, 15), (GZIP, 8)]       # (format, window exponent)
# the payloads of the deflate side in three groups, so that a test of one level and one group takes a few seconds with the oracle's share
DEFLATE_GROUPS = {"values": ["ff", "high"] + N_ZEROS + ["s1-zero", "s2-zero"] + TINY, "onehot-a": ONEHOTS[:6], "onehot-b": ONEHOTS[6:]}


@functools.lru_cache(maxsize=None)
def deflate_expected(pname: str, level: int, fmt: int, exponent: int) -> bytes:
    """the oracle's stream, asked once.  A gzip member is oracle/gzip_wrap.py's envelope around the oracle's blocks; the oracle's raw
    format always takes the window of 2^15 (DeflatorBuffers.swift:52-55), so the blocks are taken from its zlib stream at the exponent
    asked for, between the two header bytes and the four of the Adler-32 (tests/test_checksum_cases.py holds that against
    gzip_wrap.deflate over the raw format at exponent 15)"""
    data = payload(pname)
    if fmt == GZIP:
        return gw.deflate(data, lambda _d: deflate_expected(pname, level, ZLIB, exponent)[2:-4])
    return ph.orc_deflate(data, level, fmt, exponent)


# ---- the gzip header table -----------------------------------------------------------------------------------------------------------

FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
H_EXTRA, H_NAME, H_COMMENT = b"extra", b"file.bin", b"a comment that is longer than the name"
H_DATA = b"gzip header table\n" * 8


def member(flags, extra=H_EXTRA, name=H_NAME, comment=H_COMMENT, method=8, sigil=(0x1f, 0x8b), data=H_DATA):
    """-> (a gzip member with the fields its flag bits announce, the length of its header)"""
    head = bytes([sigil[0], sigil[1], method, flags, 1, 2, 3, 4, 2, 3])
    if flags & FEXTRA:
        head += len(extra).to_bytes(2, "little") + extra
    if flags & FNAME:
        head += name + b"\0"
    if flags & FCOMMENT:
        head += comment + b"\0"
    return head + _raw6(data) + (zlib.crc32(data) & 0xffffffff).to_bytes(4, "little") + len(data).to_bytes(4, "little"), len(head)


ALL_FIELDS = FTEXT | FEXTRA | FNAME | FCOMMENT


@functools.lru_cache(maxsize=None)
def header_rows():
    """-> [(name, the bytes handed to the parser, well-formed: the whole member is there and Python's gzip module must read it)]"""
    rows = []
    for f in range(16):                                                          # all 16 combinations of the four fields
        flags = (f & 1) * FTEXT | (f >> 1 & 1) * FEXTRA | (f >> 2 & 1) * FNAME | (f >> 3 & 1) * FCOMMENT
        rows.append(("fields-%02x" % flags, member(flags)[0], True))
    rows.append(("xlen-0", member(FEXTRA | FNAME, extra=b"")[0], True))
    big = high("xlen-65535", 65535)                                              # (with two zeros: a zero inside FEXTRA ends no string)
    big = big[:100] + b"\0\0" + big[102:]
    m, h = member(FEXTRA | FNAME, extra=big)
    rows.append(("xlen-65535", m, True))
    for cut in (11, 12, 13, 12 + 65534, 12 + 65535, h - 1, h):
        rows.append(("xlen-65535-cut-%d" % cut, m[:cut], False))
    rows.append(("fname-empty", member(FNAME | FCOMMENT, name=b"")[0], True))
    rows.append(("fcomment-empty", member(FNAME | FCOMMENT, comment=b"")[0], True))
    rows.append(("fname-with-sigil", member(FNAME, name=b"a\x1f\x8b\x08b")[0], True))
    m, h = member(ALL_FIELDS)
    rows.append(("header-ends-the-source", m[:h], False))
    for cut in range(h + 2):                                                     # every prefix, from 0 bytes to the first payload byte
        rows.append(("prefix-%d" % cut, m[:cut], False))
    for bit in (0x20, 0x40, 0x80):                                               # the reserved flag bits, one at a time
        rows.append(("reserved-%02x" % bit, member(bit)[0], False))
        rows.append(("reserved-%02x-with-fields" % bit, member(bit | ALL_FIELDS)[0], False))
    rows.append(("fhcrc", member(FHCRC)[0], False))
    rows.append(("fhcrc-with-fields", member(FHCRC | ALL_FIELDS)[0], False))
    for method in (0, 7, 9):
        rows.append(("method-%d" % method, member(0, method=method)[0], False))
    rows.append(("sigil-0", member(0, sigil=(0x1e, 0x8b))[0], False))
    rows.append(("sigil-1", member(0, sigil=(0x1f, 0x8a))[0], False))
    rows.append(("method-before-flags", member(0xff, method=7)[0], False))          # (the order of the checks: sigil, method, flag bits, FHCRC)
    rows.append(("flags-before-fhcrc", member(0x22)[0], False))
    assert len({r[0] for r in rows}) == len(rows)
    return rows


# ---- where a stream that arrives in pieces is cut ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def push_cuts(st: Stream):
    """-> the source lengths of the pushes in front of the last: inside the header, on a block boundary (the byte in which a block in
    the middle of the stream begins; a stream of one block has none), one byte before the trailer, inside the trailer (gzip: inside
    the CRC-32 and inside ISIZE)"""
    import deflate_tokens as dt
    z, _ = body(st)
    off = len(st.z) - len(z)
    blocks = dt.read(z[:-8] if st.fmt == GZIP else z, raw=st.fmt != ZLIB)
    cuts = {1 if st.fmt == ZLIB else 5}
    if len(blocks) > 1:
        cuts.add(off + (blocks[len(blocks) // 2].first_bit + 7) // 8)
    cuts |= {len(st.z) - 5, len(st.z) - 2} if st.fmt == ZLIB else {len(st.z) - 9, len(st.z) - 6, len(st.z) - 2}
    return sorted(c for c in cuts if 0 < c < len(st.z))
