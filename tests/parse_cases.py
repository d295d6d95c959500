"""TEST INFRASTRUCTURE: the case table of the typed chunks (spng_parse_dir_batch): the smallest files on which its kernels can go wrong.
A case is a file, the room of its directory (None: all the file could need) and what its spng_parsed must say: None -- no record holds an
error -- or (index, status, (aux0, aux1)) of the first record in file order that does; `scopes`, where given, is the scope of every
record.  Each expectation is argued from the Swift source beside it; tests/test_parse_ref.py holds the yardstick (tests/parse_ref.py) to
them, tests/test_emu_parse.py and tests/test_gpu_parse.py hold the kernels to the yardstick."""
import struct
from collections import namedtuple

import metadata_cases as mc
import metadata_ref as mr
import parse_ref as pr
import pnghelp as ph
from metadata_cases import chunk, file_of

Case = namedtuple("Case", "name file cap expect scopes")
NO, P, NH, NP = pr.SCOPE_NONE, pr.SCOPE_PARSED, pr.SCOPE_NO_HEADER, pr.SCOPE_NO_PALETTE


def ihdr(depth, color, x=32, y=32, compression=0, filt=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", x, y, depth, color, compression, filt, interlace))


def png(head, *chunks):
    """a file whose first chunk is `head`; file_of is this with the IHDR of a 32 x 32 v8 image"""
    return mc.SIG + head + b"".join(chunks) + mc.IEND


def be16(*v):
    return struct.pack(">" + "H" * len(v), *v)


def splt(name, depth, freqs, tail=b""):
    """an sPLT payload: entries of 6 or 10 bytes whose last two are the frequency"""
    colour = b"\x11\x22\x33\x44" if depth == 8 else b"\x11\x11\x22\x22\x33\x33\x44\x44"
    return name + b"\0" + bytes([depth]) + b"".join(colour + struct.pack(">H", f) for f in freqs) + tail


def descending(n, top=60000):
    return [top - i for i in range(n)]


TIME = (2000, 1, 1, 0, 0, 0)


def time_of(**kw):
    t = dict(zip(("year", "month", "day", "hour", "minute", "second"), TIME), **kw)
    return struct.pack(">HBBBBB", *t.values()), (t["year"] | t["month"] << 16 | t["day"] << 24, t["hour"] | t["minute"] << 8 | t["second"] << 16)


def cases():
    out = []

    def add(name, file, expect=None, cap=None, scopes=None):
        out.append(Case(name, file, cap, expect, scopes))

    V8, RGB8 = ihdr(8, 0), ihdr(8, 2)
    # ---- IHDR: PNG.Header.swift:73-129, the guards in their order ----------------------------------------------------------------
    for n in (12, 14, 0):                                        # :75-79
        add(f"IHDR of {n} bytes", png(chunk(b"IHDR", bytes(n)), chunk(b"gAMA", bytes(4))), (0, pr.E_HEADER_CHUNK_LENGTH, (n, 0)), scopes=(P, NH, NO))
    for depth, color in ((8, 9), (3, 0), (16, 3), (4, 2), (0, 0), (1, 4), (32, 6)):      # :81-85; (8, 9) is ErrorHandling.swift:47-63's
        add(f"pixel format code ({depth}, {color})", png(ihdr(depth, color)), (0, pr.E_HEADER_PIXEL_FORMAT_CODE, (depth, color)))
    for depth, color in pr.FORMATS:
        add(f"pixel format ({depth}, {color})", png(ihdr(depth, color)))
    add("compression method 1", png(ihdr(8, 0, compression=1)), (0, pr.E_HEADER_COMPRESSION_METHOD, (1, 0)))      # :100-104
    add("filter 1", png(ihdr(8, 0, filt=1)), (0, pr.E_HEADER_FILTER, (1, 0)))                                   # :105-109
    add("interlacing 2", png(ihdr(8, 0, interlace=2)), (0, pr.E_HEADER_INTERLACING, (2, 0)))                    # :111-119
    add("interlacing 1", png(ihdr(8, 0, interlace=1)))
    add("size (0, 1)", png(ihdr(8, 0, x=0, y=1)), (0, pr.E_HEADER_SIZE, (0, 1)))                                # :124-128
    add("size (1, 0)", png(ihdr(8, 0, x=1, y=0)), (0, pr.E_HEADER_SIZE, (1, 0)))
    add("size (1, 1)", png(ihdr(8, 0, x=1, y=1)))
    add("size (2^32 - 1, 2^32 - 1)", png(ihdr(8, 0, x=0xffffffff, y=0xffffffff)))      # (Int is 64 bits wide: positive)
    # two bad fields: the earlier guard throws
    add("pixel format code and compression", png(ihdr(8, 9, compression=1)), (0, pr.E_HEADER_PIXEL_FORMAT_CODE, (8, 9)))
    add("compression and filter", png(ihdr(8, 0, compression=2, filt=3)), (0, pr.E_HEADER_COMPRESSION_METHOD, (2, 0)))
    add("filter and interlacing", png(ihdr(8, 0, filt=3, interlace=4)), (0, pr.E_HEADER_FILTER, (3, 0)))
    add("interlacing and size", png(ihdr(8, 0, interlace=4, x=0)), (0, pr.E_HEADER_INTERLACING, (4, 0)))
    add("length and everything else", png(chunk(b"IHDR", b"\xff" * 14)), (0, pr.E_HEADER_CHUNK_LENGTH, (14, 0)))
    # CgBI: the header is entry 1, and only rgb8 / rgba8 pass (:88-95)
    cgbi = chunk(b"CgBI", b"\x50\x00\x20\x02")
    add("CgBI with rgb8", png(cgbi, ihdr(8, 2), chunk(b"gAMA", bytes(4))), scopes=(NO, P, P, NO))
    add("CgBI with rgba8", png(cgbi, ihdr(8, 6)))
    add("CgBI with v8", png(cgbi, ihdr(8, 0), chunk(b"gAMA", bytes(4))), (1, pr.E_HEADER_PIXEL_FORMAT, (8, 0)), scopes=(NO, P, NH, NO))
    add("CgBI with rgb16", png(cgbi, ihdr(16, 2)), (1, pr.E_HEADER_PIXEL_FORMAT, (16, 2)))
    add("CgBI with a pixel format code", png(cgbi, ihdr(8, 9)), (1, pr.E_HEADER_PIXEL_FORMAT_CODE, (8, 9)))
    # ---- PLTE: PNG.Palette.swift:54-81 -------------------------------------------------------------------------------------------
    for depth in (1, 2, 4, 8):
        most = 1 << depth
        for count in (0, 1, most, most + 1):                     # :70-75: 1 ... 1 << min(depth, 8)
            ok = 1 <= count <= most
            add(f"PLTE of {count} at depth {depth}", png(ihdr(depth, 3), chunk(b"PLTE", bytes(3 * count))),
                None if ok else (1, pr.E_PALETTE_COUNT, (count, most)))
    for count in (256, 257):
        add(f"PLTE of {count} in rgb8", png(RGB8, chunk(b"PLTE", bytes(3 * count))), None if count == 256 else (1, pr.E_PALETTE_COUNT, (257, 256)))
    add("PLTE of 257 in rgba16", png(ihdr(16, 6), chunk(b"PLTE", bytes(3 * 257))), (1, pr.E_PALETTE_COUNT, (257, 256)))      # min(16, 8)
    for n in (5, 1, 4):                                          # :62-67
        add(f"PLTE of {n} bytes", png(ihdr(8, 3), chunk(b"PLTE", bytes(n))), (1, pr.E_PALETTE_CHUNK_LENGTH, (n, 0)))
    for depth, color in ((8, 0), (1, 0), (16, 4)):               # :56-60, in front of the length
        add(f"PLTE in ({depth}, {color})", png(ihdr(depth, color), chunk(b"PLTE", bytes(5))), (1, pr.E_UNEXPECTED_PALETTE, (depth, color)))
    # ---- tRNS and bKGD samples: PNG.Transparency.swift:130-162, PNG.Background.swift:123-155 ---------------------------------------
    for kind, e_len, e_sample in ((b"tRNS", pr.E_TRANSPARENCY_CHUNK_LENGTH, pr.E_TRANSPARENCY_SAMPLE),
                                  (b"bKGD", pr.E_BACKGROUND_CHUNK_LENGTH, pr.E_BACKGROUND_SAMPLE)):
        greys = [(d, 0) for d in (1, 2, 4, 8, 16)] + ([(8, 4), (16, 4)] if kind == b"bKGD" else [])
        for depth, color in greys:
            most = (1 << depth) - 1
            add(f"{kind.decode()} sample {most} in ({depth}, {color})", png(ihdr(depth, color), chunk(kind, be16(most))))
            if depth < 16:
                add(f"{kind.decode()} sample {most + 1} in ({depth}, {color})", png(ihdr(depth, color), chunk(kind, be16(most + 1))),
                    (1, e_sample, (most + 1, most)))
        add(f"{kind.decode()} sample 0xffff at depth 1", png(ihdr(1, 0), chunk(kind, be16(0xffff))), (1, e_sample, (0xffff, 1)))
        for n in (0, 1, 3):
            add(f"grey {kind.decode()} of {n} bytes", png(V8, chunk(kind, bytes(n))), (1, e_len, (n, 2)))
        colours = [(8, 2), (16, 2)] + ([(8, 6), (16, 6)] if kind == b"bKGD" else [])
        for depth, color in colours:
            most = (1 << depth) - 1
            add(f"{kind.decode()} samples at {most} in ({depth}, {color})", png(ihdr(depth, color), chunk(kind, be16(most, most, most))))
        for place in range(3):                                   # the bad sample first, in the middle, last
            v = [1, 2, 3]
            v[place] = 256
            add(f"rgb8 {kind.decode()} with 256 in place {place}", png(RGB8, chunk(kind, be16(*v))), (1, e_sample, (256, 255)))
        # the payload is max(r, g, b), not the first sample that is out of range
        add(f"rgb8 {kind.decode()} (256, 300, 7)", png(RGB8, chunk(kind, be16(256, 300, 7))), (1, e_sample, (300, 255)))
        add(f"rgb8 {kind.decode()} (0xffff, 256, 0xfffe)", png(RGB8, chunk(kind, be16(0xffff, 256, 0xfffe))), (1, e_sample, (0xffff, 255)))
        for n in (0, 2, 5, 7):
            add(f"rgb8 {kind.decode()} of {n} bytes", png(RGB8, chunk(kind, bytes(n))), (1, e_len, (n, 6)))
    for depth, color in ((8, 4), (16, 4), (8, 6), (16, 6)):      # PNG.Transparency.swift:177-178
        add(f"tRNS in ({depth}, {color})", png(ihdr(depth, color), chunk(b"tRNS", bytes(2))), (1, pr.E_UNEXPECTED_TRANSPARENCY, (depth, color)))
    # ---- the palette's dependants: indexed tRNS (:164-175), indexed bKGD (PNG.Background.swift:157-174), hIST (PNG.Histogram.swift:51-56) ----
    I2, P3 = ihdr(2, 3), chunk(b"PLTE", bytes(range(9)))
    for n in (0, 3, 4):
        add(f"{n} alphas for 3 entries", png(I2, P3, chunk(b"tRNS", bytes(n))), None if n <= 3 else (2, pr.E_TRANSPARENCY_COUNT, (4, 3)))
    for index in (2, 3, 255):
        add(f"bKGD index {index} of 3 entries", png(I2, P3, chunk(b"bKGD", bytes([index]))), None if index < 3 else (2, pr.E_BACKGROUND_INDEX, (index, 2)))
    for n in (0, 2):
        add(f"indexed bKGD of {n} bytes", png(I2, P3, chunk(b"bKGD", bytes(n))), (2, pr.E_BACKGROUND_CHUNK_LENGTH, (n, 1)))
    for n in (4, 6, 8, 0):
        add(f"hIST of {n} bytes for 3 entries", png(I2, P3, chunk(b"hIST", bytes(n))), None if n == 6 else (2, pr.E_HISTOGRAM_CHUNK_LENGTH, (n, 6)))
    add("hIST beside a suggested palette of rgb8", png(RGB8, chunk(b"PLTE", bytes(3 * 256)), chunk(b"hIST", bytes(512))))
    add("hIST of 510 bytes for 256 entries", png(RGB8, chunk(b"PLTE", bytes(3 * 256)), chunk(b"hIST", bytes(510))),
        (2, pr.E_HISTOGRAM_CHUNK_LENGTH, (510, 512)))
    # ---- the fixed lengths ----------------------------------------------------------------------------------------------------------
    for kind, want, status in ((b"gAMA", 4, pr.E_GAMMA_CHUNK_LENGTH), (b"cHRM", 32, pr.E_CHROMATICITY_CHUNK_LENGTH),
                               (b"sRGB", 1, pr.E_RENDERING_CHUNK_LENGTH), (b"pHYs", 9, pr.E_PHYSICAL_CHUNK_LENGTH),
                               (b"tIME", 7, pr.E_TIME_CHUNK_LENGTH)):
        for n in (want - 1, want + 1, 0):
            add(f"{kind.decode()} of {n} bytes", file_of(chunk(kind, b"\1" * n)), (1, status, (n, 0)))
    add("gAMA", file_of(chunk(b"gAMA", struct.pack(">I", 0xfedcba98))))
    add("cHRM", file_of(chunk(b"cHRM", struct.pack(">8I", *[0x01020304 * (j + 1) + 0xf0000000 for j in range(8)]))))
    for code in (0, 3, 4, 255):
        add(f"sRGB code {code}", file_of(chunk(b"sRGB", bytes([code]))), None if code <= 3 else (1, pr.E_RENDERING_CODE, (code, 0)))
    for unit in (0, 1, 2):
        add(f"pHYs unit {unit}", file_of(chunk(b"pHYs", struct.pack(">IIB", 0xffffffff, 2835, unit))), None if unit <= 1 else (1, pr.E_PHYSICAL_UNIT, (2, 0)))
    # ---- sBIT: PNG.SignificantBits.swift:60-110 --------------------------------------------------------------------------------------
    for depth, color, arity in ((4, 0, 1), (16, 0, 1), (8, 2, 3), (16, 2, 3), (2, 3, 3), (8, 4, 2), (8, 6, 4), (16, 6, 4)):
        most = 8 if color == 3 else depth                        # :100-105: an indexed image's is 8, not its depth
        head = ihdr(depth, color)
        add(f"sBIT all {most} in ({depth}, {color})", png(head, chunk(b"sBIT", bytes([most] * arity))))
        add(f"sBIT all 1 in ({depth}, {color})", png(head, chunk(b"sBIT", bytes([1] * arity))))
        for wrong in (0, most + 1):
            for place in sorted({0, arity - 1}):
                v = [1] * arity
                v[place] = wrong
                add(f"sBIT {wrong} in place {place} of ({depth}, {color})", png(head, chunk(b"sBIT", bytes(v))),
                    (1, pr.E_SIGNIFICANT_BITS_PRECISION, (wrong, most)))
        if arity > 1:                                            # :106-109: the first in payload order
            v = [1] * arity
            v[0], v[-1] = most + 1, 0
            add(f"sBIT {most + 1} first and 0 last in ({depth}, {color})", png(head, chunk(b"sBIT", bytes(v))), (1, pr.E_SIGNIFICANT_BITS_PRECISION, (most + 1, most)))
        for n in sorted({0, arity - 1, arity + 1}):
            add(f"sBIT of {n} bytes in ({depth}, {color})", png(head, chunk(b"sBIT", b"\xff" * n)), (1, pr.E_SIGNIFICANT_BITS_CHUNK_LENGTH, (n, arity)))
    # ---- tIME: PNG.TimeModified.swift:105-120 ---------------------------------------------------------------------------------------
    for field, values in (("year", (0, 65535)), ("month", (0, 1, 12, 13)), ("day", (0, 1, 31, 32)), ("hour", (0, 23, 24)), ("minute", (59, 60)),
                          ("second", (59, 60, 61)), ("minute", (255,))):
        lo, hi = {"year": (0, 65535), "month": (1, 12), "day": (1, 31), "hour": (0, 23), "minute": (0, 59), "second": (0, 60)}[field]
        for v in values:
            payload, aux = time_of(**{field: v})
            add(f"tIME {field} {v}", file_of(chunk(b"tIME", payload)), None if lo <= v <= hi else (1, pr.E_TIME, aux))
    payload, aux = time_of(year=65535, month=13, day=32, hour=24, minute=60, second=61)
    add("tIME with everything wrong", file_of(chunk(b"tIME", payload)), (1, pr.E_TIME, aux))
    # ---- sPLT: PNG.SuggestedPalette.swift:54-156 --------------------------------------------------------------------------------------
    for depth in (8, 16):
        stride = 6 if depth == 8 else 10
        for n in (0, 1, 63, 64, 65, 128, 129):
            add(f"sPLT {depth} of {n} entries", file_of(chunk(b"sPLT", splt(b"p", depth, descending(n)))))
        for at in (1, 63, 64, 65, 128):                          # the first ascent; 64: against the frequency the step in front left behind
            f = descending(129)
            f[at] = f[at - 1] + 1
            add(f"sPLT {depth} ascending at entry {at}", file_of(chunk(b"sPLT", splt(b"p", depth, f))), (1, pr.E_SUGGESTED_PALETTE_FREQUENCY, (at, 0)))
        f = descending(129)
        f[70], f[64] = 65000, f[63] + 1
        add(f"sPLT {depth} ascending at 64 and 70", file_of(chunk(b"sPLT", splt(b"p", depth, f))), (1, pr.E_SUGGESTED_PALETTE_FREQUENCY, (64, 0)))
        add(f"sPLT {depth} of equal frequencies", file_of(chunk(b"sPLT", splt(b"p", depth, [7] * 130))))       # :134, 145: current <= previous
        add(f"sPLT {depth} from 0xffff down", file_of(chunk(b"sPLT", splt(b"p", depth, [0xffff, 0xffff, 0]))))    # previous starts at UInt16.max (:128)
        add(f"sPLT {depth} 0, 0, 1", file_of(chunk(b"sPLT", splt(b"p", depth, [0, 0, 1]))), (1, pr.E_SUGGESTED_PALETTE_FREQUENCY, (2, 0)))
        for n in (79, 80, 81):
            add(f"sPLT {depth} with a name of {n}", file_of(chunk(b"sPLT", splt(b"n" * n, depth, [5, 4]))),
                None if n <= 80 else (1, pr.E_SUGGESTED_PALETTE_NAME, (1, 0)))
        for extra in (stride - 1, stride + 1, 1):                # :73-77, 94-98
            add(f"sPLT {depth} with {extra} bytes of data", file_of(chunk(b"sPLT", splt(b"p", depth, [], bytes(extra)))),
                (1, pr.E_SUGGESTED_PALETTE_DATA_LENGTH, (extra, stride)))
    for c in mc.head_cases():                                    # the same name(parsing:) and validate(name:) as a keyword
        if c.kind == b"tEXt" and c.status == mr.E_TEXT_KEYWORD:
            add(f"sPLT named as: {c.name}", file_of(chunk(b"sPLT", c.payload)), (1, pr.E_SUGGESTED_PALETTE_NAME, (c.claim, 0)))
    add("sPLT with nothing behind its name", file_of(chunk(b"sPLT", b"name\0")), (1, pr.E_SUGGESTED_PALETTE_CHUNK_LENGTH, (5, 6)))     # :63-67
    add("sPLT with a depth and no entry", file_of(chunk(b"sPLT", b"name\0\x08")))
    for code in (0, 9, 15, 17):                                  # :114-115: the switch is on the depth, the length is looked at inside it
        add(f"sPLT with depth {code} and 5 bytes", file_of(chunk(b"sPLT", b"name\0" + bytes([code]) + bytes(5))), (1, pr.E_SUGGESTED_PALETTE_DEPTH, (code, 0)))
    f = [9] * 70000
    f[-1] = 10
    add("sPLT of 70 000 entries ascending at the last", file_of(chunk(b"sPLT", splt(b"big", 8, f))), (1, pr.E_SUGGESTED_PALETTE_FREQUENCY, (69999, 0)))
    # ---- scope: which header, which palette ---------------------------------------------------------------------------------------------
    gama, bad_time = chunk(b"gAMA", bytes(4)), chunk(b"tIME", time_of(month=13)[0])
    t13 = time_of(month=13)[1]
    add("no IHDR first", mc.SIG + gama + V8 + bad_time + mc.IEND, scopes=(NH, NH, NH, NO))          # PNG.Image.swift:303-321: required(IHDR)
    add("no IHDR at all", mc.SIG + chunk(b"PLTE", bytes(5)) + mc.IEND, scopes=(NH, NO))
    add("a bad IHDR and a bad tIME", png(ihdr(8, 9), gama, chunk(b"PLTE", bytes(5)), bad_time, chunk(b"tEXt", b"k\0t")),
        (0, pr.E_HEADER_PIXEL_FORMAT_CODE, (8, 9)), scopes=(P, NH, NH, NH, NO, NO))
    add("a second IHDR", png(V8, ihdr(8, 9)), (1, pr.E_HEADER_PIXEL_FORMAT_CODE, (8, 9)), scopes=(P, P, NO))   # (on its own; a duplicate to the host)
    add("hIST, bKGD, tRNS in front of the PLTE", png(I2, chunk(b"hIST", bytes(6)), chunk(b"bKGD", b"\7"), chunk(b"tRNS", bytes(9)), P3),
        scopes=(P, NP, NP, NP, P, NO))                           # DecodingError.required(PLTE, before:): the host's
    add("hIST without a PLTE in v8", file_of(chunk(b"hIST", bytes(6))), scopes=(P, NP, NO))
    add("bKGD and tRNS of rgb8 in front of its PLTE", png(RGB8, chunk(b"bKGD", bytes(6)), chunk(b"tRNS", bytes(6)), P3), scopes=(P, P, P, P, NO))
    add("a bad PLTE, then tRNS and hIST", png(I2, chunk(b"PLTE", bytes(5)), chunk(b"tRNS", bytes(1)), chunk(b"hIST", bytes(2))),
        (1, pr.E_PALETTE_CHUNK_LENGTH, (5, 0)), scopes=(P, P, NP, NP, NO))
    two = png(I2, chunk(b"PLTE", bytes(6)), chunk(b"PLTE", bytes(12)), chunk(b"tRNS", bytes(3)), chunk(b"bKGD", b"\3"))
    add("two PLTEs: the first one rules", two, (3, pr.E_TRANSPARENCY_COUNT, (3, 2)), scopes=(P, P, P, P, P, NO))      # PNG.Image.swift:339-355
    add("a bad PLTE, then a good one", png(I2, chunk(b"PLTE", bytes(15)), chunk(b"PLTE", bytes(6)), chunk(b"tRNS", bytes(1))),
        (1, pr.E_PALETTE_COUNT, (5, 4)), scopes=(P, P, P, NP, NO))
    cut = png(I2, gama, P3, chunk(b"tRNS", bytes(4)), bad_time)
    add("cap in front of the PLTE", cut, None, cap=2, scopes=(P, P))
    add("cap behind the PLTE", cut, None, cap=3, scopes=(P, P, P))
    add("cap behind the tRNS", cut, (3, pr.E_TRANSPARENCY_COUNT, (4, 3)), cap=4, scopes=(P, P, P, P))
    add("cap of 1", cut, None, cap=1, scopes=(P,))
    add("cap of 0", cut, None, cap=0, scopes=())
    add("chunks behind IDAT", file_of(chunk(b"IDAT", b"x"), bad_time, chunk(b"sRGB", b"\4")), (2, pr.E_TIME, t13), scopes=(P, NO, P, P, NO))
    add("two bad chunks: the earlier one", file_of(chunk(b"sRGB", b"\4"), gama, bad_time), (1, pr.E_RENDERING_CODE, (4, 0)))
    add("two bad chunks, the other way round", file_of(bad_time, gama, chunk(b"sRGB", b"\4")), (1, pr.E_TIME, t13))
    add("a bad text head is not this call's", file_of(chunk(b"tEXt", b" k\0t"), chunk(b"iCCP", b"n"), bad_time), (3, pr.E_TIME, t13), scopes=(P, NO, NO, P, NO))
    # ---- payloads at every residue of 16 --------------------------------------------------------------------------------------------------
    chrm = chunk(b"cHRM", bytes(range(1, 33)))
    for r in range(16):
        add(f"payloads {r} bytes on", file_of(chunk(b"prIv", bytes(r)), chrm, chunk(b"pHYs", bytes(range(8)) + b"\1"),
                                             chunk(b"sPLT", splt(b"p", 16, [3, 2, 9])), bad_time), (4, pr.E_SUGGESTED_PALETTE_FREQUENCY, (2, 0)))
    return out


def golden_files():
    """every PNG under tests/golden outside invalid/: the reference's integration tests decode all of them"""
    return sorted(p for p in ph.GOLDEN.rglob("*.png") if "invalid" not in p.parts)
