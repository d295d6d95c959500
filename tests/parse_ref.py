"""TEST INFRASTRUCTURE: the yardstick of the typed chunks (spng_parse_dir_batch): the twelve parsers of Sources/PNG/Parsing that are
not PNG.Text's or PNG.ColorProfile's, restated in plain Python with the reference's line numbers, and the rule by which
PNG.Image.decompress (PNG.Image.swift:298-400) and PNG.Metadata.push (PNG.Metadata.swift:151-246) hand them a header and a palette.

  a parser -> Answer(status, aux, count, k, v): what a spng_chunk_value holds beside its scope
  parse_file(chunks) -> ([Value], Parsed): the records of a file's chunks [(type, payload)] and its spng_parsed
"""
import struct
from collections import namedtuple

import metadata_ref as mr

DONE = 0
(E_HEADER_CHUNK_LENGTH, E_HEADER_PIXEL_FORMAT_CODE, E_HEADER_PIXEL_FORMAT, E_HEADER_COMPRESSION_METHOD, E_HEADER_FILTER, E_HEADER_INTERLACING,
 E_HEADER_SIZE, E_UNEXPECTED_PALETTE, E_PALETTE_CHUNK_LENGTH, E_PALETTE_COUNT, E_UNEXPECTED_TRANSPARENCY, E_TRANSPARENCY_CHUNK_LENGTH,
 E_TRANSPARENCY_SAMPLE, E_TRANSPARENCY_COUNT, E_BACKGROUND_CHUNK_LENGTH, E_BACKGROUND_SAMPLE, E_BACKGROUND_INDEX, E_HISTOGRAM_CHUNK_LENGTH,
 E_GAMMA_CHUNK_LENGTH, E_CHROMATICITY_CHUNK_LENGTH, E_RENDERING_CHUNK_LENGTH, E_RENDERING_CODE, E_SIGNIFICANT_BITS_CHUNK_LENGTH,
 E_SIGNIFICANT_BITS_PRECISION, E_PHYSICAL_CHUNK_LENGTH, E_PHYSICAL_UNIT, E_SUGGESTED_PALETTE_CHUNK_LENGTH, E_SUGGESTED_PALETTE_NAME,
 E_SUGGESTED_PALETTE_DATA_LENGTH, E_SUGGESTED_PALETTE_DEPTH, E_SUGGESTED_PALETTE_FREQUENCY, E_TIME_CHUNK_LENGTH, E_TIME) = range(128, 161)
ALL = tuple(range(128, 161))
NONE = 0xffffffff
SCOPE_NONE, SCOPE_PARSED, SCOPE_NO_HEADER, SCOPE_NO_PALETTE = 0, 1, 2, 3
PARSED_TYPES = (b"IHDR", b"PLTE", b"tRNS", b"bKGD", b"hIST", b"gAMA", b"cHRM", b"sRGB", b"sBIT", b"pHYs", b"tIME", b"sPLT")

Answer = namedtuple("Answer", "status aux count k v")
Value = namedtuple("Value", "status scope aux count k v")
Parsed = namedtuple("Parsed", "status index aux ihdr_index plte_index palette_count depth color ios interlaced")
# PNG.Format.Pixel.recognize(code:): (depth, colour type)
FORMATS = ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (8, 2), (16, 2), (1, 3), (2, 3), (4, 3), (8, 3), (8, 4), (16, 4), (8, 6), (16, 6))


def good(v=(), count=0, k=NONE):
    return Answer(DONE, (0, 0), count, k, tuple(v) + (0,) * (8 - len(v)))


def bad(status, a0, a1=0, k=NONE):
    return Answer(status, (a0, a1), 0, k, (0,) * 8)


def has_color(color):
    return color in (2, 3, 6)


def has_alpha(color):
    return color in (4, 6)


def header(data, ios):
    """PNG.Header.init(parsing:standard:), PNG.Header.swift:73-129"""
    if len(data) != 13:                                          # :75-79
        return bad(E_HEADER_CHUNK_LENGTH, len(data))
    x, y, depth, color, compression, filt, interlace = struct.unpack(">IIBBBBB", data)
    if (depth, color) not in FORMATS:                            # :81-85
        return bad(E_HEADER_PIXEL_FORMAT_CODE, depth, color)
    if ios and (depth, color) not in ((8, 2), (8, 6)):           # :88-95
        return bad(E_HEADER_PIXEL_FORMAT, depth, color)
    if compression != 0:                                         # :100-104
        return bad(E_HEADER_COMPRESSION_METHOD, compression)
    if filt != 0:                                                # :105-109
        return bad(E_HEADER_FILTER, filt)
    if interlace > 1:                                            # :111-119
        return bad(E_HEADER_INTERLACING, interlace)
    if not (x > 0 and y > 0):                                    # :124-128
        return bad(E_HEADER_SIZE, x, y)
    return good((x, y, depth, color, interlace))


def palette(data, depth, color):
    """PNG.Palette.init(parsing:pixel:), PNG.Palette.swift:54-81"""
    if not has_color(color):                                     # :56-60
        return bad(E_UNEXPECTED_PALETTE, depth, color)
    count, remainder = divmod(len(data), 3)
    if remainder:                                                # :62-67
        return bad(E_PALETTE_CHUNK_LENGTH, len(data))
    most = 1 << min(depth, 8)                                    # :70
    if not 1 <= count <= most:                                   # :71-75
        return bad(E_PALETTE_COUNT, count, most)
    return good(count=count)


def _samples(data, depth, color, e_length, e_sample):
    """the grey and rgb cases of PNG.Transparency.swift:130-162 and PNG.Background.swift:123-155"""
    n = 3 if has_color(color) else 1
    if len(data) != 2 * n:
        return bad(e_length, len(data), 2 * n)
    most = 0xffff >> (16 - depth)
    v = struct.unpack(">" + "H" * n, data)
    if any(c > most for c in v):
        return bad(e_sample, max(v), most)
    return good(v)


def transparency(data, depth, color, entries):
    """PNG.Transparency.init(parsing:pixel:palette:), PNG.Transparency.swift:126-180.  entries: of the palette, None without one"""
    if color in (4, 6):                                          # :177-178
        return bad(E_UNEXPECTED_TRANSPARENCY, depth, color)
    if color == 3:                                               # :164-175
        if entries is None:
            return None                                          # DecodingError.required(chunk: .PLTE, before: .tRNS)
        if len(data) > entries:
            return bad(E_TRANSPARENCY_COUNT, len(data), entries)
        return good(count=len(data))
    return _samples(data, depth, color, E_TRANSPARENCY_CHUNK_LENGTH, E_TRANSPARENCY_SAMPLE)


def background(data, depth, color, entries):
    """PNG.Background.init(parsing:pixel:palette:), PNG.Background.swift:119-176"""
    if color == 3:                                               # :157-174
        if entries is None:
            return None                                          # DecodingError.required(chunk: .PLTE, before: .bKGD)
        if len(data) != 1:
            return bad(E_BACKGROUND_CHUNK_LENGTH, len(data), 1)
        if not data[0] < entries:
            return bad(E_BACKGROUND_INDEX, data[0], entries - 1)
        return good((data[0],))
    return _samples(data, depth, color, E_BACKGROUND_CHUNK_LENGTH, E_BACKGROUND_SAMPLE)


def histogram(data, entries):
    """PNG.Histogram.init(parsing:palette:), PNG.Histogram.swift:49-61"""
    if len(data) != 2 * entries:                                 # :51-56
        return bad(E_HISTOGRAM_CHUNK_LENGTH, len(data), 2 * entries)
    return good(count=len(data) // 2)


def gamma(data):
    """PNG.Gamma.init(parsing:): 4 bytes, one big-endian UInt32"""
    return good(struct.unpack(">I", data)) if len(data) == 4 else bad(E_GAMMA_CHUNK_LENGTH, len(data))


def chromaticity(data):
    """PNG.Chromaticity.init(parsing:): 32 bytes, w r g b as (x, y) pairs of big-endian UInt32"""
    return good(struct.unpack(">8I", data)) if len(data) == 32 else bad(E_CHROMATICITY_CHUNK_LENGTH, len(data))


def rendering(data):
    """PNG.ColorRendering.init(parsing:): 1 byte, 0 ... 3"""
    if len(data) != 1:
        return bad(E_RENDERING_CHUNK_LENGTH, len(data))
    return good((data[0],)) if data[0] <= 3 else bad(E_RENDERING_CODE, data[0])


def significant_bits(data, depth, color):
    """PNG.SignificantBits.init(parsing:pixel:), PNG.SignificantBits.swift:60-110"""
    arity = (3 if has_color(color) else 1) + (1 if has_alpha(color) else 0)     # :62
    if len(data) != arity:                                       # :63-68
        return bad(E_SIGNIFICANT_BITS_CHUNK_LENGTH, len(data), arity)
    most = 8 if color == 3 else depth                            # :100-105
    for v in data:                                               # :106-109: in the order of the payload
        if not 1 <= v <= most:
            return bad(E_SIGNIFICANT_BITS_PRECISION, v, most)
    return good(tuple(data))


def physical(data):
    """PNG.PhysicalDimensions.init(parsing:): 9 bytes, x, y, a unit of 0 or 1"""
    if len(data) != 9:
        return bad(E_PHYSICAL_CHUNK_LENGTH, len(data))
    x, y, unit = struct.unpack(">IIB", data)
    return good((x, y, unit)) if unit <= 1 else bad(E_PHYSICAL_UNIT, unit)


def time_modified(data):
    """PNG.TimeModified.init(parsing:), PNG.TimeModified.swift:90-121"""
    if len(data) != 7:                                           # :92-96
        return bad(E_TIME_CHUNK_LENGTH, len(data))
    year, month, day, hour, minute, second = struct.unpack(">HBBBBB", data)
    if not (1 <= month <= 12 and 1 <= day <= 31 and hour <= 23 and minute <= 59 and second <= 60):      # :105-120
        return bad(E_TIME, year | month << 16 | day << 24, hour | minute << 8 | second << 16)
    return good((year, month, day, hour, minute, second))


def suggested_palette(data):
    """PNG.SuggestedPalette.init(parsing:), PNG.SuggestedPalette.swift:54-156"""
    k = data.find(b"\0")                                         # PNG.Text.name(parsing:), :58-61
    if k < 0:
        return bad(E_SUGGESTED_PALETTE_NAME, 0)
    if not mr.valid_name(data[:k]):
        return bad(E_SUGGESTED_PALETTE_NAME, 1, k=k)
    if not k + 1 < len(data):                                    # :63-67
        return bad(E_SUGGESTED_PALETTE_CHUNK_LENGTH, len(data), k + 2, k=k)
    nbytes, code = len(data) - k - 2, data[k + 1]
    if code not in (8, 16):                                      # :114-115: the switch looks at the depth before any length
        return bad(E_SUGGESTED_PALETTE_DEPTH, code, k=k)
    stride = 6 if code == 8 else 10
    if nbytes % stride:                                          # :73-77, 94-98
        return bad(E_SUGGESTED_PALETTE_DATA_LENGTH, nbytes, stride, k=k)
    previous = 0xffff                                            # descendingFrequency, :125-156
    for i in range(nbytes // stride):
        current, = struct.unpack_from(">H", data, k + 2 + i * stride + stride - 2)
        if current > previous:
            return bad(E_SUGGESTED_PALETTE_FREQUENCY, i, k=k)
        previous = current
    return good((code,), count=nbytes // stride, k=k)


def suggested_entries(data, answer):
    """the entries of a good sPLT: [(r, g, b, a, frequency)]"""
    fmt = ">BBBBH" if answer.v[0] == 8 else ">HHHHH"
    return [struct.unpack_from(fmt, data, answer.k + 2 + i * struct.calcsize(fmt)) for i in range(answer.count)]


def parse_file(chunks):
    """chunks: [(type, payload)], the entries of a file's directory.  The header is entry 0, or entry 1 behind CgBI (PNG.Image.swift:303-321);
    a chunk's palette is the first PLTE if it stands in front of the chunk and parsed (:339-355: a second one is a duplicate)"""
    none = Value(DONE, SCOPE_NONE, (0, 0), 0, NONE, (0,) * 8)
    values = [none] * len(chunks)
    kinds = [k for k, _ in chunks]
    ios = int(kinds[:1] == [b"CgBI"])
    at = ios
    depth = color = interlaced = 0
    ihdr_index = plte_index = NONE
    palette_count = 0
    if at < len(chunks) and kinds[at] == b"IHDR":
        ihdr_index = at
        a = header(chunks[at][1], ios)
        values[at] = Value(a.status, SCOPE_PARSED, *a[1:])
        if a.status == DONE:
            depth, color, interlaced = a.v[2], a.v[3], a.v[4]
    if b"PLTE" in kinds:
        plte_index = kinds.index(b"PLTE")
    for i, (kind, data) in enumerate(chunks):
        if i == ihdr_index or kind not in PARSED_TYPES:
            continue
        if not depth:
            values[i] = none._replace(scope=SCOPE_NO_HEADER)
            continue
        entries = palette_count if plte_index < i and palette_count else None
        if kind == b"IHDR":
            a = header(data, ios)
        elif kind == b"PLTE":
            a = palette(data, depth, color)
            if i == plte_index and a.status == DONE:
                palette_count = a.count
        elif kind == b"tRNS":
            a = transparency(data, depth, color, entries)
        elif kind == b"bKGD":
            a = background(data, depth, color, entries)
        elif kind == b"hIST":
            a = histogram(data, entries) if entries is not None else None
        elif kind == b"sBIT":
            a = significant_bits(data, depth, color)
        else:
            a = {b"gAMA": gamma, b"cHRM": chromaticity, b"sRGB": rendering, b"pHYs": physical, b"tIME": time_modified,
                 b"sPLT": suggested_palette}[kind](data)
        values[i] = none._replace(scope=SCOPE_NO_PALETTE) if a is None else Value(a.status, SCOPE_PARSED, *a[1:])
    first = next((i for i, v in enumerate(values) if v.status != DONE), None)
    summary = Parsed(DONE if first is None else values[first].status, NONE if first is None else first,
                     (0, 0) if first is None else values[first].aux, ihdr_index, plte_index, palette_count, depth, color, ios, interlaced)
    return values, summary


def chunks_of(data, count):
    """the first `count` chunks of the file `data` as [(type, payload)]"""
    return [(struct.pack(">I", e.type), data[e.offset:e.offset + e.length]) for e in mr.directory(data, count)]
