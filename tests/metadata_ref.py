"""TEST INFRASTRUCTURE: the yardsticks of the chunk directory and the text entry, plain Python restated from the reference.

  parse_head           PNG.Text.init(parsing:unicode:)       Sources/PNG/Parsing/PNG.Text.swift:110-200
                       name(parsing:) / validate(name:)      :202-251
                       language(parsing:) / validate(language:)   :254-301
                       PNG.ColorProfile.init(parsing:)       Sources/PNG/Parsing/PNG.ColorProfile.swift:51-85
                       -> the fields of a spng_chunk_entry's head (up to the inflator: the body is spng_inflate_batch's)
  directory            the chunks of a file in front of the first failure, by tests/file_ref.py's lexer
  latin1_to_utf8       String(uncompressed.map{ Character(Unicode.Scalar($0)) }).utf8 (:198) is bytes.decode("latin-1").encode("utf-8")
  check_utf8           bytes.decode("utf-8"): the offset of the first ill-formed sequence is UnicodeDecodeError.start; how many there
                       are is how often a decoder that replaces maximal subparts is asked to (errors="replace" puts a U+FFFD each time)
"""
import codecs
import struct
from collections import namedtuple

DONE = 0
(E_TEXT_KEYWORD, E_TEXT_CHUNK_LENGTH, E_TEXT_LANGUAGE, E_TEXT_LOCALIZED_KEYWORD, E_TEXT_COMPRESSION_METHOD, E_TEXT_COMPRESSION,
 E_TEXT_INCOMPLETE) = range(96, 103)
E_PROFILE_NAME, E_PROFILE_CHUNK_LENGTH, E_PROFILE_COMPRESSION_METHOD, E_PROFILE_INCOMPLETE = range(104, 108)
E_TEXT_ENCODING, E_OUTPUT_CAPACITY = 112, 64
NONE = 0xffffffff
Head = namedtuple("Head", "status aux k l m body_off compressed")
HEADED = (b"tEXt", b"zTXt", b"iTXt", b"iCCP")


def valid_name(name: bytes) -> bool:
    """validate(name:), PNG.Text.swift:226-251"""
    if not 1 <= len(name) <= 80:                                 # :230-234
        return False
    previous = name[0]
    for c in name:                                               # :236-248
        if not (0x20 <= c <= 0x7d or 0xa1 <= c <= 0xff) or (previous, c) == (0x20, 0x20):
            return False
        previous = c
    return previous != 0x20                                      # :250


def valid_language(tag: bytes) -> bool:
    """validate(language:), :291-301"""
    return 1 <= len(tag) <= 8 and all(0x61 <= c <= 0x7a or 0x41 <= c <= 0x5a for c in tag)


def parse_head(kind: bytes, data: bytes) -> Head:
    k = data.find(b"\0")                                         # name(parsing:), :207-211
    profile = kind == b"iCCP"
    if k < 0:
        return Head(E_PROFILE_NAME if profile else E_TEXT_KEYWORD, 0, NONE, NONE, NONE, 0, 0)
    if not valid_name(data[:k]):                                 # :217-221
        return Head(E_PROFILE_NAME if profile else E_TEXT_KEYWORD, 1, k, NONE, NONE, 0, 0)
    if profile:
        if not k + 1 < len(data):                                # PNG.ColorProfile.swift:65-69
            return Head(E_PROFILE_CHUNK_LENGTH, k + 2, k, NONE, NONE, 0, 0)
        if data[k + 1] != 0:                                     # :71-75
            return Head(E_PROFILE_COMPRESSION_METHOD, data[k + 1], k, NONE, NONE, 0, 0)
        return Head(DONE, 0, k, NONE, NONE, k + 2, 1)            # :77-78
    if kind != b"iTXt":                                          # PNG.Text.swift:175-199
        compressed = k + 1 < len(data) and data[k + 1] == 0      # :181
        return Head(DONE, 0, k, NONE, NONE, k + 2 if compressed else k + 1, int(compressed))
    if not k + 2 < len(data):                                    # :126-130
        return Head(E_TEXT_CHUNK_LENGTH, k + 3, k, NONE, NONE, 0, 0)
    l = data.find(b"\0", k + 3)                                  # language(parsing:), :258-262
    if l < 0:
        return Head(E_TEXT_LANGUAGE, 0, k, NONE, NONE, 0, 0)
    if l > k + 3:                                                # :265-269: an empty tag is no language at all
        at = k + 3
        for tag in data[k + 3:l].split(b"-"):                    # :272-286
            if not valid_language(tag):
                return Head(E_TEXT_LANGUAGE, 1 + at, k, l, NONE, 0, 0)
            at += len(tag) + 1
    m = data.find(b"\0", l + 1)                                  # :139-143
    if m < 0:
        return Head(E_TEXT_LOCALIZED_KEYWORD, 0, k, l, NONE, 0, 0)
    flag, method = data[k + 1], data[k + 2]
    if flag == 0:                                                # :151-153
        return Head(DONE, 0, k, l, m, m + 1, 0)
    if flag == 1:                                                # :154-166
        if method != 0:
            return Head(E_TEXT_COMPRESSION_METHOD, method, k, l, m, 0, 0)
        return Head(DONE, 0, k, l, m, m + 1, 1)
    return Head(E_TEXT_COMPRESSION, flag, k, l, m, 0, 0)         # :167-168


def language_of(data: bytes, head: Head):
    """the reference's `language`: the subtags, lower-cased (:285); [] for an empty tag"""
    tag = data[head.k + 3:head.l]
    return [t.decode("latin-1").lower() for t in tag.split(b"-")] if tag else []


def bad_language_tag(data: bytes, head: Head):
    """the String? of invalidTextLanguageTag: None, or the subtag that is none"""
    if head.aux == 0:
        return None
    at = head.aux - 1
    end = data.find(b"\0", at)
    return data[at:end].split(b"-")[0].decode("latin-1")


Entry = namedtuple("Entry", "type length offset head")


def directory(data: bytes, chunks: int):
    """the first `chunks` chunks of a file (the number the lexer's yardstick reports as lexed in full) as directory entries"""
    out, pos = [], 8
    for _ in range(chunks):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        payload = data[pos + 8:pos + 8 + n]
        head = parse_head(kind, payload) if kind in HEADED else Head(DONE, 0, NONE, NONE, NONE, 0, 0)
        out.append(Entry(struct.unpack(">I", kind)[0], n, pos + 8, head))
        pos += 12 + n
    return out


def latin1_to_utf8(data: bytes) -> bytes:
    return data.decode("latin-1").encode("utf-8")


def check_utf8(data: bytes):
    """-> (status, aux0, aux1)"""
    try:
        data.decode("utf-8")
        return DONE, 0, 0
    except UnicodeDecodeError as e:
        first = e.start
    calls = []

    def count(err):
        calls.append(err.start)
        return "\ufffd", err.end
    codecs.register_error("metadata_ref_count", count)
    data.decode("utf-8", "metadata_ref_count")
    assert calls[0] == first
    return E_TEXT_ENCODING, first, len(calls)


# ---- serialisation: the way back ----------------------------------------------------------------------------------------------
def itxt_head(keyword: bytes, compressed: bool, language, localized: bytes) -> bytes:
    """PNG.Text.serialized up to the content (:317-332): every text goes out as iTXt.  keyword: Latin-1 bytes; language: the
    subtags; localized: UTF-8 bytes, b"" when it equals the keyword"""
    return keyword + b"\0" + bytes([1 if compressed else 0, 0]) + b"-".join(t.encode("latin-1") for t in language) + b"\0" + localized + b"\0"


def iccp_head(name: bytes) -> bytes:
    """PNG.ColorProfile.serialized up to the stream (PNG.ColorProfile.swift:89-95)"""
    return name + b"\0\0"


# ---- PNG.Metadata.push(ancillary:...) (Sources/PNG/Decoding/PNG.Metadata.swift:151-245): what is unique, what must precede PLTE ------
BEFORE_PLTE = (b"cHRM", b"gAMA", b"sRGB", b"iCCP", b"sBIT")     # :159-164: unexpected(chunk, after: .PLTE)
UNIQUE = (b"bKGD", b"tRNS", b"hIST", b"cHRM", b"gAMA", b"sRGB", b"iCCP", b"sBIT", b"pHYs", b"tIME")   # unique(assign:to:), :98-108, 178-233
# PNG.Image.compress(stream:), Sources/PNG/PNG.Image.swift:596-656: the order the metadata goes out in
ORDER_BEFORE = (b"cHRM", b"gAMA", b"sRGB", b"iCCP", b"sBIT")    # in front of PLTE
ORDER_AFTER = (b"hIST", b"pHYs", b"tIME")                       # behind tRNS; then iTXt ..., sPLT ..., the application chunks


class Duplicate(Exception):
    """PNG.DecodingError.duplicate(chunk:)"""


class Unexpected(Exception):
    """PNG.DecodingError.unexpected(chunk:after:)"""


class Required(Exception):
    """PNG.DecodingError.required(chunk:before:)"""


def text_fields(kind: bytes, payload: bytes, inflate):
    """a text chunk -> (keyword, compressed, language, localized, content as UTF-8): what PNG.Text holds (:110-200)"""
    h = parse_head(kind, payload)
    assert h.status == DONE, h
    body = payload[h.body_off:]
    if h.compressed:
        body = inflate(body)
    keyword = payload[:h.k]
    if kind != b"iTXt":                                          # :175-199
        return keyword, bool(h.compressed), ["en"], b"", latin1_to_utf8(body)
    localized = payload[h.l + 1:h.m]
    if localized.decode("utf-8", "replace") == keyword.decode("latin-1"):       # :146-147
        localized = b""
    return keyword, bool(h.compressed), language_of(payload, h), localized, body.decode("utf-8", "replace").encode("utf-8")


def reserialize(chunks, inflate, deflate, edit=None):
    """What the reference writes for the ancillary chunks it read: `chunks` -- [(type, payload)], the file's chunks in order, critical
    ones included -- pushed through PNG.Metadata.push(ancillary:...) (PNG.Metadata.swift:151-245) as PNG.Image.decompress does
    (PNG.Image.swift:298-400), `edit(fields)` applied to the unique fields (a dict by chunk type), and written back in the order of
    PNG.Image.compress (PNG.Image.swift:596-656) with PNG.Text.serialized (PNG.Text.swift:309-349) and PNG.ColorProfile.serialized
    (PNG.ColorProfile.swift:87-103).  inflate(bytes) -> bytes; deflate(bytes) -> bytes: LZ77.Deflator(level: 13, exponent: 15).
    -> (before, after): [(type, payload)] in front of PLTE and behind tRNS; bKGD / tRNS / PLTE are the format's business"""
    unique, texts, palettes, application = {}, [], [], []
    seen_plte = False
    for kind, payload in chunks:
        if kind in (b"CgBI", b"IHDR", b"IDAT", b"IEND"):
            continue
        if kind == b"PLTE":
            seen_plte = True
            continue
        if kind in BEFORE_PLTE and seen_plte:                    # :159-164
            raise Unexpected(kind)
        if kind == b"hIST" and not seen_plte:                    # :190-194
            raise Required(kind)
        if kind in UNIQUE:
            if kind in unique:                                   # :98-108
                raise Duplicate(kind)
            unique[kind] = (parse_head(kind, payload), payload) if kind == b"iCCP" else payload
        elif kind == b"sPLT":                                    # :236-237
            palettes.append(payload)
        elif kind in (b"iTXt", b"tEXt", b"zTXt"):                # :238-241
            texts.append(text_fields(kind, payload, inflate))
        else:                                                    # :243-244
            application.append((kind, payload))
    if edit:
        edit(unique)
    if b"iCCP" in unique:
        h, payload = unique[b"iCCP"]
        assert h.status == DONE, h
        unique[b"iCCP"] = iccp_head(payload[:h.k]) + deflate(inflate(payload[h.body_off:]))
    before = [(k, unique[k]) for k in ORDER_BEFORE if k in unique]
    after = [(k, unique[k]) for k in ORDER_AFTER if k in unique]
    for keyword, compressed, language, localized, content in texts:
        after.append((b"iTXt", itxt_head(keyword, compressed, language, localized) + (deflate(content) if compressed else content)))
    after += [(b"sPLT", p) for p in palettes] + application
    return before, after
