"""TEST INFRASTRUCTURE: the case table of the chunk directory (spng_lex_dir_batch) and the text entry (spng_text_batch): the smallest
inputs on which their kernels can go wrong.  Every case names what it must produce -- a status, a field -- and tests/test_metadata_ref.py
holds the yardstick (tests/metadata_ref.py) to those claims; tests/test_emu_metadata.py and tests/test_gpu_metadata.py hold the kernels
to the yardstick."""
import struct
import zlib
from collections import namedtuple

import metadata_ref as mr
import pnghelp as ph

TILE = 4096                                                       # csrc/text.hip: TEXT_TILE
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(name, data=b"", crc=None):
    return struct.pack(">I", len(data)) + name + data + struct.pack(">I", zlib.crc32(name + data) if crc is None else crc)


IHDR = chunk(b"IHDR", struct.pack(">IIBBBBB", 32, 32, 8, 0, 0, 0, 0))
IEND = chunk(b"IEND")


def file_of(*chunks):
    return SIG + IHDR + b"".join(chunks) + IEND


# ---- directory ---------------------------------------------------------------------------------------------------------------
# a case is a batch: files, the room of each directory (None: all the file could need), the chunks each file must report
DirCase = namedtuple("DirCase", "name files caps chunks")


def pngsuite():
    return sorted((ph.GOLDEN / "pngsuite").glob("*/*.png"))


def dir_cases():
    small = (ph.GOLDEN / "pngsuite" / "common" / "basn0g01.png").read_bytes()
    many = file_of(*[chunk(b"IDAT", bytes([k])) for k in range(200)])          # 202 chunks; the lexer's list holds 65 of them
    assert len(many) // 2048 + 64 == 65
    six = [IHDR, chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tEXt", b"Title\0six chunks"), chunk(b"IDAT", b"\x78\x9c\x03\x00", crc=1),
           chunk(b"IDAT", b"\0\0\0\x01"), IEND]
    headed = file_of(chunk(b"tEXt", b"Author\0somebody"), chunk(b"iTXt", b"Title\0\0\0en\0Titel\0text"), chunk(b"IDAT", b"x"),
                     chunk(b"zTXt", b"Comment\0\0" + zlib.compress(b"body")), chunk(b"iCCP", b"profile\0\0" + zlib.compress(b"p" * 40)))
    suite = [p.read_bytes() for p in pngsuite()]
    return [
        DirCase("bad signature", [b"\x89PNG\r\n\x1a\r" + small[8:]], None, [0]),
        DirCase("every prefix of basn0g01", [small[:c] for c in range(len(small) + 1)], None, None),
        DirCase("cap = chunks, chunks - 1, 0", [headed] * 3, [7, 6, 0], [7, 7, 7]),
        DirCase("202 chunks, 65 listed", [many, many, many], [202, 201, 70], [202, 202, 202]),
        DirCase("wrong checksum in chunk 3 of 6", [SIG + b"".join(six)], None, [3]),
        DirCase("pngsuite", suite, None, None),
    ]


# ---- heads -------------------------------------------------------------------------------------------------------------------
# claim: the status, and for a good head (k, l, m, body_off, compressed) -- None where the case does not care; for a bad one the aux
HeadCase = namedtuple("HeadCase", "name kind payload status claim")
NONE = mr.NONE


def head_cases():
    out = []

    def add(name, kind, payload, status, claim=None):
        out.append(HeadCase(name, kind, payload, status, claim))

    for n in (0, 1, 79, 80, 81):
        ok = 1 <= n <= 80
        add(f"keyword of {n}", b"tEXt", b"k" * n + b"\0text", mr.DONE if ok else mr.E_TEXT_KEYWORD, (n, NONE, NONE, n + 1, 0) if ok else 1)
        add(f"profile name of {n}", b"iCCP", b"k" * n + b"\0\0zz", mr.DONE if ok else mr.E_PROFILE_NAME, (n, NONE, NONE, n + 2, 1) if ok else 1)
    for at in (63, 64, 65):                                       # the keyword's NUL around the end of the first 64 bytes
        add(f"NUL at byte {at}", b"tEXt", b"k" * at + b"\0t", mr.DONE, (at, NONE, NONE, at + 1, 0))
        tag = (b"ab-" * at)[:at - 13]                            # the language tag's NUL there too, the localised keyword's a block on
        tag = tag[:-1] + b"c" if tag.endswith(b"-") else tag
        add(f"iTXt with l at byte {at}", b"iTXt", b"k" * 10 + b"\0\0\0" + tag + b"\0" + b"L" * at + b"\0t", mr.DONE, (10, at, 2 * at + 1, 2 * at + 2, 0))
    for n in (1, 63, 64, 65, 200):
        add(f"no NUL in {n} bytes", b"zTXt", b"k" * n, mr.E_TEXT_KEYWORD, 0)
        add(f"no NUL in a profile of {n} bytes", b"iCCP", b"k" * n, mr.E_PROFILE_NAME, 0)
    add("empty payload", b"tEXt", b"", mr.E_TEXT_KEYWORD, 0)
    add("leading space", b"tEXt", b" key\0t", mr.E_TEXT_KEYWORD, 1)
    add("trailing space", b"tEXt", b"key \0t", mr.E_TEXT_KEYWORD, 1)
    add("doubled space", b"tEXt", b"a  key\0t", mr.E_TEXT_KEYWORD, 1)
    add("single spaces", b"tEXt", b"a key word\0t", mr.DONE, (10, NONE, NONE, 11, 0))
    add("a space alone", b"tEXt", b" \0t", mr.E_TEXT_KEYWORD, 1)
    add("doubled space across byte 64", b"tEXt", b"k" * 63 + b"  k\0t", mr.E_TEXT_KEYWORD, 1)
    for c, ok in ((0x1f, 0), (0x20, 1), (0x7d, 1), (0x7e, 0), (0x7f, 0), (0xa0, 0), (0xa1, 1), (0xff, 1)):
        add(f"byte {c:#x} in the keyword", b"tEXt", b"k" + bytes([c]) + b"k\0t", mr.DONE if ok else mr.E_TEXT_KEYWORD, (3, NONE, NONE, 4, 0) if ok else 1)
        add(f"byte {c:#x} at byte 70 of a name", b"iCCP", b"k" * 70 + bytes([c]) + b"k\0\0z", mr.DONE if ok else mr.E_PROFILE_NAME,
            (72, NONE, NONE, 74, 1) if ok else 1)
    # the Latin-1 path: the second NUL decides, not the type
    add("tEXt without a second NUL", b"tEXt", b"key\0text", mr.DONE, (3, NONE, NONE, 4, 0))
    add("tEXt with a second NUL", b"tEXt", b"key\0\0" + zlib.compress(b"t"), mr.DONE, (3, NONE, NONE, 5, 1))
    add("zTXt without a second NUL", b"zTXt", b"key\0\x01text", mr.DONE, (3, NONE, NONE, 4, 0))
    add("zTXt ending at k", b"zTXt", b"key\0", mr.DONE, (3, NONE, NONE, 4, 0))
    add("zTXt ending at k + 1", b"zTXt", b"key\0\0", mr.DONE, (3, NONE, NONE, 5, 1))
    add("tEXt ending at k", b"tEXt", b"key\0", mr.DONE, (3, NONE, NONE, 4, 0))
    add("iTXt ending at k", b"iTXt", b"key\0", mr.E_TEXT_CHUNK_LENGTH, 6)
    add("iTXt ending at k + 1", b"iTXt", b"key\0\0", mr.E_TEXT_CHUNK_LENGTH, 6)
    add("iTXt ending at k + 2", b"iTXt", b"key\0\0\0", mr.E_TEXT_LANGUAGE, 0)
    for tag, ok in ((b"", 1), (b"en", 1), (b"en-US", 1), (b"abcdefgh", 1), (b"abcdefghi", 0), (b"en--US", 0), (b"en-", 0), (b"-en", 0), (b"-", 0),
                    (b"en-U5", 0), (b"EN-Latn-US", 1), (b"x-abcdefgh-abcdefghi", 0), (b"en-" * 40 + b"us", 1), (b"en-" * 40 + b"u_", 0)):
        bad = None
        if not ok:
            at = 0
            for sub in tag.split(b"-"):
                if not mr.valid_language(sub):
                    bad = 1 + 6 + at
                    break
                at += len(sub) + 1
        add(f"language tag {tag[:24]!r}", b"iTXt", b"key\0\0\0" + tag + b"\0\0text", mr.DONE if ok else mr.E_TEXT_LANGUAGE,
            (3, 6 + len(tag), 7 + len(tag), 8 + len(tag), 0) if ok else bad)
    add("no NUL behind the language tag", b"iTXt", b"key\0\0\0en", mr.E_TEXT_LANGUAGE, 0)
    add("no NUL behind a bad language tag", b"iTXt", b"key\0\0\0e9", mr.E_TEXT_LANGUAGE, 0)
    add("no NUL behind the localised keyword", b"iTXt", b"key\0\0\0en\0Schluessel", mr.E_TEXT_LOCALIZED_KEYWORD, 0)
    add("nothing behind the language tag", b"iTXt", b"key\0\0\0en\0", mr.E_TEXT_LOCALIZED_KEYWORD, 0)
    add("flag 0", b"iTXt", b"key\0\0\0en\0K\0text", mr.DONE, (3, 8, 10, 11, 0))
    add("flag 1", b"iTXt", b"key\0\1\0en\0K\0" + zlib.compress(b"text"), mr.DONE, (3, 8, 10, 11, 1))
    add("flag 2", b"iTXt", b"key\0\2\0en\0K\0text", mr.E_TEXT_COMPRESSION, 2)
    add("flag 255 with method 1", b"iTXt", b"key\0\xff\1en\0K\0text", mr.E_TEXT_COMPRESSION, 255)
    add("method 1 with flag 1", b"iTXt", b"key\0\1\1en\0K\0text", mr.E_TEXT_COMPRESSION_METHOD, 1)
    add("method 1 with flag 0", b"iTXt", b"key\0\0\1en\0K\0text", mr.DONE, (3, 8, 10, 11, 0))
    add("a bad flag behind a bad language tag", b"iTXt", b"key\0\2\0e9\0K\0text", mr.E_TEXT_LANGUAGE, 7)
    add("a bad keyword in front of everything", b"iTXt", b"key \0\2\0e9", mr.E_TEXT_KEYWORD, 1)
    add("iCCP ending at k", b"iCCP", b"name\0", mr.E_PROFILE_CHUNK_LENGTH, 6)
    add("iCCP ending at k + 1", b"iCCP", b"name\0\0", mr.DONE, (4, NONE, NONE, 6, 1))
    add("iCCP with method 1", b"iCCP", b"name\0\1" + zlib.compress(b"p"), mr.E_PROFILE_COMPRESSION_METHOD, 1)
    add("a long body", b"zTXt", b"Raw profile type exif\0\0" + zlib.compress(bytes(range(256)) * 40), mr.DONE, (21, NONE, NONE, 23, 1))
    return out


def head_file(case):
    return file_of(chunk(case.kind, case.payload))


# ---- transcode -----------------------------------------------------------------------------------------------------------------
# data, the offsets of source and destination from a 16-byte boundary, out_cap as a difference from the bytes needed
TranscodeCase = namedtuple("TranscodeCase", "name data src_at dst_at cap_delta")


def pattern(n, kind):
    if kind == "ascii":
        return bytes(0x20 + k % 95 for k in range(n))
    if kind == "high":
        return bytes(0x80 + (k * 7) % 128 for k in range(n))
    if kind == "alternating":
        return bytes((0x41 + k % 26) if k % 2 else (0xa1 + k % 90) for k in range(n))
    raise ValueError(kind)


def transcode_cases():
    out = []
    for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
        for kind in ("ascii", "high", "alternating"):
            out.append(TranscodeCase(f"{n} bytes, {kind}", pattern(n, kind), 0, 0, 0))
    tail = bytearray(pattern(2 * TILE, "ascii"))
    tail[TILE - 1] = 0xe9
    tail[-1] = 0xff
    out.append(TranscodeCase("a high byte ends a tile and the input", bytes(tail), 0, 0, 0))
    out.append(TranscodeCase("one short", bytes(tail), 0, 0, -1))
    out.append(TranscodeCase("one short, no high byte", pattern(100, "ascii"), 0, 0, -1))
    out.append(TranscodeCase("room to spare", pattern(100, "high"), 0, 0, 5))
    mixed = pattern(TILE + 77, "alternating")
    for src_at in (0, 1, 2, 3, 15):
        for dst_at in (0, 1, 2, 3, 15):
            out.append(TranscodeCase(f"source at {src_at}, destination at {dst_at}", mixed, src_at, dst_at, 0))
    return out


# ---- UTF-8 check -----------------------------------------------------------------------------------------------------------------
# claim: None -- well-formed --, or (the offset of the first ill-formed sequence, how many there are)
Utf8Case = namedtuple("Utf8Case", "name data claim")
TWO, THREE, FOUR = "é".encode(), "€".encode(), "\U0001f600".encode()


def utf8_cases():
    out = [Utf8Case("empty", b"", None), Utf8Case("ascii", pattern(200, "ascii"), None),
           Utf8Case("every length", ("aé€\U0001f600" * 700).encode(), None),
           Utf8Case("the ends of the ranges", "\x7f\x80߿ࠀ퟿\U00010000\U0010ffff".encode(), None)]
    for seq in (TWO, THREE, FOUR):
        for edge in (16, 64, TILE):
            for back in range(1, len(seq)):
                good = b"a" * (edge - back) + seq + b"b" * 20
                out.append(Utf8Case(f"{len(seq)} bytes, {back} in front of byte {edge}", good, None))
                cut = good[:edge]
                out.append(Utf8Case(f"{len(seq)} bytes cut behind {back} at byte {edge}", cut, (edge - back, 1)))
                broken = good[:edge] + b"A" + good[edge + 1:]
                out.append(Utf8Case(f"{len(seq)} bytes broken behind {back} at byte {edge}", broken, (edge - back, len(seq) - back)))
    classes = {"overlong 2": (b"\xc0\xaf", 2), "overlong 3": (b"\xe0\x9f\xbf", 3), "overlong 4": (b"\xf0\x8f\xbf\xbf", 4),
               "surrogate": (b"\xed\xa0\x80", 3), "above U+10FFFF": (b"\xf4\x90\x80\x80", 4), "lead f5": (b"\xf5\x80\x80\x80", 4),
               "byte ff": (b"\xff", 1), "stray continuation": (b"\x80", 1), "four continuations": (b"\xe2\x82\xac\x80\x80\x80\x80", 4),
               "missing continuation": (b"\xe2\x82", 1), "missing second": (b"\xc3", 1), "lead after lead": (b"\xe2\xc3\xa9", 1)}
    for name, (seq, count) in classes.items():
        first = 3 if name == "four continuations" else 0
        out.append(Utf8Case(name, b"ab" + seq + b"cd", (2 + first, count)))
        out.append(Utf8Case(name + " behind a tile of good text", (THREE * (TILE // 3 + 1))[:TILE // 3 * 3] + b"a" * (TILE % 3) + seq + b"cd", (TILE + first, count)))
        out.append(Utf8Case(name + " at the end", b"ab" + seq, (2 + first, count)))
    out.append(Utf8Case("two errors, tiles apart", b"\xff" + b"a" * (2 * TILE) + b"\x80", (0, 2)))
    out.append(Utf8Case("an error in the last byte of a tile", b"a" * (TILE - 1) + b"\xc3" + b"a" * 5, (TILE - 1, 1)))
    return out
