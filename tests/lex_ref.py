"""The chunk lexer the lexer tests measure against: the reference's loop -- signature() and chunk() of
Sources/PNG/Lexing/PNG.BytestreamSource.swift:44-108, the type check of PNG.Chunk.swift:69-88, the IDAT loop of PNG.Image.swift:385-389 --
restated in plain Python, CRC-32 by zlib.  It walks the file front to back and returns at the first failure, which is what "the
first failure in file order decides" means; nothing here is shared with csrc/chunks.hip.  Pinned by tests/test_lex_ref.py."""
import struct
import zlib
from collections import namedtuple

(DONE, E_OUTPUT_CAPACITY, E_ARGUMENT, E_TRUNCATED_SIGNATURE, E_SIGNATURE, E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_CHUNK_BODY, E_CHUNK_TYPE,
 E_CHUNK_CHECKSUM) = 0, 64, 65, 80, 81, 82, 83, 84, 85
SIGNATURE = b"\x89PNG\r\n\x1a\n"
KNOWN = frozenset((b"CgBI", b"IHDR", b"PLTE", b"IDAT", b"IEND", b"cHRM", b"gAMA", b"iCCP", b"sBIT", b"sRGB", b"bKGD", b"hIST", b"tRNS", b"pHYs",
                   b"sPLT", b"tIME", b"iTXt", b"tEXt", b"zTXt"))
FIELDS = ("status", "chunks", "aux0", "aux1", "width", "height", "depth", "color", "compression", "filter", "interlace", "ios", "idat_len",
          "plte_off", "plte_len", "trns_off", "trns_len", "consumed")
Lexed = namedtuple("Lexed", FIELDS)


def lex_ref(data: bytes, idat_cap: int):
    """-> (Lexed: every field of spng_lexed, the IDAT bytes in front of idat_len)"""
    n = len(data)
    r = dict.fromkeys(FIELDS, 0)
    idat = []

    def end(status, consumed, aux0=0, aux1=0):
        r.update(status=status, aux0=aux0, aux1=aux1, consumed=min(consumed, n), idat_len=sum(len(b) for b in idat))
        return Lexed(**r), b"".join(idat)

    if n < 8:
        return end(E_TRUNCATED_SIGNATURE, 8)
    if data[:8] != SIGNATURE:
        return end(E_SIGNATURE, 8, struct.unpack(">Q", data[:8])[0])
    off = 8
    while True:
        if off + 8 > n:
            return end(E_TRUNCATED_CHUNK_HEADER, off)
        length, code = struct.unpack(">II", data[off:off + 8])
        name = data[off + 4:off + 8]
        if name not in KNOWN and (code & 0x20002000) != 0x20000000:
            return end(E_CHUNK_TYPE, off, code)
        if off + 12 + length > n:
            return end(E_TRUNCATED_CHUNK_BODY, off, length + 4)
        body = data[off + 8:off + 8 + length]
        (declared,) = struct.unpack(">I", data[off + 8 + length:off + 12 + length])
        computed = zlib.crc32(name + body)
        if declared != computed:
            return end(E_CHUNK_CHECKSUM, off, declared, computed)
        if name == b"IDAT":
            if sum(len(b) for b in idat) + length > idat_cap:
                return end(E_OUTPUT_CAPACITY, off)
            idat.append(body)
        elif name == b"CgBI":
            r["ios"] = 1
        elif name == b"IHDR" and length >= 13:
            (r["width"], r["height"], r["depth"], r["color"], r["compression"], r["filter"], r["interlace"]) = struct.unpack(">IIBBBBB", body[:13])
        elif name == b"PLTE":
            r["plte_off"], r["plte_len"] = off + 8, length
        elif name == b"tRNS":
            r["trns_off"], r["trns_len"] = off + 8, length
        r["chunks"] += 1
        off += 12 + length
        if name == b"IEND":
            return end(DONE, off)


def of_struct(info) -> Lexed:
    """a spng_lexed as the package's ctypes structure holds it"""
    return Lexed(info.status, info.chunks, info.aux[0], info.aux[1], info.width, info.height, info.depth, info.color, info.compression, info.filter,
                 info.interlace, info.ios, info.idat_len, info.plte_off, info.plte_len, info.trns_off, info.trns_len, info.consumed)
