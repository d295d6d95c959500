"""The yardstick for whole PNG files: PNG.Image.compress(stream:level:hint:) behind its encoder (Sources/PNG/PNG.Image.swift:576-668 of the
reference) in plain Python -- struct and zlib.crc32, nothing shared with the C++ of csrc/file_head.hpp or the kernels of csrc/chunks.hip.
A file is signature, head, the zlib stream in IDAT chunks of chunk_bytes (the last one shorter, none empty), IEND; the head is
    CgBI, IHDR, the blobs `before`, PLTE, bKGD, tRNS, the blobs `after`
with PLTE / bKGD / tRNS as PNG.Layout derives them from a format (Formats/PNG.Layout.swift:60-194) and the parsing types serialise
them.  A format is (depth, channels, indexed, bgr) as everywhere in this project; palette: [(r, g, b, a)]; key / fill: as PNG.Format holds
them -- an int for the grey formats (fill of an indexed one: a palette index), (r, g, b), and (b, g, r) for bgr8 / bgra8."""
import struct
import zlib
from collections import namedtuple

SIG = b"\x89PNG\r\n\x1a\n"
OWNED = (b"CgBI", b"IHDR", b"PLTE", b"bKGD", b"tRNS", b"IDAT", b"IEND")
KNOWN = OWNED + (b"cHRM", b"gAMA", b"iCCP", b"sBIT", b"sRGB", b"hIST", b"pHYs", b"sPLT", b"tIME", b"iTXt", b"tEXt", b"zTXt")
Format = namedtuple("Format", "depth channels indexed bgr")
FORMATS = {"v1": Format(1, 1, 0, 0), "v2": Format(2, 1, 0, 0), "v4": Format(4, 1, 0, 0), "v8": Format(8, 1, 0, 0), "v16": Format(16, 1, 0, 0),
           "va8": Format(8, 2, 0, 0), "va16": Format(16, 2, 0, 0), "rgb8": Format(8, 3, 0, 0), "rgb16": Format(16, 3, 0, 0),
           "bgr8": Format(8, 3, 0, 1), "rgba8": Format(8, 4, 0, 0), "rgba16": Format(16, 4, 0, 0), "bgra8": Format(8, 4, 0, 1),
           "indexed1": Format(1, 1, 1, 0), "indexed2": Format(2, 1, 1, 0), "indexed4": Format(4, 1, 1, 0), "indexed8": Format(8, 1, 1, 0)}


class Refused(ValueError):
    """what the writer answers SPNG_E_ARGUMENT to"""


def chunk(name, data=b""):
    return struct.pack(">I", len(data)) + name + data + struct.pack(">I", zlib.crc32(name + data))


def type_lexes(name):
    """PNG.Chunk.init(validating:) (PNG.Chunk.swift:69-88): one of the known chunks, or an ancillary one (lowercase first letter) whose
    reserved bit is clear (uppercase third letter)"""
    return name in KNOWN or (name[0] & 0x20 and not name[2] & 0x20)


def kind_of(depth, channels, indexed, bgr):
    if indexed:
        ok = channels == 1 and not bgr and depth in (1, 2, 4, 8)
        return "indexed" if ok else None
    if bgr:
        return {3: "rgb", 4: "rgba"}.get(channels) if depth == 8 else None
    if channels == 1:
        return "v" if depth in (1, 2, 4, 8, 16) else None
    return {2: "va", 3: "rgb", 4: "rgba"}.get(channels) if depth in (8, 16) else None


def derived(depth, channels, indexed=0, bgr=0, palette=(), key=None, fill=None):
    """-> (PLTE, bKGD, tRNS) payloads, None for a chunk the layout does not write"""
    kind = kind_of(depth, channels, indexed, bgr)
    if kind is None:
        raise Refused("no PNG.Format")
    palette = [tuple(p) for p in palette]
    most = 0 if kind in ("v", "va") else 1 << min(depth, 8)
    if len(palette) > most or (kind == "indexed" and not palette):
        raise Refused("palette count")
    if key is not None and kind not in ("v", "rgb"):
        raise Refused("a key where the format has none")
    top = 65535 if depth == 16 else 255

    def fields(v):
        v = (v,) if kind in ("v", "va") else tuple(v)
        if len(v) != (1 if kind in ("v", "va") else 3) or any(not 0 <= x <= top for x in v):
            raise Refused("a field the format does not hold")
        return b"".join(struct.pack(">H", x) for x in (v[::-1] if bgr else v))

    plte = b"".join(bytes(p[:3]) for p in palette) if palette else None
    bkgd = trns = None
    if fill is not None:
        if kind == "indexed":
            if not 0 <= fill < len(palette):
                raise Refused("fill index")
            bkgd = bytes([fill])
        else:
            bkgd = fields(fill)
            if kind == "v" and depth < 8 and fill >> depth:
                raise Refused("fill sample")
    if kind == "indexed":
        alphas = [p[3] for p in palette]
        while alphas and alphas[-1] == 255:
            alphas.pop()
        trns = bytes(alphas) if alphas else None
    elif key is not None:
        trns = fields(key)
    return plte, bkgd, trns


def head(width, height, depth, channels, indexed=0, bgr=0, interlaced=0, palette=(), key=None, fill=None, before=(), after=()):
    """the bytes between the signature and the first IDAT; before / after: [(type, payload)]"""
    plte, bkgd, trns = derived(depth, channels, indexed, bgr, palette, key, fill)
    if not width or not height:
        raise Refused("size")
    for name, data in list(before) + list(after):
        if len(name) != 4 or name in OWNED or not type_lexes(name):
            raise Refused("blob type")
    kind = kind_of(depth, channels, indexed, bgr)
    out = b""
    if bgr:
        out += chunk(b"CgBI", bytes([48, 0, 32, 6 if channels == 3 else 2]))
    code = {"v": 0, "rgb": 2, "indexed": 3, "va": 4, "rgba": 6}[kind]
    out += chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, code, 0, 0, 1 if interlaced else 0))
    out += b"".join(chunk(n, d) for n, d in before)
    for name, data in ((b"PLTE", plte), (b"bKGD", bkgd), (b"tRNS", trns)):
        if data is not None:
            out += chunk(name, data)
    return out + b"".join(chunk(n, d) for n, d in after)


def body(stream, chunk_bytes):
    if not 1 <= chunk_bytes <= 0x7fffffff:
        raise Refused("chunk_bytes")
    return b"".join(chunk(b"IDAT", stream[at:at + chunk_bytes]) for at in range(0, len(stream), chunk_bytes))


def write(stream, chunk_bytes, width, height, depth, channels, **kw):
    """the whole file"""
    return SIG + head(width, height, depth, channels, **kw) + body(stream, chunk_bytes) + chunk(b"IEND")


def parse(data):
    """a well-formed file -> [(type, payload)]"""
    assert data[:8] == SIG
    pos, out = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        name, payload = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(name + payload), name
        out.append((name, payload))
        pos += 12 + n
    assert pos == len(data) and out[-1] == (b"IEND", b"")
    return out


def pieces(data):
    """A file the reference wrote, taken apart into what write() takes: -> dict(stream, chunk_bytes, width, ..., before, after) with
    the format's inputs read back from PLTE / bKGD / tRNS the way PNG.Format.recognize does (Formats/PNG.Format.swift:396-560)"""
    cs = parse(data)
    names = [n for n, _ in cs]
    bgr = int(names[0] == b"CgBI")
    ihdr = cs[bgr][1]
    width, height, depth, code, _, _, interlace = struct.unpack(">IIBBBBB", ihdr)
    channels, indexed = {0: (1, 0), 2: (3, 0), 3: (1, 1), 4: (2, 0), 6: (4, 0)}[code]
    first = names.index(b"IDAT")
    mid = [k for k in range(bgr + 1, first) if names[k] in (b"PLTE", b"bKGD", b"tRNS")]
    lo, hi = (mid[0], mid[-1] + 1) if mid else (first, first)
    assert [names[k] for k in mid] == [n for n in (b"PLTE", b"bKGD", b"tRNS") if n in names[:first]] and mid == list(range(lo, hi))
    got = dict(cs[lo:hi])
    palette, key, fill = [], None, None
    if b"PLTE" in got:
        p = got[b"PLTE"]
        alphas = got.get(b"tRNS", b"") if indexed else b""
        palette = [(p[3 * k], p[3 * k + 1], p[3 * k + 2], alphas[k] if k < len(alphas) else 255) for k in range(len(p) // 3)]

    def unfields(raw):
        v = struct.unpack(">" + "H" * (len(raw) // 2), raw)
        return v[0] if len(v) == 1 else (v[::-1] if bgr else v)

    if b"tRNS" in got and not indexed:
        key = unfields(got[b"tRNS"])
    if b"bKGD" in got:
        fill = got[b"bKGD"][0] if indexed else unfields(got[b"bKGD"])
    idats = [d for n, d in cs if n == b"IDAT"]
    assert names[first:first + len(idats)] == [b"IDAT"] * len(idats) and names[first + len(idats):] == [b"IEND"]
    return dict(stream=b"".join(idats), chunk_bytes=max(len(d) for d in idats), width=width, height=height, depth=depth, channels=channels,
                indexed=indexed, bgr=bgr, interlaced=interlace, palette=palette, key=key, fill=fill, before=cs[bgr + 1:lo], after=cs[hi:first])
