"""tests/lex_ref.py -- the yardstick of the lexer tests -- pinned against what the project already holds: the test-side parser on every
PngSuite fixture, the reference's negative fixtures with the two checksum pairs its own tests pin
(Sources/PNGIntegrationTests/ErrorHandling.swift:30,42), and the hand-built damage of the lexer tests with the answers stated there."""
import json
import struct
import zlib

import numpy as np

import pnghelp as ph
from lex_ref import (DONE, E_CHUNK_CHECKSUM, E_CHUNK_TYPE, E_OUTPUT_CAPACITY, E_SIGNATURE, E_TRUNCATED_CHUNK_BODY, E_TRUNCATED_CHUNK_HEADER,
                     E_TRUNCATED_SIGNATURE, lex_ref)

TABLE = json.loads((ph.GOLDEN / "pngsuite.json").read_text())
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(name, data, crc=None):
    return struct.pack(">I", len(data)) + name + data + struct.pack(">I", zlib.crc32(name + data) if crc is None else crc)


IHDR = chunk(b"IHDR", struct.pack(">IIBBBBB", 32, 32, 8, 0, 0, 0, 0))
IEND = chunk(b"IEND", b"")


def payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_every_fixture_as_the_test_side_parser_reads_it():
    assert len(TABLE) >= 190
    for name in sorted(TABLE):
        f = (ph.GOLDEN / "pngsuite" / name).read_bytes()
        png = ph.parse_png(f)
        r, idat = lex_ref(f, len(f))
        assert r.status == DONE and (r.aux0, r.aux1) == (0, 0), name
        assert (r.width, r.height, r.depth, r.color, bool(r.interlace), bool(r.ios)) == (png.width, png.height, png.depth, png.color, png.interlaced, png.ios), name
        assert (r.compression, r.filter) == (0, 0), name
        assert idat == png.idat and r.idat_len == len(png.idat), name
        assert (f[r.plte_off:r.plte_off + r.plte_len] == png.palette) if png.palette is not None else (r.plte_off, r.plte_len) == (0, 0), name
        assert (f[r.trns_off:r.trns_off + r.trns_len] == png.trns) if png.trns is not None else (r.trns_off, r.trns_len) == (0, 0), name
        assert r.consumed <= len(f) and f[r.consumed - 8:r.consumed - 4] == b"IEND", name
        pos, chunks = 8, 0
        while pos < r.consumed:
            pos += 12 + struct.unpack(">I", f[pos:pos + 4])[0]
            chunks += 1
        assert r.chunks == chunks and pos == r.consumed, name


def test_the_reference_negative_fixtures():
    inv = ph.GOLDEN / "invalid"
    lex = lambda name: lex_ref((inv / f"{name}.png").read_bytes(), 1 << 30)[0]
    for name in ("xs1n0g01", "xs2n0g01", "xs4n0g01", "xs7n0g01", "xcrn0g04", "xlfn0g04"):
        r = lex(name)
        assert (r.status, r.aux0, r.consumed, r.chunks) == (E_SIGNATURE, struct.unpack(">Q", (inv / f"{name}.png").read_bytes()[:8])[0], 8, 0), name
    r = lex("xhdn0g08")
    assert (r.status, r.aux0, r.aux1, r.chunks, r.consumed) == (E_CHUNK_CHECKSUM, 1129534797, 1443964200, 0, 8)
    assert (r.width, r.height, r.depth) == (0, 0, 0)                     # (the IHDR whose checksum is wrong was never noted)
    r = lex("xcsn0g01")
    assert (r.status, r.aux0, r.aux1) == (E_CHUNK_CHECKSUM, 1129534797, 3492746441)
    for name in ("xc1n0g08", "xc9n2c08", "xd0n2c08", "xd3n2c08", "xd9n2c08", "xdtn0g01"):
        assert lex(name).status == DONE, name
    assert lex("xdtn0g01").idat_len == 0
    f = (ph.GOLDEN / "pngsuite" / "common" / "basn6a08.png").read_bytes()
    assert lex_ref(f[:5], 99)[0][:4] == (E_TRUNCATED_SIGNATURE, 0, 0, 0) and lex_ref(f[:5], 99)[0].consumed == 5
    assert lex_ref(f[:12], 99)[0].status == E_TRUNCATED_CHUNK_HEADER and lex_ref(f[:12], 99)[0].consumed == 8
    r = lex_ref(f[:30], 99)[0]
    assert (r.status, r.aux0, r.consumed, r.width) == (E_TRUNCATED_CHUNK_BODY, 13 + 4, 8, 0)
    r = lex_ref(f[:-12], len(f))[0]
    assert (r.status, r.consumed, r.width) == (E_TRUNCATED_CHUNK_HEADER, len(f) - 12, 32)
    bad = bytearray(f); bad[8 + 6] = ord("d")
    r = lex_ref(bytes(bad), len(f))[0]
    assert (r.status, r.aux0, r.consumed) == (E_CHUNK_TYPE, struct.unpack(">I", bytes(bad[12:16]))[0], 8)


def test_the_hand_built_damage_of_the_lexer_tests():
    body = payload(3000, 3)
    good = SIG + IHDR + chunk(b"IDAT", body) + chunk(b"IDAT", body[:100]) + IEND
    n, at = len(good), 8 + len(IHDR)
    r, idat = lex_ref(good, n)
    assert (r.status, r.chunks, r.idat_len, r.consumed, r.width, r.height, r.depth) == (DONE, 4, 3100, n, 32, 32, 8) and idat == body + body[:100]
    bad = bytearray(good); bad[at + 8 + 10] ^= 0x40
    r, idat = lex_ref(bytes(bad), n)
    assert (r.status, r.aux0, r.aux1) == (E_CHUNK_CHECKSUM, zlib.crc32(b"IDAT" + body), zlib.crc32(bytes(bad[at + 4:at + 8 + 3000])))
    assert (r.chunks, r.idat_len, r.consumed, idat, r.width) == (1, 0, at, b"", 32)
    assert lex_ref(bytes(bad[:at + 8 + 1000]), n)[0][:3] == (E_TRUNCATED_CHUNK_BODY, 1, 3004)
    # a bad checksum in chunk 3 and a bad type in chunk 5: the checksum wins; alone, the type is reported with nothing but its header there
    cs = [IHDR, chunk(b"gAMA", b"\0\0\0\1"), chunk(b"IDAT", body), chunk(b"IDAT", body[:50], crc=5), chunk(b"IDAT", body[:7]), chunk(b"IDaT", b"xx"), IEND]
    r, idat = lex_ref(SIG + b"".join(cs), 1 << 20)
    assert (r.status, r.aux0, r.aux1, r.chunks, r.idat_len) == (E_CHUNK_CHECKSUM, 5, zlib.crc32(b"IDAT" + body[:50]), 3, 3000) and idat == body
    cs[3] = chunk(b"IDAT", body[:50])
    data = SIG + b"".join(cs)
    upto = 8 + sum(len(c) for c in cs[:5])
    assert lex_ref(data[:upto + 3], 1 << 20)[0][:2] == (E_TRUNCATED_CHUNK_HEADER, 5)
    for k in (upto + 8, len(data)):
        r = lex_ref(data[:k], 1 << 20)[0]
        assert (r.status, r.aux0, r.chunks, r.idat_len, r.consumed) == (E_CHUNK_TYPE, struct.unpack(">I", b"IDaT")[0], 5, 3057, upto)
    # a bad signature is known with its eighth byte
    data = b"\x89PNG\r\n\x1a\r" + good[8:]
    assert (lex_ref(data[:7], n)[0].status, lex_ref(data[:7], n)[0].consumed) == (E_TRUNCATED_SIGNATURE, 7)
    for k in (8, n):
        r = lex_ref(data[:k], n)[0]
        assert (r.status, r.aux0, r.consumed) == (E_SIGNATURE, struct.unpack(">Q", data[:8])[0], 8)
    # idat_cap exceeded by the second IDAT: its checksum first
    for broken in (False, True):
        data = bytearray(good)
        if broken:
            data[at + 12 + 3000 + 8 + 3] ^= 2
        r, idat = lex_ref(bytes(data[:at + 12 + 3000 + 8 + 60]), 3050)
        assert (r.status, r.idat_len, r.chunks) == (E_TRUNCATED_CHUNK_BODY, 3000, 2) and idat == body
        r, idat = lex_ref(bytes(data), 3050)
        assert (r.status, r.chunks, r.idat_len, r.consumed) == (E_CHUNK_CHECKSUM if broken else E_OUTPUT_CAPACITY, 2, 3000, at + 12 + 3000) and idat == body
        assert (r.aux0, r.aux1) == ((zlib.crc32(b"IDAT" + body[:100]), zlib.crc32(bytes(data[at + 3016:at + 3120]))) if broken else (0, 0))
    # bytes behind IEND are ignored
    r = lex_ref(good + b"trailing bytes", n)[0]
    assert (r.status, r.consumed) == (DONE, n) and lex_ref(good[:n - 20], n)[0].status in (E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_CHUNK_BODY)
    # PLTE / tRNS: those of the last such chunk; a short IHDR is not noted
    data = SIG + chunk(b"IHDR", b"\0" * 12) + chunk(b"PLTE", b"abc") + chunk(b"tRNS", b"z") + chunk(b"CgBI", b"") + chunk(b"PLTE", b"defghi") + IEND
    r = lex_ref(data, 0)[0]
    assert (r.status, r.width, r.ios, r.plte_len, r.trns_len, r.trns_off) == (DONE, 0, 1, 6, 1, 8 + 24 + 15 + 8)
    assert data[r.plte_off:r.plte_off + 6] == b"defghi"
