"""GPU parity for files that arrive in pieces (spng_lex_resume_batch; waitSignature / waitChunk of the reference's OnlineDecoding
tutorial, Snippets/PNG/OnlineDecoding.swift): after every push every field of the result and the IDAT bytes in front of idat_len are
what tests/lex_ref.py -- the reference's loop in plain Python -- gives for the same prefix; over all pushes of
a file every byte of type + data is summed once and every IDAT byte copied once (spng_lex_resume_stats: counters, not clocks); and
the tutorial end to end, from file bytes in pieces of 4096 to the images the reference wrote after every IDAT chunk
(tests/golden/online.json)."""
import hashlib
import json
import struct
import zlib

import numpy as np
import pytest

import pnghelp as ph
from lex_ref import lex_ref, of_struct

pytestmark = pytest.mark.gpu
TABLE = json.loads((ph.GOLDEN / "pngsuite.json").read_text())
ONLINE = json.loads((ph.GOLDEN / "online.json").read_text())
SIG = b"\x89PNG\r\n\x1a\n"


def chunk(name, data, crc=None):
    return struct.pack(">I", len(data)) + name + data + struct.pack(">I", zlib.crc32(name + data) if crc is None else crc)


IHDR = chunk(b"IHDR", struct.pack(">IIBBBBB", 32, 32, 8, 0, 0, 0, 0))
IEND = chunk(b"IEND", b"")


def payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def chunks_of(data):
    pos, out = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        out.append((n, data[pos + 4:pos + 8]))
        pos += 12 + n
        if out[-1][1] == b"IEND":
            break
    return out


class Batch:
    """files on the device, their IDAT buffers and states; a push is one call for all of them"""

    def __init__(self, s, files, caps=None):
        self.s, self.files = s, files
        self.caps = [max(len(f), 1) for f in files] if caps is None else caps      # idat_cap: the size of the IDAT buffer
        self.d_png = [s.to_device(f) for f in files]
        self.d_idat = [s.empty(cap) for cap in self.caps]
        self.states = s.lex_states(len(files))
        self.summed = self.copied = self.headers = self.pushes = 0

    def push(self, lens, states=None):
        infos = self.s.lex_resume_batch(list(zip(self.d_png, lens, self.d_idat)), self.states if states is None else states)
        a, b, c = self.s.lex_resume_stats()
        self.summed, self.copied, self.headers, self.pushes = self.summed + a, self.copied + b, self.headers + c, self.pushes + 1
        self.last = (a, b, c)
        return infos

    def push_and_compare(self, lens):
        """... and lex_ref on the same prefixes says the same: every field, the padding zero, the IDAT bytes in front of idat_len"""
        infos = self.push(lens)
        for k, (got, f, n) in enumerate(zip(infos, self.files, lens)):
            want, idat = lex_ref(f[:n], self.caps[k])
            assert of_struct(got) == want and bytes(got.pad) == b"\0\0", (k, n, of_struct(got), want)
            assert bytes(self.d_idat[k][:got.idat_len].cpu().numpy()) == idat, (k, n)
        return infos

    def every_byte_once(self):
        """all files are well formed and have been lexed through IEND"""
        cs = [chunks_of(f) for f in self.files]
        assert self.summed == sum(n + 4 for c in cs for n, _ in c)
        assert self.copied == sum(n for c in cs for n, name in c if name == b"IDAT")
        assert self.headers <= sum(len(c) for c in cs) + self.pushes * len(self.files)


def test_every_cut_of_a_small_file_as_one_batch(gpu):
    s = gpu.load()
    data = (ph.GOLDEN / "pngsuite" / "common" / "basn0g01.png").read_bytes()
    n = len(data)
    b = Batch(s, [data] * (n + 1))
    first = b.push_and_compare(list(range(n + 1)))
    assert all(r.status in (gpu.E_TRUNCATED_SIGNATURE, gpu.E_TRUNCATED_CHUNK_HEADER, gpu.E_TRUNCATED_CHUNK_BODY) for r in first[:n])
    last = b.push_and_compare([n] * (n + 1))
    assert all(r.status == 0 and r.consumed == n for r in last)
    b.every_byte_once()


def test_running_crc_at_the_boundaries_of_the_piece_length(gpu):
    s = gpu.load()
    data = SIG + IHDR + chunk(b"IDAT", payload(70000, 1)) + IEND
    at = 8 + len(IHDR)
    sizes = (1, 15, 16, 17, 1023, 1024, 1025, 1040, 65535, 65536, 65537)
    b = Batch(s, [data] * len(sizes))
    b.push_and_compare([at + 8] * len(sizes))
    infos = b.push_and_compare([at + 8 + k for k in sizes])
    assert all(r.status == gpu.E_TRUNCATED_CHUNK_BODY and r.aux[0] == 70004 and r.idat_len == 0 for r in infos)
    assert b.last[:2] == (sum(sizes), sum(sizes))
    infos = b.push_and_compare([len(data)] * len(sizes))
    assert all(r.status == 0 and r.idat_len == 70000 for r in infos)
    b.every_byte_once()
    # one file, every push from the last one's running value
    b = Batch(s, [data])
    pos = at + 8
    b.push_and_compare([pos])
    for k in sizes[:9]:
        pos += k
        b.push_and_compare([pos])
        assert b.last[0] == k
    assert b.push_and_compare([len(data)])[0].status == 0
    b.every_byte_once()


def test_a_chunk_of_several_pieces(gpu):
    """2.5 MiB in one chunk, as (1 MiB + 3, the rest) and in one push; a wrong byte in its last piece"""
    s = gpu.load()
    body = payload(5 << 19, 2)
    data = SIG + IHDR + chunk(b"IDAT", body) + IEND
    at = 8 + len(IHDR)
    bad = bytearray(data); bad[at + 8 + len(body) - 5] ^= 1
    b = Batch(s, [data, data, bytes(bad)])
    infos = b.push_and_compare([at + 8 + (1 << 20) + 3, len(data), at + 8 + (1 << 20) + 3])
    assert [r.status for r in infos] == [gpu.E_TRUNCATED_CHUNK_BODY, 0, gpu.E_TRUNCATED_CHUNK_BODY]
    infos = b.push_and_compare([len(data)] * 3)
    assert [r.status for r in infos] == [0, 0, gpu.E_CHUNK_CHECKSUM]
    assert infos[2].aux[1] == zlib.crc32(bytes(bad[at + 4:at + 8 + len(body)])) and infos[2].idat_len == 0
    assert infos[0].idat_len == infos[1].idat_len == len(body)
    assert b.summed == 3 * (17 + len(body) + 4 + 4) and b.copied == 3 * len(body)     # (each byte once, the damaged file's too)


def test_more_chunks_than_the_list_holds(gpu):
    s = gpu.load()
    data = SIG + IHDR + b"".join(chunk(b"IDAT", bytes([k])) for k in range(200)) + IEND
    b = Batch(s, [data, data])
    b.push_and_compare([len(data), 1000])
    infos = b.push_and_compare([len(data), len(data)])
    assert all(r.status == 0 and r.chunks == 202 and r.idat_len == 200 for r in infos)
    b.every_byte_once()


def test_every_fixture_in_four_pushes(gpu):
    """the 193 fixtures and the reference's invalid files, cut at three seeded random places: a batch per step"""
    s = gpu.load()
    names = sorted(TABLE)
    files = [(ph.GOLDEN / "pngsuite" / n).read_bytes() for n in names]
    invalid = sorted((ph.GOLDEN / "invalid").glob("*.png"))
    files += [p.read_bytes() for p in invalid]
    rng = np.random.default_rng(14)
    cuts = [sorted(int(c) for c in rng.integers(0, len(f) + 1, 3)) + [len(f)] for f in files]
    b = Batch(s, files)
    for step in range(4):
        infos = b.push_and_compare([c[step] for c in cuts])
    for name, f, r in zip(names, files, infos):
        png = ph.parse_png(f)
        assert r.status == 0 and r.idat_len == len(png.idat), name
        assert (r.width, r.height, r.depth, r.color, bool(r.interlace), bool(r.ios)) == (png.width, png.height, png.depth, png.color, png.interlaced, png.ios)
    statuses = {p.stem: r.status for p, r in zip(invalid, infos[len(names):])}
    assert all(statuses[k] == gpu.E_SIGNATURE for k in ("xs1n0g01", "xs2n0g01", "xs4n0g01", "xs7n0g01", "xcrn0g04", "xlfn0g04"))
    assert statuses["xhdn0g08"] == statuses["xcsn0g01"] == gpu.E_CHUNK_CHECKSUM
    # every byte once: what the invalid files add is what they take when they are lexed alone
    alone = Batch(s, files[len(names):])
    for step in range(4):
        alone.push([c[step] for c in cuts[len(names):]])
    cs = [chunks_of(f) for f in files[:len(names)]]
    assert b.summed - alone.summed == sum(n + 4 for c in cs for n, _ in c)
    assert b.copied - alone.copied == sum(n for c in cs for n, name in c if name == b"IDAT")
    assert b.headers - alone.headers <= sum(len(c) for c in cs) + 4 * len(names)


def test_a_batch_whose_files_are_at_different_stages(gpu):
    s = gpu.load()
    body = payload(3000, 3)
    good = SIG + IHDR + chunk(b"IDAT", body) + chunk(b"IDAT", body[:100]) + IEND
    at, n = 8 + len(IHDR), len(good)
    broken = bytearray(good); broken[at + 8 + 10] ^= 0x40
    typed = SIG + IHDR + chunk(b"IDaT", b"xx") + IEND
    files = [good, good, good, bytes(broken), typed, good, good + b"trailing"]
    b = Batch(s, files)
    b.push_and_compare([0, 5, at + 8 + 1000, at + 8 + 1000, at + 3, n, n])
    infos = b.push_and_compare([n, at + 6, at + 8 + 1000, n, at + 8, n, n + 8])
    assert [r.status for r in infos] == [0, gpu.E_TRUNCATED_CHUNK_HEADER, gpu.E_TRUNCATED_CHUNK_BODY, gpu.E_CHUNK_CHECKSUM, gpu.E_CHUNK_TYPE, 0, 0]
    assert b.last[0] == (n - 8 - 8 * 4) + 17 + 0 + (2000 + 104 + 4) + 0 + 0 + 0        # what is new, nothing again
    # final results stay, a push that brings nothing does no work, a null state and a shrinking len are that file's own error
    states = list(b.states)
    states[1] = None
    infos = b.push([n, n, at + 8 + 999, 5, len(typed), n, n], states)
    assert [r.status for r in infos] == [0, gpu.E_ARGUMENT, gpu.E_ARGUMENT, gpu.E_CHUNK_CHECKSUM, gpu.E_CHUNK_TYPE, 0, 0]
    assert b.last == (0, 0, 0)
    infos = b.push_and_compare([n, n, n, n, len(typed), n, n + 8])
    assert [r.status for r in infos] == [0, 0, 0, gpu.E_CHUNK_CHECKSUM, gpu.E_CHUNK_TYPE, 0, 0]
    assert all(r.idat_len == 3100 for r in infos[:3])


def test_idat_cap_one_byte_short_of_the_second_idat(gpu):
    """SPNG_E_OUTPUT_CAPACITY once the chunk is complete, and with its checksum wrong the checksum: the reference's order"""
    s = gpu.load()
    body = payload(3000, 3)
    good = SIG + IHDR + chunk(b"IDAT", body) + chunk(b"IDAT", body[:100]) + IEND
    at, n = 8 + len(IHDR), len(good)
    bad = bytearray(good); bad[at + 12 + 3000 + 8 + 3] ^= 2
    b = Batch(s, [good, bytes(bad), good, bytes(bad)], [3099, 3099, 3099, 3099])
    infos = b.push_and_compare([at + 12 + 3000 + 8 + 60, at + 12 + 3000 + 8 + 60, n, n])
    assert [r.status for r in infos] == [gpu.E_TRUNCATED_CHUNK_BODY, gpu.E_TRUNCATED_CHUNK_BODY, gpu.E_OUTPUT_CAPACITY, gpu.E_CHUNK_CHECKSUM]
    infos = b.push_and_compare([n] * 4)
    assert [r.status for r in infos] == [gpu.E_OUTPUT_CAPACITY, gpu.E_CHUNK_CHECKSUM] * 2
    assert all((r.chunks, r.idat_len, r.consumed) == (2, 3000, at + 12 + 3000) for r in infos)


def test_no_files_and_null_arrays(gpu):
    import ctypes
    s = gpu.load()
    assert s.lex_resume_batch([], []) == []
    assert s.lib.spng_lex_resume_batch(s.ctx, None, None, 1, None, (gpu.Lexed * 1)()) == gpu.E_ARGUMENT
    assert int(s.lib.spng_lex_state_bytes()) % 8 == 0 and s.lex_resume_stats() is not None
    d = (gpu.FileDesc * 1)(gpu.FileDesc(None, 0, None, 0))
    sp = (ctypes.c_void_p * 1)(s.lex_states(1)[0].data_ptr())
    assert s.lib.spng_lex_resume_batch(s.ctx, d, sp, 1, None, None) == gpu.E_ARGUMENT            # nowhere to put the results


@pytest.mark.parametrize("run", sorted(ONLINE))
def test_the_tutorial_from_file_bytes_in_pieces_of_4096(gpu, run, monkeypatch):
    """PNG.decode_online: every capture is the image the reference wrote after the chunk just completed, there are as many captures as
    chunks, every scanline byte is defiltered once and every file byte summed once"""
    s = gpu.load()
    entry = ONLINE[run]
    data = (ph.GOLDEN / "tutorials" / entry["file"]).read_bytes()
    stats, shots, lex = [], [], s.lex_resume_batch

    def counted(files, states):
        infos = lex(files, states)
        stats.append(s.lex_resume_stats())
        return infos

    monkeypatch.setattr(s, "lex_resume_batch", counted)
    context, info, plte, trns = gpu.PNG.decode_online((data[i:i + 4096] for i in range(0, len(data), 4096)), overdraw=entry["overdraw"], session=s,
                                                      capture=lambda c: shots.append(hashlib.sha256(c.storage).hexdigest()))
    assert shots == entry["snapshots"]
    assert info.status == 0 and (info.width, info.height, bool(info.interlace)) == (entry["width"], entry["height"], entry["interlaced"])
    png = ph.parse_png(data)
    assert context.defiltered_total == gpu.inflated_size(png.width, png.height, png.depth, png.channels, png.interlaced)
    st, want, _ = ph.orc_decode(png)
    assert st == 0 and context.storage == want.tobytes() and (plte, trns) == (b"", b"")
    # (a chunk is 12 bytes more than its data, and its type -- 4 of them -- is summed: the signature, 8 bytes per chunk and the bytes
    # summed make the file)
    assert sum(a for a, _, _ in stats) + 8 + 8 * info.chunks == len(data) == info.consumed
    assert sum(b for _, b, _ in stats) == len(png.idat)
    assert sum(c for _, _, c in stats) <= info.chunks + len(stats)


def test_the_tutorial_raises_lexing_errors_once_they_are_final(gpu):
    s = gpu.load()
    data = bytearray((ph.GOLDEN / "tutorials" / "OnlineDecoding.png").read_bytes())
    pieces = lambda d: [bytes(d[i:i + 4096]) for i in range(0, len(d), 4096)]
    with pytest.raises(gpu.LexingError) as e:
        gpu.PNG.decode_online(pieces(data[:50000]), session=s)
    assert e.value.status in (gpu.E_TRUNCATED_CHUNK_HEADER, gpu.E_TRUNCATED_CHUNK_BODY)
    pos, idats = 8, []
    for n, name in chunks_of(bytes(data)):
        idats += [pos] if name == b"IDAT" else []
        pos += 12 + n
    data[idats[3] + 8 + 100] ^= 1                                      # in the fourth IDAT's payload
    shots = []
    with pytest.raises(gpu.LexingError) as e:
        gpu.PNG.decode_online(pieces(data), session=s, capture=lambda c: shots.append(1))
    assert e.value.status == gpu.E_CHUNK_CHECKSUM and len(shots) == 3
