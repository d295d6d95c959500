"""The case table of the file writer (spng_write_file_batch: wfile_body_kernel -> wfile_finish_kernel of csrc/chunks.hip), shared by the
emulator's run of it (tests/test_emu_write_file.py) and the device's (tests/test_gpu_write_file.py), with what every case must answer --
the bytes from tests/file_ref.py, and every file written lexed by tests/lex_ref.py to SPNG_DONE with its stream back out.  The smallest
shapes that can go wrong: chunk lengths around the 16-byte unit of the copy and the two the reference's files have, stream lengths
around a chunk's end, every residue mod 16 of head length, output and stream address (the copy aligns on the destination, whose offset
against the source changes from chunk to chunk), capacities exact and one short, lengths that exist on the device only, chunks longer
than the 1 MiB piece a wave sums."""
import functools
from collections import namedtuple

import numpy as np

import file_ref
from lex_ref import lex_ref

DONE, NEED_MORE_INPUT, E_STRING_REFERENCE, E_OUTPUT_CAPACITY, E_ARGUMENT = 0, 1, 39, 64, 65
PIECE = 1 << 20
CHUNK_BYTES = (1, 2, 15, 16, 17, 8200, 65544)
# name; kw: what file_ref.head takes (and a spng_png_desc names); head: its bytes; buffer: the stream's buffer (ends where the
# allocation ends); n: the stream's length; src: None (n is a host value) or the spng_result (status, written, aux0, aux1) it is read
# from; *_res: the addresses' residues mod 16
Case = namedtuple("Case", "name kw head buffer n stream_cap chunk_bytes head_res stream_res out_res out_cap src")


@functools.lru_cache(maxsize=None)
def noise():
    return np.random.default_rng(20).integers(0, 256, (4 << 20) + 4096, dtype=np.uint8).tobytes()


def head_kw(residue=None, fmt="rgb8"):
    """inputs of a head; residue: its length mod 16 (a tEXt blob of the length that takes)"""
    f = file_ref.FORMATS[fmt]
    kw = dict(width=640, height=480, depth=f.depth, channels=f.channels, indexed=f.indexed, bgr=f.bgr, interlaced=0, palette=[], key=None, fill=None,
              before=[], after=[])
    if f.indexed:
        kw["palette"] = [(k, 2 * k, 3 * k, 255 if k else 9) for k in range(1 << min(f.depth, 4))]
    if residue is not None:
        base = len(file_ref.head(**kw)) + 12
        kw["after"] = [(b"tEXt", noise()[100:100 + (residue - base) % 16 + 16])]
    return kw


def need(c, n=None):
    n = c.n if n is None else n
    return 8 + len(c.head) + n + 12 * -(-n // c.chunk_bytes) + 12


def make(name, chunk_bytes, n, kw=None, stream_cap=None, head_res=0, stream_res=0, out_res=0, short=0, src=None, at=0):
    kw = kw or head_kw()
    head = file_ref.head(**kw)
    c = Case(name, kw, head, noise()[at:at + n], n, n if stream_cap is None else stream_cap, chunk_bytes, head_res % 16, stream_res % 16, out_res % 16, 0, src)
    return c._replace(out_cap=need(c) - short)


def length_cases():
    out = []
    for c in CHUNK_BYTES:
        for k, n in enumerate(sorted({1, c - 1, c, c + 1, 2 * c, 3 * c + 5} - {0})):
            out.append(make(f"c={c} n={n}", c, n, head_res=3 * k + c, stream_res=5 * k + 1, out_res=7 * k + c, at=k))
    return out


def residue_cases():
    out = []
    for c, n in ((17, 3 * 17 + 5), (8200, 8201), (16, 32)):
        for r in range(16):
            out.append(make(f"c={c} head={r}", c, n, kw=head_kw(r), head_res=7 * r + 1, stream_res=11 * r + 7, out_res=5 * r + 3))
            out.append(make(f"c={c} out={r}", c, n, out_res=r, stream_res=3))
            out.append(make(f"c={c} stream={r}", c, n, stream_res=r, out_res=9))
            out.append(make(f"c={c} headaddr={r}", c, n, head_res=r))
    return out


def capacity_cases():
    return [make(f"short c={c} n={n}", c, n, short=1, out_res=c) for c, n in ((1, 1), (16, 33), (8200, 8200), (65544, 65545), (0x7fffffff, 70000))] + \
           [make("short by the whole file", 16, 40, short=need(make("", 16, 40))), make("exact beside them", 16, 33)]


def source_cases():
    far = 1 << 22
    return [make("device length", 8200, 20000, src=(DONE, 20000, 0, 0), stream_res=5),
            make("device length, capacity far above", 65544, 70001, stream_cap=far, src=(DONE, 70001, 0, 0), out_res=2),
            make("device length, one chunk, capacity far above", 0x7fffffff, 4097, stream_cap=far, src=(DONE, 4097, 0, 0)),
            make("host length, capacity above", 17, 100, stream_cap=400),
            make("need more input", 8200, 300, src=(NEED_MORE_INPUT, 300, 5, 6)),
            make("an error status", 16, 300, src=(E_STRING_REFERENCE, 12, 7, 0)),
            make("output capacity upstream", 16, 300, src=(E_OUTPUT_CAPACITY, 1 << 40, 0, 0)),
            make("device length 0", 16, 300, src=(DONE, 0, 0, 0)),
            make("device length behind the capacity", 16, 300, src=(DONE, 301, 0, 0)),
            make("host length 0", 16, 0)]


def fold_cases():
    c = 0x7fffffff
    return [make(f"one chunk n={n}", c, n, stream_res=k + 1, out_res=13 - k, kw=head_kw(k)) for k, n in enumerate((PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 17))] + \
           [make("chunks of two pieces, a short last one", PIECE + 5, 2 * (PIECE + 5) + 9, stream_res=9),
            make("chunks of two pieces, the last one too", PIECE + 5, (PIECE + 5) + PIECE + 3, out_res=6, stream_cap=3 * PIECE)]


def mixed_batch():
    lengths, residues = length_cases(), residue_cases()
    # (but for the stream whose capacity asks for 65 workgroups per file: the emulator runs every one of them for every file)
    sources = [c for c in source_cases() if c.stream_cap < 1 << 22 or c.chunk_bytes > PIECE]
    return (lengths[::5] + residues[::7] + capacity_cases() + sources + fold_cases()[1:3] + [fold_cases()[4]] +
            [make("indexed, interlaced", 8200, 8199, kw=dict(head_kw(fmt="indexed4"), interlaced=1, fill=1)),
             make("bgr8 with a key", 65544, 65544, kw=dict(head_kw(5, fmt="bgr8"), key=(1, 2, 3)))])


def expected(c):
    """-> ((status, written, consumed, aux0, aux1), file bytes or None)"""
    n = c.n
    if c.src is not None:
        status, n, aux0, aux1 = c.src
        if status != DONE:
            return (status, 0, 0, aux0, aux1), None
    if n == 0 or n > c.stream_cap:
        return (E_ARGUMENT, 0, 0, 0, 0), None
    if need(c, n) > c.out_cap:
        return (E_OUTPUT_CAPACITY, need(c, n), 0, 0, 0), None
    return (DONE, need(c, n), n, -(-n // c.chunk_bytes), 0), file_ref.SIG + c.head + file_ref.body(c.buffer[:n], c.chunk_bytes) + file_ref.chunk(b"IEND")


def check_row(c, row, data):
    """row: (status, written, consumed, aux0, aux1) as the writer answered; data: the bytes it wrote (SPNG_DONE only)"""
    want, want_file = expected(c)
    assert tuple(row) == want, (c.name, row, want)
    if want_file is None:
        return
    if data != want_file:
        at = next((k for k, (a, b) in enumerate(zip(data, want_file)) if a != b), min(len(data), len(want_file)))
        raise AssertionError(f"{c.name}: the file differs from byte {at} on ({len(data)} bytes, {len(want_file)} expected)")
    lexed, idat = lex_ref(data, len(data))
    assert lexed.status == DONE and lexed.consumed == len(data) and idat == c.buffer[:row[2]], c.name
