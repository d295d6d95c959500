"""The chunk lexers of csrc/chunks.hip, as written, run on the CPU by the wave emulator of tools/emu: the resumable one
(spng_lex_resume_batch: lexr_walk -> lexr_piece -> lexr_finish) over files that arrive push by push, and the whole-file one
(spng_lex_batch: lex_walk -> lex_chunk -> lex_finish) over prefixes: tools/emu/emu_lex_resume.cpp.  The yardstick is tests/lex_ref.py, the reference's loop in plain Python, on the same prefix with the
same idat_cap -- after every push every field of the result and the IDAT bytes in front of idat_len are its, and the padding is
zero (the `same` column of a Row) --, the statuses are also stated here, and the counters hold "every byte once": over all pushes of a file each byte of type
+ data is summed once, each IDAT byte copied once, however the pushes cut the file.
Twice: a plain build, and one with -fsanitize=address,undefined -- a CPU program of its own, run as a subprocess, nothing preloaded;
every push hands the kernels a copy of exactly the prefix, so a read behind the bytes that have arrived is seen."""
import struct
import subprocess
import zlib
from collections import namedtuple

import numpy as np
import pytest

import emu_build
import pnghelp as ph
from lex_ref import lex_ref

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
            "-DEMU_UCONTEXT")
ENV = {"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
(DONE, E_OUTPUT_CAPACITY, E_ARGUMENT, E_TRUNCATED_SIGNATURE, E_SIGNATURE, E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_CHUNK_BODY, E_CHUNK_TYPE,
 E_CHUNK_CHECKSUM) = 0, 64, 65, 80, 81, 82, 83, 84, 85
WAITS = (E_TRUNCATED_SIGNATURE, E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_CHUNK_BODY)
SIG = b"\x89PNG\r\n\x1a\n"
MAGIC = b"LEXR"                                             # the first word of a state somebody has written (csrc/chunks.hip: LEX_MAGIC)
Row = namedtuple("Row", "status chunks aux0 aux1 width height depth color compression filter interlace ios idat_len plte_off plte_len trns_off "
                        "trns_len consumed pad0 pad1 summed copied headers same")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emu(request, tmp_path_factory):
    flags = ("-fpermissive", "-Wno-attributes") + (SANITIZE if request.param == "sanitized" else ())
    return emu_build.build_plain(tmp_path_factory, "chunks.hip", "emu_lex_resume.cpp", "EMU_LEX_RESUME_SRC", "-O1", compiler="g++", flags=flags)


def chunk(name, data, crc=None):
    return struct.pack(">I", len(data)) + name + data + struct.pack(">I", zlib.crc32(name + data) if crc is None else crc)


IHDR = chunk(b"IHDR", struct.pack(">IIBBBBB", 32, 32, 8, 0, 0, 0, 0))
IEND = chunk(b"IEND", b"")


def payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def run(emu, tmp_path, data, script, timeout=900):
    """-> (the Row of every push and every whole, the `total` lines: (summed, copied, headers, pushes)).  Row.same: all 18 fields of the
    result are those of lex_ref on the same prefix with the same idat_cap, so are the IDAT bytes in front of idat_len, and the two
    padding bytes of spng_lexed are zero"""
    (tmp_path / "f.png").write_bytes(data)
    (tmp_path / "s.txt").write_text("\n".join(script) + "\n")
    r = subprocess.run([str(emu), str(tmp_path / "f.png"), str(tmp_path / "s.txt"), str(tmp_path / "idat")], capture_output=True, text=True,
                       timeout=timeout, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lexed = [s.split() for s in script if s.startswith(("push", "whole", "cap", "flip"))]
    idats, pos = (tmp_path / "idat").read_bytes(), 0
    data, cap = bytearray(data), len(data)
    rows, totals = [], []
    for line in r.stdout.splitlines():
        v = line.split()
        if len(v) == 4:
            totals.append(tuple(int(x) for x in v))
            continue
        while lexed[0][0] in ("cap", "flip"):
            cmd, *args = lexed.pop(0)
            if cmd == "cap":
                cap = int(args[0])
            else:
                data[int(args[0])] ^= int(args[1])
        got = [int(x, 16) if k in (2, 3) else int(x) for k, x in enumerate(v)]
        want, want_idat = lex_ref(bytes(data[:int(lexed.pop(0)[1])]), cap)
        rows.append(Row(*got, same=tuple(got[:18]) == tuple(want) and got[18:20] == [0, 0] and idats[pos:pos + got[12]] == want_idat))
        pos += got[12]
    assert pos == len(idats) and not [c for c in lexed if c[0] in ("push", "whole")]
    assert len(rows) == sum(s.startswith(("push", "whole")) for s in script) and len(totals) == sum(s == "total" for s in script)
    return rows, totals


def chunks_of(data):
    """[(offset, length, name)] of a well-formed file"""
    pos, out = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        out.append((pos, n, data[pos + 4:pos + 8]))
        pos += 12 + n
    return out


def every_byte_once(data, total):
    """the counters of a file lexed through IEND over `total[3]` pushes"""
    cs = chunks_of(data)
    assert total[0] == sum(n + 4 for _, n, _ in cs)
    assert total[1] == sum(n for _, n, name in cs if name == b"IDAT")
    assert total[2] <= len(cs) + total[3]


def test_every_cut_of_a_small_file(emu, tmp_path):
    """[0, c) and then the whole file, for every c: inside the signature, a length, a type, a payload, a checksum"""
    data = (ph.GOLDEN / "pngsuite" / "common" / "basn0g01.png").read_bytes()
    n = len(data)
    script = []
    for c in range(n + 1):
        script += ["reset", f"push {c}", f"push {n}", "total"]
    rows, totals = run(emu, tmp_path, data, script)
    for c in range(n + 1):
        first, second = rows[2 * c], rows[2 * c + 1]
        assert first.same and second.same, c
        assert first.status in WAITS if c < n else first.status == DONE, c
        assert second.status == DONE and second.idat_len == len(ph.parse_png(data).idat) and second.consumed == n
        every_byte_once(data, totals[c])


def test_running_crc_at_the_boundaries_of_the_piece_length(emu, tmp_path):
    """one IDAT of 70 000 bytes cut so that a push sums 1, 15, 16, 17, 1023 ... 65537 bytes from a running value: where wave_crc32's
    piece length changes.  (The first sum of a chunk is never shorter than its type: a header is lexed once it is whole.)"""
    data = SIG + IHDR + chunk(b"IDAT", payload(70000, 1)) + IEND
    at = 8 + len(IHDR)
    sizes = (1, 15, 16, 17, 1023, 1024, 1025, 1040, 65535, 65536, 65537)
    for k in sizes:
        rows, totals = run(emu, tmp_path, data, ["reset", f"push {at + 8}", f"push {at + 8 + k}", f"push {len(data)}", "total"])
        assert all(r.same for r in rows), k
        assert [r.status for r in rows] == [E_TRUNCATED_CHUNK_BODY, E_TRUNCATED_CHUNK_BODY, DONE] and rows[1].aux0 == 70004, k
        assert (rows[0].summed, rows[0].copied) == (17 + 4, 0) and (rows[1].summed, rows[1].copied, rows[1].idat_len) == (k, k, 0), k
        assert rows[2].idat_len == 70000 and rows[2].summed == 70000 - k + 4, k
        every_byte_once(data, totals[0])
    # ... and behind one another, every push from the last one's running value; then with the chunk's first sum of that length
    cuts, pos = [], at + 8
    for k in sizes[:9]:
        pos += k
        cuts.append(pos)
    rows, totals = run(emu, tmp_path, data, ["reset", f"push {at + 8}"] + [f"push {c}" for c in cuts] + [f"push {len(data)}", "total"])
    assert all(r.same for r in rows) and rows[-1].status == DONE and [r.summed for r in rows[1:10]] == list(sizes[:9])
    every_byte_once(data, totals[0])
    for k in sizes[1:]:
        rows, totals = run(emu, tmp_path, data, ["reset", f"push {at + 4 + k}", f"push {len(data)}", "total"])
        assert all(r.same for r in rows) and rows[0].summed == 17 + k and rows[1].status == DONE, k
        every_byte_once(data, totals[0])


def test_a_chunk_of_several_pieces_is_folded(emu, tmp_path):
    """2.5 MiB in one chunk: pushed as (1 MiB + 3, the rest) and in one push -- pieces of 1 MiB, a wave each, folded by the finish"""
    body = payload(5 << 19, 2)
    data = SIG + IHDR + chunk(b"IDAT", body) + IEND
    at = 8 + len(IHDR)
    rows, totals = run(emu, tmp_path, data, ["reset", f"push {at + 8 + (1 << 20) + 3}", f"push {len(data)}", "total",
                                             "reset", f"push {len(data)}", "total"])
    assert [r.status for r in rows] == [E_TRUNCATED_CHUNK_BODY, DONE, DONE] and all(r.same for r in rows)
    assert rows[0].summed == 17 + 4 + (1 << 20) + 3 and rows[0].copied == (1 << 20) + 3
    assert rows[1].idat_len == rows[2].idat_len == len(body)
    every_byte_once(data, totals[0])
    every_byte_once(data, totals[1])
    # a wrong byte in the last piece is found by the fold
    bad = bytearray(data); bad[at + 8 + len(body) - 5] ^= 1
    rows, _ = run(emu, tmp_path, bytes(bad), ["reset", f"push {at + 8 + (1 << 20) + 3}", f"push {len(data)}"])
    assert rows[1].status == E_CHUNK_CHECKSUM and rows[1].same and rows[1].aux1 == zlib.crc32(bytes(bad[at + 4:at + 8 + len(body)]))
    assert rows[1].idat_len == 0 and rows[1].chunks == 1


@pytest.mark.parametrize("listed", [None, 7, 0])
def test_more_chunks_than_the_list_holds(emu, tmp_path, listed):
    """200 chunks of twelve bytes in one push: what the list does not hold the walking wave sums itself"""
    data = SIG + IHDR + b"".join(chunk(b"IDAT", b"") for _ in range(200)) + IEND
    pre = [] if listed is None else [f"list {listed}"]
    rows, totals = run(emu, tmp_path, data, pre + ["reset", f"push {len(data)}", "total", "reset", "push 1000", f"push {len(data)}", "total"])
    assert all(r.same for r in rows) and rows[0].status == rows[2].status == DONE and rows[0].chunks == 202
    every_byte_once(data, totals[0])
    every_byte_once(data, totals[1])


def test_overflowing_chunks_with_payloads_and_a_tail_in_progress(emu, tmp_path):
    """a list of two entries: the chunks behind it, the one the input ends in among them, are summed and copied by the walking wave,
    whose running value the next push takes up"""
    parts = [payload(n, 10 + n) for n in (5, 300, 70000, 17, 2000)]
    data = SIG + IHDR + b"".join(chunk(b"IDAT", q) for q in parts) + IEND
    cuts = [8 + len(IHDR) + 12 + 5 + 12 + 300 + 8 + 33000, len(data) - 1500, len(data)]
    rows, totals = run(emu, tmp_path, data, ["list 2", "reset"] + [f"push {c}" for c in cuts] + ["total"])
    assert all(r.same for r in rows) and [r.status for r in rows] == [E_TRUNCATED_CHUNK_BODY, E_TRUNCATED_CHUNK_BODY, DONE]
    assert rows[-1].idat_len == sum(len(q) for q in parts)
    every_byte_once(data, totals[0])


def test_damage(emu, tmp_path):
    body = payload(3000, 3)
    good = SIG + IHDR + chunk(b"IDAT", body) + chunk(b"IDAT", body[:100]) + IEND
    n = len(good)
    at = 8 + len(IHDR)
    # a flipped byte in a chunk that straddles two pushes; the result stays for good
    bad = bytearray(good); bad[at + 8 + 10] ^= 0x40
    rows, totals = run(emu, tmp_path, bytes(bad), ["reset", f"push {at + 8 + 1000}", f"push {n}", f"push {n}", f"push {n - 1}", "total"])
    assert rows[0].status == E_TRUNCATED_CHUNK_BODY and rows[0].same
    for r in rows[1:]:
        assert (r.status, r.aux0, r.aux1) == (E_CHUNK_CHECKSUM, zlib.crc32(b"IDAT" + body), zlib.crc32(bytes(bad[at + 4:at + 8 + 3000])))
        assert (r.chunks, r.idat_len, r.consumed) == (1, 0, at)
    assert rows[1].same and rows[2].same and (rows[2].summed, rows[2].copied, rows[2].headers) == (0, 0, 0)
    assert totals[0][0] == sum(k + 4 for _, k, _ in chunks_of(good)) and totals[0][1] == 3100      # (each byte once, the bad chunk's too)

    # a bad checksum in chunk 3 and a bad type in chunk 5 of one push: the checksum wins
    cs = [IHDR, chunk(b"gAMA", b"\0\0\0\1"), chunk(b"IDAT", body), chunk(b"IDAT", body[:50], crc=5), chunk(b"IDAT", body[:7]),
          chunk(b"IDaT", b"xx"), IEND]
    data = SIG + b"".join(cs)
    rows, _ = run(emu, tmp_path, data, ["reset", "push 20", f"push {len(data)}", f"push {len(data)}"])
    for r in rows[1:]:
        assert (r.status, r.aux0, r.aux1, r.chunks, r.idat_len) == (E_CHUNK_CHECKSUM, 5, zlib.crc32(b"IDAT" + body[:50]), 3, 3000)
    assert rows[1].same and rows[2].headers == 0
    # ... alone, the bad type is reported, already with nothing but its header there; and stays
    cs[3] = chunk(b"IDAT", body[:50])
    data = SIG + b"".join(cs)
    upto = 8 + sum(len(c) for c in cs[:5])
    rows, _ = run(emu, tmp_path, data, ["reset", f"push {upto + 3}", f"push {upto + 8}", f"push {len(data)}"])
    assert rows[0].status == E_TRUNCATED_CHUNK_HEADER and rows[0].same
    for r in rows[1:]:
        assert (r.status, r.aux0, r.chunks, r.idat_len, r.consumed) == (E_CHUNK_TYPE, struct.unpack(">I", b"IDaT")[0], 5, 3057, upto)
    assert rows[1].same and rows[2].same and rows[2].headers == 0

    # a bad signature: known with its eighth byte, and for good
    data = b"\x89PNG\r\n\x1a\r" + good[8:]
    rows, _ = run(emu, tmp_path, data, ["reset", "push 7", "push 8", f"push {n}"])
    assert rows[0].status == E_TRUNCATED_SIGNATURE and rows[0].same and rows[0].consumed == 7
    for r in rows[1:]:
        assert (r.status, r.aux0, r.consumed) == (E_SIGNATURE, struct.unpack(">Q", data[:8])[0], 8)
    assert rows[1].same and rows[2].same

    # idat_cap exceeded by the second IDAT: SPNG_E_OUTPUT_CAPACITY once it is complete -- its checksum first
    for broken in (False, True):
        data = bytearray(good)
        if broken:
            data[at + 12 + 3000 + 8 + 3] ^= 2
        rows, totals = run(emu, tmp_path, bytes(data), ["cap 3050", "reset", f"push {at + 12 + 3000 + 8 + 60}", f"push {n}", f"push {n}", "total"])
        assert rows[0].status == E_TRUNCATED_CHUNK_BODY and rows[0].same and rows[0].idat_len == 3000 and rows[0].copied == 3000
        for r in rows[1:]:
            assert r.status == (E_CHUNK_CHECKSUM if broken else E_OUTPUT_CAPACITY) and (r.chunks, r.idat_len) == (2, 3000)
        assert rows[1].same and rows[2].same and rows[2].summed == 0
        assert totals[0][0] == 17 + 3004 + 104 and totals[0][1] == 3000

    # bytes behind IEND are ignored; a push that brings nothing repeats the answer and does no work
    rows, totals = run(emu, tmp_path, good + b"trailing bytes", ["reset", f"push {n - 20}", f"push {n - 20}", f"push {n}", f"push {n + 14}", "total"])
    assert rows[0] == rows[1]._replace(summed=rows[0].summed, copied=rows[0].copied, headers=rows[0].headers) and rows[1].same
    assert (rows[1].summed, rows[1].copied) == (0, 0) and rows[1].headers <= 1
    assert rows[2].status == rows[3].status == DONE and rows[2].same and rows[3].same and rows[3].consumed == n
    assert (rows[3].summed, rows[3].copied, rows[3].headers) == (0, 0, 0)
    every_byte_once(good, totals[0])


def test_arguments_that_only_the_device_sees(emu, tmp_path):
    """a len smaller than what the state has consumed, a state whose fields contradict each other, a null state: SPNG_E_ARGUMENT in
    that file's status, and the state stays as it was"""
    body = payload(3000, 4)
    good = SIG + IHDR + chunk(b"IDAT", body) + IEND
    n = len(good)
    at = 8 + len(IHDR)
    rows, totals = run(emu, tmp_path, good, ["reset", f"push {at + 8 + 1000}", f"push {at + 8 + 999}", f"push {at + 8}", "nostate", f"push {n}",
                                             f"push {n}", f"push {at}", "total"])
    assert [r.status for r in rows] == [E_TRUNCATED_CHUNK_BODY, E_ARGUMENT, E_ARGUMENT, E_ARGUMENT, DONE, E_ARGUMENT]
    assert rows[4].same and rows[4].idat_len == 3000
    every_byte_once(good, totals[0])
    # a header that has arrived in part has not been consumed: fewer bytes of it are a smaller prefix, nothing else
    rows, _ = run(emu, tmp_path, good, ["reset", f"push {at + 6}", f"push {at + 2}", f"push {n}"])
    assert [r.status for r in rows] == [E_TRUNCATED_CHUNK_HEADER, E_TRUNCATED_CHUNK_HEADER, DONE] and all(r.same for r in rows)
    # states nobody wrote: a wrong magic word, a chunk in progress behind a signature nobody has seen
    rows, _ = run(emu, tmp_path, good, ["reset", "poke 0 7", f"push {n}", "reset"] + [f"poke {k} {v}" for k, v in enumerate(MAGIC)] + ["poke 24 9", f"push {n}", "reset", f"push {n}"])
    assert [r.status for r in rows] == [E_ARGUMENT, E_ARGUMENT, DONE]


def test_whole_files_every_prefix(emu, tmp_path):
    """the whole-file entry on every prefix of a small file, with a list that holds everything and one of two entries"""
    data = (ph.GOLDEN / "pngsuite" / "common" / "basn0g01.png").read_bytes()
    n = len(data)
    for pre in ([], ["list 2"]):
        rows, _ = run(emu, tmp_path, data, pre + [f"whole {c}" for c in range(n + 1)])
        assert all(r.same for r in rows), [c for c, r in enumerate(rows) if not r.same]
        assert all(r.status in WAITS for r in rows[:n]) and rows[n].status == DONE and rows[n].consumed == n
        assert all((r.summed, r.copied, r.headers) == (0, 0, 0) for r in rows)       # (no counter is added for whole files)


def test_whole_files_long_chunks_list_overflow_and_idat_cap(emu, tmp_path):
    """a chunk of 2.5 MiB, more chunks than the list holds, idat_cap: from the whole-file entry"""
    body = payload(5 << 19, 2)
    data = SIG + IHDR + chunk(b"IDAT", body) + IEND
    at = 8 + len(IHDR)
    rows, _ = run(emu, tmp_path, data, [f"whole {len(data)}", f"flip {at + 8 + len(body) - 5} 1", f"whole {len(data)}", f"whole {len(data) - 13}"])
    assert [r.status for r in rows] == [DONE, E_CHUNK_CHECKSUM, E_TRUNCATED_CHUNK_BODY] and all(r.same for r in rows)
    bad = bytearray(data); bad[at + 8 + len(body) - 5] ^= 1
    assert rows[0].idat_len == len(body) and rows[1].aux1 == zlib.crc32(bytes(bad[at + 4:at + 8 + len(body)])) and rows[1].idat_len == 0
    # 200 IDAT chunks of one byte: lex_listed gives 65 entries
    data = SIG + IHDR + b"".join(chunk(b"IDAT", bytes([k])) for k in range(200)) + IEND
    rows, _ = run(emu, tmp_path, data, [f"whole {len(data)}", f"flip {8 + len(IHDR) + 150 * 13 + 8} 4", f"whole {len(data)}"])
    assert all(r.same for r in rows) and (rows[0].status, rows[0].chunks, rows[0].idat_len) == (DONE, 202, 200)
    assert (rows[1].status, rows[1].chunks, rows[1].idat_len) == (E_CHUNK_CHECKSUM, 151, 150)
    # idat_cap one byte short of the second IDAT: capacity, and with that chunk's checksum wrong the checksum
    body = payload(3000, 3)
    good = SIG + IHDR + chunk(b"IDAT", body) + chunk(b"IDAT", body[:100]) + IEND
    for listed in (None, 1):
        pre = [] if listed is None else [f"list {listed}"]
        rows, _ = run(emu, tmp_path, good, pre + ["cap 3099", f"whole {len(good)}", f"flip {at + 12 + 3000 + 8 + 3} 2", f"whole {len(good)}", "cap 3100",
                                                  f"whole {len(good)}"])
        assert [r.status for r in rows] == [E_OUTPUT_CAPACITY, E_CHUNK_CHECKSUM, E_CHUNK_CHECKSUM] and all(r.same for r in rows), listed
        assert all((r.chunks, r.idat_len, r.consumed) == (2, 3000, at + 12 + 3000) for r in rows)


def test_what_lies_behind_the_first_failure_is_not_reported(emu, tmp_path):
    """CgBI, IHDR, PLTE, tRNS, IDAT, IEND with the checksum of each chunk wrong in turn, as a whole file and in two pushes: the walk has
    noted the fields of all of them by the time a wave finds the checksum; the answer holds those in front of the failure only"""
    cs = [chunk(b"CgBI", b"\0\0\0\1"), IHDR, chunk(b"PLTE", b"abcdef"), chunk(b"tRNS", b"xy"), chunk(b"IDAT", payload(50, 5)), IEND]
    data = SIG + b"".join(cs)
    n, script, at = len(data), [], 8
    for c in cs:
        script += [f"flip {at + 8} 16", f"whole {n}", "reset", f"push {at + 9}", f"push {n}", f"flip {at + 8} 16"]
        at += len(c)
    rows, _ = run(emu, tmp_path, data, script[:-6] + [f"whole {n}"])      # (IEND has no data to damage: lexed whole instead)
    assert all(r.same for r in rows), [k for k, r in enumerate(rows) if not r.same]
    for k in range(5):
        for r in (rows[3 * k], rows[3 * k + 2]):
            assert (r.status, r.chunks) == (E_CHUNK_CHECKSUM, k), k
            assert (r.ios, r.width, r.plte_len, r.trns_len, r.idat_len) == (int(k > 0), 32 * (k > 1), 6 * (k > 2), 2 * (k > 3), 0), k
    assert (rows[-1].status, rows[-1].chunks, rows[-1].ios, rows[-1].width, rows[-1].plte_len, rows[-1].trns_len, rows[-1].idat_len) == (DONE, 6, 1, 32, 6, 2, 50)
