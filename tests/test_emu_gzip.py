"""The kernels of csrc/gzip.hip, as written, run on the CPU by the wave emulator of tools/emu (tools/emu/emu_gzip.cpp): the header parser
over the header table of tests/checksum_cases.py against oracle/gzip_wrap.py's read_header, the CRC-32 in 256 pieces and the Adler-32 of
resumed streams over every payload of the table against Python's zlib, and the trailer writer at every capacity that cuts the eight
trailer bytes.  Twice: a plain build, and one with -fsanitize=address,undefined -- a CPU program of its own, run as a subprocess,
nothing preloaded; every source and destination is a heap buffer of exactly its bytes."""
import subprocess
import zlib

import pytest

import checksum_cases as cc
import emu_build
from test_emu_lex_resume import ENV, SANITIZE
from test_oracle_gzip import gw

E_OUTPUT_CAPACITY = 64


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emu(request, tmp_path_factory):
    flags = ("-fpermissive", "-Wno-attributes") + (SANITIZE if request.param == "sanitized" else ())
    return emu_build.build_plain(tmp_path_factory, "gzip.hip", "emu_gzip.cpp", "EMU_GZIP_SRC", "-O1", compiler="g++", flags=flags)


def run(emu, *args):
    r = subprocess.run([str(emu)] + [str(a) for a in args], capture_output=True, text=True, timeout=900, env=ENV)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def test_header_table_in_one_launch(emu, tmp_path):
    """every row of the header table, one thread each: status, aux, payload offset, and how the job's and the stream's windows moved"""
    rows = cc.header_rows()
    (tmp_path / "heads").write_bytes(b"".join(z for _, z, _ in rows))
    (tmp_path / "lens").write_text("".join("%d\n" % len(z) for _, z, _ in rows))
    lines = run(emu, "pre", tmp_path / "heads", tmp_path / "lens")
    assert len(lines) == len(rows)
    seen = set()
    for (name, z, _), line in zip(rows, lines):
        status, aux0, gz, job_off, job_len, job_fmt, st_off, st_len, st_fmt, done = (int(x) for x in line.split())
        want, want_aux, off = gw.read_header(z)
        seen.add(want)
        if want == gw.DONE:
            assert (status, done, gz) == (0, 0, off), (name, line)
            assert (job_off, job_len, job_fmt) == (off, len(z) - off, cc.RAW) and (st_off, st_len, st_fmt) == (off, len(z) - off, cc.RAW), (name, line)
        else:
            assert (status, aux0, done, gz) == (want, want_aux, 1, -1), (name, line, want, want_aux)
            assert (job_off, job_len, job_fmt) == (0, len(z), cc.GZIP) and (st_off, st_len, st_fmt) == (0, 0, cc.RAW), (name, line)
    assert seen == {gw.DONE, gw.NEED_MORE_INPUT, gw.E_GZIP_SIGIL, gw.E_GZIP_METHOD, gw.E_GZIP_FLAG_BITS, gw.E_GZIP_HEADER_CHECKSUM}


@pytest.mark.parametrize("name", cc.PAYLOADS)
def test_crc_and_adler_of_every_payload(emu, tmp_path, name):
    """piece_crc + fold_pieces against zlib.crc32; resume_adler_kernel + resume_post_kernel against zlib.adler32: the right sum declared is
    accepted, one flipped bit is answered with (declared, the right sum)"""
    data = cc.payload(name)
    (tmp_path / "d").write_bytes(data)
    assert run(emu, "crc", tmp_path / "d") == ["%08x" % zlib.crc32(data)]
    good = zlib.adler32(data)
    assert run(emu, "adler", tmp_path / "d", "%x" % good) == ["0 0 0"]
    bad = good ^ 1 << cc.seed_of(name) % 32
    assert run(emu, "adler", tmp_path / "d", "%x" % bad) == ["%d %x %x" % (cc.E_STREAM_CHECKSUM, bad, good)]


@pytest.mark.parametrize("name", ["tiny-0", "tiny-1", "s1-zero", "gz-257", "gz-65537"])
def test_trailer_at_every_capacity_that_cuts_it(emu, tmp_path, name):
    """gzip_deflate_post_kernel: the bytes of CRC-32 + ISIZE in front of dst_cap are stored, written counts all eight, and only the
    capacity that holds them all answers SPNG_DONE"""
    data = cc.payload(name)
    (tmp_path / "d").write_bytes(data)
    trailer = (zlib.crc32(data).to_bytes(4, "little") + len(data).to_bytes(4, "little")).hex()
    for body in (0, 5):
        lines = run(emu, "trailer", tmp_path / "d", body)
        assert lines == ["%d %d %s" % (E_OUTPUT_CAPACITY if c < 8 else 0, body + 8, trailer[:2 * c] or "-") for c in range(9)], (name, body, lines)
