"""The file writer of csrc/chunks.hip (wfile_body_kernel -> wfile_finish_kernel: spng_write_file_batch), as written, run on the CPU by the
wave emulator of tools/emu: tools/emu/emu_write_file.cpp.  Expected bytes come from tests/file_ref.py; every file written is also lexed by
tests/lex_ref.py to SPNG_DONE with the stream back out byte for byte.  Twice: a plain build, and one with -fsanitize=address,undefined --
a CPU program of its own, run as a subprocess, nothing preloaded; every buffer ends where its allocation ends and has guard bytes in
front (write_file_cases.py lays the cases out; tests/test_gpu_write_file.py runs the same table on the device)."""
import subprocess

import pytest

import emu_build
import write_file_cases as wc

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
            "-DEMU_UCONTEXT")
ENV = {"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emu(request, tmp_path_factory):
    flags = ("-fpermissive", "-Wno-attributes") + (SANITIZE if request.param == "sanitized" else ())
    return emu_build.build_plain(tmp_path_factory, "chunks.hip", "emu_write_file.cpp", "EMU_WRITE_FILE_SRC", "-O1", compiler="g++", flags=flags)


def run(emu, tmp_path, batches, blocks_x=0, timeout=900):
    """batches: lists of cases, each list one launch -> per case (status, written, consumed, aux0, aux1, clean, file bytes)"""
    blob, script = bytearray(), []
    for cases in batches:
        for c in cases:
            head_off = len(blob); blob += c.head
            stream_off = len(blob); blob += c.buffer
            script.append("file " + " ".join(str(int(x)) for x in (
                head_off, len(c.head), c.head_res, stream_off, len(c.buffer), c.stream_res, 0 if c.src else c.n, c.stream_cap, c.chunk_bytes,
                c.out_cap, c.out_res, c.out_cap, int(c.src is not None), *(c.src or (0, 0, 0, 0)))))
        script.append(f"run {blocks_x}")
    (tmp_path / "blob").write_bytes(bytes(blob))
    (tmp_path / "script").write_text("\n".join(script) + "\n")
    r = subprocess.run([str(emu), str(tmp_path / "script"), str(tmp_path / "blob"), str(tmp_path / "files")], capture_output=True, text=True,
                       timeout=timeout, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    files, pos, rows = (tmp_path / "files").read_bytes(), 0, []
    for out in r.stdout.splitlines():
        v = [int(x) for x in out.split()]
        kept = v[1] if v[0] == wc.DONE else 0
        rows.append(tuple(v) + (files[pos:pos + kept],))
        pos += kept
    assert pos == len(files) and len(rows) == sum(len(b) for b in batches)
    return rows


def check(emu, tmp_path, batches, **kw):
    cases = [c for b in batches for c in b]
    for c, row in zip(cases, run(emu, tmp_path, batches, **kw)):
        assert row[5] == 1, ("a guard or an untouched byte was written", c.name)
        wc.check_row(c, row[:5], row[6])


def test_chunk_lengths_and_stream_lengths(emu, tmp_path):
    """chunk_bytes x n, each alone: out_cap exact"""
    check(emu, tmp_path, [[c] for c in wc.length_cases()])


def test_every_residue(emu, tmp_path):
    check(emu, tmp_path, [wc.residue_cases()])


def test_out_cap_one_short(emu, tmp_path):
    check(emu, tmp_path, [wc.capacity_cases()])


def test_length_from_a_device_result(emu, tmp_path):
    check(emu, tmp_path, [wc.source_cases()])


@pytest.mark.parametrize("blocks_x", [0, 1, 3])
def test_piece_folding(emu, tmp_path, blocks_x):
    """chunk_bytes = 0x7fffffff around 1 MiB and at 3 MiB + 17: pieces of 1 MiB, a wave each (or one wave striding over all of them),
    folded by the finish"""
    check(emu, tmp_path, [[c] for c in wc.fold_cases()], blocks_x=blocks_x)


def test_a_batch_mixing_all_of_it(emu, tmp_path):
    check(emu, tmp_path, [wc.mixed_batch()])
    check(emu, tmp_path, [wc.mixed_batch()], blocks_x=2)
