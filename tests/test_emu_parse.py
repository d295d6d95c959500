"""The kernels of the typed chunks (csrc/chunks.hip: parse_scope, parse_value, parse_first behind the lexer's and the directory's), as
written, run on the CPU by the wave emulator of tools/emu: tools/emu/emu_parse.cpp over the whole case table of tests/parse_cases.py and
the golden files, compared with tests/parse_ref.py.  Twice: a plain build, whose buffers lie between guard bytes that are looked at
afterwards, and one with -fsanitize=address,undefined, whose buffers are exactly their bytes -- a CPU program of its own, run as a
subprocess, nothing preloaded."""
import shutil
import subprocess

import pytest

import emu_build
import parse_cases as pc
import parse_ref as pr
from lex_ref import lex_ref

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
            "-DEMU_UCONTEXT")
ENV = {"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
CASES = pc.cases()


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emu(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    flags = ("-fpermissive", "-Wno-attributes") + (SANITIZE if request.param == "sanitized" else ())
    return emu_build.build_plain(tmp_path_factory, "chunks.hip", "emu_parse.cpp", "EMU_CHUNKS_SRC", "-O1", compiler="g++", flags=flags)


def run(emu, tmp_path, jobs, blocks=3):
    """jobs: [(command, data, cap)] -> per job (the P line's numbers, the V lines' numbers)"""
    blob, script = bytearray(), [f"blocks {blocks}"]
    for command, data, cap in jobs:
        script.append(f"{command} {len(blob)} {len(data)} {cap}")
        blob += data
    (tmp_path / "blob").write_bytes(bytes(blob))
    (tmp_path / "script").write_text("\n".join(script) + "\n")
    r = subprocess.run([str(emu), str(tmp_path / "blob"), str(tmp_path / "script")], capture_output=True, text=True, timeout=900, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out, lines = [], [ln.split() for ln in r.stdout.splitlines()]
    while lines:
        assert lines[0][0] == "P", lines[0]
        end = next(k for k, ln in enumerate(lines) if ln[0] == "G")
        assert lines[end] == ["G", "1"], lines[end]
        out.append(([int(x) for x in lines[0][1:]], [[int(x) for x in ln[1:]] for ln in lines[1:end]]))
        lines = lines[end + 1:]
    assert len(out) == len(jobs)
    return out


def check(got, data, cap):
    info, _ = lex_ref(data, len(data))
    values, parsed = pr.parse_file(pr.chunks_of(data, min(info.chunks, cap)))
    assert got[0] == [parsed.status, parsed.index, *parsed.aux, *parsed[3:]]
    assert got[1] == [[v.status, v.scope, *v.aux, v.count, v.k, *v.v] for v in values]


def test_case_table(emu, tmp_path):
    """every case as a file through all eight kernels"""
    caps = [len(c.file) // 12 if c.cap is None else c.cap for c in CASES]
    for got, c, cap in zip(run(emu, tmp_path, [("file", c.file, cap) for c, cap in zip(CASES, caps)]), CASES, caps):
        check(got, c.file, cap)
        assert (None if got[0][0] == pr.DONE else (got[0][1], got[0][0], (got[0][2], got[0][3]))) == c.expect, c.name


def test_case_table_on_one_block_and_on_many(emu, tmp_path):
    """a wave that strides over all entries of its file, and more waves than entries"""
    some = [c for c in CASES if c.scopes is not None or "payloads" in c.name]
    for blocks in (1, 7):
        for got, c in zip(run(emu, tmp_path, [("file", c.file, len(c.file) // 12 if c.cap is None else c.cap) for c in some], blocks), some):
            check(got, c.file, len(c.file) // 12 if c.cap is None else c.cap)


def test_golden_files(emu, tmp_path):
    """every file the reference's integration tests decode: the parse kernels over a directory of the file's chunk headers"""
    files = [p.read_bytes() for p in pc.golden_files()]
    caps = [2 if k % 3 == 2 else len(f) // 12 for k, f in enumerate(files)]       # (every third directory holds IHDR and one chunk more)
    for got, data, cap in zip(run(emu, tmp_path, [("parse", f, cap) for f, cap in zip(files, caps)]), files, caps):
        check(got, data, cap)
        assert got[0][0] == pr.DONE
