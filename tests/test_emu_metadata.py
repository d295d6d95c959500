"""The kernels of the chunk directory (csrc/chunks.hip: dir_list, dir_head behind the lexer's three) and of the text entry (csrc/text.hip:
text_count, text_scan, text_write), as written, run on the CPU by the wave emulator of tools/emu: tools/emu/emu_metadata.cpp over the
whole case table of tests/metadata_cases.py, compared with tests/metadata_ref.py (and tests/lex_ref.py for the lexer's own answer).
Twice: a plain build, and one with -fsanitize=address,undefined -- a CPU program of its own, run as a subprocess, nothing preloaded;
every input is an exact-size copy and every output lies between guard bytes, so a read or write past an end is seen."""
import os
import struct
import subprocess
import sys

import pytest

import emu_build
import metadata_cases as mc
import metadata_ref as mr
from lex_ref import lex_ref

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize=alignment", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
            "-DEMU_UCONTEXT")
ENV = {"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def emu(request, tmp_path_factory):
    """emu_build.build_plain for a driver over two sources"""
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    sys.path.insert(0, emu_build.EMU)
    import prep_deflate
    d = tmp_path_factory.mktemp("emu_metadata")
    macros = []
    for source, macro in (("chunks.hip", "EMU_CHUNKS_SRC"), ("text.hip", "EMU_TEXT_SRC")):
        inc = d / (os.path.splitext(source)[0] + "_emu.inc")
        inc.write_text(prep_deflate.prepare_plain(open(os.path.join(emu_build.CSRC, source)).read()))
        macros.append(f'-D{macro}="{inc}"')
    flags = ("-fpermissive", "-Wno-attributes") + (SANITIZE if request.param == "sanitized" else ())
    out = d / "emu_metadata"
    subprocess.run(["g++", "-O1", "-std=c++17", "-DSPNG_EMU", *macros, "-I" + emu_build.EMU, "-I" + emu_build.CSRC, "-x", "c++", *flags, "-w",
                    "-o", str(out), os.path.join(emu_build.EMU, "emu_metadata.cpp")], check=True, capture_output=True, timeout=600)
    return out


class Run:
    """a blob and a script put together piece by piece, then run once"""

    def __init__(self):
        self.blob, self.script = bytearray(), []

    def put(self, data):
        at = len(self.blob)
        self.blob += data
        return at

    def run(self, emu, tmp_path, timeout=900):
        (tmp_path / "blob").write_bytes(bytes(self.blob))
        (tmp_path / "script").write_text("\n".join(self.script) + "\n")
        r = subprocess.run([str(emu), str(tmp_path / "blob"), str(tmp_path / "script"), str(tmp_path / "out")], capture_output=True, text=True,
                           timeout=timeout, env=ENV)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        return [ln.split() for ln in r.stdout.splitlines()], (tmp_path / "out").read_bytes()


def check_dir(lines, data, cap):
    """the lines of one `dir` command against the yardsticks; -> the lines behind them"""
    want, _ = lex_ref(data, len(data))
    assert lines[0][0] == "L"
    got = [int(x, 16) if k in (2, 3) else int(x) for k, x in enumerate(lines[0][1:])]
    assert tuple(got[:18]) == tuple(want) and got[18:] == [0, 0]
    entries = mr.directory(data, want.chunks)[:cap]
    for e, ln in zip(entries, lines[1:]):
        assert ln[0] == "E" and [int(x) for x in ln[1:]] == [e.type, e.length, e.offset, *e.head, 0], (e, ln)
    assert lines[1 + len(entries)] == ["G", "1"]
    return lines[2 + len(entries):]


@pytest.mark.parametrize("case", mc.dir_cases(), ids=lambda c: c.name)
def test_directory(emu, tmp_path, case):
    run = Run()
    caps = case.caps or [len(f) // 12 for f in case.files]
    for f, cap in zip(case.files, caps):
        run.script.append(f"dir {run.put(f)} {len(f)} {cap} -1")
    lines, _ = run.run(emu, tmp_path)
    for f, cap in zip(case.files, caps):
        lines = check_dir(lines, f, cap)
    assert not lines


def test_directory_with_a_list_of_any_length(emu, tmp_path):
    """the list full from the first chunk on, after one chunk, one short of everything: the walk behind the list starts where it must"""
    data = mc.dir_cases()[2].files[0]
    run = Run()
    at = run.put(data)
    lists = (0, 1, 2, 6, 7, 8)
    for n in lists:
        run.script.append(f"dir {at} {len(data)} 7 {n}")
    lines, _ = run.run(emu, tmp_path)
    for n in lists:
        lines = check_dir(lines, data, 7)
    assert not lines


def test_heads(emu, tmp_path):
    """every head case as a file of its own (through all five kernels), and as a payload of exactly its bytes (dir_head_kernel alone)"""
    cases = mc.head_cases()
    run = Run()
    for c in cases:
        f = mc.head_file(c)
        run.script.append(f"dir {run.put(f)} {len(f)} 3 -1")
        run.script.append(f"head {c.kind.decode()} {run.put(c.payload)} {len(c.payload)}")
    lines, _ = run.run(emu, tmp_path)
    for c in cases:
        lines = check_dir(lines, mc.head_file(c), 3)
        assert lines[0][0] == "H" and [int(x) for x in lines[0][1:]] == list(mr.parse_head(c.kind, c.payload)), c.name
        lines = lines[1:]
    assert not lines


def test_heads_in_one_file(emu, tmp_path):
    cases = mc.head_cases()
    f = mc.file_of(*[mc.chunk(c.kind, c.payload) for c in cases])
    run = Run()
    run.script += ["blocks 5", f"dir {run.put(f)} {len(f)} {len(cases) + 2} -1"]
    lines, _ = run.run(emu, tmp_path)
    assert not check_dir(lines, f, len(cases) + 2)


def test_transcode(emu, tmp_path):
    cases = mc.transcode_cases()
    run = Run()
    for c in cases:
        need = len(mr.latin1_to_utf8(c.data))
        run.script.append(f"text 1 {run.put(c.data)} {len(c.data)} {c.src_at} {c.dst_at} {max(need + c.cap_delta, 0)}")
    lines, out = run.run(emu, tmp_path)
    pos = 0
    for c, ln in zip(cases, lines):
        want = mr.latin1_to_utf8(c.data)
        short = c.cap_delta < 0 and len(want) + c.cap_delta >= 0
        assert ln == ["T", str(mr.E_OUTPUT_CAPACITY if short else mr.DONE), str(len(want)), str(len(c.data)), "0", "0", "1"], c.name
        if not short:
            assert out[pos:pos + len(want)] == want, c.name
            pos += len(want)
    assert pos == len(out) and len(lines) == len(cases)


def test_check_utf8(emu, tmp_path):
    cases = mc.utf8_cases()
    run = Run()
    for k, c in enumerate(cases):
        run.script.append(f"text 2 {run.put(c.data)} {len(c.data)} {k % 4} 0 0")
    lines, out = run.run(emu, tmp_path)
    for c, ln in zip(cases, lines):
        st, first, count = mr.check_utf8(c.data)
        assert ln == ["T", str(st), "0", str(len(c.data)), str(first), str(count), "1"], c.name
    assert not out and len(lines) == len(cases)
