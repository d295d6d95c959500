"""The tables of tests/bounds_cases.py through the emulators of tools/emu, every source and destination between guard bytes
(tools/emu/guard.hpp): inflate_kernel of csrc/inflate.hip at every capacity of the inflate table, the pipeline of csrc/pinflate2.hip
with a capacity at and below the output, the deflate kernels of csrc/deflate.hip with capacities below the stream -- and once more as
programs built with -fsanitize=address,undefined, whose sources and destinations are heap buffers of exactly src_len and dst_cap
bytes: there a read behind src_len or a write behind dst_cap is the sanitizer's to report.  Each of those is a CPU program of its
own, run as a subprocess, nothing preloaded."""
import os
import shutil
import subprocess
import sys

import pytest

import bounds_cases as bc
import pnghelp as ph
from test_emu_deflate import build as build_deflate
from test_emu_inflate import CLANG, build_emu as build_inflate
from test_emu_pinflate import build_emu as build_pinflate
from test_emu_unpack import SANITIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU, CSRC = os.path.join(ROOT, "tools", "emu"), os.path.join(ROOT, "swift_png_amd", "csrc")
SAN_ENV = {"ASAN_OPTIONS": "detect_stack_use_after_return=0:detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
GUARD_EXIT = 6                                   # tools/emu/guard.hpp: a guard byte changed


def sanitized(d, driver, macro=None, inc=None, defines=()):
    """tools/emu/<driver> with the address and undefined-behaviour sanitizers, as tests/test_emu_unpack.py builds its own -> the program"""
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("clang++ not available")
    out = d / (os.path.splitext(driver)[0] + "_san")
    subprocess.run([CLANG, "-O1", "-std=c++17", "-DSPNG_EMU", "-DEMU_UCONTEXT", *([f'-D{macro}="{inc}"'] if macro else []), "-I" + EMU, "-I" + CSRC,
                    "-x", "c++", *SANITIZE, *defines, "-w", "-o", str(out), os.path.join(EMU, driver)], check=True, capture_output=True, timeout=900)
    return out


@pytest.fixture(scope="module")
def emu_inflate(tmp_path_factory):
    return build_inflate(tmp_path_factory.mktemp("emu_inflate_bounds"))


@pytest.fixture(scope="module")
def emu_inflate_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_inflate_san")
    build_inflate(d)                                                             # (leaves the prepared sources in d)
    return sanitized(d, "emu_inflate.cpp", "EMU_INFLATE_SRC", d / "inflate_emu.inc")


@pytest.fixture(scope="module")
def emu_pinflate(tmp_path_factory):
    return build_pinflate(tmp_path_factory.mktemp("emu_pinflate_bounds") / "emu_pinflate2")


@pytest.fixture(scope="module")
def emu_pinflate_san(tmp_path_factory):
    # -fno-sanitize=bounds, here only: round 0 of pinf2_decode ORs a zero into "the word behind a lane's last", one row behind the LDS
    # array vmap -- into the member the struct puts there on purpose (pinflate2.hip: the static_assert behind DLds says so).  An index
    # check of a fixed-size array inside that struct is all the flag turns off; every heap access stays the address sanitizer's.
    return sanitized(tmp_path_factory.mktemp("emu_pinflate_san"), "emu_pinflate2.cpp", defines=("-fno-sanitize=bounds",))


@pytest.fixture(scope="module")
def emu_deflate(tmp_path_factory):
    return build_deflate(tmp_path_factory.mktemp("emu_deflate_bounds"))


@pytest.fixture(scope="module")
def emu_deflate_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_deflate_san")
    build_deflate(d)
    return sanitized(d, "emu_deflate2.cpp", "EMU_DEFLATE_SRC", d / "deflate_emu.inc", ("-DSPNG_D3_WAVES=4",))


# ---- inflate_kernel ------------------------------------------------------------------------------------------------------------------

def inflate_row(emu, tmp_path, name, cap, env=None):
    """one row through emu_inflate against the oracle: status, written, bytes, consumed, payload -- and the guards (exit code)"""
    st = bc.stream(name)
    if st.fmt == bc.GZIP:                                                       # (the serial kernel sees the member's payload: gzip.hip's header kernel moves
        z, fmt = st.z[st.body_at:], bc.RAW                                      #  the window; the trailer stays behind it)
        want = ph.orc_inflate(z, fmt, cap=cap)
    else:
        z, fmt = st.z, st.fmt
        want = bc.inflate_expected(name, cap)
    (tmp_path / "z").write_bytes(z)
    r = subprocess.run([str(emu), str(tmp_path / "z"), str(fmt), str(cap), str(tmp_path / "out")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (name, cap, r.returncode, r.stdout[-300:], r.stderr[-3000:])
    status, written, consumed, aux0, aux1 = (int(x) for x in r.stdout.split())
    assert (status, written) == (want[0], len(want[1])), (name, cap, status, want[0], written, len(want[1]))
    assert (tmp_path / "out").read_bytes() == want[1], (name, cap)
    if status == 0:
        assert consumed == want[2]
    elif status != 1:
        assert (aux0, aux1) == tuple(want[3])


@pytest.mark.parametrize("name", bc.STREAMS)
def test_serial_kernel_at_every_capacity_of_the_table(emu_inflate, tmp_path, name):
    for label, cap in bc.inflate_rows(name):
        if name == "periods" and label not in ("N", "N-1", "N-17", "0", "16", "inside-match", "match-end", "inside-literals"):
            continue                                                             # (5.8 MB a run: the rows that differ in kind)
        inflate_row(emu_inflate, tmp_path, name, cap)


@pytest.mark.parametrize("name", [n for n in bc.STREAMS if n != "periods"])
def test_serial_kernel_under_the_sanitizers(emu_inflate_san, tmp_path, name):
    """N, one below, 0: exact heap buffers"""
    n = bc.stream(name).n
    for cap in (n, n - 1, 0):
        inflate_row(emu_inflate_san, tmp_path, name, cap, env=SAN_ENV)


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------

def pipeline(emu, tmp_path, name, cap, segment, env=None, **knobs):
    st = bc.stream(name)
    (tmp_path / "z").write_bytes(st.z[st.body_at:] if st.fmt == bc.GZIP else st.z)
    (tmp_path / "raw").write_bytes(st.data)
    e = dict(os.environ if env is None else env, EMU_DST_CAP=str(cap), **{k: str(v) for k, v in knobs.items()})
    r = subprocess.run([str(emu), str(tmp_path / "z"), str(tmp_path / "raw"), str(0 if st.fmt == bc.ZLIB else 1), str(segment)], capture_output=True, text=True,
                       timeout=900, env=e)
    assert r.returncode != GUARD_EXIT, (name, cap, knobs, r.stdout[-300:])
    return r


@pytest.mark.parametrize("name", ["a", "b", "c", "echo", "a-raw"])
def test_pipeline_with_an_exact_capacity_and_below(emu_pinflate, tmp_path, name):
    """capacity N: the pipeline's own answer; below N it leaves the stream to the serial kernel (exit code 3: all of it, 4: from a
    block boundary on), and the guards hold -- with one workgroup, with parts, with block cuts"""
    st, rows = bc.stream(name), dict(bc.inflate_rows(name))
    for knobs in ({}, {"EMU_PARTS": 4}, {"EMU_PARTS": 4, "EMU_MARK_TILE": 8192}, {"EMU_CUT_BYTES": 8192}):
        segment = 4096 if knobs else 1 << 20
        r = pipeline(emu_pinflate, tmp_path, name, st.n, segment, **knobs)
        assert r.returncode == 0 and "ok:" in r.stdout, (name, knobs, r.returncode, r.stdout[-300:], r.stderr[-300:])
        for label in ("N-1", "N-17", "0", "16", "inside-match", "match-end", "block-boundary", "inside-stored", "inside-literals"):
            if label in rows:
                r = pipeline(emu_pinflate, tmp_path, name, rows[label], segment, **knobs)
                assert r.returncode in (3, 4) and "ok:" not in r.stdout, (name, label, knobs, r.returncode, r.stdout[-300:], r.stderr[-300:])


@pytest.mark.parametrize("name", ["a", "b", "c", "a-raw"])
def test_pipeline_under_the_sanitizers(emu_pinflate_san, tmp_path, name):
    st = bc.stream(name)
    for knobs in ({}, {"EMU_PARTS": 4}):
        for cap in (st.n, st.n - 1, 0):
            r = pipeline(emu_pinflate_san, tmp_path, name, cap, 4096, env=SAN_ENV, **knobs)
            assert r.returncode == (0 if cap == st.n else r.returncode) and r.returncode in (0, 3, 4), (name, cap, knobs, r.returncode, r.stdout[-300:], r.stderr[-3000:])


# ---- deflate -------------------------------------------------------------------------------------------------------------------------

def deflate_row(emu, tmp_path, row, env=None, cuts=(), **knobs):
    name, level, fmt, e, label, cap = row
    f = bc.full(name, level, fmt, e)
    (tmp_path / "in").write_bytes(bc.inputs()[name])
    (tmp_path / "want").write_bytes(f)
    en = dict(os.environ if env is None else env, EMU_DST_CAP=str(cap), EMU_EXPONENT=str(e), **{k: str(v) for k, v in knobs.items()})
    r = subprocess.run([str(emu), str(tmp_path / "in"), str(tmp_path / "want"), str(level), str(fmt), "2"] + [str(c) for c in cuts], capture_output=True, text=True,
                       timeout=900, env=en)
    assert r.returncode == 0, (row, knobs, cuts, r.returncode, r.stdout[-300:], r.stderr[-3000:])
    assert r.stdout.startswith("ok (capacity):" if cap < len(f) else "ok:"), (row, r.stdout[-300:])


def emulated_rows(level, names):
    """the rows of the emulator: zlib and raw (the gzip trailer is gzip.hip's, on the device)"""
    return [r for r in bc.deflate_rows(level, names) if r[2] != bc.GZIP]


@pytest.mark.parametrize("level", bc.LEVELS)
def test_deflate_rows_of_the_small_inputs(emu_deflate, tmp_path, level):
    """every capacity of the inputs up to 5000 bytes: dfl4_scan / dfl4_place (levels 0-7), dfl2_parse's writer (8 and up)"""
    for row in emulated_rows(level, bc.SMALL_INPUTS):
        deflate_row(emu_deflate, tmp_path, row)


@pytest.mark.parametrize("level", bc.FAMILY_LEVELS)
def test_deflate_rows_of_the_70000_byte_input(emu_deflate, tmp_path, level):
    for row in emulated_rows(level, ("scan70000",)):
        deflate_row(emu_deflate, tmp_path, row)


@pytest.mark.parametrize("level", [1, 6])
def test_deflate_two_wave_writer_and_pushes_into_a_short_destination(emu_deflate, tmp_path, level):
    """dfl3_parse_kernel's writer (drain, finish_stream), one-shot (EMU_TWO_WAVE) and pushed in pieces: from the push that overflows on
    every push answers SPNG_E_OUTPUT_CAPACITY (the driver checks each)"""
    for name in ("mix5000", "scan70000"):
        for row in emulated_rows(level, (name,)):
            if row[3] != 15 or row[4] not in ("L", "L-1", "L-5", "0", "1", "1023", "1024", "1025", "2049", "L//2|1"):
                continue
            deflate_row(emu_deflate, tmp_path, row, EMU_TWO_WAVE=1)
            if row[4] in ("L", "L-1", "1", "1024", "L//2|1"):
                n = len(bc.inputs()[name])
                deflate_row(emu_deflate, tmp_path, row, cuts=list(range(4097, n, 4097 if n < 10000 else 20001)))


def test_deflate_full_search_pushes_into_a_short_destination(emu_deflate, tmp_path):
    for row in emulated_rows(9, ("mix5000",)):
        if row[4] in ("L", "L-1", "1", "1024", "L//2|1"):
            deflate_row(emu_deflate, tmp_path, row, cuts=[1500, 4097])


@pytest.mark.parametrize("level", bc.LEVELS)
def test_deflate_under_the_sanitizers(emu_deflate_san, tmp_path, level):
    """L, one below, 0 on the 5000-byte input, zlib and raw; the small inputs at L; L and one below on the 70 000-byte input at levels 1
    and 6: exact heap buffers, no padding behind the input"""
    for row in emulated_rows(level, ("mix5000",)):
        if row[4] in ("L", "L-1", "0"):
            deflate_row(emu_deflate_san, tmp_path, row, env=SAN_ENV)
            if level in (1, 6) and row[4] != "0":
                deflate_row(emu_deflate_san, tmp_path, row, env=SAN_ENV, EMU_TWO_WAVE=1)
    for row in emulated_rows(level, ("n0", "n1", "n2", "n3", "n4", "text200")):
        if row[4] == "L":
            deflate_row(emu_deflate_san, tmp_path, row, env=SAN_ENV)
    # many drains of the staging ring, several blocks, exponents 15 and 8 -- at levels 1 and 6.  Not at level 9: there the address
    # sanitizer stops at a read of LDS, not of the source or the destination -- d2_forward's blind read of the offer table, lane 63
    # (pq == 3, whose offer is never used) at the batch's last vertex reads g_ptab[66][0], the word behind the table's two rows of
    # padding; on the device a value nobody uses, in the emulator the end of a global array.  profiles/r17_bounds.md has the report.
    if level in (1, 6):
        for row in emulated_rows(level, ("scan70000",)):
            if row[2] == bc.ZLIB and row[4] in ("L", "L-1"):
                deflate_row(emu_deflate_san, tmp_path, row, env=SAN_ENV)
