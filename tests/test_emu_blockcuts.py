"""Block cuts of the parallel inflate pipeline (csrc/pinflate2.hip: pinf2_cutplan_kernel, pinf2_cutdecode_kernel,
pinf2_cutjoin_kernel, pinf2_cutscan_kernel) on the CPU, by the wave emulator of tools/emu: streams that are ONE block -- or
many blocks without a findable header -- cut into segments that decode from guessed bits and are joined to the chain afterwards.
The driver tries cuts only when EMU_CUT_BYTES is set; the streams come from tests/oneblock.py, the expected bytes from zlib."""
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import oneblock as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("emu") / "emu_pinflate2_cov"
    subprocess.run(["g++", "-O1", "-std=c++17", "-DSPNG_EMU", "-DSPNG_EMU_COV", "-I" + os.path.join(ROOT, "tools", "emu"), "-x", "c++", "-fpermissive",
                    "-Wno-attributes", "-w", "-o", str(out), os.path.join(ROOT, "tools", "emu", "emu_pinflate2.cpp")],
                   check=True, capture_output=True, timeout=600)
    return out


def damaged(z, how):
    if how == "truncated":
        return z[:len(z) * 2 // 3]
    b = bytearray(z)
    b[len(b) // 2] ^= 0x10
    return bytes(b)


def streams():
    dyn = ob.one_dynamic_block(1, 300000)
    fix = ob.one_fixed_block(2, 200000)
    zf = np.random.default_rng(5).integers(0, 40, 300000, dtype=np.uint8).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    return {"dynamic": dyn, "fixed": fix, "zfixed": (zf, co.compress(zf) + co.flush()), "dynamic+fixed": ob.dynamic_then_fixed(3, 100000, 200000),
            "truncated": (dyn[0], damaged(dyn[1], "truncated")), "flipped": (dyn[0], damaged(dyn[1], "flipped"))}


# (stream, segment bytes, EMU_CUT_BYTES or 0, EMU_PARTS or 0)
CASES = [("dynamic", 2048, 8192, 0), ("dynamic", 4096, 8192, 4), ("dynamic", 2048, 1 << 20, 0), ("fixed", 2048, 8192, 0), ("fixed", 4096, 8192, 0),
         ("zfixed", 2048, 8192, 0), ("dynamic+fixed", 2048, 8192, 0), ("truncated", 2048, 0, 0), ("truncated", 2048, 8192, 0),
         ("flipped", 2048, 0, 0), ("flipped", 2048, 8192, 0)]


@pytest.fixture(scope="module")
def runs(emu, tmp_path_factory):
    """every case once: {case: (exit code, (tried, joined, redone) or None, verdict lines, log, the three COV counters)}"""
    tmp = tmp_path_factory.mktemp("cuts")
    out = {}
    made = streams()
    for case in CASES:
        name, seg, cut, parts = case
        data, z = made[name]
        (tmp / "z").write_bytes(z)
        (tmp / "want").write_bytes(data)
        env = dict(os.environ)
        for k in ("EMU_CUT_BYTES", "EMU_PARTS", "EMU_VERBOSE"):
            env.pop(k, None)
        if cut:
            env["EMU_CUT_BYTES"] = str(cut)
        if parts:
            env["EMU_PARTS"] = str(parts)
        r = subprocess.run([str(emu), str(tmp / "z"), str(tmp / "want"), "0", str(seg)], capture_output=True, text=True, timeout=900, env=env)
        m = re.search(r"cuts tried=(\d+) joined=(\d+) redone=(\d+)", r.stdout)
        stats = tuple(int(g) for g in m.groups()) if m else None
        assert (stats is not None) == bool(cut), r.stdout + r.stderr
        c = re.search(r"COVCUT (\d+) (\d+) (\d+)", r.stderr)
        cov = tuple(int(g) for g in c.groups()) if c else (0, 0, 0)
        verdict = [line for line in r.stdout.splitlines() if not line.startswith("cuts ")]
        out[case] = (r.returncode, stats, verdict, r.stdout + r.stderr, cov)
    return out


def test_the_writers_streams_inflate_with_zlib():
    for data, z in (ob.one_dynamic_block(1, 300000), ob.one_fixed_block(2, 100000), ob.dynamic_then_fixed(3, 100000, 100000)):
        assert zlib.decompress(z) == data and len(data) > 90000
    rows = np.random.default_rng(4).integers(0, 7, 50000, dtype=np.uint8).tobytes()
    assert zlib.decompress(ob.literal_block(rows)) == rows


@pytest.mark.parametrize("seg, parts", [(2048, 0), (4096, 4)])
def test_one_dynamic_block(runs, seg, parts):
    rc, (tried, joined, redone), _, log, _ = runs[("dynamic", seg, 8192, parts)]
    assert rc == 0, log
    assert tried >= 8 and joined >= 1 and redone == 0, log
    if parts:
        assert f"parts: {parts}" in log, "the chain of a one-block stream has segment boundaries to cut at"


@pytest.mark.parametrize("seg", [2048, 4096])
def test_one_fixed_block_of_literals(runs, seg):
    """eight-bit codes only: a guess at the wrong bit meets look-alikes of the end-of-block code and undefined codes before it merges"""
    rc, (tried, joined, redone), _, log, _ = runs[("fixed", seg, 8192, 0)]
    assert rc == 0, log
    assert tried >= 8 and joined >= 1 and redone == 0, log


def test_zlib_fixed_strategy_stream(runs):
    """Z_FIXED: many fixed blocks, no header that find could see -- the blocks share their tables, so segments join across them"""
    rc, (tried, joined, redone), _, log, _ = runs[("zfixed", 2048, 8192, 0)]
    assert rc == 0, log
    assert tried >= 8 and joined >= 1, log


def test_other_tables_behind_the_anchor_redo(runs):
    """the segments lie in a fixed block, their anchor's tables are a dynamic block's: the cuts do not stitch, the stream is decoded
    again without cuts -- by the pipeline (exit code 0: SPNG_DONE with reserved == 1), not by the serial kernel"""
    rc, (tried, joined, redone), _, log, _ = runs[("dynamic+fixed", 2048, 8192, 0)]
    assert rc == 0, log
    assert tried >= 8 and redone >= 1, log


@pytest.mark.parametrize("damage", ["truncated", "flipped"])
def test_malformed_streams_end_as_without_cuts(runs, damage):
    rc0, _, verdict0, log0, _ = runs[(damage, 2048, 0, 0)]
    rc1, stats, verdict1, log1, _ = runs[(damage, 2048, 8192, 0)]
    assert rc0 not in (0, 1), log0
    assert (rc1, verdict1) == (rc0, verdict0), log0 + log1
    assert stats[0] >= 1


def test_short_runs_are_left_alone(runs):
    """a run shorter than the threshold: no cut is tried, the stream goes the way it went before"""
    rc, stats, _, log, _ = runs[("dynamic", 2048, 1 << 20, 0)]
    assert rc == 0 and stats == (0, 0, 0), log


def test_the_rare_paths_were_reached(runs):
    cov = [sum(r[4][i] for r in runs.values()) for i in range(3)]
    assert cov[0] > 0, "no guess slid after a bogus end of block or an undefined code"
    assert cov[1] > 0, "no join needed more than one chunk"
    assert cov[2] > 0, "no stream was redone"
