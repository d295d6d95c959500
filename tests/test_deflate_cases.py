"""The case table of tests/deflate_cases.py -- DEFLATE streams that no compressor writes -- checked on the CPU: zlib and the oracle
agree on every valid case and the oracle still says what the table records for every malformed one; each case proves from its
tokens, in plain Python, that it is what it claims; and every case runs through both wave emulators of tools/emu -- the parallel
pipeline (segments of 256 bytes and 1 MiB; one workgroup per stream and 4 parts with marker tiles of 4096 and 8192), built with
counters that say how often the three resolve paths the table is for were reached, and, the malformed ones, the serial kernel.
Timing and memory ordering are not modelled, nor is v_rcp_f32 (the host's 1 / x stands in): tests/test_gpu_deflate_cases.py runs
the same table on the device."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import oneblock as ob
import pnghelp as ph
from test_emu_inflate import build_emu as build_serial_emu, check as serial_check
from test_emu_pinflate import build_emu as build_pipeline_emu

# (segment bytes, parts, marker tile)
CONFIGS = [(256, 0, 0), (1 << 20, 0, 0), (256, 4, 4096), (256, 4, 8192), (1 << 20, 4, 4096), (1 << 20, 4, 8192)]


# ---- zlib, the oracle, the record --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.VALID)
def test_valid_case_is_zlibs_and_the_oracles(name):
    c = dc.case(name)
    want = zlib.decompress(c.stream)
    st, out, consumed, aux = ph.orc_inflate(c.stream, c.fmt, cap=len(want) + 64)
    assert st == 0 and out == want == c.info["data"] and consumed == len(c.stream)
    assert zlib.decompressobj(-15).decompress(c.body) == want
    assert len(want) < 6 << 20 and len(c.stream) < 200_000


@pytest.mark.parametrize("name", dc.INVALID)
def test_malformed_case_is_what_the_table_records(name):
    c = dc.case(name)
    st, out, consumed, aux = dc.expected(c)
    assert c.expect is not None and (st, len(out), tuple(aux)) == c.expect
    assert len(c.stream) < 200_000
    if name != "periods-capacity":                                               # (zlib knows no capacity)
        with pytest.raises(zlib.error):
            zlib.decompress(c.stream)


def test_reach_twins_differ_by_one_byte_of_distance():
    a, b = dc.case("reach-exact"), dc.case("reach-beyond")
    (_, _, da), (_, _, db) = dc.runs_and_distances(a.blocks[1]), dc.runs_and_distances(b.blocks[1])
    assert len(a.blocks[0]) == 1000 and da[0] == 1000 and db[0] == 1001


# ---- each case is what it claims, from its tokens ------------------------------------------------------------------------------------

def test_periods_holds_every_pair():
    ref, run, dist = dc.runs_and_distances(dc.case("periods").blocks[0])
    pairs = list(zip(run[ref].tolist(), dist[ref].tolist()))
    below = {(r, d) for r in range(3, 259) for d in range(1, r)}
    assert len(below) == 33152
    want = below | {(d, d) for d in range(3, 259)} | {(d - 1, d) for d in range(4, 259)}
    assert set(pairs) == want and len(pairs) == len(want)                        # (each once)
    i = np.nonzero(ref)[0]
    assert not ref[i - 1].any()                                                  # a literal in front of every reference


def test_extremes_holds_every_end_of_every_field():
    t = dc.case("extremes").blocks[0]
    ref, run, dist = dc.runs_and_distances(t)
    assert not ref[:dc.HEAD].any() and ref[dc.HEAD:].all()
    have = {(int(s), int(x), int(d)) for s, x, d in zip(t[ref, 0], t[ref, 1], dist[ref])}
    ends_d = {int(b) + e for b, x in zip(ob.DIST_BASE, ob.DIST_EXTRA) for e in (0, (1 << int(x)) - 1)}
    ends_l = {(257 + k, e) for k, x in enumerate(ob.LEN_EXTRA) for e in (0, (1 << int(x)) - 1)}
    assert have == {(s, x, d) for s, x in ends_l for d in ends_d}
    assert {(285, 0, 32768), (284, 31, 32768), (257, 0, 32768), (285, 0, 1), (284, 31, 1)} <= have
    assert set(run[ref].tolist()) >= {3, 258} and int(dist.max()) == 32768


@pytest.mark.parametrize("name", ["dense3", "dense34", "dense-blocks"])
def test_dense_cases_exceed_the_reference_cap_in_every_window(name):
    c = dc.case(name)
    assert len(c.blocks) == (17 if name == "dense-blocks" else 1)
    ref, run, _ = dc.runs_and_distances(np.concatenate(c.blocks))
    pos = np.cumsum(run) - run
    head, total = c.info["head"], int(run.sum())
    assert not ref[:head].any() and int(ref.sum()) >= 20000
    dist = dc.runs_and_distances(np.concatenate(c.blocks))[2][ref]
    assert int(dist.min()) < 10 and int(dist.max()) > 32700                      # (uniform over 1 .. 32768)
    starts = pos[ref]
    for window, cap in ((8192, 1024), (4096, 512)):                              # RGeo: MAXM = TILE / 8
        w = np.arange(head, total - window + 1)
        inside = np.searchsorted(starts, w + window, side="left") - np.searchsorted(starts, w, side="left")
        assert len(w) > 2 * window and int(inside.min()) > cap, (window, int(inside.min()))
    if name == "dense3":
        assert set(run[ref].tolist()) == {3}
    else:
        assert set(run[ref].tolist()) == {3, 4} and (~ref[head:]).sum() > 1000
        # a reference's first halfword (a literal is one halfword, a reference two) falls on every one of a thread's eight
        hw = np.cumsum(np.where(ref, 2, 1)) - np.where(ref, 2, 1)
        assert set((hw[ref] % 8).tolist()) == set(range(8))


def test_echo_is_its_first_window_over_and_over():
    c = dc.case("echo")
    data = c.info["data"]
    assert len(c.blocks) == dc.ECHO_BLOCKS + 1 >= 25 and data == data[:32768] * (dc.ECHO_BLOCKS + 1)
    for t in c.blocks[1:]:
        ref, run, dist = dc.runs_and_distances(t)
        assert ref.all() and len(t) == 128 and run.tolist() == [258] * 126 + [130, 130] and set(dist.tolist()) == {32768}


def test_edges_blocks_begin_with_the_four_sources():
    c = dc.case("edges")
    assert len(c.blocks) - 1 >= 40
    P = dc.HEAD
    for t in c.blocks[1:]:
        ref, run, dist = dc.runs_and_distances(t)
        assert ref[:4].all() and not ref[4:].any()
        at = P + np.cumsum(run[:4]) - run[:4]
        src = (at - dist[:4]).tolist()
        assert src[:3] == [P - 32768, P - 1, P]
        assert P - 100 < src[3] < P < src[3] + run[3]                            # begins in the block before, runs across P
        assert 2600 <= int(run.sum()) <= 4100                                    # about 3 KB
        P += int(run.sum())
    assert P == len(c.info["data"])


def test_header_cases_are_what_they_claim():
    special = {n: dc.case(n).blocks[3] for n in dc.HEADERS}
    t = special["headers-one-distance"]
    assert (t[:, 2] >= 0).sum() == 300 and set(t[t[:, 2] >= 0, 2].tolist()) == {10}
    assert not (special["headers-no-distance"][:, 2] >= 0).any()
    ll, dl = dc.deep_lengths()
    t = special["headers-deep15"]
    ref = t[:, 2] >= 0
    assert ll.max() == 15 and dl.max() == 15
    for lens in (ll, dl):                                                        # complete codes
        assert sum(2.0 ** -int(v) for v in lens if v) == 1.0
    assert {284, 285} <= set(t[ref, 0].tolist()) and {28, 29} <= set(t[ref, 2].tolist())     # the four 15-bit codes are used
    assert ((t[ref, 0] == 284) & (t[ref, 2] == 29)).any()                        # ... also in one token of 48 bits
    ll, dl = dc.full_lengths()
    assert len(ll) == 286 and len(dl) == 30 and ll.all() and dl.all()
    for lens in (ll, dl):
        assert sum(2.0 ** -int(v) for v in lens) == 1.0
    items = ob.header_items(np.concatenate([ll, dl]), repeats=True)
    assert sum(n for _, _, _, n in items) == 316
    across = [(s, at, n) for s, _, at, n in items if at < 286 < at + n]
    assert across and across[0][0] == 16, across                                 # "copy the previous length" over the HLIT boundary
    t = special["headers-full"]
    ref = t[:, 2] >= 0
    assert set(t[ref, 0].tolist()) == set(range(257, 286)) and set(t[ref, 2].tolist()) == set(range(30))
    clen = dc.cl7_lengths()
    assert clen.max() == 7 and sum(2.0 ** -int(v) for v in clen if v) == 1.0
    assert set(np.concatenate([ll, dl]).tolist()) <= set(np.nonzero(clen)[0].tolist())


def test_malformed_blocks_lie_behind_50_kb_of_good_ones():
    for name in dc.MALFORMED:
        c = dc.case(name)
        front, _ = ob.concat_bits([dc._block(t) for t in c.blocks[:3]])
        assert len(front) > 50_000
        st, out, consumed, _ = dc.expected(c)
        if st not in (0, 1):
            assert consumed > 50_000


# ---- the emulators -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_cases")
    return build_pipeline_emu(d / "emu_pinflate2_cov", "-DSPNG_EMU_COV"), d, {}


def run(pipeline, name, segment, parts, tile):
    """one run of the pipeline emulator (kept: the coverage tests below look at the same runs) -> (exit code, stdout, [COV 9, 10, 11, 12])"""
    emu, d, runs = pipeline
    key = (name, segment, parts, tile)
    if key not in runs:
        c = dc.case(name)
        z, want = d / (name + ".z"), d / (name + ".want")
        if not z.exists():
            z.write_bytes(c.stream)
            want.write_bytes(dc.expected(c)[1])
        env = dict(os.environ)
        if parts:
            env.update(EMU_PARTS=str(parts), EMU_MARK_TILE=str(tile))
        r = subprocess.run([str(emu), str(z), str(want), str(c.fmt), str(segment)], capture_output=True, text=True, timeout=600, env=env)
        cov = [ln for ln in r.stderr.splitlines() if ln.startswith("RESOLVE_COV")]
        assert cov, r.stderr[-300:]
        runs[key] = (r.returncode, r.stdout, [int(v) for v in cov[-1].split()[1:]])
    return runs[key]


@pytest.mark.parametrize("name", dc.VALID)
def test_emulated_pipeline_takes_every_valid_case(pipeline, name):
    for segment, parts, tile in CONFIGS:
        rc, out, cov = run(pipeline, name, segment, parts, tile)
        assert rc == 0 and "ok:" in out, (name, segment, parts, tile, rc, out[-300:])
        # COV(12): the period reduction never leaves an offset at or beyond its distance (a quotient one too small would, and no byte
        # would tell: the source it names holds the same value, one level deeper in the chain)
        assert cov[3] == 0, (name, segment, parts, tile, cov)


@pytest.mark.parametrize("name", dc.INVALID)
def test_emulated_pipeline_never_accepts_a_malformed_case(pipeline, name):
    """3: everything left to the serial kernel, 4: a right prefix kept and the serial kernel goes on from there, 5: the pipeline's own
    error (the checksum)"""
    for segment, parts, tile in CONFIGS:
        rc, out, _ = run(pipeline, name, segment, parts, tile)
        assert rc in (3, 4, 5) and "ok:" not in out, (name, segment, parts, tile, rc, out[-300:])


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    return build_serial_emu(tmp_path_factory.mktemp("emu_inflate_cases"))


@pytest.mark.parametrize("name", dc.NAMES)
def test_emulated_serial_kernel_says_what_the_oracle_says(serial, tmp_path, name):
    """status, byte count, bytes and payload: the malformed cases from the point where the pipeline stops, and the valid ones too (the
    serial kernel is what SPNG_INFLATE_SERIAL runs on the device)"""
    c = dc.case(name)
    if c.valid:
        assert serial_check(serial, tmp_path, c.stream, c.fmt, len(c.info["data"]) + 64) == 0
    else:
        assert serial_check(serial, tmp_path, c.stream, c.fmt, c.cap) == c.expect[0]


def test_resolve_paths_are_reached(pipeline):
    """counted, not assumed (COV(9) .. COV(11) of csrc/pinflate2.hip, nothing in the product): the tile ended by the cap on its
    references, in both geometries; the bytes beyond a run's first period; the markers for bytes in front of a part"""
    assert run(pipeline, "dense3", 1 << 20, 0, 0)[2][0] > 0                      # 8 KiB tiles: MAXM = 1024
    assert run(pipeline, "dense34", 1 << 20, 0, 0)[2][0] > 0
    small, big = run(pipeline, "dense-blocks", 256, 4, 4096), run(pipeline, "dense-blocks", 256, 4, 8192)
    assert int(small[1].split("parts:")[1].split()[0]) >= 2 and small[2][0] > big[2][0] > 0      # 4 KiB marker tiles: MAXM = 512
    assert run(pipeline, "periods", 1 << 20, 0, 0)[2][1] >= 33152
    for name in ("echo", "edges"):
        for tile in (4096, 8192):
            rc, out, cov = run(pipeline, name, 256, 4, tile)
            assert int(out.split("parts:")[1].split()[0]) >= 2 and cov[2] > 0, (name, tile, out[-200:], cov)
