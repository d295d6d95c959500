"""The encoder's case table (tests/encode_cases.py, proven from the oracle's tokens by tests/test_encode_cases.py) on the device:
every case alone at every level it speaks about, the whole table in one mixed call, beside other streams (the chunk geometry
follows the batch), pushed in pieces.  Every comparison is exact against the oracle's bytes: status DONE, `written`, the stream."""
import functools
import gzip

import numpy as np
import pytest

import encode_cases as ec
import pnghelp as ph
import swift_png_amd as spng

pytestmark = pytest.mark.gpu
FULL = (8, 9, 13)                     # d3_search_chunk<true> is the same walk with the per-decade rule on top: bytes only


@functools.lru_cache(maxsize=None)
def want(name, level, fmt=0):
    c = ec.case(name)
    return ph.orc_deflate(c.data, level, fmt, c.exponent)


def full_levels(name):
    """(the round-boundary twins leave level 13 out: 2 MiB of runs cost the ORACLE 17 s there, attempts being unbounded)"""
    return (8, 9) if name.startswith("round-edge-") else FULL


@pytest.mark.parametrize("name", ec.NAMES)
def test_case_alone(gpu, name):
    s = gpu.load()
    c = ec.case(name)
    for lv in tuple(c.levels) + full_levels(name):
        assert s.deflate(c.data, lv, spng.FORMAT_ZLIB, c.exponent) == want(name, lv), (name, lv, c.purpose)
    lv = c.levels[-1]
    assert s.deflate(c.data, lv, spng.FORMAT_IOS, c.exponent) == want(name, lv, 1), (name, lv, "raw", c.purpose)


def _mixed_plan():
    """one stream per case; levels 0-13 interleaved so that the sort of deflate_launch (levels < 8 first) moves every stream, zlib
    and raw interleaved, the exponent of the case in its descriptor"""
    plan = []
    for i, name in enumerate(ec.NAMES):
        c = ec.case(name)
        if i % 2 == 0:
            lv = c.levels[(i // 2) % len(c.levels)]
        else:
            lv = (8, 9, 10, 11, 12, 13)[(i // 2) % 6] if not name.startswith("round-edge-") else 9
        plan.append((name, lv, spng.FORMAT_IOS if i % 3 == 1 else spng.FORMAT_ZLIB))
    return plan


def test_whole_table_in_one_mixed_batch(gpu):
    s = gpu.load()
    plan = _mixed_plan()
    assert {lv for _, lv, _ in plan} == set(range(14))
    assert all((a[1] < 8) != (b[1] < 8) for a, b in zip(plan, plan[1:]))
    tens = [s.to_device(ec.case(n).data) for n, _, _ in plan]
    outs, res = s.deflate_batch(tens, None, [f for _, _, f in plan], levels=[lv for _, lv, _ in plan], exponents=[ec.case(n).exponent for n, _, _ in plan])
    for (name, lv, fmt), o, r in zip(plan, outs, res):
        c = ec.case(name)
        expected = want(name, lv, fmt)
        assert r.status == gpu.DONE and r.written == len(expected), (name, lv, fmt, r.status, r.written, len(expected))
        got = bytes(o[:r.written].cpu().numpy())
        assert got == expected, (name, lv, fmt, c.purpose)
        assert got == s.deflate(c.data, lv, fmt, c.exponent), (name, lv, fmt, "alone")


def test_gzip_members_of_the_table(gpu):
    from test_oracle_gzip import gw, raw_deflate
    s = gpu.load()
    plan = [("second-e15-0", 1), ("bucket-same-batch", 0), ("lazy-win", 6), ("tail-run-263", 4), ("block-edge-pair-out", 6), ("goal-24", 3), ("dense-block", 0),
            ("attempts-20", 9)]
    tens = [s.to_device(ec.case(n).data) for n, _ in plan]
    outs, res = s.deflate_batch(tens, None, spng.FORMAT_GZIP, levels=[lv for _, lv in plan])
    for (name, lv), o, r in zip(plan, outs, res):
        data = ec.case(name).data
        expected = gw.deflate(data, raw_deflate(lv))
        assert r.status == gpu.DONE and r.written == len(expected), (name, lv)
        got = bytes(o[:r.written].cpu().numpy())
        assert got == expected and gzip.decompress(got) == data, (name, lv)


def test_stream_envelope_matrix(gpu):
    """header, stored tail, Adler-32, padding and result of every parse kernel on inputs of 0 ... 4 bytes, both sides of the stored
    tail's limit of 3, greedy / lazy / full, zlib at the window exponents 15 and 8, raw and gzip: all one-shot streams in ONE call
    (dfl4_scan_kernel, dfl2_parse_kernel), then each pushed whole and a byte per push (the dfl3 writer, dfl2_parse_kernel with a state)"""
    from test_gpu_resume import _push_deflate
    from test_oracle_gzip import gw, raw_deflate
    s = gpu.load()
    plan = [(bytes(range(65, 65 + n)), lv, fmt, e) for n in range(5) for lv in (0, 4, 9)
            for fmt, e in ((spng.FORMAT_ZLIB, 15), (spng.FORMAT_ZLIB, 8), (spng.FORMAT_IOS, 15), (spng.FORMAT_GZIP, 15))]

    def expected(data, lv, fmt, e):
        return gw.deflate(data, raw_deflate(lv)) if fmt == spng.FORMAT_GZIP else ph.orc_deflate(data, lv, 1 if fmt == spng.FORMAT_IOS else 0, e)

    outs, res = s.deflate_batch([s.to_device(d) for d, _, _, _ in plan], None, [f for _, _, f, _ in plan], levels=[lv for _, lv, _, _ in plan],
                                exponents=[e for _, _, _, e in plan])
    for (data, lv, fmt, e), o, r in zip(plan, outs, res):
        exp = expected(data, lv, fmt, e)
        assert (r.status, r.written, r.consumed) == (gpu.DONE, len(exp), len(data)), (len(data), lv, fmt, e, r.status, r.written, r.consumed)
        assert bytes(o[:r.written].cpu().numpy()) == exp, (len(data), lv, fmt, e)
        if fmt == spng.FORMAT_GZIP:
            assert gzip.decompress(exp) == data
    for data, lv, fmt, e in plan:
        exp = expected(data, lv, fmt, e)
        for sizes in ([max(len(data), 1)], [1]):
            # (_push_deflate asserts NEED_MORE_INPUT of every push but the last, DONE and consumed == len(data) of the last; what it
            #  returns are the `written` bytes of the last)
            got, avail = _push_deflate(s, data, sizes, lv, fmt, e)
            assert got == exp and avail[-1] == len(exp), (len(data), lv, fmt, e, sizes)


GEOMETRY = [n for n in ec.NAMES if n.startswith(("chunk-edge-", "edge-e15-"))]


@pytest.mark.parametrize("name", GEOMETRY)
def test_bytes_do_not_depend_on_the_streams_beside(gpu, name):
    """search_chunks() cuts a stream alone into chunks of 32768 positions, five streams into chunks of 40384 (no multiple of 256:
    the warm-up start is rounded down), 256 streams into chunks of 2^20: the same bytes every time, wherever the stream stands"""
    s = gpu.load()
    c = ec.case(name)
    rng = np.random.default_rng(7)
    noise = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 400, 255)]
    d_case, d_noise = s.to_device(c.data), [s.to_device(b) for b in noise]
    for lv in c.levels:
        expected = want(name, lv)
        for others in (0, 4, 255):
            for at in {0, others // 2, others}:
                tens = d_noise[:at] + [d_case] + d_noise[at:others]
                outs, res = s.deflate_batch(tens, lv)
                assert len(tens) == others + 1 and res[at].status == gpu.DONE and res[at].written == len(expected), (name, lv, others, at)
                assert bytes(outs[at][:res[at].written].cpu().numpy()) == expected, (name, lv, others, at, c.purpose)
                k = (at + 1) % len(tens)                       # ... and a neighbour's are its own
                if others:
                    assert bytes(outs[k][:res[k].written].cpu().numpy()) == ph.orc_deflate((noise[:at] + [c.data] + noise[at:others])[k], lv)


PIECES = [n for n in ec.NAMES if n.startswith(("lazy-", "tail-", "block-edge-", "round-edge-"))]


@pytest.mark.parametrize("name", PIECES)
def test_pushed_in_pieces(gpu, name):
    """cuts one position before, at and after each planted match and 258 / 259 positions before it (what a push that is not the
    last holds back): the stream after the last push is the one-shot stream"""
    from test_gpu_resume import _push_deflate
    s = gpu.load()
    c = ec.case(name)
    for lv in c.levels:
        cuts = ec.cuts(c, lv)
        if not cuts:
            continue
        edges = (0,) + cuts + (len(c.data),)
        got, _ = _push_deflate(s, c.data, [b - a for a, b in zip(edges, edges[1:])], lv, spng.FORMAT_ZLIB, c.exponent)
        assert got == want(name, lv), (name, lv, cuts, c.purpose)
