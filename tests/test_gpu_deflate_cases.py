"""The case table of tests/deflate_cases.py on the device: DEFLATE streams that no compressor writes -- every (run, distance) of the
period reduction in pinf2_resolve_kernel's expand step (v_rcp_f32, which no emulator has), tiles ended by the cap on their back-
references, markers at a part's first byte / one byte in front of it / 32768 bytes in front of it in both marker geometries, token
fields at their ends, headers zlib does not write, malformed blocks behind 50 KB of good ones -- through the C ABI, alone under every
knob, all in one batch, pushed in pieces, with block cuts, and as raw and gzip streams.  The comparison is exact against the oracle:
status, written, bytes, consumed (when done), error payload (for an error other than need-more-input); no tolerances.  Every valid
case must be the PIPELINE's (spng_result.reserved == 1): a silent fall-back to the serial kernel would keep the bytes right and
test nothing of the above."""
import pytest

import deflate_cases as dc
import oneblock as ob
import pnghelp as ph
import swift_png_amd as spng

pytestmark = pytest.mark.gpu


def cap_of(c):
    return len(c.info["data"]) + 64 if c.valid else c.cap


def same(res, out, want, where):
    """one spng_result and its output tensor against the oracle's (status, bytes, consumed, aux)"""
    st, data, consumed, aux = want
    assert (res.status, res.written) == (st, len(data)), (where, res.status, st, res.written, len(data))
    assert bytes(out[:len(data)].cpu().numpy()) == data, where
    if st == 0:
        assert res.consumed == consumed, (where, res.consumed, consumed)
    elif st != spng.NEED_MORE_INPUT:
        assert tuple(res.aux) == tuple(aux), (where, tuple(res.aux), aux)


@pytest.fixture(scope="module")
def wants():
    """the oracle's answer for every case, asked once"""
    return {n: dc.expected(dc.case(n)) for n in dc.NAMES}


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_alone_under_every_knob(gpu, wants, name):
    """INFLATE_SERIAL, and INFLATE_AUTO with segments of the default length and of 256 bytes (geometry.hpp `inflate_segment_bytes` rounds to multiples of 256 and
    takes 256 as it is) x one workgroup per stream and 4 parts (one stream: 3 marker parts, the 8 KiB geometry)"""
    s = gpu.load()
    c = dc.case(name)
    d_z = s.to_device(c.stream)
    s.configure(spng.CFG_INFLATE_MODE, spng.INFLATE_SERIAL)
    try:
        outs, res = s.inflate_batch([d_z], [cap_of(c)], c.fmt)
    finally:
        s.configure(spng.CFG_INFLATE_MODE, spng.INFLATE_AUTO)
    same(res[0], outs[0], wants[name], (name, "serial"))
    for segment in (0, 256):
        for parts in (1, 4):
            s.configure(spng.CFG_SEGMENT_BYTES, segment)
            s.configure(spng.CFG_RESOLVE_PARTS, parts)
            try:
                outs, res = s.inflate_batch([d_z], [cap_of(c)], c.fmt)
            finally:
                s.configure(spng.CFG_SEGMENT_BYTES, 0)
                s.configure(spng.CFG_RESOLVE_PARTS, 0)
            same(res[0], outs[0], wants[name], (name, segment, parts))
            if c.valid:
                assert res[0].reserved == 1, f"{name}, segment {segment}, parts {parts}: fell back to the serial kernel"


def test_all_cases_in_one_batch_in_both_marker_geometries(gpu, wants):
    """SPNG_CFG_RESOLVE_PARTS 64: streams x 63 marker parts are more than the 256 of launch_pinf2_parts' rule, so they run the 4 KiB
    tiles (two workgroups per CU, 512 references per tile); 8 parts per stream stay below it and keep the 8 KiB tiles.  Either way
    every stream ends as it ends alone."""
    s = gpu.load()
    cases = [dc.case(n) for n in dc.NAMES]
    d_in = [s.to_device(c.stream) for c in cases]
    caps = [cap_of(c) for c in cases]
    alone = []
    for c, d_z, cap in zip(cases, d_in, caps):
        outs, res = s.inflate_batch([d_z], [cap], c.fmt)
        same(res[0], outs[0], wants[c.name], (c.name, "alone"))
        alone.append((res[0].status, res[0].written, res[0].consumed, tuple(res[0].aux), res[0].reserved,
                      bytes(outs[0][:res[0].written].cpu().numpy())))
    for parts, small_tiles in ((64, True), (8, False)):
        assert (len(cases) * (parts - 1) > 256) == small_tiles                   # (pinflate2.hip, launch_pinf2_parts)
        s.configure(spng.CFG_RESOLVE_PARTS, parts)
        try:
            outs, res = s.inflate_batch(d_in, caps, [c.fmt for c in cases])
        finally:
            s.configure(spng.CFG_RESOLVE_PARTS, 0)
        for c, o, r, a in zip(cases, outs, res, alone):
            same(r, o, wants[c.name], (c.name, "batch", parts))
            got = (r.status, r.written, r.consumed, tuple(r.aux), r.reserved, bytes(o[:r.written].cpu().numpy()))
            if r.status == spng.NEED_MORE_INPUT:                                 # (consumed and aux carry the resume point then)
                got, a = got[:2] + got[5:], a[:2] + a[5:]
            assert got == a, (c.name, parts, got[:5], a[:5])
            if c.valid:
                assert r.reserved == 1, f"{c.name}, {parts} parts: fell back to the serial kernel"


@pytest.mark.parametrize("piece", [7000, 100000])
@pytest.mark.parametrize("name", ["periods", "echo", "edges", "headers-deep15"])
def test_cases_pushed_in_pieces(gpu, name, piece):
    """spng_inflate_resume_batch: after every push the device answers as the oracle does for that prefix"""
    from test_gpu_resume import check_prefixes
    s = gpu.load()
    c = dc.case(name)
    data = c.info["data"]
    last, p = check_prefixes(s, c.stream, [piece], every=1)
    assert last.status == 0 and last.written == len(data) and last.consumed == len(c.stream) and p.out(len(data)) == data


@pytest.mark.parametrize("name", ["periods", "dense3"])
def test_one_block_cases_with_and_without_block_cuts(gpu, wants, name):
    """each is ONE block: with a 64 KiB threshold and 16 KiB segments it is cut and joined; the same bytes and the same result as
    without cuts, and the pipeline's own"""
    from test_gpu_blockcuts import inflate_one
    s = gpu.load()
    c = dc.case(name)
    data = c.info["data"]
    assert len(c.blocks) == 1
    r0, out0, st0, _ = inflate_one(s, c.stream, len(data) + 64, cut=spng.BLOCK_CUT_NEVER, segment=16384)
    r1, out1, (tried, joined, redone), _ = inflate_one(s, c.stream, len(data) + 64, cut=65536, segment=16384)
    print(f"{name}: cuts tried {tried} joined {joined} redone {redone}")
    assert st0 == (0, 0, 0) and tried >= 1
    assert (r0.status, r0.written, r0.consumed, r0.reserved, tuple(r0.aux)) == (r1.status, r1.written, r1.consumed, r1.reserved, tuple(r1.aux))
    assert out0 == out1 == data == wants[name][1]
    assert r1.status == 0 and r1.consumed == len(c.stream) and r1.reserved == 1, f"{name}: fell back to the serial kernel"


@pytest.mark.parametrize("fmt", ["raw", "gzip"])
@pytest.mark.parametrize("name", ["extremes", "echo"])
def test_cases_as_raw_and_gzip_streams(gpu, name, fmt):
    """raw DEFLATE (the iOS variant) has no checksum and a gzip member's CRC-32 is compared after the fact: nothing but the bytes
    tells a wrong decode from a right one"""
    from test_oracle_gzip import gw, raw_inflate
    s = gpu.load()
    c = dc.case(name)
    data = c.info["data"]
    cap = len(data) + 64
    if fmt == "raw":
        z, f = c.body, spng.FORMAT_IOS
        want = ph.orc_inflate(z, dc.RAW, cap=cap)
    else:
        z, f = ob.gzip_wrap(c.body, data), spng.FORMAT_GZIP
        want = gw.inflate(z, lambda p, _c: raw_inflate(p, cap), cap)
    assert want[0] == 0 and want[1] == data and want[2] == len(z)
    d_z = s.to_device(z)
    for mode in (spng.INFLATE_AUTO, spng.INFLATE_SERIAL):
        s.configure(spng.CFG_INFLATE_MODE, mode)
        try:
            outs, res = s.inflate_batch([d_z], [cap], f)
        finally:
            s.configure(spng.CFG_INFLATE_MODE, spng.INFLATE_AUTO)
        same(res[0], outs[0], want, (name, fmt, mode))
        if mode == spng.INFLATE_AUTO:
            assert res[0].reserved == 1, f"{name} as {fmt}: fell back to the serial kernel"
