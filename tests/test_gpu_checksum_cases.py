"""The checksum table (tests/checksum_cases.py) on the device: every Adler-32 and CRC-32 the library computes, driven to the limits of
its partial sums.  What a stream must answer is Python's zlib / gzip, the oracle's deflate and oracle/gzip_wrap.py, exactly: status,
byte count, bytes, consumed, and for a twin with a flipped trailer bit SPNG_E_STREAM_CHECKSUM with aux == (declared, the RIGHT sum) --
a kernel that computes a wrong sum cannot pass a stream and its twin.

Which path a case reaches is asserted where the library says so: reserved == 1 is the pipeline's own verdict, and the part plan of a
call -- how many slots plan_parts gave the stream and how many parts pinf2_scan_kernel cut its chain into -- is read from the line the
library writes to stderr under SPNG_TRACE_PINFLATE ("parts n of m"; 0 of 0: one workgroup).  A forced count is an upper bound: the
streams that must split (cc.splits) are held to two parts or more, and the payload long enough for seven (cc.PARTS7) to exactly 2, 3
and 7, the counts the emulator reports for the same streams (tests/test_checksum_cases.py).
profiles/r18_checksums.md has the table of cases and paths."""
import gzip
import os
import re
import zlib

import pytest

import bounds
import checksum_cases as cc
import pnghelp as ph
import swift_png_amd as spng
from test_oracle_gzip import gw, raw_inflate

pytestmark = pytest.mark.gpu

SEGMENT = 256                                    # bytes of a segment where parts are forced (as tests/test_checksum_cases.py)


class knobs:
    """the inflate knobs for the length of a with block"""

    def __init__(self, s, mode=spng.INFLATE_AUTO, parts=0, segment=0):
        self.s, self.v = s, ((spng.CFG_INFLATE_MODE, mode), (spng.CFG_RESOLVE_PARTS, parts), (spng.CFG_SEGMENT_BYTES, segment))

    def __enter__(self):
        for k, v in self.v:
            self.s.configure(k, v)

    def __exit__(self, *exc):
        for k, _ in self.v:
            self.s.configure(k, 0)


PATHS = [("serial", dict(mode=spng.INFLATE_SERIAL), False), ("pipeline", dict(parts=1), True),
         ("parts-2", dict(parts=2, segment=SEGMENT), True), ("parts-3", dict(parts=3, segment=SEGMENT), True), ("parts-7", dict(parts=7, segment=SEGMENT), True)]


def same(res, out, st, where, pipeline=False):
    n = len(st.data)
    assert (res.status, res.written) == (st.status, n), (where, res.status, st.status, res.written, n, tuple(res.aux))
    assert bytes(out[:n]) == st.data, where
    if st.status == cc.DONE:
        assert res.consumed == len(st.z), (where, res.consumed, len(st.z))
    else:
        assert tuple(res.aux) == st.aux, (where, [hex(a) for a in res.aux], [hex(a) for a in st.aux])
    if pipeline:
        assert res.reserved == 1, f"{where}: the pipeline left the stream to the serial kernel"


class traced:
    """SPNG_TRACE_PINFLATE for the length of a with block; plan(): (parts made, slots) of stream 0 of the most recent call"""

    def __init__(self, capfd):
        self.capfd = capfd

    def __enter__(self):
        os.environ["SPNG_TRACE_PINFLATE"] = "1"
        self.capfd.readouterr()
        return self

    def __exit__(self, *exc):
        del os.environ["SPNG_TRACE_PINFLATE"]

    def plan(self, where):
        err = self.capfd.readouterr().err
        found = re.findall(r"\[pinflate\] stream 0: .* parts (\d+) of (\d+)", err)
        assert found, (where, "no trace of the call", err[-300:])
        return int(found[-1][0]), int(found[-1][1])


def prefix_status(st, cut):
    """the oracle's status for the first `cut` bytes of a stream"""
    n = len(st.data)
    if st.fmt == cc.GZIP:
        return gw.inflate(st.z[:cut], lambda p, _c: raw_inflate(p, max(n, 1)), max(n, 1))[0]
    return ph.orc_inflate(st.z[:cut], st.fmt, cap=max(n, 1))[0]


def host(t, n):
    return bytes(t[:n].cpu().numpy()) if n else b""


# ---- inflate -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pname", cc.PAYLOADS)
def test_inflate_every_stream_alone_on_every_path(gpu, capfd, pname):
    """the serial kernel (`flush`), the pipeline with one workgroup (the tile loop, the bytes behind the last unit), and 2, 3 and 7 parts
    (pinf2_fixup_kernel, pinf2_verdict_kernel); gzip members: piece_crc / fold_pieces behind each of them.  With parts forced the
    stream has as many slots as were asked for (plan_parts did not fall back to one workgroup), and a stream that must split did."""
    s = gpu.load()
    sts = cc.streams(pname)
    d_in = [s.to_device(st.z) for st in sts]
    for label, kn, auto in PATHS:
        with knobs(s, **kn), traced(capfd) as trace:
            for st, d in zip(sts, d_in):
                outs, res = s.inflate_batch([d], [len(st.data)], st.fmt)
                same(res[0], host(outs[0], len(st.data)), st, (st.name, label), pipeline=auto and len(st.data) > 0)
                if auto:
                    made, slots = trace.plan((st.name, label))
                    forced = kn["parts"]
                    assert slots == (forced if forced > 1 else 0), (st.name, label, made, slots)
                    assert made <= slots and (made >= 2 if forced > 1 and cc.splits(st) else True), (st.name, label, made, slots)


def test_inflate_in_exactly_the_parts_asked_for(gpu, capfd):
    """2, 3 and 7 parts, each honoured in full: the payload long enough for seven, zlib's stream and the oracle's, with their twins"""
    s = gpu.load()
    for st in cc.streams(cc.PARTS7):
        if st.fmt == cc.GZIP:
            continue
        d = s.to_device(st.z)
        for parts in (2, 3, 7):
            with knobs(s, parts=parts, segment=SEGMENT), traced(capfd) as trace:
                outs, res = s.inflate_batch([d], [len(st.data)], st.fmt)
                same(res[0], host(outs[0], len(st.data)), st, (st.name, parts), pipeline=True)
                assert trace.plan((st.name, parts)) == (parts, parts), (st.name, parts)


def test_inflate_all_streams_in_one_batch_of_mixed_formats(gpu):
    s = gpu.load()
    sts = cc.all_streams()
    got = bounds.inflate(s, [st.z for st in sts], [len(st.data) for st in sts], [st.fmt for st in sts], where="all")
    for (res, out), st in zip(got, sts):
        same(res, out, st, st.name)


@pytest.mark.parametrize("pname", cc.PAYLOADS)
def test_inflate_pushed_in_pieces(gpu, pname):
    """spng_inflate_resume_batch: cut inside the header, on a block boundary, one byte before the trailer and inside it, then the rest;
    and the whole stream in one push, by the pipeline and by the serial kernel alone -- resume_adler_kernel / resume_post_kernel check the
    Adler-32 of every stream the pipeline did not hold from its first bit, the gzip kernels the CRC-32"""
    s = gpu.load()
    for st in cc.streams(pname):
        if st.fmt == cc.RAW:
            continue
        n = len(st.data)
        p = bounds.InflatePush(s, st.z, n, st.fmt)
        for cut in cc.push_cuts(st) + [len(st.z)]:
            res, out = p.push(cut, where=f"{st.name} cut {cut}")
            # what the prefix answers is the oracle's: more input wanted -- or, for a gzip twin cut inside ISIZE, the checksum error already
            want = prefix_status(st, cut)
            assert res.status == want, (st.name, cut, res.status, want)
            if want != spng.NEED_MORE_INPUT:
                assert want == st.status
                same(res, out, st, (st.name, "pushed", cc.push_cuts(st), cut))
                break
        for mode in (spng.INFLATE_AUTO, spng.INFLATE_SERIAL):
            with knobs(s, mode=mode):
                res, out = bounds.InflatePush(s, st.z, n, st.fmt).push(len(st.z), where=st.name)
                same(res, out, st, (st.name, "one push", mode))
                assert n == 0 or res.reserved == (1 if mode == spng.INFLATE_AUTO else 0), (st.name, mode, res.reserved)


@pytest.mark.parametrize("pname", cc.ADLER_PAYLOADS)
def test_inflate_at_destination_residues(gpu, pname):
    """d_dst at 0, 1 and 15 from a 16-byte boundary: the units of the checksums lie on multiples of 16 of the STREAM position, whatever
    the address (`pos & 15` is subtracted from the tile's position); between guard bytes"""
    s = gpu.load()
    sts = [st for st in cc.streams(pname) if st.fmt == cc.ZLIB]
    for label, kn, auto in (PATHS[0], PATHS[1], PATHS[3]):
        with knobs(s, **kn):
            for st in sts:
                got = bounds.inflate(s, [st.z] * 3, [len(st.data)] * 3, st.fmt, dst_res=[0, 1, 15], where=f"{st.name} {label}")
                for (res, out), r in zip(got, (0, 1, 15)):
                    same(res, out, st, (st.name, label, "residue", r))


# ---- deflate -------------------------------------------------------------------------------------------------------------------------

LEVELS, SHAPES, GROUPS = cc.DEFLATE_LEVELS, cc.DEFLATE_SHAPES, cc.DEFLATE_GROUPS


def deflated(z, pname, level, fmt, exponent, where):
    """byte for byte the oracle's stream -- and, said once more without it, the trailer is Python's sum and Python reads the stream"""
    data = cc.payload(pname)
    assert z == cc.deflate_expected(pname, level, fmt, exponent), (where, len(z))
    if fmt == cc.ZLIB:
        assert z[-4:] == zlib.adler32(data).to_bytes(4, "big") and zlib.decompress(z) == data, where
    else:
        assert z[-8:] == zlib.crc32(data).to_bytes(4, "little") + len(data).to_bytes(4, "little") and gzip.decompress(z) == data, where


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("level", LEVELS)
def test_deflate_every_payload_alone(gpu, level, group):
    """d3_insert / d3_insert_quad of both search kernels, adler32_word, the stored tail, gzip's CRC-32 of the input: one stream a call"""
    s = gpu.load()
    for pname in GROUPS[group] + (cc.GZ if group == "values" else []):
        data = cc.payload(pname)
        d = s.to_device(data)
        for fmt, e in SHAPES if pname in cc.ADLER_PAYLOADS else SHAPES[2:3]:
            outs, res = s.deflate_batch([d], level, fmt, exponents=[e])
            assert res[0].status == spng.DONE and res[0].consumed == len(data), (pname, level, fmt, e, res[0].status)
            deflated(host(outs[0], res[0].written), pname, level, fmt, e, (pname, level, fmt, e))


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("level", LEVELS)
def test_deflate_every_payload_in_one_call_of_256_streams(gpu, level, group):
    """the same streams beside 255 others: fewer search chunks per stream, so other chunk boundaries and another warm-up of `pm`"""
    s = gpu.load()
    jobs = [(p, fmt, e) for p in GROUPS[group] for fmt, e in SHAPES]
    filler = s.to_device(cc.payload("gz-257"))
    d_in = {p: s.to_device(cc.payload(p)) for p in GROUPS[group]}
    streams = [d_in[p] for p, _, _ in jobs] + [filler] * (256 - len(jobs))
    assert len(streams) == 256
    fmts = [f for _, f, _ in jobs] + [cc.ZLIB] * (256 - len(jobs))
    exps = [e for _, _, e in jobs] + [15] * (256 - len(jobs))
    outs, res = s.deflate_batch(streams, level, fmts, exponents=exps)
    for i, (p, fmt, e) in enumerate(jobs):
        assert res[i].status == spng.DONE, (p, level, fmt, e, res[i].status)
        deflated(host(outs[i], res[i].written), p, level, fmt, e, (p, level, fmt, e, "of 256"))
    for i in range(len(jobs), 256):
        assert res[i].status == spng.DONE and host(outs[i], res[i].written) == cc.deflate_expected("gz-257", level, cc.ZLIB, 15)


PUSH_CUTS = (65520, 65521, 65522)


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("level", LEVELS)
def test_deflate_pushed_in_three_pieces(gpu, level, group):
    """spng_deflate_resume_batch with the first cut at 65520, 65521 and 65522 (the second 70001 bytes on): the position modulo 65521
    restarts with every push.  `ff` and `high` in every shape at every cut; the other payloads long enough one shape a cut."""
    s = gpu.load()
    for pname in GROUPS[group]:
        data = cc.payload(pname)
        n = len(data)
        if n <= PUSH_CUTS[-1]:
            continue
        combos = [(c, f, e) for c in PUSH_CUTS for f, e in SHAPES] if pname in ("ff", "high") else list(zip(PUSH_CUTS, (cc.GZIP, cc.ZLIB, cc.ZLIB), (8, 15, 8)))
        for cut, fmt, e in combos:
            p = bounds.DeflatePush(s, data, int(s.lib.spng_deflate_bound(n)), fmt, level, e)
            for upto in (cut, min(cut + 70001, n - 1)):
                res, _ = p.push(upto, False, where=f"{pname} {level} {cut}")
                assert res.status == spng.NEED_MORE_INPUT, (pname, level, cut, upto, res.status)
            res, out = p.push(n, True, where=f"{pname} {level} {cut}")
            assert res.status == spng.DONE and res.consumed == n, (pname, level, cut, res.status)
            deflated(out[:res.written], pname, level, fmt, e, (pname, level, fmt, e, "pushed", cut))


# ---- the other entries ---------------------------------------------------------------------------------------------------------------

def test_adler32_and_crc32_entries(gpu):
    """spng_adler32 (adler_partial_kernel and the host fold) over the whole table; spng_crc32 over the lengths at which gzip's 256 pieces
    change shape"""
    s = gpu.load()
    for p in cc.PAYLOADS:
        assert s.adler32(cc.payload(p)) == zlib.adler32(cc.payload(p)), p
    for p in cc.GZ + ["ff", "high", "tiny-0"]:
        assert s.crc32(cc.payload(p)) == zlib.crc32(cc.payload(p)), p


def test_gzip_header_table_in_one_call(gpu):
    s = gpu.load()
    rows = cc.header_rows()
    cap = len(cc.H_DATA)
    wants = [gw.inflate(z, lambda p, _c: raw_inflate(p, cap), cap) for _, z, _ in rows]
    got = bounds.inflate(s, [z for _, z, _ in rows], [cap] * len(rows), cc.GZIP, where="header table")
    for (name, z, _), (res, out), want in zip(rows, got, wants):
        assert (res.status, res.written) == (want[0], len(want[1])), (name, res.status, want[0], res.written)
        assert out[:len(want[1])] == want[1], name
        if want[0] == cc.DONE:
            assert res.consumed == want[2] == len(z), name
        elif want[0] != cc.NEED_MORE_INPUT:
            assert tuple(res.aux) == tuple(want[3]), (name, tuple(res.aux), want[3])
    assert {w[0] for w in wants} >= {0, 1, gw.E_GZIP_SIGIL, gw.E_GZIP_METHOD, gw.E_GZIP_FLAG_BITS, gw.E_GZIP_HEADER_CHECKSUM}


def test_gzip_header_arrives_byte_by_byte(gpu):
    """every prefix of the member with all fields as a push of its own (the header is parsed again in every call), then the rest"""
    s = gpu.load()
    m, h = cc.member(cc.ALL_FIELDS)
    p = bounds.InflatePush(s, m, len(cc.H_DATA), cc.GZIP)
    for cut in range(h + 2):
        res, _ = p.push(cut, where=f"prefix {cut}")
        assert res.status == spng.NEED_MORE_INPUT, (cut, res.status)
    res, out = p.push(len(m), where="whole")
    assert (res.status, res.written, res.consumed) == (spng.DONE, len(cc.H_DATA), len(m)) and out == cc.H_DATA
