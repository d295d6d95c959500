"""Destination bounds of the inflate and deflate entries on the device: the tables of tests/bounds_cases.py -- capacities that end
inside a match, on a match's last byte, at a block boundary, inside a stored block, inside a header or a trailer, on the staging
ring's drain threshold, and the exact need -- with every source and destination between 64 KiB of guard bytes at a chosen residue
from a 16-byte boundary (tests/bounds.py).  The answers are the oracle's, exactly: status, written, bytes, consumed (when done), error
payload; and no guard byte may change, in front of a destination or behind its capacity.  Bytes in [written, capacity) are
unspecified and not looked at.

Store paths and the rows that reach them: profiles/r17_bounds.md."""
import ctypes
import zlib

import numpy as np
import pytest

import bounds
import bounds_cases as bc
import pnghelp as ph
import swift_png_amd as spng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wants():
    """the oracle's answer for every inflate row, asked once"""
    return {(n, cap): bc.inflate_expected(n, cap) for n in bc.STREAMS for _, cap in bc.inflate_rows(n)}


def same(got, want, where, pipeline=None):
    """(Result, the destination's first `capacity` bytes) against the oracle's (status, bytes, consumed, aux)"""
    res, dst = got
    st, data, consumed, aux = want
    assert (res.status, res.written) == (st, len(data)), (where, res.status, st, res.written, len(data))
    assert dst[:len(data)] == data, where
    if st == 0:
        assert res.consumed == consumed, (where, res.consumed, consumed)
    elif st != spng.NEED_MORE_INPUT:
        assert tuple(res.aux) == tuple(aux), (where, tuple(res.aux), aux)
    if pipeline is not None and st == 0:
        assert res.reserved == 1, f"{where}: an exact capacity cost the pipeline (fell back to the serial kernel)"


def knobs(s):
    """INFLATE_SERIAL, then INFLATE_AUTO x segments of the default length and of 256 bytes x one workgroup per stream and 4 parts"""
    s.configure(spng.CFG_INFLATE_MODE, spng.INFLATE_SERIAL)
    try:
        yield ("serial",), False
    finally:
        s.configure(spng.CFG_INFLATE_MODE, spng.INFLATE_AUTO)
    for segment in (0, 256):
        for parts in (1, 4):
            s.configure(spng.CFG_SEGMENT_BYTES, segment)
            s.configure(spng.CFG_RESOLVE_PARTS, parts)
            try:
                yield (segment, parts), True
            finally:
                s.configure(spng.CFG_SEGMENT_BYTES, 0)
                s.configure(spng.CFG_RESOLVE_PARTS, 0)


@pytest.mark.parametrize("name", bc.STREAMS)
def test_inflate_every_row_alone_under_every_knob(gpu, wants, name):
    s = gpu.load()
    st = bc.stream(name)
    for knob, auto in knobs(s):
        for label, cap in bc.inflate_rows(name):
            where = (name, label, cap) + knob
            got = bounds.inflate(s, [st.z], [cap], st.fmt, where=str(where))[0]
            same(got, wants[name, cap], where, pipeline=True if auto and cap in (st.n, st.n + 1) else None)


@pytest.mark.parametrize("name", bc.STREAMS)
def test_inflate_all_rows_of_a_stream_in_one_call(gpu, wants, name):
    """the same source, a destination per row"""
    s = gpu.load()
    st, rows = bc.stream(name), bc.inflate_rows(name)
    got = bounds.inflate(s, [st.z] * len(rows), [c for _, c in rows], st.fmt, where=name)
    for g, (label, cap) in zip(got, rows):
        same(g, wants[name, cap], (name, label, cap))


def test_inflate_all_rows_of_all_streams_in_one_call(gpu, wants):
    s = gpu.load()
    rows = [(n, label, cap) for n in bc.STREAMS for label, cap in bc.inflate_rows(n)]
    s.configure(spng.CFG_RESOLVE_PARTS, 8)
    try:
        got = bounds.inflate(s, [bc.stream(n).z for n, _, _ in rows], [c for _, _, c in rows], [bc.stream(n).fmt for n, _, _ in rows], where="all")
    finally:
        s.configure(spng.CFG_RESOLVE_PARTS, 0)
    for g, (n, label, cap) in zip(got, rows):
        same(g, wants[n, cap], (n, label, cap))


@pytest.mark.parametrize("name", ["a", "echo"])
def test_inflate_at_every_alignment(gpu, wants, name):
    """dst at every residue with src at residue 0, src at every residue with dst at residue 5; capacities N and N - 1; the serial
    kernel and the pipeline with one part and four.  One call per configuration: a stream per (residue, capacity)."""
    s = gpu.load()
    st = bc.stream(name)
    combos = [(0, r) for r in range(16)] + [(r, 5) for r in range(16)]
    zs, caps, sres, dres = [], [], [], []
    for sr, dr in combos:
        for cap in (st.n, st.n - 1):
            zs.append(st.z); caps.append(cap); sres.append(sr); dres.append(dr)
    for mode, parts in ((spng.INFLATE_SERIAL, 0), (spng.INFLATE_AUTO, 1), (spng.INFLATE_AUTO, 4)):
        s.configure(spng.CFG_INFLATE_MODE, mode)
        s.configure(spng.CFG_RESOLVE_PARTS, parts)
        try:
            got = bounds.inflate(s, zs, caps, st.fmt, sres, dres, where=f"{name} mode {mode} parts {parts}")
        finally:
            s.configure(spng.CFG_INFLATE_MODE, spng.INFLATE_AUTO)
            s.configure(spng.CFG_RESOLVE_PARTS, 0)
        for g, cap, sr, dr in zip(got, caps, sres, dres):
            same(g, wants[name, cap], (name, cap, "src residue", sr, "dst residue", dr, mode, parts))


def test_inflate_periods_with_block_cuts(gpu, wants):
    """one huge block cut at 64 KiB with 16 KiB segments: the same answers as without cuts"""
    s = gpu.load()
    st, rows = bc.stream("periods"), dict(bc.inflate_rows("periods"))
    for cut in (spng.BLOCK_CUT_NEVER, 65536):
        s.configure(spng.CFG_BLOCK_CUT_BYTES, cut)
        s.configure(spng.CFG_SEGMENT_BYTES, 16384)
        try:
            for label in ("N", "N-1", "inside-match"):
                got = bounds.inflate(s, [st.z], [rows[label]], st.fmt, where=f"periods {label} cut {cut}")[0]
                tried = s.cut_stats()[0]
                same(got, wants["periods", rows[label]], ("periods", label, cut))
                if cut == 65536 and label == "N":
                    assert tried >= 1 and got[0].reserved == 1
        finally:
            s.configure(spng.CFG_BLOCK_CUT_BYTES, 0)
            s.configure(spng.CFG_SEGMENT_BYTES, 0)


@pytest.mark.parametrize("below", [0, 1])
def test_inflate_resumed_into_an_exact_destination(gpu, below):
    """stream (a) in pieces of 7000 through spng_inflate_resume_batch: after every push the oracle's answer for that prefix at that
    capacity, the guards whole"""
    s = gpu.load()
    st = bc.stream("a")
    cap = st.n - below
    p = bounds.InflatePush(s, st.z, cap, st.fmt)
    res = None
    for end in list(range(7000, len(st.z), 7000)) + [len(st.z)]:
        res, dst = p.push(end, where=f"resumed, {end} bytes, capacity {cap}")
        want = ph.orc_inflate(st.z[:end], st.fmt, cap=cap)
        same((res, dst), want, ("resumed", end, cap))
        if res.status not in (spng.DONE, spng.NEED_MORE_INPUT):
            break
    assert res.status == (spng.E_OUTPUT_CAPACITY if below else spng.DONE)


# ---- deflate -----------------------------------------------------------------------------------------------------------------------

def same_deflate(got, row, where):
    res, dst = got
    name, level, fmt, e, label, cap = row
    status, written, consumed, head = bc.deflate_expected(name, level, fmt, e, cap)
    assert (res.status, res.written, res.consumed) == (status, written, consumed), (where, row[:1] + row[1:], res.status, res.written, res.consumed, written)
    assert dst[:len(head)] == head, (where, row)


def run_deflate_rows(s, rows, where, src_res=0, dst_res=0):
    data = bc.inputs()
    got = bounds.deflate(s, [data[r[0]] for r in rows], [r[5] for r in rows], [r[2] for r in rows], [r[1] for r in rows],
                         [0 if r[3] == 15 else r[3] for r in rows], src_res, dst_res, where=where)
    for g, r in zip(got, rows):
        same_deflate(g, r, where)


@pytest.mark.parametrize("level", bc.LEVELS)
def test_deflate_every_row_of_a_level_in_one_call(gpu, level):
    """every (input, format, capacity) of the table, mixed formats, one spng_deflate_batch"""
    s = gpu.load()
    rows = bc.deflate_rows(level)
    assert len(rows) > 300
    run_deflate_rows(s, rows, f"level {level}")


@pytest.mark.parametrize("level", bc.LEVELS)
def test_deflate_rows_alone(gpu, level):
    """L, L - 1 and 0 of the 5000- and 70 000-byte inputs, one stream per call"""
    s = gpu.load()
    for r in bc.deflate_rows(level, ("mix5000", "scan70000")):
        if r[4] in ("L", "L-1", "0"):
            run_deflate_rows(s, [r], f"alone {r}")


@pytest.mark.parametrize("level", bc.FAMILY_LEVELS)
def test_deflate_at_every_alignment(gpu, level):
    s = gpu.load()
    L = len(bc.full("mix5000", level, bc.ZLIB))
    combos = [(0, r) for r in range(16)] + [(r, 5) for r in range(16)]
    rows, sres, dres = [], [], []
    for sr, dr in combos:
        for label, cap in (("L", L), ("L-1", L - 1)):
            rows.append(("mix5000", level, bc.ZLIB, 15, label, cap)); sres.append(sr); dres.append(dr)
    run_deflate_rows(s, rows, f"alignment, level {level}", sres, dres)


@pytest.mark.parametrize("fmt", [bc.ZLIB, bc.GZIP])
@pytest.mark.parametrize("level", bc.FAMILY_LEVELS)
@pytest.mark.parametrize("name", ["mix5000", "scan70000"])
def test_deflate_resumed_into_a_short_destination(gpu, name, level, fmt):
    """pieces of 4097 through spng_deflate_resume_batch: before the overflow every push wants more input and leaves a prefix of the
    stream; from the push that overflows on every push answers SPNG_E_OUTPUT_CAPACITY; the last reports what the whole stream needs;
    the first `capacity` bytes are the stream's own; guards whole after every push"""
    s = gpu.load()
    data, f = bc.inputs()[name], bc.full(name, level, fmt)
    L = len(f)
    for cap in (L, L - 1, L // 2 | 1, 1):
        p = bounds.DeflatePush(s, data, cap, fmt, level)
        over, seen = False, 0
        ends = list(range(4097, len(data), 4097)) + [len(data)]
        for end in ends:
            last = end == len(data)
            where = (name, level, fmt, cap, end)
            res, dst = p.push(end, last, where=str(where))
            if res.status == spng.E_OUTPUT_CAPACITY:
                over = True
                assert res.written > cap, where
            else:
                assert not over, (where, "a push after the overflow answered", res.status)
                assert res.status == (spng.DONE if last else spng.NEED_MORE_INPUT), (where, res.status)
                assert seen <= res.written <= cap and dst[:res.written] == f[:res.written], where
            assert res.written >= seen, where
            seen = res.written
            if last:
                assert over == (cap < L) and res.written == L and res.consumed == len(data), (where, res.status, res.written, L)
                assert dst[:min(cap, L)] == f[:min(cap, L)], where


# ---- host-pointer forms ----------------------------------------------------------------------------------------------------------------

def test_host_pointer_forms_leave_the_bytes_behind_the_capacity(gpu):
    """spng_inflate and spng_deflate_window with a host buffer of capacity + 64"""
    s = gpu.load()
    st = bc.stream("a")
    for cap in (st.n, st.n - 1, 0):
        buf = (ctypes.c_uint8 * (cap + 64))(*([0xEE] * (cap + 64)))
        res = spng.Result()
        spng._check(s.lib, s.lib.spng_inflate(s.ctx, spng._cbuf(st.z), len(st.z), st.fmt, buf, cap, ctypes.byref(res)))
        same((res, bytes(buf[:cap])), bc.inflate_expected("a", cap), ("spng_inflate", cap))
        assert bytes(buf[cap:]) == b"\xee" * 64, ("spng_inflate", cap)
    data = bc.inputs()["mix5000"]
    for level in bc.FAMILY_LEVELS:
        for fmt in (bc.ZLIB, bc.GZIP):
            L = len(bc.full("mix5000", level, fmt))
            for cap in (L, L - 1, 0):
                buf = (ctypes.c_uint8 * (cap + 64))(*([0xEE] * (cap + 64)))
                res = spng.Result()
                spng._check(s.lib, s.lib.spng_deflate_window(s.ctx, spng._cbuf(data), len(data), fmt, level, 15, buf, cap, ctypes.byref(res)))
                same_deflate((res, bytes(buf[:cap])), ("mix5000", level, fmt, 15, "", cap), "spng_deflate_window")
                assert bytes(buf[cap:]) == b"\xee" * 64, ("spng_deflate_window", level, fmt, cap)


# ---- decode ----------------------------------------------------------------------------------------------------------------------------

def test_decode_batch_with_exact_rows_and_storage(gpu):
    """three images in one spng_decode_batch, rows_cap == U and the storage exactly S, both between guards; IDAT streams that inflate
    to U, U - 1 and U + 1 bytes"""
    s = gpu.load()
    rng = np.random.default_rng(17)
    shapes = [(64, 64, 8, 6, 4, False), (33, 20, 4, 3, 1, True), (9, 17, 16, 2, 3, True)]      # w, h, depth, colour type, channels, Adam7
    for delta in (0, -1, 1):
        pngs, idats, U, S = [], [], [], []
        for w, h, depth, color, ch, inter in shapes:
            png = ph.Png(w, h, depth, color, inter, False, b"")
            u, size = ph.orc_sizes(png)
            storage = rng.integers(0, 1 << min(depth, 8), size, dtype=np.uint8)
            rows = ph.orc_filter(storage, w, h, depth, ch, inter)
            assert len(rows) == u
            idats.append(zlib.compress(rows[:u - 1] if delta < 0 else rows + b"\0" * delta, 6))
            pngs.append(png); U.append(u); S.append(size)
        a_rows = bounds.Arena(s, idats, U, 3, 7)
        a_sto = bounds.Arena(s, [b""] * 3, S, 0, 9)
        descs = (spng.ImageDesc * 3)()
        for i, (w, h, depth, color, ch, inter) in enumerate(shapes):
            descs[i] = spng.ImageDesc(a_rows.d_src.data_ptr() + a_rows.src_off[i], len(idats[i]), a_rows.d_dst.data_ptr() + a_rows.dst_off[i], U[i],
                                      a_sto.d_dst.data_ptr() + a_sto.dst_off[i], w, h, depth, ch, int(inter), spng.FORMAT_ZLIB, 0)
        res = s.decode_batch(descs)
        a_rows.check(f"rows, delta {delta}")
        storages = a_sto.check(f"storage, delta {delta}")
        for i, png in enumerate(pngs):
            st, want, aux = ph.orc_decode(png, idats[i])
            assert res[i].status == st, (delta, i, res[i].status, st)
            if delta == 0:
                assert st == 0
                assert storages[i] == want.tobytes(), (delta, i)
            elif st != spng.NEED_MORE_INPUT:
                assert tuple(res[i].aux) == tuple(aux), (delta, i)
