"""Block cuts for streams that arrive in pieces (spng_inflate_resume_batch; csrc/pinflate2.hip "resumed calls", csrc/host_decode.hip
cut_into_segments): a call whose state is not all zero and that brings at least SPNG_CFG_BLOCK_CUT_BYTES behind its resume point
decodes the huge block it stands in -- or in front of -- on many waves, from the exact token of its state, and hands the tail the end of
the input cuts off to the serial kernel at the last proven join.  After every push: what the oracle reports for the same prefix, and
what the same push reports under SPNG_BLOCK_CUT_NEVER, states included.  No clock is asserted on (times are printed)."""
import ctypes
import hashlib
import sys
import time
import zlib

import numpy as np
import pytest

import oneblock as ob
import pnghelp as ph
import swift_png_amd as spng
from test_gpu_blockcuts import KINDS, make, scanlines
from test_gpu_resume import Pusher

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(ph.ROOT / "oracle"))
import gzip_wrap as gw          # noqa: E402


def oracle(seen, fmt, cap):
    if fmt == spng.FORMAT_GZIP:
        return gw.inflate(seen, lambda p, c: ph.orc_inflate(p, spng.FORMAT_IOS, cap), cap)
    return ph.orc_inflate(seen, fmt, cap)


def split(z, first, k):
    """a first piece of `first` bytes, then k roughly equal ones"""
    rest = len(z) - first
    step = (rest + k - 1) // k
    return [z[:first]] + [z[first + i * step:first + (i + 1) * step] for i in range(k)]


def knobs(s, cut=None, segment=None):
    s.configure(spng.CFG_BLOCK_CUT_BYTES, 0 if cut is None else cut)
    s.configure(spng.CFG_SEGMENT_BYTES, 0 if segment is None else segment)


def run_pushes(s, parts, cap, fmt=spng.FORMAT_ZLIB, cut=None, segment=None, stop_on_error=True):
    """the pieces pushed one by one on a fresh Pusher under the given knobs -> (Pusher, per push: (status, written, consumed, aux),
    the state returned, spng_cut_stats, milliseconds)"""
    knobs(s, cut, segment)
    try:
        p = Pusher(s, fmt, cap)
        rows = []
        for piece in parts:
            s.sync()
            t0 = time.perf_counter()
            res = p.push(piece)
            s.sync()
            ms = (time.perf_counter() - t0) * 1e3
            rows.append(((res.status, res.written, res.consumed, (res.aux[0], res.aux[1])), p.state, s.cut_stats(), ms))
            if stop_on_error and res.status not in (0, 1):
                break
    finally:
        knobs(s)
    return p, rows


def check_against_oracle(p, rows, parts, fmt, cap, data=None):
    seen = b""
    for k, (piece, (got, state, stats, ms)) in enumerate(zip(parts, rows)):
        seen += piece
        st, out, consumed, aux = oracle(seen, fmt, cap)
        assert got[0] == st, (k, got, st)
        assert got[1] == len(out), (k, got, len(out))
        assert hashlib.sha256(p.out(got[1])).digest() == hashlib.sha256(out).digest(), k     # (the buffer still holds every prefix)
        if st not in (0, 1):
            assert got[3] == tuple(aux), k
        if st == 0:
            assert got[2] == consumed, k
    if data is not None:
        assert rows[-1][0][0] == 0 and p.out(len(data)) == data


@pytest.fixture(scope="module")
def blocks():
    return {"fixed": ob.one_fixed_block(11, 32 << 20), "dynamic": ob.one_dynamic_block(7, 24 << 20)}


@pytest.fixture(scope="module")
def pushed(gpu, blocks):
    """case 1 and 2 share their runs: {which: (parts, automatic run, run under SPNG_BLOCK_CUT_NEVER)}"""
    s = gpu.load()
    out = {}
    for which, (data, z) in blocks.items():
        parts = split(z, 65536, 4)
        out[which] = (parts, run_pushes(s, parts, len(data) + 64), run_pushes(s, parts, len(data) + 64, cut=spng.BLOCK_CUT_NEVER))
    return out


@pytest.mark.parametrize("which", ["fixed", "dynamic"])
def test_large_pushes_inside_one_block_are_cut(gpu, blocks, pushed, which):
    data, z = blocks[which]
    parts, (p, rows), _ = pushed[which]
    for k, (got, state, stats, ms) in enumerate(rows):
        print(f"{which} push {k}: {len(parts[k])} bytes in {ms:.1f} ms, status {got[0]} written {got[1]}, state {state}, cuts {stats}")
    assert len(rows) == len(parts)
    check_against_oracle(p, rows, parts, spng.FORMAT_ZLIB, len(data) + 64, data)
    # the state moves forward in all four words, and stands inside the block after every push but the last
    for a, b in zip(p.states[:-1], p.states[1:-1]):
        assert all(y >= x for x, y in zip(a, b)), (a, b)
        assert b[2] > a[2] and b[3] > a[3] and b[2] > b[0], (a, b)
    for k in range(1, len(parts) - 1):
        tried, joined, redone = rows[k][2]
        assert tried >= 1 and joined >= 1 and redone == 0, (k, rows[k][2])
    last = rows[-1][0]
    assert last[0] == 0 and last[1] == len(data) and last[2] == len(z)
    assert rows[-1][2][0] >= 1 and rows[-1][2][2] == 0, "the final push reaches the final block by joins"
    assert zlib.adler32(p.out(len(data))) == int.from_bytes(z[-4:], "big")


def test_checksum_over_all_pushes_is_compared(gpu, blocks):
    """the Adler-32 of a stream whose pushes were cut is taken over the whole output: a wrong trailer shows at the last push"""
    s = gpu.load()
    data, z = blocks["fixed"]
    bad = bytearray(z); bad[-1] ^= 1
    parts = split(bytes(bad), 65536, 4)
    _, rows = run_pushes(s, parts, len(data) + 64)
    assert [r[0][0] for r in rows[:-1]] == [1] * 4
    assert rows[-1][0][0] == spng.E_STREAM_CHECKSUM
    assert rows[-1][0][3] == (int.from_bytes(bad[-4:], "big"), zlib.adler32(data))


@pytest.mark.parametrize("which", ["fixed", "dynamic"])
def test_the_knob_changes_no_result(gpu, pushed, which):
    parts, (_, rows), (_, never) = pushed[which]
    print(f"{which}: automatic {sum(r[3] for r in rows):.1f} ms, never {sum(r[3] for r in never):.1f} ms over {len(parts)} pushes")
    assert [r[0] for r in rows] == [r[0] for r in never]
    assert [r[1] for r in rows] == [r[1] for r in never]
    assert all(r[2] == (0, 0, 0) for r in never)


def test_the_gate_zero_state_and_small_pieces(gpu, blocks):
    """a call with an all-zero state is a whole stream and keeps the plan it had; pushes below the threshold stay on the serial kernel"""
    s = gpu.load()
    data, z = blocks["fixed"]
    p, rows = run_pushes(s, [z], len(data) + 64)
    assert rows[0][0][:3] == (0, len(data), len(z)) and rows[0][2] == (0, 0, 0)
    assert hashlib.sha256(p.out(len(data))).digest() == hashlib.sha256(data).digest()
    data, z = ob.one_fixed_block(12, 4 << 20)
    parts = [z[i:i + 65536] for i in range(0, len(z), 65536)]
    p, rows = run_pushes(s, parts, len(data) + 64)
    assert all(r[2] == (0, 0, 0) for r in rows)
    assert rows[-1][0][:3] == (0, len(data), len(z)) and p.out(len(data)) == data


@pytest.mark.parametrize("kind", KINDS)
def test_the_gate_aggressive_cuts_on_ordinary_streams(gpu, kind):
    """a 64 KiB threshold and 16 KiB segments, 400 000-byte pieces: cuts wherever four segments in a row have no block start"""
    s = gpu.load()
    z = make(kind, 3 << 20)
    want = zlib.decompress(z)
    parts = [z[i:i + 400000] for i in range(0, len(z), 400000)]
    p, rows = run_pushes(s, parts, len(want) + 64, cut=65536, segment=16384)
    print(f"{kind}: {len(parts)} pushes, cuts {[r[2] for r in rows]}")
    check_against_oracle(p, rows, parts, spng.FORMAT_ZLIB, len(want) + 64, want)
    assert all(r[2][2] in (0, 1) for r in rows)


@pytest.mark.parametrize("case", ["other tables", "flipped"])
def test_streams_that_do_not_stitch_end_as_without_cuts(gpu, case):
    s = gpu.load()
    if case == "other tables":
        data, z = ob.dynamic_then_fixed(3, 1 << 20, 6 << 20)
        parts = split(z, 65536, 3)
    else:
        data, z = ob.one_dynamic_block(5, 24 << 20)
        b = bytearray(z); b[len(b) * 3 // 4] ^= 0x10
        z = bytes(b)
        parts = split(z, 65536, 4)
    p0, never = run_pushes(s, parts, len(data) + 64, cut=spng.BLOCK_CUT_NEVER)
    p1, rows = run_pushes(s, parts, len(data) + 64)
    print(f"{case}: statuses {[r[0][0] for r in rows]}, cuts {[r[2] for r in rows]}")
    assert [r[0] for r in rows] == [r[0] for r in never]
    assert [r[1] for r in rows] == [r[1] for r in never]
    assert p1.out(rows[-1][0][1]) == p0.out(never[-1][0][1])
    assert all(r[2] == (0, 0, 0) for r in never)
    if case == "other tables":
        assert rows[-1][0][0] == 0 and p1.out(len(data)) == data
        assert any(r[2][0] >= 1 for r in rows)
    else:
        check_against_oracle(p1, rows, parts, spng.FORMAT_ZLIB, len(data) + 64)


def test_output_capacity_in_a_large_push(gpu, blocks):
    s = gpu.load()
    data, z = blocks["fixed"]
    first, n = 65536, 65536 + (8 << 20)
    d_in = s.to_device(z[:n])
    want = oracle(z[:n], spng.FORMAT_ZLIB, len(data) + 64)
    seen = []
    for cut in (0, spng.BLOCK_CUT_NEVER):
        knobs(s, cut)
        try:
            small = s.empty(1 << 20)
            r0, state = s.inflate_resume(d_in, first, small, spng.FORMAT_ZLIB, (0, 0, 0, 0))
            assert r0.status == 1 and state[2] != 0
            r1, same = s.inflate_resume(d_in, n, small, spng.FORMAT_ZLIB, state)
            assert r1.status == spng.E_OUTPUT_CAPACITY and same == state
            grown = s.empty(len(data) + 64); grown[:small.numel()] = small
            r2, state2 = s.inflate_resume(d_in, n, grown, spng.FORMAT_ZLIB, state)
            stats = s.cut_stats()
        finally:
            knobs(s)
        assert r2.status == want[0] == 1 and r2.written == len(want[1])
        assert bytes(grown[:r2.written].cpu().numpy()) == want[1]
        seen.append(((r1.status, r1.written, r1.consumed, tuple(r1.aux)), (r2.status, r2.written, r2.consumed, tuple(r2.aux)), state2))
        if cut == 0:
            assert stats[0] >= 1 and stats[1] >= 1 and stats[2] == 0
    assert seen[0] == seen[1]


def resume_batch(s, items):
    """one spng_inflate_resume_batch call over several streams: items = (input tensor, bytes so far, output tensor, format, state)
    -> per stream (Result, next state)"""
    n = len(items)
    descs = (spng.StreamDesc * n)(*[spng.StreamDesc(s._ptr(i[0]), int(i[1]), s._ptr(i[2]), i[2].numel(), i[3], 0) for i in items])
    st = (ctypes.c_uint64 * (4 * n))(*[int(v) for i in items for v in i[4]])
    res = (spng.Result * n)()
    assert s.lib.spng_inflate_resume_batch(s.ctx, descs, st, n, None, res) == 0
    out = []
    for k, r in enumerate(res):
        tok = int(r.consumed)
        nxt = (int(r.aux[0]), int(r.aux[1]), tok, int(r.written) if tok else 0) if r.status == 1 else tuple(items[k][4])
        out.append((r, nxt))
    return out


def test_a_mixed_batch_in_one_call(gpu):
    """a stream inside a huge block with a large push, one inside a huge block with a small push, a zlib-6 stream in the middle of its
    pushes and one with a zero state: all exact, and the cuts tried are those of the first alone"""
    s = gpu.load()
    seg = 65536
    streams = []                                    # (data, stream, bytes of the first push, bytes after the second)
    streams.append(ob.one_dynamic_block(9, 24 << 20) + (65536, 65536 + (2 << 20)))      # (the stream is ~4 MiB long)
    streams.append(ob.one_fixed_block(13, 8 << 20) + (2 << 20, (2 << 20) + 65536))
    d = scanlines(41, 3 << 20)
    streams.append((d, zlib.compress(d, 6), 300000, 700000))
    d = scanlines(42, 200 * 4096)
    streams.append((d, zlib.compress(d, 6), 0, None))
    knobs(s, None, seg)
    try:
        items = []
        for data, z, n0, n1 in streams:
            n1 = len(z) if n1 is None else n1
            assert n0 < n1 <= len(z), "a push may not name more input than the buffer holds"
            d_in, d_out = s.to_device(z[:n1]), s.empty(len(data) + 64)
            state = (0, 0, 0, 0)
            if n0:
                r, state = s.inflate_resume(d_in, n0, d_out, spng.FORMAT_ZLIB, state)
                assert r.status == 1
            items.append((d_in, n1, d_out, spng.FORMAT_ZLIB, state))
        assert items[0][4][2] != 0 and items[1][4][2] - items[1][4][0] > 8 << 20, "both stand inside their block, the second deep inside"
        (alone, _), = resume_batch(s, items[:1])
        tried_alone, joined_alone, redone_alone = s.cut_stats()
        got = resume_batch(s, items)
        tried, joined, redone = s.cut_stats()
    finally:
        knobs(s)
    print(f"alone: tried {tried_alone} joined {joined_alone}; in the batch: tried {tried} joined {joined} redone {redone}")
    for k, ((data, z, n0, n1), (r, nxt)) in enumerate(zip(streams, got)):
        n1 = len(z) if n1 is None else n1
        st, out, consumed, aux = oracle(z[:n1], spng.FORMAT_ZLIB, len(data) + 64)
        assert (r.status, r.written) == (st, len(out)), k
        assert bytes(items[k][2][:r.written].cpu().numpy()) == out, k
        if st == 0:
            assert r.consumed == consumed
    assert (alone.status, alone.written, alone.consumed) == (got[0][0].status, got[0][0].written, got[0][0].consumed)
    assert tried_alone >= 1 and joined_alone >= 1 and redone_alone == 0
    assert (tried, joined, redone) == (tried_alone, joined_alone, 0)


@pytest.mark.parametrize("fmt", ["ios", "gzip"])
def test_formats(gpu, blocks, fmt):
    """the fixed block of case 1 as raw DEFLATE and as a gzip member: the states are bits of the DEFLATE payload"""
    s = gpu.load()
    data, z = blocks["fixed"]
    raw = z[2:-4]
    if fmt == "ios":
        f, stream = spng.FORMAT_IOS, raw
    else:
        f, stream = spng.FORMAT_GZIP, gw.HEADER + raw + (zlib.crc32(data) & 0xffffffff).to_bytes(4, "little") + (len(data) & 0xffffffff).to_bytes(4, "little")
    parts = split(stream, 65536, 4)
    p, rows = run_pushes(s, parts, len(data) + 64, fmt=f)
    print(f"{fmt}: states {[r[1] for r in rows]}, cuts {[r[2] for r in rows]}")
    check_against_oracle(p, rows, parts, f, len(data) + 64, data)
    assert rows[-1][0][2] == len(stream)
    for k in range(1, len(parts) - 1):
        assert rows[k][2][0] >= 1 and rows[k][2][1] >= 1 and rows[k][2][2] == 0, (k, rows[k][2])
        assert rows[k][1][2] < 8 * len(raw), "a bit of the payload, not of the member"


def test_through_the_mirror(gpu):
    """PNG.Context.push: a 2048 x 2048 RGBA8 image whose filtered rows are one block of literals, as 64 KiB and then the rest"""
    import torch
    from swift_png_amd import synth
    s = gpu.load()
    W = H = 2048
    img = synth.image(5, W, H)
    U = spng.inflated_size(W, H, 8, 4, False)
    d_sto, d_rows = s.to_device(img.tobytes()), s.empty(U)
    torch.cuda.synchronize()
    assert s.filter_batch([s.image_desc(None, d_rows, d_sto, W, H, 8, 4, False)])[0].status == 0
    rows = bytes(d_rows.cpu().numpy())
    z = ob.literal_block(rows)
    assert zlib.decompress(z) == rows
    ctx = gpu.PNG.Context((W, H), 8, 4, False, spng.FORMAT_ZLIB, session=s)
    ctx.push(z[:65536])
    t0 = time.perf_counter()
    ctx.push(z[65536:])
    dt = time.perf_counter() - t0
    tried, joined, redone = s.cut_stats()
    ctx.push_ancillary_iend()
    print(f"mirror: {len(z)} bytes in one block, second push {dt * 1e3:.1f} ms; cuts tried {tried} joined {joined} redone {redone}")
    assert ctx.storage == img.tobytes()
    assert ctx.defiltered_total == U
    assert tried >= 1 and joined >= 1 and redone == 0
