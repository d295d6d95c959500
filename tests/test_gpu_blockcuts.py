"""Block cuts of the parallel inflate pipeline on the GPU (csrc/pinflate2.hip, SPNG_CFG_BLOCK_CUT_BYTES, spng_cut_stats): a stream
that is ONE huge block -- or a run of blocks without a findable header -- is cut into segments that decode side by side and are
joined to the chain afterwards.  Always the same bytes and the same verdict as without cuts, and as zlib; no clock is asserted on
(times are printed)."""
import hashlib
import time
import zlib

import numpy as np
import pytest

import oneblock as ob
import swift_png_amd as spng

pytestmark = pytest.mark.gpu


def scanlines(seed, n):
    """filtered-PNG-like bytes: small deltas, runs, the occasional noisy row"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, n).astype(np.int16)
    a[rng.random(n) < 0.6] = 0
    rows = a.astype(np.uint8).reshape(-1, 4096)
    rows[::37] = rng.integers(0, 256, (len(rows[::37]), 4096), dtype=np.uint8)
    rows[::4, 0] = 1
    return rows.tobytes()


def make(kind, n):
    """the kinds of stream of tests/test_gpu_pinflate.py"""
    rng = np.random.default_rng(99)
    if kind.startswith("zlib"):
        return zlib.compress(scanlines(1, n), int(kind[4:]))
    if kind == "noise":
        return zlib.compress(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 6)
    if kind == "huffonly":
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
        return co.compress(rng.integers(0, 256, n, dtype=np.uint8).tobytes()) + co.flush()
    if kind == "text16":
        return zlib.compress(rng.integers(0, 16, n, dtype=np.uint8).tobytes(), 6)
    if kind == "zeros":
        return zlib.compress(bytes(n), 6)
    if kind == "period4":
        return zlib.compress(bytes([1, 2, 3, 255]) * (n // 4), 6)
    if kind == "fixed":
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
        return co.compress(scanlines(2, n)) + co.flush()
    if kind == "flushes":
        co = zlib.compressobj(6)
        d = scanlines(3, n)
        out = b""
        for i in range(0, n, 50000):
            out += co.compress(d[i:i + 50000]) + co.flush(zlib.Z_FULL_FLUSH if (i // 50000) % 3 else zlib.Z_SYNC_FLUSH)
        return out + co.flush()
    if kind == "stored_mix":
        d = scanlines(4, n)
        co = zlib.compressobj(0)
        head = co.compress(d[:n // 3]) + co.flush(zlib.Z_FULL_FLUSH)
        c6 = zlib.compressobj(6, zlib.DEFLATED, -15)
        tail = c6.compress(d[n // 3:]) + c6.flush()
        return head + tail + zlib.adler32(d).to_bytes(4, "big")
    raise KeyError(kind)


KINDS = ["zlib1", "zlib6", "zlib9", "noise", "huffonly", "text16", "zeros", "period4", "fixed", "flushes", "stored_mix"]


@pytest.fixture(scope="module")
def huge():
    """the two one-block streams: 32 MiB of literals in one fixed block, ~64 MiB of output in one dynamic block"""
    return {"fixed": ob.one_fixed_block(11, 32 << 20), "dynamic": ob.one_dynamic_block(7, 68 << 20)}


def inflate_one(s, z, cap, cut=None, segment=None):
    """one single-stream call under the given knobs -> (Result, output bytes, cut_stats, seconds)"""
    d_z = s.to_device(z)
    if cut is not None:
        s.configure(spng.CFG_BLOCK_CUT_BYTES, cut)
    if segment is not None:
        s.configure(spng.CFG_SEGMENT_BYTES, segment)
    try:
        s.sync()
        t0 = time.perf_counter()
        outs, res = s.inflate_batch([d_z], [cap])
        s.sync()
        dt = time.perf_counter() - t0
        stats = s.cut_stats()
    finally:
        s.configure(spng.CFG_BLOCK_CUT_BYTES, 0)
        s.configure(spng.CFG_SEGMENT_BYTES, 0)
    return res[0], bytes(outs[0][:res[0].written].cpu().numpy()), stats, dt


@pytest.mark.parametrize("which", ["fixed", "dynamic"])
def test_one_huge_block_is_cut_and_joined(gpu, huge, which):
    s = gpu.load()
    data, z = huge[which]
    res, out, (tried, joined, redone), dt = inflate_one(s, z, len(data) + 64)
    print(f"{which}: {len(z)} -> {len(data)} bytes in {dt * 1e3:.1f} ms; cuts tried {tried} joined {joined} redone {redone}")
    assert res.status == 0 and res.written == len(data) and res.consumed == len(z)
    assert hashlib.sha256(out).digest() == hashlib.sha256(data).digest()
    assert res.reserved == 1, "fell back to the serial kernel"
    assert tried >= 1 and joined >= 1


@pytest.mark.parametrize("which", ["fixed", "dynamic"])
def test_the_knob_changes_no_result(gpu, huge, which):
    s = gpu.load()
    data, z = huge[which]
    r0, out0, st0, t0 = inflate_one(s, z, len(data) + 64, cut=spng.BLOCK_CUT_NEVER)
    r1, out1, st1, t1 = inflate_one(s, z, len(data) + 64, cut=0)
    print(f"{which}: never {t0 * 1e3:.1f} ms, automatic {t1 * 1e3:.1f} ms; cuts {st1}")
    assert st0[0] == 0 and st0 == (0, 0, 0)
    assert (r0.status, r0.written, r0.consumed, r0.reserved, tuple(r0.aux)) == (r1.status, r1.written, r1.consumed, r1.reserved, tuple(r1.aux))
    assert out0 == out1 == data


@pytest.mark.parametrize("kind", KINDS)
def test_aggressive_cuts_on_ordinary_streams(gpu, kind):
    """a 64 KiB threshold and 16 KiB segments: cuts wherever four segments in a row have no block start"""
    s = gpu.load()
    z = make(kind, 3 << 20)
    want = zlib.decompress(z)
    res, out, (tried, joined, redone), _ = inflate_one(s, z, len(want) + 64, cut=65536, segment=16384)
    print(f"{kind}: cuts tried {tried} joined {joined} redone {redone}")
    assert res.status == 0 and res.written == len(want) and res.consumed == len(z)
    assert out == want
    assert res.reserved == 1, f"{kind}: fell back to the serial kernel"
    assert redone in (0, 1)


def damaged(z, how):
    if how == "truncated":
        return z[:len(z) * 2 // 3]
    b = bytearray(z)
    b[len(b) // 2] ^= 0x10
    return bytes(b)


@pytest.mark.parametrize("case", ["other tables", "truncated", "flipped"])
def test_streams_that_do_not_stitch_end_as_without_cuts(gpu, case):
    s = gpu.load()
    if case == "other tables":
        data, z = ob.dynamic_then_fixed(3, 1 << 20, 6 << 20)       # a dynamic block, then 6 MiB in a fixed block no search finds
    else:
        data, z = ob.one_dynamic_block(5, 24 << 20)
        z = damaged(z, case)
    r0, out0, st0, _ = inflate_one(s, z, len(data) + 64, cut=spng.BLOCK_CUT_NEVER)
    r1, out1, (tried, joined, redone), _ = inflate_one(s, z, len(data) + 64, cut=0)
    print(f"{case}: status {r1.status} written {r1.written}; cuts tried {tried} joined {joined} redone {redone}")
    assert st0 == (0, 0, 0) and tried >= 1
    assert (r1.status, r1.written, r1.consumed, r1.reserved, tuple(r1.aux)) == (r0.status, r0.written, r0.consumed, r0.reserved, tuple(r0.aux))
    assert out1 == out0 and data.startswith(out0[:min(len(out0), 1 << 16)])
    if case == "other tables":
        assert r1.status == 0 and out1 == data and redone >= 1
        assert r1.reserved == 1, "a stream whose cuts do not stitch is the pipeline's once more, not the serial kernel's"
    if case == "truncated":
        assert r1.status != 0


def test_one_block_stream_among_ordinary_ones(gpu):
    """31 zlib streams and one one-block stream in one call: all exact, and the cuts tried are those of the one-block stream alone --
    with the segment length pinned, as many as a call over that stream by itself tries, and never more than it has segments"""
    s = gpu.load()
    seg = 65536
    data, z = ob.one_dynamic_block(9, 24 << 20)
    alone, _, (tried_alone, joined_alone, _), _ = inflate_one(s, z, len(data) + 64, segment=seg)
    datas = [scanlines(20 + i, 4096 * (100 + 7 * i)) for i in range(31)]
    zs = [zlib.compress(d, 1 + i % 9) for i, d in enumerate(datas)]
    datas.insert(13, data)
    zs.insert(13, z)
    s.configure(spng.CFG_SEGMENT_BYTES, seg)
    try:
        outs, res = s.inflate_batch([s.to_device(x) for x in zs], [len(d) + 64 for d in datas])
        tried, joined, redone = s.cut_stats()
    finally:
        s.configure(spng.CFG_SEGMENT_BYTES, 0)
    print(f"alone: tried {tried_alone} joined {joined_alone}; in the batch: tried {tried} joined {joined} redone {redone}")
    for i, d in enumerate(datas):
        assert res[i].status == 0 and res[i].written == len(d) and res[i].reserved == 1, i
        assert bytes(outs[i][:len(d)].cpu().numpy()) == d, i
    assert alone.status == 0 and tried_alone >= 1
    assert tried == tried_alone and tried <= (len(z) + seg - 1) // seg - 1
    assert 1 <= joined <= tried and joined == joined_alone and redone == 0


def test_fpnge_shaped_image(gpu):
    """a 4096 x 4096 RGBA8 raster whose filtered scanlines are ONE dynamic block, as an fpnge-style encoder writes them"""
    import torch
    from swift_png_amd import synth
    s = gpu.load()
    W = H = 4096
    img = synth.image(3, W, H)
    S, U = spng.storage_size(W, H, 8, 4), spng.inflated_size(W, H, 8, 4, False)
    d_sto = s.to_device(img.tobytes())
    d_rows = s.empty(U)
    torch.cuda.synchronize()
    fr = s.filter_batch([s.image_desc(None, d_rows, d_sto, W, H, 8, 4, False)])
    assert fr[0].status == 0
    rows = bytes(d_rows.cpu().numpy())
    z = ob.literal_block(rows)
    assert zlib.decompress(z) == rows
    d_z = s.to_device(z)
    d_back = s.empty(S)
    d_rows2 = s.empty(U + 64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = s.decode_batch([s.image_desc(d_z, d_rows2, d_back, W, H, 8, 4, False)])
    dt = time.perf_counter() - t0
    tried, joined, redone = s.cut_stats()
    print(f"fpnge-shaped 4K image: {len(z)} bytes in one block, decode_batch {dt * 1e3:.1f} ms; cuts tried {tried} joined {joined} redone {redone}")
    assert res[0].status == 0
    assert torch.equal(d_back, d_sto)
    assert tried >= 1 and joined >= 1


def test_headline_streams_are_never_cut(gpu):
    """the structural guarantee: in zlib-made and device-made level-6 streams no run of segments without a block start reaches the
    automatic threshold, so no cut is tried: every segment is decoded by the code it was decoded by before (a stream of 1 MiB and
    more is long enough to hold such a run, so its batch does take the plan kernel and the launches that look for cut segments)"""
    s = gpu.load()
    data = scanlines(31, 64 << 20)
    for name, z in (("zlib 6", zlib.compress(data, 6)), ("device 6", s.deflate(data, 6))):
        res, out, stats, dt = inflate_one(s, z, len(data) + 64)
        print(f"{name}: {len(z)} -> {len(data)} bytes in {dt * 1e3:.1f} ms; cuts {stats}")
        assert res.status == 0 and res.reserved == 1 and out == data
        assert stats == (0, 0, 0)
