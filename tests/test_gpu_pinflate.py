"""The intra-stream parallel inflate pipeline (csrc/pinflate2.hip) on the kinds of stream it must take itself:
output bit-exact AND produced by the pipeline (spng_result.reserved == 1), not by the serial kernel it falls
back to -- a silent fallback would keep every parity test green and lose the speed."""
import zlib

import numpy as np
import pytest

import pnghelp as ph
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
    rng = np.random.default_rng(99)
    if kind.startswith("zlib"):
        return zlib.compress(scanlines(1, n), int(kind[4:]))
    if kind == "noise":                       # incompressible: zlib stores it
        return zlib.compress(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 6)
    if kind == "huffonly":                    # the same bytes Huffman-coded without matches: ~8-bit codes everywhere
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
        return co.compress(rng.integers(0, 256, n, dtype=np.uint8).tobytes()) + co.flush()
    if kind == "text16":                      # 16 symbols, 4-bit codes
        return zlib.compress(rng.integers(0, 16, n, dtype=np.uint8).tobytes(), 6)
    if kind == "zeros":                       # maximal runs, distance 1
        return zlib.compress(bytes(n), 6)
    if kind == "period4":                     # runs longer than their distance (RGBA of one colour)
        return zlib.compress(bytes([1, 2, 3, 255]) * (n // 4), 6)
    if kind == "fixed":
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
        return co.compress(scanlines(2, n)) + co.flush()
    if kind == "flushes":                     # many short blocks, empty stored blocks between them
        co = zlib.compressobj(6)
        d = scanlines(3, n)
        out = b""
        for i in range(0, n, 50000):
            out += co.compress(d[i:i + 50000]) + co.flush(zlib.Z_FULL_FLUSH if (i // 50000) % 3 else zlib.Z_SYNC_FLUSH)
        return out + co.flush()
    if kind == "stored_mix":                  # stored blocks between Huffman blocks
        d = scanlines(4, n)
        co = zlib.compressobj(0)
        head = co.compress(d[:n // 3]) + co.flush(zlib.Z_FULL_FLUSH)      # zlib header + stored blocks
        c6 = zlib.compressobj(6, zlib.DEFLATED, -15)
        tail = c6.compress(d[n // 3:]) + c6.flush()
        return head + tail + zlib.adler32(d).to_bytes(4, "big")
    raise KeyError(kind)


KINDS = ["zlib1", "zlib6", "zlib9", "noise", "huffonly", "text16", "zeros", "period4", "fixed", "flushes", "stored_mix"]


@pytest.mark.parametrize("segment", [0, 16384])
@pytest.mark.parametrize("kind", KINDS)
def test_pipeline_takes_regular_streams(gpu, kind, segment):
    s = gpu.load()
    n = 3 << 20
    z = make(kind, n)
    want = zlib.decompress(z)
    s.configure(spng.CFG_SEGMENT_BYTES, segment)          # 0: the default (>= 256 KiB); 16 KiB: ~100 segments
    try:
        outs, res = s.inflate_batch([s.to_device(z)], [len(want) + 64])
    finally:
        s.configure(spng.CFG_SEGMENT_BYTES, 0)
    assert res[0].status == 0 and res[0].written == len(want) and res[0].consumed == len(z)
    assert bytes(outs[0][:len(want)].cpu().numpy()) == want
    assert res[0].reserved == 1, f"{kind}: fell back to the serial kernel"


def test_pipeline_takes_swiftpng_made_streams(gpu):
    """swift-png's own level-6 output: 2047-token blocks (LZ77.DeflatorBuffers.Stream.swift), one chunk of
    subsequences per block."""
    s = gpu.load()
    d = scanlines(5, 2 << 20)
    z = s.deflate(d, 6)
    outs, res = s.inflate_batch([s.to_device(z)], [len(d) + 64])
    assert res[0].status == 0 and res[0].reserved == 1
    assert bytes(outs[0][:len(d)].cpu().numpy()) == d


def test_token_stats_of_the_last_call(gpu):
    """spng_token_stats: the 64 KiB token pages the last parallel-inflate call took cover its tokens (a literal is one halfword,
    a back-reference two: at least the bytes of a stream of literals), and its blocks were counted."""
    s = gpu.load()
    d = np.random.default_rng(9).integers(0, 256, 3 << 20, dtype=np.uint8).tobytes()     # nothing to match: ~3 Mi literals
    z = zlib.compress(d, 6)
    outs, res = s.inflate_batch([s.to_device(z)], [len(d) + 64])
    assert res[0].status == 0 and res[0].reserved == 1
    page_bytes, blocks, dry = s.token_stats()
    assert not dry and blocks >= 1
    assert 2 * len(d) <= page_bytes <= 2 * len(d) + 65536 * (len(z) // 16384 + 64)      # (a page per segment may stay partly empty)
    assert page_bytes % 65536 == 0


def test_pipeline_batch_of_ragged_streams(gpu):
    """one call, streams from 0 bytes to MiBs, valid and not: the pipeline's verdicts never differ from zlib's"""
    s = gpu.load()
    rng = np.random.default_rng(5)
    datas = [scanlines(10 + i, int(4096 * rng.integers(1, 400))) for i in range(24)] + [b"", b"a"]
    zs = [zlib.compress(d, int(rng.integers(1, 10))) for d in datas]
    zs[3] = zs[3][:len(zs[3]) // 2]                       # truncated
    bad = bytearray(zs[5]); bad[len(bad) // 2] ^= 0x10; zs[5] = bytes(bad)    # corrupted
    outs, res = s.inflate_batch([s.to_device(z) for z in zs], [len(d) + 16 for d in datas])
    for i, (d, z) in enumerate(zip(datas, zs)):
        if i in (3, 5):
            continue
        assert res[i].status == 0 and bytes(outs[i][:len(d)].cpu().numpy()) == d, i
    assert res[3].status != 0
    try:
        ok5 = zlib.decompress(zs[5]) == datas[5]
    except zlib.error:
        ok5 = False
    assert (res[5].status == 0) == ok5


@pytest.mark.parametrize("pool", [0, 1 << 20])
def test_mixed_batch_in_repeated_calls_with_dry_pool_retry(gpu, pool):
    """A mixed batch of small segments, three calls on one context.  Same verdicts and bytes as the oracle for every stream
    -- valid, truncated, corrupted, wrong Adler-32, empty, one byte -- with the automatic pool, and also when the pool is far
    too small and the streams that found it empty take the retry pass; and again in the next calls (the page counters, the
    events and what the last batch taught are the context's)."""
    s = gpu.load()
    rng = np.random.default_rng(6)
    datas = [scanlines(40 + i, int(4096 * rng.integers(1, 300))) for i in range(21)] + [b"", b"a", bytes(300000)]
    zs = [zlib.compress(d, int(rng.integers(1, 10))) for d in datas]
    zs[2] = zs[2][:len(zs[2]) * 2 // 3]
    bad = bytearray(zs[17]); bad[-1] ^= 0x01; zs[17] = bytes(bad)          # Adler-32
    bad = bytearray(zs[9]); bad[len(bad) // 3] ^= 0x42; zs[9] = bytes(bad)
    d_in = [s.to_device(z) for z in zs]
    caps = [len(d) + 16 for d in datas]
    s.configure(spng.CFG_SEGMENT_BYTES, 8192)
    s.configure(spng.CFG_TOKEN_BYTES, pool)
    try:
        for _ in range(3):
            outs, res = s.inflate_batch(d_in, caps)
            for i, z in enumerate(zs):
                st, out, used, aux = ph.orc_inflate(z, 0, cap=caps[i])
                assert (res[i].status, res[i].written) == (st, len(out)), (i, res[i].status, st)
                assert bytes(outs[i][:len(out)].cpu().numpy()) == out, i
                if st == 0:
                    assert res[i].consumed == used
                elif st != spng.NEED_MORE_INPUT:
                    assert tuple(res[i].aux) == tuple(aux), i
            if pool == 0:
                assert sum(r.reserved == 1 for r in res) >= 20       # (the pipeline's own work, not the serial kernel's)
    finally:
        s.configure(spng.CFG_SEGMENT_BYTES, 0)
        s.configure(spng.CFG_TOKEN_BYTES, 0)


def test_reserved_configure_keys_are_refused(gpu):
    """Keys 4 and 6 of spng_configure named modes that have been removed: both are refused with SPNG_E_ARGUMENT whatever the
    value, and the refusals leave the context as it was -- the next inflate_batch on it matches the oracle."""
    s = gpu.load()
    for key in (4, 6):
        for value in (0, 1):
            with pytest.raises(spng.SpngError) as err:
                s.configure(key, value)
            assert err.value.status == spng.E_ARGUMENT, (key, value)
    datas = [scanlines(90 + i, 4096 * (40 + 30 * i)) for i in range(4)] + [b""]
    zs = [zlib.compress(d, 6) for d in datas]
    zs[1] = zs[1][:len(zs[1]) // 2]
    caps = [len(d) + 16 for d in datas]
    outs, res = s.inflate_batch([s.to_device(z) for z in zs], caps)
    for i, z in enumerate(zs):
        st, out, used, aux = ph.orc_inflate(z, 0, cap=caps[i])
        assert (res[i].status, res[i].written) == (st, len(out)), (i, res[i].status, st)
        assert bytes(outs[i][:len(out)].cpu().numpy()) == out, i
        if st == 0:
            assert res[i].consumed == used


def test_retry_pass_takes_the_streams_a_dry_pool_left(gpu):
    """A token pool far too small for the batch (SPNG_CFG_TOKEN_BYTES): the streams whose segments found it empty take the
    retry pass -- the pool to themselves -- and come out of the PIPELINE (reserved == 1), not of the serial kernel.
    ADVICE r3: PSEG_NOPAGE had become unreachable, so the retry launches never did anything."""
    s = gpu.load()
    datas = [scanlines(70 + i, 4096 * 160) for i in range(12)]
    zs = [zlib.compress(d, 6) for d in datas]
    d_in = [s.to_device(z) for z in zs]
    caps = [len(d) + 16 for d in datas]
    # two groups' worth of estimate, but sized by the default 3.2 bytes per byte while these streams need less: force dryness
    # with a pool that holds a few streams' tokens only
    s.configure(spng.CFG_TOKEN_BYTES, 3 << 20)
    s.configure(spng.CFG_SEGMENT_BYTES, 16384)
    try:
        outs, res = s.inflate_batch(d_in, caps)
        for i, d in enumerate(datas):
            assert res[i].status == 0 and res[i].written == len(d), (i, res[i].status)
            assert bytes(outs[i][:len(d)].cpu().numpy()) == d, i
        assert all(r.reserved == 1 for r in res), [r.reserved for r in res]
    finally:
        s.configure(spng.CFG_TOKEN_BYTES, 0)
        s.configure(spng.CFG_SEGMENT_BYTES, 0)


@pytest.mark.parametrize("parts", [0, 1, 7, 64])
def test_streams_resolved_by_several_workgroups(gpu, parts):
    """SPNG_CFG_RESOLVE_PARTS (batches of <= 384 streams): a stream's chain cut into parts that resolve side by side -- symbols with
    markers for what lies in front of a part, windows handed from part to part, symbols -> bytes, one verdict.  Whatever the
    number of parts (0: automatic, 1: one workgroup as in large batches), every stream -- long zero runs and 4-byte periods
    that reach across parts, stored data, flushes, a truncated one, a wrong Adler-32, empty input -- gives the oracle's status,
    byte count, bytes and error payload."""
    s = gpu.load()
    rng = np.random.default_rng(7)
    co = zlib.compressobj(6)
    flat = bytes(3 << 20)
    zeros = b"".join(co.compress(flat[i:i + 50000]) + co.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(flat), 50000)) + co.flush()
    co = zlib.compressobj(6)
    per = bytes([7, 0, 255, 3]) * (1 << 19)
    period = b"".join(co.compress(per[i:i + 70000]) + co.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(per), 70000)) + co.flush()
    datas = [scanlines(60 + i, int(4096 * rng.integers(200, 900))) for i in range(5)]
    zs = [zlib.compress(d, int(rng.integers(1, 10))) for d in datas] + [zeros, period, make("stored_mix", 2 << 20), make("flushes", 3 << 20), b""]
    wants = datas + [flat, per, zlib.decompress(zs[7]), zlib.decompress(zs[8]), b""]
    zs[1] = zs[1][:len(zs[1]) * 3 // 5]                                         # truncated inside a block
    bad = bytearray(zs[3]); bad[-3] ^= 0x08; zs[3] = bytes(bad)                 # Adler-32
    d_in = [s.to_device(z) for z in zs]
    caps = [len(w) + 32 for w in wants]
    s.configure(spng.CFG_RESOLVE_PARTS, parts)
    try:
        for _ in range(2):
            outs, res = s.inflate_batch(d_in, caps)
            for i, z in enumerate(zs):
                st, out, used, aux = ph.orc_inflate(z, 0, cap=caps[i])
                assert (res[i].status, res[i].written) == (st, len(out)), (i, res[i].status, st, res[i].written, len(out))
                assert bytes(outs[i][:len(out)].cpu().numpy()) == out, i
                if st == 0:
                    assert res[i].consumed == used
                elif st != spng.NEED_MORE_INPUT:
                    assert tuple(res[i].aux) == tuple(aux), i
            assert sum(r.reserved == 1 for r in res) >= 8                          # (the pipeline's own results)
    finally:
        s.configure(spng.CFG_RESOLVE_PARTS, 0)


@pytest.mark.parametrize("fmt", ["ios", "gzip"])
def test_pipeline_agrees_with_the_serial_kernel_where_nothing_else_checks(gpu, fmt):
    """raw DEFLATE (the iOS variant) has no checksum and a gzip member's CRC-32 is compared after the fact, so for
    those the pipeline's SPNG_DONE is final.  Differential run: random valid streams of every kind, and the same streams with
    a flipped bit, through the pipeline and through the serial kernel alone (SPNG_INFLATE_SERIAL): same status, counts, bytes."""
    import gzip as gz
    s = gpu.load()
    rng = np.random.default_rng(21)
    raws, zs = [], []
    for i, kind in enumerate(KINDS):
        z = make(kind, int(4096 * rng.integers(100, 500)))
        raw = zlib.decompress(z)
        if fmt == "ios":
            co = zlib.compressobj(int(rng.integers(1, 10)), zlib.DEFLATED, -15)
            z2 = co.compress(raw) + co.flush() if kind not in ("stored_mix", "flushes", "fixed", "huffonly") else z[2:-4]
        else:
            z2 = gz.compress(raw, int(rng.integers(1, 10)))
        zs.append(z2); raws.append(raw)
        dam = bytearray(z2); dam[len(dam) * 2 // 3] ^= 1 << int(rng.integers(0, 8))
        zs.append(bytes(dam)); raws.append(raw)
    f = spng.FORMAT_IOS if fmt == "ios" else spng.FORMAT_GZIP
    d_in = [s.to_device(z) for z in zs]
    caps = [len(r) + 4096 for r in raws]
    got = {}
    for mode in (spng.INFLATE_AUTO, spng.INFLATE_SERIAL):
        s.configure(spng.CFG_INFLATE_MODE, mode)
        try:
            outs, res = s.inflate_batch(d_in, caps, fmt=f)
        finally:
            s.configure(spng.CFG_INFLATE_MODE, spng.INFLATE_AUTO)
        got[mode] = [(r.status, r.written, r.consumed if r.status == 0 else 0, tuple(r.aux) if r.status not in (0, 1) else (),
                      bytes(o[:r.written].cpu().numpy())) for o, r in zip(outs, res)]
        if mode == spng.INFLATE_AUTO:
            assert sum(r.reserved == 1 for r in res) >= len(KINDS) - 1          # (the valid ones are the pipeline's)
    for i, (a, b) in enumerate(zip(got[spng.INFLATE_AUTO], got[spng.INFLATE_SERIAL])):
        assert a[:4] == b[:4], (i, a[:4], b[:4])
        assert a[4] == b[4], i
        if i % 2 == 0:
            assert a[0] == 0 and a[4] == raws[i]


def test_damaged_streams_cost_one_block_not_the_batch(gpu):
    """VERDICT r2 "bound the fallback cost": a batch with one stream whose Adler-32 trailer is wrong and one that is cut off
    in the middle of a block.  Statuses, byte counts and payloads are the oracle's (LZ77.InflatorBuffers.swift:112-130); the
    pipeline reports the checksum itself and keeps everything in front of the block the truncated stream ends in, so the
    serial kernel decodes one block instead of two whole 64 MiB streams: the damaged batch takes <= 1.15 x the clean one."""
    import time
    import torch
    from swift_png_amd import synth
    s = gpu.load()
    w = h = 4096
    n = 64
    uniq = []
    for seed in range(2):
        rows = s.filter(synth.image(seed, w, h).tobytes(), w, h, 8, 4, False)
        uniq.append((rows, zlib.compress(rows, 6)))
    U = len(uniq[0][0])
    good = [s.to_device(z) for _, z in uniq]
    bad_adler = bytearray(uniq[0][1]); bad_adler[-2] ^= 0x40
    cut = uniq[1][1][:len(uniq[1][1]) * 5 // 8]
    d_bad, d_cut = s.to_device(bytes(bad_adler)), s.to_device(cut)
    outs = [s.empty(U + 64) for _ in range(n)]

    def run(streams):
        descs = (spng.StreamDesc * n)()
        for i, z in enumerate(streams):
            descs[i] = spng.StreamDesc(z.data_ptr(), z.numel(), outs[i].data_ptr(), U + 64, 0, 0)
        res = (spng.Result * n)()
        assert s.lib.spng_inflate_batch(s.ctx, descs, n, None, res) == 0              # warm-up (pool sizing)
        torch.cuda.synchronize()
        best = 1e9
        s.profile(True)
        for _ in range(3):
            t0 = time.perf_counter()
            assert s.lib.spng_inflate_batch(s.ctx, descs, n, None, res) == 0
            best = min(best, time.perf_counter() - t0)
        print({k: round(s.profile_get(getattr(spng, "K_" + k))[0] / 3, 2) for k in ("PINF_FIND", "PINF_DECODE", "PINF_RESOLVE", "INFLATE")})
        s.profile(False)
        return best, list(res)

    clean = [good[i % 2] for i in range(n)]
    t_clean, res = run(clean)
    assert all(r.status == 0 and r.written == U and r.reserved == 1 for r in res)
    damaged = list(clean)
    damaged[7], damaged[40] = d_bad, d_cut
    t_bad, res = run(damaged)
    # the oracle's verdicts
    st_a, out_a, used_a, aux_a = ph.orc_inflate(bytes(bad_adler), 0, cap=U + 64)
    st_c, out_c, used_c, aux_c = ph.orc_inflate(cut, 0, cap=U + 64)
    assert st_a == spng.E_STREAM_CHECKSUM and st_c == spng.NEED_MORE_INPUT
    assert (res[7].status, res[7].written, tuple(res[7].aux)) == (st_a, len(out_a), tuple(aux_a))
    assert res[7].reserved == 1                                  # (reported by the pipeline itself)
    assert (res[40].status, res[40].written, tuple(res[40].aux)) == (st_c, len(out_c), (0, 0))
    assert bytes(outs[40][:len(out_c)].cpu().numpy()) == out_c
    assert all(r.status == 0 and r.written == U for i, r in enumerate(res) if i not in (7, 40))
    print(f"clean {t_clean * 1e3:.1f} ms, with a bad-checksum and a truncated stream {t_bad * 1e3:.1f} ms")
    assert t_bad <= 1.15 * t_clean + 2e-3, (t_clean, t_bad)
