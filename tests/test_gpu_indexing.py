"""GPU parity of spng_census_batch / spng_pack_indexed_batch (csrc/indexing.hip: the indexer closures of PNG.RGBA.swift:409-423,
PNG.VA.swift:334-350 and PNG.Image.swift:767-782, 935-996 as tables) against the numpy restatement in tests/indexing_ref.py, through
the C ABI; the host layer's pack(indexer=) / unpack(deindexer=); and the reference's indexed-colour tutorial end to end."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

import indexing_ref as ref
import pnghelp as ph

pytestmark = pytest.mark.gpu

RGBA, VA, SCALAR = 0, 1, 2
MASK = {RGBA: 0xFFFFFFFF, VA: 0xFFFF, SCALAR: 0xFF}
SENTINEL32, SENTINEL64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF          # what run_census fills the outputs with
CASES = [(bits, layout) for bits in (8, 16) for layout in (RGBA, VA, SCALAR)]


def dtype_of(bits):
    return "<u1" if bits == 8 else "<u2"


def pixels_of(keys, bits, layout, rng):
    """pixels of T whose keys are `keys`; T = UInt16: random low bytes"""
    keys = np.asarray(keys, dtype=np.uint64)
    c = np.stack([(keys >> (8 * z)) & 255 for z in range((4, 2, 1)[layout])], axis=1)
    if bits == 16:
        c = c << 8 | rng.integers(0, 256, c.shape, dtype=np.uint64)
    return np.ascontiguousarray(c.astype(dtype_of(bits)))


def distinct(n, layout, rng):
    if n > (MASK[layout] + 1) // 2:
        return rng.permutation(MASK[layout] + 1)[:n].astype(np.uint32)
    k = np.unique(rng.integers(0, MASK[layout] + 1, 2 * n + 64, dtype=np.uint64))
    assert len(k) >= n
    return rng.permutation(k)[:n].astype(np.uint32)


def run_census(s, arrays, bits, layout, cap, premultiply=0, counts=True):
    """spng_census_batch over numpy pixel arrays -> list of (status, written, keys[:cap], counts[:cap] or None)"""
    tens = [s.to_device(a.tobytes()) for a in arrays]
    fill = bytes([0xFF]) * (8 * cap)                              # (host to device: complete when to_device returns)
    outs = [(s.to_device(fill[:4 * cap]), s.to_device(fill) if counts else None) for _ in arrays]
    outs, res = s.census_batch(tens, bits, layout, cap, premultiply, counts, outs=outs)
    s.sync()
    out = []
    for (k, c), r in zip(outs, res):
        out.append((r.status, int(r.written), k.cpu().numpy().view(np.uint32), c.cpu().numpy().view(np.uint64) if c is not None else None))
    return out


def check_census(got, px, bits, layout, cap, premultiply=0):
    status, written, keys, counts = got
    wk, wc = ref.census(px, bits, layout, premultiply)
    if len(wk) > cap:
        assert status == 64 and written == 0, (status, written, len(wk), cap)
        return
    assert status == 0 and written == len(wk), (status, written, len(wk))
    assert (keys[:written] == wk).all()
    assert (keys[written:] == SENTINEL32).all()                   # untouched behind `written`
    if counts is not None:
        assert (counts[:written] == wc).all() and int(counts[:written].sum()) == len(np.asarray(px).reshape(-1, (4, 2, 1)[layout]))
        assert (counts[written:] == SENTINEL64).all()


@pytest.mark.parametrize("bits,layout", CASES)
def test_census_sizes_flat_and_structured_keys(gpu, bits, layout):
    """pixel counts around the quad and the workgroup; 2^20 equal pixels; the keys 0 and 0xFFFFFFFF; {k << s}; T = UInt16 pixels that
    differ in their low bytes only; no counts; the same call twice"""
    s = gpu.load()
    rng = np.random.default_rng(bits + layout)
    few = distinct(40, layout, rng)
    arrays = [pixels_of(few[rng.integers(0, 40, n)], bits, layout, rng) for n in (0, 1, 3, 4, 5, 259, 65537)]
    for got, px in zip(run_census(s, arrays, bits, layout, 256), arrays):
        check_census(got, px, bits, layout, 256)
    flat = pixels_of(np.full(1 << 20, 0x80FF8040 & MASK[layout]), bits, layout, rng)
    got = run_census(s, [flat], bits, layout, 1)[0]
    check_census(got, flat, bits, layout, 1)
    assert got[1] == 1 and got[3][0] == 1 << 20
    ends = pixels_of(np.array([0, MASK[layout], 1, MASK[layout] - 1])[rng.integers(0, 4, 5000)], bits, layout, rng)
    structured = [ends, pixels_of(np.full(300, MASK[layout]), bits, layout, rng), pixels_of(np.zeros(300), bits, layout, rng)]
    for sh in range(0, (32, 16, 8)[layout], 8):
        k = np.arange(256, dtype=np.uint64) << sh
        structured.append(pixels_of(np.concatenate([k, k[rng.integers(0, 256, 3000)]]), bits, layout, rng))
    first = run_census(s, structured, bits, layout, 256)
    for got, px in zip(first, structured):
        check_census(got, px, bits, layout, 256)
    again = run_census(s, structured, bits, layout, 256)
    for a, b in zip(first, again):
        assert a[:2] == b[:2] and (a[2] == b[2]).all() and (a[3] == b[3]).all()
    for got, px in zip(run_census(s, structured, bits, layout, 256, counts=False), structured):
        assert got[3] is None
        check_census(got, px, bits, layout, 256)
    if bits == 16:
        one = pixels_of(np.full(256, 0x12345678 & MASK[layout]), bits, layout, rng)
        one[:, 0] = (one[:, 0] & 0xFF00) | np.arange(256)
        got = run_census(s, [one], bits, layout, 1)[0]
        assert got[:2] == (0, 1) and got[3][0] == 256


@pytest.mark.parametrize("bits,layout", CASES)
def test_census_exactly_cap_and_one_more(gpu, bits, layout):
    s = gpu.load()
    rng = np.random.default_rng(10 * bits + layout)
    for cap in (1, 256, 65536):
        for extra in (0, 1):
            if cap + extra > MASK[layout] + 1:
                continue
            keys = distinct(cap + extra, layout, rng)
            px = pixels_of(np.concatenate([keys, keys[rng.integers(0, len(keys), 3000)]]), bits, layout, rng)
            got = run_census(s, [px], bits, layout, cap)[0]
            assert got[0] == (64 if extra else 0)
            check_census(got, px, bits, layout, cap)


@pytest.mark.parametrize("bits,layout", [(b, l) for b, l in CASES if l != SCALAR])
def test_census_many_keys(gpu, bits, layout):
    """2^20 pixels drawn with a skewed distribution from 5000 keys at cap 8192; key counts on both sides of the sort's LDS limit;
    more distinct keys inside one workgroup's share than its LDS table may hold, then the same keys again, in workgroups that make
    several rounds (256 arrays in one call: 16 workgroups each)"""
    s = gpu.load()
    rng = np.random.default_rng(20 * bits + layout)
    keys = distinct(5000, layout, rng)
    skew = pixels_of(keys[(rng.random(1 << 20) ** 3 * 5000).astype(np.int64)], bits, layout, rng)
    check_census(run_census(s, [skew], bits, layout, 8192)[0], skew, bits, layout, 8192)
    arrays = []
    for nk in (gpu.CENSUS_FINISH_LDS_KEYS - 1, gpu.CENSUS_FINISH_LDS_KEYS, gpu.CENSUS_FINISH_LDS_KEYS + 1, 2 * gpu.CENSUS_FINISH_LDS_KEYS + 1):
        k = distinct(nk, layout, rng)
        arrays.append(pixels_of(np.concatenate([k, k[rng.integers(0, nk, 1000)]]), bits, layout, rng))
    for got, px in zip(run_census(s, arrays, bits, layout, 16384), arrays):
        check_census(got, px, bits, layout, 16384)
    nk = 3 * gpu.CENSUS_LDS_LIMIT
    k = distinct(nk, layout, rng)
    px = pixels_of(np.concatenate([k, k, k[rng.integers(0, nk, 40000 - 2 * nk)]]), bits, layout, rng)
    t = s.to_device(px.tobytes())
    outs, res = s.census_batch([t] * 256, bits, layout, 2048)
    s.sync()
    wk, wc = ref.census(px, bits, layout)
    for (dk, dc), r in zip(outs, res):
        assert r.status == 0 and r.written == nk
        assert (dk[:nk].cpu().numpy().view(np.uint32) == wk).all() and (dc[:nk].cpu().numpy().view(np.uint64) == wc).all()


def test_census_batch_equals_each_array_alone(gpu):
    """unequal counts, one of them 0, one overflowing, disjoint key sets"""
    s = gpu.load()
    rng = np.random.default_rng(77)
    sets = [distinct(n, RGBA, rng) for n in (10, 300, 200, 1, 100)]
    sets[1] |= 0x01000000
    sets[2] &= 0x00FFFFFF                                         # (disjoint from the second)
    counts = (70000, 5000, 0, 1, 1023)
    arrays = [pixels_of(k[rng.integers(0, len(k), n)], 16, RGBA, rng) for k, n in zip(sets, counts)]
    together = run_census(s, arrays, 16, RGBA, 256)
    assert [g[0] for g in together] == [0, 64, 0, 0, 0]
    for got, px in zip(together, arrays):
        alone = run_census(s, [px], 16, RGBA, 256)[0]
        check_census(got, px, 16, RGBA, 256)
        assert got[:2] == alone[:2]
        if got[0] == 0:
            assert (got[2] == alone[2]).all() and (got[3] == alone[3]).all()


@pytest.mark.parametrize("bits,layout,op", [(8, RGBA, 1), (16, RGBA, 1), (16, RGBA, 2), (8, VA, 1), (16, VA, 2)])
def test_census_premultiplied_equals_alpha_then_census(gpu, bits, layout, op):
    s = gpu.load()
    rng = np.random.default_rng(bits + op)
    px = rng.integers(0, 1 << bits, (3001, (4, 2)[layout])).astype(dtype_of(bits))
    fused = run_census(s, [px], bits, layout, 8192, premultiply=op)[0]
    check_census(fused, px, bits, layout, 8192, premultiply=op)
    pre = np.frombuffer(s.alpha(px.tobytes(), bits, layout, op)[0], dtype=dtype_of(bits))
    two = run_census(s, [pre], bits, layout, 8192)[0]
    assert fused[:2] == two[:2] and (fused[2] == two[2]).all() and (fused[3] == two[3]).all()


def test_census_refusals(gpu):
    s = gpu.load()
    t = s.to_device(bytes(64))
    for kw in (dict(cap=0), dict(cap=65537), dict(layout=SCALAR, premultiply=1), dict(bits=8, premultiply=2), dict(premultiply=3)):
        args = dict(bits=8, layout=RGBA, cap=256, premultiply=0)
        args.update(kw)
        with pytest.raises(gpu.SpngError) as e:
            s.census_batch([t], args["bits"], args["layout"], args["cap"], args["premultiply"])
        assert e.value.status == gpu.E_ARGUMENT
    with pytest.raises(gpu.SpngError) as e:
        s.census(bytes(range(200)) * 4, 8, RGBA, cap=16)
    assert e.value.status == gpu.E_OUTPUT_CAPACITY
    # raw descs: a valid one of 16 pixels with one field spoiled at a time, alone and behind a valid desc whose poisoned outputs stay
    buf = s.to_device(bytes([0xEE]) * 4096)
    base, E = buf.data_ptr(), gpu.E_ARGUMENT

    def desc(d_pixels=base, count=16, d_keys=base + 1024, d_counts=base + 2048, cap=16, bits=8, layout=RGBA, premultiply=0, reserved=0):
        d = gpu.CensusDesc(d_pixels, count, d_keys, d_counts, cap, bits, layout, premultiply)
        d.reserved[0] = reserved
        return d

    def call(*descs, ctx=s.ctx):
        return s.lib.spng_census_batch(ctx, (gpu.CensusDesc * len(descs))(*descs), len(descs), None, (gpu.Result * max(len(descs), 1))())

    assert call(desc()) == 0 and call(desc(bits=16)) == 0 and call(desc(d_counts=None)) == 0 and call(desc(count=0, d_pixels=None)) == 0
    assert call(desc(bits=12)) == E
    for kw in (dict(d_keys=None), dict(d_keys=base + 1026), dict(d_counts=base + 2052), dict(bits=16, d_pixels=base + 1), dict(d_pixels=None),
               dict(count=1 << 60), dict(reserved=1), dict(bits=16), dict(layout=3)):
        first = desc(d_keys=base + 3072, d_counts=base + 3200, bits=16 if "d_pixels" in kw and kw.get("bits") == 16 else 8)
        assert call(desc(**kw)) == (0 if kw == dict(bits=16) else E), kw
        assert call(first, desc(**kw)) == E, kw
    assert call() == 0 and s.lib.spng_census_batch(s.ctx, None, 0, None, None) == 0 and call(desc(), ctx=None) == E
    assert s.lib.spng_census_batch(s.ctx, (gpu.CensusDesc * 1)(desc()), 1, None, None) == E       # nowhere to put the results
    s.sync()
    assert (buf[3072:].cpu().numpy() == 0xEE).all()


# ---- mapped pack ---------------------------------------------------------------------------------------------------------------
def run_pack(s, arrays, bits, layout, maps, miss=0, premultiply=0, offsets=None):
    """spng_pack_indexed_batch over numpy pixel arrays; maps: per array (keys ascending, indices); offsets: of each storage behind
    a 4-byte boundary.  -> list of (status, written, missed, storage bytes); the bytes around every storage are checked"""
    torch = s.torch
    tens = [s.to_device(a.tobytes()) for a in arrays]
    ns = [len(a.reshape(-1, (4, 2, 1)[layout])) for a in arrays]
    offsets = offsets or [0] * len(arrays)
    bufs = [s.to_device(bytes([0xEE]) * (n + 16)) for n in ns]     # (host to device: complete when to_device returns)
    stor = [b[4 + o:4 + o + n] for b, o, n in zip(bufs, offsets, ns)]
    dk = [torch.from_numpy(np.asarray(k, dtype=np.uint32).view(np.int32).copy()).to(s.tdev) for k, _ in maps]
    di = [torch.from_numpy(np.asarray(i, dtype=np.uint8).copy()).to(s.tdev) for _, i in maps]
    _, res = s.pack_indexed_batch(tens, [(n, 1) for n in ns], bits, layout, dk, di, miss, premultiply, storages=stor)
    s.sync()
    out = []
    for b, o, n, r in zip(bufs, offsets, ns, res):
        raw = b.cpu().numpy()
        assert (raw[:4 + o] == 0xEE).all() and (raw[4 + o + n:] == 0xEE).all()
        out.append((r.status, int(r.written), int(r.aux[0]), raw[4 + o:4 + o + n]))
    return out


def check_pack(got, px, bits, layout, keys, indices, miss=0, premultiply=0):
    want, missed = ref.pack_indexed(px, bits, layout, keys, indices, miss, premultiply)
    assert got[0] == 0 and got[1] == len(want) and got[2] == missed, (got[:3], len(want), missed)
    assert (got[3] == want).all()


def a_map(keys, rng, modulo=256):
    keys = np.unique(np.asarray(keys, dtype=np.uint32))           # ascending and distinct
    return keys, rng.integers(0, modulo, len(keys)).astype(np.uint8)


@pytest.mark.parametrize("bits,layout", CASES)
def test_pack_indexed_sizes_offsets_and_map_sizes(gpu, bits, layout):
    s = gpu.load()
    rng = np.random.default_rng(30 * bits + layout)
    few = distinct(40, layout, rng)
    m = a_map(np.concatenate([few[:20], distinct(20, layout, rng)]), rng)         # half of the pixels' keys, and keys no pixel has
    for off in range(4):
        arrays = [pixels_of(few[rng.integers(0, 40, n)], bits, layout, rng) for n in (0, 1, 3, 4, 5, 259)]
        for got, px in zip(run_pack(s, arrays, bits, layout, [m] * 6, miss=7, offsets=[off] * 6), arrays):
            check_pack(got, px, bits, layout, *m, miss=7)
    lds = gpu.PACK_INDEXED_LDS_KEYS
    for mc in (0, 1, 255, 256, 257, lds - 1, lds, lds + 1, 65536):
        if mc > MASK[layout] + 1:
            continue
        keys = distinct(mc, layout, rng)
        pool = np.concatenate([keys, distinct(50, layout, rng)])
        px = pixels_of(pool[rng.integers(0, len(pool), 5000)], bits, layout, rng)
        m = a_map(keys, rng, 5)                                   # (many-to-one)
        got = run_pack(s, [px], bits, layout, [m], miss=200, offsets=[1])[0]
        check_pack(got, px, bits, layout, *m, miss=200)
        if mc == 0:
            assert got[2] == 5000 and (got[3] == 200).all()
    # the keys 0 and ~0: present, and absent with pixels of those colours; on both sides of the LDS threshold
    for present in (False, True):
        for extra in (10, lds + 10):
            if extra + 2 > MASK[layout]:
                continue
            keys = distinct(extra + 2, layout, rng)
            keys = keys[(keys != 0) & (keys != MASK[layout])][:extra]
            ends = np.array([0, MASK[layout]], dtype=np.uint32)
            pool = np.concatenate([keys, ends])
            px = pixels_of(pool[rng.integers(0, len(pool), 3000)], bits, layout, rng)
            m = a_map(pool if present else keys, rng)
            check_pack(run_pack(s, [px], bits, layout, [m], miss=99)[0], px, bits, layout, *m, miss=99)
    if layout == SCALAR:                                          # the tutorial's indexer, Int.init
        px = pixels_of(rng.integers(0, 256, 4000), bits, layout, rng)
        got = run_pack(s, [px], bits, layout, [(np.arange(256), np.arange(256))])[0]
        assert got[2] == 0 and (got[3] == (px[:, 0] >> (bits - 8))).all()
    if layout == VA:                                              # every key there is
        px = rng.integers(0, 1 << bits, (6000, 2)).astype(dtype_of(bits))
        m = (np.arange(65536), (np.arange(65536) * 7 >> 3).astype(np.uint8))
        check_pack(run_pack(s, [px], bits, layout, [m])[0], px, bits, layout, *m)


@pytest.mark.parametrize("bits,layout,op", [(8, RGBA, 1), (16, RGBA, 1), (16, RGBA, 2), (8, VA, 1), (16, VA, 2)])
def test_pack_indexed_premultiplied(gpu, bits, layout, op):
    s = gpu.load()
    rng = np.random.default_rng(40 * bits + op)
    px = rng.integers(0, 1 << bits, (3001, (4, 2)[layout])).astype(dtype_of(bits))
    m = a_map(np.unique(ref.keys(px, bits, layout, op))[::2], rng)
    check_pack(run_pack(s, [px], bits, layout, [m], miss=3, premultiply=op, offsets=[2])[0], px, bits, layout, *m, miss=3, premultiply=op)


def test_pack_indexed_batch_of_unequal_images_and_the_default_indexer(gpu):
    s = gpu.load()
    rng = np.random.default_rng(5)
    sets = [distinct(n, RGBA, rng) for n in (30, 700, 5)]
    arrays = [pixels_of(k[rng.integers(0, len(k), n)], 8, RGBA, rng) for k, n in zip(sets, (4099, 64, 0))]
    maps = [a_map(k[: len(k) // 2 + 1], rng) for k in sets]
    for got, px, m, miss in zip(run_pack(s, arrays, 8, RGBA, maps, miss=[1, 2, 3]), arrays, maps, (1, 2, 3)):
        check_pack(got, px, 8, RGBA, *m, miss=miss)
    # a map that equals the default indexer of a 256-entry palette: the storage spng_pack_batch gives for that palette
    for bits in (8, 16):
        pal = distinct(256, RGBA, rng)
        pool = np.concatenate([pal, distinct(20, RGBA, rng)])     # (some colours are not in the palette: entry 0)
        px = pixels_of(pool[rng.integers(0, len(pool), 64 * 33)], bits, RGBA, rng)
        order = np.argsort(pal)
        got = run_pack(s, [px], bits, RGBA, [(pal[order], order.astype(np.uint8))], miss=0)[0]
        palette = pal.astype("<u4").tobytes()                     # (r, g, b, a) in memory order = the key
        assert got[3].tobytes() == s.pack(px.tobytes(), 64, 33, 8, 1, indexed=True, source=bits, palette=palette)


def test_pack_indexed_refusals(gpu):
    s = gpu.load()
    with pytest.raises(gpu.SpngError) as e:                       # keys that are not ascending: seen in the host-pointer form
        s.pack_indexed(bytes(16), 4, 1, 8, RGBA, [5, 3], bytes(2))
    assert e.value.status == gpu.E_ARGUMENT
    with pytest.raises(gpu.SpngError) as e:
        s.pack_indexed(bytes(16), 4, 1, 8, RGBA, [5, 5], bytes(2))
    assert e.value.status == gpu.E_ARGUMENT
    sto, missed = s.pack_indexed(bytes(16), 4, 1, 8, RGBA, [0], b"\x09", miss=1)
    assert sto == b"\x09" * 4 and missed == 0
    # raw descs: a valid one of a 4 x 4 image with one field spoiled at a time, alone and behind a valid desc whose poisoned
    # storage stays
    host = np.full(4096, 0xEE, dtype=np.uint8)
    host[1024:1032] = np.array([1, 2], dtype="<u4").view(np.uint8)
    host[1040:1042] = (0, 1)
    buf = s.to_device(host)
    base, E = buf.data_ptr(), gpu.E_ARGUMENT

    def desc(d_pixels=base, d_storage=base + 2048, d_keys=base + 1024, d_indices=base + 1040, size=4, map_count=2, source=8, layout=RGBA,
             premultiply=0, reserved=None):
        d = gpu.PackIndexedDesc(d_pixels, d_storage, d_keys, d_indices, size, size, map_count, source, layout, premultiply, 7)
        if reserved is not None:
            d.reserved[reserved] = 1
        return d

    def call(*descs, ctx=s.ctx):
        res = (gpu.Result * max(len(descs), 1))()
        return s.lib.spng_pack_indexed_batch(ctx, (gpu.PackIndexedDesc * len(descs))(*descs), len(descs), None, res)

    assert call(desc()) == 0 and call(desc(source=16)) == 0 and call(desc(source=16, premultiply=2)) == 0
    assert call(desc(map_count=0, d_keys=None, d_indices=None)) == 0 and call(desc(size=0, d_pixels=None, d_storage=None)) == 0
    assert call(desc(source=12)) == E
    for kw in (dict(source=16), dict(layout=3), dict(premultiply=3), dict(premultiply=2), dict(layout=SCALAR, premultiply=1),
               dict(map_count=65537), dict(d_keys=None), dict(d_indices=None), dict(d_keys=base + 1026), dict(d_pixels=None),
               dict(d_storage=None), dict(source=16, d_pixels=base + 1), dict(reserved=0), dict(reserved=7)):
        first = desc(d_storage=base + 3072, source=16 if "d_pixels" in kw and kw.get("source") == 16 else 8)
        assert call(desc(**kw)) == (0 if kw == dict(source=16) else E), kw
        assert call(first, desc(**kw)) == E, kw
    assert call() == 0 and s.lib.spng_pack_indexed_batch(s.ctx, None, 0, None, None) == 0 and call(desc(), ctx=None) == E
    assert s.lib.spng_pack_indexed_batch(s.ctx, (gpu.PackIndexedDesc * 1)(desc()), 1, None, None) == E      # nowhere to put the results
    s.sync()
    assert (buf[3072:].cpu().numpy() == 0xEE).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _encode(s, gpu, d_storage, w, h, level=6):
    u = gpu.inflated_size(w, h, 8, 1, False)
    cap = s.lib.spng_deflate_bound(u)
    d_rows, d_out = s.empty(u), s.empty(cap)
    d = s.image_desc(d_out, d_rows, d_storage, w, h, 8, 1, False, 0, rows_cap=u)
    d.idat_len = cap
    res = (gpu.Result * 1)()
    assert s.lib.spng_encode_batch(s.ctx, (gpu.ImageDesc * 1)(d), level, 1, None, res) == 0 and res[0].status == 0
    return d_out[:res[0].written]


def test_rgba8_image_to_indexed_png_and_back_on_the_device(gpu):
    """a 64 x 64 RGBA8 image of 200 colours: census -> palette -> mapped pack -> spng_encode_batch (indexed8, level 6) ->
    spng_decode_batch -> spng_unpack_batch with that palette = the pixels; nothing but the 200 keys visits the host"""
    s = gpu.load()
    torch = s.torch
    rng = np.random.default_rng(64)
    colours = distinct(200, RGBA, rng)
    px = pixels_of(colours[rng.integers(0, 200, 64 * 64)], 8, RGBA, rng)
    d_px = s.to_device(px.tobytes())
    (outs, res) = s.census_batch([d_px], 8, RGBA, 256)
    assert res[0].status == 0 and res[0].written == 200
    d_keys = outs[0][0][:200]
    assert int(outs[0][1][:200].sum()) == 64 * 64
    d_idx = s.to_device(bytes(range(200)))                        # the indexer: palette entry i is colour i of the census
    (sto,), res = s.pack_indexed_batch([d_px], [(64, 64)], 8, RGBA, [d_keys], [d_idx])
    assert res[0].status == 0 and res[0].aux[0] == 0
    d_stream = _encode(s, gpu, sto, 64, 64)
    u = gpu.inflated_size(64, 64, 8, 1, False)
    d_rows, d_back = s.empty(u), s.empty(64 * 64)
    r = s.decode_batch([s.image_desc(d_stream.contiguous(), d_rows, d_back, 64, 64, 8, 1, False)])
    assert r[0].status == 0
    d_pal = d_keys.contiguous().view(torch.uint8)                  # the keys ARE (r, g, b, a) quadruplets in memory order
    d_out = s.empty(64 * 64 * 4)
    desc = (gpu.UnpackDesc * 1)(gpu.UnpackDesc(s._ptr(d_back), s._ptr(d_out), s._ptr(d_pal), 64, 64, 200, (ctypes.c_uint16 * 3)(0, 0, 0),
                                               8, 1, 1, 0, 0, 8, RGBA, 0))
    assert s.lib.spng_unpack_batch(s.ctx, desc, 1) == 0
    s.sync()
    assert bytes(d_out[:64 * 64 * 4].cpu().numpy()) == px.tobytes()


def test_the_indexing_tutorial_s_scalar_path(gpu):
    """Snippets/PNG/Indexing.swift: the gradient (first row of the reference's own rendering of it) is the palette; an 8-bit image is
    packed with the identity indexer (storage == pixels), unpacked with the identity deindexer (indices == v), and as RGBA<UInt8>
    with the default deindexer it is gradient[v]"""
    s = gpu.load()
    png = ph.parse_png((ph.GOLDEN / "indexing" / "Indexing-gradient.png").read_bytes())
    st, storage, _ = s.decode(png.idat, 256, 16, 8, 3, False)
    assert st == 0
    rgb = np.frombuffer(storage, dtype=np.uint8).reshape(16, 256, 3)
    assert (rgb == rgb[0]).all()
    gradient = np.concatenate([rgb[0], np.full((256, 1), 255, dtype=np.uint8)], axis=1)
    rng = np.random.default_rng(1)
    v = ((np.arange(300 * 41) * 256 // (300 * 41) + rng.integers(-9, 10, 300 * 41)).clip(0, 255)).astype(np.uint8)
    packed = s.pack(v.tobytes(), 300, 41, 8, 1, indexed=True, source=8, layout=SCALAR, palette=gradient.tobytes(), indexer=lambda _: int)
    assert packed == v.tobytes()
    kw = dict(indexed=True, target=8, palette=gradient.tobytes())
    assert s.unpack(packed, 300, 41, 8, 1, layout=SCALAR, deindexer=lambda _: (lambda i: i), **kw) == v.tobytes()
    assert s.unpack(packed, 300, 41, 8, 1, **kw) == gradient[v].tobytes()
    # a VA deindexer, and an RGBA one that is not the palette
    got = s.unpack(packed, 300, 41, 8, 1, layout=VA, deindexer=lambda _: (lambda i: (255 - i, i)), **kw)
    assert got == np.stack([255 - v, v], axis=1).astype(np.uint8).tobytes()
    got = s.unpack(packed, 300, 41, 8, 1, deindexer=lambda pal: (lambda i: pal[255 - i]), **kw)
    assert got == gradient[255 - v.astype(np.int64)].tobytes()


def test_pack_with_a_nearest_palette_indexer_on_rgba16(gpu):
    s = gpu.load()
    rng = np.random.default_rng(300)
    palette = rng.integers(0, 256, (60, 4), dtype=np.uint8)
    colours = distinct(300, RGBA, rng)
    px = pixels_of(colours[rng.integers(0, 300, 97 * 31)], 16, RGBA, rng)

    def indexer(entries):
        pal = np.array(entries, dtype=np.int64)
        return lambda c: int(((pal - np.array(c, dtype=np.int64)) ** 2).sum(axis=1).argmin())
    got = s.pack(px.tobytes(), 97, 31, 8, 1, indexed=True, source=16, palette=palette.tobytes(), indexer=indexer)
    index = indexer([tuple(int(x) for x in e) for e in palette])
    want = bytes(index(tuple(int(x) >> 8 for x in p)) for p in px)
    assert got == want
    many = rng.integers(0, 256, (70000, 4), dtype=np.uint8)
    with pytest.raises(gpu.SpngError) as e:
        s.pack(many.tobytes(), 70000, 1, 8, 1, indexed=True, source=8, palette=palette.tobytes(), indexer=indexer)
    assert e.value.status == gpu.E_OUTPUT_CAPACITY


CHILD = r"""
import ctypes, sys
from pathlib import Path
import numpy as np
root = Path(sys.argv[1])
sys.path.insert(0, str(root / "tests"))
import indexing_ref as ref
assert "torch" not in sys.modules
lib = ctypes.CDLL(str(root / "swift_png_amd" / "libspng_mi355.so"))
class Result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reserved", ctypes.c_int32), ("written", ctypes.c_uint64),
                ("consumed", ctypes.c_uint64), ("aux", ctypes.c_uint64 * 2)]
vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
rp = ctypes.POINTER(Result)
lib.spng_create.argtypes = [ci, vp, ctypes.POINTER(vp)]
lib.spng_destroy.argtypes = [vp]; lib.spng_destroy.restype = None
lib.spng_census.argtypes = [vp, vp, u64, ci, ci, ci, u32, vp, vp, rp]
lib.spng_pack_indexed.argtypes = [vp, vp, u32, u32, ci, ci, ci, vp, vp, u32, ci, vp, rp]
ctx = vp()
assert lib.spng_create(0, None, ctypes.byref(ctx)) == 0
rng = np.random.default_rng(9)
colours = rng.integers(0, 1 << 16, (500, 4)).astype("<u2")
px = np.ascontiguousarray(colours[rng.integers(0, 500, 123 * 45)])
keys, counts = (ctypes.c_uint32 * 1024)(), (ctypes.c_uint64 * 1024)()
res = Result()
assert lib.spng_census(ctx, px.ctypes.data, len(px), 16, 0, 0, 1024, keys, counts, ctypes.byref(res)) == 0 and res.status == 0
wk, wc = ref.census(px, 16, 0)
n = res.written
assert n == len(wk) and (np.array(keys[:n]) == wk).all() and (np.array(counts[:n]) == wc).all()
assert lib.spng_census(ctx, px.ctypes.data, len(px), 16, 0, 0, 64, keys, None, ctypes.byref(res)) == 0 and res.status == 64 and res.written == 0
idx = (np.arange(n) % 251).astype(np.uint8)
out = (ctypes.c_uint8 * len(px))()
assert lib.spng_pack_indexed(ctx, px.ctypes.data, 123, 45, 16, 0, 0, keys, idx.ctypes.data, n - 100, 250, out, ctypes.byref(res)) == 0
want, missed = ref.pack_indexed(px, 16, 0, wk[:n - 100], idx[:n - 100], 250)
assert res.status == 0 and res.written == len(px) and res.aux[0] == missed and bytes(out) == want.tobytes()
bad = (ctypes.c_uint32 * 2)(7, 7)
assert lib.spng_pack_indexed(ctx, px.ctypes.data, 123, 45, 16, 0, 0, bad, idx.ctypes.data, 2, 0, out, ctypes.byref(res)) == 65
lib.spng_destroy(ctx)
assert "torch" not in sys.modules
print("torch-free indexing ok")
"""


def test_host_pointer_forms_without_torch(gpu):
    r = subprocess.run([sys.executable, "-c", CHILD, str(ph.ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch-free indexing ok" in r.stdout
