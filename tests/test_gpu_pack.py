"""GPU parity of spng_pack_batch / spng_pack_as (f3, the encode half: PNG.Image.init(packing:size:layout:)) against
oracle/pixels.py, which tests/test_oracle_pack.py pins on the reference's golden pixels; and of the scalar unpack target."""
import ctypes
import json
import sys

import numpy as np
import pytest

import pnghelp as ph

sys.path.insert(0, str(ph.ROOT / "oracle"))
import pixels as orc_pixels  # noqa: E402
import unpack_cases  # noqa: E402
from test_oracle_pack import golden_case, repeats_a_colour  # noqa: E402

pytestmark = pytest.mark.gpu
TABLE = json.loads((ph.GOLDEN / "pngsuite.json").read_text())


@pytest.mark.parametrize("name", sorted(TABLE))
def test_pack_golden_pixels_vs_oracle(gpu, name):
    """every PngSuite image: its golden RGBA<UInt16> pixels (and their UInt8 / VA / scalar views) packed as the image's own
    format on the device = the oracle's storage = (T = UInt16, RGBA) the storage the decode produced."""
    s = gpu.load()
    png, storage, rgba, kw = golden_case(name)
    args = (png.width, png.height, png.depth, png.channels)
    dkw = dict(indexed=kw["indexed"], bgr=kw["bgr"], palette=kw["palette"])
    if kw["indexed"] and repeats_a_colour(kw["palette"]):
        # the reference traps here; the device's documented answer: the lowest index of a repeated colour
        got = np.frombuffer(s.pack(rgba.astype("<u2").tobytes(), *args, source=16, **dkw), dtype=np.uint8)
        pal = np.frombuffer(kw["palette"], dtype=np.uint8).reshape(-1, 4)
        first = {}
        for i, e in enumerate(pal):
            first.setdefault(tuple(e), i)
        want = np.array([first[tuple(pal[i])] for i in storage], dtype=np.uint8)
        assert (got == want).all()
        return
    for dt, src in (("<u2", rgba), ("u1", (rgba >> 8).astype(np.uint8))):
        bits = 16 if dt == "<u2" else 8
        got = s.pack(src.astype(dt).tobytes(), *args, source=bits, **dkw)
        assert got == orc_pixels.pack(src, **kw), (name, bits)
        if bits == 16:
            assert got == storage.tobytes()
        va = np.ascontiguousarray(src[:, [0, 3]])
        assert s.pack(va.astype(dt).tobytes(), *args, source=bits, layout=gpu.TARGET_VA, **dkw) == \
            orc_pixels.pack(va, layout=orc_pixels.VA, **kw)
        v = np.ascontiguousarray(src[:, 0])
        assert s.pack(v.astype(dt).tobytes(), *args, source=bits, layout=gpu.TARGET_SCALAR, **dkw) == \
            orc_pixels.pack(v, layout=orc_pixels.SCALAR, **kw)


FORMATS = [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (8, 2), (16, 2), (8, 3), (16, 3), (8, 4), (16, 4)]


@pytest.mark.parametrize("depth,channels", FORMATS)
@pytest.mark.parametrize("bits", [8, 16])
def test_pack_random_pixels_every_format(gpu, depth, channels, bits):
    """random pixels of every colour target into every format (bgr too), sizes that leave 0-3 pixels behind the last quad, and those
    of the case table (tests/unpack_cases.py): 255 / 256 / 257 quads, and full and partly filled last waves for the pixels of 3 and 6
    bytes that leave through LDS"""
    s = gpu.load()
    rng = np.random.default_rng(depth * 100 + channels * 10 + bits)
    dt = np.uint8 if bits == 8 else np.uint16
    for (w, h) in [(1, 1), (3, 1), (5, 3), (64, 9), (257, 31), (1023, 17)] + [z for z in unpack_cases.PACK_SIZES if z not in unpack_cases.TAILS + unpack_cases.TURNS]:
        n = w * h
        for layout, k in ((orc_pixels.RGBA, 4), (orc_pixels.VA, 2), (orc_pixels.SCALAR, 1)):
            px = rng.integers(0, 1 << bits, (n, k), dtype=np.uint32).astype(dt)
            for bgr in ((False, True) if (channels >= 3 and depth == 8) else (False,)):
                want = orc_pixels.pack(px if k > 1 else px[:, 0], depth, channels, bgr=bgr, layout=layout)
                got = s.pack(px.astype("<u%d" % (bits // 8)).tobytes(), w, h, depth, channels, bgr=bgr, source=bits, layout=layout)
                assert got == want, (w, h, layout, bgr)


@pytest.mark.parametrize("depth", [1, 2, 4, 8])
@pytest.mark.parametrize("bits", [8, 16])
def test_pack_indexed_with_strangers(gpu, depth, bits):
    """indexed formats: the default indexer finds the entry equal to the pixel (reduced to 8 bits) and gives entry 0 to colours
    the palette does not hold (PNG.Color.swift:182-190)"""
    s = gpu.load()
    rng = np.random.default_rng(depth + bits)
    count = min(1 << depth, 256)
    pal = np.unique(rng.integers(0, 256, (600, 4), dtype=np.uint8), axis=0)
    pal = pal[rng.permutation(len(pal))[:count]]
    dt = np.uint8 if bits == 8 else np.uint16
    w, h = 331, 47
    idx = rng.integers(0, count, w * h)
    px = pal[idx].astype(np.uint32)
    strangers = rng.random(w * h) < 0.2
    px[strangers] = rng.integers(0, 256, (int(strangers.sum()), 4))
    if bits == 16:
        px = px << 8 | rng.integers(0, 256, px.shape)       # the low byte is shifted away
    px = px.astype(dt)
    for layout, view in ((orc_pixels.RGBA, px), (orc_pixels.VA, np.ascontiguousarray(px[:, [0, 3]])),
                         (orc_pixels.SCALAR, np.ascontiguousarray(px[:, 0]))):
        want = orc_pixels.pack(view, depth, 1, indexed=True, palette=pal.tobytes(), layout=layout)
        got = s.pack(view.astype("<u%d" % (bits // 8)).tobytes(), w, h, depth, 1, indexed=True, source=bits, palette=pal.tobytes(),
                     layout=layout)
        assert got == want, layout
    # grey palettes, so that the (v, v, v, a) and (v, v, v, 255) indexers find something
    g = rng.permutation(256)[:count].astype(np.uint8)
    gpal = np.stack([g, g, g, np.full(count, 255, dtype=np.uint8)], axis=1)
    v = g[rng.integers(0, count, w * h)].astype(dt)
    if bits == 16:
        v = (v.astype(np.uint32) << 8 | 0x5a).astype(dt)
    want = orc_pixels.pack(v, depth, 1, indexed=True, palette=gpal.tobytes(), layout=orc_pixels.SCALAR)
    assert np.frombuffer(want, dtype=np.uint8).any()
    assert s.pack(v.astype("<u%d" % (bits // 8)).tobytes(), w, h, depth, 1, indexed=True, source=bits, palette=gpal.tobytes(),
                  layout=gpu.TARGET_SCALAR) == want


@pytest.mark.parametrize("name", sorted(TABLE)[::5])
def test_unpack_scalar_target(gpu, name):
    """PNG.Image.unpack<T>(as:) (PNG.Image.swift:682-760, 1030-1040): the grey value / the red channel / palette[i].r, keys
    ignored -- the r component of the RGBA<T> pixels the goldens pin"""
    import struct
    s = gpu.load()
    png, storage, rgba, kw = golden_case(name)
    key = ph.format_key(png)                                        # (a CgBI file's tRNS reversed: the bgr8 format's key is (b, g, r))
    args = (storage.tobytes(), png.width, png.height, png.depth, png.channels)
    ukw = dict(indexed=kw["indexed"], bgr=kw["bgr"], palette=kw["palette"], key=key)
    got16 = np.frombuffer(s.unpack(*args, target=16, layout=gpu.TARGET_SCALAR, **ukw), dtype="<u2")
    assert (got16 == rgba[:, 0]).all()
    got8 = np.frombuffer(s.unpack(*args, target=8, layout=gpu.TARGET_SCALAR, **ukw), dtype=np.uint8)
    assert (got8 == (rgba[:, 0] >> 8)).all()


def test_pack_then_encode_then_decode_round_trip(gpu):
    """pixels -> storage -> PNG stream -> storage -> pixels on the device: what Image(packing:).compress / decompress.unpack do"""
    import zlib
    s = gpu.load()
    rng = np.random.default_rng(5)
    w, h = 200, 120
    px = rng.integers(0, 256, (w * h, 4), dtype=np.uint8)
    px[:, :3] &= 0xf0
    storage = s.pack(px.tobytes(), w, h, 8, 3, source=8)
    assert storage == px[:, :3].tobytes()
    rows = s.filter(storage, w, h, 8, 3, False)
    z = s.deflate(rows, 9)
    assert zlib.decompress(z) == rows
    st, back, _ = s.decode(z, w, h, 8, 3, False)
    assert st == 0 and back == storage
    out = np.frombuffer(s.unpack(back, w, h, 8, 3, target=8), dtype=np.uint8).reshape(-1, 4)
    assert (out[:, :3] == px[:, :3]).all() and (out[:, 3] == 255).all()


def test_refusals(gpu):
    """SPNG_E_ARGUMENT from spng_unpack_batch and spng_pack_batch, each refused on the host before anything is enqueued: a valid base
    desc of a 4 x 4 image with one field spoiled at a time, alone and behind a valid desc whose poisoned output stays untouched"""
    s = gpu.load()
    buf = s.to_device(bytes([0xEE]) * 4096)
    base = buf.data_ptr()
    E = gpu.E_ARGUMENT
    RGBA, SCALAR = gpu.TARGET_RGBA, gpu.TARGET_SCALAR
    quiet = base + 3072                                          # (the output of the valid desc in front of a spoiled one)

    def udesc(d_storage=base, d_out=base + 2048, d_palette=None, palette_count=0, depth=8, channels=4, indexed=0, target=8,
              layout=RGBA, premultiply=0):
        return gpu.UnpackDesc(d_storage, d_out, d_palette, 4, 4, palette_count, (ctypes.c_uint16 * 3)(), depth, channels, indexed, 0, 0,
                              target, layout, premultiply)

    def unpack(*descs, ctx=s.ctx):
        return s.lib.spng_unpack_batch(ctx, (gpu.UnpackDesc * len(descs))(*descs), len(descs))

    def pdesc(d_pixels=base, d_storage=base + 2048, d_palette=None, palette_count=0, depth=8, channels=4, indexed=0, source=8,
              layout=RGBA, premultiply=0):
        return gpu.PackDesc(d_pixels, d_storage, d_palette, 4, 4, palette_count, depth, channels, indexed, 0, source, layout, premultiply)

    def pack(*descs, ctx=s.ctx):
        return s.lib.spng_pack_batch(ctx, (gpu.PackDesc * len(descs))(*descs), len(descs))

    common = [dict(depth=3), dict(d_storage=None), dict(indexed=1, channels=3), dict(indexed=1, channels=1, depth=16),
              dict(indexed=1, channels=1, palette_count=4), dict(layout=3), dict(premultiply=5), dict(premultiply=2),
              dict(layout=SCALAR, premultiply=1)]
    # spng_unpack_batch
    assert unpack(udesc()) == 0 and unpack(udesc(target=16)) == 0 and unpack(udesc(target=16, premultiply=4)) == 0
    assert unpack(udesc(target=12)) == E and unpack(udesc(target=12), udesc(target=12)) == E
    for kw in common + [dict(target=16), dict(d_out=None), dict(premultiply=4)]:
        assert unpack(udesc(**kw)) == (0 if kw == dict(target=16) else E), kw
        assert unpack(udesc(d_out=quiet), udesc(**kw)) == E, kw
    assert unpack() == 0 and s.lib.spng_unpack_batch(s.ctx, None, 0) == 0 and s.lib.spng_unpack_batch(s.ctx, None, 1) == E
    assert unpack(udesc(), ctx=None) == E
    # spng_pack_batch
    assert pack(pdesc()) == 0 and pack(pdesc(source=16)) == 0 and pack(pdesc(source=16, premultiply=2)) == 0
    assert pack(pdesc(source=12)) == E and pack(pdesc(source=12), pdesc(source=12)) == E
    for kw in common + [dict(source=16), dict(d_pixels=None), dict(premultiply=3), dict(source=16, d_pixels=base + 1),
                        dict(indexed=1, channels=1, d_palette=base + 1024, palette_count=257)]:
        assert pack(pdesc(**kw)) == (0 if kw == dict(source=16) else E), kw
        first = pdesc(d_storage=quiet, source=16) if kw.get("d_pixels") == base + 1 else pdesc(d_storage=quiet)
        assert pack(first, pdesc(**kw)) == E, kw
    assert pack(pdesc(indexed=1, channels=1, d_palette=base + 1024, palette_count=256)) == 0
    assert pack() == 0 and s.lib.spng_pack_batch(s.ctx, None, 0) == 0 and s.lib.spng_pack_batch(s.ctx, None, 1) == E
    assert pack(pdesc(), ctx=None) == E
    s.sync()
    assert (buf[3072:].cpu().numpy() == 0xEE).all()
