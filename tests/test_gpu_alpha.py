"""GPU checks of spng_alpha_batch / spng_alpha (premultiplied <-> straight alpha on arrays of RGBA<T> / VA<T> pixels) and of the
fused forms: spng_unpack_desc.premultiply = SPNG_STRAIGHTEN*, spng_pack_desc.premultiply.

Expected values come from `alpha` of oracle/pixels.py (`restate` here): PNG.premultiply / PNG.straighten (Sources/PNG/PNG.swift:55-117) and the
(as: UInt8.self) forms (PNG.RGBA.swift:146-158, 192-206) written out in integers.  Where the reference traps (a > 0 and the quotient
exceeds T.max) the documented answer of the device is T.max and a count in aux[0]."""
import ctypes
import json
import sys

import numpy as np
import pytest

import pnghelp as ph

sys.path.insert(0, str(ph.ROOT / "oracle"))
from pixels import alpha as restate  # noqa: E402

pytestmark = pytest.mark.gpu

P, P8, S, S8 = 1, 2, 3, 4                  # SPNG_PREMULTIPLY, _AS_U8, SPNG_STRAIGHTEN, _AS_U8
RGBA, VA, SCALAR = 0, 1, 2
TABLE = json.loads((ph.GOLDEN / "pngsuite.json").read_text())
IOS = sorted(n for n in TABLE if n.startswith("ios/"))


def dtype_of(bits):
    return np.dtype("u1") if bits == 8 else np.dtype("<u2")


def run_batch(s, arrays, bits, layout, op, offset=0, in_place=True):
    """every array of `arrays` ((n, k) integers) as one desc of ONE spng_alpha_batch call, on slots of one device buffer that start
    `offset` bytes behind a 16-byte boundary, 64 bytes apart at least; everything around the slots is poisoned.  Checks status, byte
    count, trap count, the pixels and every byte outside the outputs against `restate`."""
    slots, pos = [], 0
    for a in arrays:
        nbytes = a.size * (bits // 8)
        slots.append((pos + offset, nbytes))
        pos = (pos + offset + nbytes + 64 + 15) & ~15
    host = np.full(pos + 16, 0xEE, dtype=np.uint8)
    want = host.copy()
    trapped = []
    for (at, nbytes), a in zip(slots, arrays):
        host[at:at + nbytes] = np.frombuffer(a.astype(dtype_of(bits)).tobytes(), dtype=np.uint8)
        out, t = restate(a, bits, op)
        want[at:at + nbytes] = np.frombuffer(out.astype(dtype_of(bits)).tobytes(), dtype=np.uint8)
        trapped.append(t)
    d_in = s.to_device(host)
    d_out = d_in if in_place else s.to_device(np.full_like(host, 0xEE))
    res = s.alpha_batch([d_in[at:at + n] for at, n in slots], bits, layout, op, outs=[d_out[at:at + n] for at, n in slots])
    back = d_out.cpu().numpy()
    for r, (at, nbytes), t in zip(res, slots, trapped):
        assert (r.status, r.written, r.aux[0]) == (0, nbytes, t), (r.status, r.written, r.aux[0], nbytes, t)
    bad = np.flatnonzero(back != want)
    assert bad.size == 0, (bits, layout, op, offset, in_place, bad[:8], back[bad[:8]], want[bad[:8]])
    return res


def test_the_references_premultiplication_test(gpu):
    """Sources/PNGTests/Premultiplication.swift for VA<UInt8> over all pairs and VA<UInt16> over 512 x 512 random ones: the premultiplied
    v is round(a c / M), and premultiplied == premultiplied.straightened.premultiplied, the middle step without a trapping component"""
    s = gpu.load()
    rng = np.random.default_rng(1)
    for bits in (8, 16):
        M = (1 << bits) - 1
        if bits == 8:
            c, a = np.divmod(np.arange(65536), 256)
        else:
            c, a = rng.integers(0, 65536, 512 * 512), rng.integers(0, 65536, 512 * 512)
        va = np.stack([c, a], axis=1).astype(dtype_of(bits))
        pre, t0 = s.alpha(va.tobytes(), bits, VA, P)
        pre_px = np.frombuffer(pre, dtype=dtype_of(bits)).reshape(-1, 2).astype(np.int64)
        assert t0 == 0 and (pre_px[:, 1] == a).all()
        assert (pre_px[:, 0] == (2 * a * c + M) // (2 * M)).all()            # round(a c / M): a c / M is never an integer and a half
        straight, t1 = s.alpha(pre, bits, VA, S)
        assert t1 == 0
        again, t2 = s.alpha(straight, bits, VA, P)
        assert t2 == 0 and again == pre
        # the mirror's spelling of the same
        assert (gpu.PNG.VA.premultiplied(gpu.PNG.VA.straightened(gpu.PNG.VA.premultiplied(va, bits), bits), bits) == pre_px).all()


def test_straighten_every_pair_of_eight_bits(gpu):
    """all (p, a) as one VA<UInt8> array: saturation to 255 where p > a > 0 -- 32385 = sum over a of (255 - a) components --, p
    unchanged where a == 0; the same grid as RGBA<UInt8> with three different colour columns"""
    s = gpu.load()
    p, a = np.divmod(np.arange(65536), 256)
    va = np.stack([p, a], axis=1)
    res = run_batch(s, [va], 8, VA, S)
    assert res[0].aux[0] == 32385 == sum(255 - k for k in range(1, 256))
    out, trapped = s.alpha(va.astype(np.uint8).tobytes(), 8, VA, S)
    got = np.frombuffer(out, dtype=np.uint8).reshape(-1, 2)
    assert trapped == 32385 and (got[(p > a) & (a > 0), 0] == 255).all() and (got[a == 0, 0] == p[a == 0]).all()
    rgba = np.stack([p, (p + 85) & 255, (p * 7 + 3) & 255, a], axis=1)
    run_batch(s, [rgba], 8, RGBA, S)
    run_batch(s, [rgba], 8, RGBA, P, in_place=False)
    with pytest.raises(ValueError):
        gpu.PNG.RGBA.straightened(rgba.astype(np.uint8), 8)                 # the mirror's stand-in for the reference's trap
    assert (gpu.PNG.RGBA.straightened(np.array([[10, 20, 30, 40]], dtype=np.uint8), 8) == [[64, 128, 191, 40]]).all()


def sweep16(nc):
    """every alpha of 16 bits with the components 0, 1, a - 1, a, a + 1, 65535 and 66 random ones (half of them below alpha)"""
    rng = np.random.default_rng(16 + nc)
    a = np.arange(65536, dtype=np.int64)[:, None]
    edge = np.concatenate([np.zeros_like(a), np.ones_like(a), (a - 1) & 0xffff, a, (a + 1) & 0xffff, np.full_like(a, 65535)], axis=1)
    below = rng.integers(0, 1 << 62, (65536, 33)) % (a + 1)
    comps = np.concatenate([edge, below, rng.integers(0, 65536, (65536, 33))], axis=1)          # (65536, 72)
    px = np.concatenate([comps.reshape(-1, nc), np.repeat(a, 72 // nc, axis=0)], axis=1)
    return px


@pytest.mark.parametrize("layout", [RGBA, VA])
def test_sixteen_bits_every_alpha(gpu, layout):
    s = gpu.load()
    px = sweep16(1 if layout == VA else 3)
    assert px.shape == (65536 * 72 // (px.shape[1] - 1), px.shape[1])
    for op in (P, P8, S, S8):
        run_batch(s, [px], 16, layout, op, in_place=op != S)


COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("layout", [RGBA, VA])
def test_shapes_offsets_and_batches(gpu, bits, layout):
    """pixel counts around the 16-byte access, the wave and the block; bases on a 16-byte boundary and one pixel behind it; in and out of
    place; descs of very different lengths (an empty one among them) in one call; 1024 opaque, 3 semi-transparent, 1024 clear pixels
    (the wave-uniform shortcut from both sides); 64 poisoned bytes behind every output"""
    s = gpu.load()
    k = 4 if layout == RGBA else 2
    rng = np.random.default_rng(bits + layout)
    M = (1 << bits) - 1
    arrays = []
    for n in COUNTS + [0, 70001]:
        px = rng.integers(0, M + 1, (n, k))
        px[::3, :-1] = px[::3, :-1] * px[::3, -1:] // M                 # (a third of them premultiplied: straighten without a trap)
        arrays.append(px)
    edge = rng.integers(0, M + 1, (2051, k))
    edge[:1024, -1] = M
    edge[1024:1027, -1] = (M // 3, 1, M - 1)
    edge[1027:, -1] = 0
    arrays.append(edge)
    for op in (P, S) + ((P8, S8) if bits == 16 else ()):
        for offset in (0, k * bits // 8):
            for in_place in (True, False):
                run_batch(s, arrays, bits, layout, op, offset=offset, in_place=in_place)
    # one call whose descs differ in layout and operation too
    mixed = [arrays[11], arrays[5][:, :2] if layout == RGBA else arrays[5], arrays[12]]
    layouts = [layout, VA, layout]
    res = s.alpha_batch([s.to_device(np.ascontiguousarray(m).astype(dtype_of(bits)).tobytes()) for m in mixed], bits, layouts, [S, P, P])
    assert [r.status for r in res] == [0, 0, 0] and res[0].aux[0] == restate(mixed[0], bits, S)[1] and res[2].written == 0
    assert s.alpha_batch([], bits, layout, P) == [] and s.alpha(b"", bits, layout, S) == (b"", 0)


def test_refusals(gpu):
    """SPNG_E_ARGUMENT: unknown op / layout / bits, (as: UInt8.self) on eight bits, misaligned pointers, reserved bytes, ranges that
    overlap without being equal, descs that disagree on bits; the fused forms' own"""
    s = gpu.load()
    buf = s.empty(4096)
    base = buf.data_ptr()

    def call(*descs):
        arr = (gpu.AlphaDesc * len(descs))(*descs)
        res = (gpu.Result * len(descs))()
        return s.lib.spng_alpha_batch(s.ctx, arr, len(descs), None, res)

    def desc(d_in=base, d_out=base, count=16, bits=8, layout=RGBA, op=P, reserved=0):
        d = gpu.AlphaDesc(d_in, d_out, count, bits, layout, op)
        d.reserved[4] = reserved
        return d

    assert call(desc()) == 0
    assert call(desc(d_out=base + 64)) == 0 and call(desc(d_in=base + 64)) == 0          # (adjacent ranges)
    assert call(desc(count=0, d_in=None, d_out=None)) == 0
    E = gpu.E_ARGUMENT
    assert call(desc(op=0)) == E and call(desc(op=5)) == E
    assert call(desc(layout=SCALAR)) == E and call(desc(layout=3)) == E
    assert call(desc(bits=12)) == E and call(desc(bits=0)) == E
    assert call(desc(op=P8)) == E and call(desc(op=S8)) == E and call(desc(bits=16, op=S8)) == 0
    assert call(desc(bits=16, d_in=base + 1)) == E and call(desc(bits=16, d_out=base + 1, d_in=base + 512)) == E
    assert call(desc(bits=8, d_in=base + 1, d_out=base + 1)) == 0
    assert call(desc(reserved=1)) == E
    assert call(desc(d_out=base + 4)) == E and call(desc(d_in=base + 60, d_out=base)) == E and call(desc(d_out=base + 63)) == E
    assert call(desc(), desc(bits=16)) == E and call(desc(bits=16), desc(bits=16, d_in=base + 1024, d_out=base + 1024)) == 0
    assert call(desc(d_in=None)) == E
    arr = (gpu.AlphaDesc * 1)(desc())
    assert s.lib.spng_alpha_batch(s.ctx, arr, 1, None, None) == E                     # nowhere to put the results
    assert s.lib.spng_alpha_batch(s.ctx, None, 0, None, None) == 0
    assert s.lib.spng_alpha_batch(None, arr, 1, None, (gpu.Result * 1)()) == E
    quiet = s.to_device(bytes([0xEE]) * 64)                       # a valid desc in front of a spoiled one: nothing is enqueued
    for spoiled in (desc(op=0), desc(reserved=1), desc(d_out=base + 4), desc(bits=16)):
        assert call(desc(d_in=quiet.data_ptr(), d_out=quiet.data_ptr()), spoiled) == E
    s.sync()
    assert (quiet.cpu().numpy() == 0xEE).all()
    # spng_unpack_batch
    def unpack(target, layout, op):
        d = gpu.UnpackDesc(base, base + 2048, None, 4, 4, 0, (ctypes.c_uint16 * 3)(), 8, 4, 0, 0, 0, target, layout, op)
        return s.lib.spng_unpack_batch(s.ctx, (gpu.UnpackDesc * 1)(d), 1)
    assert unpack(8, RGBA, S) == 0 and unpack(16, VA, S8) == 0
    assert unpack(8, RGBA, S8) == E and unpack(8, VA, P8) == E and unpack(16, SCALAR, S) == E and unpack(8, SCALAR, S) == E
    assert unpack(16, RGBA, 5) == E
    # spng_pack_batch
    def pack(source, layout, op, reserved=0):
        d = gpu.PackDesc(base, base + 2048, None, 4, 4, 0, 8, 4, 0, 0, source, layout, op)
        return s.lib.spng_pack_batch(s.ctx, (gpu.PackDesc * 1)(d), 1)
    assert pack(8, RGBA, P) == 0 and pack(16, VA, P8) == 0 and pack(8, SCALAR, 0) == 0
    assert pack(8, RGBA, P8) == E and pack(8, RGBA, S) == E and pack(16, RGBA, S8) == E and pack(16, RGBA, 5) == E
    assert pack(8, SCALAR, P) == E and pack(16, SCALAR, P8) == E
    s.sync()


def _decoded(s, name):
    png = ph.parse_png((ph.GOLDEN / "pngsuite" / name).read_bytes())
    st, storage, _ = s.decode(png.idat, png.width, png.height, png.depth, png.channels, png.interlaced, png.fmt)
    assert st == 0 and png.depth == 8 and png.color in (2, 6)
    return png, storage


def test_fused_unpack_equals_unpack_then_alpha(gpu):
    """every iOS golden: unpack(premultiply: STRAIGHTEN) == alpha(unpack(...), STRAIGHTEN), both targets, both layouts (and the
    (as: UInt8.self) form at sixteen bits)"""
    s = gpu.load()
    assert len(IOS) == 32
    for name in IOS:
        png, storage = _decoded(s, name)
        args = (storage, png.width, png.height, 8, png.channels)
        for target in (8, 16):
            for layout in (RGBA, VA):
                plain = s.unpack(*args, bgr=True, target=target, layout=layout)
                for op in (S,) + ((S8,) if target == 16 else ()):
                    fused = s.unpack(*args, bgr=True, target=target, layout=layout, premultiply=op)
                    two, _ = s.alpha(plain, target, layout, op)
                    assert fused == two, (name, target, layout, op)
                    assert fused == restate(np.frombuffer(plain, dtype=dtype_of(target)).reshape(-1, 4 if layout == RGBA else 2),
                                            target, op)[0].astype(dtype_of(target)).tobytes()


@pytest.mark.parametrize("bits", [8, 16])
def test_fused_pack_equals_alpha_then_pack(gpu, bits):
    """random RGBA<T> arrays of 4096 pixels (the pack kernel's 16-byte paths are taken when the operation is off) and 4099:
    pack(..., premultiply) == pack(alpha(pixels)) into rgba8, bgra8, rgb8, va8, rgba16 and indexed8 (the palette holds the
    premultiplied colours)"""
    s = gpu.load()
    rng = np.random.default_rng(bits)
    M = (1 << bits) - 1
    for n in (4096, 4099):
        base = rng.integers(0, M + 1, (200, 4))
        base[:20, 3] = M; base[20:30, 3] = 0
        px = base[rng.integers(0, 200, n)]
        raw = px.astype(dtype_of(bits)).tobytes()
        for op in (P,) + ((P8,) if bits == 16 else ()):
            pre, trapped = s.alpha(raw, bits, RGBA, op)
            assert trapped == 0 and pre == restate(px, bits, op)[0].astype(dtype_of(bits)).tobytes()
            pre8 = np.frombuffer(pre, dtype=dtype_of(bits)).reshape(-1, 4) >> (bits - 8)
            palette = np.unique(pre8.astype(np.uint8), axis=0)
            assert 150 <= len(palette) <= 256
            palette = palette[rng.permutation(len(palette))].tobytes()
            for (depth, ch, kw) in ((8, 4, {}), (8, 4, dict(bgr=True)), (8, 3, {}), (8, 3, dict(bgr=True)), (8, 2, {}), (16, 4, {}),
                                    (16, 3, {}), (8, 1, dict(indexed=True, palette=palette))):
                two = s.pack(pre, n, 1, depth, ch, source=bits, **kw)
                assert s.pack(raw, n, 1, depth, ch, source=bits, premultiply=op, **kw) == two, (n, op, depth, ch, kw)
                assert s.pack(raw, n, 1, depth, ch, source=bits, **kw) != two
            idx = np.frombuffer(s.pack(raw, n, 1, 8, 1, source=bits, premultiply=op, indexed=True, palette=palette), dtype=np.uint8)
            assert (np.frombuffer(palette, dtype=np.uint8).reshape(-1, 4)[idx] == pre8).all()
            # a VA source too
            va = np.ascontiguousarray(px[:, [0, 3]]).astype(dtype_of(bits)).tobytes()
            assert s.pack(va, n, 1, 8, 2, source=bits, layout=VA, premultiply=op) == \
                s.pack(s.alpha(va, bits, VA, op)[0], n, 1, 8, 2, source=bits, layout=VA)


def _encode(s, gpu, storage, w, h, channels, fmt):
    """spng_encode_batch on one image: -> the stream"""
    u = gpu.inflated_size(w, h, 8, channels, False)
    cap = s.lib.spng_deflate_bound(u)
    d_storage, d_rows, d_out = s.to_device(storage), s.empty(u), s.empty(cap)
    d = s.image_desc(d_out, d_rows, d_storage, w, h, 8, channels, False, fmt, rows_cap=u)
    d.idat_len = cap
    res = (gpu.Result * 1)()
    assert s.lib.spng_encode_batch(s.ctx, (gpu.ImageDesc * 1)(d), 9, 1, None, res) == 0 and res[0].status == 0
    return bytes(d_out[:res[0].written].cpu().numpy())


@pytest.mark.parametrize("name", ["ios/basi6a08.png", "ios/basn6a08.png", "ios/bgan6a08.png", "ios/bgwn6a08.png", "ios/pp0n6a08.png",
                                  "ios/PngSuite.png"])
def test_the_iphone_optimized_tutorial_on_the_device(gpu, name):
    """Snippets/PNG/iPhoneOptimized.swift: decode a CgBI file, unpack(as: RGBA<UInt8>).map(\\.straightened), re-encode as rgb8;
    .map(\\.premultiplied), pack as bgra8, compress with PNG.Standard.ios -- and the file decoded again is the first unpack"""
    s = gpu.load()
    png, storage = _decoded(s, name)
    w, h = png.width, png.height
    first = s.unpack(storage, w, h, 8, png.channels, bgr=True, target=8)
    straight, trapped = s.alpha(first, 8, RGBA, S)
    assert trapped == 0
    assert straight == s.unpack(storage, w, h, 8, png.channels, bgr=True, target=8, premultiply=S)
    if "6a08" in name:
        a = np.frombuffer(first, dtype=np.uint8)[3::4]
        assert ((a > 0) & (a < 255)).sum() == 960 and straight != first
    # rgb8, PNG.Standard.common
    rgb = s.pack(straight, w, h, 8, 3, source=8)
    st, back, _ = s.decode(_encode(s, gpu, rgb, w, h, 3, gpu.FORMAT_ZLIB), w, h, 8, 3, False, gpu.FORMAT_ZLIB)
    assert st == 0 and back == rgb == np.frombuffer(straight, dtype=np.uint8).reshape(-1, 4)[:, :3].tobytes()
    # premultiplied, bgra8, PNG.Standard.ios
    bgra = s.pack(straight, w, h, 8, 4, bgr=True, source=8, premultiply=P)
    assert bgra == s.pack(s.alpha(straight, 8, RGBA, P)[0], w, h, 8, 4, bgr=True, source=8)
    st, back, _ = s.decode(_encode(s, gpu, bgra, w, h, 4, gpu.FORMAT_IOS), w, h, 8, 4, False, gpu.FORMAT_IOS)
    assert st == 0 and back == bgra
    assert s.unpack(back, w, h, 8, 4, bgr=True, target=8) == first
