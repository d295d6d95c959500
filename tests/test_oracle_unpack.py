"""CPU oracle of `unpack` (oracle/pixels.py), pinned without a GPU on the reference's own goldens.

The reference holds, per PngSuite input, the RGBA<UInt16> pixels it must decode to (Sources/PNGIntegrationTests/RGBA/*.rgba; digests
in tests/golden/pngsuite.json, checked against the reference's files by test_oracle_decode.py).  The storage the pinned decode oracle
produces, unpacked by the restatement here, must have that digest -- for the CgBI set too, whose goldens are the common image's
pixels premultiplied in eight bits (Roundtripping.swift:206-215)."""
import hashlib
import json
import sys

import numpy as np
import pytest

import pnghelp as ph

sys.path.insert(0, str(ph.ROOT / "oracle"))
import pixels as orc  # noqa: E402
from test_oracle_pack import palette_quads, repeats_a_colour  # noqa: E402

TABLE = json.loads((ph.GOLDEN / "pngsuite.json").read_text())
IOS = sorted(n.split("/", 1)[1] for n in TABLE if n.startswith("ios/"))


def fixture(name):
    png = ph.parse_png((ph.GOLDEN / "pngsuite" / name).read_bytes())
    st, storage, _ = ph.orc_decode(png)
    assert st == 0
    key = ph.format_key(png)                    # tRNS (r, g, b); (b, g, r) for a CgBI file, as PNG.Format.swift:427-430 builds .bgr8
    kw = dict(depth=png.depth, channels=png.channels, indexed=png.color == 3, bgr=png.ios and png.color in (2, 6),
              palette=palette_quads(png) if png.color == 3 else None, key=key)
    return png, storage, kw


def test_the_table_holds_all_fixtures():
    assert len(TABLE) == 193 and len(IOS) == 32


@pytest.mark.parametrize("name", sorted(TABLE))
def test_unpack_of_the_storage_is_the_golden(name):
    """RGBA<UInt16> against the reference's digest; RGBA<UInt8> is the same pixels >> 8 (depth <= 8: v * 257 >> 8 == v * (255 / max);
    16: the shift itself); VA<T> is (r, a) of them and the scalar r -- with the key, which it ignores -- and the helper of the other
    tests agrees"""
    png, storage, kw = fixture(name)
    rgba = orc.unpack(storage, target=16, **kw)
    assert rgba.dtype == np.uint16 and rgba.shape == (png.width * png.height, 4)
    assert hashlib.sha256(rgba.astype("<u2").tobytes()).hexdigest() == TABLE[name]["rgba16_sha256"]
    assert (rgba == ph.unpack_rgba16(storage, png)).all()
    rgba8 = orc.unpack(storage, target=8, **kw)
    assert rgba8.dtype == np.uint8 and (rgba8 == rgba >> 8).all()
    for target, px in ((16, rgba), (8, rgba8)):
        assert (orc.unpack(storage, target=target, layout=orc.VA, **kw) == px[:, [0, 3]]).all()
        assert (orc.unpack(storage, target=target, layout=orc.SCALAR, **dict(kw, key=None)) == px[:, 0]).all()
        wide = px.astype(np.uint64)
        tmax = (1 << target) - 1
        pre = orc.unpack(storage, target=target, premultiply=orc.PREMULTIPLY, **kw)
        assert (pre[:, :3] == (wide[:, :3] * wide[:, 3:] + (tmax >> 1)) // tmax).all() and (pre[:, 3] == px[:, 3]).all()
        assert (orc.unpack(storage, target=target, layout=orc.VA, premultiply=orc.PREMULTIPLY, **kw) == pre[:, [0, 3]]).all()


@pytest.mark.parametrize("name", IOS)
def test_premultiplied_as_uint8_is_the_ios_golden(name):
    """.premultiplied(as: UInt8.self) (PNG.RGBA.swift:146-158) of the COMMON image has the digest kept for the CgBI one, and is what
    the helper's premultiply8 gives"""
    png, storage, kw = fixture("common/" + name)
    got = orc.unpack(storage, target=16, premultiply=orc.PREMULTIPLY_AS_U8, **kw)
    assert hashlib.sha256(got.astype("<u2").tobytes()).hexdigest() == TABLE["ios/" + name]["rgba16_sha256"]
    assert (got == ph.premultiply8(orc.unpack(storage, target=16, **kw))).all()


@pytest.mark.parametrize("name", sorted(TABLE))
def test_pack_of_unpack_is_the_storage(name):
    """pack(unpack(storage)) == storage on the fixtures, for every T and layout where the trip is exact:
      T = UInt16 always, T = UInt8 up to depth 8 (the low byte of a 16-bit sample is shifted away);
      VA<T> for v and va formats and the scalar for v formats (a colour format keeps its red channel only, a va format its v);
      indexed formats whose palette holds no colour twice (`pack` refuses the others as the reference traps), through RGBA<T> only:
      a VA / scalar pixel is looked up as (v, v, v, a) / (v, v, v, 255), which finds grey / opaque grey entries alone."""
    png, storage, kw = fixture(name)
    pkw = {k: v for k, v in kw.items() if k != "key"}
    if kw["indexed"] and repeats_a_colour(kw["palette"]):
        with pytest.raises(ValueError):
            orc.pack(orc.unpack(storage, target=16, **kw), **pkw)
        return
    for target in (16, 8) if png.depth <= 8 else (16,):
        assert orc.pack(orc.unpack(storage, target=target, **kw), **pkw) == storage.tobytes()
        if png.channels <= 2 and not kw["indexed"]:
            assert orc.pack(orc.unpack(storage, target=target, layout=orc.VA, **kw), layout=orc.VA, **pkw) == storage.tobytes()
        if png.channels == 1 and not kw["indexed"]:
            assert orc.pack(orc.unpack(storage, target=target, layout=orc.SCALAR, **dict(kw, key=None)), layout=orc.SCALAR, **pkw) == \
                storage.tobytes()


@pytest.mark.parametrize("depth,channels", [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (8, 2), (16, 2), (8, 3), (16, 3), (8, 4), (16, 4)])
def test_pack_of_unpack_on_random_storage(depth, channels):
    """the same trip on random storage of every format (bgr too), the values of 16-bit samples in both bytes"""
    rng = np.random.default_rng(depth * 10 + channels)
    atoms = rng.integers(0, 1 << depth, (333, channels))
    storage = atoms.astype(">u2" if depth == 16 else np.uint8).tobytes()
    for bgr in (False, True) if depth == 8 and channels >= 3 else (False,):
        for target in (16, 8) if depth <= 8 else (16,):
            assert orc.pack(orc.unpack(storage, depth, channels, bgr=bgr, target=target), depth, channels, bgr=bgr) == storage
        got8 = orc.unpack(storage, depth, channels, bgr=bgr, target=8)
        assert (got8 == orc.unpack(storage, depth, channels, bgr=bgr, target=16) >> 8).all()


def test_quantum_and_shift():
    """PNG.swift:255-261, :503-522: depth 2 -> UInt8 times 85, -> UInt16 times 21845; depth 16 -> UInt8 the high byte; a storage byte
    above the depth's range wraps in T (`&*`)"""
    assert orc.unpack(bytes([0, 1, 2, 3]), 2, 1, target=8, layout=orc.SCALAR).tolist() == [0, 85, 170, 255]
    assert orc.unpack(bytes([0, 1, 2, 3]), 2, 1, target=16, layout=orc.SCALAR).tolist() == [0, 21845, 43690, 65535]
    assert orc.unpack(bytes([1, 0]), 1, 1, target=16).tolist() == [[65535] * 4, [0, 0, 0, 65535]]
    assert orc.unpack(bytes([0x12, 0x34, 0xff, 0x01]), 16, 2, target=8).tolist() == [[0x12] * 3 + [0xff]]
    assert orc.unpack(bytes([0x12, 0x34, 0xff, 0x01]), 16, 2, target=16, layout=orc.VA).tolist() == [[0x1234, 0xff01]]
    assert orc.unpack(bytes([7]), 2, 1, target=8, layout=orc.SCALAR).tolist() == [(7 * 85) & 255]


def test_a_key_is_compared_with_the_storage_tuple():
    """PNG.RGBA.swift:318-323: `.bgr8` tests k == key on the atoms as stored and swizzles the output only.  Storage (b, g, r) =
    (1, 2, 3): the key (1, 2, 3) hits, (3, 2, 1) -- the pixel's (r, g, b) -- does not.  `key` is the FORMAT's key, in storage order;
    how a file's tRNS becomes one is the next test."""
    sto = bytes([1, 2, 3, 3, 2, 1])
    hit = orc.unpack(sto, 8, 3, bgr=True, key=(1, 2, 3), target=8)
    assert hit.tolist() == [[3, 2, 1, 0], [1, 2, 3, 255]]
    assert orc.unpack(sto, 8, 3, bgr=True, key=(3, 2, 1), target=8).tolist() == [[3, 2, 1, 255], [1, 2, 3, 0]]
    assert orc.unpack(sto, 8, 3, bgr=True, key=(1, 2, 3), target=8, layout=orc.VA).tolist() == [[3, 0], [1, 255]]
    # at the source depth: 16-bit keys need both bytes, a sub-byte key is the unscaled sample
    assert orc.unpack(bytes([0x12, 0x34, 0x12, 0x35, 0x13, 0x34]), 16, 1, key=(0x1234,), target=8, layout=orc.VA).tolist() == \
        [[0x12, 0], [0x12, 255], [0x13, 255]]
    assert orc.unpack(bytes([2, 3]), 2, 1, key=(2,), target=8, layout=orc.VA).tolist() == [[170, 0], [255, 255]]


def test_the_key_of_a_cgbi_file_is_its_trns_reversed():
    """a FILE's tRNS holds (r, g, b) (PNG.Transparency.swift:154-162); for a CgBI rgb image the reference builds the format's key from
    it as (b, g, r) (PNG.Format.swift:427-430) and compares that with the storage tuple: the pixel whose (r, g, b) equals the tRNS key is
    the keyed one.  Storage (b, g, r) = (1, 2, 3), (3, 2, 1) with tRNS r = 1, g = 2, b = 3 keys the SECOND pixel: through
    pnghelp.format_key and the oracle, and through the helper that models the file"""
    sto = bytes([1, 2, 3, 3, 2, 1])
    png = ph.Png(2, 1, 8, 2, False, True, b"", trns=bytes([0, 1, 0, 2, 0, 3]))
    assert ph.format_key(png) == (3, 2, 1)
    want = [[3, 2, 1, 255], [1, 2, 3, 0]]
    got = orc.unpack(sto, 8, 3, bgr=True, key=ph.format_key(png), target=8)
    assert got.tolist() == want and (got[got[:, 3] == 0, :3] == (1, 2, 3)).all()
    assert (ph.unpack_rgba16(np.frombuffer(sto, dtype=np.uint8), png) >> 8).tolist() == want
    # the same file without CgBI: storage is (r, g, b), the key as tRNS has it, and the first pixel is the keyed one
    common = ph.Png(2, 1, 8, 2, False, False, b"", trns=bytes([0, 1, 0, 2, 0, 3]))
    assert ph.format_key(common) == (1, 2, 3)
    assert orc.unpack(sto, 8, 3, key=ph.format_key(common), target=8).tolist() == [[1, 2, 3, 0], [3, 2, 1, 255]]
    assert (ph.unpack_rgba16(np.frombuffer(sto, dtype=np.uint8), common) >> 8).tolist() == [[1, 2, 3, 0], [3, 2, 1, 255]]
    # grey and indexed files
    assert ph.format_key(ph.Png(1, 1, 16, 0, False, True, b"", trns=bytes([0x12, 0x34]))) == (0x1234,)
    assert ph.format_key(ph.Png(1, 1, 8, 3, False, False, b"", trns=bytes([0, 1]))) is None and ph.format_key(common.__class__(1, 1, 8, 2, False, True, b"")) is None


def test_an_index_beyond_the_palette():
    """the reference traps (`palette[i]`, PNG.Color.swift:204); the device's documented departure is (0, 0, 0, 0)"""
    pal = bytes([10, 20, 30, 40, 50, 60, 70, 80])
    assert orc.unpack(bytes([1, 0]), 8, 1, indexed=True, palette=pal, target=8).tolist() == [[50, 60, 70, 80], [10, 20, 30, 40]]
    assert orc.unpack(bytes([1]), 1, 1, indexed=True, palette=pal, target=16).tolist() == [[50 * 257, 60 * 257, 70 * 257, 80 * 257]]
    with pytest.raises(ValueError):
        orc.unpack(bytes([2]), 8, 1, indexed=True, palette=pal, target=8)
    with pytest.raises(ValueError):
        orc.unpack(bytes([0]), 8, 1, indexed=True, palette=b"", target=8)
    assert orc.unpack(bytes([2, 1]), 8, 1, indexed=True, palette=pal, target=8, beyond_palette=(0, 0, 0, 0)).tolist() == \
        [[0, 0, 0, 0], [50, 60, 70, 80]]
    assert orc.unpack(bytes([9]), 8, 1, indexed=True, palette=pal, target=16, layout=orc.VA, beyond_palette=(0, 0, 0, 0)).tolist() == [[0, 0]]


def test_the_operations_on_unpacked_pixels():
    """premultiply: every operation spng_unpack_batch accepts, as `alpha` of the plain pixels; none for a scalar"""
    sto = bytes([200, 100, 50, 128, 9, 9, 9, 0, 255, 255, 255, 255])
    plain = orc.unpack(sto, 8, 4, target=16)
    for op in (orc.PREMULTIPLY, orc.PREMULTIPLY_AS_U8, orc.STRAIGHTEN, orc.STRAIGHTEN_AS_U8):
        assert (orc.unpack(sto, 8, 4, target=16, premultiply=op) == orc.alpha(plain, 16, op)[0]).all()
    assert orc.unpack(sto, 8, 4, target=8, premultiply=orc.PREMULTIPLY).tolist() == [[100, 50, 25, 128], [0, 0, 0, 0], [255] * 4]
    assert orc.unpack(sto, 8, 4, target=8, premultiply=orc.STRAIGHTEN).tolist() == [[255, 199, 100, 128], [9, 9, 9, 0], [255] * 4]
    with pytest.raises(ValueError):
        orc.unpack(sto, 8, 4, target=8, premultiply=orc.PREMULTIPLY_AS_U8)
    with pytest.raises(ValueError):
        orc.unpack(sto, 8, 4, target=8, layout=orc.SCALAR, premultiply=orc.PREMULTIPLY)
