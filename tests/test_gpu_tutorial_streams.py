"""GPU: the reference's tutorial Snippets/PNG/BasicEncoding.swift end to end on the device from the committed raster, and the device's
encoder against the streams the reference's tutorials wrote (tests/golden/tutorials.json: length and SHA-256 of every file's
concatenated IDAT).  Levels 0, 4, 8, 9 and 13 of the rgb8 picture, its red channel and its luminance as v8 and rgb8 at level 9, and
the two interlaced files re-encoded at their own levels.  The pixels never leave the device between the file and the stream."""
import ctypes
import json

import pytest

import pnghelp as ph
import tutorial_ref as tr

pytestmark = pytest.mark.gpu

TABLE = json.loads((ph.GOLDEN / "tutorials.json").read_text())
W, H, N = 638, 425, 638 * 425


def decode_file(s, gpu, name):
    """a committed file through spng_lex_batch and spng_decode_batch: -> (its spng_lexed, the storage on the device, the IDAT)"""
    data = (tr.COPIES / name).read_bytes()
    d_png, d_idat = s.to_device(data), s.empty(len(data))
    infos = (gpu.Lexed * 1)()
    files = (gpu.FileDesc * 1)(gpu.FileDesc(s._ptr(d_png), len(data), s._ptr(d_idat), len(data)))
    assert s.lib.spng_lex_batch(s.ctx, files, 1, None, infos) == 0 and infos[0].status == 0
    r = infos[0]
    channels = ph.CHANNELS[r.color]
    d_rows = s.empty(gpu.inflated_size(r.width, r.height, r.depth, channels, bool(r.interlace)))
    d_storage = s.empty(r.width * r.height * channels * r.depth // 8)
    res = s.decode_batch([s.image_desc(d_idat[:r.idat_len], d_rows, d_storage, r.width, r.height, r.depth, channels, bool(r.interlace))])
    assert res[0].status == 0
    return r, d_storage, d_idat[:r.idat_len]


def encode(s, gpu, d_storage, w, h, channels, interlaced, level):
    """spng_encode_batch on one image: -> the stream's bytes"""
    u = gpu.inflated_size(w, h, 8, channels, interlaced)
    cap = s.lib.spng_deflate_bound(u)
    d_rows, d_out = s.empty(u), s.empty(cap)
    d = s.image_desc(d_out, d_rows, d_storage, w, h, 8, channels, interlaced, 0, rows_cap=u)
    d.idat_len = cap
    res = (gpu.Result * 1)()
    assert s.lib.spng_encode_batch(s.ctx, (gpu.ImageDesc * 1)(d), level, 1, None, res) == 0 and res[0].status == 0
    return bytes(d_out[:res[0].written].cpu().numpy())


def pack(s, gpu, d_pixels, channels, layout):
    """spng_pack_batch of RGBA<UInt8> / UInt8 pixels into v8 (channels 1) or rgb8 (3): -> the storage on the device"""
    d_storage = s.empty(N * channels)
    pd = (gpu.PackDesc * 1)(gpu.PackDesc(s._ptr(d_pixels), s._ptr(d_storage), None, W, H, 0, 8, channels, 0, 0, 8, layout, 0))
    assert s.lib.spng_pack_batch(s.ctx, pd, 1) == 0
    return d_storage


@pytest.fixture(scope="module")
def rgba(gpu):
    """let rgba:[PNG.RGBA<UInt8>] of the tutorial, on the device: the committed rgb8 file decoded and unpacked (alpha 255 throughout)"""
    s = gpu.load()
    r, d_storage, _ = decode_file(s, gpu, tr.RASTER)
    assert (r.width, r.height, r.depth, r.color, r.interlace) == (W, H, 8, 2, 0)
    d_rgba = s.empty(4 * N)
    und = (gpu.UnpackDesc * 1)(gpu.UnpackDesc(s._ptr(d_storage), s._ptr(d_rgba), None, W, H, 0, (ctypes.c_uint16 * 3)(0, 0, 0), 8, 3, 0, 0, 0,
                                              8, gpu.TARGET_RGBA, 0))
    assert s.lib.spng_unpack_batch(s.ctx, und, 1) == 0
    s.sync()
    return d_rgba


def check(name, idat):
    e = TABLE[name]
    assert (len(idat), tr.sha(idat)) == (e["idat_len"], e["idat_sha256"]), name


@pytest.mark.parametrize("level", sorted(tr.RGB_LEVELS))
def test_the_picture_as_rgb8_at_the_tutorials_levels(gpu, rgba, level):
    """PNG.Image.init(packing: rgba, layout: .rgb8) and compress(level:) for level 0, 4, 8, 9 (the default) and 13"""
    s = gpu.load()
    check(tr.RGB_LEVELS[level], encode(s, gpu, pack(s, gpu, rgba, 3, gpu.TARGET_RGBA), W, H, 3, False, level))


def test_the_picture_as_v8_keeps_the_red_channel(gpu, rgba):
    s = gpu.load()
    check("BasicEncoding-color-v.png", encode(s, gpu, pack(s, gpu, rgba, 1, gpu.TARGET_RGBA), W, H, 1, False, 9))


@pytest.mark.parametrize("name,channels", [("BasicEncoding-luminance-v.png", 1), ("BasicEncoding-luminance-rgb.png", 3)])
def test_the_luminance_as_v8_and_rgb8(gpu, rgba, name, channels):
    """rgba.map(COMPUTE_LUMINANCE) by spng_luminance_batch, the scalar pack, level 9"""
    s = gpu.load()
    (d_l,), (r,) = s.luminance_batch([rgba[:4 * N]], gpu.LUMINANCE_V8)
    assert (r.status, r.written, r.consumed) == (0, N, 4 * N)
    check(name, encode(s, gpu, pack(s, gpu, d_l, channels, gpu.TARGET_SCALAR), W, H, channels, False, 9))


@pytest.mark.parametrize("name", ["OnlineDecoding-progressive.png", "ImagesInMemory.png.png"])
def test_the_interlaced_files_reencode_to_their_own_streams(gpu, name):
    """decoded on the device and encoded again, Adam7, at the level their tutorial wrote them at (9 and 13)"""
    s = gpu.load()
    e = TABLE[name]
    r, d_storage, d_idat = decode_file(s, gpu, name)
    assert r.interlace == 1 and (r.width, r.height) == (e["width"], e["height"])
    idat = encode(s, gpu, d_storage, r.width, r.height, ph.CHANNELS[r.color], True, e["level"])
    check(name, idat)
    assert idat == bytes(d_idat.cpu().numpy())
