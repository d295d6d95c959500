"""GPU: whole files against the files the reference wrote (tests/golden/files.json: length and SHA-256 of every file, the inputs of its
head, where its IDATs are cut).  The 28 outputs of the reference's integration tests from the committed baselines -- lexed, decoded
and compressed on the device, all 28 formats in ONE spng_compress_batch call; the BasicEncoding tutorial's eight files at levels 0, 4,
8, 9 and 13; every snapshot the OnlineDecoding tutorial wrote, plain, progressive and overdrawn; and spng_compress_batch against
spng_encode_batch + a host wait + spng_write_file_batch.  Where a file differs, the message says which chunk: with the IDAT digest of
the fixture still matching the fault is in the head or the cut, otherwise in the encoder."""
import base64
import ctypes
import hashlib
import json

import pytest

import file_ref
import pnghelp as ph
import tutorial_ref as tr

pytestmark = pytest.mark.gpu

FIXTURE = json.loads((ph.GOLDEN / "files.json").read_text())
FILES, BLOBS = FIXTURE["files"], {k: base64.b64decode(v) for k, v in FIXTURE["blobs"].items()}
ONLINE = json.loads((ph.GOLDEN / "online.json").read_text())
OUTPUTS = sorted(n for n, e in FILES.items() if e["source"].startswith("Tests/Outputs/"))
W, H, N = 638, 425, 638 * 425


def sha(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def format_of(e):
    """an entry of files.json -> what swift_png_amd.png_desc takes"""
    as_field = lambda v: None if v is None else v if isinstance(v, int) else tuple(v)
    return dict(indexed=e["indexed"], bgr=e["bgr"], interlaced=e["interlaced"], palette=BLOBS[e["palette"]] if e["palette"] else None,
                key=as_field(e["key"]), fill=as_field(e["fill"]), chunk_bytes=e["chunk_bytes"],
                before=[(n.encode("latin-1"), BLOBS[d]) for n, d in e["before"]], after=[(n.encode("latin-1"), BLOBS[d]) for n, d in e["after"]])


def same_file(name, data):
    """the file is the reference's; if it is not: which chunk"""
    e = FILES[name]
    if (len(data), sha(data)) == (e["len"], e["sha256"]):
        return
    got = file_ref.parse(data)
    idat = b"".join(d for n, d in got if n == b"IDAT")
    if (len(idat), sha(idat)) != (e["idat_len"], e["idat_sha256"]):
        raise AssertionError(f"{name}: the encoder's stream differs ({len(idat)} bytes, {e['idat_len']} in the reference's file)")
    f = format_of(e)
    chunk_bytes = f.pop("chunk_bytes")
    f["palette"] = [tuple(f["palette"][k:k + 4]) for k in range(0, len(f["palette"] or b""), 4)]
    want = file_ref.parse(file_ref.write(idat, chunk_bytes, e["width"], e["height"], e["depth"], e["channels"], **f))
    for k, (a, b) in enumerate(zip(got, want)):
        if a != b:
            raise AssertionError(f"{name}: chunk {k} is {a[0]!r} of {len(a[1])} bytes, the reference has {b[0]!r} of {len(b[1])}: the head or the cut")
    raise AssertionError(f"{name}: {len(got)} chunks, the reference has {len(want)}")


def decode_files(s, gpu, datas):
    """files through spng_lex_batch and spng_decode_batch, each one call: -> [(spng_lexed, the storage on the device)]"""
    n = len(datas)
    d_png, d_idat = [s.to_device(d) for d in datas], [s.empty(len(d)) for d in datas]
    files = (gpu.FileDesc * n)(*[gpu.FileDesc(s._ptr(a), len(d), s._ptr(b), len(d)) for a, b, d in zip(d_png, d_idat, datas)])
    infos = (gpu.Lexed * n)()
    assert s.lib.spng_lex_batch(s.ctx, files, n, None, infos) == 0 and all(r.status == 0 for r in infos)
    descs, keep, storages = [], [], []
    for r, idat in zip(infos, d_idat):
        ch = ph.CHANNELS[r.color]
        d_rows = s.empty(gpu.inflated_size(r.width, r.height, r.depth, ch, bool(r.interlace)))
        d_storage = s.empty(gpu.storage_size(r.width, r.height, r.depth, ch))
        descs.append(s.image_desc(idat[:r.idat_len], d_rows, d_storage, r.width, r.height, r.depth, ch, bool(r.interlace)))
        keep.append(d_rows)
        storages.append(d_storage)
    assert all(r.status == 0 for r in s.decode_batch(descs))
    return list(zip(infos, storages))


@pytest.fixture(scope="module")
def outputs(gpu):
    """the 28 baselines decoded on the device: name -> dict(storage, size, depth, channels) + the fixture's format"""
    s = gpu.load()
    datas = [(ph.GOLDEN / "encode" / n.replace(".png", ".baseline.png")).read_bytes() for n in OUTPUTS]
    images = []
    for name, (r, d_storage) in zip(OUTPUTS, decode_files(s, gpu, datas)):
        e = FILES[name]
        assert (r.width, r.height, r.depth, ph.CHANNELS[r.color], r.interlace) == (e["width"], e["height"], e["depth"], e["channels"], e["interlaced"]), name
        images.append(dict(format_of(e), storage=d_storage, size=(r.width, r.height), depth=r.depth, channels=e["channels"]))
    return images


def test_the_integration_outputs_in_one_call_of_28_mixed_formats(gpu, outputs):
    s = gpu.load()
    assert len(outputs) == 28 and len({(e["depth"], e["channels"], e["indexed"]) for e in (FILES[n] for n in OUTPUTS)}) >= 7
    for name, data in zip(OUTPUTS, s.compress_batch(outputs, level=9)):
        same_file(name, data)


def test_compress_is_encode_wait_write(gpu, outputs):
    """spng_compress_batch byte for byte what spng_encode_batch, a host wait and spng_write_file_batch give: five formats, one chunk
    length that cuts inside the stream everywhere"""
    s = gpu.load()
    images = [dict(im, chunk_bytes=8200) for im in outputs[::6]]
    whole = s.compress_batch(images, level=6)
    for im, data in zip(images, whole):
        im = dict(im)
        d_storage, (w, h), depth, channels = im.pop("storage"), im.pop("size"), im.pop("depth"), im.pop("channels")
        u = gpu.inflated_size(w, h, depth, channels, bool(im["interlaced"]))
        cap = s.lib.spng_deflate_bound(u)
        d_rows, d_idat = s.empty(u), s.empty(cap)
        d = s.image_desc(d_idat, d_rows, d_storage, w, h, depth, channels, bool(im["interlaced"]), 0, rows_cap=u)
        res = (gpu.Result * 1)()
        assert s.lib.spng_encode_batch(s.ctx, (gpu.ImageDesc * 1)(d), 6, 1, None, res) == 0 and res[0].status == 0      # (the host waits here)
        stream = bytes(d_idat[:res[0].written].cpu().numpy())
        assert s.write_file(stream, (w, h), depth, channels, **im) == data
        assert [len(p) for n, p in file_ref.parse(data) if n == b"IDAT"][:-1] == [8200] * ((len(stream) - 1) // 8200)


@pytest.fixture(scope="module")
def rgba(gpu):
    """let rgba:[PNG.RGBA<UInt8>] of the BasicEncoding tutorial, on the device: the committed rgb8 file decoded and unpacked"""
    s = gpu.load()
    (r, d_storage), = decode_files(s, gpu, [(tr.COPIES / tr.RASTER).read_bytes()])
    assert (r.width, r.height, r.depth, r.color, r.interlace) == (W, H, 8, 2, 0)
    d_rgba = s.empty(4 * N)
    und = (gpu.UnpackDesc * 1)(gpu.UnpackDesc(s._ptr(d_storage), s._ptr(d_rgba), None, W, H, 0, (ctypes.c_uint16 * 3)(0, 0, 0), 8, 3, 0, 0, 0,
                                              8, gpu.TARGET_RGBA, 0))
    assert s.lib.spng_unpack_batch(s.ctx, und, 1) == 0
    s.sync()
    return d_rgba


def pack(s, gpu, d_pixels, channels, layout):
    d_storage = s.empty(N * channels)
    pd = (gpu.PackDesc * 1)(gpu.PackDesc(s._ptr(d_pixels), s._ptr(d_storage), None, W, H, 0, 8, channels, 0, 0, 8, layout, 0))
    assert s.lib.spng_pack_batch(s.ctx, pd, 1) == 0
    return d_storage


def test_the_basic_encoding_tutorials_files(gpu, rgba):
    """Snippets/PNG/BasicEncoding.swift end to end: the picture as rgb8 at levels 0, 4, 8, 9 and 13, its red channel as v8, its
    luminance as v8 and rgb8 -- the eight files, the levels of one kind in one call each"""
    s = gpu.load()
    (d_l,), _ = s.luminance_batch([rgba[:4 * N]], gpu.LUMINANCE_V8)
    storages = {"BasicEncoding-color-v.png": pack(s, gpu, rgba, 1, gpu.TARGET_RGBA), "BasicEncoding-luminance-v.png": pack(s, gpu, d_l, 1, gpu.TARGET_SCALAR),
                "BasicEncoding-luminance-rgb.png": pack(s, gpu, d_l, 3, gpu.TARGET_SCALAR)}
    rgb = pack(s, gpu, rgba, 3, gpu.TARGET_RGBA)
    storages.update({name: rgb for name in tr.RGB_LEVELS.values()})
    assert len(storages) == 8
    by_level = {}
    for name in storages:
        by_level.setdefault(FILES[name]["level"], []).append(name)
    assert sorted(by_level) == [0, 4, 8, 9, 13]
    for level, names in sorted(by_level.items()):
        images = [dict(format_of(FILES[n]), storage=storages[n], size=(W, H), depth=8, channels=FILES[n]["channels"]) for n in names]
        for name, data in zip(names, s.compress_batch(images, level=level)):
            same_file(name, data)


@pytest.mark.parametrize("run", sorted(ONLINE))
def test_the_online_decoding_tutorials_snapshots(gpu, run):
    """PNG.decode_online over the committed file in pieces of 4096 bytes, capture compressing the image after every IDAT chunk as the
    tutorial does (image.compress(path:) at the defaults): the files are the reference's snapshot files"""
    s = gpu.load()
    entry = ONLINE[run]
    data = (tr.COPIES / entry["file"]).read_bytes()
    stem = entry["file"][:-4] + ("-overdrawn" if entry["overdraw"] else "")
    shots = []

    def capture(context):
        name = f"{stem}-{len(shots)}.png"
        e = FILES[name]
        shots.append((name, gpu.PNG.compress(context.storage, context.size, context.depth, context.channels, level=e["level"], session=s, **format_of(e))))

    gpu.PNG.decode_online((data[i:i + 4096] for i in range(0, len(data), 4096)), overdraw=entry["overdraw"], capture=capture, session=s)
    assert len(shots) == len(entry["idat_chunks"]) == len([n for n in FILES if n.startswith(stem + "-") and n[len(stem) + 1:-4].isdigit()])
    for name, got in shots:
        same_file(name, got)


def test_standards_interlacing_and_sizes_mixed_in_one_call(gpu):
    """bgr8 with a key, bgra8 interlaced, indexed4 interlaced with alphas and a fill, v16 with a key and blobs, one pixel of v1: one
    call at level 4; every file is file_ref's around the stream the filter and deflate entries give for the same storage"""
    import numpy as np
    s = gpu.load()
    rng = np.random.default_rng(7)
    pal = [(k, 255 - k, 7 * k % 256, 255 if k % 3 else 10 * k) for k in range(13)]
    blobs = [(b"gAMA", b"\0\1\x86\xa0")], [(b"tEXt", b"Title\0mixed"), (b"prVt", b"")]
    images = [dict(size=(33, 9), depth=8, channels=3, bgr=1, key=(1, 2, 3), chunk_bytes=64),
              dict(size=(17, 21), depth=8, channels=4, bgr=1, interlaced=1, fill=(9, 8, 7), chunk_bytes=65544),
              dict(size=(45, 11), depth=4, channels=1, indexed=1, interlaced=1, palette=pal, fill=12, chunk_bytes=8200),
              dict(size=(20, 30), depth=16, channels=1, key=0x1234, before=blobs[0], after=blobs[1], chunk_bytes=100),
              dict(size=(1, 1), depth=1, channels=1, chunk_bytes=1)]
    for im in images:
        (w, h), samples = im["size"], im["channels"] * im["depth"] // 8 or 1
        top = len(pal) if im.get("indexed") else 2 if im["depth"] == 1 else 256
        im["storage"] = rng.integers(0, top, w * h * samples, dtype=np.uint8).tobytes()
    got = s.compress_batch(images, level=4)
    for im, data in zip(images, got):
        (w, h), il, fmt = im["size"], bool(im.get("interlaced")), gpu.FORMAT_IOS if im.get("bgr") else gpu.FORMAT_ZLIB
        stream = s.deflate(s.filter(im["storage"], w, h, im["depth"], im["channels"], il), 4, fmt)
        kw = {k: im[k] for k in ("indexed", "bgr", "interlaced", "palette", "key", "fill", "before", "after") if k in im}
        assert data == file_ref.write(stream, im["chunk_bytes"], w, h, im["depth"], im["channels"], **kw), im["size"]
        assert ph.parse_png(data).idat == stream
