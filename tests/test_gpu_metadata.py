"""GPU: the chunk directory (spng_lex_dir_batch), the text entry (spng_text_batch) and the metadata round trip of the host mirror
(PNG.decompress, PNG.compress(metadata=)).  The case table of tests/metadata_cases.py through the C ABI against tests/metadata_ref.py --
every case in a call of its own, and all of them in one batch --, the directory's infos against spng_lex_batch's field for field, and
the reference's tutorials end to end: a source file through the device gives, byte for byte, the file the reference wrote from it
(SHA-256 from tests/golden/files.json)."""
import base64
import ctypes
import hashlib
import json
import struct
import zlib

import pytest

import metadata_cases as mc
import metadata_ref as mr
import pnghelp as ph
from lex_ref import lex_ref, of_struct

pytestmark = pytest.mark.gpu
FILES = json.loads((ph.GOLDEN / "files.json").read_text())
META = ph.GOLDEN / "metadata"
DIR_CASES, HEAD_CASES, TRANSCODE_CASES, UTF8_CASES = mc.dir_cases(), mc.head_cases(), mc.transcode_cases(), mc.utf8_cases()


def head_of(e):
    return mr.Head(e.status, e.aux, e.k, e.l, e.m, e.body_off, e.compressed)


def dir_vs_ref(gpu, s, files, caps=None):
    """spng_lex_dir_batch over `files` as one batch: the infos are spng_lex_batch's byte for byte and lex_ref's field for field, the IDAT
    bytes are the same, the entries in front of min(chunks, cap) are metadata_ref's, and behind them nothing has been touched"""
    n = len(files)
    caps = [len(f) // 12 for f in files] if caps is None else list(caps)
    size = ctypes.sizeof(gpu.ChunkEntry)
    d_png = [s.to_device(f) for f in files]
    d_idat = [[s.to_device(b"\xEE" * (len(f) + 32)) for f in files] for _ in range(2)]
    d_ent = [s.to_device(b"\xEE" * ((cap + 2) * size)) for cap in caps]
    descs = [(gpu.FileDesc * n)(*[gpu.FileDesc(s._ptr(a), len(f), s._ptr(b), len(f)) for f, a, b in zip(files, d_png, d_idat[k])]) for k in range(2)]
    dirs = (gpu.ChunkDir * n)(*[gpu.ChunkDir(e.data_ptr() if cap else None, cap, 0) for e, cap in zip(d_ent, caps)])
    plain, infos = (gpu.Lexed * n)(), (gpu.Lexed * n)()
    assert s.lib.spng_lex_batch(s.ctx, descs[0], n, None, plain) == 0
    assert s.lib.spng_lex_dir_batch(s.ctx, descs[1], dirs, n, None, infos) == 0
    assert bytes(plain) == bytes(infos)
    for k, (f, cap, got) in enumerate(zip(files, caps, infos)):
        want, idat = lex_ref(f, len(f))
        assert of_struct(got) == want, (k, of_struct(got), want)
        a, b = bytes(d_idat[0][k].cpu().numpy()), bytes(d_idat[1][k].cpu().numpy())
        assert a[:got.idat_len] == b[:got.idat_len] == idat and b[len(f):] == b"\xEE" * 32, k
        filled = min(got.chunks, cap)
        raw = bytes(d_ent[k].cpu().numpy())
        entries = list((gpu.ChunkEntry * filled).from_buffer_copy(raw[:filled * size]))
        for e, w in zip(entries, mr.directory(f, got.chunks)):
            assert (e.type, e.length, e.offset, head_of(e), bytes(e.pad)) == (w.type, w.length, w.offset, w.head, bytes(7)), (k, w)
        assert raw[filled * size:] == b"\xEE" * (len(raw) - filled * size), k
    return list(infos)


@pytest.mark.parametrize("case", DIR_CASES, ids=[c.name for c in DIR_CASES])
def test_directory(gpu, case):
    infos = dir_vs_ref(gpu, gpu.load(), case.files, case.caps)
    if case.chunks is not None:
        assert [r.chunks for r in infos] == case.chunks


def test_directory_all_in_one_batch(gpu):
    files, caps = [], []
    for case in DIR_CASES:
        files += case.files
        caps += case.caps or [len(f) // 12 for f in case.files]
    dir_vs_ref(gpu, gpu.load(), files, caps)


def test_heads_each_alone(gpu):
    s = gpu.load()
    for c in HEAD_CASES:
        f = mc.head_file(c)
        (info,), _, (entries,) = s.lex_dir_batch([f])
        assert info.status == 0 and len(entries) == 3, c.name
        assert head_of(entries[1]) == mr.parse_head(c.kind, c.payload), c.name
        assert entries[1].status == c.status, c.name


def test_heads_in_one_batch_and_in_one_file(gpu):
    """a head's status is that chunk's only: the file lexes as it would without it"""
    s = gpu.load()
    dir_vs_ref(gpu, s, [mc.head_file(c) for c in HEAD_CASES])
    (info,) = dir_vs_ref(gpu, s, [mc.file_of(*[mc.chunk(c.kind, c.payload) for c in HEAD_CASES])])
    assert info.status == 0 and info.chunks == len(HEAD_CASES) + 2


def placed(s, data, at):
    """`data` on the device, `at` bytes behind a 16-byte boundary, 0xA5 around it -> (the whole tensor, its offset in it)"""
    whole = s.to_device(b"\xA5" * (len(data) + 96))
    off = (-whole.data_ptr()) % 16 + 32 + at
    if data:
        whole[off:off + len(data)] = s.to_device(data)
    return whole, off


def transcode(gpu, s, cases):
    """one spng_text_batch call over `cases`, compared with the yardstick, the bytes around every output included"""
    n = len(cases)
    srcs = [placed(s, c.data, c.src_at) for c in cases]
    wants = [mr.latin1_to_utf8(c.data) for c in cases]
    caps = [max(len(w) + c.cap_delta, 0) for w, c in zip(wants, cases)]
    dsts = [placed(s, b"\xA5" * cap, c.dst_at) for cap, c in zip(caps, cases)]
    descs = (gpu.TextDesc * n)()
    for i, ((src, so), (dst, do), c, cap) in enumerate(zip(srcs, dsts, cases, caps)):
        descs[i] = gpu.TextDesc(src.data_ptr() + so, len(c.data), dst.data_ptr() + do, cap, gpu.TEXT_LATIN1_TO_UTF8, (ctypes.c_uint8 * 7)())
        assert (src.data_ptr() + so) % 16 == c.src_at and (dst.data_ptr() + do) % 16 == c.dst_at
    res = (gpu.Result * n)()
    assert s.lib.spng_text_batch(s.ctx, descs, n, None, res) == 0
    for r, c, want, cap, (dst, do) in zip(res, cases, wants, caps, dsts):
        short = cap < len(want)
        assert (r.status, r.written, r.consumed, r.aux[0], r.aux[1]) == (mr.E_OUTPUT_CAPACITY if short else mr.DONE, len(want), len(c.data), 0, 0), c.name
        got = bytes(dst.cpu().numpy())
        assert got == b"\xA5" * do + (b"" if short else want) + b"\xA5" * (len(got) - do - (0 if short else len(want))), c.name


def test_transcode_each_alone(gpu):
    s = gpu.load()
    for c in TRANSCODE_CASES:
        transcode(gpu, s, [c])


def test_transcode_in_one_batch(gpu):
    transcode(gpu, gpu.load(), TRANSCODE_CASES)


def check(gpu, s, cases):
    n = len(cases)
    srcs = [placed(s, c.data, k % 4) for k, c in enumerate(cases)]
    descs = (gpu.TextDesc * n)()
    for i, ((src, so), c) in enumerate(zip(srcs, cases)):
        descs[i] = gpu.TextDesc(src.data_ptr() + so, len(c.data), None, 0, gpu.TEXT_CHECK_UTF8, (ctypes.c_uint8 * 7)())
    res = (gpu.Result * n)()
    assert s.lib.spng_text_batch(s.ctx, descs, n, None, res) == 0
    for r, c in zip(res, cases):
        st, first, count = mr.check_utf8(c.data)
        assert (r.status, r.written, r.consumed, r.aux[0], r.aux[1]) == (st, 0, len(c.data), first, count), c.name
        assert (None if r.status == 0 else (r.aux[0], r.aux[1])) == c.claim, c.name


def test_check_utf8_each_alone(gpu):
    s = gpu.load()
    for c in UTF8_CASES:
        check(gpu, s, [c])


def test_check_utf8_in_one_batch(gpu):
    check(gpu, gpu.load(), UTF8_CASES)


def test_a_text_of_many_tiles_and_mixed_operations(gpu):
    """1 MiB + 1 of text on many workgroups, transcoded and checked in one call"""
    s = gpu.load()
    data = mc.pattern((1 << 20) + 1, "alternating")
    good = mr.latin1_to_utf8(data)
    bad = good[:700001] + b"\xa9" + good[700001:]
    outs, res = s.text_batch([data, good, bad], [gpu.TEXT_LATIN1_TO_UTF8, gpu.TEXT_CHECK_UTF8, gpu.TEXT_CHECK_UTF8])
    assert res[0].status == 0 and bytes(outs[0][:res[0].written].cpu().numpy()) == good
    assert (res[1].status, res[1].aux[0], res[1].aux[1]) == (0, 0, 0)
    assert (res[2].status, res[2].aux[0], res[2].aux[1]) == mr.check_utf8(bad)


def test_text_batch_refuses(gpu):
    s = gpu.load()
    t = s.to_device(b"abcdefgh" * 8)
    res = (gpu.Result * 1)()
    for d in (gpu.TextDesc(t.data_ptr(), 8, t.data_ptr() + 32, 16, 3, (ctypes.c_uint8 * 7)()),                  # an unknown op
              gpu.TextDesc(t.data_ptr(), 8, t.data_ptr() + 32, 16, 1, (ctypes.c_uint8 * 7)(0, 0, 1)),             # a reserved byte
              gpu.TextDesc(None, 8, t.data_ptr() + 32, 16, 1, (ctypes.c_uint8 * 7)()),                            # no input
              gpu.TextDesc(t.data_ptr(), 8, None, 16, 1, (ctypes.c_uint8 * 7)()),                                 # no output
              gpu.TextDesc(t.data_ptr(), 16, t.data_ptr() + 8, 32, 1, (ctypes.c_uint8 * 7)())):                   # overlap
        assert s.lib.spng_text_batch(s.ctx, (gpu.TextDesc * 1)(d), 1, None, res) == gpu.E_ARGUMENT
    assert s.lib.spng_text_batch(s.ctx, None, 0, None, None) == 0
    # no room at all is a question, not a mistake: the bytes needed come back
    assert s.lib.spng_text_batch(s.ctx, (gpu.TextDesc * 1)(gpu.TextDesc(t.data_ptr(), 8, None, 0, 1, (ctypes.c_uint8 * 7)())), 1, None, res) == 0
    assert (res[0].status, res[0].written) == (gpu.E_OUTPUT_CAPACITY, 8)
    assert gpu.load_library().spng_status_string(gpu.E_TEXT_ENCODING) == b"text is not well-formed utf-8"


# ---- end to end: the reference's tutorials -----------------------------------------------------------------------------------------
def recorded(name):
    entry = FILES["files"][name]
    return [(k.encode("latin-1"), base64.b64decode(FILES["blobs"][h])) for k, h in entry["before"] + entry["after"]]


def round_trip(gpu, source, written, level, edit=None):
    from swift_png_amd.mirror import PNG
    s = gpu.load()
    image = PNG.decompress((META / source).read_bytes(), session=s)
    if edit:
        edit(image.metadata)
    out = PNG.compress(image.storage, image.size, image.depth, image.channels, level=level, chunk_bytes=FILES["files"][written]["chunk_bytes"],
                       metadata=image.metadata, session=s, **image.format())
    entry = FILES["files"][written]
    assert len(out) == entry["len"] and hashlib.sha256(out).hexdigest() == entry["sha256"]
    return image


def test_image_metadata_tutorial(gpu):
    """Snippets/PNG/ImageMetadata.swift: read the metadata, set the time, write the file back"""
    def set_time(metadata):
        assert metadata.time == (2024, 1, 30, 22, 1, 56)
        metadata.time = (1992, 8, 3, 0, 0, 0)
    image = round_trip(gpu, "ImageMetadata.png", "ImageMetadata-newtime.png", 9, set_time)
    m = image.metadata
    assert m.gamma == 45455 and m.physicalDimensions == (2835, 2835, 1) and image.fill == (255, 255, 255)
    assert m.colorProfile.name == "ICC profile" and len(m.colorProfile.profile) == 672
    assert [(t.keyword, t.language, t.compressed) for t in m.text] == [(("Raw profile type exif", ""), ["en"], True),
                                                                         (("XML:com.adobe.xmp", ""), [], False)]
    assert len(m.text[0].content.encode("utf-8")) >= 37124


def test_images_in_memory_tutorial(gpu):
    round_trip(gpu, "ImagesInMemory.png", "ImagesInMemory.png.png", 13)


def test_basic_decoding_metadata(gpu):
    """the chunks of BasicDecoding.png around a one-pixel image: its metadata, written back, is the ancillary chunks of BasicDecoding.va.png"""
    from swift_png_amd.mirror import PNG
    s = gpu.load()
    table = json.loads((META / "metadata.json").read_text())["BasicDecoding.png"]
    chunks = [(k.encode("latin-1"), base64.b64decode(v)) for k, v in table["chunks"]]
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    small = [(b"IHDR", struct.pack(">IIBBBBB", 1, 1, 8, 0, 0, 0, 0))] + chunks[1:-1] + [(b"IDAT", zlib.compress(b"\0\x7f")), (b"IEND", b"")]
    image = PNG.decompress(mc.SIG + b"".join(mc.chunk(k, v) for k, v in small), session=s)
    assert image.storage == b"\x7f" and image.size == (1, 1)
    m = image.metadata
    outs, res = s.deflate_batch([s.to_device(p) for p in m.to_deflate()], 13)
    before, after = m.chunks([bytes(o[:r.written].cpu().numpy()) for o, r in zip(outs, res)])
    assert before + after == recorded("BasicDecoding.va.png") == recorded("BasicDecoding.v.png")


def test_decompress_raises_what_the_reference_throws(gpu):
    from swift_png_amd.mirror import PNG, DuplicateChunk, RequiredChunk, UnexpectedChunk
    s = gpu.load()
    idat = mc.chunk(b"IDAT", zlib.compress((b"\0" + bytes(32)) * 32))
    gama = mc.chunk(b"gAMA", struct.pack(">I", 45455))
    plte = mc.chunk(b"PLTE", bytes(6))
    ihdr3 = mc.chunk(b"IHDR", struct.pack(">IIBBBBB", 32, 32, 8, 3, 0, 0, 0))
    text = lambda p: mc.chunk(b"iTXt", p)  # noqa: E731
    ok = PNG.decompress(mc.file_of(gama, text(b"Title\0\0\0EN-us\0Titel\0caf\xc3\xa9"), idat, mc.chunk(b"tEXt", b"Author\0\xe9")), session=s)
    assert ok.storage == bytes(32 * 32) and ok.metadata.gamma == 45455
    assert ok.metadata.text == [PNG.Text(False, ("Title", "Titel"), ["en", "us"], "café"), PNG.Text(False, ("Author", ""), ["en"], "é")]
    repaired = PNG.decompress(mc.file_of(text(b"Title\0\0\0\0\0caf\xe9!"), idat), session=s)
    assert repaired.metadata.text[0].content == "caf\ufffd!"
    cases = [(mc.SIG + gama + mc.IHDR + idat + mc.IEND, RequiredChunk, ("IHDR", "gAMA")),
             (mc.file_of(mc.IHDR, idat), DuplicateChunk, ("IHDR",)),
             (mc.file_of(gama, gama, idat), DuplicateChunk, ("gAMA",)),
             (mc.file_of(plte, gama, idat), UnexpectedChunk, ("gAMA", "PLTE")),
             (mc.file_of(idat, gama), UnexpectedChunk, ("gAMA", "IDAT")),
             (mc.file_of(idat, mc.chunk(b"tEXt", b"k\0v"), idat), UnexpectedChunk, ("IDAT", "IDAT")),
             (mc.SIG + ihdr3 + idat + mc.IEND, RequiredChunk, ("PLTE", "IDAT")),
             (mc.file_of(gama), RequiredChunk, ("IDAT", "IEND"))]
    for data, kind, args in cases:
        with pytest.raises(kind) as err:
            PNG.decompress(data, session=s)
        assert err.value.args[0] == kind(*args).args[0]
    for data, status, aux in ((mc.file_of(text(b"Title\0\2\0en\0\0x"), idat), gpu.E_TEXT_COMPRESSION, 2),
                              (mc.file_of(mc.chunk(b"zTXt", b"Title\0\0" + zlib.compress(b"body" * 50)[:-6]), idat), gpu.E_TEXT_INCOMPLETE, 0),
                              (mc.file_of(mc.chunk(b"iCCP", b"name\0\0" + zlib.compress(b"body" * 50)[:-6]), idat), gpu.E_PROFILE_INCOMPLETE, 0)):
        with pytest.raises(gpu.ParsingError) as err:
            PNG.decompress(data, session=s)
        assert (err.value.status, err.value.aux[0]) == (status, aux)
    # a failure of the lexer comes behind what is wrong with the chunks in front of it
    broken = mc.file_of(gama, gama, idat)[:-5]
    with pytest.raises(DuplicateChunk):
        PNG.decompress(broken, session=s)
    with pytest.raises(gpu.LexingError):
        PNG.decompress(mc.file_of(gama, idat)[:-5], session=s)
