"""GPU: the typed chunks (spng_parse_dir_batch) and PNG.decompress(typed=True).  The case table of tests/parse_cases.py and the golden
files through the C ABI against tests/parse_ref.py -- every case in a call of its own, all of them in one call beside the golden files
with mixed caps --, both forms of the call directly behind spng_lex_dir_batch with nothing waiting in between, the records behind
min(chunks, cap) untouched, a batch that splits its launch at 65 535 files, and the host mirror's typed path against what the reference
throws and writes."""
import ctypes
import hashlib
import json
import struct
import zlib

import numpy as np
import pytest

import metadata_cases as mc
import parse_cases as pc
import parse_ref as pr
import pnghelp as ph
from lex_ref import lex_ref
from test_gpu_grid_rows import dtype_of, table

pytestmark = pytest.mark.gpu
CASES = pc.cases()
FILES = json.loads((ph.GOLDEN / "files.json").read_text())
META = ph.GOLDEN / "metadata"
FILL = 0xEE


def value_of(v):
    return pr.Value(v.status, v.scope, tuple(v.aux), v.count, v.k, tuple(v.v))


def parsed_of(p):
    return pr.Parsed(p.status, p.index, tuple(p.aux), p.ihdr_index, p.plte_index, p.palette_count, p.depth, p.color, p.ios, p.interlaced)


def want_of(data, cap):
    info, _ = lex_ref(data, len(data))
    return pr.parse_file(pr.chunks_of(data, min(info.chunks, cap)))


def lex_and_parse(gpu, s, files, caps, host_form):
    """spng_lex_dir_batch with its infos left on the device, and directly behind it -- no wait in between -- spng_parse_dir_batch: with
    h_parsed (host_form), or with d_parsed alone, fully asynchronous.  Two records of room behind every file's `cap`, filled with a
    pattern.  -> ([[Value]], [Parsed]); the records behind min(chunks, cap) are seen to be untouched"""
    n = len(files)
    vsz, esz = ctypes.sizeof(gpu.ChunkValue), ctypes.sizeof(gpu.ChunkEntry)
    assert (vsz, ctypes.sizeof(gpu.Parsed)) == (64, 40)
    lens = np.array([len(f) for f in files], dtype=np.int64)
    at = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)])
    blob = np.full(int(at[-1]) + 16, FILL, dtype=np.uint8)
    for f, a in zip(files, at):
        blob[a:a + len(f)] = np.frombuffer(f, dtype=np.uint8)
    d_png, d_idat = s.to_device(blob), s.empty(int(at[-1]) + 16)
    caps = np.array(caps, dtype=np.int64)
    rec_at = np.concatenate([[0], np.cumsum(caps + 2)])
    d_ent = s.to_device(np.full(int(rec_at[-1]) * esz, FILL, dtype=np.uint8))
    d_val = s.to_device(np.full(int(rec_at[-1]) * vsz, FILL, dtype=np.uint8))
    d_infos = s.to_device(np.zeros(n * ctypes.sizeof(gpu.Lexed), dtype=np.uint8))
    d_parsed = s.to_device(np.full(n * ctypes.sizeof(gpu.Parsed), FILL, dtype=np.uint8))
    descs, _ = table(gpu.FileDesc, n, d_png=d_png.data_ptr() + at[:-1], len=lens, d_idat=d_idat.data_ptr() + at[:-1], idat_cap=lens)
    dirs, _ = table(gpu.ChunkDir, n, d_entries=np.where(caps > 0, d_ent.data_ptr() + esz * rec_at[:-1], 0), cap=caps)
    vals = (ctypes.c_void_p * n).from_buffer(np.where(caps > 0, d_val.data_ptr() + vsz * rec_at[:-1], 0).astype(np.uint64))
    h_parsed = (gpu.Parsed * n)()
    assert s.lib.spng_lex_dir_batch(s.ctx, descs, dirs, n, d_infos.data_ptr(), None) == 0
    if host_form:
        assert s.lib.spng_parse_dir_batch(s.ctx, descs, dirs, d_infos.data_ptr(), vals, n, None, h_parsed) == 0
    else:
        assert s.lib.spng_parse_dir_batch(s.ctx, descs, dirs, d_infos.data_ptr(), vals, n, d_parsed.data_ptr(), None) == 0
        s.sync()
        h_parsed = (gpu.Parsed * n).from_buffer_copy(d_parsed.cpu().numpy().tobytes())
    infos = np.frombuffer(d_infos.cpu().numpy().tobytes(), dtype=dtype_of(gpu.Lexed))
    raw = d_val.cpu().numpy()
    filled = np.minimum(infos["chunks"].astype(np.int64), caps)
    keep = np.ones(len(raw), dtype=bool)
    for j in range(n):
        keep[vsz * rec_at[j]:vsz * (rec_at[j] + filled[j])] = False
    assert (raw[keep] == FILL).all()                             # behind min(chunks, cap), and in a file without room: untouched
    values = [[value_of(v) for v in (gpu.ChunkValue * int(filled[j])).from_buffer_copy(raw[vsz * rec_at[j]:vsz * (rec_at[j] + filled[j])].tobytes())]
              for j in range(n)]
    return values, [parsed_of(p) for p in h_parsed]


def caps_of(cases):
    return [len(c.file) // 12 if c.cap is None else c.cap for c in cases]


def test_every_case_alone(gpu):
    s = gpu.load()
    for c, cap in zip(CASES, caps_of(CASES)):
        (values,), (parsed,) = lex_and_parse(gpu, s, [c.file], [cap], host_form=True)
        assert (values, parsed) == want_of(c.file, cap), c.name
        assert (None if parsed.status == pr.DONE else (parsed.index, parsed.status, parsed.aux)) == c.expect, c.name
        if c.scopes is not None:
            assert tuple(v.scope for v in values) == tuple(c.scopes), c.name


@pytest.mark.parametrize("host_form", [True, False], ids=["h_parsed", "asynchronous"])
def test_table_and_golden_files_in_one_call(gpu, host_form):
    """the whole table beside the golden files, every third of which has a directory of two entries; both forms of the call"""
    s = gpu.load()
    golden = [p.read_bytes() for p in pc.golden_files()]
    files = [c.file for c in CASES] + golden
    caps = caps_of(CASES) + [2 if k % 3 == 2 else len(f) // 12 for k, f in enumerate(golden)]
    values, parsed = lex_and_parse(gpu, s, files, caps, host_form)
    for k, (f, cap) in enumerate(zip(files, caps)):
        assert (values[k], parsed[k]) == want_of(f, cap), k
    assert all(p.status == pr.DONE for p in parsed[len(CASES):])


def test_a_batch_that_splits_its_launch(gpu):
    """65 537 minimal files, the last with a bad tIME: the launch is split at 65 535 rows, and both halves are seen to write"""
    s = gpu.load()
    N = 65537
    minimal = mc.SIG + pc.ihdr(8, 0, x=1, y=1) + mc.chunk(b"IDAT", zlib.compress(b"\0\0", 9)) + mc.IEND
    assert len(minimal) == 67
    last = minimal[:-12] + mc.chunk(b"tIME", pc.time_of(second=61)[0]) + mc.IEND
    at = 67 * np.arange(N + 1, dtype=np.int64)
    at[N] += 19
    d_png = s.to_device(minimal * (N - 1) + last)
    d_idat = s.empty(int(at[-1]))
    vsz, esz = ctypes.sizeof(gpu.ChunkValue), ctypes.sizeof(gpu.ChunkEntry)
    d_ent, d_val = s.empty(N * 4 * esz), s.to_device(np.full(N * 4 * vsz, FILL, dtype=np.uint8))
    d_infos = s.empty(N * ctypes.sizeof(gpu.Lexed))
    descs, _ = table(gpu.FileDesc, N, d_png=d_png.data_ptr() + at[:-1], len=np.diff(at), d_idat=d_idat.data_ptr() + at[:-1], idat_cap=np.diff(at))
    dirs, _ = table(gpu.ChunkDir, N, d_entries=d_ent.data_ptr() + 4 * esz * np.arange(N), cap=4)
    vals = (ctypes.c_void_p * N).from_buffer((d_val.data_ptr() + 4 * vsz * np.arange(N)).astype(np.uint64))
    parsed = (gpu.Parsed * N)()
    assert s.lib.spng_lex_dir_batch(s.ctx, descs, dirs, N, d_infos.data_ptr(), None) == 0
    assert s.lib.spng_parse_dir_batch(s.ctx, descs, dirs, d_infos.data_ptr(), vals, N, None, parsed) == 0
    got = np.frombuffer(parsed, dtype=dtype_of(gpu.Parsed))
    assert (got["status"][:-1] == 0).all() and (got["index"][:-1] == pr.NONE).all() and (got["ihdr_index"] == 0).all() and (got["depth"] == 8).all()
    want_values, want_parsed = want_of(last, 4)
    assert parsed_of(parsed[N - 1]) == want_parsed and want_parsed.status == pr.E_TIME and want_parsed.index == 2
    raw = d_val.cpu().numpy().reshape(N, 4 * vsz)
    one = np.frombuffer(b"".join(bytes(gpu.ChunkValue(v.status, v.scope, v.aux, v.count, v.k, v.v)) for v in want_of(minimal, 4)[0]) + bytes([FILL]) * vsz,
                        dtype=np.uint8)
    assert (raw[:-1] == one).all()                               # files 0 ... 65534 are the first launch's, 65535 the second's
    assert [value_of(v) for v in (gpu.ChunkValue * 4).from_buffer_copy(raw[-1].tobytes())] == want_values


def test_refuses_null_arrays(gpu):
    s = gpu.load()
    lib = s.lib
    f = pc.png(pc.ihdr(8, 0))
    d_png, d_ent, d_val, d_infos = s.to_device(f), s.empty(512), s.empty(512), s.empty(ctypes.sizeof(gpu.Lexed))
    descs = (gpu.FileDesc * 1)(gpu.FileDesc(d_png.data_ptr(), len(f), None, 0))
    dirs = (gpu.ChunkDir * 1)(gpu.ChunkDir(d_ent.data_ptr(), 2, 0))
    vals = (ctypes.c_void_p * 1)(d_val.data_ptr())
    parsed = (gpu.Parsed * 1)()
    assert lib.spng_lex_dir_batch(s.ctx, descs, dirs, 1, d_infos.data_ptr(), None) == 0
    di = d_infos.data_ptr()
    assert lib.spng_parse_dir_batch(s.ctx, descs, dirs, di, vals, 1, None, parsed) == 0 and parsed[0].status == 0
    for args in ((None, dirs, di, vals, 1, None, parsed), (descs, None, di, vals, 1, None, parsed), (descs, dirs, None, vals, 1, None, parsed),
                 (descs, dirs, di, None, 1, None, parsed), (descs, dirs, di, vals, 1, None, None),
                 (descs, dirs, di, (ctypes.c_void_p * 1)(None), 1, None, parsed),                       # room in the directory, none for its records
                 (descs, (gpu.ChunkDir * 1)(gpu.ChunkDir(None, 2, 0)), di, vals, 1, None, parsed),
                 (descs, (gpu.ChunkDir * 1)(gpu.ChunkDir(d_ent.data_ptr(), 2, 1)), di, vals, 1, None, parsed)):
        assert lib.spng_parse_dir_batch(s.ctx, *args) == gpu.E_ARGUMENT
    assert lib.spng_parse_dir_batch(s.ctx, None, None, None, None, 0, None, None) == 0
    assert gpu.load_library().spng_status_string(gpu.E_PARSE_TIME) == b"invalid time"
    assert gpu.load_library().spng_status_string(gpu.E_PARSE_HEADER_PIXEL_FORMAT_CODE) == b"invalid flag code"


def test_session_parse_dir_batch(gpu):
    """the binding's own form, behind lex_dir_batch's pieces"""
    s = gpu.load()
    files = [c.file for c in CASES[:40]]
    infos, entries, values, parsed, _, _ = s.lex_parse_batch(files)
    for f, vs, p in zip(files, values, parsed):
        assert ([value_of(v) for v in vs], parsed_of(p)) == want_of(f, len(f) // 12)


# ---- PNG.decompress(typed=True) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,code", [("xc1n0g08", (8, 1)), ("xc9n2c08", (8, 9)), ("xd0n2c08", (0, 2)), ("xd3n2c08", (3, 2)), ("xd9n2c08", (99, 2))])
def test_typed_decompress_raises_the_header_error(gpu, name, code):
    """Sources/PNGIntegrationTests/ErrorHandling.swift:47-63"""
    from swift_png_amd.mirror import PNG
    with pytest.raises(gpu.ParsingError) as err:
        PNG.decompress((ph.GOLDEN / "invalid" / f"{name}.png").read_bytes(), typed=True, session=gpu.load())
    assert (err.value.status, err.value.aux) == (gpu.E_PARSE_HEADER_PIXEL_FORMAT_CODE, code)


def test_typed_decompress_validates_plte_trns_bkgd(gpu):
    from swift_png_amd.mirror import PNG, RequiredChunk, UnexpectedChunk
    s = gpu.load()
    idat = mc.chunk(b"IDAT", zlib.compress((b"\0" + bytes(32)) * 32))
    gama, plte = mc.chunk(b"gAMA", struct.pack(">I", 45455)), mc.chunk(b"PLTE", bytes(6))
    grey = mc.file_of(plte, gama, idat)
    with pytest.raises(gpu.ParsingError) as err:                 # PNG.Image.swift:355 throws at the PLTE, in front of the gAMA behind it
        PNG.decompress(grey, typed=True, session=s)
    assert (err.value.status, err.value.aux) == (gpu.E_PARSE_UNEXPECTED_PALETTE, (8, 0))
    with pytest.raises(UnexpectedChunk) as order:                # the default is what it was
        PNG.decompress(grey, session=s)
    assert order.value.args[0] == UnexpectedChunk("gAMA", "PLTE").args[0]
    i8 = pc.ihdr(8, 3)
    for chunks, status, aux in (((plte, mc.chunk(b"tRNS", bytes(3))), gpu.E_PARSE_TRANSPARENCY_COUNT, (3, 2)),
                                ((plte, mc.chunk(b"bKGD", b"\2")), gpu.E_PARSE_BACKGROUND_INDEX, (2, 1)),
                                ((mc.chunk(b"PLTE", bytes(5)),), gpu.E_PARSE_PALETTE_CHUNK_LENGTH, (5, 0)),
                                ((mc.chunk(b"sRGB", b"\4"), plte), gpu.E_PARSE_RENDERING_CODE, (4, 0))):
        with pytest.raises(gpu.ParsingError) as err:
            PNG.decompress(pc.png(i8, *chunks, idat), typed=True, session=s)
        assert (err.value.status, err.value.aux) == (status, aux)
        PNG.decompress(pc.png(i8, *chunks, idat), session=s)     # (untyped: they come back as an image)
    with pytest.raises(gpu.ParsingError) as err:
        PNG.decompress(pc.png(pc.ihdr(8, 2), mc.chunk(b"tRNS", pc.be16(1, 256, 2)), idat), typed=True, session=s)
    assert (err.value.status, err.value.aux) == (gpu.E_PARSE_TRANSPARENCY_SAMPLE, (256, 255))
    with pytest.raises(RequiredChunk) as need:                   # PNG.Transparency.swift:165-169
        PNG.decompress(pc.png(i8, mc.chunk(b"tRNS", b"\0"), plte, idat), typed=True, session=s)
    assert need.value.args[0] == RequiredChunk("PLTE", "tRNS").args[0]
    # the order rules come first: a second gAMA is a duplicate whatever its length
    from swift_png_amd.mirror import DuplicateChunk
    with pytest.raises(DuplicateChunk):
        PNG.decompress(mc.file_of(gama, mc.chunk(b"gAMA", bytes(3)), idat), typed=True, session=s)
    ok = PNG.decompress(pc.png(i8, plte, mc.chunk(b"tRNS", b"\7"), mc.chunk(b"bKGD", b"\1"), idat), typed=True, session=s)
    assert ok.palette == [(0, 0, 0, 7), (0, 0, 0, 255)] and ok.fill == 1 and ok.key is None


def test_typed_image_metadata_tutorial(gpu):
    """ImageMetadata.png typed, the time set, compressed at level 9: byte for byte the reference's ImageMetadata-newtime.png"""
    from swift_png_amd.mirror import PNG
    s = gpu.load()
    image = PNG.decompress((META / "ImageMetadata.png").read_bytes(), typed=True, session=s)
    m = image.metadata
    assert m.time == (2024, 1, 30, 22, 1, 56) and m.gamma == 45455 and m.physicalDimensions == (2835, 2835, 1) and image.fill == (255, 255, 255)
    m.time = (1992, 8, 3, 0, 0, 0)
    entry = FILES["files"]["ImageMetadata-newtime.png"]
    out = PNG.compress(image.storage, image.size, image.depth, image.channels, level=9, chunk_bytes=entry["chunk_bytes"], metadata=m, session=s,
                       **image.format())
    assert len(out) == entry["len"] and hashlib.sha256(out).hexdigest() == entry["sha256"]


@pytest.mark.parametrize("name", ["ch1n3p04", "ps1n2c16", "ccwn2c08", "cs5n3p08"])
def test_typed_fields_write_back_their_payloads(gpu, name):
    """hIST and sBIT (ch1n3p04), sPLT (ps1n2c16), cHRM (ccwn2c08): typed and serialised again they are their own payloads, and what the
    untyped decompress carries"""
    from swift_png_amd.mirror import PNG
    s = gpu.load()
    data = (ph.GOLDEN / "pngsuite" / "common" / f"{name}.png").read_bytes()
    typed, plain = PNG.decompress(data, typed=True, session=s), PNG.decompress(data, session=s)
    assert typed.metadata.chunks([]) == plain.metadata.chunks([])
    assert (typed.palette, typed.key, typed.fill, typed.storage) == (plain.palette, plain.key, plain.fill, plain.storage)
    info, _ = lex_ref(data, len(data))
    own = [(k, p) for k, p in pr.chunks_of(data, info.chunks) if k in (b"cHRM", b"sBIT", b"hIST", b"sPLT")]
    before, after = typed.metadata.chunks([])
    assert own and sorted(own) == sorted((k, p) for k, p in before + after if k in (b"cHRM", b"sBIT", b"hIST", b"sPLT"))
    m = typed.metadata
    if name == "ch1n3p04":
        assert m.significantBits == (4, 4, 4) and isinstance(m.histogram, list) and len(m.histogram) == len(typed.palette) == 15
    if name == "ps1n2c16":
        (palette,) = m.suggestedPalettes
        assert palette[0] == "six-cube" and palette[1] == 8 and len(palette[2]) == 216 and len(palette[2][0]) == 5
    if name == "ccwn2c08":
        assert isinstance(m.chromaticity, tuple) and len(m.chromaticity) == 8
