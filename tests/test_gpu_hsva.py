"""GPU checks of spng_hsva_batch / spng_hsva (the HSVA colour target of the reference's Snippets/PNG/CustomColor.swift) and of the mirror's
PNG.HSVA.  Expected values come from tests/hsva_ref.py, the tutorial's integer formulas in numpy with plain `//` and `%`, which
tests/test_hsva_ref.py holds against the files the reference itself wrote.  Where the reference traps (fatalError("unreachable"): a
sector above 5 with s > 0 and v > 0) the documented answer of the device is (v, v, v, a) and a count in aux[0]."""
import ctypes
import hashlib
import json
import struct

import numpy as np
import pytest

import hsva_ref
import pnghelp as ph

pytestmark = pytest.mark.gpu

FROM, TO_RGBA, TO_VA = hsva_ref.FROM_RGBA8, hsva_ref.TO_RGBA8, hsva_ref.TO_VA8
IN_BYTES, OUT_BYTES = {FROM: 4, TO_RGBA: 8, TO_VA: 8}, {FROM: 8, TO_RGBA: 4, TO_VA: 2}
TABLE = json.loads((ph.GOLDEN / "customcolor.json").read_text())
FIXTURE = ph.GOLDEN / "customcolor" / "CustomColor.png"


def run_batch(s, jobs, in_off=0, out_off=0):
    """jobs: [(op, input bytes)], each one desc of ONE spng_hsva_batch call, on slots of two device buffers that start `in_off` /
    `out_off` bytes behind a 16-byte boundary, 64 bytes apart at least; the output buffer is poisoned.  Checks status, byte counts, trap
    count, the pixels and every byte outside the outputs against hsva_ref."""
    ins, outs, ipos, opos = [], [], 0, 0
    for op, data in jobs:
        n = len(data) // IN_BYTES[op]
        ins.append((ipos + in_off, len(data)))
        outs.append((opos + out_off, n * OUT_BYTES[op]))
        ipos = (ipos + in_off + len(data) + 64 + 15) & ~15
        opos = (opos + out_off + n * OUT_BYTES[op] + 64 + 15) & ~15
    host = np.zeros(ipos + 16, dtype=np.uint8)
    want = np.full(opos + 16, 0xEE, dtype=np.uint8)
    trapped = []
    for (op, data), (ia, il), (oa, ol) in zip(jobs, ins, outs):
        host[ia:ia + il] = np.frombuffer(data, dtype=np.uint8)
        out, t = hsva_ref.convert(op, data)
        want[oa:oa + ol] = np.frombuffer(out, dtype=np.uint8)
        trapped.append(t)
    d_in, d_out = s.to_device(host), s.to_device(np.full_like(want, 0xEE))
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    _, res = s.hsva_batch([d_in[a:a + n] for a, n in ins], [op for op, _ in jobs], outs=[d_out[a:a + n] for a, n in outs])
    back = d_out.cpu().numpy()
    for r, (_, il), (_, ol), t in zip(res, ins, outs, trapped):
        assert (r.status, r.written, r.consumed, r.aux[0]) == (0, ol, il, t), (r.status, r.written, r.consumed, r.aux[0], ol, il, t)
    bad = np.flatnonzero(back != want)
    assert bad.size == 0, ([op for op, _ in jobs], in_off, out_off, bad[:8], back[bad[:8]], want[bad[:8]])
    return res


@pytest.fixture(scope="module")
def every_colour():
    """all 2^24 colours as (n, 4) uint8 -- alpha a byte derived from the index -- and their HSVA records by hsva_ref, computed once"""
    c = np.arange(1 << 24, dtype=np.uint32)
    px = np.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255, ((c * 7 + 3) >> 5) & 255], axis=1).astype(np.uint8)
    want = np.empty(1 << 24, dtype=hsva_ref.HSVA)
    for at in range(0, 1 << 24, 1 << 22):
        want[at:at + (1 << 22)] = hsva_ref.from_rgba(px[at:at + (1 << 22)])
    want.setflags(write=False)
    px.setflags(write=False)
    return px, want


def test_from_rgba8_every_colour_in_one_call(gpu, every_colour):
    """the two reciprocal divisions on the real v_rcp_f32: every (mid - min, d) and (d, max) there is"""
    s = gpu.load()
    px, want = every_colour
    d_in = s.to_device(px.reshape(-1).copy())                  # (the shared array stays read-only)
    (d_out,), (r,) = s.hsva_batch([d_in], FROM)
    assert (r.status, r.written, r.consumed, r.aux[0]) == (0, 8 << 24, 4 << 24, 0)
    got = d_out.cpu().numpy().view(hsva_ref.HSVA)
    for k in "hsva":
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (k, px[bad[:4]], got[k][bad[:4]], want[k][bad[:4]])
    assert int(got["h"].max()) == 392964 < 6 * 65537


def test_round_trip_on_the_device_every_colour(gpu):
    """TO_RGBA8(FROM_RGBA8(c)) == c for all 2^24 colours, nothing trapped; compared on the device"""
    s = gpu.load()
    torch = s.torch
    c = torch.arange(1 << 24, dtype=torch.int32, device=s.tdev)
    rgba = (c | (((c * 7 + 3) >> 5) & 255) << 24).view(torch.uint8)
    (hsva,), (r0,) = s.hsva_batch([rgba], FROM)
    (back,), (r1,) = s.hsva_batch([hsva], TO_RGBA)
    assert (r0.status, r0.aux[0], r1.status, r1.aux[0], r1.written) == (0, 0, 0, 0, 4 << 24)
    assert torch.equal(back, rgba)
    (va,), (r2,) = s.hsva_batch([hsva], TO_VA)
    assert r2.status == 0 and r2.aux[0] == 0 and r2.written == 2 << 24
    assert torch.equal(va.view(-1, 2), hsva.view(-1, 8)[:, 6:8])


def hsva_grid():
    """h in k 65537 + {0, 1, 32768, 65535, 65536}, k = 0 ... 7, and 2^32 - 1; s in eight values; every v"""
    hs = np.array([k * 65537 + o for k in range(8) for o in (0, 1, 32768, 65535, 65536)] + [2 ** 32 - 1], dtype=np.int64)
    ss = np.array([0, 1, 255, 256, 32767, 32768, 65534, 65535], dtype=np.int64)
    h, sv, v = np.meshgrid(hs, ss, np.arange(256), indexing="ij")
    p = np.zeros(h.size, dtype=hsva_ref.HSVA)
    p["h"], p["s"], p["v"] = h.reshape(-1), sv.reshape(-1), v.reshape(-1)
    p["a"] = (np.arange(h.size) * 11) & 255
    return p


def test_to_rgba8_and_to_va8_on_the_grid(gpu):
    s = gpu.load()
    p = hsva_grid()
    assert p.size == 41 * 8 * 256
    res = run_batch(s, [(TO_RGBA, p.tobytes()), (TO_VA, p.tobytes())])
    # sectors 6 and 7 and 2^32 - 1 with s > 0 and v > 0: (2 * 5 + 1) h, 7 s, 255 v
    assert res[0].aux[0] == 11 * 7 * 255 and res[1].aux[0] == 0


def test_to_rgba8_and_to_va8_on_random_draws(gpu):
    """2^20 pixels with h below 6 * 65537 (a uniformly random 32-bit h traps 99.6 % of the time) and 2^16 with h over all 32 bits"""
    s = gpu.load()
    rng = np.random.default_rng(20)
    valid, wide = np.zeros(1 << 20, dtype=hsva_ref.HSVA), np.zeros(1 << 16, dtype=hsva_ref.HSVA)
    for p, top in ((valid, 6 * 65537), (wide, 1 << 32)):
        p["h"], p["s"] = rng.integers(0, top, p.size), rng.integers(0, 65536, p.size)
        p["v"], p["a"] = rng.integers(0, 256, p.size), rng.integers(0, 256, p.size)
    res = run_batch(s, [(TO_RGBA, valid.tobytes()), (TO_RGBA, wide.tobytes()), (TO_VA, valid.tobytes()), (TO_VA, wide.tobytes())])
    assert res[0].aux[0] == 0 and res[1].aux[0] > 60000


COUNTS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 1025, 4 * 64 * 256 + 7]


def random_input(op, n, rng):
    if op == FROM:
        return rng.integers(0, 256, 4 * n, dtype=np.uint8).tobytes()
    p = np.zeros(n, dtype=hsva_ref.HSVA)
    p["h"], p["s"] = rng.integers(0, 6 * 65537, n), rng.integers(0, 65536, n)
    p["v"], p["a"] = rng.integers(0, 256, n), rng.integers(0, 256, n)
    p["h"][::37] = rng.integers(6 * 65537, 1 << 32, len(p["h"][::37]))          # (some that trap)
    return p.tobytes()


@pytest.mark.parametrize("op", [FROM, TO_RGBA, TO_VA])
def test_shapes_and_offsets(gpu, op):
    """pixel counts around the 16-byte access, the wave and the block, in one call each: on 16-byte boundaries; inputs 4 and outputs 8
    bytes behind one (pixel by pixel); and the RGBA8 / VA8 side at an odd byte offset"""
    s = gpu.load()
    rng = np.random.default_rng(op)
    jobs = [(op, random_input(op, n, rng)) for n in COUNTS]
    run_batch(s, jobs)
    run_batch(s, jobs, in_off=4, out_off=8)
    if op == FROM:
        run_batch(s, jobs, in_off=3, out_off=0)
        run_batch(s, jobs, in_off=1, out_off=4)
    else:
        run_batch(s, jobs, in_off=0, out_off=1)
        run_batch(s, jobs, in_off=12, out_off=7)


def test_a_mixed_batch(gpu):
    """the three operations and several lengths, empty ones among them, in one call: each result equals its array alone"""
    s = gpu.load()
    rng = np.random.default_rng(7)
    jobs = [(op, random_input(op, n, rng)) for op, n in ((TO_VA, 4099), (FROM, 0), (TO_RGBA, 70001), (FROM, 1030), (TO_VA, 0), (TO_RGBA, 2),
                                                          (FROM, 65537), (TO_RGBA, 0), (TO_VA, 8), (TO_VA, 7))]
    run_batch(s, jobs)
    for op, data in jobs:
        assert s.hsva(data, op) == hsva_ref.convert(op, data)
    assert s.hsva_batch([], FROM) == ([], [])
    assert s.lib.spng_hsva_batch(s.ctx, None, 0, None, None) == 0


def test_a_large_batch_crosses_the_grid_limit(gpu):
    """70 000 one-pixel jobs, the three operations in turn"""
    s = gpu.load()
    n = 70000
    rng = np.random.default_rng(70)
    p = np.zeros(n, dtype=hsva_ref.HSVA)
    p["h"], p["s"] = rng.integers(0, 7 * 65537, n), rng.integers(0, 65536, n)
    p["v"], p["a"] = rng.integers(0, 256, n), rng.integers(0, 256, n)
    raw = p.view(np.uint8).reshape(n, 8)
    ops = np.arange(n) % 3 + 1
    want = np.full((n, 8), 0xEE, dtype=np.uint8)
    want[ops == FROM] = np.frombuffer(hsva_ref.from_rgba(raw[ops == FROM, :4]).tobytes(), dtype=np.uint8).reshape(-1, 8)
    rgba, trap = hsva_ref.to_rgba(p[ops == TO_RGBA])
    want[ops == TO_RGBA, :4] = rgba
    want[ops == TO_VA, :2] = hsva_ref.to_va(p[ops == TO_VA])
    traps = np.zeros(n, dtype=np.int64)
    traps[ops == TO_RGBA] = trap
    assert 2000 < traps.sum() < 6000
    d_in, d_out = s.to_device(raw.reshape(-1)), s.to_device(np.full(8 * n, 0xEE, dtype=np.uint8))
    descs = (gpu.HsvaDesc * n)()
    a, b = d_in.data_ptr(), d_out.data_ptr()
    for i in range(n):
        descs[i] = gpu.HsvaDesc(a + 8 * i, b + 8 * i, 1, int(ops[i]))
    res = (gpu.Result * n)()
    assert s.lib.spng_hsva_batch(s.ctx, descs, n, None, res) == 0
    assert (d_out.cpu().numpy().reshape(n, 8) == want).all()
    got = np.array([(r.status, r.written, r.aux[0]) for r in res])
    assert (got[:, 0] == 0).all() and (got[:, 1] == np.array([0, 8, 4, 2])[ops]).all() and (got[:, 2] == traps).all()


def test_refusals(gpu):
    """SPNG_E_ARGUMENT: a non-zero reserved byte, an unknown op, d_out == d_in, ranges that overlap, an HSVA pointer not aligned to 4;
    the RGBA8 / VA8 side may have any alignment"""
    s = gpu.load()
    buf = s.empty(8192)
    base = buf.data_ptr()
    assert base % 16 == 0

    def call(*descs):
        arr = (gpu.HsvaDesc * len(descs))(*descs)
        res = (gpu.Result * len(descs))()
        return s.lib.spng_hsva_batch(s.ctx, arr, len(descs), None, res)

    def desc(d_in=base, d_out=base + 4096, count=16, op=FROM, reserved=None):
        d = gpu.HsvaDesc(d_in, d_out, count, op)
        if reserved is not None:
            d.reserved[reserved] = 1
        return d

    E = gpu.E_ARGUMENT
    assert call(desc()) == 0 and call(desc(op=TO_RGBA)) == 0 and call(desc(op=TO_VA)) == 0
    assert call(desc(count=0, d_in=None, d_out=None)) == 0
    assert call(desc(op=0)) == E and call(desc(op=4)) == E and call(desc(op=255)) == E
    for k in range(7):
        assert call(desc(reserved=k)) == E
    assert call(desc(d_out=base)) == E and call(desc(d_out=base, op=TO_RGBA)) == E and call(desc(d_out=base, op=TO_VA, count=0)) == E
    assert call(desc(d_out=base + 60)) == E and call(desc(d_out=base + 64)) == 0                     # (16 RGBA8 pixels are 64 bytes)
    assert call(desc(d_in=base + 4096 + 124, d_out=base + 4096)) == E and call(desc(d_in=base + 4096 + 128, d_out=base + 4096)) == 0
    # the HSVA side: the output of FROM_RGBA8, the input of the others
    assert call(desc(d_out=base + 4096 + 2)) == E and call(desc(d_out=base + 4096 + 1)) == E and call(desc(d_out=base + 4096 + 4)) == 0
    assert call(desc(d_in=base + 2, op=TO_RGBA)) == E and call(desc(d_in=base + 3, op=TO_VA)) == E and call(desc(d_in=base + 4, op=TO_VA)) == 0
    # the other side: anything
    assert call(desc(d_in=base + 1)) == 0 and call(desc(d_out=base + 4096 + 3, op=TO_RGBA)) == 0 and call(desc(d_out=base + 4096 + 1, op=TO_VA)) == 0
    assert call(desc(d_in=None)) == E and call(desc(d_out=None)) == E
    assert call(desc(), desc(op=9)) == E and call(desc(), desc(op=TO_VA)) == 0
    arr = (gpu.HsvaDesc * 1)(desc())
    assert s.lib.spng_hsva_batch(s.ctx, arr, 1, None, None) == E                      # nowhere to put the results
    assert s.lib.spng_hsva_batch(s.ctx, None, 0, None, None) == 0 and s.lib.spng_hsva_batch(None, arr, 1, None, (gpu.Result * 1)()) == E
    quiet = s.to_device(bytes([0xEE]) * 128)                      # a valid desc in front of a spoiled one: nothing is enqueued
    for spoiled in (desc(op=0), desc(reserved=3), desc(d_out=base), desc(d_out=base + 4096 + 2), desc(d_in=None)):
        assert call(desc(d_out=quiet.data_ptr()), spoiled) == E
    res = gpu.Result()
    assert s.lib.spng_hsva(s.ctx, None, 4, FROM, None, ctypes.byref(res)) == E and s.lib.spng_hsva(s.ctx, None, 0, 7, None, ctypes.byref(res)) == E
    s.sync()
    assert (quiet.cpu().numpy() == 0xEE).all()


def test_the_custom_colour_tutorial_on_the_device(gpu):
    """Snippets/PNG/CustomColor.swift from the committed input: lex, decode, unpack(as: RGBA<UInt8>), HSVA.init(r:g:b:a:), the four
    field edits of :316-341 with torch on the device tensor, .rgba, pack as rgb8 -- the storage is the raster of the file the reference
    wrote, for all four; one of them goes on through spng_encode_batch and decodes again to the same raster"""
    s = gpu.load()
    torch = s.torch
    data = FIXTURE.read_bytes()
    d_png, d_idat = s.to_device(data), s.empty(len(data))
    infos = (gpu.Lexed * 1)()
    files = (gpu.FileDesc * 1)(gpu.FileDesc(s._ptr(d_png), len(data), s._ptr(d_idat), len(data)))
    assert s.lib.spng_lex_batch(s.ctx, files, 1, None, infos) == 0
    r = infos[0]
    assert (r.status, r.width, r.height, r.depth, r.color, r.interlace) == (0, 400, 588, 8, 2, 0)
    w, h, n = r.width, r.height, r.width * r.height
    u = gpu.inflated_size(w, h, 8, 3, False)
    d_rows, d_storage = s.empty(u), s.empty(3 * n)
    res = s.decode_batch([s.image_desc(d_idat[:r.idat_len], d_rows, d_storage, w, h, 8, 3, False)])
    assert res[0].status == 0
    d_rgba = s.empty(4 * n)
    und = (gpu.UnpackDesc * 1)(gpu.UnpackDesc(s._ptr(d_storage), s._ptr(d_rgba), None, w, h, 0, (ctypes.c_uint16 * 3)(0, 0, 0), 8, 3, 0, 0, 0,
                                              8, gpu.TARGET_RGBA, 0))
    assert s.lib.spng_unpack_batch(s.ctx, und, 1) == 0
    (d_hsva,), (r0,) = s.hsva_batch([d_rgba], FROM)
    assert r0.status == 0 and r0.written == 8 * n
    f = d_hsva.view(torch.int32).view(n, 2)                     # h | s, v << 16, a << 24
    A, V = -(1 << 24), 255 << 16                                # (the alpha byte as a signed mask; v = .max)
    hue, sat, val = f.clone(), f.clone(), f.clone()
    hue[:, 1] = (f[:, 1] & A) | V | (65535 // 2)                # (h: $0.h, s: .max / 2, v: .max, a: $0.a)
    sat[:, 0] = 370000
    sat[:, 1] = (f[:, 1] & (A | 0xffff)) | V                    # (h: 370000, s: $0.s, v: .max, a: $0.a)
    val[:, 0] = 0
    val[:, 1] = f[:, 1] & ~0xffff                               # (h: 0, s: 0, v: $0.v, a: $0.a)
    edits = {"CustomColor-hue.png": hue, "CustomColor-saturation.png": sat, "CustomColor-value.png": val, "CustomColor.png.png": f}
    outs, rs = s.hsva_batch([e.view(torch.uint8).view(-1) for e in edits.values()], TO_RGBA)
    assert all((x.status, x.written, x.aux[0]) == (0, 4 * n, 0) for x in rs)
    stores = [s.empty(3 * n) for _ in outs]
    pds = (gpu.PackDesc * 4)(*[gpu.PackDesc(s._ptr(o), s._ptr(t), None, w, h, 0, 8, 3, 0, 0, 8, gpu.TARGET_RGBA, 0) for o, t in zip(outs, stores)])
    assert s.lib.spng_pack_batch(s.ctx, pds, 4) == 0
    s.sync()
    for name, t in zip(edits, stores):
        assert hashlib.sha256(t[:3 * n].cpu().numpy().tobytes()).hexdigest() == TABLE[name]["sha256"], name
    # the hue image as a file's stream and back
    cap = s.lib.spng_deflate_bound(u)
    d_out = s.empty(cap)
    d = s.image_desc(d_out, d_rows, stores[0], w, h, 8, 3, False, 0, rows_cap=u)
    d.idat_len = cap
    eres = (gpu.Result * 1)()
    assert s.lib.spng_encode_batch(s.ctx, (gpu.ImageDesc * 1)(d), 6, 1, None, eres) == 0 and eres[0].status == 0
    d_back = s.empty(3 * n)
    res = s.decode_batch([s.image_desc(d_out[:eres[0].written].contiguous(), s.empty(u), d_back, w, h, 8, 3, False)])
    assert res[0].status == 0 and torch.equal(d_back[:3 * n], stores[0][:3 * n])


def _palette_quads(png):
    pal = np.frombuffer(png.palette, dtype=np.uint8).reshape(-1, 3)
    quads = np.full((len(pal), 4), 255, dtype=np.uint8)
    quads[:, :3] = pal
    if png.trns:
        t = np.frombuffer(png.trns, dtype=np.uint8)[:len(pal)]
        quads[:len(t), 3] = t
    return quads.tobytes()


# a grey, a keyed grey, a keyed colour, an indexed (with tRNS), two 16-bit, a bgr and a bgra fixture; True: pack(unpack(x)) is x
MIRROR_CASES = [("common/basn0g08.png", True), ("common/tbbn0g04.png", True), ("common/tbrn2c08.png", True), ("common/tbbn3p08.png", False),
                ("common/basn6a16.png", False), ("common/basn4a16.png", False), ("ios/basn2c08.png", True), ("ios/basn6a08.png", True)]


@pytest.mark.parametrize("name,lossless", MIRROR_CASES)
def test_mirror_unpack_and_pack(gpu, name, lossless):
    """PNG.HSVA.unpack == hsva_ref.from_rgba of the existing RGBA<UInt8> unpack -- and, for the grey formats, the tutorial's own
    (h: 0, s: 0, v, a) of the existing VA<UInt8> unpack --; PNG.HSVA.pack(unpack(x)) == the routing restated: (v, a) through the VA<UInt8>
    pack for grey formats, .rgba through the RGBA<UInt8> pack (default indexer) for the others"""
    s = gpu.load()
    png = ph.parse_png((ph.GOLDEN / "pngsuite" / name).read_bytes())
    st, storage, _ = s.decode(png.idat, png.width, png.height, png.depth, png.channels, png.interlaced, png.fmt)
    assert st == 0
    key = ph.format_key(png)                                        # (a CgBI file's tRNS reversed: the bgr8 format's key is (b, g, r))
    indexed, bgr = png.color == 3, png.ios and png.color in (2, 6)
    fmt = (png.width, png.height, png.depth, png.channels)
    kw = dict(indexed=indexed, bgr=bgr, palette=_palette_quads(png) if indexed else None)
    got = gpu.PNG.HSVA.unpack(storage, *fmt, key=key, **kw)
    rgba8 = np.frombuffer(s.unpack(storage, *fmt, target=8, key=key, **kw), dtype=np.uint8).reshape(-1, 4)
    want = hsva_ref.from_rgba(rgba8)
    assert got == want.tobytes()
    rec = np.frombuffer(got, dtype=hsva_ref.HSVA)
    grey = png.color in (0, 4)
    if grey:
        va8 = np.frombuffer(s.unpack(storage, *fmt, target=8, key=key, layout=gpu.TARGET_VA, **kw), dtype=np.uint8).reshape(-1, 2)
        assert not rec["h"].any() and not rec["s"].any() and (rec["v"] == va8[:, 0]).all() and (rec["a"] == va8[:, 1]).all()
        if key is not None:
            assert 0 < (rec["a"] == 0).sum() < rec.size
        routed = s.pack(hsva_ref.to_va(want).tobytes(), *fmt, source=8, layout=gpu.TARGET_VA)
    else:
        assert rec["s"].any()
        routed = s.pack(hsva_ref.to_rgba(want)[0].tobytes(), *fmt, source=8, **kw)
    packed = gpu.PNG.HSVA.pack(got, *fmt, **kw)
    assert packed == routed
    if lossless:
        assert packed == storage
    # the numpy spellings of the mirror
    some = rgba8[:1000]
    h = gpu.PNG.HSVA.from_rgba(some)
    assert h.dtype == gpu.PNG.HSVA.dtype() == hsva_ref.HSVA and (h == want[:1000]).all()
    assert (gpu.PNG.HSVA.rgba(h) == some).all() and (gpu.PNG.HSVA.va(h) == hsva_ref.to_va(h)).all()


def test_mirror_rgba_raises_where_the_reference_traps(gpu):
    p = np.array([(6 * 65537, 1, 200, 9), (5, 0, 5, 5)], dtype=hsva_ref.HSVA)
    with pytest.raises(ValueError):
        gpu.PNG.HSVA.rgba(p)
    with pytest.raises(ValueError):
        gpu.PNG.HSVA.pack(p.tobytes(), 2, 1, 8, 3)
    assert gpu.PNG.HSVA.pack(p.tobytes(), 2, 1, 8, 1) == bytes([200, 5])             # (grey formats never look at h)
    assert gpu.PNG.HSVA.rgba(p[1:]).tolist() == [[5, 5, 5, 5]]
