"""GPU parity of spng_census_wide_batch / spng_map_batch (csrc/colour_tables.hip: colour tables without the ceiling of 65 536 keys and
of one byte per result) over the case table of tests/colour_table_cases.py, against tests/indexing_ref.py (np.unique) for the census
and a gather through np.searchsorted for the map; against the old entries where both accept the input; the refusals one by one; and the
reference's CustomColor tutorial (97 388 colours) as a table -- the picture hsva.hip had to be written by hand for."""
import ctypes
import functools
import subprocess
import sys

import numpy as np
import pytest

import colour_table_cases as ct
import hsva_ref
import indexing_ref as ref
import pnghelp as ph
import tutorial_ref

pytestmark = pytest.mark.gpu

RGBA, VA, SCALAR = 0, 1, 2
CENSUS = [c for c in ct.CASES if c.kind == "census"]
MAPS = [c for c in ct.CASES if c.kind == "map"]
GUARD = 8                                                         # entries behind the room of every output, which stay 0xFF


@functools.lru_cache(maxsize=None)
def census_input(name):
    """(pixels, keys, counts) of a census case: built and counted once, shared, never written"""
    c = ct.BY_NAME[name]
    px = c.build()
    k, n = ref.census(px, c.bits, c.layout, c.premultiply)
    for a in (px, k, n):
        a.setflags(write=False)
    return px, k, n


@functools.lru_cache(maxsize=None)
def map_input(name):
    """(pixels, keys, values, wanted values per pixel, misses) of a map case"""
    c = ct.BY_NAME[name]
    px, keys, values = c.build()
    want, missed = ct.map_oracle(px, c, keys, values)
    for a in (px, keys, values, want):
        a.setflags(write=False)
    return px, keys, values, want, missed


def device_pixels(s, px, offset=0):
    """the pixels on the device, `offset` bytes behind a 16-byte boundary (torch's allocations are aligned to more)"""
    t = s.to_device(bytes(16 + offset) + px.tobytes())
    assert t.data_ptr() % 16 == 0
    return t[16 + offset:]


def room_of(c, px):
    return min(c.cap, max(len(px), 1))


def run_census(s, cases, wide=True, counts=True):
    """spng_census_wide_batch (or the old entry) over cases of one `bits` -> list of (status, written, keys, counts or None), the
    arrays as long as their outputs: room + GUARD entries filled with 0xFF in front of the call"""
    bits = cases[0].bits
    pxs = [census_input(c.name)[0] for c in cases]
    tens = [device_pixels(s, px, c.offset) for c, px in zip(cases, pxs)]
    rooms = [(room_of(c, px) if wide else c.cap) + GUARD for c, px in zip(cases, pxs)]
    outs = [(s.to_device(b"\xff" * (4 * r)), s.to_device(b"\xff" * (8 * r)) if counts else None) for r in rooms]
    outs, res = s.census_batch(tens, bits, [c.layout for c in cases], [c.cap for c in cases], [c.premultiply for c in cases], counts, outs=outs,
                               wide=wide)
    s.sync()
    return [(r.status, int(r.written), k.cpu().numpy().view(np.uint32), c.cpu().numpy().view(np.uint64) if c is not None else None)
            for (k, c), r in zip(outs, res)]


def check_census(got, case):
    status, written, keys, counts = got
    px, wk, wc = census_input(case.name)
    if len(wk) > case.cap:
        assert (status, written) == (64, 0), (case.name, status, written)
        return
    assert (status, written) == (0, len(wk)), (case.name, status, written, len(wk))
    assert (keys[:written] == wk).all() and (keys[written:] == 0xFFFFFFFF).all(), case.name      # untouched behind `written`
    if counts is not None:
        assert (counts[:written] == wc).all() and int(counts[:written].sum()) == len(px), case.name
        assert (counts[written:] == 0xFFFFFFFFFFFFFFFF).all(), case.name


def same(a, b):
    return a[:2] == b[:2] and (a[0] != 0 or ((a[2][:a[1]] == b[2][:a[1]]).all() and (a[3][:a[1]] == b[3][:a[1]]).all()))


# ---- wide census ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CENSUS, ids=lambda c: c.name)
def test_census_case_alone(gpu, case):
    """every case alone against numpy, guard entries behind `written` in both arrays; where the old entry accepts the cap, its bytes"""
    s = gpu.load()
    got = run_census(s, [case])[0]
    check_census(got, case)
    if case.cap <= 65536:
        old = run_census(s, [case], wide=False)[0]
        assert same(got, old), case.name


@pytest.mark.parametrize("bits", [8, 16])
def test_census_batch_equals_each_case_alone_and_repeats(gpu, bits):
    s = gpu.load()
    cases = [c for c in CENSUS if c.bits == bits]
    first = run_census(s, cases)
    for got, c in zip(first, cases):
        check_census(got, c)
        assert same(got, run_census(s, [c])[0]), c.name
    again = run_census(s, cases)
    for a, b, c in zip(first, again, cases):
        assert a[:2] == b[:2] and (a[0] != 0 or ((a[2] == b[2]).all() and (a[3] == b[3]).all())), c.name


def test_census_result_forms_and_no_counts(gpu):
    s = gpu.load()
    cases = [ct.BY_NAME[n] for n in ("census/distinct/4097", "census/cap/65535/over/back", "census/empty", "census/ends/both/u8/rgba")]
    for got, c in zip(run_census(s, cases, counts=False), cases):
        assert got[3] is None
        check_census(got, c)
    # d_results alone, h_results alone, both
    tens = [device_pixels(s, census_input(c.name)[0]) for c in cases]
    descs = (gpu.CensusDesc * len(cases))()
    keep = []
    for i, (c, t) in enumerate(zip(cases, tens)):
        k = s.empty(4 * room_of(c, census_input(c.name)[0]))
        keep.append(k)
        descs[i] = gpu.CensusDesc(s._ptr(t), len(census_input(c.name)[0]), s._ptr(k), None, c.cap, 8, c.layout, 0)
    want = [(0, 4097), (64, 0), (0, 0), (0, 2)]
    d_res = s.to_device(b"\xee" * (40 * len(cases)))
    h_res = (gpu.Result * len(cases))()
    for d, h in ((d_res, None), (None, h_res), (d_res, h_res)):
        assert s.lib.spng_census_wide_batch(s.ctx, descs, len(cases), s._ptr(d) if d is not None else None, h) == 0
        s.sync()
        if d is not None:
            r = np.frombuffer(d.cpu().numpy().tobytes(), dtype=[("status", "<i4"), ("r", "<i4"), ("written", "<u8"), ("consumed", "<u8"), ("aux", "<u8", 2)])
            assert [(int(x["status"]), int(x["written"])) for x in r] == want
        if h is not None:
            assert [(x.status, x.written) for x in h] == want
            assert [x.consumed for x in h] == [len(census_input(c.name)[0]) if w[0] == 0 else 0 for c, w in zip(cases, want)]


def test_census_cap_of_2_24_with_5_pixels(gpu):
    s = gpu.load()
    keys, counts = s.census_wide(bytes([1, 2, 3, 4] * 3 + [9, 9, 9, 9] * 2), 8, RGBA, cap=1 << 24)
    assert keys.tolist() == [0x04030201, 0x09090909] and counts.tolist() == [3, 2]
    keys, counts = s.census_wide(b"", 8, RGBA)
    assert len(keys) == 0 and len(counts) == 0
    with pytest.raises(gpu.SpngError) as e:
        s.census_wide(bytes(range(200)) * 4, 8, RGBA, cap=16)
    assert e.value.status == gpu.E_OUTPUT_CAPACITY


def test_census_wide_refusals(gpu):
    s = gpu.load()
    buf = s.to_device(bytes([0xEE]) * 4096)
    base, E = buf.data_ptr(), gpu.E_ARGUMENT

    def desc(d_pixels=base, count=16, d_keys=base + 1024, d_counts=base + 2048, cap=16, bits=8, layout=RGBA, premultiply=0, reserved=0):
        d = gpu.CensusDesc(d_pixels, count, d_keys, d_counts, cap, bits, layout, premultiply)
        d.reserved[0] = reserved
        return d

    def call(*descs, ctx=s.ctx):
        return s.lib.spng_census_wide_batch(ctx, (gpu.CensusDesc * len(descs))(*descs), len(descs), None, (gpu.Result * max(len(descs), 1))())

    assert call(desc()) == 0 and call(desc(bits=16)) == 0 and call(desc(d_counts=None)) == 0 and call(desc(count=0, d_pixels=None)) == 0
    assert call(desc(cap=1 << 24)) == 0 and call(desc(cap=65537)) == 0
    assert call(desc(cap=(1 << 24) + 1)) == E
    assert call(desc(cap=0)) == E
    assert call(desc(bits=12)) == E
    assert call(desc(d_keys=None)) == E
    assert call(desc(d_keys=base + 1026)) == E
    assert call(desc(d_counts=base + 2052)) == E
    assert call(desc(bits=16, d_pixels=base + 1)) == E
    assert call(desc(d_pixels=None)) == E
    assert call(desc(count=1 << 60)) == E
    assert call(desc(reserved=1)) == E
    assert call(desc(layout=3)) == E
    assert call(desc(premultiply=3)) == E
    assert call(desc(premultiply=2)) == E                         # (the as-UInt8 form: T = UInt16 only)
    assert call(desc(layout=SCALAR, premultiply=1)) == E
    first = desc(d_keys=base + 3072, d_counts=base + 3200)
    assert call(first, desc(bits=16)) == E                        # descs of one call disagree on T
    assert call(first, desc(cap=(1 << 24) + 1)) == E
    assert call() == 0 and s.lib.spng_census_wide_batch(s.ctx, None, 0, None, None) == 0 and call(desc(), ctx=None) == E
    assert s.lib.spng_census_wide_batch(s.ctx, (gpu.CensusDesc * 1)(desc()), 1, None, None) == E      # nowhere to put the results
    s.sync()
    assert (buf[3072:].cpu().numpy() == 0xEE).all()               # a refused call enqueues nothing
    # the old entry's ceiling stays
    assert s.lib.spng_census_batch(s.ctx, (gpu.CensusDesc * 1)(desc(cap=65537)), 1, None, (gpu.Result * 1)()) == E


# ---- map -----------------------------------------------------------------------------------------------------------------------
def run_map(s, cases):
    """spng_map_batch over cases of one `bits`; every output `offset` values behind a 16-byte boundary, between guard bytes ->
    list of (status, written, consumed, missed, values per pixel as uint64)"""
    torch = s.torch
    ins = [map_input(c.name) for c in cases]
    tens = [device_pixels(s, i[0]) for i in ins]
    bufs = [s.to_device(b"\xee" * (32 + (c.offset + len(i[0])) * c.value_bytes + 32)) for c, i in zip(cases, ins)]
    outs = [b[32 + c.offset * c.value_bytes:32 + (c.offset + len(i[0])) * c.value_bytes] for b, c, i in zip(bufs, cases, ins)]
    dk = [torch.from_numpy(i[1].view(np.int32).copy()).to(s.tdev) for i in ins]
    dv = [torch.from_numpy(i[2].astype("<u%d" % c.value_bytes).view(np.uint8).copy()).to(s.tdev) for c, i in zip(cases, ins)]
    _, res = s.map_batch(tens, cases[0].bits, [c.layout for c in cases], dk, dv, [c.value_bytes for c in cases],
                         [ct.MISS & ((1 << 8 * c.value_bytes) - 1) for c in cases], [c.premultiply for c in cases], outs=outs)
    s.sync()
    got = []
    for b, c, i, r in zip(bufs, cases, ins, res):
        raw = b.cpu().numpy()
        lo, hi = 32 + c.offset * c.value_bytes, 32 + (c.offset + len(i[0])) * c.value_bytes
        assert (raw[:lo] == 0xEE).all() and (raw[hi:] == 0xEE).all(), c.name
        got.append((r.status, int(r.written), int(r.consumed), int(r.aux[0]), raw[lo:hi].view("<u%d" % c.value_bytes).astype(np.uint64)))
    return got


def check_map(got, case):
    px, keys, values, want, missed = map_input(case.name)
    assert got[:4] == (0, len(px) * case.value_bytes, len(px), missed), (case.name, got[:4], missed)
    assert (got[4] == want).all(), case.name


@pytest.mark.parametrize("case", MAPS, ids=lambda c: c.name)
def test_map_case_alone(gpu, case):
    """every case against numpy; with 1-byte values and a map the old entry accepts, against spng_pack_indexed_batch too"""
    s = gpu.load()
    got = run_map(s, [case])[0]
    check_map(got, case)
    if case.value_bytes == 1 and 0 <= len(map_input(case.name)[1]) <= 65536 and not case.duplicate:
        px, keys, values = map_input(case.name)[:3]
        t = s.torch
        dk = t.from_numpy(keys.view(np.int32).copy()).to(s.tdev)
        di = t.from_numpy(values.astype(np.uint8)).to(s.tdev)
        (sto,), res = s.pack_indexed_batch([device_pixels(s, px)], [(len(px), 1)], case.bits, case.layout, [dk], [di], ct.MISS & 255, case.premultiply)
        s.sync()
        assert res[0].status == 0 and res[0].aux[0] == got[3] and (sto[:len(px)].cpu().numpy() == got[4]).all()


@pytest.mark.parametrize("bits", [8, 16])
def test_map_batch_of_every_case(gpu, bits):
    """maps in LDS and in scratch, values of every size, in one call: each table has its own place in the scratch"""
    s = gpu.load()
    cases = [c for c in MAPS if c.bits == bits]
    for got, c in zip(run_map(s, cases), cases):
        check_map(got, c)


def test_map_refusals(gpu):
    s = gpu.load()
    with pytest.raises(gpu.SpngError) as e:                       # keys that are not ascending: seen in the host-pointer form
        s.map(bytes(16), 8, RGBA, [5, 3], np.zeros(2, dtype=np.uint16))
    assert e.value.status == gpu.E_ARGUMENT
    with pytest.raises(gpu.SpngError) as e:
        s.map(bytes(16), 8, RGBA, [5, 5], np.zeros(2, dtype=np.uint16))
    assert e.value.status == gpu.E_ARGUMENT
    out, missed = s.map(bytes(16), 8, RGBA, [0], np.array([0x1234], dtype=np.uint16), miss=1)
    assert out.tolist() == [0x1234] * 4 and missed == 0
    host = np.full(8192, 0xEE, dtype=np.uint8)
    host[1024:1032] = np.array([1, 2], dtype="<u4").view(np.uint8)
    buf = s.to_device(host)
    base, E = buf.data_ptr(), gpu.E_ARGUMENT

    def desc(d_pixels=base, d_out=base + 2048, d_keys=base + 1024, d_values=base + 1040, count=16, map_count=2, source=8, layout=RGBA,
             premultiply=0, value_bytes=8, reserved=None):
        d = gpu.MapDesc(d_pixels, d_out, d_keys, d_values, count, map_count, source, layout, premultiply, value_bytes)
        if reserved is not None:
            d.reserved[reserved] = 1
        return d

    def call(*descs, ctx=s.ctx):
        return s.lib.spng_map_batch(ctx, (gpu.MapDesc * len(descs))(*descs), len(descs), None, (gpu.Result * max(len(descs), 1))())

    assert call(desc()) == 0 and call(desc(source=16)) == 0 and call(desc(source=16, premultiply=2)) == 0
    for vb in (1, 2, 4):
        assert call(desc(value_bytes=vb, d_out=base + 2048 + vb, d_values=base + 1040 + vb)) == 0      # aligned to a value is enough
    assert call(desc(map_count=0, d_keys=None, d_values=None)) == 0 and call(desc(count=0, d_pixels=None, d_out=None)) == 0
    assert call(desc(source=12)) == E
    assert call(desc(reserved=0)) == E
    assert call(desc(reserved=7)) == E
    assert call(desc(value_bytes=0)) == E
    assert call(desc(value_bytes=3)) == E
    assert call(desc(value_bytes=16)) == E
    assert call(desc(d_out=base + 2052)) == E                     # 8-byte values at an address that is 4 mod 8
    assert call(desc(d_values=base + 1044)) == E
    assert call(desc(value_bytes=2, d_out=base + 2049)) == E
    assert call(desc(d_keys=base + 1026)) == E
    assert call(desc(d_keys=None)) == E
    assert call(desc(d_values=None)) == E
    assert call(desc(d_pixels=None)) == E
    assert call(desc(d_out=None)) == E
    assert call(desc(source=16, d_pixels=base + 1)) == E
    assert call(desc(map_count=(1 << 24) + 1)) == E
    assert call(desc(layout=3)) == E
    assert call(desc(premultiply=3)) == E
    assert call(desc(premultiply=2)) == E
    assert call(desc(layout=SCALAR, premultiply=1)) == E
    assert call(desc(count=1 << 60)) == E
    first = desc(d_out=base + 4096)
    assert call(first, desc(source=16)) == E                      # descs of one call disagree on `source`
    assert call(first, desc(value_bytes=3)) == E
    assert call() == 0 and s.lib.spng_map_batch(s.ctx, None, 0, None, None) == 0 and call(desc(), ctx=None) == E
    assert s.lib.spng_map_batch(s.ctx, (gpu.MapDesc * 1)(desc()), 1, None, None) == E                  # nowhere to put the results
    s.sync()
    assert (buf[4096:].cpu().numpy() == 0xEE).all()               # a refused call enqueues nothing
    # the old entry's ceiling stays
    old = gpu.PackIndexedDesc(base, base + 2048, base + 1024, base + 1040, 4, 4, 65537, 8, RGBA, 0, 7)
    assert s.lib.spng_pack_indexed_batch(s.ctx, (gpu.PackIndexedDesc * 1)(old), 1, None, (gpu.Result * 1)()) == E


def test_profile_counts_the_launches_under_the_old_ids(gpu):
    """no new kernel id: the wide census is timed under SPNG_K_CENSUS (the counting stage, and the stages behind the wait), the map
    under SPNG_K_PACK_INDEXED; 20 is still no kernel"""
    s = gpu.load()
    case = ct.BY_NAME["census/distinct/4097"]
    t = device_pixels(s, census_input(case.name)[0])
    s.profile(True)
    before_c, before_m = s.profile_get(gpu.K_CENSUS)[1], s.profile_get(gpu.K_PACK_INDEXED)[1]
    s.census_wide_batch([t], 8, RGBA, case.cap)
    run_map(s, [ct.BY_NAME["map/count/513/v4"]])
    (ms_c, n_c), (ms_m, n_m) = s.profile_get(gpu.K_CENSUS), s.profile_get(gpu.K_PACK_INDEXED)
    s.profile(False)
    assert n_c - before_c == 2 and n_m - before_m == 1 and ms_c >= 0 and ms_m >= 0
    assert s.lib.spng_profile_get(s.ctx, 20, ctypes.byref(ctypes.c_double(0)), ctypes.byref(ctypes.c_uint64(0))) == gpu.E_ARGUMENT


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
lib.spng_census_wide.argtypes = [vp, vp, u64, ci, ci, ci, u32, vp, vp, rp]
lib.spng_map.argtypes = [vp, vp, u64, ci, ci, ci, vp, vp, u32, ci, vp, vp, rp]
ctx = vp()
assert lib.spng_create(0, None, ctypes.byref(ctx)) == 0
rng = np.random.default_rng(9)
colours = rng.integers(0, 1 << 16, (70000, 4)).astype("<u2")
px = np.ascontiguousarray(np.concatenate([colours, colours[rng.integers(0, 70000, 5000)]]))
n = len(px)
keys, counts = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
res = Result()
assert lib.spng_census_wide(ctx, px.ctypes.data, n, 16, 0, 0, 1 << 24, keys.ctypes.data, counts.ctypes.data, ctypes.byref(res)) == 0 and res.status == 0
wk, wc = ref.census(px, 16, 0)
m = res.written
assert m == len(wk) > 65536 and (keys[:m] == wk).all() and (counts[:m] == wc).all()
assert lib.spng_census_wide(ctx, px.ctypes.data, n, 16, 0, 0, 66000, keys.ctypes.data, None, ctypes.byref(res)) == 0 and res.status == 64 and res.written == 0
values = (wk.astype(np.uint64) * 0x9E3779B97F4A7C15) ^ 0x5555
out = np.zeros(n, dtype=np.uint64)
miss = np.array([0x0102030405060708], dtype=np.uint64)
assert lib.spng_map(ctx, px.ctypes.data, n, 16, 0, 0, wk.ctypes.data, values.ctypes.data, m - 100, 8, miss.ctypes.data, out.ctypes.data, ctypes.byref(res)) == 0
k = ref.keys(px, 16, 0)
at = np.searchsorted(wk[:m - 100], k)
hit = (at < m - 100) & (wk[np.minimum(at, m - 101)] == k)
assert res.status == 0 and res.written == 8 * n and res.consumed == n and res.aux[0] == int((~hit).sum()) > 0
assert (out == np.where(hit, values[np.minimum(at, m - 101)], miss[0])).all()
bad = np.array([7, 7], dtype=np.uint32)
assert lib.spng_map(ctx, px.ctypes.data, n, 16, 0, 0, bad.ctypes.data, values.ctypes.data, 2, 8, miss.ctypes.data, out.ctypes.data, ctypes.byref(res)) == 65
assert lib.spng_map(ctx, px.ctypes.data, n, 16, 0, 0, wk.ctypes.data, values.ctypes.data, 2, 3, miss.ctypes.data, out.ctypes.data, ctypes.byref(res)) == 65
lib.spng_destroy(ctx)
assert "torch" not in sys.modules
print("torch-free colour tables ok")
"""


def test_host_pointer_forms_without_torch(gpu):
    r = subprocess.run([sys.executable, "-c", CHILD, str(ph.ROOT)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch-free colour tables ok" in r.stdout


# ---- the tutorial as a table ---------------------------------------------------------------------------------------------------
def test_the_custom_colour_tutorial_as_a_table(gpu):
    """Snippets/PNG/CustomColor.swift without a kernel of its own: lex, decode and unpack(as: RGBA<UInt8>) on the device, a wide
    census (97 388 keys: more than spng_census_batch can report), HSVA.init(r:g:b:a:) on the keys' aggregates on the host, and an
    8-byte map -- byte for byte what spng_hsva_batch(FROM_RGBA8) writes.  The same through Session.map_colours; the BasicEncoding
    tutorial's luminance as a 1-byte table against spng_luminance_batch; and the nearest-palette indexer Session.pack(indexer=)
    refuses on this picture."""
    from swift_png_amd.mirror import PNG
    s = gpu.load()
    torch = s.torch
    data = (ph.GOLDEN / "customcolor" / "CustomColor.png").read_bytes()
    d_png, d_idat = s.to_device(data), s.empty(len(data))
    infos = (gpu.Lexed * 1)()
    files = (gpu.FileDesc * 1)(gpu.FileDesc(s._ptr(d_png), len(data), s._ptr(d_idat), len(data)))
    assert s.lib.spng_lex_batch(s.ctx, files, 1, None, infos) == 0
    r = infos[0]
    assert (r.status, r.width, r.height, r.depth, r.color, r.interlace) == (0, 400, 588, 8, 2, 0)
    w, h, n = r.width, r.height, r.width * r.height
    d_rows, d_storage = s.empty(gpu.inflated_size(w, h, 8, 3, False)), s.empty(3 * n)
    assert s.decode_batch([s.image_desc(d_idat[:r.idat_len], d_rows, d_storage, w, h, 8, 3, False)])[0].status == 0
    d_rgba = s.empty(4 * n)
    und = (gpu.UnpackDesc * 1)(gpu.UnpackDesc(s._ptr(d_storage), s._ptr(d_rgba), None, w, h, 0, (ctypes.c_uint16 * 3)(0, 0, 0), 8, 3, 0, 0, 0,
                                              8, gpu.TARGET_RGBA, 0))
    assert s.lib.spng_unpack_batch(s.ctx, und, 1) == 0
    d_rgba = d_rgba[:4 * n]
    # the census: exactly the 97 388 colours tests/test_hsva_ref.py counts
    ((d_keys, d_counts),), (rc,) = s.census_wide_batch([d_rgba], 8, RGBA, cap=n)
    assert (rc.status, rc.written, rc.consumed) == (0, 97388, 235200) and n == 235200
    keys = d_keys[:97388].cpu().numpy().view(np.uint32)
    assert int(d_counts[:97388].sum()) == n and (np.diff(keys.astype(np.int64)) > 0).all()
    _, (ro,) = s.census_batch([d_rgba], 8, RGBA, 65536)
    assert (ro.status, ro.written) == (gpu.E_OUTPUT_CAPACITY, 0)  # (the old entry, at its ceiling)
    # the function, once per key, on the host; the map on the device
    table = hsva_ref.from_rgba(keys.view(np.uint8).reshape(-1, 4))
    assert table.dtype.itemsize == 8
    d_values = s.to_device(table.tobytes())
    (d_out,), (rm,) = s.map_batch([d_rgba], 8, RGBA, [d_keys[:97388]], [d_values], 8)
    assert (rm.status, rm.written, rm.consumed, rm.aux[0]) == (0, 8 * n, n, 0)
    (d_hsva,), (rh,) = s.hsva_batch([d_rgba], gpu.HSVA_FROM_RGBA8)
    assert rh.status == 0
    got = d_out[:8 * n].cpu().numpy()
    assert got.tobytes() == d_hsva[:8 * n].cpu().numpy().tobytes()
    rgba = d_rgba.cpu().numpy().reshape(-1, 4)
    assert got.tobytes() == hsva_ref.from_rgba(rgba).tobytes()
    # the same through the host layer
    calls = []

    def to_hsva(k):
        calls.append(len(k))
        return hsva_ref.from_rgba(k.view(np.uint8).reshape(-1, 4)).view(PNG.HSVA.dtype())
    out = s.map_colours(rgba.tobytes(), 8, RGBA, to_hsva, PNG.HSVA.dtype())
    assert calls == [97388] and out.dtype == PNG.HSVA.dtype() and out.tobytes() == got.tobytes()
    # the BasicEncoding tutorial's luminance as a 1-byte table
    lum = s.map_colours(rgba.tobytes(), 8, RGBA, lambda k: tutorial_ref.luminance(k.view(np.uint8).reshape(-1, 4)), np.uint8)
    (d_lum,), (rl,) = s.luminance_batch([d_rgba], gpu.LUMINANCE_V8)
    s.sync()
    assert rl.status == 0 and lum.tobytes() == d_lum[:n].cpu().numpy().tobytes()
    # a nearest-palette indexer over the picture's colours: what Session.pack(indexer=) refuses here
    rng = np.random.default_rng(97388)
    palette = rng.integers(0, 256, (16, 4)).astype(np.int32)

    def nearest(k):
        c = np.ascontiguousarray(k).view(np.uint8).reshape(-1, 4).astype(np.int32)
        return np.concatenate([((c[i:i + 16384, None, :] - palette[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
                               for i in range(0, len(c), 16384)]).astype(np.uint8)
    idx = s.map_colours(rgba.tobytes(), 8, RGBA, nearest, np.uint8)
    assert (idx == nearest(ref.keys(rgba, 8, RGBA))).all()
    with pytest.raises(gpu.SpngError) as e:
        s.pack(rgba.tobytes(), w, h, 8, 1, indexed=True, source=8, palette=palette.astype(np.uint8).tobytes(),
               indexer=lambda entries: (lambda c: 0))
    assert e.value.status == gpu.E_OUTPUT_CAPACITY
