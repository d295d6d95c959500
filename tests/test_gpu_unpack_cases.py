"""unpack_kernel and pack_kernel on the device over the case table of tests/unpack_cases.py, byte for byte against the oracle
(oracle/pixels.py): every case through Session.unpack / Session.pack; the cases that sit off a 16-byte boundary, mixed batches, a 1 x 1
image under a 2049 x 2048 one's grid and indexed jobs with different palettes through raw descs (UnpackDesc / PackDesc) that point into
one device buffer filled with 0xEE, every byte of which is compared afterwards."""
import ctypes

import numpy as np
import pytest

import unpack_cases as uc

pytestmark = pytest.mark.gpu

GUARD = 64


def groups():
    g = {}
    for c in uc.CASES:
        if c.at == (0, 0) and not c.huge:
            g.setdefault("/".join(c.name.split("/")[:2]), []).append(c)
    return g


def through_session(s, c):
    if c.kind == "unpack":
        return s.unpack(uc.storage(c), c.width, c.height, c.depth, c.channels, indexed=c.indexed, bgr=c.bgr, target=c.bits,
                        palette=uc.palette(c), key=c.key, layout=c.layout, premultiply=c.premultiply)
    return s.pack(uc.source(c), c.width, c.height, c.depth, c.channels, indexed=c.indexed, bgr=c.bgr, source=c.bits, palette=uc.palette(c),
                  layout=c.layout, premultiply=c.premultiply)


@pytest.mark.parametrize("group", sorted(groups()))
def test_every_case_of_the_table(gpu, group):
    s = gpu.load()
    for c in groups()[group]:
        got, want = through_session(s, c), uc.expected(c)
        assert len(got) == len(want), c.name
        if got != want:
            bad = np.flatnonzero(np.frombuffer(got, dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8))
            pytest.fail("%s (%s): %d bytes differ, the first at %d" % (c.name, c.reason, bad.size, bad[0]))


@pytest.mark.parametrize("case", [c for c in uc.CASES if c.huge], ids=lambda c: c.name)
def test_above_the_cap_of_the_grid(gpu, case):
    """4097 x 4096 grey8 <-> UInt8 scalars: 4096 workgroups, every thread comes round a fifth time"""
    s = gpu.load()
    got, want = through_session(s, case), uc.expected(case)
    assert len(got) == len(want) == case.n
    assert (np.frombuffer(got, dtype=np.uint8) == np.frombuffer(want, dtype=np.uint8)).all()


def run_descs(s, gpu, cases, expect=0):
    """`cases` (one kind, one T) as the descs of ONE spng_unpack_batch / spng_pack_batch call.  Inputs, palettes and outputs are slots of
    one device buffer of 0xEE: every slot starts `at` bytes behind a 16-byte boundary, the outputs back to back with 64 poisoned bytes
    at least between them.  The whole buffer is compared with what the oracle says it must hold."""
    kind, bits = cases[0].kind, cases[0].bits
    assert all(c.kind == kind and c.bits == bits for c in cases)
    pos, slots = 0, []

    def take(nbytes, off):
        nonlocal pos
        at = pos + off
        pos = (at + nbytes + GUARD + 15) & ~15
        return at

    parts = [(uc.source(c), uc.palette(c) or b"", uc.expected(c)) for c in cases]
    for c, (src, pal, want) in zip(cases, parts):
        slots.append((take(len(src), c.at[0]), take(len(pal), 0)))
    outs = [take(len(want), c.at[1]) for c, (_, _, want) in zip(cases, parts)]
    host = np.full(pos + 4096, 0xEE, dtype=np.uint8)
    for (src, pal, _), (i, p) in zip(parts, slots):
        host[i:i + len(src)] = np.frombuffer(src, dtype=np.uint8)
        host[p:p + len(pal)] = np.frombuffer(pal, dtype=np.uint8)
    image = host.copy()
    for (_, _, want), o in zip(parts, outs):
        image[o:o + len(want)] = np.frombuffer(want, dtype=np.uint8)
    buf = s.to_device(host)
    base = buf.data_ptr()
    assert base % 16 == 0
    descs = []
    for c, (i, p), o in zip(cases, slots, outs):
        pal = base + p if c.indexed and c.palette_count else None
        count = c.palette_count if c.indexed else 0
        if kind == "unpack":
            key = (ctypes.c_uint16 * 3)(*(list(c.key or ()) + [0, 0, 0])[:3])
            descs.append(gpu.UnpackDesc(base + i, base + o, pal, c.width, c.height, count, key, c.depth, c.channels, int(c.indexed), int(c.bgr),
                                        int(c.key is not None), bits, c.layout, c.premultiply))
        else:
            descs.append(gpu.PackDesc(base + i, base + o, pal, c.width, c.height, count, c.depth, c.channels, int(c.indexed), int(c.bgr), bits,
                                      c.layout, c.premultiply))
    if kind == "unpack":
        st = s.lib.spng_unpack_batch(s.ctx, (gpu.UnpackDesc * len(descs))(*descs), len(descs))
    else:
        st = s.lib.spng_pack_batch(s.ctx, (gpu.PackDesc * len(descs))(*descs), len(descs))
    assert st == expect
    s.sync()
    back = buf.cpu().numpy()
    if expect:
        image = host
    bad = np.flatnonzero(back != image)
    if bad.size:
        first = int(bad[0])
        owner = [c.name + (" (output)" if o <= first < o + len(w) else " (around the output)")
                 for c, o, (_, _, w) in zip(cases, outs, parts) if o - GUARD - 16 <= first < o + len(w) + GUARD + 16]
        pytest.fail("%d bytes differ, the first at %d: got %02x, want %02x: %s" % (bad.size, first, back[first], image[first], owner))


MOVED = [c for c in uc.CASES if c.at != (0, 0)]


@pytest.mark.parametrize("kind", ["unpack", "pack"])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("side", ["input", "output"])
def test_off_the_sixteen_byte_boundary(gpu, kind, bits, side):
    """the storage and, independently, the pixels 1, 2, 3, 4, 8 and 12 bytes behind a 16-byte boundary (pixels of UInt16: 2, 4, 8, 12,
    which is what the header allows): 1 - 3 turn off the 16-byte paths of rgba8 / bgra8, pack's 16-byte load for rgb8 / bgr8 and its
    dword stores; 4, 8, 12 only its store of 3- and 6-byte pixels through LDS.  Every offset of a side in one call, the 0xEE around
    every output untouched."""
    s = gpu.load()
    cases = [c for c in MOVED if c.kind == kind and c.bits == bits and (c.at[0] != 0) == (side == "input")]
    assert len(cases) >= 8 * 3 * 4
    run_descs(s, gpu, cases)


def test_a_misaligned_output_of_sixteen_bit_pixels_is_refused(gpu):
    """spng_unpack_batch: d_out at a multiple of T (include/spng_mi355.h) -- an odd address with T = UInt16 is SPNG_E_ARGUMENT and
    nothing is enqueued, behind a valid desc too; with T = UInt8 it is taken"""
    s = gpu.load()
    ok = uc.BY_NAME["unpack/rgba8/u16/rgba/5x3"]
    for off in (1, 3):
        odd = uc.Case(**{**ok.__dict__, "name": "odd", "at": (0, off)})
        run_descs(s, gpu, [odd], expect=gpu.E_ARGUMENT)
        run_descs(s, gpu, [ok, odd], expect=gpu.E_ARGUMENT)
    run_descs(s, gpu, [uc.BY_NAME["unpack/rgba8/u8/rgba/at0+1"], uc.BY_NAME["unpack/rgba8/u8/rgba/at0+3"]])


def test_the_key_of_a_cgbi_file_is_its_trns_reversed(gpu):
    """a file's tRNS holds (r, g, b); the bgr8 format of a CgBI image keeps it as (b, g, r) (PNG.Format.swift:427-430), which is what
    spng_unpack_desc.key takes: on storage whose pixels have r != b, the device given pnghelp.format_key(png) keys the pixels whose
    (r, g, b) equals the tRNS key -- as the helper that models the file says -- and given the tRNS key unreversed it keys others"""
    import pnghelp as ph
    s = gpu.load()
    c = uc.BY_NAME["unpack/bgr8/u16/rgba/keyed"]                    # storage (b, g, r), its key (b, g, r) = c.key
    trns = b"".join(int(v).to_bytes(2, "big") for v in c.key[::-1])  # the file's chunk: (r, g, b)
    png = ph.Png(c.width, c.height, 8, 2, False, True, b"", trns=trns)
    assert ph.format_key(png) == c.key and c.key[0] != c.key[2]
    sto = uc.storage(c)
    got = s.unpack(sto, c.width, c.height, 8, 3, bgr=True, target=16, key=ph.format_key(png))
    want = ph.unpack_rgba16(np.frombuffer(sto, dtype=np.uint8), png)
    assert got == uc.expected(c) == want.astype("<u2").tobytes()
    keyed = want[want[:, 3] == 0]
    assert len(keyed) and (keyed[:, :3] >> 8 == c.key[::-1]).all()
    assert s.unpack(sto, c.width, c.height, 8, 3, bgr=True, target=16, key=c.key[::-1]) != got


def mixed(kind, bits):
    """about 40 cases of one kind and T: every format once, sizes and layouts turning, from 1 pixel to 1023 x 17; the keyed and the
    indexed ones (unpack), those with a palette of their own (pack)"""
    sizes = uc.SIZES if kind == "unpack" else uc.PACK_SIZES
    cases = []
    for j in range(1 if kind == "unpack" else 2):                   # (pack: twice, with other sizes and layouts)
        for i, (depth, channels, indexed, bgr) in enumerate(f for f in uc._formats() if kind == "unpack" or not f[2]):
            w, h = sizes[(3 * i + 7 * j) % len(sizes)]
            cases.append(uc.BY_NAME["%s/%s/u%d/%s/%dx%d" % (kind, uc._fmt(depth, channels, indexed, bgr), bits, uc._lname((i + j) % 3), w, h)])
    extra = [c for c in uc.CASES if c.kind == kind and c.bits == bits and c.at == (0, 0) and not c.huge and
             (c.content in ("keyed", "alphas") or (c.content == "beyond" and c.depth in (2, 8)) or (kind == "pack" and c.indexed)
              or c.premultiply)]
    extra.sort(key=lambda c: not c.indexed)                          # (stable: the indexed ones first)
    return cases + [c for i, c in enumerate(extra) if c.layout == i % 3 or (kind == "pack" and c.indexed)][:40 - len(cases)]


@pytest.mark.parametrize("kind", ["unpack", "pack"])
@pytest.mark.parametrize("bits", [8, 16])
def test_one_call_of_forty_mixed_descs(gpu, kind, bits):
    s = gpu.load()
    cases = mixed(kind, bits)
    assert 30 <= len(cases) <= 40 and min(c.n for c in cases) == 1 and max(c.n for c in cases) == 1023 * 17
    assert len({(c.depth, c.channels, c.indexed, c.bgr) for c in cases}) == (17 if kind == "unpack" else 13 + 4)
    if kind == "pack":
        assert len({uc.palette(c) for c in cases if c.indexed}) >= 2          # (the LDS table of a workgroup is its own job's)
    run_descs(s, gpu, cases)
    run_descs(s, gpu, cases[::-1])


@pytest.mark.parametrize("kind", ["unpack", "pack"])
def test_a_small_job_under_a_large_jobs_grid(gpu, kind):
    """1 x 1 beside 2049 x 2048 rgba8 <-> RGBA<UInt8>: all jobs of a call share the grid of the largest, 1025 workgroups here, of which
    the small job needs one thread; and indexed8 jobs with different palettes beside it"""
    s = gpu.load()
    big = uc.Case("batch/%s/rgba8/2049x2048" % kind, kind, 2049, 2048, 8, 4, 8, reason="sets the grid of the call")
    one = uc.BY_NAME["%s/rgb8/u8/rgba/1x1" % kind]
    run_descs(s, gpu, [one, big])
    run_descs(s, gpu, [big, one])
    if kind == "pack":
        indexed = [uc.BY_NAME["pack/indexed8/u8/rgba/strangers"], uc.BY_NAME["pack/indexed4/u8/rgba/strangers"]]
        assert uc.palette(indexed[0]) != uc.palette(indexed[1])
        run_descs(s, gpu, [indexed[0], big, indexed[1], one])
