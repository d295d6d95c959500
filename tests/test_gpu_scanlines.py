"""The scanline kernels -- unfilter (csrc/unfilter.hip) and filter-select (csrc/encode.hip) -- on the device at production geometry,
byte for byte against the CPU oracle: hundreds of bands handed from wave to wave through the output raster, chains cut into pieces
by every branch of `launch_plan`, the 32-unit-tile kernels, rows on both sides of 2048 bytes, mixed batches in buffers at every
alignment, the piece-rows knob, rows that arrive in pieces, and the filter selection with its carries between the 1 KiB steps of a
row.  The cases and their generators are tests/scanline_cases.py; tests/test_scanline_cases.py shows (without a GPU) that each
case lies where it claims to.  No tolerance anywhere: storage a call did not decode must still hold the sentinel.

Under `-s` the module prints its wall time and the oracle's share of it when it ends (measured: profiles/README.md)."""
import time

import numpy as np
import pytest

import pnghelp as ph
import scanline_cases as sc

pytestmark = pytest.mark.gpu

UNFILTER = sc.unfilter_cases()
FILTER = sc.filter_cases()
GAP = 64                                 # sentinel bytes kept between two images of one buffer
ORACLE_SECONDS = [0.0]


@pytest.fixture(scope="module", autouse=True)
def _oracle_share():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_scanlines: {time.perf_counter() - t0:.1f} s, of which the oracle {ORACLE_SECONDS[0]:.1f} s")


def _oracle_unfilter(c, rows, rows_len=None):
    t0 = time.perf_counter()
    st, want = sc.oracle_unfilter(c, rows, rows_len)
    ORACLE_SECONDS[0] += time.perf_counter() - t0
    assert st == 0, c.name
    return want


def _oracle_filter(c, src):
    t0 = time.perf_counter()
    rows = np.frombuffer(ph.orc_filter(src, *c.fmt), np.uint8)
    ORACLE_SECONDS[0] += time.perf_counter() - t0
    return rows


def _layout(sizes, residues):
    """offsets of the images inside one buffer: image i starts `residues[i]` bytes behind a 16-byte boundary, GAP bytes at least
    behind the image before it -> (offsets, bytes of the buffer)"""
    offs, at = [], 0
    for n, r in zip(sizes, residues):
        at = (at + GAP + 15) // 16 * 16 + r
        offs.append(at)
        at += n
    return offs, at + GAP


def _upload(s, arrays, residues, fill=sc.SENTINEL):
    offs, total = _layout([len(a) for a in arrays], residues)
    host = np.full(total, fill, np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + len(a)] = a
    dev = s.to_device(host)
    assert dev.data_ptr() % 16 == 0
    return dev, offs


def _blank(s, sizes, residues):
    offs, total = _layout(sizes, residues)
    dev = s.torch.full((total,), sc.SENTINEL, dtype=s.torch.uint8, device=s.tdev)
    assert dev.data_ptr() % 16 == 0
    return dev, offs


def _gaps_hold_the_sentinel(host, offs, sizes, what):
    at = 0
    for o, n in zip(offs, sizes):
        assert (host[at:o] == sc.SENTINEL).all(), f"{what}: bytes in front of offset {o} were written"
        at = o + n
    assert (host[at:] == sc.SENTINEL).all(), f"{what}: bytes behind the last image were written"


def _descs(s, gpu, cases, rows_dev, rows_offs, st_dev, st_offs):
    descs = []
    for c, ro, so in zip(cases, rows_offs, st_offs):
        u, n = sc.inflated_size(c), sc.storage_size(c)
        assert u == gpu.inflated_size(*c.fmt) and n == gpu.storage_size(c.width, c.height, c.depth, c.channels)
        descs.append(s.image_desc(None, rows_dev[ro:ro + u], st_dev[so:so + n], *c.fmt, rows_cap=u))
    return descs


def _unfilter(s, gpu, cases, inputs, rows_len=None, rows_res=None, st_res=None):
    """ONE spng_unfilter_batch over `cases` -> the storage of each, as the device left it over the sentinel"""
    zero = [0] * len(cases)
    sizes = [sc.storage_size(c) for c in cases]
    rows_dev, rows_offs = _upload(s, inputs, rows_res or zero)
    st_dev, st_offs = _blank(s, sizes, st_res or zero)
    descs = _descs(s, gpu, cases, rows_dev, rows_offs, st_dev, st_offs)
    if rows_res is not None:
        assert {d.d_rows % 16 for d in descs} == set(range(16)) and {d.d_storage % 16 for d in descs} == set(range(16))
    res = s.unfilter_batch(descs, rows_len=rows_len)
    assert [r.status for r in res] == zero
    host = st_dev.cpu().numpy()
    _gaps_hold_the_sentinel(host, st_offs, sizes, "unfilter storage")
    return [host[o:o + n] for o, n in zip(st_offs, sizes)]


def _filter(s, gpu, cases, sources, rows_res=None, st_res=None):
    """ONE spng_filter_batch over `cases` -> the scanline stream of each"""
    zero = [0] * len(cases)
    sizes = [sc.inflated_size(c) for c in cases]
    st_dev, st_offs = _upload(s, sources, st_res or zero)
    rows_dev, rows_offs = _blank(s, sizes, rows_res or zero)
    descs = _descs(s, gpu, cases, rows_dev, rows_offs, st_dev, st_offs)
    res = s.filter_batch(descs)
    assert [r.status for r in res] == zero and [r.written for r in res] == sizes
    host = rows_dev.cpu().numpy()
    _gaps_hold_the_sentinel(host, rows_offs, sizes, "filter rows")
    return [host[o:o + n] for o, n in zip(rows_offs, sizes)], descs


def _same(c, got, want, row_bytes=None, note=""):
    report = sc.diff_report(c.name + note, got, want, row_bytes or sc.storage_row_bytes(c))
    assert not report, report


def _residues(n, mul, add):
    return [(mul * i + add) % 16 for i in range(n)]


# ---- a. unfilter, one large image per launch path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", UNFILTER, ids=[c.name for c in UNFILTER])
def test_unfilter_at_size(gpu, c):
    s = gpu.load()
    rows = sc.unfilter_input(c)
    want = _oracle_unfilter(c, rows)
    got, = _unfilter(s, gpu, [c], [rows])
    _same(c, got, want)


def test_unfilter_at_the_edge_of_the_wait_across_bands(gpu):
    """the ten shapes on the two sides of `band_may_wait` (csrc/geometry.hpp), one call each: one long piece of more bands than
    waves, the last step count at which a wave never waits for the first tile of its next band and the first at which it may"""
    s = gpu.load()
    assert len(sc.BOUND_EDGE_CASES) == 10
    for _, c in sc.BOUND_EDGE_CASES:
        rows = sc.unfilter_input(c)
        want = _oracle_unfilter(c, rows)
        got, = _unfilter(s, gpu, [c], [rows])
        _same(c, got, want)


@pytest.mark.parametrize("c", sc.SHORT_CASES, ids=[c.name for c in sc.SHORT_CASES])
def test_unfilter_short_input_at_size(gpu, c):
    """`rows_len` cuts the stream inside a row, exactly at a row's end, inside the last piece: the rows that are whole are the
    oracle's, everything behind them is left as it was"""
    s = gpu.load()
    rows = sc.unfilter_input(c)
    stride, rowb = sc.passes(c)[0][0] + 1, sc.storage_row_bytes(c)
    for n in sc.short_lengths(c):
        want = _oracle_unfilter(c, rows, n)
        got, = _unfilter(s, gpu, [c], [rows], rows_len=[n])
        done = (n // stride) * rowb
        assert (want[done:] == sc.SENTINEL).all()
        _same(c, got[:done], want[:done], rowb, f" cut at {n}")
        left = np.nonzero(got[done:] != sc.SENTINEL)[0]
        assert not len(left), f"{c.name} cut at {n}: row {(done + int(left[0])) // rowb} behind the last whole row {n // stride - 1} was written"


# ---- b. one call, mixed batch ------------------------------------------------------------------------------------------------------
def _batch(s, gpu, cases, rows_res=None, st_res=None):
    inputs = [sc.unfilter_input(c) for c in cases]
    wants = [_oracle_unfilter(c, r) for c, r in zip(cases, inputs)]
    gots = _unfilter(s, gpu, cases, inputs, rows_res=rows_res, st_res=st_res)
    for c, got, want in zip(cases, gots, wants):
        _same(c, got, want)


@pytest.mark.parametrize("k", sorted(sc.BATCH_FORMATS))
def test_unfilter_mixed_batch_at_every_alignment(gpu, k):
    """one pixel size, rows of one byte ... more than 2048 and 1 ... more than 1024 of them in ONE call (the narrow images go through
    the kernel and the piece length the widest one selects), rows and storage slices of two buffers at every residue mod 16"""
    s = gpu.load()
    cases = sc.batch_cases(k)
    _batch(s, gpu, cases, rows_res=_residues(len(cases), 1, 0), st_res=_residues(len(cases), 5, 3))


def test_unfilter_batch_of_many_rows(gpu):
    """more than 128 * 4096 rows in one call: the piece length follows `total_rows / 4096`"""
    _batch(gpu.load(), gpu, sc.scaled_batch_cases())


@pytest.mark.parametrize("ceiling", [False, True], ids=["term", "ceiling"])
def test_unfilter_batch_on_the_wide_branch_beyond_its_floor(gpu, ceiling):
    """one row of 2048 bytes among hundreds of narrow tall images: the 32-unit-tile kernel for all of them, pieces of
    `total_rows / 2048` rows (300 images) and of the 1024-row ceiling (1200 images)"""
    _batch(gpu.load(), gpu, sc.wide_batch_cases(ceiling))


@pytest.mark.parametrize("k", [4, 8])
def test_unfilter_batch_on_the_four_band_floor(gpu, k):
    """128 images of 800 rows: the pieces of the line-aligned kernels are held at four bands (`floor4`)"""
    _batch(gpu.load(), gpu, sc.floor4_batch_cases(k))


# ---- c. the piece-rows knob changes no result --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", sc.KNOB_CASES, ids=[c.name for c in sc.KNOB_CASES])
def test_piece_rows_knob_changes_no_result(gpu, c):
    s = gpu.load()
    rows = sc.unfilter_input(c)
    want = _oracle_unfilter(c, rows)
    try:
        for v in sc.KNOB_VALUES:
            s.configure(gpu.CFG_UNFILTER_PIECE_ROWS, v)
            got, = _unfilter(s, gpu, [c], [rows])
            _same(c, got, want, note=f" pieces of {v} rows")
    finally:
        s.configure(gpu.CFG_UNFILTER_PIECE_ROWS, 0)


# ---- d. rows that arrive in pieces, at size ----------------------------------------------------------------------------------------
def _whole_rows(c, n):
    """bytes of the first n inflated bytes that are whole scanlines"""
    off = done = 0
    for pitch, h, _ in sc.passes(c):
        stride = pitch + 1
        done += min(h, max(0, n - off) // stride) * stride
        off += stride * h
    return done


@pytest.mark.parametrize("c", sc.RESUME_CASES, ids=[c.name for c in sc.RESUME_CASES])
def test_rows_arrive_in_pieces_at_size(gpu, c):
    """spng_unfilter_resume_batch: after every push the rows that are whole by then are the oracle's for that prefix, the rest of
    storage is untouched, and `written` adds up to the scanline bytes -- pushes of less than a row, one row, thousands of rows, ending
    inside rows.  The device's scanline buffer holds nothing but what has been pushed."""
    s = gpu.load()
    rows = sc.unfilter_input(c)
    u, n = sc.inflated_size(c), sc.storage_size(c)
    src = s.to_device(rows)
    d_rows = s.torch.full((u,), 0xFF, dtype=s.torch.uint8, device=s.tdev)
    d_st = s.torch.full((n,), sc.SENTINEL, dtype=s.torch.uint8, device=s.tdev)
    work = s.torch.full((u,), 0xFF, dtype=s.torch.uint8, device=s.tdev) if (c.interlaced or c.volume < 8) else None
    desc = s.image_desc(None, d_rows, d_st, *c.fmt, rows_cap=u)
    prev = written = 0
    for now in sc.resume_pushes(c):
        d_rows[prev:now] = src[prev:now]
        r = s.unfilter_resume(desc, work, prev, now)
        assert r.status == 0
        written += r.written
        assert written == r.consumed == _whole_rows(c, now), (c.name, now, written, r.consumed)
        want = _oracle_unfilter(c, rows, now)
        _same(c, d_st.cpu().numpy(), want, note=f" after {now} bytes")
        prev = now
    assert written == u


# ---- e. filter-select vs the oracle ------------------------------------------------------------------------------------------------
def _filter_and_back(s, gpu, cases, rows_res=None, st_res=None):
    sources = [sc.filter_source(c) for c in cases]
    wants = [_oracle_filter(c, src) for c, src in zip(cases, sources)]
    gots, _ = _filter(s, gpu, cases, sources, rows_res=rows_res, st_res=st_res)
    for c, got, want in zip(cases, gots, wants):
        _same(c, got, want, max(p for p, _, _ in sc.passes(c)) + 1 if not c.interlaced else 1 << 62)
    # and back: the device defilters what the device filtered
    backs = _unfilter(s, gpu, cases, gots)
    for c, back, src in zip(cases, backs, sources):
        _same(c, back, src, note=" defiltered again")


@pytest.mark.parametrize("c", FILTER, ids=[c.name for c in FILTER])
def test_filter_at_size(gpu, c):
    """every format at a row of several 1 KiB steps that takes the 16-bytes-per-lane path and at one that does not, sub-byte rows
    of PACKED_ROW and PACKED_ROW + 1 bytes, images taller than the grid, Adam7 -- on noise, a synthetic image (four to five filter
    types) and noise rows between zero rows (exact ties of None / Up and of Sub / Paeth).  Buffers start wherever the case's name
    puts them mod 16."""
    seed = sc.seed_of(c.name)
    _filter_and_back(gpu.load(), gpu, [c], rows_res=[seed % 16], st_res=[(seed >> 4) % 16])


def test_filter_mixed_batch_at_every_alignment(gpu):
    cases = sc.filter_batch_cases()
    s = gpu.load()
    rows_res, st_res = _residues(len(cases), 1, 0), _residues(len(cases), 7, 2)
    assert set(rows_res) == set(range(16)) and set(st_res) == set(range(16))
    _filter_and_back(s, gpu, cases, rows_res=rows_res, st_res=st_res)
