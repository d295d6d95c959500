"""The table of tests/scanline_cases.py really is where tests/test_gpu_scanlines.py needs it to be.  For every case: the input is
built, the oracle runs (status 0), and the properties the GPU tests rely on are asserted -- which kernel and which piece-length
branch the dispatch takes, on which side of the 2048-byte row it lies, that its filter-type bytes are what its regime says --
so that a threshold that moves in csrc/geometry.hpp (the arithmetic of csrc/host_decode.hip `launch_plan`, csrc/unfilter.hip
`launch_unfilter` and csrc/encode.hip `launch_filter`, called here as the library calls it: tests/geometry.py) or csrc/encode.hip
`PACKED_ROW` makes this file fail instead of silently taking a path out of the GPU tests.  No GPU needed."""
import os

import numpy as np
import pytest

import geometry as geo
import pnghelp as ph
import scanline_cases as sc

CSRC = os.path.join(str(ph.ROOT), "swift_png_amd", "csrc")
UNFILTER = sc.unfilter_cases()
FILTER = sc.filter_cases()


def test_the_mirrored_lines_are_still_in_the_sources():
    text = {}
    for name, line in sc.SOURCE_LINES:
        if name not in text:
            text[name] = open(os.path.join(CSRC, name)).read()
        assert line in text[name], (name, line)
    # `piece_start`, which both kernels call, starts a piece on None / Sub rows only -- and is the only place that looks for one
    assert text["unfilter.hip"].count("const unsigned long long m = __ballot(r < rows && ft <= 1);") == 1


def test_sizes_agree_with_the_oracle_and_stay_under_the_cap():
    lib = ph.oracle()
    total = 0
    names = set()
    for c in sc.all_cases():
        assert c.name not in names, c.name
        names.add(c.name)
        assert sc.inflated_size(c) == lib.orc_inflated_size(c.width, c.height, c.depth, c.channels, int(c.interlaced)), c.name
        assert sc.storage_size(c) == lib.orc_storage_size(c.width, c.height, c.depth, c.channels), c.name
        total += sc.inflated_size(c) + sc.storage_size(c)
    print(f"table: {len(names)} cases, {total / 2**20:.0f} MiB of scanlines and storage")
    assert total < sc.TOTAL_BYTES_CAP, total
    assert sc.seed_of("a") == 0xe8b7be43                         # (CRC-32: the same in every process, unlike hash())


def _check_regime(c, rows):
    for t in sc.types_of(c, rows):
        cuts = np.nonzero(t <= 1)[0]
        if c.regime == "mixed":
            assert set(range(5)) <= set(int(x) for x in t), c.name
        elif c.regime in ("up", "average", "paeth"):
            assert t[0] == 1 and (t[1:] == {"up": 2, "average": 3, "paeth": 4}[c.regime]).all(), c.name
        elif c.regime == "nocut":
            assert t[0] <= 1 and (t[1:] >= 2).all() and (t[1:] <= 4).all(), c.name
        elif c.regime == "rare":
            assert cuts[0] == 0 and (np.diff(cuts) > sc.BAND).all(), c.name


@pytest.mark.parametrize("c", UNFILTER, ids=[c.name for c in UNFILTER])
def test_unfilter_case(c):
    rows = sc.unfilter_input(c)
    st, storage = sc.oracle_unfilter(c, rows)
    assert st == 0
    assert (storage != sc.SENTINEL).any()
    jobs = [(p, h) for p, h, _ in sc.passes(c)]
    kernel, branch, piece, pieces = sc.case_plan(c)
    assert (kernel, branch) == (c.kernel, c.branch), (c.name, kernel, branch, piece, pieces)
    assert pieces >= 2, (c.name, piece, pieces)                  # every case of the table claims pieces
    widest = max(p for p, _ in jobs)
    if c.bpp in (1, 2):
        assert (widest >= sc.WIDE_ROW) == c.kernel.endswith(",32>"), c.name
    if c.bpp not in (4, 8):
        assert (widest >= sc.WIDE_ROW) == (c.branch == "wide"), c.name
    else:
        assert c.branch in ("rr", "few") and widest < (1 << 16)
        assert (c.branch == "few") == (c.bpp == 4 and c.height >= sc.PK_FEW_HEIGHT), c.name
    _check_regime(c, rows)
    if c.regime == "rare" and not c.interlaced:
        # a piece boundary whose next None / Sub row is 64 rows or more away: the ballot of `piece_start` goes round again -- and at least
        # two pieces survive (a cut row exists behind the first boundary)
        t = sc.types_of(c, rows)[0]
        cuts = np.nonzero(t <= 1)[0]
        far = [x for x in range(piece, c.height, piece)
               if (cuts[cuts >= x][0] if (cuts >= x).any() else c.height) - x >= sc.BAND]
        assert far, c.name
        assert (cuts >= piece).any(), c.name


def test_unfilter_table_reaches_every_path():
    got = {(c.kernel, c.branch) for c in UNFILTER}
    for k in ("u<4,1>", "u<4,2>", "u<3>", "u<6>"):
        assert (k, "floor128") in got, k
    for k in ("u<4,1,32>", "u<4,2,32>", "u<3>", "u<6>"):
        assert (k, "wide") in got, k
    assert {("pk<4>", "rr"), ("pk<4>", "few"), ("pk<8>", "rr")} <= got
    # every regime on every primary path
    for g in sc.PRIMARY:
        assert {c.regime for c in UNFILTER if c.name.startswith(g.name + " ")} == set(sc.REGIMES), g.name
    # rows of 2047 / 2048 / 2049 bytes (two-byte pixels: 2046 / 2048 / 2050, their rows are even), and both sides at large
    pitches = {1: set(), 2: set()}
    for c in UNFILTER:
        if c.bpp in pitches and not c.interlaced:
            pitches[c.bpp].add(sc.passes(c)[0][0])
    assert {2047, 2048, 2049} <= pitches[1] and min(pitches[1]) < 1600 and max(pitches[1]) >= 4096
    assert {2046, 2048, 2050} <= pitches[2] and min(pitches[2]) < 1900 and max(pitches[2]) >= 4096
    subbyte = {sc.passes(c)[0][0] >= sc.WIDE_ROW for c in UNFILTER if c.volume < 8 and not c.interlaced}
    assert subbyte == {False, True}
    # the line-aligned kernel of four-byte pixels: both sides of `2 NW + 1 < nph` (and its very edge: 1024 / 1028 bytes), both
    # sides of the 1024 rows of the `few` branch
    pk4 = [c for c in UNFILTER if c.bpp == 4]
    assert {(sc.pk_may_block(c.width * 4), c.height >= sc.PK_FEW_HEIGHT) for c in pk4} == {(a, b) for a in (False, True) for b in (False, True)}
    assert not sc.pk_may_block(1024) and sc.pk_may_block(1028)
    assert {1024, 1028} <= {sc.passes(c)[0][0] for c in pk4}
    # unfilter_kernel's wait for the next band (`NW * (K + 1) + 1 < ntiles`): rows that may wait, rows of the gap the former bound
    # left (in one long piece: the single-type regimes), rows too short for either -- for every byte-wise kernel
    assert (sc.u_may_block(6, 1800, False), sc.u_may_block(3, 900, False), sc.u_may_block(1, 900, False)) == ("gap",) * 3
    assert [sc.u_tiles(6, 6 * w, False)[1] for w in (330, 360)] == [13, 14] and sc.u_may_block(6, 6 * 330, False) == "gap"
    assert sc.u_may_block(6, 6 * 360, False) == "blocks" and sc.u_may_block(3, 3 * 520, False) == "blocks"
    for kernel, k in (("u<4,1>", 1), ("u<4,2>", 2), ("u<3>", 3), ("u<6>", 6)):
        seen = {sc.u_may_block(k, sc.passes(c)[0][0], False) for c in UNFILTER
                if c.kernel == kernel and not c.interlaced and c.regime == "paeth" and c.height > 4 * sc.BAND}
        assert seen == {"blocks", "gap", "never"}, (kernel, seen)
    # <3> and <6> on the wide branch: more than 1024 rows, two pieces at least of 256 .. 1024 rows
    for c in UNFILTER:
        if c.kernel in ("u<3>", "u<6>") and c.branch == "wide" and not c.interlaced:
            _, _, piece, pieces = sc.case_plan(c)
            assert c.height > 1024 and sc.WIDE_FLOOR <= piece <= sc.WIDE_CEIL and pieces >= 2
    # Adam7 at size: sub-byte, 3-byte, 8-byte
    assert {c.bpp if c.volume >= 8 else 0 for c in UNFILTER if c.interlaced} == {0, 3, 8}


def test_bound_edge_cases():
    """every pair lies on the two sides of `band_may_wait`, the first of it exactly at the edge, in one piece of more bands than waves"""
    assert len(sc.BOUND_EDGE_CASES) == 10 and {c.kernel for _, c in sc.BOUND_EDGE_CASES} == {"u<6>", "u<3>", "u<4,1>", "u<4,2>", "pk<4>", "pk<8>"}
    for steps, c in sc.BOUND_EDGE_CASES:
        nw, reach, per_band = sc.band_steps(c)
        assert per_band == steps, (c.name, per_band)
        edge = nw * (reach + 1) + 1                              # (spelled out here once: the figure the names carry)
        assert steps in (edge, edge + 1) and geo.band_may_wait(nw, reach, steps) == (steps == edge + 1), c.name
        assert not geo.band_may_wait(nw, reach, edge) and geo.band_may_wait(nw, reach, edge + 1)
        kernel, branch, piece, pieces = sc.case_plan(c)
        assert (kernel, branch) == (c.kernel, c.branch) and pieces >= 2, c.name
        rows = sc.unfilter_input(c)
        t, = sc.types_of(c, rows)
        assert t[0] == 1 and (t[1:] >= 2).all()                  # no row lets a second piece start: all of it is piece 0
        assert c.height > nw * (sc.BAND if c.bpp not in (4, 8) else sc.PK_TILE_BYTES // c.bpp)
        assert sc.oracle_unfilter(c, rows)[0] == 0
    # the needed count is the one the kernels wait for: band 5 of four waves, its producer's second band
    assert geo.band_steps_needed(5, 0, 4, 14, 2) == 14 + 2 + 1 and geo.band_steps_needed(5, 12, 4, 14, 2) == 14 + 13 + 1
    assert geo.band_steps_needed(1, 3, 4, 10, 1) == 3 + 1 + 1 and geo.band_steps_needed(4, 9, 4, 10, 1) == 9 + 1


def test_short_input_lengths():
    for c in sc.SHORT_CASES:
        stride = sc.passes(c)[0][0] + 1
        _, _, piece, pieces = sc.case_plan(c)
        ns = sc.short_lengths(c)
        assert any(n % stride not in (0, stride - 1) for n in ns)                  # inside a row
        assert any(n % stride == 0 for n in ns)                                     # exactly at a row's end
        assert any((pieces - 1) * piece < n // stride < c.height - 1 for n in ns)  # inside the last piece
        assert all(0 < n < sc.inflated_size(c) for n in ns)
    assert {c.kernel for c in sc.SHORT_CASES} == {"u<4,1,32>", "u<3>", "pk<4>"}


@pytest.mark.parametrize("k", sorted(sc.BATCH_FORMATS))
def test_mixed_batch(k):
    cases = sc.batch_cases(k)
    assert len(cases) >= 16                                   # one image per residue mod 16 of the buffer offsets
    assert all(c.bpp == k for c in cases)
    pitches = [sc.passes(c)[0][0] for c in cases]
    heights = [c.height for c in cases]
    assert min(c.width for c in cases) == 1 and max(pitches) >= sc.WIDE_ROW
    assert min(heights) == 1 and max(heights) > 1024
    kernel, branch, piece, pieces = sc.batch_plan(k, cases)
    assert pieces >= 2
    want = {1: ("u<4,1,32>", "wide"), 2: ("u<4,2,32>", "wide"), 3: ("u<3>", "wide"), 6: ("u<6>", "wide"), 4: ("pk<4>", "few"),
            8: ("pk<8>", "rr")}[k]
    assert (kernel, branch) == want
    # narrow images ride in the wide call: alone they would have taken the other kernel / branch
    alone = {sc.case_plan(c)[:2] for c in cases}
    assert len(alone) >= 2 or k == 8
    for c in cases:
        st, _ = sc.oracle_unfilter(c, sc.unfilter_input(c))
        assert st == 0


def test_scaled_and_floor4_batches():
    cases = sc.scaled_batch_cases()
    assert sum(c.height for c in cases) > 128 * sc.SCALE_ROWS
    kernel, branch, piece, pieces = sc.batch_plan(1, cases)
    assert (kernel, branch) == ("u<4,1>", "scaled") and piece > sc.PIECE_FLOOR and pieces >= 2
    for k in (4, 8):
        cases = sc.floor4_batch_cases(k)
        kernel, branch, piece, pieces = sc.batch_plan(k, cases)
        assert (kernel, branch, piece) == (f"pk<{k}>", "floor4", 64) and pieces >= 2
    # the wide branch beyond its 256-row floor: the `total_rows / 2048` term, and the 1024-row ceiling
    for ceiling in (False, True):
        cases = sc.wide_batch_cases(ceiling)
        kernel, branch, piece, pieces = sc.batch_plan(1, cases)
        assert (kernel, branch) == ("u<4,1,32>", "wide") and pieces >= 2
        raw = (sum(c.height for c in cases) // sc.WIDE_SCALE_ROWS + 63) & ~63
        assert (raw > sc.WIDE_CEIL and piece == sc.WIDE_CEIL) if ceiling else (sc.WIDE_FLOOR < raw == piece < sc.WIDE_CEIL)
        assert sc.oracle_unfilter(cases[-1], sc.unfilter_input(cases[-1]))[0] == 0
    for c in sc.scaled_batch_cases()[:3] + sc.floor4_batch_cases(4)[:3] + sc.floor4_batch_cases(8)[:3]:
        assert sc.oracle_unfilter(c, sc.unfilter_input(c))[0] == 0


def test_knob_and_resume_cases():
    assert {c.kernel for c in sc.KNOB_CASES} == {"u<4,1,32>", "u<4,2>", "u<3>", "u<6>", "pk<4>", "pk<8>"}
    assert min(sc.KNOB_VALUES) >= 8 and any(v % sc.BAND for v in sc.KNOB_VALUES)
    assert max(sc.KNOB_VALUES) > max(c.height for c in sc.KNOB_CASES)
    for c in sc.KNOB_CASES:
        for v in sc.KNOB_VALUES:
            assert sc.unfilter_plan(c.bpp, [(p, h) for p, h, _ in sc.passes(c)], v)[1:3] == ("configured", v)
    assert {c.kernel for c in sc.RESUME_CASES} >= {"u<4,1,32>", "u<3>", "pk<4>", "pk<8>"}
    assert any(c.interlaced for c in sc.RESUME_CASES) and any(c.volume < 8 and not c.interlaced for c in sc.RESUME_CASES)
    for c in sc.RESUME_CASES:
        assert sc.case_plan(c)[:2] == (c.kernel, c.branch), c.name
        stride = sc.passes(c)[0][0] + 1
        marks = sc.resume_pushes(c)
        steps = np.diff([0] + marks)
        assert marks[-1] == sc.inflated_size(c) and (steps > 0).all()
        assert steps[0] < stride and marks[1] == stride                             # less than a row; exactly one row
        assert max(steps) > 1000 * max(p + 1 for p, _, _ in sc.passes(c))           # thousands of rows
        assert sum(1 for m in marks[:-1] if m % stride) >= 3                        # pushes that end inside a row
        rows = sc.unfilter_input(c)
        assert sc.oracle_unfilter(c, rows)[0] == 0
        assert sc.oracle_unfilter(c, rows, marks[2])[0] == 0


@pytest.mark.parametrize("c", FILTER, ids=[c.name for c in FILTER])
def test_filter_case(c):
    src = sc.filter_source(c)
    assert len(src) == sc.storage_size(c)
    assert c.depth >= 8 or int(src.max()) < (1 << c.depth)
    rows = np.frombuffer(ph.orc_filter(src, *c.fmt), np.uint8)
    assert len(rows) == sc.inflated_size(c)
    st, back = sc.oracle_unfilter(c, rows)
    assert st == 0 and (back == src).all()
    pitch = max(p for p, _, _ in sc.passes(c))
    assert sc.filter_path(c, pitch, not c.interlaced) == c.kernel, (c.name, pitch)
    if c.kernel == "fast":
        assert pitch % 16 == 0 and (pitch > 2 * sc.FAST_STEP or c.height > sc.FILTER_GRID_ROWS)
    elif c.height == 260:
        assert (pitch % 16 != 0 and pitch > sc.FAST_STEP) if c.volume >= 8 else pitch in (sc.PACKED_ROW, sc.PACKED_ROW + 1)
    types = np.concatenate(sc.types_of(c, rows))
    assert types.max() <= 4
    if c.content == "synth" and c.volume >= 8:
        assert len(set(types.tolist())) >= 4, np.bincount(types, minlength=5)   # (what makes the image a test of the selection)
    if c.content == "zebra" and not c.interlaced:
        # noise under a zero row: Up scores what None scores and Paeth what Sub scores -- the first of a tie is taken, so neither
        # Up nor Paeth is ever written there; `<=` for `<` in the selection would write them
        assert not np.isin(types[1::2], (2, 4)).any()
        assert np.isin(types[1::2], (0, 1)).any()


def test_filter_table_reaches_every_path():
    plain = [c for c in FILTER if c.height == 260]
    for depth, ch in sc.FORMATS:
        mine = [c for c in plain if (c.depth, c.channels) == (depth, ch)]
        assert {c.content for c in mine} == set(sc.CONTENTS)
        assert {c.kernel for c in mine} == ({"fast", "generic"} if depth * ch >= 8 else {"packed", "generic"})
    # the carry between the 1 KiB steps of filter_row_fast for every pixel size
    assert {c.bpp for c in plain if c.kernel == "fast"} == {1, 2, 3, 4, 6, 8}
    assert all(sc.passes(c)[0][0] == sc.FAST_PITCH and sc.FAST_PITCH > 2 * sc.FAST_STEP for c in plain if c.kernel == "fast")
    tall = [c for c in FILTER if c.height > sc.FILTER_GRID_ROWS]
    assert {c.kernel for c in tall} == {"fast", "packed", "generic"} and all(c.width <= 100 for c in tall)
    assert {c.bpp if c.volume >= 8 else 0 for c in FILTER if c.interlaced} >= {0, 3, 8}
    batch = sc.filter_batch_cases()
    assert len(batch) >= 16 and {(c.depth, c.channels) for c in batch} == set(sc.FORMATS)
    assert any(c.interlaced for c in batch)
    for c in batch:
        src = sc.filter_source(c)
        rows = np.frombuffer(ph.orc_filter(src, *c.fmt), np.uint8)
        st, back = sc.oracle_unfilter(c, rows)
        assert st == 0 and (back == src).all(), c.name
