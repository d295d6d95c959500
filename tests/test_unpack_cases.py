"""No GPU: the case table of unpack_kernel / pack_kernel (tests/unpack_cases.py) held to what it claims -- every case's input does
what its reason says -- and the oracle's answers held to the digests of tests/golden/unpack_cases.json."""
import json

import numpy as np
import pytest

import geometry as geo
import pnghelp as ph
import unpack_cases as uc

GOLDEN = ph.GOLDEN / "unpack_cases.json"


def of(kind=None, **kw):
    return [c for c in uc.CASES if (kind is None or c.kind == kind) and all(getattr(c, k) == v for k, v in kw.items())]


def test_the_lines_the_shapes_are_built_around_are_still_there():
    for file, line in uc.SOURCE_LINES:
        assert line in (ph.ROOT / "swift_png_amd" / "csrc" / file).read_text(), (file, line)


def test_every_case_has_a_name_a_reason_and_a_valid_format():
    assert len({c.name for c in uc.CASES}) == len(uc.CASES)
    for c in uc.CASES:
        assert c.reason and c.kind in ("unpack", "pack") and c.bits in (8, 16) and c.layout in uc.LAYOUTS, c.name
        assert (c.depth, c.channels) in uc.FORMATS and (not c.bgr or (c.depth == 8 and c.channels >= 3)), c.name
        assert not c.indexed or (c.channels == 1 and c.depth <= 8 and 0 <= c.palette_count <= 256), c.name
        assert c.premultiply == 0 or (c.layout != uc.SCALAR and (c.bits == 16 or c.premultiply in (uc.P, uc.S))), c.name
        assert c.kind == "unpack" or c.premultiply in (0, uc.P, uc.P8), c.name
        # pixels of T lie on multiples of T
        assert (c.at[1] if c.kind == "unpack" else c.at[0]) % (c.bits // 8) == 0, c.name
        assert len(uc.source(c) if not c.huge else b"") == (0 if c.huge else c.storage_bytes if c.kind == "unpack" else c.pixel_bytes), c.name


def test_sizes_every_format_target_and_layout():
    """17 formats (11, bgr8 / bgra8, indexed 1, 2, 4, 8) x T = UInt8, UInt16 x three layouts at every size of SIZES; tails of 1, 2 and 3;
    several workgroups whose threads come round four times; 255, 256, 257 quads; pack: the same for the 13 formats without a
    palette, and 63 / 64 / 65 quads around a wave"""
    formats = list(uc._formats())
    assert len(formats) == 17
    assert {w * h % 4 for w, h in uc.TAILS + [(2, 1), (6, 1)]} == {1, 2, 3} and {w * h for w, h in uc.SIZES} >= {1, 3, 15, 257 * 31}
    for (w, h) in uc.TURNS:
        blocks, quads = geo.blocks_for(w * h, uc.PER_BLOCK), (w * h + 3) // 4
        assert blocks > 1 and 3 * blocks * uc.BLOCK < quads <= 4 * blocks * uc.BLOCK      # a fourth turn, for some threads the last full one
    assert [w * h // 4 for w, h in uc.WAVES] == [255, 256, 257] and all(w * h % 4 == 0 for w, h in uc.WAVES)
    assert sorted(w * h for w, h in uc.STAGED) == [252, 255, 256, 257, 260, 1021]
    for depth, channels, indexed, bgr in formats:
        for bits in (8, 16):
            for layout in uc.LAYOUTS:
                kw = dict(depth=depth, channels=channels, indexed=indexed, bgr=bgr, bits=bits, layout=layout, premultiply=0, at=(0, 0),
                          content="noise")
                assert {(c.width, c.height) for c in of("unpack", **kw)} >= set(uc.SIZES), kw
                if not indexed:
                    assert {(c.width, c.height) for c in of("pack", **kw)} >= set(uc.PACK_SIZES), kw


def test_one_case_each_way_above_the_cap_of_the_grid():
    huge = [c for c in uc.CASES if c.huge]
    assert sorted(c.kind for c in huge) == ["pack", "unpack"] and not [c for c in uc.CASES if not c.huge and c.n > 1 << 16]
    for c in huge:
        assert (c.depth, c.channels, c.bits, c.layout) == (8, 1, 8, uc.SCALAR)
        assert c.n > 4096 * uc.PER_BLOCK and geo.blocks_for(c.n, uc.PER_BLOCK) == 4096 and (c.n + 3) // 4 > 4 * 4096 * uc.BLOCK
        assert c.n % 4 == 0 and 16 << 20 < c.storage_bytes == c.pixel_bytes < 17 << 20


@pytest.mark.parametrize("case", of(content="keyed"), ids=lambda c: c.name)
def test_keyed_cases_hold_hits_and_every_near_miss(case):
    colors, hi = case.channels, 1 << case.depth
    key = np.array(case.key)
    sto = uc.storage(case)
    atoms = np.frombuffer(sto, dtype=">u2" if case.depth == 16 else np.uint8).astype(np.int64).reshape(-1, colors)
    same = atoms == key
    hits = same.all(axis=1)
    assert hits.any() and not hits.all()
    if case.depth >= 8:
        assert 0.03 < hits.mean() < 0.2                            # (about a tenth of 427 pixels)
    by_one = np.isin((atoms - key) % hi, (1, hi - 1))
    near = [by_one[:, z] & np.delete(same, z, axis=1).all(axis=1) for z in range(colors)]      # one channel off by one, the others equal
    assert all(m.any() for m in near)
    if case.depth >= 8:
        assert 0.03 < sum(m.mean() for m in near) < 0.2
    if case.depth == 16:
        high = ((atoms >> 8) == (key >> 8)).all(axis=1) & ((atoms & 255) != (key & 255)).all(axis=1)
        low = ((atoms & 255) == (key & 255)).all(axis=1) & ((atoms >> 8) != (key >> 8)).all(axis=1)
        assert 0.03 < (high & ~by_one.any(axis=1)).mean() < 0.2 and low.any()
    out = np.frombuffer(uc.expected(case), dtype="<u%d" % (case.bits // 8))
    if case.layout == uc.SCALAR:
        assert len(out) == case.n                                   # (no alpha: the key is ignored)
        return
    a = out.reshape(case.n, -1)[:, -1]
    assert ((a == 0) == hits).all() and (a[~hits] == (1 << case.bits) - 1).all()
    if colors == 3:
        swapped = (atoms == key[::-1]).all(axis=1)
        assert key[0] != key[2] and swapped.any() and not (swapped & hits).any()
        if case.bgr:                                                # (r, g, b) of these pixels equals the key; the storage tuple does not
            rgb = out.reshape(case.n, -1)[swapped]
            assert case.layout != uc.RGBA or ((rgb[:, :3] >> (case.bits - 8)) == key).all()
            assert (a[swapped] != 0).all()


def test_keys_for_every_grey_depth_and_the_colour_formats():
    keyed = of(content="keyed")
    assert {(c.depth, c.channels, c.bgr) for c in keyed} == {(1, 1, False), (2, 1, False), (4, 1, False), (8, 1, False), (16, 1, False),
                                                             (8, 3, False), (16, 3, False), (8, 3, True)}
    assert {(c.bits, c.layout) for c in keyed} == {(b, l) for b in (8, 16) for l in uc.LAYOUTS}


@pytest.mark.parametrize("case", of(content="beyond"), ids=lambda c: c.name)
def test_indexed_cases_hold_indices_on_both_sides_of_the_palette(case):
    idx = np.frombuffer(uc.storage(case), dtype=np.uint8)
    count = case.palette_count
    assert len(uc.palette(case)) == 4 * count
    assert (idx >= count).any() == (count < 256) and (idx < count).any() == (count > 0)
    for v in (count - 1, count, count + 1):
        assert not 0 <= v <= 255 or v in idx
    out = np.frombuffer(uc.expected(case), dtype="<u%d" % (case.bits // 8)).reshape(case.n, -1)
    assert (out[idx >= count] == 0).all()


def test_palettes_of_every_count_and_alphas_under_every_operation():
    assert {(c.depth, c.palette_count) for c in of(content="beyond")} == {(d, k) for d in (1, 2, 4, 8) for k in (0, 1, 1 << d, 256)}
    alphas = of(content="alphas")
    assert {(c.bits, c.premultiply, c.layout) for c in alphas} == \
        {(b, op, l) for b, ops in ((8, (uc.P, uc.S)), (16, (uc.P, uc.P8, uc.S, uc.S8))) for op in ops for l in (uc.RGBA, uc.VA)}
    for c in alphas:
        pal = np.frombuffer(uc.palette(c), dtype=np.uint8).reshape(-1, 4)
        used = pal[np.frombuffer(uc.storage(c), dtype=np.uint8)]
        assert set(used[:, 3]) == {0, 1, 254, 255} and (used[:, :3] != 0).all()
        assert uc.expected(c) != uc.expected(uc.Case(**{**c.__dict__, "premultiply": 0}))


def test_repeated_palette_colours_take_the_lowest_index():
    """the oracle refuses such a palette as the reference traps on it; the case's answer is the device's documented one"""
    cases = of("pack", content="repeats")
    assert {(c.depth, c.bits) for c in cases} == {(d, b) for d in (2, 8) for b in (8, 16)}
    for c in cases:
        pal = np.frombuffer(uc.palette(c), dtype=np.uint8).reshape(-1, 4)
        half = c.palette_count // 2
        assert (pal[half:] == pal[:half]).all() and len(np.unique(pal[:half], axis=0)) == half
        with pytest.raises(ValueError):
            uc.orc.pack(uc.pixels(c), c.depth, 1, indexed=True, palette=uc.palette(c))
        got = np.frombuffer(uc.expected(c), dtype=np.uint8)
        px = uc.pixels(c).astype(np.uint32) >> (c.bits - 8)
        assert (got < half).all() and len(set(got)) > half // 2
        held = np.array([(pal == p).all(axis=1).any() for p in px])
        assert held.any() and not held.all() and (pal[got[held]] == px[held]).all() and (got[~held] == 0).all()


def test_pack_into_indexed_formats_with_palettes_of_their_own():
    cases = of("pack", indexed=True, content="noise")
    assert {(c.depth, c.bits, c.layout) for c in cases} == {(d, b, l) for d in (1, 2, 4, 8) for b in (8, 16) for l in uc.LAYOUTS}
    assert len({uc.palette(c) for c in cases}) == len(cases)
    for c in cases:
        got = np.frombuffer(uc.expected(c), dtype=np.uint8)
        assert (got < c.palette_count).all() and (c.layout != uc.RGBA or len(set(got)) > c.palette_count // 2)
        px = uc.pixels(c).reshape(c.n, -1).astype(np.uint32) >> (c.bits - 8)
        entries = {tuple(e) for e in np.frombuffer(uc.palette(c), dtype=np.uint8).reshape(-1, 4)[:, {uc.RGBA: [0, 1, 2, 3], uc.VA: [0, 3], uc.SCALAR: [0]}[c.layout]]}
        strangers = np.array([tuple(p) not in entries for p in px])
        assert strangers.any() and not strangers.all() and (c.layout != uc.RGBA or (got[strangers] == 0).all())
        if c.layout == uc.RGBA:                                     # most strangers are an entry, not the first, of another case's palette
            others = [np.frombuffer(uc.palette(o), dtype=np.uint8).reshape(-1, 4) for o in cases if o is not c and o.bits == c.bits]
            assert sum(any((o[1:] == p).all(axis=1).any() for o in others) for p in px[strangers][:32]) >= 16


def test_offsets_reach_every_path_they_switch():
    """input and output, independently, 1, 2, 3, 4, 8 and 12 bytes behind a 16-byte boundary (pixels of UInt16 at even ones): the
    16-byte paths of rgba8 / bgra8 both ways, pack's rgb8 / bgr8 load, its dword stores, and the store through LDS of rgb8 (from both T)
    and rgb16"""
    moved = [c for c in uc.CASES if c.at != (0, 0)]
    assert all((c.width, c.height) == uc.OFFSET_SIZE and (c.at[0] == 0) != (c.at[1] == 0) for c in moved)
    n = uc.OFFSET_SIZE[0] * uc.OFFSET_SIZE[1]
    assert n % 4 == 3 and n // 4 > 2 * 64                           # two full waves and a partly filled one
    free, even = set(uc.OFFSETS[1:]), {o for o in uc.OFFSETS[1:] if o % 2 == 0}
    for kind, fmt, bits in (("unpack", (8, 4, False), 8), ("unpack", (8, 4, True), 8), ("unpack", (8, 3, False), 16), ("unpack", (16, 4, False), 16),
                            ("pack", (8, 4, False), 8), ("pack", (8, 4, True), 8), ("pack", (8, 3, False), 8), ("pack", (8, 3, True), 8),
                            ("pack", (8, 3, False), 16), ("pack", (16, 3, False), 8), ("pack", (16, 3, False), 16), ("pack", (8, 1, False), 8),
                            ("pack", (16, 4, False), 16), ("pack", (8, 2, False), 8)):
        for layout in uc.LAYOUTS:
            mine = [c for c in moved if c.kind == kind and (c.depth, c.channels, c.bgr) == fmt and c.bits == bits and c.layout == layout]
            pixel_side = 1 if kind == "unpack" else 0
            assert {c.at[pixel_side] for c in mine} - {0} == (free if bits == 8 else even), (kind, fmt, bits, layout)
            assert {c.at[1 - pixel_side] for c in mine} - {0} == free, (kind, fmt, bits, layout)


@pytest.mark.parametrize("group", sorted(uc.groups()))
def test_the_oracles_answers_are_stable(group):
    """the inputs and the oracle's answers of every case, group by group, against the digests kept in tests/golden/unpack_cases.json
    (written by tests/golden/make_unpack_cases.py, for a table that changed on purpose; no test writes them)"""
    assert json.loads(GOLDEN.read_text())[group] == uc.digest(uc.groups()[group])


def test_the_digests_are_of_this_table():
    assert sorted(json.loads(GOLDEN.read_text())) == sorted(uc.groups())
