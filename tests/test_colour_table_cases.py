"""tests/colour_table_cases.py held to its own claims with numpy (no GPU): the distinct keys each case says its pixels have, the side
of each threshold it says it is on, the rule it says it plants.  Passes on its own by construction; it keeps the table honest for
tests/test_gpu_colour_tables.py."""
import numpy as np
import pytest

import colour_table_cases as ct
import indexing_ref as ref
import swift_png_amd as spng

CENSUS = [c for c in ct.CASES if c.kind == "census"]
MAPS = [c for c in ct.CASES if c.kind == "map"]


def test_the_table_s_numbers_are_the_binding_s():
    assert (ct.TILE, ct.MAP_LDS_KEYS, ct.WIDE_CAP) == (spng.CENSUS_WIDE_TILE, spng.MAP_LDS_KEYS, spng.CENSUS_WIDE_CAP)
    assert ct.TILE == spng.CENSUS_FINISH_LDS_KEYS and ct.MAP_LDS_KEYS == spng.PACK_INDEXED_LDS_KEYS
    assert len(set(ct.MISS.to_bytes(8, "little"))) == 8


def test_the_table_covers_what_it_promises():
    counts = {c.keys for c in CENSUS}
    assert {1, 4095, 4096, 4097, 65535, 65536, 65537, 131073, (1 << 20) + 1, 0} <= counts
    assert {c.cap for c in CENSUS if c.name.startswith("census/cap/")} == {65535, 65537}
    assert {c.offset for c in CENSUS if c.bits == 8 and c.layout == ct.RGBA} >= set(range(16))
    assert {(c.bits, c.layout, c.premultiply) for c in CENSUS} >= {(8, 0, 0), (8, 1, 0), (8, 2, 0), (16, 0, 0), (16, 1, 0), (16, 2, 0),
                                                                     (8, 0, 1), (16, 0, 1), (16, 0, 2), (8, 1, 1), (16, 1, 2)}
    assert {c.keys for c in MAPS} >= {0, 1, 511, 512, 513, 65536, 65537, 131073}
    for mc in (512, 513):
        assert {c.value_bytes for c in MAPS if c.keys == mc} == {1, 2, 4, 8}
    assert any(c.duplicate and c.keys > ct.MAP_LDS_KEYS for c in MAPS) and any(c.duplicate and c.keys <= ct.MAP_LDS_KEYS for c in MAPS)
    assert max(c.build().nbytes for c in CENSUS if c.name == "census/distinct/2^20+1") == 4 * ((1 << 20) + 4099)


@pytest.mark.parametrize("case", CENSUS, ids=lambda c: c.name)
def test_census_case_holds_its_claim(case):
    px = case.build()
    assert px.dtype == np.dtype(ct.dtype_of(case.bits)) and px.shape[1] == (4, 2, 1)[case.layout]
    keys, counts = ref.census(px, case.bits, case.layout, case.premultiply)
    if case.keys >= 0:
        assert len(keys) == case.keys
    assert int(counts.sum()) == len(px) and 1 <= case.cap <= ct.WIDE_CAP
    assert (case.offset * 8) % case.bits == 0 and 0 <= case.offset < 16
    if case.name.startswith("census/cap/"):
        assert len(keys) - case.cap == (1 if "/over/" in case.name else 0)
        k = ref.keys(px, case.bits, case.layout)
        first, last = k[:1024], k[-1024:]                         # what the first and the last workgroup read first
        if case.name.endswith("front"):
            assert len(np.unique(k[:len(keys)])) == len(keys) and len(np.unique(first)) == 1024
        else:
            assert len(np.unique(first)) == 1 and len(np.unique(last)) == 1024 and len(np.unique(k[:-len(keys)])) == 1
    if case.name.startswith("census/ends/"):
        want = {"both": {0, ct.MASK[case.layout]}, "zero": {0}, "ones": {ct.MASK[case.layout]}}[case.name.split("/")[2]]
        assert set(int(x) for x in keys) == want
    if case.name.startswith("census/bytes/"):
        varying = np.bitwise_or.reduce(keys ^ keys[0])
        assert varying == (0xFF if "/low/" in case.name else 0xFF << (24 if case.layout == ct.RGBA else 8))
    if case.name == "census/flat/70000":
        assert counts.max() == 70000 > 1 << 16
    if case.name == "census/duplication":
        assert len(px) == 200000
    if case.name == "census/cap-far-above":
        assert len(px) == 5 and case.cap == 1 << 24


@pytest.mark.parametrize("case", MAPS, ids=lambda c: c.name)
def test_map_case_holds_its_claim(case):
    px, keys, values = case.build()
    assert keys.dtype == np.uint32 and values.dtype == np.uint64 and len(keys) == len(values)
    if case.keys >= 0:
        assert len(keys) == case.keys
    assert (values >> np.uint64(8 * case.value_bytes - 1) >> np.uint64(1) == 0).all()
    steps = np.diff(keys.astype(np.int64))
    if case.duplicate:
        assert (steps >= 0).all() and int((steps == 0).sum()) == 1
        d = int(np.flatnonzero(steps == 0)[0])
        assert values[d] != values[d + 1] and (ref.keys(px, case.bits, case.layout)[:64] == keys[d]).all()
    else:
        assert (steps > 0).all()
    got, missed = ct.map_oracle(px, case, keys, values)
    assert len(got) == len(px)
    if case.misses >= 0:
        assert missed == case.misses == len(px)
    elif "/count/" in case.name:
        assert 0 < missed < len(px)                               # hits and misses both
    pk = ref.keys(px, case.bits, case.layout, case.premultiply)
    if "/ends/" in case.name:
        ends = {0, ct.MASK[case.layout]}
        assert ends <= set(int(x) for x in pk)
        assert (ends <= set(int(x) for x in keys)) == ("/present/" in case.name) and not (("/absent/" in case.name) and ends & set(int(x) for x in keys))
    if "/runs/" in case.name:
        assert len(set(pk[3:8])) == 1 and len(set(pk[1022:1029])) == 1 and len(set(pk[2046:3076])) == 1
    if "/offset/" in case.name:
        assert case.offset % 2 == 1
