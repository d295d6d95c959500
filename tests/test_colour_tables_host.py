"""Host side of the colour tables without a ceiling (spng_census_wide_batch, spng_map_batch), without a GPU: the ctypes mirror of
spng_map_desc has the size and the offsets the header gives it, the thresholds mirrored in the binding are the source's, the four
entries are exported and declared, the kernel ids stay where they were, and Session.map_colours calls its function once, with the
ascending distinct keys (device calls stubbed with tests/indexing_ref.py)."""
import ctypes
import re
import shutil
import subprocess

import numpy as np
import pytest

import indexing_ref as ref
import pnghelp as ph
import swift_png_amd as spng

CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
HEADER = (ph.ROOT / "include" / "spng_mi355.h").read_text()
NAMES = ["spng_census_wide_batch", "spng_census_wide", "spng_map_batch", "spng_map"]


def test_map_desc_layout_matches_the_header(tmp_path):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    n, c = "spng_map_desc", spng.MapDesc
    prints = f'printf("{n} %zu\\n", sizeof({n}));' + "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f, _ in c._fields_)
    prints += 'printf("cap %d\\n", (int)SPNG_CENSUS_WIDE_CAP);'
    src = tmp_path / "sizes.cpp"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "spng_mi355.h"\nint main() {{ {prints} return 0; }}\n')
    exe = tmp_path / "sizes"
    subprocess.run([CXX, "-I", str(ph.ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[n]) == ctypes.sizeof(c) == 64
    for f, _ in c._fields_:
        assert int(got[f"{n}.{f}"]) == getattr(c, f).offset, f
    assert int(got["cap"]) == 1 << 24 == spng.CENSUS_WIDE_CAP


def test_mirrored_thresholds_are_the_source_s():
    src = (ph.ROOT / "swift_png_amd" / "csrc" / "colour_tables.hip").read_text()
    for name in ("CENSUS_WIDE_TILE", "MAP_LDS_KEYS", "MAP_LDS_SLOTS", "MAP_MIN_SLOTS"):
        m = re.search(r"static constexpr uint32_t %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == getattr(spng, name), name
    assert "SPNG_CENSUS_WIDE_CAP = 16777216" in HEADER and spng.CENSUS_WIDE_CAP == 1 << 24 == 16777216


def test_names_and_kernel_ids():
    for name in NAMES:
        assert name in spng.EXPORTS and re.search(r"\bint32_t %s\(" % name, HEADER), name
    assert spng.K_CENSUS == 16 and spng.K_PACK_INDEXED == 17
    assert "SPNG_K_CENSUS = 16" in HEADER and "SPNG_K_PACK_INDEXED = 17" in HEADER and "SPNG_K_COUNT = 19" in HEADER


def test_sort_launches():
    """one launch up to a tile; per stage above it one per stride of at least a tile, and one for the rest"""
    T = spng.CENSUS_WIDE_TILE
    assert [spng.census_wide_sort_launches(n) for n in (0, 1, T, T + 1, 2 * T, 2 * T + 1, 1 << 24)] == [1, 1, 1, 3, 3, 6, 91]


class Stub(spng.Session):
    """a Session whose device calls are the numpy helper's"""

    def __init__(self):
        self.calls = []

    def census_wide(self, pixels, bits, layout, cap=spng.CENSUS_WIDE_CAP, premultiply=0):
        self.calls.append(("census_wide", cap))
        k, n = ref.census(np.frombuffer(pixels, dtype="<u%d" % (bits // 8)), bits, layout, premultiply)
        assert len(k) <= cap
        return k, n

    def map(self, pixels, source, layout, keys, values, miss=0, premultiply=0):
        self.calls.append(("map", len(keys), values.dtype.itemsize))
        k = ref.keys(np.frombuffer(pixels, dtype="<u%d" % (source // 8)), source, layout, premultiply)
        at = np.searchsorted(keys, k)
        assert (keys[at] == k).all()
        return values[at], 0


def test_map_colours_calls_the_function_once_with_the_ascending_keys():
    rng = np.random.default_rng(5)
    colours = rng.integers(0, 256, (70001, 4), dtype=np.uint8)          # more colours than the old ceiling
    px = np.concatenate([colours, colours[rng.integers(0, len(colours), 19999)]])
    seen = []

    def fn(keys):
        seen.append(keys)
        return ((keys & 255) + (keys >> 24)).astype(np.uint16)
    s = Stub()
    out = s.map_colours(px.tobytes(), 8, spng.TARGET_RGBA, fn, np.uint16)
    want = np.unique(ref.keys(px, 8, ref.RGBA))
    assert len(seen) == 1 and seen[0].dtype == np.uint32 and (seen[0] == want).all() and len(want) > 65536
    assert out.dtype == np.uint16 and (out == px[:, 0].astype(np.uint16) + px[:, 3]).all()
    assert s.calls == [("census_wide", 90000), ("map", len(want), 2)]
    rec = np.dtype([("h", "<u4"), ("s", "<u2"), ("v", "u1"), ("a", "u1")])       # a structured dtype of 8 bytes
    out = s.map_colours(px[:100].tobytes(), 8, spng.TARGET_RGBA, lambda k: np.array([(x, 1, 2, 3) for x in k], dtype=rec), rec)
    assert out.dtype == rec and (out["h"] == ref.keys(px[:100], 8, ref.RGBA)).all() and (out["a"] == 3).all()
    for bad in (np.dtype("V3"), np.dtype([("a", "u1"), ("b", "<u2")]), np.dtype("<u2, <u4")):
        with pytest.raises(ValueError):
            s.map_colours(px.tobytes(), 8, spng.TARGET_RGBA, fn, bad)
    with pytest.raises(ValueError):
        s.map_colours(px.tobytes(), 8, spng.TARGET_RGBA, lambda k: np.zeros(3, dtype=np.uint8), np.uint8)    # not one item per key
    with pytest.raises(ValueError):
        s.map_colours(bytes(7), 8, spng.TARGET_RGBA, fn, np.uint16)


def test_host_visible_refusals():
    """what is refused before any device is touched"""
    lib = spng.load_library()
    res = (spng.Result * 1)()
    assert lib.spng_census_wide_batch(None, (spng.CensusDesc * 1)(), 1, None, res) == spng.E_ARGUMENT
    assert lib.spng_map_batch(None, (spng.MapDesc * 1)(), 1, None, res) == spng.E_ARGUMENT
    assert lib.spng_census_wide(None, None, 0, 8, 0, 0, 16, None, None, res) == spng.E_ARGUMENT
    assert lib.spng_map(None, None, 0, 8, 0, 0, None, None, 0, 1, None, None, res) == spng.E_ARGUMENT
    with pytest.raises(ValueError):
        spng.miss_bytes(b"\1\2\3", 2)
    assert spng.miss_bytes(0x0102, 2) == b"\2\1" and spng.miss_bytes(b"\7" * 8, 8) == b"\7" * 8
