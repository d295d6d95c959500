"""Host side of the indexed-colour path, without a GPU: the ctypes mirrors of spng_census_desc / spng_pack_indexed_desc have the
sizes and offsets the header gives them, the thresholds mirrored in the binding are the source's, pack(indexer=) /
unpack(deindexer=) tabulate closures as the reference would call them (device calls stubbed, compared with tests/indexing_ref.py),
and the gradient fixture is the reference's own file."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import indexing_ref as ref
import pnghelp as ph
import swift_png_amd as spng

CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
FIXTURE = ph.GOLDEN / "indexing" / "Indexing-gradient.png"


def test_struct_layouts_match_the_header(tmp_path):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    fields = {"spng_census_desc": spng.CensusDesc, "spng_pack_indexed_desc": spng.PackIndexedDesc}
    prints = "".join(f'printf("{n} %zu\\n", sizeof({n}));' +
                     "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for f, _ in c._fields_) for n, c in fields.items())
    src = tmp_path / "sizes.cpp"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "spng_mi355.h"\nint main() {{ {prints} return 0; }}\n')
    exe = tmp_path / "sizes"
    subprocess.run([CXX, "-I", str(ph.ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True, timeout=120)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for n, c in fields.items():
        assert int(got[n]) == ctypes.sizeof(c), n
        for f, _ in c._fields_:
            assert int(got[f"{n}.{f}"]) == getattr(c, f).offset, (n, f)
    assert ctypes.sizeof(spng.CensusDesc) == 40 and ctypes.sizeof(spng.PackIndexedDesc) == 56


def test_mirrored_thresholds_are_the_source_s():
    src = (ph.ROOT / "swift_png_amd" / "csrc" / "indexing.hip").read_text()
    for name in ("CENSUS_LDS_SLOTS", "CENSUS_LDS_LIMIT", "CENSUS_FINISH_LDS_KEYS", "PACK_INDEXED_LDS_KEYS"):
        m = re.search(r"static constexpr uint32_t %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == getattr(spng, name), name
    assert spng.K_CENSUS == 16 and spng.K_PACK_INDEXED == 17


class Stub(spng.Session):
    """a Session whose device calls are the numpy helper's"""

    def __init__(self):
        self.calls = []

    def census(self, pixels, bits, layout, cap=256, premultiply=0):
        self.calls.append(("census", cap))
        px = np.frombuffer(pixels, dtype="<u%d" % (bits // 8))
        k, n = ref.census(px, bits, layout, premultiply)
        if len(k) > cap:
            raise spng.SpngError(spng.E_OUTPUT_CAPACITY)
        return [int(x) for x in k], [int(x) for x in n]

    def pack_indexed(self, pixels, w, h, source, layout, keys, indices, miss=0, premultiply=0):
        self.calls.append(("pack_indexed", len(keys)))
        assert list(keys) == sorted(set(keys)) and len(keys) == len(indices)
        px = np.frombuffer(pixels, dtype="<u%d" % (source // 8))
        sto, missed = ref.pack_indexed(px, source, layout, keys, indices, miss, premultiply)
        return sto.tobytes(), missed


def nearest(palette):
    def index(c):
        return min(range(len(palette)), key=lambda i: sum((int(a) - int(b)) ** 2 for a, b in zip(palette[i], c)))
    return index


@pytest.mark.parametrize("bits", [8, 16])
def test_pack_with_an_rgba_indexer_calls_it_once_per_colour(bits):
    rng = np.random.default_rng(bits)
    palette = rng.integers(0, 256, (40, 4), dtype=np.uint8)
    colours = rng.integers(0, 1 << bits, (90, 4)).astype("<u%d" % (bits // 8))
    px = colours[rng.integers(0, 90, 64 * 9)]
    seen = []

    def indexer(entries):
        assert entries == [tuple(int(x) for x in e) for e in palette]
        inner = nearest(entries)

        def index(c):
            seen.append(c)
            return inner(c)
        return index
    s = Stub()
    got = s.pack(px.tobytes(), 64, 9, 8, 1, indexed=True, source=bits, palette=palette.tobytes(), indexer=indexer)
    k = ref.keys(px, bits, ref.RGBA)
    assert len(seen) == len(set(seen)) == len(np.unique(k))          # once per distinct colour
    want = bytes(nearest([tuple(int(x) for x in e) for e in palette])(ref.aggregate(x, ref.RGBA)) for x in k)
    assert got == want and s.calls == [("census", 65536), ("pack_indexed", len(seen))]


def test_pack_with_scalar_and_va_indexers_tabulates_every_argument():
    rng = np.random.default_rng(3)
    s = Stub()
    v = rng.integers(0, 256, 300, dtype=np.uint8)
    assert s.pack(v.tobytes(), 100, 3, 8, 1, indexed=True, source=8, layout=spng.TARGET_SCALAR, palette=b"", indexer=lambda _: int) == v.tobytes()
    assert s.calls == [("pack_indexed", 256)]
    va = rng.integers(0, 65536, (200, 2)).astype("<u2")
    got = s.pack(va.tobytes(), 50, 4, 8, 1, indexed=True, source=16, layout=spng.TARGET_VA, palette=b"",
                 indexer=lambda _: (lambda c: (c[0] + c[1]) >> 1))
    assert got == (((va[:, 0] >> 8) + (va[:, 1] >> 8)) >> 1).astype(np.uint8).tobytes()
    assert s.calls[-1] == ("pack_indexed", 65536)


def test_an_index_that_does_not_fit_uint8_raises_and_too_many_colours_too():
    s = Stub()
    px = np.arange(8, dtype=np.uint8).reshape(2, 4)
    with pytest.raises(OverflowError):
        s.pack(px.tobytes(), 2, 1, 8, 1, indexed=True, source=8, palette=b"", indexer=lambda _: (lambda c: 256))
    with pytest.raises(OverflowError):
        s.pack(px.tobytes(), 2, 1, 8, 1, indexed=True, source=8, palette=b"", indexer=lambda _: (lambda c: -1))
    many = np.arange(70000, dtype="<u4").view(np.uint8)
    with pytest.raises(spng.SpngError) as e:
        s.pack(many.tobytes(), 70000, 1, 8, 1, indexed=True, source=8, palette=b"", indexer=lambda _: (lambda c: 0))
    assert e.value.status == spng.E_OUTPUT_CAPACITY
    with pytest.raises(ValueError):
        s.pack(px.tobytes(), 2, 1, 8, 3, source=8, indexer=lambda _: (lambda c: 0))


def test_deindexer_tables():
    pal = [(i, 255 - i, i ^ 85, 255) for i in range(256)]
    t = spng.tabulate_deindexer(lambda i: pal[i])
    assert t == bytes(x for e in pal for x in e)
    t = spng.tabulate_deindexer(lambda i: (i, 255 - i), spng.TARGET_VA)
    assert t[0::4] == bytes(range(256)) and t[3::4] == bytes(255 - i for i in range(256))
    t = spng.tabulate_deindexer(lambda i: i, spng.TARGET_SCALAR)        # the tutorial's UInt8.init
    assert t[0::4] == bytes(range(256))
    with pytest.raises(OverflowError):
        spng.tabulate_deindexer(lambda i: 300, spng.TARGET_SCALAR)
    assert spng.palette_entries(bytes(range(8))) == [(0, 1, 2, 3), (4, 5, 6, 7)]
    assert spng.key_aggregate(0x04030201, spng.TARGET_RGBA) == (1, 2, 3, 4) and spng.key_aggregate(0x0201, spng.TARGET_VA) == (1, 2)


def test_gradient_fixture():
    data = FIXTURE.read_bytes()
    assert len(data) == 247
    png = ph.parse_png(data)
    assert (png.width, png.height, png.depth, png.channels) == (256, 16, 8, 3)
    theirs = ph.REFERENCE / "Sources" / "PNG" / "docs.docc" / "Indexing" / "Indexing-gradient.png"
    if theirs.exists():
        assert theirs.read_bytes() == data
