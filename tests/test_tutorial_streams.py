"""No GPU: the CPU oracle's encoder against the streams the reference's own tutorials wrote (tests/golden/tutorials.json; the files
under Sources/PNG/docs.docc/*/ of the reference).  They pin the level table bit for bit at levels 0, 4, 8, 9 and 13 -- greedy, lazy
and both ends of the full search --, Adam7 encoding at 9 and 13, and, where the reference checkout is present, CgBI encoding; and
they hold the numpy restatement of BasicEncoding.swift's COMPUTE_LUMINANCE (tests/tutorial_ref.py) against the file the tutorial
wrote with it.  IDAT concatenations are compared: how the reference cuts them into chunks depends on its allocator."""
import json

import numpy as np
import pytest

import pnghelp as ph
import tutorial_ref as tr

TABLE = json.loads((ph.GOLDEN / "tutorials.json").read_text())
W, H = 638, 425


@pytest.fixture(scope="module")
def raster():
    """the tutorial's picture: the storage of the committed rgb8 file, (n, 3) uint8"""
    png = ph.parse_png((tr.COPIES / tr.RASTER).read_bytes())
    st, storage, _ = ph.orc_decode(png)
    assert st == 0 and (png.width, png.height, png.depth, png.color, png.interlaced) == (W, H, 8, 2, False)
    rgb = storage.reshape(-1, 3).copy()
    rgb.setflags(write=False)
    return rgb


@pytest.fixture(scope="module")
def luminance(raster):
    l = tr.luminance(raster)
    l.setflags(write=False)
    return l


def test_the_table_lists_every_file():
    assert sorted(TABLE) == sorted(name for _, name, _ in tr.FILES) and len(TABLE) == 17
    assert {TABLE[n]["level"] for n in TABLE} == {0, 4, 8, 9, 13}
    assert [TABLE[n]["format"] for n in tr.COPIED] == ["rgb8", "v8", "rgba8", "v8"]
    assert [TABLE[n]["interlaced"] for n in tr.COPIED] == [False, False, True, True]


@pytest.mark.parametrize("name", tr.COPIED)
def test_committed_copies_match_their_digests_and_reencode_to_themselves(name):
    data = (tr.COPIES / name).read_bytes()
    e = TABLE[name]
    assert (len(data), tr.sha(data)) == (e["file_len"], e["file_sha256"])
    png, idat = tr.reencode(data, e["level"])
    assert (tr.format_name(png), png.width, png.height, png.interlaced) == (e["format"], e["width"], e["height"], e["interlaced"])
    assert (len(png.idat), tr.sha(png.idat)) == (e["idat_len"], e["idat_sha256"])
    assert idat == png.idat


@pytest.mark.parametrize("level", sorted(tr.RGB_LEVELS))
def test_the_rgb_raster_at_every_level_the_tutorial_wrote(raster, level):
    e = TABLE[tr.RGB_LEVELS[level]]
    idat = tr.orc_encode(raster, W, H, 8, 3, False, 0, level)
    assert e["level"] == level and (len(idat), tr.sha(idat)) == (e["idat_len"], e["idat_sha256"])


def test_color_v_is_the_red_channel(raster):
    """PNG.Image.init(packing: rgba, layout: .v8) keeps r (BasicEncoding.swift:49-55)"""
    e = TABLE["BasicEncoding-color-v.png"]
    idat = tr.orc_encode(raster[:, 0], W, H, 8, 1, False, 0, 9)
    assert (len(idat), tr.sha(idat)) == (e["idat_len"], e["idat_sha256"])


def test_the_restated_luminance_is_the_tutorials(luminance):
    png = ph.parse_png((tr.COPIES / "BasicEncoding-luminance-v.png").read_bytes())
    st, storage, _ = ph.orc_decode(png)
    assert st == 0 and (png.width, png.height, png.depth, png.color) == (W, H, 8, 0)
    assert np.array_equal(storage, luminance)


@pytest.mark.parametrize("name,channels", [("BasicEncoding-luminance-v.png", 1), ("BasicEncoding-luminance-rgb.png", 3)])
def test_luminance_streams(luminance, name, channels):
    """the [UInt8] packed into v8 and into rgb8 (v replicated), level 9"""
    e = TABLE[name]
    idat = tr.orc_encode(np.repeat(luminance, channels), W, H, 8, channels, False, 0, 9)
    assert (len(idat), tr.sha(idat)) == (e["idat_len"], e["idat_sha256"])


def test_restatement_edges():
    """halves go away from zero (the first of the 38 colours that land on one), the clamp never bites below white"""
    assert tr.luminance(np.array([[0, 0, 0], [255, 255, 255], [0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=np.uint8)).tolist() == [0, 255, 0, 1, 1]
    c = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=1).astype(np.float64)
    l = np.sqrt(((0.299 * rgb[:, 0]) * rgb[:, 0] + (0.587 * rgb[:, 1]) * rgb[:, 1]) + (0.114 * rgb[:, 2]) * rgb[:, 2])
    halves = np.flatnonzero(l - np.floor(l) == 0.5)
    assert halves.size == 38
    got = tr.luminance(rgb[halves].astype(np.uint8))
    assert np.array_equal(got, np.floor(l[halves]) + 1) and (np.floor(l[halves]) % 2 == 0).any()    # (half-even would differ)


@pytest.mark.parametrize("folder,name,level", tr.FILES)
def test_every_tutorial_file_reencodes_to_its_own_stream(folder, name, level):
    if not tr.DOCS.is_dir():
        pytest.skip("no reference checkout")
    data = (tr.DOCS / folder / name).read_bytes()
    if name in tr.COPIED:
        assert data == (tr.COPIES / name).read_bytes()
    png, idat = tr.reencode(data, level)
    e = TABLE[name]
    assert (level, tr.format_name(png), len(png.idat), tr.sha(png.idat)) == (e["level"], e["format"], e["idat_len"], e["idat_sha256"])
    assert idat == png.idat
