"""No GPU: the numpy restatement of the HSVA tutorial (tests/hsva_ref.py; Snippets/PNG/CustomColor.swift) against the rasters the
reference itself wrote (tests/golden/customcolor.json: SHA-256 of the decoded RGB8 rasters of the tutorial's input and its four
outputs), the fixtures against the reference checkout where there is one, and what of spng_hsva_batch the host alone decides."""
import ctypes
import hashlib
import json

import numpy as np
import pytest

import hsva_ref
import pnghelp as ph
import swift_png_amd as spng

TABLE = json.loads((ph.GOLDEN / "customcolor.json").read_text())
FIXTURE = ph.GOLDEN / "customcolor" / "CustomColor.png"
OUTPUTS = ["CustomColor-hue.png", "CustomColor-saturation.png", "CustomColor-value.png", "CustomColor.png.png"]
REF_DIR = ph.REFERENCE / "Sources" / "PNG" / "docs.docc" / "CustomColor"


def _raster(path):
    png = ph.parse_png(path.read_bytes())
    st, storage, _ = ph.orc_decode(png)
    assert st == 0 and (png.width, png.height, png.depth, png.color) == (400, 588, 8, 2)
    return storage


@pytest.fixture(scope="module")
def unpacked():
    """the fixture as the tutorial's `image.unpack(as: HSVA.self)`: rgb8 gives a = .max"""
    rgb = _raster(FIXTURE).reshape(-1, 3)
    assert hashlib.sha256(rgb.tobytes()).hexdigest() == TABLE["CustomColor.png"]["sha256"]
    assert len(np.unique(rgb.astype(np.uint32) @ np.array([1, 256, 65536], dtype=np.uint32))) == 97388   # (too many for the census)
    return hsva_ref.from_rgba(np.concatenate([rgb, np.full((len(rgb), 1), 255, dtype=np.uint8)], axis=1))


@pytest.mark.parametrize("name", OUTPUTS)
def test_restatement_reproduces_the_references_outputs(unpacked, name):
    rgba, trap = hsva_ref.to_rgba(hsva_ref.tutorial_edits(unpacked)[name])
    assert not trap.any() and (rgba[:, 3] == 255).all()
    assert hashlib.sha256(rgba[:, :3].tobytes()).hexdigest() == TABLE[name]["sha256"]


def test_fixtures_are_the_references_files():
    if not REF_DIR.is_dir():
        pytest.skip("no reference checkout")
    assert FIXTURE.read_bytes() == (REF_DIR / "CustomColor.png").read_bytes()
    assert hashlib.sha256(FIXTURE.read_bytes()).hexdigest() == TABLE["CustomColor.png"]["file_sha256"]
    for name in ["CustomColor.png"] + OUTPUTS:
        assert hashlib.sha256(_raster(REF_DIR / name).tobytes()).hexdigest() == TABLE[name]["sha256"], name


def test_restatement_edges():
    """ties take the sector the switch gives them, grey is (0, 0, v, a), VA is (v, a) and not .rgba.r, a sector above 5 traps"""
    h = hsva_ref.from_rgba([[7, 7, 7, 1], [9, 9, 3, 2], [3, 9, 9, 3], [9, 3, 9, 4], [255, 0, 0, 5], [0, 0, 255, 6], [0, 0, 0, 7]])
    assert h["h"].tolist() == [0, 0 * 65537 + 65537, 2 * 65537 + 65537, 5 * 65537 + 0, 1, 4 * 65537 + 1, 0]    # (sectors 0, 0, 2, 5, 0, 4, 0)
    assert h["s"].tolist() == [0, 43690, 43690, 43690, 65535, 65535, 0] and h["v"].tolist() == [7, 9, 9, 9, 255, 255, 0]
    assert h["a"].tolist() == [1, 2, 3, 4, 5, 6, 7]
    p = np.array([(6 * 65537, 1, 200, 9), (6 * 65537 - 1, 65535, 200, 9), (2 ** 32 - 1, 0, 200, 9), (2 ** 32 - 1, 9, 0, 9)], dtype=hsva_ref.HSVA)
    rgba, trap = hsva_ref.to_rgba(p)
    assert trap.tolist() == [True, False, False, False]
    assert rgba.tolist() == [[200, 200, 200, 9], [200, 0, 0, 9], [200, 200, 200, 9], [0, 0, 0, 9]]
    assert hsva_ref.to_va(p).tolist() == [[200, 9], [200, 9], [200, 9], [0, 9]]


def test_struct_sizes_and_constants():
    assert ctypes.sizeof(spng.HsvaDesc) == 32 and spng.HsvaDesc.op.offset == 24 and spng.HsvaDesc.reserved.offset == 25
    assert hsva_ref.HSVA.itemsize == 8 and [hsva_ref.HSVA.fields[k][1] for k in "hsva"] == [0, 4, 6, 7]
    assert spng.K_HSVA == 18
    assert (spng.HSVA_FROM_RGBA8, spng.HSVA_TO_RGBA8, spng.HSVA_TO_VA8) == (1, 2, 3) == (hsva_ref.FROM_RGBA8, hsva_ref.TO_RGBA8, hsva_ref.TO_VA8)
    header = (ph.ROOT / "include" / "spng_mi355.h").read_text()
    assert "SPNG_K_HSVA = 18" in header and "SPNG_K_COUNT = 19" in header
    assert "SPNG_HSVA_FROM_RGBA8 = 1, SPNG_HSVA_TO_RGBA8 = 2, SPNG_HSVA_TO_VA8 = 3" in header
    assert {"spng_hsva_batch", "spng_hsva"} <= set(spng.EXPORTS)


def test_host_visible_refusals():
    """what is refused before any device is touched: no context; pixels that are not whole or an unknown op in the Python layer"""
    lib = spng.load_library()
    d = (spng.HsvaDesc * 1)(spng.HsvaDesc(None, None, 0, spng.HSVA_FROM_RGBA8))
    res = (spng.Result * 1)()
    assert lib.spng_hsva_batch(None, d, 1, None, res) == spng.E_ARGUMENT
    assert lib.spng_hsva(None, None, 0, spng.HSVA_TO_VA8, None, res) == spng.E_ARGUMENT
    for pixels, op in ((b"\0" * 7, spng.HSVA_FROM_RGBA8), (b"\0" * 12, spng.HSVA_TO_RGBA8), (b"\0" * 4, spng.HSVA_TO_VA8),
                       (b"\0" * 8, 0), (b"\0" * 8, 4)):
        with pytest.raises(ValueError):
            spng.Session.hsva(None, pixels, op)
