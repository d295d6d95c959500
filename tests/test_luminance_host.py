"""No GPU: what of spng_luminance_batch the host alone decides -- the desc's layout, the constants against the header, and what is
refused before any device is touched."""
import ctypes

import pytest

import pnghelp as ph
import swift_png_amd as spng


def test_struct_sizes_and_constants():
    assert ctypes.sizeof(spng.LuminanceDesc) == 32 and spng.LuminanceDesc.op.offset == 24 and spng.LuminanceDesc.reserved.offset == 25
    assert spng.K_LUMINANCE == 19 and (spng.LUMINANCE_V8, spng.LUMINANCE_VA8) == (1, 2)
    header = (ph.ROOT / "include" / "spng_mi355.h").read_text()
    assert "SPNG_K_LUMINANCE = 19" in header and "SPNG_LUMINANCE_V8 = 1, SPNG_LUMINANCE_VA8 = 2" in header
    assert {"spng_luminance_batch", "spng_luminance"} <= set(spng.EXPORTS)


def test_host_visible_refusals():
    """no context; pixels that are not whole or an unknown op in the Python layer"""
    lib = spng.load_library()
    d = (spng.LuminanceDesc * 1)(spng.LuminanceDesc(None, None, 0, spng.LUMINANCE_V8))
    res = (spng.Result * 1)()
    assert lib.spng_luminance_batch(None, d, 1, None, res) == spng.E_ARGUMENT
    assert lib.spng_luminance(None, None, 0, spng.LUMINANCE_VA8, None, res) == spng.E_ARGUMENT
    for pixels, op in ((b"\0" * 7, spng.LUMINANCE_V8), (b"\0" * 6, spng.LUMINANCE_VA8), (b"\0" * 8, 0), (b"\0" * 8, 3)):
        with pytest.raises(ValueError):
            spng.Session.luminance(None, pixels, op)
