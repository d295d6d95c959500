"""The yardstick of the typed chunks (tests/parse_ref.py) held to what the reference itself pins: its integration tests decode every
golden file outside invalid/, so no record of those may hold an error; ErrorHandling.swift:47-63 names the pixel format codes of five
invalid files; the ImageMetadata tutorial names its values; and every case of tests/parse_cases.py states what it must give."""
import pytest

import parse_cases as pc
import parse_ref as pr
import pnghelp as ph
from lex_ref import lex_ref

CASES = pc.cases()


def summary(data, cap=None):
    info, _ = lex_ref(data, len(data))
    n = info.chunks if cap is None else min(info.chunks, cap)
    return pr.parse_file(pr.chunks_of(data, n))


def test_no_golden_file_holds_an_error():
    """the cap is zero exceptions: the reference decodes all of these"""
    files = pc.golden_files()
    assert len(files) >= 200
    seen = {}
    for p in files:
        data = p.read_bytes()
        values, parsed = summary(data)
        assert parsed.status == pr.DONE and parsed.index == pr.NONE and parsed.ihdr_index != pr.NONE, p.name
        for (kind, _), v in zip(pr.chunks_of(data, len(values)), values):
            assert v.scope in (pr.SCOPE_NONE, pr.SCOPE_PARSED), (p.name, kind)
            if v.scope == pr.SCOPE_PARSED:
                seen[kind] = seen.get(kind, 0) + 1
    # every parser but sRGB's has met a file of the reference's
    assert set(seen) >= {b"IHDR", b"PLTE", b"tRNS", b"bKGD", b"hIST", b"gAMA", b"cHRM", b"sBIT", b"pHYs", b"tIME", b"sPLT"}, seen


@pytest.mark.parametrize("name,code", [("xc1n0g08", (8, 1)), ("xc9n2c08", (8, 9)), ("xd0n2c08", (0, 2)), ("xd3n2c08", (3, 2)), ("xd9n2c08", (99, 2))])
def test_invalid_color_format(name, code):
    """Sources/PNGIntegrationTests/ErrorHandling.swift:47-63"""
    _, parsed = summary((ph.GOLDEN / "invalid" / f"{name}.png").read_bytes())
    assert (parsed.index, parsed.status, parsed.aux) == (0, pr.E_HEADER_PIXEL_FORMAT_CODE, code)


def test_image_metadata_values():
    """what tests/test_gpu_metadata.py::test_image_metadata_tutorial asserts of the untyped decompress"""
    (path,) = [p for p in pc.golden_files() if p.name == "ImageMetadata.png"]
    data = path.read_bytes()
    values, parsed = summary(data)
    by_kind = {kind: v for (kind, _), v in zip(pr.chunks_of(data, len(values)), values)}
    assert by_kind[b"tIME"].v[:6] == (2024, 1, 30, 22, 1, 56)
    assert by_kind[b"gAMA"].v[0] == 45455 and by_kind[b"pHYs"].v[:3] == (2835, 2835, 1) and by_kind[b"bKGD"].v[:3] == (255, 255, 255)
    assert parsed.status == pr.DONE


def test_the_table_names_every_status():
    assert {c.expect[1] for c in CASES if c.expect} == set(pr.ALL) and len(pr.ALL) == 33


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(case):
    values, parsed = summary(case.file, case.cap)
    got = None if parsed.status == pr.DONE else (parsed.index, parsed.status, parsed.aux)
    assert got == case.expect
    assert (parsed.status == pr.DONE) == (parsed.index == pr.NONE)
    if case.scopes is not None:
        assert tuple(v.scope for v in values) == tuple(case.scopes)
    for v in values:                                             # a record that holds an error holds nothing else; unused words are zero
        if v.status != pr.DONE:
            assert v.scope == pr.SCOPE_PARSED and v.count == 0 and not any(v.v)
        if v.scope != pr.SCOPE_PARSED:
            assert v == pr.Value(pr.DONE, v.scope, (0, 0), 0, pr.NONE, (0,) * 8)
