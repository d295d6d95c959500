"""tests/metadata_ref.py -- the plain-Python yardstick of the chunk directory, the text entry and the metadata round trip -- held to
what pins it, without a GPU: the claims of the case table (tests/metadata_cases.py: every case names the field or error it must
produce), and the reference's own files: the restatement plus the checker under oracle/ (inflate, deflate at level 13) turns the
ancillary chunks of ImageMetadata.png, ImagesInMemory.png and BasicDecoding.png into exactly the chunks tests/golden/files.json
records for the files the reference wrote from them."""
import base64
import hashlib
import json
import struct

import pytest

import file_ref
import metadata_cases as mc
import metadata_ref as mr
import pnghelp as ph

FILES = json.loads((ph.GOLDEN / "files.json").read_text())
META = ph.GOLDEN / "metadata"
NEW_TIME = struct.pack(">HBBBBB", 1992, 8, 3, 0, 0, 0)           # Snippets/PNG/ImageMetadata.swift: the time it sets


def source_chunks(name):
    if (META / name).exists():
        return file_ref.parse((META / name).read_bytes())
    table = json.loads((META / "metadata.json").read_text())[name]
    return [(k.encode("latin-1"), base64.b64decode(v)) for k, v in table["chunks"]]


def recorded(name):
    """the ancillary chunks files.json records for a file the reference wrote, in file order (bKGD / tRNS / PLTE are the format's)"""
    entry = FILES["files"][name]
    return [(k.encode("latin-1"), base64.b64decode(FILES["blobs"][h])) for k, h in entry["before"] + entry["after"]]


def inflate(data):
    st, out, _, _ = ph.orc_inflate(data)
    assert st == 0
    return out


def deflate(data):
    return ph.orc_deflate(data, 13)


def set_time(fields):
    fields[b"tIME"] = NEW_TIME


ROUND_TRIPS = [("ImageMetadata.png", "ImageMetadata-newtime.png", set_time), ("ImagesInMemory.png", "ImagesInMemory.png.png", None),
               ("BasicDecoding.png", "BasicDecoding.v.png", None), ("BasicDecoding.png", "BasicDecoding.va.png", None)]


@pytest.mark.parametrize("source,written,edit", ROUND_TRIPS, ids=[r[1] for r in ROUND_TRIPS])
def test_the_restatement_and_the_oracle_reproduce_what_the_reference_wrote(source, written, edit):
    before, after = mr.reserialize(source_chunks(source), inflate, deflate, edit)
    assert before + after == recorded(written)
    if FILES["files"][written]["after"]:
        assert before == recorded(written)[:len(before)] and len(before) == len(FILES["files"][written]["before"])


def test_the_exif_text_of_the_tutorial_goes_the_way_the_issue_walked_it():
    kind, payload = source_chunks("ImageMetadata.png")[1]
    assert kind == b"zTXt" and len(payload) == 21085 and payload.startswith(b"Raw profile type exif\0\0")
    keyword, compressed, language, localized, content = mr.text_fields(kind, payload, inflate)
    assert (keyword, compressed, language, localized) == (b"Raw profile type exif", True, ["en"], b"")
    assert len(inflate(payload[23:])) == 37124 and len(content) >= 37124
    out = mr.itxt_head(keyword, compressed, language, localized) + deflate(content)
    assert len(out) == 19256 and out.startswith(b"Raw profile type exif\0\1\0en\0\0")
    assert hashlib.sha256(out).hexdigest()[:16] in FILES["blobs"] or out in [v for _, v in recorded("ImageMetadata-newtime.png")]


def test_push_rules():
    """PNG.Metadata.swift:98-108, 159-164, 190-194"""
    g = (b"gAMA", struct.pack(">I", 45455))
    with pytest.raises(mr.Duplicate):
        mr.reserialize([g, g], inflate, deflate)
    with pytest.raises(mr.Unexpected):
        mr.reserialize([(b"PLTE", bytes(3)), g], inflate, deflate)
    with pytest.raises(mr.Required):
        mr.reserialize([(b"hIST", bytes(2))], inflate, deflate)
    t = (b"tEXt", b"Title\0one")
    before, after = mr.reserialize([t, (b"prVt", b"x"), (b"sPLT", b"p"), t, (b"pHYs", bytes(9)), g], inflate, deflate)
    assert before == [g]
    assert after == [(b"pHYs", bytes(9)), (b"iTXt", b"Title\0\0\0en\0\0one"), (b"iTXt", b"Title\0\0\0en\0\0one"), (b"sPLT", b"p"), (b"prVt", b"x")]


# ---- the case table's claims -----------------------------------------------------------------------------------------------------
HEADS = mc.head_cases()


@pytest.mark.parametrize("case", HEADS, ids=[c.name for c in HEADS])
def test_head_claims(case):
    h = mr.parse_head(case.kind, case.payload)
    assert h.status == case.status
    if case.status == mr.DONE:
        want = tuple(g if w is None else w for w, g in zip(case.claim, h[2:]))
        assert tuple(h[2:]) == want and h.aux == 0
    else:
        assert h.aux == case.claim and h.body_off == 0 and h.compressed == 0


def test_head_table_covers_every_status():
    seen = {c.status for c in HEADS}
    assert seen == {mr.DONE, mr.E_TEXT_KEYWORD, mr.E_TEXT_CHUNK_LENGTH, mr.E_TEXT_LANGUAGE, mr.E_TEXT_LOCALIZED_KEYWORD,
                    mr.E_TEXT_COMPRESSION_METHOD, mr.E_TEXT_COMPRESSION, mr.E_PROFILE_NAME, mr.E_PROFILE_CHUNK_LENGTH,
                    mr.E_PROFILE_COMPRESSION_METHOD}


def test_language_is_lower_cased_by_the_host():
    case = next(c for c in HEADS if b"EN-Latn-US" in c.payload)
    assert mr.language_of(case.payload, mr.parse_head(case.kind, case.payload)) == ["en", "latn", "us"]
    bad = next(c for c in HEADS if b"en-U5" in c.payload)
    assert mr.bad_language_tag(bad.payload, mr.parse_head(bad.kind, bad.payload)) == "U5"


def test_directory_claims():
    from lex_ref import lex_ref
    for case in mc.dir_cases():
        for i, data in enumerate(case.files):
            info, _ = lex_ref(data, len(data))
            if case.chunks is not None:
                assert info.chunks == case.chunks[i], case.name
            entries = mr.directory(data, info.chunks)
            assert len(entries) == info.chunks
            if info.status == 0:
                parsed = file_ref.parse(data)
                assert [(struct.pack(">I", e.type), data[e.offset:e.offset + e.length]) for e in entries] == parsed, case.name
    assert len(mc.pngsuite()) == 193


UTF8 = mc.utf8_cases()


@pytest.mark.parametrize("case", UTF8, ids=[c.name for c in UTF8])
def test_utf8_claims(case):
    st, first, count = mr.check_utf8(case.data)
    assert (None if st == mr.DONE else (first, count)) == case.claim
    assert st in (mr.DONE, mr.E_TEXT_ENCODING)
    assert case.data.decode("utf-8", "replace").count("\ufffd") == count


def test_transcode_claims():
    for case in mc.transcode_cases():
        out = mr.latin1_to_utf8(case.data)
        assert len(out) == len(case.data) + sum(b >= 0x80 for b in case.data), case.name
        assert out.decode("utf-8") == "".join(chr(b) for b in case.data)
    names = [c.name for c in mc.transcode_cases()]
    assert len(set(names)) == len(names)


# ---- the host mirror's PNG.Metadata, without a device: bodies by the oracle ------------------------------------------------------
@pytest.mark.parametrize("source,written,edit", ROUND_TRIPS, ids=[r[1] for r in ROUND_TRIPS])
def test_the_mirror_orders_and_serialises_as_the_reference(source, written, edit):
    from swift_png_amd.mirror import PNG
    m = PNG.Metadata()
    for kind, payload in source_chunks(source):
        name = kind.decode("latin-1")
        if name in ("IHDR", "IDAT", "IEND", "bKGD", "tRNS", "PLTE"):
            continue
        parsed = None
        if name in ("tEXt", "zTXt", "iTXt"):
            keyword, compressed, language, localized, content = mr.text_fields(kind, payload, inflate)
            parsed = PNG.Text(compressed, (keyword.decode("latin-1"), localized.decode("utf-8")), language, content.decode("utf-8"))
        elif name == "iCCP":
            h = mr.parse_head(kind, payload)
            parsed = PNG.ColorProfile(payload[:h.k].decode("latin-1"), inflate(payload[h.body_off:]))
        m.push((name, payload), palette_seen=False, parsed=parsed)
    if edit:
        assert m.time is not None
        m.time = (1992, 8, 3, 0, 0, 0)
    before, after = m.chunks([deflate(p) for p in m.to_deflate()])
    assert before + after == recorded(written)


def test_the_mirror_applies_the_push_rules():
    from swift_png_amd.mirror import PNG, DuplicateChunk, RequiredChunk, UnexpectedChunk
    g = ("gAMA", struct.pack(">I", 45455))
    m = PNG.Metadata()
    m.push(g)
    assert m.gamma == 45455
    with pytest.raises(DuplicateChunk):
        m.push(g)
    with pytest.raises(UnexpectedChunk):
        PNG.Metadata().push(g, palette_seen=True)
    with pytest.raises(RequiredChunk):
        PNG.Metadata().push(("hIST", bytes(2)))
    m.push(("pHYs", struct.pack(">IIB", 2835, 2835, 1)))
    m.push(("prVt", b"x"))
    m.push(("tIME", struct.pack(">HBBBBB", 2024, 1, 30, 22, 1, 56)))
    assert m.physicalDimensions == (2835, 2835, 1) and m.time == (2024, 1, 30, 22, 1, 56) and m.application == [("prVt", b"x")]
    assert m.chunks([]) == ([(b"gAMA", g[1])], [(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), (b"tIME", struct.pack(">HBBBBB", 2024, 1, 30, 22, 1, 56)),
                                                (b"prVt", b"x")])
