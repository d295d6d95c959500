"""tests/file_ref.py -- the plain-Python yardstick of the file writer -- against the reference's own files, and tests/golden/files.json
against both.  The whole files the reference wrote that are committed under tests/golden/ are taken apart and written again from their
own pieces; every entry of files.json states the PLTE / bKGD / tRNS payloads its file holds, and file_ref derives the same from the
recorded inputs; where the reference checkout is present, the fixture's digests are its files'."""
import base64
import hashlib
import json

import pytest

import file_ref
import pnghelp as ph

FIXTURE = json.loads((ph.GOLDEN / "files.json").read_text())
FILES, BLOBS = FIXTURE["files"], {k: base64.b64decode(v) for k, v in FIXTURE["blobs"].items()}
COMMITTED = sorted((ph.GOLDEN / "encode").glob("*.swiftpng9.png")) + sorted((ph.GOLDEN / "tutorials").glob("*.png"))


def sha(data):
    return hashlib.sha256(data).hexdigest()


def inputs(e):
    """an entry of files.json -> what file_ref.head takes"""
    pal = BLOBS[e["palette"]] if e["palette"] else b""
    as_field = lambda v: None if v is None else v if isinstance(v, int) else tuple(v)
    return dict(width=e["width"], height=e["height"], depth=e["depth"], channels=e["channels"], indexed=e["indexed"], bgr=e["bgr"],
                interlaced=e["interlaced"], palette=[tuple(pal[k:k + 4]) for k in range(0, len(pal), 4)], key=as_field(e["key"]), fill=as_field(e["fill"]),
                before=[(n.encode("latin-1"), BLOBS[d]) for n, d in e["before"]], after=[(n.encode("latin-1"), BLOBS[d]) for n, d in e["after"]])


@pytest.mark.parametrize("path", COMMITTED, ids=lambda p: p.name)
def test_a_committed_file_from_its_own_pieces(path):
    data = path.read_bytes()
    p = file_ref.pieces(data)
    stream, chunk_bytes = p.pop("stream"), p.pop("chunk_bytes")
    assert file_ref.write(stream, chunk_bytes, **p) == data
    e = FILES.get(path.name.replace(".swiftpng9", ""))
    # (the files the reference wrote through compress are in the fixture: the same bytes from what the fixture records)
    if e is not None and e["sha256"] == sha(data):
        assert file_ref.SIG + file_ref.head(**inputs(e)) + file_ref.body(stream, e["chunk_bytes"]) + file_ref.chunk(b"IEND") == data
        assert (len(stream), sha(stream), -(-len(stream) // chunk_bytes)) == (e["idat_len"], e["idat_sha256"], e["idat_chunks"])


def test_the_committed_files_cover_the_fixture():
    """five of the integration tests' outputs and four of the tutorials' files are committed whole and are entries of the fixture"""
    hits = [p.name for p in COMMITTED if FILES.get(p.name.replace(".swiftpng9", ""), {}).get("sha256") == sha(p.read_bytes())]
    assert len([n for n in hits if n.endswith(".swiftpng9.png")]) == 5 and len(hits) >= 9


@pytest.mark.parametrize("name", sorted(FILES))
def test_expected_chunks_derive_from_the_recorded_inputs(name):
    e = FILES[name]
    kw = inputs(e)
    got = file_ref.derived(e["depth"], e["channels"], e["indexed"], e["bgr"], kw["palette"], kw["key"], kw["fill"])
    assert got == tuple(BLOBS[e[k]] if e[k] else None for k in ("plte", "bkgd", "trns"))
    head = file_ref.head(**kw)
    chunks = -(-e["idat_len"] // e["chunk_bytes"])
    assert chunks == e["idat_chunks"] and 8 + len(head) + e["idat_len"] + 12 * chunks + 12 == e["len"]
    # the order compress writes: the format's chunks between the two groups of blobs
    names = [n for n, _ in file_ref.parse(file_ref.SIG + head + file_ref.chunk(b"IEND"))][:-1]
    mid = [n for n, k in ((b"PLTE", "plte"), (b"bKGD", "bkgd"), (b"tRNS", "trns")) if e[k]]
    assert names == [b"CgBI"] * e["bgr"] + [b"IHDR"] + [n.encode() for n, _ in e["before"]] + mid + [n.encode() for n, _ in e["after"]]


def test_the_fixture_holds_what_the_issue_names():
    outputs = [n for n, e in FILES.items() if e["source"].startswith("Tests/Outputs/")]
    assert len(outputs) == 28 and all(FILES[n]["level"] == 9 for n in outputs)
    assert len([n for n in FILES if n.startswith("BasicEncoding-")]) == 8
    snaps = [n for n in FILES if n.startswith("OnlineDecoding") and n[:-4].rsplit("-", 1)[1].isdigit()]
    assert len(snaps) == 35 and len({json.dumps([FILES[n][k] for k in ("before", "after", "fill", "width", "height")]) for n in snaps}) == 1
    assert {"Indexing-indexed.png", "ImagesInMemory.png.png", "CustomColor-hue.png", "CustomColor-saturation.png", "CustomColor-value.png"} <= set(FILES)
    assert (ph.GOLDEN / "files.json").stat().st_size < 518000


def test_the_fixture_is_the_references_files():
    if not ph.REFERENCE.exists():
        pytest.skip("the reference checkout is not here")
    for name, e in FILES.items():
        data = (ph.REFERENCE / e["source"]).read_bytes()
        assert (len(data), sha(data)) == (e["len"], e["sha256"]), name
        idats = [d for n, d in file_ref.parse(data) if n == b"IDAT"]
        assert max(len(d) for d in idats) == e["chunk_bytes"] and len(idats) == e["idat_chunks"], name
