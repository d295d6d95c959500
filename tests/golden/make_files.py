"""Writes tests/golden/files.json: the whole files the reference wrote through PNG.Image.compress(stream:level:hint:) and committed to its
checkout, as a yardstick for the device's file writer.  Needs the reference checkout (first argument, default pnghelp.REFERENCE), so it
runs where that exists only and is not run by the tests.

    python tests/golden/make_files.py [REFERENCE]

Data only.  For every file: its length and SHA-256, the largest IDAT as chunk_bytes (where the reference cut: twice the capacity its
output buffer got, an allocator fact -- 65544 at the default hint, 8200 at hint 4096) with the number of IDATs, length and SHA-256 of the
concatenated IDAT, the level its writer states, the IHDR / CgBI fields, the chunks in front of PLTE and behind tRNS as (type, blob), the
PLTE / bKGD / tRNS payloads as EXPECTED values, and the inputs they derive from -- palette (r, g, b, a), key, fill as PNG.Format
holds them, read back the way PNG.Format.recognize does (tests/file_ref.py: pieces).  Payloads are base64, stored once in a table keyed by
the first 16 hex digits of their SHA-256: the OnlineDecoding snapshots share one head.

In: Tests/Outputs/*.png (the integration tests' own output, level 9), the files of tests/tutorial_ref.py's list, the three
CustomColor-*.png and every OnlineDecoding-*-<n>.png snapshot.  Not candidates -- the reference did not write them with compress --: files
of several IDATs of 8192 bytes (BasicDecoding.png, CustomColor.png, OnlineDecoding.png ...)."""
import base64
import json
import re
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import file_ref  # noqa: E402
import pnghelp as ph  # noqa: E402
import tutorial_ref as tr  # noqa: E402


def main():
    ref = Path(sys.argv[1]) if len(sys.argv) > 1 else ph.REFERENCE
    docs = ref / "Sources" / "PNG" / "docs.docc"
    sources = [("Tests/Outputs/" + p.name, 9) for p in sorted((ref / "Tests" / "Outputs").glob("*.png"))]
    sources += [(f"Sources/PNG/docs.docc/{folder}/{name}", level) for folder, name, level in tr.FILES]
    sources += [(f"Sources/PNG/docs.docc/CustomColor/CustomColor-{k}.png", 9) for k in ("hue", "saturation", "value")]
    snaps = [p for p in (docs / "OnlineDecoding").glob("OnlineDecoding*-*.png") if re.search(r"-\d+\.png$", p.name)]
    sources += [("Sources/PNG/docs.docc/OnlineDecoding/" + p.name, 9) for p in sorted(snaps, key=lambda p: (p.name.rsplit("-", 1)[0], int(p.stem.rsplit("-", 1)[1])))]
    blobs, files = {}, {}

    def keep(data):
        if data is None:
            return None
        digest = tr.sha(data)[:16]
        blobs[digest] = base64.b64encode(data).decode()
        return digest

    for rel, level in dict(sources).items():
        data = (ref / rel).read_bytes()
        p = file_ref.pieces(data)
        idats = [d for n, d in file_ref.parse(data) if n == b"IDAT"]
        if len(idats) > 1 and max(len(d) for d in idats) == 8192:
            print("not written by compress:", rel)
            continue
        assert all(len(d) == p["chunk_bytes"] for d in idats[:-1]) and idats[-1]
        plte, bkgd, trns = file_ref.derived(p["depth"], p["channels"], p["indexed"], p["bgr"], p["palette"], p["key"], p["fill"])
        got = dict(file_ref.parse(data))
        assert (plte, bkgd, trns) == (got.get(b"PLTE"), got.get(b"bKGD"), got.get(b"tRNS")), rel
        files[Path(rel).name] = {
            "source": rel, "len": len(data), "sha256": tr.sha(data), "level": level, "chunk_bytes": p["chunk_bytes"], "idat_chunks": len(idats),
            "idat_len": len(p["stream"]), "idat_sha256": tr.sha(p["stream"]),
            "width": p["width"], "height": p["height"], "depth": p["depth"], "channels": p["channels"], "indexed": p["indexed"], "bgr": p["bgr"],
            "interlaced": p["interlaced"], "palette": keep(bytes(x for e in p["palette"] for x in e) if p["palette"] else None),
            "key": p["key"], "fill": p["fill"],
            "before": [[n.decode("latin-1"), keep(d)] for n, d in p["before"]], "after": [[n.decode("latin-1"), keep(d)] for n, d in p["after"]],
            "plte": keep(plte), "bkgd": keep(bkgd), "trns": keep(trns)}
        assert file_ref.write(p["stream"], p["chunk_bytes"], p["width"], p["height"], p["depth"], p["channels"], indexed=p["indexed"], bgr=p["bgr"],
                              interlaced=p["interlaced"], palette=p["palette"], key=p["key"], fill=p["fill"], before=p["before"], after=p["after"]) == data, rel
    out = HERE / "files.json"
    out.write_text(json.dumps({"blobs": blobs, "files": files}, indent=1, sort_keys=True) + "\n")
    print(len(files), "files,", len(blobs), "blobs,", out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
