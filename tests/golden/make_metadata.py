"""Writes tests/golden/metadata/: the source files of the reference's tutorials that read metadata and write it back.  Needs the
reference checkout (first argument, default pnghelp.REFERENCE), so it runs where that exists only; no test runs it.

    python tests/golden/make_metadata.py [REFERENCE]

Data the reference's programs read: ImageMetadata.png and ImagesInMemory.png whole (the inputs of Snippets/PNG/ImageMetadata.swift
and ImagesInMemory.swift); of BasicDecoding.png (1.8 MB) only the chunks that are not IDAT, in file order, as base64 in
metadata.json.  What the reference wrote from them -- ImageMetadata-newtime.png, ImagesInMemory.png.png, BasicDecoding.v.png / .va.png --
is in tests/golden/files.json already, ancillary chunks included."""
import base64
import json
import shutil
import struct
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pnghelp as ph  # noqa: E402

WHOLE = ("ImageMetadata/ImageMetadata.png", "ImagesInMemory/ImagesInMemory.png")
CHUNKS_ONLY = ("BasicDecoding/BasicDecoding.png",)


def chunks(data):
    pos = 8
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        yield data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        pos += 12 + n


def main():
    ref = Path(sys.argv[1]) if len(sys.argv) > 1 else ph.REFERENCE
    docs = ref / "Sources" / "PNG" / "docs.docc"
    out = ph.GOLDEN / "metadata"
    out.mkdir(exist_ok=True)
    table = {}
    for rel in WHOLE:
        shutil.copyfile(docs / rel, out / Path(rel).name)
        (out / Path(rel).name).chmod(0o644)
    for rel in CHUNKS_ONLY:
        data = (docs / rel).read_bytes()
        table[Path(rel).name] = {"source": "Sources/PNG/docs.docc/" + rel, "len": len(data),
                                 "chunks": [[k.decode("latin-1"), base64.b64encode(v).decode("ascii")] for k, v in chunks(data) if k != b"IDAT"]}
    (out / "metadata.json").write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
