"""Writes tests/golden/online.json and copies OnlineDecoding.png to tests/golden/tutorials/: needs the reference checkout (first
argument, default pnghelp.REFERENCE), so it runs where that exists only.

    python tests/golden/make_online.py [REFERENCE]

The reference's OnlineDecoding tutorial (Snippets/PNG/OnlineDecoding.swift) decodes two files as they arrive and writes the image after
every IDAT chunk: OnlineDecoding-{0..10}.png from OnlineDecoding.png, OnlineDecoding-progressive-{0..11}.png and, with overdraw,
OnlineDecoding-progressive-overdrawn-{0..11}.png from the interlaced OnlineDecoding-progressive.png -- 35 snapshots, committed under
Sources/PNG/docs.docc/OnlineDecoding/.  Data only: per run the input's name, its IDAT chunk lengths and, per snapshot, the SHA-256
of the storage the snapshot file decodes to (the checker under oracle/ decodes it); no snapshot is copied."""
import hashlib
import json
import shutil
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pnghelp as ph  # noqa: E402

FOLDER = "OnlineDecoding"
# run: (input file, overdraw, snapshots, the stem of the snapshot files)
RUNS = {"plain": ("OnlineDecoding.png", False, 11, "OnlineDecoding-"),
        "progressive": ("OnlineDecoding-progressive.png", False, 12, "OnlineDecoding-progressive-"),
        "progressive-overdrawn": ("OnlineDecoding-progressive.png", True, 12, "OnlineDecoding-progressive-overdrawn-")}
COPIES = ph.GOLDEN / "tutorials"


def derive(docs: Path) -> dict:
    """the table, from the reference's files under `docs` (Sources/PNG/docs.docc)"""
    table = {}
    for run, (name, overdraw, count, stem) in RUNS.items():
        data = (docs / FOLDER / name).read_bytes()
        png = ph.parse_png(data)
        snapshots = []
        for k in range(count):
            shot = ph.parse_png((docs / FOLDER / f"{stem}{k}.png").read_bytes())
            assert (shot.width, shot.height, shot.depth, shot.color) == (png.width, png.height, png.depth, png.color), (run, k)
            st, storage, _ = ph.orc_decode(shot)
            assert st == 0, (run, k, st)
            snapshots.append(hashlib.sha256(storage.tobytes()).hexdigest())
        table[run] = {"file": name, "file_len": len(data), "file_sha256": hashlib.sha256(data).hexdigest(), "overdraw": overdraw,
                      "width": png.width, "height": png.height, "depth": png.depth, "color": png.color, "interlaced": png.interlaced,
                      "idat_chunks": png.idat_chunks, "snapshots": snapshots}
    return table


def main():
    docs = (Path(sys.argv[1]) if len(sys.argv) > 1 else ph.REFERENCE) / "Sources" / "PNG" / "docs.docc"
    table = derive(docs)
    COPIES.mkdir(exist_ok=True)
    shutil.copyfile(docs / FOLDER / "OnlineDecoding.png", COPIES / "OnlineDecoding.png")
    (HERE / "online.json").write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
