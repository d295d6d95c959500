"""Writes tests/golden/customcolor.json and copies the tutorial's input: needs the reference checkout (first argument, default
pnghelp.REFERENCE), so it runs where that exists only.

    python tests/golden/make_customcolor.py [REFERENCE]

For Sources/PNG/docs.docc/CustomColor/CustomColor.png (the input of Snippets/PNG/CustomColor.swift) and the four files the
tutorial wrote from it, the SHA-256 of the decoded 400 x 588 RGB8 raster (decoded by the CPU oracle).  Data only: the input is
copied to tests/golden/customcolor/CustomColor.png, the outputs are recorded by digest."""
import hashlib
import json
import shutil
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pnghelp as ph  # noqa: E402

NAMES = ["CustomColor.png", "CustomColor-hue.png", "CustomColor-saturation.png", "CustomColor-value.png", "CustomColor.png.png"]


def raster_digest(path: Path):
    png = ph.parse_png(path.read_bytes())
    st, storage, _ = ph.orc_decode(png)
    assert st == 0 and (png.depth, png.color, png.interlaced) == (8, 2, False), (path, st, png.depth, png.color)
    return {"width": png.width, "height": png.height, "sha256": hashlib.sha256(storage.tobytes()).hexdigest()}


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else ph.REFERENCE) / "Sources" / "PNG" / "docs.docc" / "CustomColor"
    (HERE / "customcolor").mkdir(exist_ok=True)
    shutil.copyfile(ref / NAMES[0], HERE / "customcolor" / NAMES[0])
    table = {name: raster_digest(ref / name) for name in NAMES}
    table["CustomColor.png"]["file_sha256"] = hashlib.sha256((ref / NAMES[0]).read_bytes()).hexdigest()
    (HERE / "customcolor.json").write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
