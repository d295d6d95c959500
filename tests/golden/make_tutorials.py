"""Writes tests/golden/tutorials.json and copies four of the files the reference's tutorials wrote: needs the reference checkout
(first argument, default pnghelp.REFERENCE), so it runs where that exists only.

    python tests/golden/make_tutorials.py [REFERENCE]

The reference commits what its tutorials wrote under Sources/PNG/docs.docc/*/: streams of its own encoder at levels 0, 4, 8, 9 and
13, interlaced and CgBI ones among them (tests/tutorial_ref.py lists them with the level each tutorial states).  For every one: the
level, the format, the length and SHA-256 of its concatenated IDAT.  Data only: four files are copied to tests/golden/tutorials/
(the raster of BasicEncoding.rgba as an rgb8 file, the luminance the tutorial computed from it, and the two interlaced files) and
recorded by the SHA-256 of the whole file; the others are recorded by digest alone."""
import json
import shutil
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pnghelp as ph  # noqa: E402
import tutorial_ref as tr  # noqa: E402


def main():
    docs = Path(sys.argv[1]) / "Sources" / "PNG" / "docs.docc" if len(sys.argv) > 1 else tr.DOCS
    tr.COPIES.mkdir(exist_ok=True)
    table = {}
    for folder, name, level in tr.FILES:
        data = (docs / folder / name).read_bytes()
        png = ph.parse_png(data)
        table[name] = {"folder": folder, "level": level, "format": tr.format_name(png), "width": png.width, "height": png.height,
                       "interlaced": png.interlaced, "idat_len": len(png.idat), "idat_sha256": tr.sha(png.idat)}
        if name in tr.COPIED:
            shutil.copyfile(docs / folder / name, tr.COPIES / name)
            table[name]["file_len"] = len(data)
            table[name]["file_sha256"] = tr.sha(data)
    (HERE / "tutorials.json").write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
