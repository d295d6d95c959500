"""Writes tests/golden/unpack_cases.json: one digest per group of the case table of tests/unpack_cases.py (names, palettes, inputs and
the oracle's answers), which tests/test_unpack_cases.py holds the table to.  Run by hand when the table or the oracle changes on
purpose:  python tests/golden/make_unpack_cases.py"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import unpack_cases as uc  # noqa: E402

if __name__ == "__main__":
    table = {group: uc.digest(cases) for group, cases in uc.groups().items()}
    (HERE / "unpack_cases.json").write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    print("%d groups, %d cases" % (len(table), len(uc.CASES)))
