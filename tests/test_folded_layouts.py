"""pgpu_fold_layout_of, pgpu_select_layout_of and pgpu_mode_layout_of (host only) against the record of what they
answered before they came to share one layout builder: every return code, every refusal's text and every byte of every
returned layout over the grid of tests/golden/folded_layouts.json (written by tools/folded_layouts.py)."""
import ctypes as C
import json

from pinot_amd import _lib
from pinot_amd._lib import TableLayout
from tools import folded_layouts as rec

# every refusal of the three functions but "null argument" (below) is in the record at least once
REFUSALS = ("fold over 0 inner keys", "table of 0 sections", "table of 18 sections", "are no multiple of",
            "two key words", "more than a collect returns", "no section left for the distinct count",
            "no aggregation entry left for the distinct count", "percentiles (1..8 are selected at once)",
            "no section left for 8 percentiles", "no aggregation entry left for 1 percentiles", "mode reducers 0x",
            "no section left for the 5 mode sections", "no aggregation entry left for the mode")


def test_every_recorded_layout_and_refusal_is_unchanged():
    lib = _lib.load()
    with open(rec.GOLDEN) as f:
        gold = json.load(f)
    # the record covers the grid the generator spells out, whole
    assert gold["calls"] == rec.CALLS
    assert [row[:-1] for row in gold["tables"]] == list(rec.tables())
    outcomes = gold["outcomes"]
    messages = " | ".join(text for rc, text in outcomes if rc != 0)
    for part in REFUSALS:
        assert part in messages, part
    wrong = []
    for row in gold["tables"]:
        for call, want in zip(gold["calls"], row[-1]):
            got = rec.answer(lib, row[:-1], call)
            if got != outcomes[want]:
                wrong.append((row[:-1], call, got, outcomes[want]))
    assert not wrong, f"{len(wrong)} cases differ, the first: {wrong[0]}"


def test_null_arguments_are_refused_first():
    lib = _lib.load()
    L, F = rec.table(_lib.PGPU_KEYS_DENSE, 1, 1, 1, 14), TableLayout()
    for a, b in ((None, C.byref(F)), (C.byref(L), None)):
        # (a bad mask and a bad number of percentiles behind it: the null argument is what is reported)
        for call in (lambda: lib.pgpu_fold_layout_of(a, 0, b), lambda: lib.pgpu_select_layout_of(a, 0, 9, b),
                     lambda: lib.pgpu_mode_layout_of(a, 0, 9, 8, b)):
            assert call() == _lib.PGPU_E_INVALID and _lib.last_error() == "null argument"
