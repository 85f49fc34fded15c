"""Records what pgpu_fold_layout_of / pgpu_select_layout_of / pgpu_mode_layout_of answer over a grid of inputs into
tests/golden/folded_layouts.json (host only: no device is opened).  tests/test_folded_layouts.py replays the record, so
the three functions can be rebuilt on shared code without any return code, message or layout byte moving.

    python -m tools.folded_layouts            # rewrite the record from the library as built

File: "calls" = [function, num_percentiles, reducers] (function 0 fold, 1 select, 2 mode); "outcomes" = [rc, text] with
text the last_error() of a refusal and the sha256 of the returned pgpu_table_layout's bytes of a success; "tables" =
[key_kind, key_words, num_sections, used_entries, num_keys, inner_keys, [outcome index per call]].
"""
from __future__ import annotations

import ctypes as C
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pinot_amd import _lib  # noqa: E402
from pinot_amd._lib import PGPU_FOLD_MAX_KEYS, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_RED_SUM_I64, TableLayout  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "folded_layouts.json")
FOLD, SELECT, MODE = 0, 1, 2
PERCENTILES = (-1, 0, 1, 8, 9)
REDUCERS = (-1, 0, 1, 2, 3, 4, 7, 8)
CALLS = ([[FOLD, 0, 0]] + [[SELECT, k, 0] for k in PERCENTILES] +
         [[MODE, k, r] for k in PERCENTILES for r in REDUCERS])


def table(key_kind: int, key_words: int, num_sections: int, used_entries: int, num_keys: int) -> TableLayout:
    """`used_entries` COUNT(*) entries over `num_sections` int64 SUM sections."""
    L = TableLayout()
    L.num_keys, L.num_sections = num_keys, num_sections
    for s in range(min(num_sections, 17)):
        L.section_op[s] = PGPU_RED_SUM_I64
    for a in range(used_entries):
        L.agg_section[a], L.agg_value_type[a] = 0, -1
    L.key_kind, L.key_words = key_kind, key_words
    return L


def tables():
    """[key_kind, key_words, num_sections, used_entries, num_keys, inner_keys] of the grid."""
    for (kind, kw), nsec, used, inner in itertools.product(
            ((PGPU_KEYS_DENSE, 1), (PGPU_KEYS_HASH, 1), (PGPU_KEYS_HASH, 2)), (0, 1, 2, 12, 13, 16, 17, 18),
            (0, 1, 7, 8, 14, 15, 16), (0, 1, 9, PGPU_FOLD_MAX_KEYS, PGPU_FOLD_MAX_KEYS + 1)):
        # 9 is the non-divisor; every other inner divides num_keys, so that a dense table reaches the later checks
        yield [kind, kw, nsec, used, 2 * inner if inner > PGPU_FOLD_MAX_KEYS else 2 * PGPU_FOLD_MAX_KEYS, inner]


def answer(lib, tab, call) -> list:
    """[rc, text] of one call on one table against the loaded library."""
    kind, kw, nsec, used, num_keys, inner = tab
    fn, k, r = call
    L, F = table(kind, kw, nsec, used, num_keys), TableLayout()
    if fn == FOLD:
        rc = lib.pgpu_fold_layout_of(C.byref(L), inner, C.byref(F))
    elif fn == SELECT:
        rc = lib.pgpu_select_layout_of(C.byref(L), inner, k, C.byref(F))
    else:
        rc = lib.pgpu_mode_layout_of(C.byref(L), inner, k, r, C.byref(F))
    return [rc, hashlib.sha256(bytes(F)).hexdigest() if rc == 0 else _lib.last_error()]


def main() -> None:
    lib = _lib.load()
    outcomes, index, rows = [], {}, []
    for tab in tables():
        got = []
        for call in CALLS:
            out = answer(lib, tab, call)
            got.append(index.setdefault(tuple(out), len(index)))
            if got[-1] == len(outcomes):
                outcomes.append(out)
        rows.append(tab + [got])
    with open(GOLDEN, "w") as f:
        f.write('{"calls": %s,\n "outcomes": [\n' % json.dumps(CALLS, separators=(",", ":")))
        f.write(",\n".join("  " + json.dumps(o) for o in outcomes))
        f.write('\n ],\n "tables": [\n')
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    print(f"{len(rows) * len(CALLS)} cases, {len(outcomes)} outcomes, {os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")


if __name__ == "__main__":
    main()
