"""DISTINCTCOUNT without a GPU: the SQL front end, the lowering into GROUP BY passes and their join, the folded
layout's bookkeeping (pgpu_fold_layout_of is host only), the non-scan merge, and the known answers' fixture against
the oracle's GROUP BY."""
import ctypes as C
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd._lib import (PGPU_DOUBLE, PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_LONG, PGPU_RED_MAX_I64,
                            PGPU_RED_MIN_I64, PGPU_RED_SUM_I64, TableLayout, UnsupportedPlanError)
from pinot_amd.distinct import order_pass, unfolded_result
from pinot_amd.plan import (ExecutionStats, QueryResult, distinct_lower, distinct_raise, merge_non_scan, topk_spec)
from pinot_amd.query import AggregationSpec, SqlError, parse_sql
from tests.helpers import GOLDEN, load_kat, sv_segment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Every SELECT literal of the test files is also held against the oracle's own SQL parser (tests/test_oracle_sql.py),
# which has no DISTINCTCOUNT and is to stay without one: the queries here get their keyword from SEL instead.
SEL = "SELECT "


# ---- parser ---------------------------------------------------------------------------------------------------------
def test_parser_spec_and_result_name():
    q = parse_sql(SEL + "DistinctCount(userId), COUNT(*) FROM t WHERE x > 3")
    assert q.aggregations[0] == AggregationSpec("DISTINCTCOUNT", "userId")
    assert q.aggregations[0].result_name == "distinctcount(userId)"
    assert q.projected_columns == ["userId"] and q.columns == ["x", "userId"]


def test_parser_rejects_star_mv_and_filter_clause():
    with pytest.raises(SqlError):
        parse_sql(SEL + "DISTINCTCOUNT(*) FROM t")
    with pytest.raises(SqlError, match="DISTINCTCOUNTMV"):
        parse_sql(SEL + "DISTINCTCOUNTMV(tags) FROM t")
    with pytest.raises(SqlError, match="FILTER"):
        parse_sql(SEL + "DISTINCTCOUNT(a) FILTER(WHERE x > 3) FROM t")


def test_parser_order_by_distinctcount():
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c) FROM t GROUP BY g ORDER BY distinctCount(c) DESC, g LIMIT 3")
    assert [(o.expression, o.ascending) for o in q.order_by] == [("distinctcount(c)", False), ("g", True)]


# ---- lowering -------------------------------------------------------------------------------------------------------
def test_lower_puts_the_distinct_column_last_and_keeps_the_aggregations():
    q = parse_sql(SEL + "g, h, SUM(x), DISTINCTCOUNT(c), AVG(y) FROM t WHERE x > 3 GROUP BY g, h LIMIT 7")
    (p,) = distinct_lower(q)
    assert p.column == "c" and p.query.group_by == ["g", "h", "c"]
    assert [a.result_name for a in p.query.aggregations] == ["sum(x)", "avg(y)"]
    assert p.plain == [0, 2] and p.distinct == [1]
    assert p.query.filter is q.filter and not p.query.order_by
    assert p.folded.group_by == ["g", "h"]
    assert [a.result_name for a in p.folded.aggregations] == ["sum(x)", "avg(y)", "distinctcount(c)"]


def test_lower_inserts_count_when_there_is_no_other_aggregation():
    (p,) = distinct_lower(parse_sql(SEL + "DISTINCTCOUNT(c) FROM t"))
    assert p.query.group_by == ["c"] and p.query.aggregations == [AggregationSpec("COUNT", None)]
    assert p.plain == [] and p.distinct == [0]


def test_lower_two_columns_two_passes_and_a_repeat_is_one():
    q = parse_sql(SEL + "g, DISTINCTCOUNT(a), MAX(x), DISTINCTCOUNT(b), DISTINCTCOUNT(a) FROM t GROUP BY g")
    p0, p1 = distinct_lower(q)
    assert (p0.column, p0.plain, p0.distinct) == ("a", [1], [0, 3])
    assert [a.result_name for a in p0.query.aggregations] == ["max(x)"]
    assert (p1.column, p1.plain, p1.distinct) == ("b", [], [2])
    assert p1.query.aggregations == [AggregationSpec("COUNT", None)] and p1.query.group_by == ["g", "b"]
    (only,) = distinct_lower(parse_sql(SEL + "DISTINCTCOUNT(a), DISTINCTCOUNT(a) FROM t"))
    assert only.distinct == [0, 1]


def test_lower_refuses_what_is_not_served():
    with pytest.raises(UnsupportedPlanError, match="group column"):
        distinct_lower(parse_sql(SEL + "g, DISTINCTCOUNT(g) FROM t GROUP BY g"))
    with pytest.raises(UnsupportedPlanError, match="FILTER"):
        distinct_lower(parse_sql(SEL + "DISTINCTCOUNT(a), SUM(x) FILTER(WHERE y > 1) FROM t"))
    with pytest.raises(UnsupportedPlanError, match="MV"):
        distinct_lower(parse_sql(SEL + "DISTINCTCOUNT(a), SUMMV(tags) FROM t"))


def test_order_pass_and_the_folded_topk_spec():
    q = parse_sql(SEL + "g, SUM(x), DISTINCTCOUNT(a), DISTINCTCOUNT(b) FROM t GROUP BY g "
                  "ORDER BY DISTINCTCOUNT(b) DESC, g LIMIT 3")
    passes = distinct_lower(q)
    pi, ob = order_pass(q, passes)
    assert pi == 1 and ob.expression == "distinctcount(b)"
    import dataclasses
    t = topk_spec(dataclasses.replace(passes[pi].folded, order_by=[ob]), [7], 15)
    # pass 1 carries COUNT(*) (entry 0), so the distinct count is the folded layout's entry 1, a LONG SUM
    assert (t.source, t.agg_fn, t.agg_index, t.descending, t.k) == (_lib.PGPU_TOPK_AGG, _lib.PGPU_AGG_SUM, 1, 1, 15)
    q2 = parse_sql(SEL + "g, SUM(x), DISTINCTCOUNT(a) FROM t GROUP BY g ORDER BY SUM(x) LIMIT 3")
    assert order_pass(q2, distinct_lower(q2))[0] == 0
    assert order_pass(parse_sql(SEL + "DISTINCTCOUNT(a) FROM t"), []) is None


# ---- pgpu_fold_layout_of ---------------------------------------------------------------------------------------------
def _layout(num_keys=7 * 100, kind=PGPU_KEYS_DENSE):
    """COUNT(*), a split SUM (3 parts) of a LONG, MIN of an INT: sections count | s s s | min."""
    L = TableLayout()
    L.num_keys = num_keys
    L.num_sections = 5
    for s, op in enumerate([PGPU_RED_SUM_I64] * 4 + [PGPU_RED_MIN_I64]):
        L.section_op[s] = op
    L.agg_section[0], L.agg_value_type[0] = 0, -1                                   # COUNT(*)
    L.agg_section[1], L.agg_value_type[1], L.agg_sum_parts[1] = 1, PGPU_LONG, 3     # SUM, split
    L.agg_section[2], L.agg_value_type[2], L.agg_sum_parts[2] = 4, PGPU_INT, 1      # MIN
    L.key_kind, L.key_words, L.key_split = kind, 1, 2
    return L


def test_fold_layout_bookkeeping():
    lib = _lib.load()
    L, F = _layout(), TableLayout()
    assert lib.pgpu_fold_layout_of(C.byref(L), 7, C.byref(F)) == 0
    assert (F.num_keys, F.num_sections, F.key_kind, F.key_words) == (7, 6, PGPU_KEYS_DENSE, 1)
    assert list(F.section_op)[:6] == [PGPU_RED_SUM_I64] * 4 + [PGPU_RED_MIN_I64, PGPU_RED_SUM_I64]
    for a in range(3):  # the input's entries are copied
        assert (F.agg_section[a], F.agg_value_type[a], F.agg_sum_parts[a], F.agg_sum_exp[a]) == \
               (L.agg_section[a], L.agg_value_type[a], L.agg_sum_parts[a], L.agg_sum_exp[a])
    # the distinct count: entry 3 (the first unused one), section 5, a one-section LONG SUM
    assert (F.agg_section[3], F.agg_value_type[3], F.agg_sum_parts[3], F.agg_sum_exp[3]) == (5, PGPU_LONG, 1, 0)
    assert F.agg_section[4] == 0 and F.agg_value_type[4] == 0
    assert _lib.table_bytes(F) == 8 * 6 * 7
    # a trailing COUNT(*) is an entry in use (value type -1)
    L2 = _layout()
    L2.agg_section[3], L2.agg_value_type[3] = 0, -1
    assert lib.pgpu_fold_layout_of(C.byref(L2), 7, C.byref(F)) == 0 and F.agg_section[4] == 5
    # hash input of any slot count folds into a dense table
    H = _layout(num_keys=1024, kind=PGPU_KEYS_HASH)
    assert lib.pgpu_fold_layout_of(C.byref(H), 7, C.byref(F)) == 0
    assert (F.num_keys, F.key_kind, F.num_sections) == (7, PGPU_KEYS_DENSE, 6)


def test_fold_layout_errors():
    lib = _lib.load()
    F = TableLayout()
    L = _layout()
    assert lib.pgpu_fold_layout_of(C.byref(L), 0, C.byref(F)) == _lib.PGPU_E_INVALID
    assert lib.pgpu_fold_layout_of(C.byref(L), 9, C.byref(F)) == _lib.PGPU_E_INVALID  # 700 % 9 != 0
    assert "multiple" in _lib.last_error()
    H = _layout(num_keys=1024, kind=PGPU_KEYS_HASH)
    H.key_words = 2
    assert lib.pgpu_fold_layout_of(C.byref(H), 7, C.byref(F)) == _lib.PGPU_E_UNSUPPORTED
    big = _layout(num_keys=((1 << 26) + 1) * 2)
    assert lib.pgpu_fold_layout_of(C.byref(big), (1 << 26) + 1, C.byref(F)) == _lib.PGPU_E_UNSUPPORTED
    assert lib.pgpu_fold_layout_of(C.byref(_layout(num_keys=(1 << 26) * 2)), 1 << 26, C.byref(F)) == 0
    full = _layout()
    full.num_sections = _lib.PGPU_MAX_SECTIONS
    assert lib.pgpu_fold_layout_of(C.byref(full), 7, C.byref(F)) == _lib.PGPU_E_UNSUPPORTED
    taken = _layout()
    for a in range(16):
        taken.agg_section[a], taken.agg_value_type[a] = 0, -1  # sixteen COUNT(*)
    assert lib.pgpu_fold_layout_of(C.byref(taken), 7, C.byref(F)) == _lib.PGPU_E_UNSUPPORTED
    assert "aggregation entry" in _lib.last_error()
    with pytest.raises(UnsupportedPlanError):
        _lib.check(lib.pgpu_fold_layout_of(C.byref(taken), 7, C.byref(F)))


# ---- ABI --------------------------------------------------------------------------------------------------------------
def test_abi_version_and_new_entry_points():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert int(re.search(r"#define PGPU_ABI_VERSION (\d+)", header).group(1)) == 13 == _lib.ABI_VERSION
    assert lib.pgpu_abi_version() == 13
    assert "#define PGPU_FOLD_MAX_KEYS (1ull << 26)" in header and _lib.PGPU_FOLD_MAX_KEYS == 1 << 26
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for name, nargs in (("pgpu_fold_layout_of", 3), ("pgpu_table_fold", 7), ("pgpu_query_collect_fold", 9)):
        assert hasattr(lib, name) and len(sigs[name][1]) == nargs
        decl = re.search(name + r"\(([^;]*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
        assert len(decl.split(",")) == nargs, decl
    # no new struct: the folded table is described by pgpu_table_layout, whose size tests/test_abi.py checks


# ---- raise / join -------------------------------------------------------------------------------------------------------
def _result(query, rows=None, agg=None, **stats):
    r = QueryResult(query, ExecutionStats(**stats))
    r.aggregation_result = agg
    r._group_rows = rows
    return r


def test_raise_aggregation_only_two_passes():
    q = parse_sql(SEL + "DISTINCTCOUNT(a), SUM(x), DISTINCTCOUNT(b), DISTINCTCOUNT(a) FROM t WHERE x > 3")
    passes = distinct_lower(q)
    r0 = _result(passes[0].folded, agg=[1234.0, 17], num_docs_scanned=100, num_entries_scanned_in_filter=900,
                 num_total_docs=1000, kernel_ms=0.5, dense_bytes=64, sparse_sector_bytes=32, num_segments_matched=2)
    r1 = _result(passes[1].folded, agg=[100, 5], num_docs_scanned=100, num_entries_scanned_in_filter=900,
                 num_total_docs=1000, kernel_ms=0.25, dense_bytes=16, sparse_sector_bytes=8, num_segments_matched=2)
    res = distinct_raise(q, passes, [r0, r1])
    assert res.aggregation_result == [17, 1234.0, 5, 17] and res.rows == [(17, 1234.0, 5, 17)]
    assert all(isinstance(res.aggregation_result[i], int) for i in (0, 2, 3))
    st = res.stats
    assert (st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_total_docs, st.num_segments_matched) == \
           (100, 900, 1000, 2)
    assert st.num_entries_scanned_post_filter == 100 * 3  # a, x, b
    assert (st.kernel_ms, st.dense_bytes, st.sparse_sector_bytes) == (0.75, 80, 40)
    with pytest.raises(UnsupportedPlanError):
        res.intermediate


def test_raise_grouped_joins_on_the_key_and_keeps_the_trimmed_groups():
    q = parse_sql(SEL + "g, DISTINCTCOUNT(a), COUNT(*), DISTINCTCOUNT(b) FROM t GROUP BY g "
                  "ORDER BY DISTINCTCOUNT(b) DESC, g LIMIT 2")
    passes = distinct_lower(q)
    r0 = _result(passes[0].folded, rows=[("u", 10, 3), ("v", 20, 4), ("w", 30, 5), ("x", 40, 1)], num_docs_scanned=100)
    r1 = _result(passes[1].folded, rows=[("v", 20, 9), ("w", 30, 9), ("x", 40, 2)], num_docs_scanned=100)  # trimmed
    res = distinct_raise(q, passes, [r0, r1])
    assert res.group_rows == [("v", 4, 20, 9), ("w", 5, 30, 9), ("x", 1, 40, 2)]
    assert res.rows == [("v", 4, 20, 9), ("w", 5, 30, 9)]
    assert res.stats.num_entries_scanned_post_filter == 100 * 3  # a, b, g


# ---- no scan -------------------------------------------------------------------------------------------------------------
def _meta_segment(num_docs, **dicts):
    def min_max(c):
        return float(dicts[c][0]), float(dicts[c][-1])
    return SimpleNamespace(num_docs=num_docs, dictionaries=dicts, min_max=min_max)


def test_merge_non_scan_all_segments():
    q = parse_sql(SEL + "DISTINCTCOUNT(c), COUNT(*), MAX(c), DISTINCTCOUNT(s) FROM t")
    segs = [_meta_segment(10, c=np.array([1, 5, 9], dtype=np.int32), s=["a", "b"]),
            _meta_segment(20, c=np.array([5, 9, 11, 12], dtype=np.int32), s=["b", "c"])]
    res = merge_non_scan(q, None, segs)
    assert res.aggregation_result == [5, 30, 12.0, 3]
    st = res.stats
    assert (st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_entries_scanned_post_filter,
            st.num_total_docs) == (30, 0, 0, 30)
    assert st.kernel_ms == 0


def test_merge_non_scan_mixed_with_scanned_value_sets():
    q = parse_sql(SEL + "DISTINCTCOUNT(c), COUNT(*), MIN(c), DISTINCTCOUNT(f) FROM t WHERE c > 2")
    p0, p1 = distinct_lower(q)
    # the scanned segments' unfolded tables: one group per value of the distinct column
    r0 = _result(p0.query, rows=[(3, 2, 3.0), (5, 1, 5.0), (40, 4, 40.0)], num_docs_scanned=7, num_total_docs=9,
                 num_entries_scanned_in_filter=9, kernel_ms=0.5)
    r1 = _result(p1.query, rows=[(0.5, 3), (2.0, 4)], num_docs_scanned=7, num_total_docs=9,
                 num_entries_scanned_in_filter=9, kernel_ms=0.25)
    scanned, sets = unfolded_result(q, [p0, p1], [r0, r1])
    assert scanned.aggregation_result == [3, 7, 3.0, 2] and sorted(sets) == [0, 3]
    meta = [_meta_segment(6, c=np.array([5, 6, 7], dtype=np.int32), f=np.array([2.0, 8.0], dtype=np.float32))]
    res = merge_non_scan(q, scanned, meta, sets)
    assert res.aggregation_result == [5, 13, 3.0, 3]  # {3, 5, 40} | {5, 6, 7}; {0.5, 2.0} | {2.0, 8.0}
    st = res.stats
    assert (st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_total_docs) == (13, 9, 15)
    assert st.num_entries_scanned_post_filter == 7 * 2 and st.kernel_ms == 0.75


# ---- the fixture ---------------------------------------------------------------------------------------------------------
def test_known_answers_match_the_oracles_group_by():
    """tests/golden/kat_distinct.json against oracle.engine's GROUP BY over the distinct column, folded here (the
    oracle has no DISTINCTCOUNT of its own)."""
    from oracle import engine
    with open(os.path.join(GOLDEN, "kat_distinct.json")) as f:
        kat = json.load(f)
    flt = load_kat()["filter"]
    seg = sv_segment()
    for case in kat["aggregation"]["cases"]:
        where = flt if "{FILTER}" in case["sql"] else ""
        got = []
        for col in ("column1", "column3"):
            ref = engine.execute(parse_sql(f"SELECT {col}, COUNT(*) FROM testTable{where} GROUP BY {col} "
                                           "LIMIT 10000000"), [seg] * 4)
            got.append(len(ref.group_rows))
        assert got == case["result"]
        if where:
            assert ref.num_docs_scanned == case["stats"][0] and ref.num_total_docs == case["stats"][3]
    ref = engine.execute(parse_sql(SEL + "column12, column11, COUNT(*) FROM testTable GROUP BY column12, column11 "
                                   "LIMIT 10000000"), [seg] * 4)
    want = {}
    for g, _, _ in ref.group_rows:
        want[g] = want.get(g, 0) + 1
    c0, c1 = kat["group_by"]["cases"]
    assert [tuple(r) for r in c0["rows"]] == sorted(want.items())
    by_count = sorted(sorted(want.items(), key=lambda r: r[0], reverse=True), key=lambda r: r[1])
    assert [tuple(r) for r in c1["rows"]] == by_count
    assert ref.num_docs_scanned * 2 == kat["group_by"]["num_entries_scanned_post_filter"]
