"""Exact MODE without a GPU: the SQL front end and the shared result name, the lowering into the folded passes it shares
with DISTINCTCOUNT and PERCENTILE, the ORDER BY matched by function, column and reducer, the join that turns the mode
cells into values, and the mode layout's bookkeeping (pgpu_mode_layout_of is host only)."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd._lib import (PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_LONG, PGPU_RED_MIN_I64, PGPU_RED_SUM_F64,
                            PGPU_RED_SUM_I64, TableLayout, UnsupportedPlanError)
from pinot_amd.distinct import order_pass
from pinot_amd.plan import (ExecutionStats, GroupTable, QueryResult, distinct_lower, distinct_raise, finish, has_distinct,
                            topk_spec)
from pinot_amd.query import AggregationSpec, OrderByExpr, SqlError, parse_sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Every SELECT literal of the test files is also held against the oracle's own SQL parser (tests/test_oracle_sql.py),
# which has no MODE and is to stay without one: the queries here get their keyword from SEL instead.
SEL = "SELECT "


# ---- parser ---------------------------------------------------------------------------------------------------------
def test_parser_forms_default_reducer_and_result_name():
    q = parse_sql(SEL + "MODE(c) FROM t")
    assert q.aggregations == [AggregationSpec("MODE", "c", reducer="MIN")]
    q = parse_sql(SEL + "mode(c), Mode(c, 'MIN'), MODE(c, 'MAX'), MODE(c,'AVG'), MODE(d), COUNT(*) FROM t WHERE x > 3")
    a = q.aggregations
    assert [(s.function, s.column, s.reducer) for s in a[:5]] == [
        ("MODE", "c", "MIN"), ("MODE", "c", "MIN"), ("MODE", "c", "MAX"), ("MODE", "c", "AVG"), ("MODE", "d", "MIN")]
    assert a[0] == a[1] and a[0] != a[2]
    # BaseSingleInputAggregationFunction.getResultColumnName: the reducer is no part of the name
    assert [s.result_name for s in a] == ["mode(c)"] * 4 + ["mode(d)", "count(*)"]
    assert q.projected_columns == ["c", "d"] and q.columns == ["x", "c", "d"]
    # existing specs are unchanged by the new optional field
    assert a[5] == AggregationSpec("COUNT", None) and a[5].reducer is None
    assert AggregationSpec("SUM", "m") == AggregationSpec("SUM", "m", None, None, False, None)
    assert OrderByExpr("g") == OrderByExpr("g", True) and OrderByExpr("g").aggregation is None


@pytest.mark.parametrize("item,match", [
    ("MODE(c, 'min')", "quoted literals"), ("MODE(c, 'MEDIAN')", "quoted literals"), ("MODE(c, MIN)", "quoted literals"),
    ("MODE(c, 1)", "quoted literals"), ("MODE(c, '')", "quoted literals"), ("MODE(c, 'MIN', 'MAX')", "at most one"),
    ("MODE(c, 'AVG', 3)", "at most one"), ("MODEMV(tags)", "MODEMV"), ("MODEMV(tags, 'MAX')", "MODEMV"),
    ("MODE(c) FILTER(WHERE x > 3)", "MODE with FILTER"), ("MODE(c, 'MAX') FILTER(WHERE x > 3)", "MODE with FILTER"),
    ("MODE(*)", "identifier"), ("MODE()", "identifier")])
def test_parser_refuses(item, match):
    with pytest.raises(SqlError, match=match):
        parse_sql(SEL + item + " FROM t")


def test_parser_order_by_carries_the_aggregation():
    q = parse_sql(SEL + "g, MODE(c), MODE(c, 'MAX') FROM t GROUP BY g ORDER BY MODE(c, 'MAX') DESC, g LIMIT 3")
    assert [(o.expression, o.ascending) for o in q.order_by] == [("mode(c)", False), ("g", True)]
    assert q.order_by[0].aggregation == q.aggregations[1] and q.order_by[1].aggregation is None
    # other expressions are what they were
    q = parse_sql(SEL + "g, SUM(x) FROM t GROUP BY g ORDER BY SUM(x) DESC")
    assert q.order_by == [OrderByExpr("sum(x)", False)] and q.order_by[0].aggregation is None


# ---- lowering -------------------------------------------------------------------------------------------------------
def test_lower_every_reducer_of_one_column_is_one_pass():
    q = parse_sql(SEL + "g, MODE(c), MODE(c, 'MAX'), MODE(c, 'AVG') FROM t WHERE x > 3 GROUP BY g LIMIT 7")
    assert has_distinct(q)
    (p,) = distinct_lower(q)
    assert p.column == "c" and p.query.group_by == ["g", "c"] and p.folded.group_by == ["g"]
    assert [a.result_name for a in p.query.aggregations] == ["count(*)"]  # inserted: nothing else to carry
    assert (p.plain, p.distinct, p.percentile, p.mode) == ([], [], [], [0, 1, 2])
    assert p.reducers == _lib.PGPU_MODE_MIN | _lib.PGPU_MODE_MAX | _lib.PGPU_MODE_AVG == 7
    f = p.folded.aggregations
    assert [a.result_name for a in f] == ["count(*)", "distinctcount(c)", "mode(c)", "mode(c)", "mode(c)"]
    assert [a.reducer for a in f[2:]] == ["MIN", "MAX", "AVG"]
    assert p.query.filter is q.filter and not p.query.order_by


def test_lower_shares_the_pass_with_distinctcount_and_percentiles_of_the_column():
    q = parse_sql(SEL + "PERCENTILE(c, 33.3), MODE(c, 'MAX'), DISTINCTCOUNT(c), SUM(x), PERCENTILE99(c) FROM t")
    (p,) = distinct_lower(q)
    assert (p.plain, p.distinct, p.percentile, p.mode) == ([3], [2], [0, 4], [1])
    assert p.percentiles == [33.3, 99.0]
    # LO and HI are always laid out (MIN and MAX entries); S only for an AVG reducer
    assert [(a.function, a.reducer) for a in p.folded.aggregations[2:]] == [
        ("PERCENTILE", None), ("PERCENTILE", None), ("MODE", "MIN"), ("MODE", "MAX")]
    assert p.reducers == _lib.PGPU_MODE_MIN | _lib.PGPU_MODE_MAX
    assert [a.result_name for a in p.query.aggregations] == ["sum(x)"]


def test_lower_two_columns_two_passes():
    q = parse_sql(SEL + "g, SUM(x), MODE(a), PERCENTILE90(b), MODE(b, 'AVG'), MODE(a, 'MAX'), DISTINCTCOUNT(d) "
                  "FROM t GROUP BY g")
    p0, p1, p2 = distinct_lower(q)
    assert (p0.column, p0.plain, p0.distinct, p0.percentile, p0.mode) == ("a", [0], [], [], [1, 4])
    assert (p1.column, p1.plain, p1.distinct, p1.percentile, p1.mode) == ("b", [], [], [2], [3])
    assert (p2.column, p2.plain, p2.distinct, p2.percentile, p2.mode, p2.reducers) == ("d", [], [5], [], [], 0)
    assert p1.reducers == 7 and [a.reducer for a in p1.folded.aggregations[-3:]] == ["MIN", "MAX", "AVG"]


def test_lower_refuses_what_is_not_served():
    with pytest.raises(UnsupportedPlanError, match="MODE of the group column 'g'"):
        distinct_lower(parse_sql(SEL + "g, MODE(g) FROM t GROUP BY g"))
    with pytest.raises(UnsupportedPlanError, match=r"MODE in a query with FILTER"):
        distinct_lower(parse_sql(SEL + "MODE(a), SUM(x) FILTER(WHERE y > 1) FROM t"))
    with pytest.raises(UnsupportedPlanError, match=r"MODE together with \*MV"):
        distinct_lower(parse_sql(SEL + "MODE(a), SUMMV(tags) FROM t"))
    # the limit of 8 percentiles per column stands beside a MODE of the column
    nine = ", ".join(f"PERCENTILE{10 * k + 5}(a)" for k in range(9))
    with pytest.raises(UnsupportedPlanError, match="at most 8"):
        distinct_lower(parse_sql(SEL + "MODE(a), " + nine + " FROM t"))


def _maker_that_must_not_launch():
    """A GpuPlanMaker with no context whose prepare and launch steps fail the test when reached."""
    from pinot_amd.plan import GpuPlanMaker
    pm = object.__new__(GpuPlanMaker)
    pm._distinct, pm._prepared = {}, {}
    pm.collect_stats = pm.exact_filter_stats = pm.host_planning = False
    pm.gpu_topk, pm.query_flags, pm.min_server_group_trim_size = True, 0, 5000
    pm.num_groups_limit, pm.max_init_group_holder_capacity = 100_000, 10_000

    def reached(*a, **k):
        raise AssertionError("the query was prepared or launched")
    pm._prepare = pm._launch = pm.build_desc = reached
    return pm


def _stub_segment(uid, **columns):
    """A segment as check_distinct sees it: columns by name with is_mv / is_raw / data_type / cardinality."""
    from types import SimpleNamespace
    cols = {n: SimpleNamespace(is_mv=mv, is_raw=False, data_type=t, cardinality=7) for n, (t, mv) in columns.items()}
    return SimpleNamespace(uid=uid, name=f"s{uid}", column=cols.__getitem__, group_view=lambda n: n)


@pytest.mark.parametrize("sql", ["MODE(tags) FROM t", "g, SUM(x), MODE(tags, 'AVG') FROM t GROUP BY g"])
def test_multi_value_column_raises_before_anything_is_prepared_or_launched(sql):
    segs = [_stub_segment(i, tags=(PGPU_INT, True), x=(PGPU_INT, False), g=(PGPU_INT, False)) for i in range(2)]
    q = parse_sql(SEL + sql)
    pm = _maker_that_must_not_launch()
    for entry in (pm.submit, pm.execute):
        with pytest.raises(UnsupportedPlanError, match="MODE on a multi-value column 'tags'"):
            entry(q, segs)
    # the same maker does reach the prepare step for a single-value column: the stub proves something
    ok = [_stub_segment(i, tags=(PGPU_INT, False), x=(PGPU_INT, False), g=(PGPU_INT, False)) for i in range(2)]
    with pytest.raises(AssertionError, match="prepared or launched"):
        pm.submit(q, ok)


def test_string_column_key_space_and_avg_order_raise_before_anything_is_prepared_or_launched():
    from pinot_amd._lib import PGPU_STRING
    pm = _maker_that_must_not_launch()
    segs = [_stub_segment(0, s=(PGPU_INT, False), g=(PGPU_INT, False)),
            _stub_segment(1, s=(PGPU_STRING, False), g=(PGPU_INT, False))]  # STRING in any segment
    q = parse_sql(SEL + "g, MODE(s, 'MAX') FROM t GROUP BY g")
    for entry in (pm.submit, pm.execute):
        with pytest.raises(UnsupportedPlanError, match="MODE over the STRING column 's'"):
            entry(q, segs)
    ok = [_stub_segment(0, x=(PGPU_INT, False), g=(PGPU_INT, False))]
    with pytest.raises(UnsupportedPlanError, match=r"ORDER BY MODE\(x, 'AVG'\)"):
        pm.submit(parse_sql(SEL + "g, MODE(x, 'AVG') FROM t GROUP BY g ORDER BY MODE(x, 'AVG') LIMIT 3"), ok)
    pm.num_groups_limit = 7  # the key space of g (7) is not below it
    with pytest.raises(UnsupportedPlanError, match="MODE with a group key space of 7 .* numGroupsLimit"):
        pm.submit(parse_sql(SEL + "g, MODE(x) FROM t GROUP BY g"), ok)


def test_refused_by_the_multi_gpu_executors_and_the_mergeable_forms():
    from pinot_amd import combine, datatable, node
    q = parse_sql(SEL + "MODE(a, 'AVG') FROM t")
    for refuse in (combine._refuse_distinct, node._refuse_distinct, datatable._refuse_distinct):
        with pytest.raises(UnsupportedPlanError, match="MODE"):
            refuse(q)
        refuse(parse_sql(SEL + "SUM(a) FROM t"))
    with pytest.raises(UnsupportedPlanError, match="MODE"):
        QueryResult(q).intermediate


def test_a_mode_query_is_never_a_non_scan_plan():
    from types import SimpleNamespace

    from pinot_amd.plan import GpuPlanMaker
    seg = SimpleNamespace(num_docs=10)  # (never looked at: the function list decides first)
    for sql in ("MODE(a) FROM t", "COUNT(*), MAX(a), MODE(a, 'MAX') FROM t"):
        assert GpuPlanMaker.non_scan_segments(None, parse_sql(SEL + sql), [seg, seg]) == [False, False]


# ---- order ------------------------------------------------------------------------------------------------------------
def test_order_pass_matches_function_column_and_reducer():
    q = parse_sql(SEL + "g, SUM(x), MODE(a, 'MAX'), PERCENTILE90(b), MODE(b), MODE(b, 'MAX') FROM t "
                  "GROUP BY g ORDER BY MODE(b, 'MAX') DESC, g LIMIT 3")
    passes = distinct_lower(q)
    pi, ob = order_pass(q, passes)
    assert pi == 1 and ob.aggregation == AggregationSpec("MODE", "b", reducer="MAX")
    t = topk_spec(dataclasses.replace(passes[pi].folded, order_by=[ob]), [7], 15)
    # pass 1: COUNT(*) (entry 0), the distinct count (1), PERCENTILE90 (2), then LO (3) and HI (4)
    assert (t.source, t.agg_fn, t.agg_index, t.descending, t.k) == (_lib.PGPU_TOPK_AGG, _lib.PGPU_AGG_SUM, 4, 1, 15)
    # MODE(b) beside it is the other entry, MODE(a, 'MAX') the other pass
    q = parse_sql(SEL + "g, SUM(x), MODE(a, 'MAX'), PERCENTILE90(b), MODE(b), MODE(b, 'MAX') FROM t "
                  "GROUP BY g ORDER BY MODE(b) LIMIT 3")
    pi, ob = order_pass(q, distinct_lower(q))
    t = topk_spec(dataclasses.replace(distinct_lower(q)[pi].folded, order_by=[ob]), [7], 15)
    assert (pi, t.agg_index, t.descending) == (1, 3, 0)
    q = parse_sql(SEL + "g, SUM(x), MODE(a, 'MAX'), MODE(b) FROM t GROUP BY g ORDER BY MODE(a, 'MAX') LIMIT 3")
    pi, ob = order_pass(q, distinct_lower(q))
    t = topk_spec(dataclasses.replace(distinct_lower(q)[pi].folded, order_by=[ob]), [7], 15)
    assert (pi, t.agg_index) == (0, 3)  # pass 0: SUM (0), the distinct count (1), LO (2), HI (3)
    # the mean of several modes is no cell to trim by
    q = parse_sql(SEL + "g, MODE(a, 'AVG'), MODE(a) FROM t GROUP BY g ORDER BY MODE(a, 'AVG') LIMIT 3")
    with pytest.raises(UnsupportedPlanError, match=r"ORDER BY MODE\(a, 'AVG'\)"):
        order_pass(q, distinct_lower(q))
    # other expressions go where they went
    q2 = parse_sql(SEL + "g, SUM(x), MODE(a) FROM t GROUP BY g ORDER BY SUM(x) LIMIT 3")
    assert order_pass(q2, distinct_lower(q2))[0] == 0


# ---- raise / join -------------------------------------------------------------------------------------------------------
def _result(query, rows=None, agg=None, values=None, **stats):
    r = QueryResult(query, ExecutionStats(**stats))
    r.aggregation_result = agg
    r._group_rows = rows
    r.value_dictionary = values
    return r


def test_raise_aggregation_only_reducers_types_and_the_empty_result():
    q = parse_sql(SEL + "MODE(a, 'MAX'), SUM(x), MODE(a), MODE(a, 'AVG'), MODE(b) FROM t WHERE x > 3")
    passes = distinct_lower(q)
    big = (1 << 53) + 2  # a LONG beyond the doubles' integers: converted once, from the dictionary
    da = np.array([-5, 7, big, 1 << 62], dtype=np.int64)
    db = np.array([0.25, 0.5], dtype=np.float32)
    # folded rows: sum | distinct | LO | HI | S / T     and     count | distinct | LO | HI
    r0 = _result(passes[0].folded, agg=[12.0, 3, 1, 2, 4503599627370500.0], values=da, num_docs_scanned=10)
    r1 = _result(passes[1].folded, agg=[10, 2, 1, 1], values=db, num_docs_scanned=10)
    res = distinct_raise(q, passes, [r0, r1])
    assert res.aggregation_result == [float(big), 12.0, 7.0, 4503599627370500.0, 0.5]
    assert [type(v) for v in res.aggregation_result] == [float] * 5
    assert res.stats.num_entries_scanned_post_filter == 10 * 3  # a, x, b
    # nothing matched (M = 0: no id is tied, the distinct count is 0) -> DEFAULT_FINAL_RESULT
    r0 = _result(passes[0].folded, agg=[0.0, 0, 0, 0, -math.inf], values=da)
    r1 = _result(passes[1].folded, agg=[0, 0, 0, 0], values=db)
    assert distinct_raise(q, passes, [r0, r1]).aggregation_result == [-math.inf, 0.0, -math.inf, -math.inf, -math.inf]


def test_raise_grouped_joins_on_the_key_and_orders_by_the_right_reducer():
    q = parse_sql(SEL + "g, MODE(a), MODE(a, 'MAX'), COUNT(*) FROM t GROUP BY g ORDER BY MODE(a, 'MAX') DESC, g LIMIT 3")
    (p,) = distinct_lower(q)
    d = np.array([10, 20, 30], dtype=np.int32)
    rows = [("u", 4, 2, 0, 0), ("v", 5, 1, 1, 1), ("w", 6, 3, 0, 2), ("x", 7, 3, 2, 2), ("y", 8, 1, 0, 1)]  # g | count |
    res = distinct_raise(q, [p], [_result(p.folded, rows=rows, values=d, num_docs_scanned=30)])   # distinct | LO | HI
    # by the MAX reducer (the second mode(a)), not the first column of that name; ties broken by the key
    assert res.rows == [("w", 10.0, 30.0, 6), ("x", 30.0, 30.0, 7), ("v", 20.0, 20.0, 5)]
    assert all(type(r[1]) is float and type(r[2]) is float for r in res.group_rows)


def _mode_layout(avg):
    """COUNT(*) folded over 4 keys with the mode sections behind the distinct count: count | distinct | M T LO HI (S)."""
    lib = _lib.load()
    L, F = TableLayout(), TableLayout()
    L.num_keys, L.num_sections = 4 * 3, 1
    L.section_op[0] = PGPU_RED_SUM_I64
    L.agg_section[0], L.agg_value_type[0] = 0, -1
    L.key_kind, L.key_words = PGPU_KEYS_DENSE, 1
    assert lib.pgpu_mode_layout_of(C.byref(L), 4, 0, 7 if avg else 3, C.byref(F)) == 0
    return F


def test_finish_decodes_the_mode_sections_of_a_folded_table():
    """The folded pass's rows from hand-made cells: LO and HI as ids, S / T as a double, -inf where nothing is tied."""
    q = parse_sql(SEL + "g, MODE(a), MODE(a, 'AVG'), MODE(a, 'MAX') FROM t GROUP BY g")
    (p,) = distinct_lower(q)
    F = _mode_layout(avg=True)
    assert F.num_sections == 7
    s = np.array([2.5 + 4.5, 7.0], dtype=np.float64).view(np.int64)
    cells = np.array([[9, 3, 4, 2, 0, 2, s[0]],      # two ids tied at count 4
                      [5, 1, 5, 1, 1, 1, s[1]]], dtype=np.int64)
    res = finish(p.folded, GroupTable.sorted(np.array([0, 2], dtype=np.int64), cells, F), [np.array([5, 6, 7, 8])],
                 ExecutionStats())
    # g | count | distinct | LO | HI | S / T
    assert res.group_rows == [(5, 9, 3, 0, 2, 3.5), (7, 5, 1, 1, 1, 7.0)]
    assert [type(v) for v in res.group_rows[0]] == [int, int, int, int, int, float]
    res.value_dictionary = np.array([2.5, 3.0, 4.5])
    out = distinct_raise(q, [p], [res])
    assert out.group_rows == [(5, 2.5, 3.5, 4.5), (7, 3.0, 7.0, 3.0)]
    # aggregation only, nothing matched: the identities of every section
    q1 = parse_sql(SEL + "MODE(a, 'AVG'), MODE(a, 'MAX') FROM t")
    (p1,) = distinct_lower(q1)
    empty = GroupTable.sorted(np.zeros(0, dtype=np.int64), np.zeros((0, 7), dtype=np.int64), F)
    r1 = finish(p1.folded, empty, [], ExecutionStats())
    assert r1.aggregation_result == [0, 0, 0, 0, -math.inf]
    r1.value_dictionary = np.array([2.5, 3.0, 4.5])
    assert distinct_raise(q1, [p1], [r1]).aggregation_result == [-math.inf, -math.inf]


# ---- library ----------------------------------------------------------------------------------------------------------------
def test_abi_version_and_new_entry_points():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert int(re.search(r"#define PGPU_ABI_VERSION (\d+)", header).group(1)) == 13 == _lib.ABI_VERSION
    assert lib.pgpu_abi_version() == 13
    for name, value in (("PGPU_MODE_MIN", 1), ("PGPU_MODE_MAX", 2), ("PGPU_MODE_AVG", 4)):
        assert f"#define {name} {value}" in header and getattr(_lib, name) == value
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for name, nargs in (("pgpu_mode_layout_of", 5), ("pgpu_table_mode", 12), ("pgpu_query_collect_mode", 14)):
        assert hasattr(lib, name) and len(sigs[name][1]) == nargs
        decl = re.search(name + r"\(([^;]*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1)
        assert len(decl.split(",")) == nargs, decl


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


def _entry(L, a):
    return L.agg_section[a], L.agg_value_type[a], L.agg_sum_parts[a], L.agg_sum_exp[a]


def test_mode_layout_bookkeeping():
    lib = _lib.load()
    L, F, S, M = _layout(), TableLayout(), TableLayout(), TableLayout()
    assert lib.pgpu_fold_layout_of(C.byref(L), 7, C.byref(F)) == 0
    assert lib.pgpu_select_layout_of(C.byref(L), 7, 3, C.byref(S)) == 0
    # without percentiles: the folded layout, then M, T, LO, HI
    assert lib.pgpu_mode_layout_of(C.byref(L), 7, 0, _lib.PGPU_MODE_MAX, C.byref(M)) == 0
    assert (M.num_keys, M.num_sections, M.key_kind, M.key_words) == (7, 10, PGPU_KEYS_DENSE, 1)
    assert list(M.section_op)[:6] == list(F.section_op)[:6] and list(M.section_op)[6:10] == [PGPU_RED_SUM_I64] * 4
    assert all(_entry(M, a) == _entry(F, a) for a in range(4))
    assert _entry(M, 4) == (8, PGPU_LONG, 1, 0) and _entry(M, 5) == (9, PGPU_LONG, 1, 0)  # LO, HI; M and T: sections only
    assert M.agg_section[6] == 0 and M.agg_value_type[6] == 0
    assert _lib.table_bytes(M) == 8 * 10 * 7
    # with percentiles and the AVG reducer: the selected layout, then M, T, LO, HI and the float64 S
    assert lib.pgpu_mode_layout_of(C.byref(L), 7, 3, _lib.PGPU_MODE_MIN | _lib.PGPU_MODE_AVG, C.byref(M)) == 0
    assert M.num_sections == 14 and list(M.section_op)[:9] == list(S.section_op)[:9]
    assert list(M.section_op)[9:14] == [PGPU_RED_SUM_I64] * 4 + [PGPU_RED_SUM_F64]
    assert all(_entry(M, a) == _entry(S, a) for a in range(7))
    assert _entry(M, 7) == (11, PGPU_LONG, 1, 0) and _entry(M, 8) == (12, PGPU_LONG, 1, 0)
    assert M.agg_section[9] == 0 and M.agg_value_type[9] == 0
    H = _layout(num_keys=1024, kind=PGPU_KEYS_HASH)
    assert lib.pgpu_mode_layout_of(C.byref(H), 7, 0, 7, C.byref(M)) == 0
    assert (M.num_keys, M.key_kind, M.num_sections) == (7, PGPU_KEYS_DENSE, 11)


def test_mode_layout_errors():
    lib = _lib.load()
    M = TableLayout()
    L = _layout()
    for r in (0, 8, 9, -1, 1 << 20):
        assert lib.pgpu_mode_layout_of(C.byref(L), 7, 0, r, C.byref(M)) == _lib.PGPU_E_INVALID
        assert "reducers" in _lib.last_error()
    for k in (-1, 9):
        assert lib.pgpu_mode_layout_of(C.byref(L), 7, k, 1, C.byref(M)) == _lib.PGPU_E_INVALID
        assert "percentiles" in _lib.last_error()
    assert lib.pgpu_mode_layout_of(C.byref(L), 0, 0, 1, C.byref(M)) == _lib.PGPU_E_INVALID
    assert lib.pgpu_mode_layout_of(C.byref(L), 9, 0, 1, C.byref(M)) == _lib.PGPU_E_INVALID  # 700 % 9 != 0
    H = _layout(num_keys=1024, kind=PGPU_KEYS_HASH)
    H.key_words = 2
    assert lib.pgpu_mode_layout_of(C.byref(H), 7, 0, 1, C.byref(M)) == _lib.PGPU_E_UNSUPPORTED
    assert "two key words" in _lib.last_error()
    big = _layout(num_keys=((1 << 26) + 1) * 2)
    assert lib.pgpu_mode_layout_of(C.byref(big), (1 << 26) + 1, 0, 1, C.byref(M)) == _lib.PGPU_E_UNSUPPORTED
    # sections: 17 at most.  11 in use + the distinct count leaves 5: M, T, LO, HI and S, or a percentile instead of S
    tight = _layout()
    tight.num_sections = 11
    assert lib.pgpu_mode_layout_of(C.byref(tight), 7, 0, 7, C.byref(M)) == 0 and M.num_sections == 17
    assert lib.pgpu_mode_layout_of(C.byref(tight), 7, 1, 3, C.byref(M)) == 0 and M.num_sections == 17
    assert lib.pgpu_mode_layout_of(C.byref(tight), 7, 1, 7, C.byref(M)) == _lib.PGPU_E_UNSUPPORTED
    assert "section" in _lib.last_error()
    # aggregation entries: 16 at most.  13 COUNT(*) + the distinct count leaves 2: LO and HI
    taken = _layout()
    for a in range(13):
        taken.agg_section[a], taken.agg_value_type[a] = 0, -1
    assert lib.pgpu_mode_layout_of(C.byref(taken), 7, 0, 7, C.byref(M)) == 0 and M.agg_section[15] == 9
    assert lib.pgpu_mode_layout_of(C.byref(taken), 7, 1, 1, C.byref(M)) == _lib.PGPU_E_UNSUPPORTED
    assert "aggregation entry" in _lib.last_error()
    with pytest.raises(UnsupportedPlanError):
        _lib.check(lib.pgpu_mode_layout_of(C.byref(taken), 7, 1, 1, C.byref(M)))
