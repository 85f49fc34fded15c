"""Exact PERCENTILE without a GPU: the SQL front end and the result names, the lowering into the folded passes it shares
with DISTINCTCOUNT and their join, the rank arithmetic against a sort, the selected layout's bookkeeping
(pgpu_select_layout_of is host only), and the known answers' fixture against the rank formula in numpy."""
import ctypes as C
import dataclasses
import json
import math
import os
import re

import numpy as np
import pytest

from pinot_amd import _lib
from pinot_amd._lib import (PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_LONG, PGPU_RED_MIN_I64, PGPU_RED_SUM_I64,
                            TableLayout, UnsupportedPlanError)
from pinot_amd.distinct import order_pass
from pinot_amd.plan import ExecutionStats, QueryResult, distinct_lower, distinct_raise, has_distinct, topk_spec
from pinot_amd.query import AggregationSpec, SqlError, java_double_string, parse_sql
from tests.helpers import GOLDEN, load_kat, sv_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Every SELECT literal of the test files is also held against the oracle's own SQL parser (tests/test_oracle_sql.py),
# which has no PERCENTILE and is to stay without one: the queries here get their keyword from SEL instead.
SEL = "SELECT "

with open(os.path.join(GOLDEN, "kat_percentile.json")) as _f:
    KAT = json.load(_f)


# ---- parser ---------------------------------------------------------------------------------------------------------
def test_parser_forms_and_result_names():
    q = parse_sql(SEL + "Percentile90(m), PERCENTILE5(m), PERCENTILE(m, 50), percentile(m, '99.9'), PERCENTILE(m, 0), "
                  "PERCENTILE(m, 100.0), COUNT(*) FROM t WHERE x > 3")
    a = q.aggregations
    assert [s.function for s in a[:6]] == ["PERCENTILE"] * 6 and all(s.column == "m" for s in a[:6])
    assert [s.percentile for s in a[:6]] == [90.0, 5.0, 50.0, 99.9, 0.0, 100.0]
    # PercentileAggregationFunction.java:65-70: the one-argument form keeps its number, the other Double.toString(p)
    assert [s.result_name for s in a] == ["percentile90(m)", "percentile5(m)", "percentile(m, 50.0)",
                                          "percentile(m, 99.9)", "percentile(m, 0.0)", "percentile(m, 100.0)", "count(*)"]
    assert q.projected_columns == ["m"] and q.columns == ["x", "m"]
    # existing specs are unchanged by the new optional fields
    assert a[6] == AggregationSpec("COUNT", None) and a[6].percentile is None
    assert AggregationSpec("SUM", "m") == AggregationSpec("SUM", "m", None, None)


def test_java_double_string():
    assert [java_double_string(x) for x in (50, 99.9, 0, 100, 33.3, 0.001, 0.0005, 1e-5, 2.5e-7)] == \
        ["50.0", "99.9", "0.0", "100.0", "33.3", "0.001", "5.0E-4", "1.0E-5", "2.5E-7"]


@pytest.mark.parametrize("item,match", [
    ("PERCENTILEEST90(m)", "PERCENTILEEST"), ("PERCENTILEEST(m, 90)", "PERCENTILEEST"),
    ("PERCENTILETDIGEST90(m)", "PERCENTILETDIGEST"), ("PERCENTILETDIGEST(m, 90)", "PERCENTILETDIGEST"),
    ("PERCENTILERAWEST90(m)", "PERCENTILERAW"), ("PERCENTILERAWTDIGEST(m, 90)", "PERCENTILERAW"),
    ("PERCENTILE90MV(tags)", "PERCENTILE90MV"), ("PERCENTILEMV(tags, 90)", "PERCENTILEMV"),
    ("PERCENTILEESTMV(tags, 90)", "PERCENTILEEST"),
    ("PERCENTILE90(m) FILTER(WHERE x > 3)", "FILTER"), ("PERCENTILE(m, 90) FILTER(WHERE x > 3)", "FILTER"),
    ("PERCENTILE(m, 101)", "outside"), ("PERCENTILE(m, -1)", "outside"), ("PERCENTILE(m, 'abc')", "not a number"),
    ("PERCENTILE(m, 'nan')", "outside"), ("PERCENTILE123(m)", "digits"), ("PERCENTILE(m)", "expected"),
    ("PERCENTILE90(*)", "identifier")])
def test_parser_refuses(item, match):
    with pytest.raises(SqlError, match=match):
        parse_sql(SEL + item + " FROM t")


def test_parser_order_by_percentile():
    q = parse_sql(SEL + "g, percentile90(m) FROM t GROUP BY g ORDER BY PERCENTILE90(m) DESC, g LIMIT 3")
    assert [(o.expression, o.ascending) for o in q.order_by] == [("percentile90(m)", False), ("g", True)]
    q = parse_sql(SEL + "g, PERCENTILE(m, 50) FROM t GROUP BY g ORDER BY percentile(m, '50.0') LIMIT 3")
    assert q.order_by[0].expression == "percentile(m, 50.0)" == q.aggregations[0].result_name


# ---- lowering -------------------------------------------------------------------------------------------------------
def test_lower_three_percentiles_of_one_column_are_one_pass():
    q = parse_sql(SEL + "g, PERCENTILE50(c), PERCENTILE90(c), PERCENTILE99(c) FROM t WHERE x > 3 GROUP BY g LIMIT 7")
    assert has_distinct(q)
    (p,) = distinct_lower(q)
    assert p.column == "c" and p.query.group_by == ["g", "c"] and p.folded.group_by == ["g"]
    assert [a.result_name for a in p.query.aggregations] == ["count(*)"]  # inserted: nothing else to carry
    assert p.plain == [] and p.distinct == [] and p.percentile == [0, 1, 2] and p.percentiles == [50.0, 90.0, 99.0]
    assert [a.result_name for a in p.folded.aggregations] == ["count(*)", "distinctcount(c)", "percentile50(c)",
                                                              "percentile90(c)", "percentile99(c)"]
    assert p.query.filter is q.filter and not p.query.order_by


def test_lower_distinctcount_beside_percentiles_of_the_column_is_one_pass():
    q = parse_sql(SEL + "PERCENTILE(c, 33.3), DISTINCTCOUNT(c), SUM(x), PERCENTILE99(c) FROM t")
    (p,) = distinct_lower(q)
    assert (p.plain, p.distinct, p.percentile, p.percentiles) == ([2], [1], [0, 3], [33.3, 99.0])
    assert [a.result_name for a in p.query.aggregations] == ["sum(x)"]


def test_lower_two_columns_two_passes_and_the_plain_aggregations_ride_in_the_first():
    q = parse_sql(SEL + "g, SUM(x), PERCENTILE50(a), AVG(y), PERCENTILE90(b), DISTINCTCOUNT(b), PERCENTILE99(a) "
                  "FROM t GROUP BY g")
    p0, p1 = distinct_lower(q)
    assert (p0.column, p0.plain, p0.distinct, p0.percentile) == ("a", [0, 2], [], [1, 5])
    assert (p1.column, p1.plain, p1.distinct, p1.percentile) == ("b", [], [4], [3])
    assert [a.result_name for a in p0.query.aggregations] == ["sum(x)", "avg(y)"]
    assert [a.result_name for a in p1.query.aggregations] == ["count(*)"]
    assert p0.query.group_by == ["g", "a"] and p1.query.group_by == ["g", "b"]


def test_lower_refuses_what_is_not_served():
    with pytest.raises(UnsupportedPlanError, match="PERCENTILE of the group column"):
        distinct_lower(parse_sql(SEL + "g, PERCENTILE50(g) FROM t GROUP BY g"))
    with pytest.raises(UnsupportedPlanError, match="FILTER"):
        distinct_lower(parse_sql(SEL + "PERCENTILE50(a), SUM(x) FILTER(WHERE y > 1) FROM t"))
    with pytest.raises(UnsupportedPlanError, match="MV"):
        distinct_lower(parse_sql(SEL + "PERCENTILE50(a), SUMMV(tags) FROM t"))
    nine = ", ".join(f"PERCENTILE{10 * k + 5}(a)" for k in range(9))
    with pytest.raises(UnsupportedPlanError, match="at most 8"):
        distinct_lower(parse_sql(SEL + nine + " FROM t"))


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


@pytest.mark.parametrize("sql", ["PERCENTILE50(tags) FROM t", "g, SUM(x), PERCENTILE(tags, 99.9) FROM t GROUP BY g",
                                 "DISTINCTCOUNT(tags), PERCENTILE90(tags) FROM t"])
def test_multi_value_column_raises_before_anything_is_prepared_or_launched(sql):
    segs = [_stub_segment(i, tags=(PGPU_INT, True), x=(PGPU_INT, False), g=(PGPU_INT, False)) for i in range(2)]
    q = parse_sql(SEL + sql)
    pm = _maker_that_must_not_launch()
    with pytest.raises(UnsupportedPlanError, match="multi-value column 'tags'"):
        pm.check_distinct(q, distinct_lower(q), segs)
    for entry in (pm.submit, pm.execute):
        with pytest.raises(UnsupportedPlanError, match="multi-value column 'tags'"):
            entry(q, segs)
    # the same maker does reach the prepare step for a single-value column: the stub proves something
    ok = [_stub_segment(i, tags=(PGPU_INT, False), x=(PGPU_INT, False), g=(PGPU_INT, False)) for i in range(2)]
    pm.check_distinct(q, distinct_lower(q), ok)
    with pytest.raises(AssertionError, match="prepared or launched"):
        pm.submit(q, ok)


def test_string_column_and_key_space_raise_before_anything_is_prepared_or_launched():
    from pinot_amd._lib import PGPU_STRING
    pm = _maker_that_must_not_launch()
    segs = [_stub_segment(0, s=(PGPU_INT, False), g=(PGPU_INT, False)),
            _stub_segment(1, s=(PGPU_STRING, False), g=(PGPU_INT, False))]  # STRING in any segment
    q = parse_sql(SEL + "g, PERCENTILE50(s) FROM t GROUP BY g")
    for entry in (pm.submit, pm.execute):
        with pytest.raises(UnsupportedPlanError, match="STRING column 's'"):
            entry(q, segs)
    # DISTINCTCOUNT of the same column is served: only the percentile needs an order on the values it can return
    pm.check_distinct(parse_sql(SEL + "g, DISTINCTCOUNT(s) FROM t GROUP BY g"),
                      distinct_lower(parse_sql(SEL + "g, DISTINCTCOUNT(s) FROM t GROUP BY g")), segs)
    pm.num_groups_limit = 7  # the key space of g (7) is not below it
    with pytest.raises(UnsupportedPlanError, match="numGroupsLimit"):
        pm.submit(parse_sql(SEL + "g, PERCENTILE50(x) FROM t GROUP BY g"),
                  [_stub_segment(0, x=(PGPU_INT, False), g=(PGPU_INT, False))])


def test_refused_by_the_multi_gpu_executors_and_the_mergeable_forms():
    from pinot_amd import combine, datatable, node
    q = parse_sql(SEL + "PERCENTILE50(a) FROM t")
    for refuse in (combine._refuse_distinct, node._refuse_distinct, datatable._refuse_distinct):
        with pytest.raises(UnsupportedPlanError, match="PERCENTILE"):
            refuse(q)
        refuse(parse_sql(SEL + "SUM(a) FROM t"))
    with pytest.raises(UnsupportedPlanError, match="PERCENTILE"):
        QueryResult(q).intermediate


def test_a_percentile_query_is_never_a_non_scan_plan():
    from types import SimpleNamespace

    from pinot_amd.plan import GpuPlanMaker
    seg = SimpleNamespace(num_docs=10)  # (never looked at: the function list decides first)
    for sql in ("PERCENTILE50(a) FROM t", "COUNT(*), MAX(a), PERCENTILE(a, 100) FROM t"):
        assert GpuPlanMaker.non_scan_segments(None, parse_sql(SEL + sql), [seg, seg]) == [False, False]


def test_order_pass_and_the_selected_topk_spec():
    q = parse_sql(SEL + "g, SUM(x), PERCENTILE50(a), DISTINCTCOUNT(b), PERCENTILE90(b), PERCENTILE99(b) FROM t "
                  "GROUP BY g ORDER BY PERCENTILE99(b) DESC, g LIMIT 3")
    passes = distinct_lower(q)
    pi, ob = order_pass(q, passes)
    assert pi == 1 and ob.expression == "percentile99(b)"
    t = topk_spec(dataclasses.replace(passes[pi].folded, order_by=[ob]), [7], 15)
    # pass 1 carries COUNT(*) (entry 0) and the distinct count (entry 1): PERCENTILE99 is the second pick, entry 3
    assert (t.source, t.agg_fn, t.agg_index, t.descending, t.k) == (_lib.PGPU_TOPK_AGG, _lib.PGPU_AGG_SUM, 3, 1, 15)
    q2 = parse_sql(SEL + "g, SUM(x), PERCENTILE50(a) FROM t GROUP BY g ORDER BY SUM(x) LIMIT 3")
    assert order_pass(q2, distinct_lower(q2))[0] == 0


# ---- raise / join -------------------------------------------------------------------------------------------------------
def _result(query, rows=None, agg=None, values=None, **stats):
    r = QueryResult(query, ExecutionStats(**stats))
    r.aggregation_result = agg
    r._group_rows = rows
    r.value_dictionary = values
    return r


def test_raise_aggregation_only_values_types_and_the_empty_result():
    q = parse_sql(SEL + "PERCENTILE50(a), SUM(x), DISTINCTCOUNT(a), PERCENTILE(b, 99.9) FROM t WHERE x > 3")
    passes = distinct_lower(q)
    da = np.array([-5, 7, 1 << 40], dtype=np.int64)
    db = np.array([0.25, 0.5], dtype=np.float32)
    r0 = _result(passes[0].folded, agg=[12.0, 3, 2], values=da, num_docs_scanned=10)       # sum | distinct | cid
    r1 = _result(passes[1].folded, agg=[10, 2, 1], values=db, num_docs_scanned=10)         # count | distinct | cid
    res = distinct_raise(q, passes, [r0, r1])
    assert res.aggregation_result == [float(1 << 40), 12.0, 3, 0.5]
    assert [type(v) for v in res.aggregation_result] == [float, float, int, float]
    assert res.stats.num_entries_scanned_post_filter == 10 * 3  # a, x, b
    # nothing matched: the distinct count is 0 and the pick's cell too -> DEFAULT_FINAL_RESULT
    r0 = _result(passes[0].folded, agg=[0.0, 0, 0], values=da)
    r1 = _result(passes[1].folded, agg=[0, 0, 0], values=db)
    assert distinct_raise(q, passes, [r0, r1]).aggregation_result == [-math.inf, 0.0, 0, -math.inf]


def test_raise_grouped_joins_on_the_key_and_orders_by_value_then_key():
    q = parse_sql(SEL + "g, PERCENTILE90(a), COUNT(*) FROM t GROUP BY g ORDER BY PERCENTILE90(a), g LIMIT 3")
    (p,) = distinct_lower(q)
    d = np.array([10, 20, 30], dtype=np.int32)
    rows = [("u", 4, 2, 2), ("v", 5, 1, 1), ("w", 6, 3, 1), ("x", 7, 3, 0), ("y", 8, 1, 1)]  # g | count | distinct | cid
    res = distinct_raise(q, [p], [_result(p.folded, rows=rows, values=d, num_docs_scanned=30)])
    assert res.rows == [("x", 10.0, 7), ("v", 20.0, 5), ("w", 20.0, 6)]  # three ties at 20.0: the key decides
    assert all(type(r[1]) is float for r in res.group_rows)


# ---- rank arithmetic ----------------------------------------------------------------------------------------------------
def _rank(n, p):
    """PercentileAggregationFunction.java:152-165 in IEEE double, the device's operation order."""
    return n - 1 if p == 100 else int(float(n) * p / 100.0)


@pytest.mark.parametrize("p", [0, 33.3, 50, 99.9, 100])
def test_rank_formula_against_a_sort(p):
    rng = np.random.default_rng(int(p * 10))
    for n in (1, 2, 3, 1000):
        values = rng.integers(0, 50, n)
        values.sort()
        want = values[n - 1] if p == 100 else values[int(n * p / 100)]  # the reference's index into its sorted list
        ids, counts = np.unique(values, return_counts=True)              # the table: count per (sorted) id
        cid = int(np.searchsorted(np.cumsum(counts), _rank(n, p), side="right"))
        assert ids[cid] == want, (n, p)
    from fractions import Fraction
    for n in (1, 2, 3, 1000, (1 << 31) - 1):
        r = _rank(n, p)
        assert 0 <= r < n
        # against exact rational arithmetic with p as the double it is: the two roundings of the double computation
        # can carry the quotient across an integer, by one at the most
        exact = n - 1 if p == 100 else int(Fraction(n) * Fraction(float(p)) / 100)
        assert abs(r - exact) <= 1, (n, p, r, exact)
    big = (1 << 31) - 1  # (no int32 overflow: the product is formed in double)
    assert [_rank(big, q) for q in (0, 50, 100)] == [0, 1073741823, big - 1]


# ---- library ----------------------------------------------------------------------------------------------------------------
def test_abi_version_and_new_entry_points():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert int(re.search(r"#define PGPU_ABI_VERSION (\d+)", header).group(1)) == 13 == _lib.ABI_VERSION
    assert lib.pgpu_abi_version() == 13
    assert "#define PGPU_SELECT_MAX 8" in header and _lib.PGPU_SELECT_MAX == 8
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for name, nargs in (("pgpu_select_layout_of", 4), ("pgpu_table_select", 9), ("pgpu_query_collect_select", 11)):
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


def test_select_layout_bookkeeping():
    lib = _lib.load()
    L, F, S = _layout(), TableLayout(), TableLayout()
    assert lib.pgpu_fold_layout_of(C.byref(L), 7, C.byref(F)) == 0
    assert lib.pgpu_select_layout_of(C.byref(L), 7, 3, C.byref(S)) == 0
    assert (S.num_keys, S.num_sections, S.key_kind, S.key_words) == (7, 9, PGPU_KEYS_DENSE, 1)
    # the folded layout, then three int64 sections
    assert list(S.section_op)[:6] == list(F.section_op)[:6] and list(S.section_op)[6:9] == [PGPU_RED_SUM_I64] * 3
    for a in range(4):  # the input's entries and the distinct count (entry 3, section 5) as the fold describes them
        assert (S.agg_section[a], S.agg_value_type[a], S.agg_sum_parts[a], S.agg_sum_exp[a]) == \
               (F.agg_section[a], F.agg_value_type[a], F.agg_sum_parts[a], F.agg_sum_exp[a])
    for j in range(3):  # percentile j: entry n + 1 + j, a one-section LONG
        assert (S.agg_section[4 + j], S.agg_value_type[4 + j], S.agg_sum_parts[4 + j], S.agg_sum_exp[4 + j]) == \
               (6 + j, PGPU_LONG, 1, 0)
    assert S.agg_section[7] == 0 and S.agg_value_type[7] == 0
    assert _lib.table_bytes(S) == 8 * 9 * 7
    H = _layout(num_keys=1024, kind=PGPU_KEYS_HASH)
    assert lib.pgpu_select_layout_of(C.byref(H), 7, 8, C.byref(S)) == 0
    assert (S.num_keys, S.key_kind, S.num_sections) == (7, PGPU_KEYS_DENSE, 14)


def test_select_layout_errors():
    lib = _lib.load()
    S = TableLayout()
    L = _layout()
    for k in (0, -1, 9):
        assert lib.pgpu_select_layout_of(C.byref(L), 7, k, C.byref(S)) == _lib.PGPU_E_INVALID
        assert "percentiles" in _lib.last_error()
    assert lib.pgpu_select_layout_of(C.byref(L), 0, 1, C.byref(S)) == _lib.PGPU_E_INVALID
    assert lib.pgpu_select_layout_of(C.byref(L), 9, 1, C.byref(S)) == _lib.PGPU_E_INVALID  # 700 % 9 != 0
    H = _layout(num_keys=1024, kind=PGPU_KEYS_HASH)
    H.key_words = 2
    assert lib.pgpu_select_layout_of(C.byref(H), 7, 1, C.byref(S)) == _lib.PGPU_E_UNSUPPORTED
    big = _layout(num_keys=((1 << 26) + 1) * 2)
    assert lib.pgpu_select_layout_of(C.byref(big), (1 << 26) + 1, 1, C.byref(S)) == _lib.PGPU_E_UNSUPPORTED
    # sections: 17 at most.  12 in use + the distinct count leaves 4
    tight = _layout()
    tight.num_sections = 12
    assert lib.pgpu_select_layout_of(C.byref(tight), 7, 4, C.byref(S)) == 0 and S.num_sections == 17
    assert lib.pgpu_select_layout_of(C.byref(tight), 7, 5, C.byref(S)) == _lib.PGPU_E_UNSUPPORTED
    assert "section" in _lib.last_error()
    # aggregation entries: 16 at most.  13 COUNT(*) + the distinct count leaves 2
    taken = _layout()
    for a in range(13):
        taken.agg_section[a], taken.agg_value_type[a] = 0, -1
    assert lib.pgpu_select_layout_of(C.byref(taken), 7, 2, C.byref(S)) == 0 and S.agg_section[15] == 7
    assert lib.pgpu_select_layout_of(C.byref(taken), 7, 3, C.byref(S)) == _lib.PGPU_E_UNSUPPORTED
    assert "aggregation entry" in _lib.last_error()
    with pytest.raises(UnsupportedPlanError):
        _lib.check(lib.pgpu_select_layout_of(C.byref(taken), 7, 3, C.byref(S)))


# ---- the fixture ----------------------------------------------------------------------------------------------------------
def test_known_answers_follow_the_rank_formula():
    """The unfiltered known answers from the rank formula over the golden columns four times: they pin the rank
    arithmetic, not only the plumbing."""
    cols = sv_columns()
    assert "PERCENTILE" in KAT["aggregation"]["cases"][0]["sql"] and load_kat()["filter"].startswith(" WHERE")
    for case in KAT["aggregation"]["cases"]:
        if case["stats"] != "all":
            continue
        p = float(re.search(r"PERCENTILE(?:\(column1, '?)?(\d+)", case["sql"]).group(1))
        for name, want in zip(("column1", "column3"), case["result"]):
            ids, counts = np.unique(np.tile(np.asarray(cols[name][1]), 4), return_counts=True)
            cid = int(np.searchsorted(np.cumsum(counts), _rank(int(counts.sum()), p), side="right"))
            assert float(ids[cid]) == want, case["sql"]
