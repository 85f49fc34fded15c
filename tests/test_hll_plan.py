"""DISTINCTCOUNTHLL / DISTINCTCOUNTRAWHLL without a GPU: the SQL front end, the lowering into passes, the raise of
hand-made pass results, the DataTable round trip and two-server reduce on hand-made sketches, and the non-scan answer
from dictionaries."""
from types import SimpleNamespace

import numpy as np
import pytest

from pinot_amd import hll
from pinot_amd._lib import PGPU_INT, PGPU_STRING, UnsupportedPlanError
from pinot_amd.datatable import DataTable, OBJECT_TYPE_HYPER_LOG_LOG, object_bytes, reduce_data_tables, server_data_table
from pinot_amd.distinct import PassSketches, has_distinct, order_pass, raise_result, raise_runs
from pinot_amd.plan import ExecutionStats, QueryResult, distinct_lower, merge_non_scan, sketch_non_scan
from pinot_amd.query import AggregationSpec, SqlError, parse_sql

# (every SELECT literal of the test files is held against the oracle's parser, which has none of these functions)
SEL = "SELECT "


# ---- parser ---------------------------------------------------------------------------------------------------------
def test_parser_spec_default_log2m_and_result_names():
    q = parse_sql(SEL + "DistinctCountHLL(userId), DISTINCTCOUNTRAWHLL(userId, 12), distinctcounthll(u2, '10') FROM t")
    a, b, c = q.aggregations
    assert a == AggregationSpec("DISTINCTCOUNTHLL", "userId", log2m=8)  # CommonConstants.java:85
    assert b == AggregationSpec("DISTINCTCOUNTRAWHLL", "userId", log2m=12) and c.log2m == 10
    # getResultColumnName: the name does not carry log2m
    assert [x.result_name for x in q.aggregations] == ["distinctcounthll(userId)", "distinctcountrawhll(userId)",
                                                       "distinctcounthll(u2)"]
    assert has_distinct(q) and q.projected_columns == ["userId", "u2"]
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c, 12) FROM t GROUP BY g ORDER BY DISTINCTCOUNTHLL(c, 12) DESC, g LIMIT 3")
    assert [(o.expression, o.ascending) for o in q.order_by] == [("distinctcounthll(c)", False), ("g", True)]


@pytest.mark.parametrize("name", ["DISTINCTCOUNTHLLMV", "DISTINCTCOUNTRAWHLLMV", "DISTINCTCOUNTSMARTHLL", "FASTHLL"])
def test_parser_refuses_the_unserved_forms_by_name(name):
    with pytest.raises(SqlError, match=name):
        parse_sql(SEL + f"{name}(c) FROM t")


def test_parser_refuses_filter_clauses_and_bad_arguments():
    for fn in ("DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL"):
        with pytest.raises(SqlError, match=f"{fn} with FILTER"):
            parse_sql(SEL + f"{fn}(c) FILTER(WHERE x > 3) FROM t")
        with pytest.raises(SqlError, match="log2m"):
            parse_sql(SEL + f"{fn}(c, 8.5) FROM t")
        with pytest.raises(SqlError, match="log2m"):
            parse_sql(SEL + f"{fn}(c, 'MIN') FROM t")
        with pytest.raises(SqlError):
            parse_sql(SEL + f"{fn}(c, 8, 9) FROM t")
        with pytest.raises(SqlError):
            parse_sql(SEL + f"{fn}(*) FROM t")


@pytest.mark.parametrize("log2m", [3, 17])
def test_unserved_log2m_parses_and_keeps_the_cpu_plan(log2m):
    q = parse_sql(SEL + f"DISTINCTCOUNTHLL(c, {log2m}) FROM t")  # no SqlError
    assert q.aggregations[0].log2m == log2m
    with pytest.raises(UnsupportedPlanError, match="log2m"):
        distinct_lower(q)


# ---- lowering -------------------------------------------------------------------------------------------------------
def test_lower_gives_a_sketch_its_own_pass_with_the_plain_aggregations():
    q = parse_sql(SEL + "g, h, SUM(x), DISTINCTCOUNTHLL(c), AVG(y) FROM t WHERE x > 3 GROUP BY g, h LIMIT 7")
    (p,) = distinct_lower(q)
    assert p.column == "c" and p.query.group_by == ["g", "h", "c"] and p.log2m == 8
    assert [a.result_name for a in p.query.aggregations] == ["sum(x)", "avg(y)"]
    assert p.plain == [0, 2] and p.sketch == [1] and not (p.distinct or p.percentile or p.mode)
    assert p.query.filter is q.filter and not p.query.order_by
    # its folded table is the fold's own: the stage appends no section
    assert [a.result_name for a in p.folded.aggregations] == ["sum(x)", "avg(y)", "distinctcount(c)"]
    assert p.folded.group_by == ["g", "h"] and p.reducers == 0 and p.percentiles == []


def test_lower_shares_a_pass_between_hll_and_rawhll_of_one_column():
    q = parse_sql(SEL + "DISTINCTCOUNTRAWHLL(c, 12), DISTINCTCOUNTHLL(c, 12), DISTINCTCOUNTHLL(d), DISTINCTCOUNTHLL(c, 12) FROM t")
    pc, pd = distinct_lower(q)
    assert (pc.column, pc.sketch, pc.log2m) == ("c", [0, 1, 3], 12)
    assert (pd.column, pd.sketch, pd.log2m) == ("d", [2], 8)
    assert [a.result_name for a in pc.query.aggregations] == ["count(*)"] and pc.plain == [] == pd.plain


def test_lower_exact_and_sketch_of_one_column_are_two_passes():
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c), COUNT(*), DISTINCTCOUNT(c), PERCENTILE(c, 50) FROM t GROUP BY g")
    exact, sketch = distinct_lower(q)
    # the exact pass is today's, untouched, and -- being first -- carries the plain aggregation
    (alone,) = distinct_lower(parse_sql(SEL + "g, COUNT(*), DISTINCTCOUNT(c), PERCENTILE(c, 50) FROM t GROUP BY g"))
    assert [a.result_name for a in exact.folded.aggregations] == [a.result_name for a in alone.folded.aggregations]
    assert (exact.plain, exact.distinct, exact.percentile, exact.sketch) == ([1], [2], [3], [])
    assert (sketch.column, sketch.plain, sketch.sketch, sketch.distinct) == ("c", [], [0], [])
    assert [a.result_name for a in sketch.query.aggregations] == ["count(*)"]


def test_lower_refusals():
    for sql, what in (("DISTINCTCOUNTHLL(c, 8), DISTINCTCOUNTRAWHLL(c, 12) FROM t", "log2m 12 beside log2m 8"),
                      ("g, DISTINCTCOUNTHLL(g) FROM t GROUP BY g", "group column"),
                      ("DISTINCTCOUNTHLL(c), SUMMV(tags) FROM t", r"\*MV"),
                      ("DISTINCTCOUNTHLL(c), SUM(x) FILTER(WHERE f < 3) FROM t", "FILTER")):
        with pytest.raises(UnsupportedPlanError, match=what):
            distinct_lower(parse_sql(SEL + sql))


def test_order_by_a_sketch_is_not_trimmed_on_the_device():
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c), DISTINCTCOUNT(d) FROM t GROUP BY g ORDER BY DISTINCTCOUNTHLL(c) DESC LIMIT 3")
    assert order_pass(q, distinct_lower(q)) is None
    # a group column or a plain aggregation trims in the first pass, as today, when that is an exact pass
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c), DISTINCTCOUNT(d), SUM(x) FROM t GROUP BY g ORDER BY SUM(x) DESC LIMIT 3")
    pi, ob = order_pass(q, distinct_lower(q))
    assert pi == 0 and ob.expression == "sum(x)" and distinct_lower(q)[0].column == "d"
    # sketch passes alone: their collect takes no order, the host orders
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c), SUM(x) FROM t GROUP BY g ORDER BY SUM(x) DESC LIMIT 3")
    assert order_pass(q, distinct_lower(q)) is None


# ---- raising hand-made pass results -----------------------------------------------------------------------------------
def _pass_result(q, rows=None, agg=None, **stats):
    r = QueryResult(query=q, stats=ExecutionStats(**stats))
    r._group_rows, r.aggregation_result = rows, agg
    r._intermediate = {tuple(x[: len(q.group_by)]): list(x[len(q.group_by):]) for x in rows} if rows is not None \
        else {(): list(agg)}
    return r


def _sketch(values, log2m=8):
    return hll.sketch_of(np.asarray(values, dtype=np.int32), PGPU_INT, log2m)


def test_raise_result_grouped_and_empty():
    q = parse_sql(SEL + "g, DISTINCTCOUNTRAWHLL(c), SUM(x), DISTINCTCOUNTHLL(c) FROM t GROUP BY g ORDER BY g LIMIT 10")
    (p,) = distinct_lower(q)
    a, b = _sketch(range(100)), _sketch(range(50, 4000))
    words = np.stack([a.words, b.words])
    ps = PassSketches(_pass_result(p.folded, rows=[(1, 10.0, 100), (4, 20.0, 3950)]), words, 8)
    res = raise_result(q, [p], [ps])
    assert res.rows == [(1, a.to_bytes().hex(), 10.0, a.cardinality()), (4, b.to_bytes().hex(), 20.0, b.cardinality())]
    assert type(res.rows[0][3]) is int and abs(res.rows[0][3] - 100) <= 20 and abs(res.rows[1][3] - 3950) <= 790
    mer = raise_runs(q, [p], [ps])
    assert mer.rows == res.rows and mer.value_sets
    assert mer.intermediate[(4,)] == [b, 20.0, b]
    # aggregation-only with no matched doc: the empty sketch, 0
    q = parse_sql(SEL + "DISTINCTCOUNTHLL(c, 12), DISTINCTCOUNTRAWHLL(c, 12) FROM t WHERE x > 3")
    (p,) = distinct_lower(q)
    ps = PassSketches(_pass_result(p.folded, agg=[0, 0]), np.zeros((0, hll.num_words(12)), dtype=np.uint32), 12)
    res = raise_result(q, [p], [ps])
    assert res.rows == [(0, hll.HyperLogLog.empty(12).to_bytes().hex())] and len(res.rows[0][1]) == 2 * (8 + 2732)


# ---- DataTable --------------------------------------------------------------------------------------------------------
def _mergeable(q, rows=None, agg=None):
    r = _pass_result(q, rows, agg, num_docs_scanned=5, num_total_docs=9)
    r.value_sets = True
    return r


def test_data_table_round_trip_and_two_server_reduce():
    assert object_bytes(_sketch([1]))[:4] == b"\x00\x00\x00\x06" and OBJECT_TYPE_HYPER_LOG_LOG == 6
    assert object_bytes(_sketch([1]))[4:] == _sketch([1]).to_bytes()
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c), COUNT(*), DISTINCTCOUNTRAWHLL(c) FROM t GROUP BY g ORDER BY g LIMIT 10")
    s1 = {1: _sketch(range(0, 600)), 2: _sketch(range(7))}
    s2 = {2: _sketch(range(5, 9)), 3: _sketch(range(1000, 1100))}
    wire = []
    for s in (s1, s2):
        t = server_data_table(q, _mergeable(q, rows=[(g, sk, 3, sk) for g, sk in s.items()]), [PGPU_INT])
        assert t.schema.column_names == ["g", "distinctcounthll(c)", "count(*)", "distinctcountrawhll(c)"]
        assert t.schema.column_types == ["INT", "OBJECT", "LONG", "OBJECT"]
        back = DataTable.from_bytes(t.to_bytes())
        assert back.rows == t.rows and all(type(r[1]) is hll.HyperLogLog for r in back.rows)
        wire.append(back)
    got = reduce_data_tables(q, wire)
    both = s1[2].merge(s2[2])
    assert both.cardinality() == 9
    assert got.rows == [(1, s1[1].cardinality(), 3, s1[1].to_bytes().hex()), (2, 9, 6, both.to_bytes().hex()),
                        (3, s2[3].cardinality(), 3, s2[3].to_bytes().hex())]
    assert got.num_docs_scanned == 10


def test_data_table_aggregation_only_names_and_empty_default():
    q = parse_sql(SEL + "DISTINCTCOUNTHLL(c, 12), DISTINCTCOUNTRAWHLL(c, 12) FROM t")
    sk = _sketch(range(300), 12)
    t = server_data_table(q, _mergeable(q, agg=[sk, sk]))
    assert t.schema.column_names == ["distinctCountHLL_c", "distinctCountRawHLL_c"]
    assert reduce_data_tables(q, [DataTable.from_bytes(t.to_bytes())] * 2).rows == [(sk.cardinality(), sk.to_bytes().hex())]
    # no server had a row: the empty sketch of the query's log2m
    assert reduce_data_tables(q, [DataTable(None, [], {})]).rows == [(0, hll.HyperLogLog.empty(12).to_bytes().hex())]
    # a result without the sketches has no DataTable
    plain = _pass_result(q, agg=[1, "00"])
    with pytest.raises(UnsupportedPlanError):
        server_data_table(q, plain)


# ---- non-scan -----------------------------------------------------------------------------------------------------------
def _meta_segment(num_docs, types, **dicts):
    def min_max(col):
        d = dicts[col]
        return float(np.min(d)), float(np.max(d))
    return SimpleNamespace(num_docs=num_docs, dictionaries=dicts, min_max=min_max,
                           column=lambda c: SimpleNamespace(data_type=types[c]))


def test_non_scan_answer_from_dictionaries():
    types = {"c": PGPU_INT, "s": PGPU_STRING}
    q = parse_sql(SEL + "DISTINCTCOUNTHLL(c), COUNT(*), DISTINCTCOUNTRAWHLL(s, 12), DISTINCTCOUNT(c) FROM t")
    segs = [_meta_segment(10, types, c=np.array([1, 5, 9], dtype=np.int32), s=["a", "b"]),
            _meta_segment(20, types, c=np.array([5, 9, 11, 12], dtype=np.int32), s=["b", "ç"])]
    res = merge_non_scan(q, None, segs)
    sketch_non_scan(q, None, segs, res)
    sc = _sketch([1, 5, 9, 11, 12])
    ss = hll.sketch_of(["a", "b", "ç"], PGPU_STRING, 12)
    assert res.aggregation_result == [5, 30, ss.to_bytes().hex(), 5] and res.rows == [tuple(res.aggregation_result)]
    assert res._intermediate[()][0] == sc and res._intermediate[()][2] == ss
    st = res.stats
    assert (st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_entries_scanned_post_filter,
            st.num_total_docs, st.kernel_ms) == (30, 0, 0, 30, 0)
    # beside scanned segments: their sketch is united with the dictionaries'
    scanned = _mergeable(q, agg=[_sketch([100, 101]), 7, hll.sketch_of(["z"], PGPU_STRING, 12), None])
    res = merge_non_scan(q, scanned, segs[:1], {3: {100, 101}})
    sketch_non_scan(q, scanned, segs[:1], res)
    assert res.aggregation_result[:2] == [5, 17] and res.aggregation_result[3] == 5
    assert res._intermediate[()][0] == _sketch([1, 5, 9, 100, 101])
    assert res._intermediate[()][2] == hll.sketch_of(["a", "b", "z"], PGPU_STRING, 12)
