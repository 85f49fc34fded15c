"""The mergeable intermediates of DISTINCTCOUNT, PERCENTILE and MODE on the host (no GPU): their OBJECT cells on the wire
against hand-written bytes, the broker's merge and final of two hand-built servers, and what stays refused."""
import ctypes as C
import math
import struct

import pytest

from pinot_amd import _lib
from pinot_amd._lib import PGPU_DOUBLE, PGPU_FLOAT, PGPU_INT, PGPU_LONG, PGPU_STRING, UnsupportedPlanError
from pinot_amd.datatable import (OBJECT, DataSchema, DataTable, _agg_column, object_bytes, object_from_bytes,
                                 reduce_data_tables, server_data_table)
from pinot_amd.distinct import ValueList, ValueMap, ValueSet
from pinot_amd.plan import QueryResult
from pinot_amd.query import parse_sql

SEL = "SELECT "  # (every SELECT literal of the test files is held against the oracle's SQL parser, which has none of these)
H = bytes.fromhex

# one small value of each object type: int ObjectType value, int size, the elements (ObjectSerDeUtils.java)
WIRE = [
    (ValueSet([3, 7], PGPU_INT), H("00000009 00000002 00000003 00000007")),
    (ValueSet([-1, 1 << 40], PGPU_LONG), H("0000000f 00000002 ffffffffffffffff 0000010000000000")),
    (ValueSet([-0.0, 1.5], PGPU_FLOAT), H("00000010 00000002 80000000 3fc00000")),
    (ValueSet([0.5, 2.0], PGPU_DOUBLE), H("00000011 00000002 3fe0000000000000 4000000000000000")),
    (ValueSet(["a", "éz"], PGPU_STRING), H("00000012 00000002 00000001 61 00000003 c3a97a")),
    (ValueList([1.0, 2.5], [2, 1]), H("00000003 00000003 3ff0000000000000 3ff0000000000000 4004000000000000")),
    (ValueMap([5, 9], [2, 7], PGPU_INT), H("00000017 00000002 00000005 0000000000000002 00000009 0000000000000007")),
    (ValueMap([-2, 4], [1, 3], PGPU_LONG),
     H("00000018 00000002 fffffffffffffffe 0000000000000001 0000000000000004 0000000000000003")),
    (ValueMap([0.25], [4], PGPU_FLOAT), H("00000019 00000001 3e800000 0000000000000004")),
    (ValueMap([1.5, 2.0], [2, 9], PGPU_DOUBLE),
     H("0000001a 00000002 3ff8000000000000 0000000000000002 4000000000000000 0000000000000009")),
]


@pytest.mark.parametrize("value,wire", WIRE, ids=[f"{type(v).__name__}-{w[3]}" for v, w in WIRE])
def test_object_cells_on_the_wire(value, wire):
    assert object_bytes(value) == wire
    assert object_from_bytes(b"\0\0\0" + wire, 3) == value
    # through a whole DataTable, beside an AvgPair
    t = DataTable(DataSchema(["g", "x", "avg(y)"], ["INT", OBJECT, OBJECT]), [(4, value, (2.5, 3)), (5, value, (0.0, 0))],
                  {"numDocsScanned": "9"})
    back = DataTable.from_bytes(t.to_bytes())
    assert back.rows == t.rows and back.metadata == t.metadata


def test_a_list_in_any_order_reads_back_as_runs():
    raw = struct.pack(">ii3d", 3, 3, 2.5, 1.0, 1.0)
    assert object_from_bytes(raw, 0) == ValueList([1.0, 2.5], [2, 1])


def test_a_cell_past_a_java_array_is_refused_before_it_is_built():
    with pytest.raises(UnsupportedPlanError, match="OBJECT cell"):
        object_bytes(ValueList([1.0], [1 << 28]))  # 2^31 bytes of doubles
    with pytest.raises(UnsupportedPlanError, match="OBJECT cell"):
        DataTable(DataSchema(["percentile50_c"], [OBJECT]), [(ValueList([1.0, 2.0], [1 << 27, 1 << 27]),)]).to_bytes()


def test_column_names_and_types():
    q = parse_sql(SEL + "DISTINCTCOUNT(c), PERCENTILE95(c), PERCENTILE(c, 99.9), MODE(c, 'MAX'), AVG(c) FROM t")
    assert [_agg_column(a, False) for a in q.aggregations] == [
        ("distinctCount_c", OBJECT), ("percentile95_c", OBJECT), ("percentile99.9_c", OBJECT), ("mode_c", OBJECT),
        ("avg_c", OBJECT)]
    assert [_agg_column(a, True)[0] for a in q.aggregations] == [
        "distinctcount(c)", "percentile95(c)", "percentile(c, 99.9)", "mode(c)", "avg(c)"]


def _server(q, inter, docs):
    """A hand-built server's result: value sets collected, the given intermediates."""
    r = QueryResult(q)
    r.value_sets = True
    r._intermediate = inter
    r.stats.num_docs_scanned = r.stats.num_total_docs = docs
    return server_data_table(q, r, [PGPU_INT] * len(q.group_by))


def _wire(tables):
    return [DataTable.from_bytes(t.to_bytes()) for t in tables]


def test_two_servers_whose_sets_overlap():
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c), PERCENTILE(c, 50), MODE(c), MODE(c, 'MAX'), MODE(c, 'AVG'), COUNT(*) FROM t "
                  "GROUP BY g ORDER BY g LIMIT 10")

    def inter(values, counts):
        m = ValueMap(values, counts, PGPU_INT)
        return [ValueSet(values, PGPU_INT), ValueList([float(v) for v in values], counts), m, m, m, sum(counts)]

    a = _server(q, {(1,): inter([10, 20, 30], [5, 1, 1]), (2,): inter([7], [2])}, 9)
    b = _server(q, {(1,): inter([20, 30, 40, 50], [3, 3, 1, 6])}, 13)
    alone_a = reduce_data_tables(q, _wire([a])).rows
    alone_b = reduce_data_tables(q, _wire([b])).rows
    both = reduce_data_tables(q, _wire([a, b]))
    # g = 1: the union {10, 20, 30, 40, 50}.  a's list 10 x5, 20, 30 has its median (element 3 of 7) at 10, b's 20 x3,
    # 30 x3, 40, 50 x6 (element 6 of 13) at 40, the merged 10 x5, 20 x4, 30 x4, 40, 50 x6 (element 10 of 20) at 30;
    # the mode is 10 on a (5 times) and 50 on b and after the merge (6 against 5)
    assert alone_a[0] == (1, 3, 10.0, 10.0, 10.0, 10.0, 7) and alone_b[0] == (1, 4, 40.0, 50.0, 50.0, 50.0, 13)
    assert both.rows == [(1, 5, 30.0, 50.0, 50.0, 50.0, 20), (2, 1, 7.0, 7.0, 7.0, 7.0, 2)]
    assert [type(v) for v in both.rows[0]] == [int, int, float, float, float, float, int]
    assert both.num_docs_scanned == 22 and both.total_docs == 22
    # ties after the merge: 20 and 30 both reach 4 once 10 is gone
    c = _server(q, {(1,): inter([20, 30], [4, 4])}, 8)
    assert reduce_data_tables(q, _wire([c])).rows == [(1, 2, 30.0, 20.0, 30.0, 25.0, 8)]


def test_float_keys_merge_by_their_bits():
    q = parse_sql(SEL + "DISTINCTCOUNT(d), MODE(d) FROM t")
    nan = float("nan")

    def inter(values, counts):
        return {(): [ValueSet(values, PGPU_DOUBLE), ValueMap(values, counts, PGPU_DOUBLE)]}

    a = _server(q, inter([-0.0, 1.0, nan], [1, 1, 2]), 4)
    other_nan = struct.unpack(">d", H("fff8000000000001"))[0]  # another NaN's bits: the same key
    b = _server(q, inter([0.0, 1.0, other_nan], [1, 1, 2]), 4)
    (row,) = reduce_data_tables(q, _wire([a, b])).rows
    assert row[0] == 4  # -0.0, 0.0, 1.0 and one NaN
    assert math.isnan(row[1])  # NaN x4 against 1.0 x2
    # an aggregation-only reduce with no server row at all: the functions' empty results
    q2 = parse_sql(SEL + "DISTINCTCOUNT(d), PERCENTILE(d, 50), MODE(d) FROM t")
    assert reduce_data_tables(q2, [DataTable(None)]).rows == [(0, -math.inf, -math.inf)]


def test_results_without_value_sets_stay_refused():
    for sql in ("DISTINCTCOUNT(c) FROM t", "g, PERCENTILE(c, 50) FROM t GROUP BY g", "MODE(c, 'AVG') FROM t"):
        q = parse_sql(SEL + sql)
        r = QueryResult(q)
        with pytest.raises(UnsupportedPlanError, match="no intermediate result"):
            r.intermediate
        with pytest.raises(UnsupportedPlanError, match="no DataTable"):
            server_data_table(q, r, [PGPU_INT] * len(q.group_by))
        final = DataTable(DataSchema(list(q.group_by) + ["v"], ["INT"] * len(q.group_by) + ["DOUBLE"]), [])
        with pytest.raises(UnsupportedPlanError, match="no DataTable"):
            reduce_data_tables(q, [final])
        r.value_sets = True  # execute_mergeable's mark: nothing raises (there is nothing in it either)
        assert r.intermediate is None


def test_new_symbols_are_exported_and_the_abi_is_unchanged():
    lib = _lib.load()
    assert lib.pgpu_abi_version() == _lib.ABI_VERSION == 13
    sig = {n: a for n, _, a in _lib.SIGNATURES}
    assert len(sig["pgpu_table_runs"]) == 9 and len(sig["pgpu_query_collect_runs"]) == 13
    assert hasattr(lib, "pgpu_table_runs") and hasattr(lib, "pgpu_query_collect_runs")
    # host-only refusals reach the caller before any device is touched
    L = _lib.TableLayout()
    L.num_keys, L.num_sections = 6, 1
    assert lib.pgpu_table_runs(None, C.byref(L), None, None, 3, None, None, None, 0) == _lib.PGPU_E_INVALID
    n = C.c_uint64()
    assert lib.pgpu_query_collect_runs(None, 1, None, None, 0, C.byref(n), None, None, None, 0, C.byref(n), None,
                                       None) == _lib.PGPU_E_INVALID
    from pinot_amd.plan import GpuPlanMaker
    assert all(hasattr(GpuPlanMaker, m) for m in ("execute_mergeable", "submit_mergeable", "collect_mergeable"))
