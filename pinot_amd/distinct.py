"""DISTINCTCOUNT on the GPU path: lowered to GROUP BY queries whose tables are folded on the device, and raised back.

DistinctCountAggregationFunction (core/query/aggregation/function/DistinctCountAggregationFunction.java:66-250) keeps a
bitmap of the column's dictionary ids per group and turns it into a value set only to merge segments (:252-310); the
final result is the set's size as an INT (:303-310).  With the sorted global dictionaries of the group-by path, "which
(group, id) pairs occur" is the occupancy of the table ``GROUP BY g_1..g_n, c`` builds, so a query ``Q`` with
aggregations ``A + {DISTINCTCOUNT(c)}`` over group columns ``g`` runs as

    Q'  = aggregations A (COUNT(*) when A is empty), GROUP BY g_1..g_n, c      (c last: key = g + inner * cid)

and the partial table of ``Q'`` is folded over ``cid`` on the device (pgpu_query_collect_fold, include/pinot_gpu.h)
into the table ``GROUP BY g`` alone produces plus one section: the number of occupied ``cid`` per ``g``.

Several DISTINCTCOUNT columns run one pass each, all in flight together like the passes of FILTER clauses; the first
carries ``A``, the others only COUNT(*); a column named twice is computed once.  The passes share the filter, so they
meet the same groups and are joined on the group key.

Exact PERCENTILE (PercentileAggregationFunction.java:82-100,152-165: every value of the column per group, sorted,
``values[(int) ((long) size * percentile / 100)]``) rides the same passes: the global dictionary of ``c`` is sorted, so
the counts of ``Q'`` along ``cid`` are that sorted multiset, and the device picks the smallest ``cid`` whose running
count passes the rank behind the fold (pgpu_query_collect_select).  One pass per column carries DISTINCTCOUNT(c) and
every percentile of ``c`` together -- one table, one fold, K picks; the final value is ``float(dictionary[cid])``.

Exact MODE (ModeAggregationFunction.java:463-672: a value -> count map per group, the value of the largest count, and
of several such values the smallest, the largest or their mean, :59-75) rides them too: the counts of ``Q'`` along
``cid`` are that map, and one reduction behind the fold (pgpu_query_collect_mode) leaves per group the largest count,
the number of tied ids, the smallest and the largest of them and -- for the AVG reducer -- the sum of their values.  The
pass of ``c`` carries every MODE of ``c`` whatever its reducer: one table, one fold, one mode reduction.

Those are final values, right for a table on one server.  What a broker merges across servers is the value set, the
value list and the value -> count map, and the counts of ``Q'`` along ``cid`` are all three: the mergeable execution
(GpuPlanMaker.execute_mergeable) runs the same passes and collects, per group, the occupied ``cid`` with their counts --
value runs (pgpu_query_collect_runs) -- from which ``raise_runs`` computes the same rows on the host and the
intermediates ``ValueSet`` / ``ValueList`` / ``ValueMap`` (written and merged by pinot_amd/datatable.py).
"""
from __future__ import annotations

import copy
import math
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from . import _lib
from ._lib import UnsupportedPlanError
from .query import HLL_AGGS, MODE_REDUCERS, MV_AGGS, AggregationSpec, OrderByExpr, QueryContext

UNLIMITED = 1 << 62
DISTINCT = "DISTINCTCOUNT"
PERCENTILE = "PERCENTILE"
MODE = "MODE"
FOLDED = (DISTINCT, PERCENTILE, MODE)  # the functions answered from the table folded over their column
MODE_BITS = {"MIN": _lib.PGPU_MODE_MIN, "MAX": _lib.PGPU_MODE_MAX, "AVG": _lib.PGPU_MODE_AVG}
HLL, RAWHLL = HLL_AGGS
SKETCHED = HLL_AGGS  # the functions answered from the HyperLogLog registers raised beside the fold (pinot_amd/hll.py)


def has_distinct(query: QueryContext) -> bool:
    return any(a.function in FOLDED or a.function in SKETCHED for a in query.aggregations)


def has_sketches(query: QueryContext) -> bool:
    return any(a.function in SKETCHED for a in query.aggregations)


def folded_names(query: QueryContext) -> str:
    """The folded functions a query holds, for messages: 'DISTINCTCOUNT', 'PERCENTILE', 'MODE' or several of them as
    'DISTINCTCOUNT / PERCENTILE'."""
    return " / ".join(f for f in FOLDED + SKETCHED if any(a.function == f for a in query.aggregations))


def _unsupported(why: str) -> UnsupportedPlanError:
    return UnsupportedPlanError(_lib.PGPU_E_UNSUPPORTED, why)


@dataclass
class DistinctPass:
    """One pass of a DISTINCTCOUNT / PERCENTILE / MODE query."""
    query: QueryContext     # Q': GROUP BY g..., column with the pass's plain aggregations
    folded: QueryContext    # what the folded table answers: GROUP BY g... with Q's aggregations + DISTINCTCOUNT(column)
                            # + the pass's percentiles (their cells hold the selected ids of column) + when the pass
                            # has a MODE: MODE(column, 'MIN'), MODE(column, 'MAX') (the cells LO and HI: ids of
                            # column) and, when asked for, MODE(column, 'AVG') (S / T: already the value)
    column: str             # the folded column
    plain: List[int]        # original indexes of Q's aggregations, in their order ([]: Q' carries an inserted COUNT(*))
    distinct: List[int]     # original indexes of DISTINCTCOUNT(column) (every mention of it)
    percentile: List[int] = field(default_factory=list)  # original indexes of PERCENTILE(column, p), one pick each

    mode: List[int] = field(default_factory=list)  # original indexes of MODE(column, reducer), every reducer
    # a sketch pass (collected through pgpu_query_collect_hll; distinct, percentile and mode are empty then): original
    # indexes of DISTINCTCOUNTHLL(column, log2m) / DISTINCTCOUNTRAWHLL(column, log2m), and their log2m
    sketch: List[int] = field(default_factory=list)
    log2m: int = 0

    @property
    def reducers(self) -> int:
        """The reducer mask of the pass's mode reduction (PGPU_MODE_*), 0 without a MODE."""
        mask = 0
        for a in self.folded.aggregations:
            if a.function == MODE:
                mask |= MODE_BITS[a.reducer]
        return mask

    @property
    def percentiles(self) -> List[float]:
        """The pass's percentiles, in the order of its pick sections."""
        return [a.percentile for a in self.folded.aggregations if a.function == PERCENTILE]


def lower(query: QueryContext) -> List[DistinctPass]:
    """The passes of a DISTINCTCOUNT / PERCENTILE / MODE query.  Raises UnsupportedPlanError for the combinations not
    served."""
    if not has_distinct(query):
        raise ValueError("query has no DISTINCTCOUNT, PERCENTILE or MODE")
    what = folded_names(query)
    if query.has_filtered_aggregations:
        raise _unsupported(f"{what} in a query with FILTER(WHERE ...) aggregations")
    if any(a.function in MV_AGGS for a in query.aggregations):
        raise _unsupported(f"{what} together with *MV aggregations")
    plain = [i for i, a in enumerate(query.aggregations) if a.function not in FOLDED and a.function not in SKETCHED]
    by_col: Dict[str, Tuple[List[int], List[int], List[int]]] = {}
    sketches: Dict[str, List[int]] = {}
    for i, a in enumerate(query.aggregations):
        if a.function in FOLDED or a.function in SKETCHED:
            if a.column in query.group_by:
                raise _unsupported(f"{a.function} of the group column {a.column!r}")
        if a.function in FOLDED:
            by_col.setdefault(a.column, ([], [], []))[FOLDED.index(a.function)].append(i)
        elif a.function in SKETCHED:
            from .hll import check_log2m
            check_log2m(a.log2m)
            mine = sketches.setdefault(a.column, [])
            if mine and query.aggregations[mine[0]].log2m != a.log2m:
                raise _unsupported(f"{a.function} of {a.column!r} with log2m {a.log2m} beside log2m "
                                   f"{query.aggregations[mine[0]].log2m}: one sketch size per column and query")
            mine.append(i)
    passes = []
    for k, (col, (idx, pidx, midx)) in enumerate(by_col.items()):
        if len(pidx) > _lib.PGPU_SELECT_MAX:
            raise _unsupported(f"{len(pidx)} percentiles of {col!r} (at most {_lib.PGPU_SELECT_MAX} per column)")
        mine = plain if k == 0 else []
        aggs = [query.aggregations[i] for i in mine] or [AggregationSpec("COUNT", None)]
        groups = list(query.group_by)
        low = QueryContext(table=query.table, select=groups + [col] + aggs, aggregations=list(aggs),
                           filter=query.filter, group_by=groups + [col], order_by=[], limit=UNLIMITED,
                           options=dict(query.options))
        faggs = list(aggs) + [AggregationSpec(DISTINCT, col)] + [query.aggregations[i] for i in pidx]
        if midx:  # LO and HI are always there; S only when the AVG reducer is asked for
            faggs += [AggregationSpec(MODE, col, reducer=r) for r in ("MIN", "MAX")]
            if any(query.aggregations[i].reducer == "AVG" for i in midx):
                faggs.append(AggregationSpec(MODE, col, reducer="AVG"))
        folded = QueryContext(table=query.table, select=groups + faggs, aggregations=faggs, filter=query.filter,
                              group_by=groups, order_by=[], limit=UNLIMITED, options=dict(query.options))
        passes.append(DistinctPass(low, folded, col, list(mine), idx, pidx, midx))
    # a sketch of c is a pass of its own, whatever else the query asks of c: the same Q', its folded table as the fold
    # leaves it (the stage appends no section), the registers beside it.  HLL and RAWHLL of one column share it.
    for col, sidx in sketches.items():
        mine = plain if not passes else []
        aggs = [query.aggregations[i] for i in mine] or [AggregationSpec("COUNT", None)]
        groups = list(query.group_by)
        low = QueryContext(table=query.table, select=groups + [col] + aggs, aggregations=list(aggs),
                           filter=query.filter, group_by=groups + [col], order_by=[], limit=UNLIMITED,
                           options=dict(query.options))
        faggs = list(aggs) + [AggregationSpec(DISTINCT, col)]
        folded = QueryContext(table=query.table, select=groups + faggs, aggregations=faggs, filter=query.filter,
                              group_by=groups, order_by=[], limit=UNLIMITED, options=dict(query.options))
        passes.append(DistinctPass(low, folded, col, list(mine), [], sketch=sidx,
                                   log2m=query.aggregations[sidx[0]].log2m))
    return passes


def order_pass(query: QueryContext, passes: Sequence[DistinctPass]) -> Optional[Tuple[int, OrderByExpr]]:
    """(pass, expression) the server's ORDER BY trim selects by: the first ORDER BY expression, in the pass whose folded
    table holds it -- a group column or a plain aggregation in the first pass, DISTINCTCOUNT(c), a percentile of c or a
    MIN / MAX-reducer MODE of c in c's pass (its cell is an id of c: the order of the ids is the order of the values).
    A MODE is matched by function, column and reducer -- mode(c) names every reducer of c; the mean of several modes
    is no cell of the table to order by.  The other passes return every group; the join keeps the groups every pass
    returned."""
    if not query.group_by or not query.order_by:
        return None
    ob = query.order_by[0]
    if any(ob.expression == query.aggregations[i].result_name for p in passes for i in p.sketch):
        return None  # ORDER BY a sketch's estimate: every group returns and the host orders (a trim only saves bytes)
    if passes[0].sketch:
        return None  # only sketch passes (the exact ones come first), whose collect takes no order: likewise
    if ob.aggregation is not None and ob.aggregation.function == MODE:
        if ob.aggregation.reducer == "AVG":
            raise _unsupported(f"ORDER BY MODE({ob.aggregation.column}, 'AVG'): the trim on the device orders by a "
                               "mode's dictionary id, which the mean of several modes does not have")
        for pi, p in enumerate(passes):
            if ob.aggregation in p.folded.aggregations:
                return pi, ob
    for pi, p in enumerate(passes):
        if any(ob.expression == a.result_name for a in p.folded.aggregations if a.function in (DISTINCT, PERCENTILE)):
            return pi, ob
    return 0, ob


def _join_stats(query: QueryContext, results: Sequence):
    """Statistics of the joined passes: the doc counts of one pass (every pass has the same filter),
    numEntriesScannedPostFilter over the original query's projected columns (they include the distinct columns),
    kernel time and byte counters summed."""
    st = copy.copy(results[0].stats)
    for r in results[1:]:
        st.kernel_ms += r.stats.kernel_ms
        st.sparse_sector_bytes += r.stats.sparse_sector_bytes
        st.dense_bytes += r.stats.dense_bytes
    st.num_entries_scanned_post_filter = st.num_docs_scanned * len(query.projected_columns)
    return st


@dataclass
class PassSketches:
    """What one sketch pass's pgpu_query_collect_hll brought back: the folded rows decoded (a QueryResult of the pass's
    plain aggregations + DISTINCTCOUNT(column), groups ascending by key) and the register words of those rows."""
    result: object          # QueryResult
    words: object           # uint32 [rows][W]
    log2m: int

    def sketch(self, row: int):
        """The HyperLogLog of a row; row < 0 (no doc matched): the empty sketch."""
        from .hll import HyperLogLog
        return HyperLogLog.empty(self.log2m) if row < 0 else HyperLogLog(self.log2m, self.words[row].copy())


def place_sketches(query: QueryContext, p: DistinctPass, sketch, fin: list, inter: Optional[list] = None) -> None:
    """The finals of a sketch pass's functions: the estimate as a LONG, for the raw form the lowercase hex of the
    serialised sketch (SerializedHLL.java:39-41); their intermediate is the sketch."""
    for i in p.sketch:
        fin[i] = sketch.to_bytes().hex() if query.aggregations[i].function == RAWHLL else sketch.cardinality()
        if inter is not None:
            inter[i] = sketch


def raise_result(query: QueryContext, passes: Sequence[DistinctPass], results: Sequence):
    """The original query's QueryResult from the passes' folded results (QueryResults of ``DistinctPass.folded``; a pass
    with percentiles or modes carries the global dictionary of its column as ``value_dictionary``; a sketch pass comes
    as PassSketches)."""
    from .plan import QueryResult, order_and_limit, to_select_order

    sketches = [r if isinstance(r, PassSketches) else None for r in results]
    results = [r.result if isinstance(r, PassSketches) else r for r in results]
    res = QueryResult(query=query, stats=_join_stats(query, results))
    na = len(query.aggregations)
    dicts = {id(p): r.value_dictionary for p, r in zip(passes, results) if p.percentile or p.mode}

    def place(fin: list, p: DistinctPass, vals: Sequence, sk=None, row: int = -1) -> None:
        for j, i in enumerate(p.plain):
            fin[i] = vals[j]
        if p.sketch:
            place_sketches(query, p, sk.sketch(row), fin)
            return
        nm = sum(a.function == MODE for a in p.folded.aggregations)
        nd = len(vals) - 1 - len(p.percentile) - nm  # plain aggregations, the distinct count, the picks, the modes
        for i in p.distinct:
            fin[i] = int(vals[nd])  # ColumnDataType.INT (DistinctCountAggregationFunction.java:303-310)
        for j, i in enumerate(p.percentile):
            # DOUBLE; no value met: DEFAULT_FINAL_RESULT (PercentileAggregationFunction.java:152-165)
            fin[i] = float(dicts[id(p)][int(vals[nd + 1 + j])]) if int(vals[nd]) > 0 else -math.inf
        for i in p.mode:
            # DOUBLE.  MIN / MAX: the value of the smallest / largest tied id, converted once; AVG: S / T, taken where
            # the cells are decoded (plan.mode_value).  No value met (M = 0, as the distinct count):
            # DEFAULT_FINAL_RESULT (ModeAggregationFunction.java:61,468-470)
            r = query.aggregations[i].reducer
            v = vals[len(vals) - nm + MODE_REDUCERS.index(r)]
            if int(vals[nd]) <= 0:
                fin[i] = -math.inf
            else:
                fin[i] = float(v) if r == "AVG" else float(dicts[id(p)][int(v)])

    if not query.group_by:
        fin: list = [None] * na
        for p, r, sk in zip(passes, results, sketches):
            place(fin, p, r.aggregation_result, sk, 0 if sk is not None and len(sk.words) else -1)
        res.aggregation_result = fin
        res.rows = [to_select_order(query, tuple(fin))]
        return res
    ng = len(query.group_by)
    # (a sketch pass's rows are ascending by key, as its words: the row of a group is its position)
    index = [{tuple(r[:ng]): k for k, r in enumerate(rr.group_rows)} for rr in results]
    rows = []
    for r in results[0].group_rows:
        key = tuple(r[:ng])
        if not all(key in m for m in index[1:]):
            continue  # trimmed away by the pass that carries the ORDER BY expression
        fin = [None] * na
        for p, rr, m, sk in zip(passes, results, index, sketches):
            place(fin, p, rr.group_rows[m[key]][ng:], sk, m[key])
        rows.append(key + tuple(fin))
    res._group_rows = rows
    res.rows = [to_select_order(query, r) for r in order_and_limit(query, rows)]
    return res


def value_key(v):
    """Identity of a column value in a distinct set: FLOAT / DOUBLE by their bits (one NaN), as the group keys."""
    if isinstance(v, float):
        return ("f", "nan" if math.isnan(v) else struct.pack(">d", v))
    return v


def value_keys(values) -> set:
    """value_key of every entry of a dictionary (numpy array or list of strings) or list of group values."""
    vals = values.tolist() if hasattr(values, "tolist") else list(values)
    return {value_key(v) for v in vals}


# ---- the mergeable intermediates: value runs (pgpu_query_collect_runs) ----------------------------------------------
@dataclass
class ValueSet:
    """DISTINCTCOUNT's intermediate (DistinctCountAggregationFunction.java:252-310): the distinct values, ascending."""
    values: list
    stored_type: int  # PGPU_INT .. PGPU_STRING: which of the reference's sets it is on the wire


@dataclass
class ValueList:
    """PERCENTILE's intermediate (PercentileAggregationFunction.java:82-100), a list of doubles, kept as runs: the
    ascending distinct values with their counts."""
    values: list
    counts: list


@dataclass
class ValueMap:
    """MODE's intermediate (ModeAggregationFunction.java:416-456), value -> count, ascending by value."""
    values: list
    counts: list
    stored_type: int  # PGPU_INT .. PGPU_DOUBLE: which of the reference's maps it is on the wire


def value_order(v):
    """Sort key of column values as Arrays.sort orders doubles: -0.0 before 0.0, NaN last."""
    if isinstance(v, float):
        return (1, 0.0, 0.0) if math.isnan(v) else (0, v, math.copysign(1.0, v))
    return v


def merge_runs(parts) -> Tuple[list, list]:
    """(values, counts) of several runs united: counts of one value (value_key: by bits, one NaN) added, ascending."""
    acc: Dict[object, list] = {}
    for values, counts in parts:
        for v, c in zip(values, counts):
            e = acc.get(value_key(v))
            if e is None:
                acc[value_key(v)] = [v, int(c)]
            else:
                e[1] += int(c)
    items = sorted(acc.values(), key=lambda e: value_order(e[0]))
    return [e[0] for e in items], [e[1] for e in items]


def select_rank(n: int, p: float) -> int:
    """pgpu_select.hip's select_rank: PercentileAggregationFunction.java:152-165 in IEEE double."""
    if p == 100.0:
        return n - 1
    return min(int(float(n) * p / 100.0), n - 1)


def runs_percentile(values, counts, p: float) -> float:
    """The percentile of sorted runs; no value: DEFAULT_FINAL_RESULT."""
    n = int(sum(counts))
    if n <= 0:
        return -math.inf
    r, run = select_rank(n, p), 0
    for v, c in zip(values, counts):
        run += c
        if run > r:
            return float(v)
    return float(values[-1])


def runs_mode(values, counts, reducer: str) -> float:
    """ModeAggregationFunction.java:486-672 over ascending runs: the value of the largest count, of several the
    smallest, the largest or their mean (each converted to double before it is added); none: DEFAULT_FINAL_RESULT."""
    if not len(values):
        return -math.inf
    m = max(counts)
    tied = [v for v, c in zip(values, counts) if c == m]
    if reducer == "MIN":
        return float(tied[0])
    if reducer == "MAX":
        return float(tied[-1])
    s = 0.0
    for v in tied:
        s += float(v)
    return s / len(tied)


@dataclass
class PassRuns:
    """What one pass's pgpu_query_collect_runs brought back: the folded rows decoded (a QueryResult of the pass's
    plain aggregations + DISTINCTCOUNT(column), groups ascending by key) and the runs of those rows."""
    result: object          # QueryResult
    offsets: object         # uint64 [rows + 1]
    cids: object            # uint32 [runs]: ids of `dictionary`
    counts: object          # int64 [runs]
    dictionary: object      # the global dictionary of the pass's column (numpy array or list of str)
    stored_type: int


def raise_runs(query: QueryContext, passes: Sequence[DistinctPass], runs: Sequence[PassRuns]):
    """The original query's QueryResult from the passes' value runs: finals computed here on the host, and the
    intermediates -- ValueSet per DISTINCTCOUNT, ValueList per PERCENTILE, ValueMap per MODE -- per group."""
    from .plan import QueryResult, order_and_limit, to_select_order

    res = QueryResult(query=query, stats=_join_stats(query, [pr.result for pr in runs]))
    res.value_sets = True
    na = len(query.aggregations)
    ng = len(query.group_by)

    def place(fin: list, inter: list, p: DistinctPass, pr, row: int, vals: Sequence, ivals: Sequence) -> None:
        for j, i in enumerate(p.plain):
            fin[i], inter[i] = vals[j], ivals[j]
        if p.sketch:  # (pr: PassSketches)
            place_sketches(query, p, pr.sketch(row), fin, inter)
            return
        lo, hi = (int(pr.offsets[row]), int(pr.offsets[row + 1])) if row >= 0 else (0, 0)
        d = pr.dictionary
        ids = pr.cids[lo:hi]
        values = [d[int(c)] for c in ids] if isinstance(d, list) else d[ids].tolist()
        counts = pr.counts[lo:hi].tolist()
        for i in p.distinct:
            fin[i], inter[i] = len(values), ValueSet(values, pr.stored_type)
        if p.percentile:
            fv = [float(v) for v in values]
            for i in p.percentile:
                fin[i] = runs_percentile(values, counts, query.aggregations[i].percentile)
                inter[i] = ValueList(fv, counts)
        for i in p.mode:
            fin[i] = runs_mode(values, counts, query.aggregations[i].reducer)
            inter[i] = ValueMap(values, counts, pr.stored_type)

    def pass_intermediate(r) -> dict:
        if r._intermediate is None and r._columns is not None:
            r._intermediate = r._columns.intermediate()
        return r._intermediate or {}

    if not ng:
        fin, inter = [None] * na, [None] * na
        for p, pr in zip(passes, runs):
            nrows = len(pr.words) if p.sketch else len(pr.offsets) - 1
            place(fin, inter, p, pr, 0 if nrows else -1, pr.result.aggregation_result, pass_intermediate(pr.result)[()])
        res.aggregation_result = fin
        res._intermediate = {(): inter}
        res.rows = [to_select_order(query, tuple(fin))]
        return res
    # every pass returns every group the filter meets, ascending by key: the row of a group is the same in all
    index = [{tuple(r[:ng]): k for k, r in enumerate(pr.result.group_rows)} for pr in runs]
    inters = [pass_intermediate(pr.result) for pr in runs]
    rows, merged = [], {}
    for k, r in enumerate(runs[0].result.group_rows):
        key = tuple(r[:ng])
        if not all(key in m for m in index[1:]):
            continue
        fin, inter = [None] * na, [None] * na
        for p, pr, m, im in zip(passes, runs, index, inters):
            row = m[key]
            place(fin, inter, p, pr, row, pr.result.group_rows[row][ng:], im[key])
        rows.append(key + tuple(fin))
        merged[key] = inter
    res._group_rows = rows
    res._intermediate = merged
    res.rows = [to_select_order(query, r) for r in order_and_limit(query, rows)]
    return res


def unfolded_result(query: QueryContext, passes: Sequence[DistinctPass], results: Sequence):
    """The scanned half of a partly non-scan aggregation-only query, from the passes' *unfolded* results (QueryResults
    of ``DistinctPass.query``, one group per value of the distinct column): (QueryResult with the plain aggregations
    merged over the groups, {original aggregation index: the value set as value_key}).  Only COUNT / MIN / MAX occur
    beside DISTINCTCOUNT in a non-scan plan (AggregationPlanNode.java:185-197)."""
    from .plan import QueryResult

    na = len(query.aggregations)
    fin: list = [None] * na
    sets: Dict[int, set] = {}
    for p, r in zip(passes, results):
        rows = r.group_rows
        for j, i in enumerate(p.plain):
            fn = query.aggregations[i].function
            col = [row[1 + j] for row in rows]
            if fn == "COUNT":
                fin[i] = int(sum(col))
            elif fn == "MIN":
                fin[i] = min(col, default=math.inf)
            elif fn == "MAX":
                fin[i] = max(col, default=-math.inf)
            else:
                raise _unsupported(f"{fn} beside DISTINCTCOUNT in a non-scan plan")
        keys = value_keys([row[0] for row in rows])
        for i in p.distinct:
            sets[i] = keys
            fin[i] = len(keys)
    res = QueryResult(query=query, stats=_join_stats(query, results))
    res.aggregation_result = fin
    return res, sets
