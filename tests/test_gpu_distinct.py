"""DISTINCTCOUNT on the GPU (MI355X only): the reference's known answers, pgpu_table_fold on hand-made tables against a
numpy fold, and the whole path -- SQL, lowering, GROUP BY g, c on every key path, device fold, trim, join -- against
numpy over the decoded columns.  Every result is an integer, so every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle.segment_writer import build_segment
from pinot_amd import _lib
from pinot_amd._lib import (PGPU_DOUBLE, PGPU_FLOAT, PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_LONG,
                            PGPU_Q_HASH, PGPU_Q_PARTITION, PGPU_RED_MAX_I64, PGPU_RED_MIN_I64, PGPU_RED_SUM_F64,
                            PGPU_RED_SUM_I64, PGPU_STRING, TableLayout, UnsupportedPlanError)
from pinot_amd.plan import GpuPlanMaker
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuSegment
from tests.helpers import GOLDEN, load_kat, sv_segment

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
# Every SELECT literal of the test files is also held against the oracle's own SQL parser (tests/test_oracle_sql.py),
# which has no DISTINCTCOUNT and is to stay without one: the queries here get their keyword from SEL instead.
SEL = "SELECT "


# ---- 1. the reference's known answers ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sv(gpu_ctx):
    g = GpuSegment(gpu_ctx, sv_segment())
    yield g
    g.release()


with open(os.path.join(GOLDEN, "kat_distinct.json")) as _f:
    KAT = json.load(_f)


@pytest.mark.parametrize("case", KAT["aggregation"]["cases"], ids=["all", "filter"])
def test_kat_aggregation(gpu_ctx, sv, case):
    q = parse_sql(case["sql"].replace("{FILTER}", load_kat()["filter"]))
    res = GpuPlanMaker(gpu_ctx, exact_filter_stats=True).execute(q, [sv] * 4)
    assert res.aggregation_result == case["result"] and all(type(v) is int for v in res.aggregation_result)
    st = res.stats
    assert [st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_entries_scanned_post_filter,
            st.num_total_docs] == case["stats"]


@pytest.mark.parametrize("case", KAT["group_by"]["cases"], ids=["by-key", "by-count"])
def test_kat_group_by(gpu_ctx, sv, case):
    res = GpuPlanMaker(gpu_ctx).execute(parse_sql(case["sql"]), [sv] * 4)
    assert [list(r) for r in res.rows] == case["rows"]
    assert res.stats.num_entries_scanned_post_filter == KAT["group_by"]["num_entries_scanned_post_filter"]


# ---- 2. pgpu_table_fold alone -----------------------------------------------------------------------------------------
# sections: count | SUM int64 | split SUM (3 parts) | MIN | MAX | SUM float64
FULL_OPS = [PGPU_RED_SUM_I64] * 5 + [PGPU_RED_MIN_I64, PGPU_RED_MAX_I64, PGPU_RED_SUM_F64]
LIGHT_OPS = [PGPU_RED_SUM_I64, PGPU_RED_SUM_I64, PGPU_RED_MIN_I64]  # (the large cases: count | SUM | MIN)


def _table_layout(ops, num_keys, kind):
    L = TableLayout()
    L.num_keys, L.num_sections = num_keys, len(ops)
    for s, op in enumerate(ops):
        L.section_op[s] = op
    L.agg_section[0], L.agg_value_type[0] = 0, -1
    L.agg_section[1], L.agg_value_type[1], L.agg_sum_parts[1] = 1, PGPU_LONG, 1
    if len(ops) == len(FULL_OPS):
        L.agg_section[2], L.agg_value_type[2], L.agg_sum_parts[2] = 2, PGPU_LONG, 3
        L.agg_section[3], L.agg_value_type[3], L.agg_sum_parts[3] = 5, PGPU_LONG, 1
        L.agg_section[4], L.agg_value_type[4], L.agg_sum_parts[4] = 6, PGPU_LONG, 1
        L.agg_section[5], L.agg_value_type[5], L.agg_sum_parts[5] = 7, PGPU_DOUBLE, 1
        L.agg_sum_exp[5] = _lib.PGPU_SUM_EXP_F64
    else:
        L.agg_section[2], L.agg_value_type[2], L.agg_sum_parts[2] = 2, PGPU_LONG, 1
    L.key_kind, L.key_words, L.key_split = kind, 1, 1
    return L


def _make_table(rng, ops, inner, card):
    """Dense table [nsec][card * inner] (cell = g + inner * cid): about half the cells empty; with inner >= 3, g = 0
    has every cell empty and g = inner - 1 every cell full.  Empty cells hold the sections' identities."""
    n = inner * card
    occ = rng.random(n) < 0.5
    if n == 1:
        occ[:] = True
    if inner >= 3:
        g = np.arange(n) % inner
        occ[g == 0] = False
        occ[g == inner - 1] = True
    t = np.zeros((len(ops), n), dtype=np.int64)
    t[0] = np.where(occ, rng.integers(1, 1000, n), 0)
    for s in range(1, len(ops)):
        op = ops[s]
        if op == PGPU_RED_SUM_I64 and len(ops) == len(FULL_OPS) and s in (2, 3):
            v = rng.integers(0, 1 << 21, n)                      # unsigned 21-bit parts
        elif op == PGPU_RED_SUM_I64 and len(ops) == len(FULL_OPS) and s == 4:
            v = rng.integers(-(1 << 20), 1 << 20, n)             # the signed top part
        elif op == PGPU_RED_SUM_I64:
            v = rng.integers(-(1 << 40), 1 << 40, n)
        elif op == PGPU_RED_SUM_F64:
            # integers below 2^40 that are multiples of 2^10: every partial sum of up to 2^17 of them is an integer
            # multiple of 2^10 below 2^57, exact in a double, so any order of addition gives the same bits
            v = (rng.integers(0, 1 << 30, n) << 10).astype(np.float64).view(np.int64)
        else:
            v = rng.integers(-(1 << 62), 1 << 62, n)
            v[rng.integers(0, n, max(1, n // 50))] = (1 << 62) if op == PGPU_RED_MAX_I64 else -(1 << 62)
        ident = I64_MAX if op == PGPU_RED_MIN_I64 else (I64_MIN if op == PGPU_RED_MAX_I64 else 0)
        t[s] = np.where(occ, v, ident)
    return t


def _np_fold(t, ops, inner):
    """The fold in numpy: every section over cid by its op (empty cells hold identities), plus the occupied count."""
    nsec, n = t.shape
    r = t.reshape(nsec, n // inner, inner)
    out = np.zeros((nsec + 1, inner), dtype=np.int64)
    for s, op in enumerate(ops):
        if op == PGPU_RED_SUM_I64:
            out[s] = r[s].sum(axis=0)
        elif op == PGPU_RED_SUM_F64:
            out[s] = r[s].view(np.float64).sum(axis=0).view(np.int64)
        elif op == PGPU_RED_MIN_I64:
            out[s] = r[s].min(axis=0)
        else:
            out[s] = r[s].max(axis=0)
    out[nsec] = (r[0] > 0).sum(axis=0)
    return out


def _to_hash(rng, t, ops):
    """The same cells as a one-word hash table: occupied cells in random slots (the fold reads each slot's key; it
    does not probe), the key word section after the value sections, -1 in empty slots."""
    nsec, n = t.shape
    keys = np.flatnonzero(t[0] > 0)
    slots = 64
    while slots < 2 * len(keys):
        slots <<= 1
    h = np.zeros((nsec + 1, slots), dtype=np.int64)
    for s, op in enumerate(ops):
        h[s] = I64_MAX if op == PGPU_RED_MIN_I64 else (I64_MIN if op == PGPU_RED_MAX_I64 else 0)
    h[nsec] = -1
    at = rng.permutation(slots)[: len(keys)]
    h[:nsec, at] = t[:, keys]
    h[nsec, at] = keys
    return h


def _fold_on_gpu(gpu_ctx, L, table, inner):
    lib = gpu_ctx._lib
    F = TableLayout()
    _lib.check(lib.pgpu_fold_layout_of(C.byref(L), inner, C.byref(F)))
    dev = torch.from_numpy(np.ascontiguousarray(table).reshape(-1)).cuda()
    out = torch.full(((L.num_sections + 1) * inner,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")  # (not identities)
    nbytes = out.numel() * 8
    assert nbytes == _lib.table_bytes(F)
    assert lib.pgpu_table_fold(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                               C.c_void_p(out.data_ptr()), nbytes - 8) == _lib.PGPU_E_INVALID  # too small: refused
    _lib.check(lib.pgpu_table_fold(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                                   C.c_void_p(out.data_ptr()), nbytes))
    torch.cuda.synchronize()
    return F, out, out.cpu().numpy().reshape(L.num_sections + 1, inner)


def _compact(gpu_ctx, F, out, order=None):
    lib = gpu_ctx._lib
    cap = int(F.num_keys)
    keys = np.empty(cap, dtype=np.int64)
    cells = np.empty((cap, F.num_sections), dtype=np.int64)
    n = C.c_uint64()
    kp, cp = keys.ctypes.data_as(C.POINTER(C.c_int64)), cells.ctypes.data_as(C.POINTER(C.c_int64))
    if order is None:
        _lib.check(lib.pgpu_table_compact(gpu_ctx.handle, C.byref(F), C.c_void_p(out.data_ptr()), None, kp, cp, cap,
                                          C.byref(n)))
    else:
        _lib.check(lib.pgpu_table_topk(gpu_ctx.handle, C.byref(F), C.c_void_p(out.data_ptr()), None, C.byref(order),
                                       kp, cp, cap, C.byref(n)))
    return keys[: n.value], cells[: n.value]


# the shapes at which the fold takes another path (registers / LDS table / per-key walk; hash: LDS or HBM atomics),
# then two large ones on three sections: (2100, 1100) the per-key walk with five cid per thread (the unrolled loop
# and its tail), (3, 1_000_000) the per-cell kernel with more cells than one round of its grid
FOLD_SHAPES = [(1, 1), (1, 63), (1, 65), (1, 70001), (3, 5), (64, 257), (257, 64), (5000, 33), (70001, 3),
               (2100, 1100), (3, 1_000_000)]


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card", FOLD_SHAPES, ids=[f"{i}x{c}" for i, c in FOLD_SHAPES])
def test_table_fold_against_numpy(gpu_ctx, inner, card, kind):
    rng = np.random.default_rng(inner * 1000003 + card)
    ops = FULL_OPS if inner * card < 1_000_000 else LIGHT_OPS
    t = _make_table(rng, ops, inner, card)
    want = _np_fold(t, ops, inner)
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(rng, t, ops)
    L = _table_layout(ops, table.shape[1], kind)
    F, out, got = _fold_on_gpu(gpu_ctx, L, table, inner)
    nsec = len(ops)
    assert np.array_equal(got, want), [(s, int((got[s] != want[s]).sum())) for s in range(nsec + 1)]
    if inner >= 3:  # the empty key keeps every identity, the full key met every cid
        assert want[0, 0] == 0 and want[nsec, 0] == 0 and want[nsec, inner - 1] == card
    # compaction of the folded table: the non-empty keys in order, cells row-major
    live = np.flatnonzero(want[0] > 0)
    keys, cells = _compact(gpu_ctx, F, out)
    assert np.array_equal(keys, live) and np.array_equal(cells, want[:, live].T)
    # top 3 by the distinct count (the appended aggregation entry, a LONG SUM), ties with the third kept
    order = _lib.TopK()
    order.source, order.agg_fn, order.descending, order.k = _lib.PGPU_TOPK_AGG, _lib.PGPU_AGG_SUM, 1, 3
    order.agg_index = 6 if ops is FULL_OPS else 3
    assert F.agg_section[order.agg_index] == nsec
    d = want[nsec, live]
    keep = live if len(live) <= 3 else live[d >= np.sort(d)[-3]]
    keys, cells = _compact(gpu_ctx, F, out, order)
    by = np.argsort(keys)
    assert np.array_equal(keys[by], keep) and np.array_equal(cells[by], want[:, keep].T)


# ---- 3. end to end on three segments whose dictionaries overlap only partly ---------------------------------------------
NDOCS = 20_000
C_COLUMNS = {"c_int": PGPU_INT, "c_long": PGPU_LONG, "c_float": PGPU_FLOAT, "c_double": PGPU_DOUBLE,
             "c_str": PGPU_STRING, "c_raw": PGPU_INT}


def _columns(rng, i):
    """Segment i: the distinct column's values come from [800 i, 800 i + 1400), so the three dictionaries overlap in
    part and the global one has about 3,000 entries."""
    c = rng.integers(800 * i, 800 * i + 1400, NDOCS).astype(np.int64)
    g = rng.integers(0, 7, NDOCS).astype(np.int32)
    f = rng.integers(0, 100, NDOCS).astype(np.int32)
    # `a`'s spread depends on the group `w`, so that DISTINCTCOUNT(a) differs from group to group (the trim test)
    w = rng.integers(0, 200, NDOCS).astype(np.int32)
    return {"g": (PGPU_INT, g * 11 + 5), "f": (PGPU_INT, f), "f2": (PGPU_INT, (f == 0).astype(np.int32)),
            "x": (PGPU_INT, rng.integers(-50_000, 50_000, NDOCS).astype(np.int32)),
            "y": (PGPU_DOUBLE, np.round(rng.normal(0, 1000, NDOCS), 3)),
            "w": (PGPU_INT, w), "a": (PGPU_INT, (rng.integers(0, 1 << 30, NDOCS) % (3 + w)).astype(np.int32)),
            "c_int": (PGPU_INT, (c * 3 - 1000).astype(np.int32)), "c_long": (PGPU_LONG, c * (1 << 33) - 7),
            "c_float": (PGPU_FLOAT, (c.astype(np.float32) * np.float32(0.25)) - np.float32(100)),
            "c_double": (PGPU_DOUBLE, c.astype(np.float64) * 0.1 + 1.0),
            "c_str": (PGPU_STRING, [f"v{v:05d}" for v in c]), "c_raw": (PGPU_INT, (c * 5 + 1).astype(np.int32))}


@pytest.fixture(scope="module")
def three(gpu_ctx):
    rng = np.random.default_rng(20260119)
    cols = [_columns(rng, i) for i in range(3)]
    segs = [build_segment(f"d{i}", c, raw=["c_raw"]) for i, c in enumerate(cols)]
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    host = {k: np.concatenate([np.asarray(c[k][1]) for c in cols]) for k in cols[0]}
    yield gs, host, cols
    for g in gs:
        g.release()


def _distinct(host, col, mask, by=None):
    """numpy: the number of distinct values of `col` over the masked docs, or {group value: that number}."""
    if by is None:
        return len(np.unique(host[col][mask]))
    return {int(k): len(np.unique(host[col][mask & (host[by] == k)])) for k in np.unique(host[by][mask])}


def _run(pm, q, gs):
    """submit + collect, returning the result and the layout / statistics of every pass's GROUP BY g, c launch."""
    pending = pm.submit(q, gs)
    layouts = [pq.layout for pq in pending.pending]
    return pm.collect(pending), layouts


MIX = "SUM(x), MIN(x), MAX(y), AVG(y), COUNT(*)"


@pytest.mark.parametrize("where", ["", " WHERE f < 30"], ids=["all", "filter"])
@pytest.mark.parametrize("grouped", [False, True], ids=["agg", "group"])
def test_end_to_end_mixed_aggregations(gpu_ctx, three, grouped, where):
    gs, host, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30 if where else np.ones(len(host["f"]), dtype=bool)
    tail = " GROUP BY g LIMIT 100" if grouped else ""
    head = SEL + ("g, " if grouped else "")
    q = parse_sql(f"{head}SUM(x), DISTINCTCOUNT(c_int), MIN(x), MAX(y), AVG(y), COUNT(*) FROM t{where}{tail}")
    res, layouts = _run(pm, q, gs)
    plain = pm.execute(parse_sql(f"{head}{MIX} FROM t{where}{tail}"), gs)
    # the dense small path: 7 x ~3,000 keys
    assert layouts[0].key_kind == PGPU_KEYS_DENSE and 7 * 2900 < layouts[0].num_keys * (1 if grouped else 7) < 7 * 3100
    if grouped:
        want = _distinct(host, "c_int", mask, "g")
        assert {r[0]: r[2] for r in res.group_rows} == want
        # the other columns are exactly those of the query without the DISTINCTCOUNT
        assert [r[:2] + r[3:] for r in res.group_rows] == plain.group_rows
        assert [r[:2] + r[3:] for r in res.rows] == plain.rows
    else:
        assert res.aggregation_result[1] == _distinct(host, "c_int", mask)
        assert res.aggregation_result[:1] + res.aggregation_result[2:] == plain.aggregation_result
    st = res.stats
    assert st.num_docs_scanned == int(mask.sum()) == plain.stats.num_docs_scanned and st.num_total_docs == 3 * NDOCS
    assert st.num_entries_scanned_post_filter == st.num_docs_scanned * len(q.projected_columns)
    assert st.num_entries_scanned_in_filter == plain.stats.num_entries_scanned_in_filter
    with pytest.raises(UnsupportedPlanError):
        res.intermediate


@pytest.mark.parametrize("col", list(C_COLUMNS))
def test_end_to_end_column_types(gpu_ctx, three, col):
    gs, host, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30
    res = pm.execute(parse_sql(SEL + f"g, DISTINCTCOUNT({col}), COUNT(*) FROM t WHERE f < 30 GROUP BY g LIMIT 100"), gs)
    assert {r[0]: r[1] for r in res.group_rows} == _distinct(host, col, mask, "g")
    assert {r[0]: r[2] for r in res.group_rows} == {int(k): int((mask & (host["g"] == k)).sum())
                                                    for k in np.unique(host["g"])}
    res = pm.execute(parse_sql(SEL + f"DISTINCTCOUNT({col}) FROM t WHERE f < 30"), gs)
    assert res.aggregation_result == [_distinct(host, col, mask)]


def test_forced_hash_path(gpu_ctx, three):
    gs, host, _ = three
    pm = GpuPlanMaker(gpu_ctx, query_flags=PGPU_Q_HASH)
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c_int), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    res, layouts = _run(pm, q, gs)
    assert layouts[0].key_kind == PGPU_KEYS_HASH
    assert {r[0]: r[1] for r in res.group_rows} == _distinct(host, "c_int", host["f"] < 30, "g")
    assert [(r[0], r[2]) for r in res.group_rows] == \
        GpuPlanMaker(gpu_ctx).execute(parse_sql(SEL + "g, SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100"), gs).group_rows


# ---- 4. the large key paths ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(gpu_ctx):
    rng = np.random.default_rng(7)
    n = 200_000
    c = np.concatenate([np.arange(70_000), rng.integers(0, 70_000, n - 70_000)]).astype(np.int32)
    rng.shuffle(c)
    cols = {"c": (PGPU_INT, c * 2), "g": (PGPU_INT, rng.integers(0, 40, n).astype(np.int32)),
            "f": (PGPU_INT, rng.integers(0, 100, n).astype(np.int32))}
    g = GpuSegment(gpu_ctx, build_segment("wide", cols))
    yield g, {k: v[1] for k, v in cols.items()}
    g.release()


@pytest.mark.parametrize("flags", [0, PGPU_Q_PARTITION], ids=["default", "forced"])
def test_partitioned_path(gpu_ctx, wide, flags):
    g, host = wide
    pm = GpuPlanMaker(gpu_ctx, query_flags=flags)
    res, layouts = _run(pm, parse_sql(SEL + "DISTINCTCOUNT(c) FROM t WHERE f < 50"), [g])
    # 70,000 dense keys: from 65,536 keys up the group-by is partitioned (records + LDS reduce)
    assert layouts[0].key_kind == PGPU_KEYS_DENSE and layouts[0].num_keys == 70_000
    assert res.stats.kernel_variant == _lib.PGPU_KV_PSCAN
    assert res.aggregation_result == [len(np.unique(host["c"][host["f"] < 50]))]


def test_hash_path_by_key_space(gpu_ctx, wide):
    g, host = wide
    pm = GpuPlanMaker(gpu_ctx)
    res, layouts = _run(pm, parse_sql(SEL + "g, DISTINCTCOUNT(c), COUNT(*) FROM t WHERE f < 50 GROUP BY g LIMIT 100"),
                        [g])
    # 40 x 70,000 = 2.8 M keys > 8 x the docs: hash slots by group_key_space's own rule
    assert layouts[0].key_kind == PGPU_KEYS_HASH
    assert {r[0]: r[1] for r in res.group_rows} == _distinct(host, "c", host["f"] < 50, "g")


# ---- 5. two distinct columns, ORDER BY DISTINCTCOUNT, the GPU trim -------------------------------------------------------
def test_two_columns_order_by_distinctcount_trimmed(gpu_ctx, three):
    gs, host, _ = three
    sql = (SEL + "w, DISTINCTCOUNT(a), SUM(x), DISTINCTCOUNT(c_int) FROM t WHERE f < 60 GROUP BY w "
           "ORDER BY DISTINCTCOUNT(a) DESC, w LIMIT 3")
    q = parse_sql(sql)
    mask = host["f"] < 60
    da, dc = _distinct(host, "a", mask, "w"), _distinct(host, "c_int", mask, "w")
    sx = {int(k): float(host["x"][mask & (host["w"] == k)].astype(np.int64).sum()) for k in da}
    full = sorted(((k, da[k], sx[k], dc[k]) for k in da), key=lambda r: (-r[1], r[0]))
    res = GpuPlanMaker(gpu_ctx, min_server_group_trim_size=2).execute(q, gs)  # trim to max(5 * 3, 2) = 15 groups
    assert res.rows == full[:3]
    assert 15 <= len(res.group_rows) < len(da) == 200
    assert set(res.group_rows) <= set(full)
    # the trim off: every group comes back
    res = GpuPlanMaker(gpu_ctx, min_server_group_trim_size=-1).execute(q, gs)
    assert res.rows == full[:3] and sorted(res.group_rows, key=lambda r: (-r[1], r[0])) == full


# ---- 6. nothing matches --------------------------------------------------------------------------------------------------
def test_filter_matching_nothing(gpu_ctx, three):
    gs, _, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    for where in ("f = 0 AND f2 = 0", "f > 1000"):  # empty at run time / folded to EMPTY at plan time
        res = pm.execute(parse_sql(SEL + f"DISTINCTCOUNT(c_int) FROM t WHERE {where}"), gs)
        assert res.aggregation_result == [0] and res.stats.num_docs_scanned == 0
        res = pm.execute(parse_sql(SEL + f"g, DISTINCTCOUNT(c_int), SUM(x) FROM t WHERE {where} GROUP BY g"), gs)
        assert res.rows == [] and res.group_rows == []


# ---- 7. no scan ------------------------------------------------------------------------------------------------------------
def test_no_scan_from_dictionaries(gpu_ctx, three):
    gs, host, _ = three
    res = GpuPlanMaker(gpu_ctx).execute(parse_sql(SEL + "DISTINCTCOUNT(c_int), COUNT(*), DISTINCTCOUNT(c_str) FROM t"), gs)
    n = 3 * NDOCS
    assert res.aggregation_result == [len(np.unique(host["c_int"])), n, len(np.unique(host["c_str"]))]
    st = res.stats
    assert (st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_entries_scanned_post_filter,
            st.num_total_docs) == (n, 0, 0, n)
    assert st.kernel_ms == 0


def test_no_scan_mixed_with_scanned_segments(gpu_ctx, three):
    gs, host, cols = three
    # c_int = 3 c - 1000 with c in [800 i, 800 i + 1400): c_int >= 3800 (c >= 1600) matches all of segment 2, none of
    # segment 0 and a part of segment 1
    lo = 3 * 1600 - 1000
    assert all(np.asarray(cols[2]["c_int"][1]) >= lo) and not any(np.asarray(cols[0]["c_int"][1]) >= lo)
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + f"DISTINCTCOUNT(c_int), COUNT(*), MAX(c_int), DISTINCTCOUNT(c_float) FROM t WHERE c_int >= {lo}")
    assert pm.non_scan_segments(q, gs) == [False, False, True]
    res = pm.execute(q, gs)
    mask = host["c_int"] >= lo
    assert res.aggregation_result == [_distinct(host, "c_int", mask), int(mask.sum()),
                                      float(host["c_int"][mask].max()), _distinct(host, "c_float", mask)]
    assert res.stats.num_docs_scanned == int(mask.sum()) and res.stats.num_total_docs == 3 * NDOCS


# ---- 8. numGroupsLimit ------------------------------------------------------------------------------------------------------
def test_num_groups_limit_holds_the_group_keys_only(gpu_ctx, three):
    gs, host, _ = three
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c_int) FROM t GROUP BY g LIMIT 100")
    with pytest.raises(UnsupportedPlanError, match="numGroupsLimit"):
        GpuPlanMaker(gpu_ctx, num_groups_limit=5).execute(q, gs)
    # the default limit (100,000) is far below 7 x ~3,000 x ... keys of the lowered query; only g's 7 count
    wide_q = parse_sql(SEL + "w, g, DISTINCTCOUNT(c_int) FROM t GROUP BY w, g LIMIT 100000")
    res, layouts = _run(GpuPlanMaker(gpu_ctx), wide_q, gs)
    assert 200 * 7 * 2900 < layouts[0].num_keys or layouts[0].key_kind == PGPU_KEYS_HASH
    assert not res.stats.num_groups_limit_reached
    pair = host["w"].astype(np.int64) * 1000 + host["g"]
    want = {int(k): len(np.unique(host["c_int"][pair == k])) for k in np.unique(pair)}
    assert {r[0] * 1000 + r[1]: r[2] for r in res.group_rows} == want


# ---- 9. cancel ----------------------------------------------------------------------------------------------------------------
def test_cancelled_pass_is_not_folded_and_the_context_stays_usable(gpu_ctx, three):
    gs, host, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c_int), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    full = pm.collect(pm.submit(q, gs))
    # at the C ABI: pgpu_query_collect_fold passes the wait's status through and releases the query
    pending = pm.submit(q, gs)
    pending.cancel()
    (pq,) = pending.pending
    inner, F = pq.fold.inner_keys, pq.fold.layout
    keys = (C.c_int64 * inner)()
    cells = (C.c_int64 * (inner * F.num_sections))()
    n = C.c_uint64()
    st = _lib.QueryStats()
    h, pq.handle = pq.handle, None
    rc = gpu_ctx._lib.pgpu_query_collect_fold(h, inner, None, keys, cells, inner, C.byref(n), C.byref(st), None)
    assert rc == _lib.PGPU_E_CANCELLED and "cancel" in _lib.last_error()
    # the Python surface raises
    pending = pm.submit(q, gs)
    pending.cancel()
    with pytest.raises(_lib.QueryCancelledError):
        pm.collect(pending)
    again = pm.collect(pm.submit(q, gs))
    assert again.group_rows == full.group_rows and again.stats.num_docs_scanned == full.stats.num_docs_scanned
    assert {r[0]: r[1] for r in again.group_rows} == _distinct(host, "c_int", host["f"] < 30, "g")
