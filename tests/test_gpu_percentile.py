"""Exact PERCENTILE on the GPU (MI355X only): the reference's known answers, pgpu_table_select on hand-made tables
against numpy (cumsum over cid and searchsorted), and the whole path -- SQL, lowering, GROUP BY g, c on every key path,
device fold and pick, trim, join -- against a sort over the decoded columns.  Every selected value is a dictionary
entry, so every comparison is exact."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

from oracle.segment_writer import build_segment
from pinot_amd import _lib
from pinot_amd._lib import (PGPU_DOUBLE, PGPU_FLOAT, PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_LONG,
                            PGPU_Q_HASH, PGPU_RED_MAX_I64, PGPU_RED_MIN_I64, PGPU_RED_SUM_I64, PGPU_STRING,
                            TableLayout, UnsupportedPlanError)
from pinot_amd.plan import GpuPlanMaker
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuSegment
from tests.helpers import GOLDEN, load_kat, sv_segment

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
# Every SELECT literal of the test files is also held against the oracle's own SQL parser (tests/test_oracle_sql.py),
# which has no PERCENTILE and is to stay without one: the queries here get their keyword from SEL instead, and the
# reference's query texts live in tests/golden/kat_percentile.json.
SEL = "SELECT "


# ---- 1. the reference's known answers ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sv(gpu_ctx):
    g = GpuSegment(gpu_ctx, sv_segment())
    yield g
    g.release()


with open(os.path.join(GOLDEN, "kat_percentile.json")) as _f:
    KAT = json.load(_f)


@pytest.mark.parametrize("case", KAT["aggregation"]["cases"],
                         ids=[f"{i}-{c['stats']}" for i, c in enumerate(KAT["aggregation"]["cases"])])
def test_kat_aggregation(gpu_ctx, sv, case):
    q = parse_sql(case["sql"].replace("{FILTER}", load_kat()["filter"]))
    res = GpuPlanMaker(gpu_ctx, exact_filter_stats=True).execute(q, [sv] * 4)
    assert res.aggregation_result == case["result"] and all(type(v) is float for v in res.aggregation_result)
    st = res.stats
    assert [st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_entries_scanned_post_filter,
            st.num_total_docs] == KAT["aggregation"]["stats"][case["stats"]]


@pytest.mark.parametrize("case", KAT["group_by"]["cases"], ids=["three-ties"])
def test_kat_group_by(gpu_ctx, sv, case):
    res = GpuPlanMaker(gpu_ctx).execute(parse_sql(case["sql"]), [sv] * 4)
    assert [list(r) for r in res.rows] == case["rows"] and all(type(r[1]) is float for r in res.rows)
    assert res.stats.num_entries_scanned_post_filter == KAT["group_by"]["num_entries_scanned_post_filter"]


# ---- 2. pgpu_table_select alone -----------------------------------------------------------------------------------------
OPS = [PGPU_RED_SUM_I64, PGPU_RED_SUM_I64, PGPU_RED_MIN_I64, PGPU_RED_MAX_I64]  # count | SUM | MIN | MAX
NSEC = len(OPS)
PS = [0.0, 33.3, 50.0, 90.0, 99.9, 100.0]


def _table_layout(num_keys, kind):
    L = TableLayout()
    L.num_keys, L.num_sections = num_keys, NSEC
    for s, op in enumerate(OPS):
        L.section_op[s] = op
    L.agg_section[0], L.agg_value_type[0] = 0, -1
    for a in (1, 2, 3):
        L.agg_section[a], L.agg_value_type[a], L.agg_sum_parts[a] = a, PGPU_LONG, 1
    L.key_kind, L.key_words, L.key_split = kind, 1, 1
    return L


def _fill(rng, counts):
    """The table [NSEC][n] of these counts: random values where count > 0, the sections' identities elsewhere."""
    n = len(counts)
    t = np.zeros((NSEC, n), dtype=np.int64)
    t[0] = counts
    occ = counts > 0
    t[1] = np.where(occ, rng.integers(-(1 << 40), 1 << 40, n), 0)
    t[2] = np.where(occ, rng.integers(-(1 << 62), 1 << 62, n), I64_MAX)
    t[3] = np.where(occ, rng.integers(-(1 << 62), 1 << 62, n), I64_MIN)
    return t


def _random_counts(rng, inner, card):
    """Counts in [1, 1000) with about half the cells empty (cell = g + inner * cid); with inner >= 3, g = 0 has every
    cell empty and g = inner - 1 every cell full."""
    n = inner * card
    occ = rng.random(n) < 0.5
    if n == 1:
        occ[:] = True
    if inner >= 3:
        g = np.arange(n) % inner
        occ[g == 0] = False
        occ[g == inner - 1] = True
    return np.where(occ, rng.integers(1, 1000, n), 0)


def _np_select(t, inner, ps):
    """The fold and the selection in numpy: [NSEC + 1 + K][inner].  Per g: cumsum over cid and
    searchsorted(cum, r, side="right") with r = N - 1 at 100, else int(double(N) * p / 100.0)."""
    r3 = t.reshape(NSEC, -1, inner)
    out = np.zeros((NSEC + 1 + len(ps), inner), dtype=np.int64)
    out[0], out[1], out[2], out[3] = r3[0].sum(axis=0), r3[1].sum(axis=0), r3[2].min(axis=0), r3[3].max(axis=0)
    out[NSEC] = (r3[0] > 0).sum(axis=0)
    N = out[0]
    ranks = np.stack([N - 1 if p == 100.0 else (N.astype(np.float64) * p / 100.0).astype(np.int64) for p in ps])
    cum = np.cumsum(r3[0], axis=0)
    for g in np.flatnonzero(N > 0):
        out[NSEC + 1:, g] = np.searchsorted(cum[:, g], ranks[:, g], side="right")
    return out


def _to_hash(rng, t):
    """The same cells as a one-word hash table: occupied cells in random slots, the key word section after the value
    sections, -1 in empty slots."""
    keys = np.flatnonzero(t[0] > 0)
    slots = 64
    while slots < 2 * len(keys):
        slots <<= 1
    h = np.zeros((NSEC + 1, slots), dtype=np.int64)
    h[2], h[3], h[NSEC] = I64_MAX, I64_MIN, -1
    at = rng.permutation(slots)[: len(keys)]
    h[:NSEC, at] = t[:, keys]
    h[NSEC, at] = keys
    return h


def _select_on_gpu(gpu_ctx, L, table, inner, ps):
    """pgpu_table_fold and pgpu_table_select of the same device table: (selected layout, device output, host copy of
    the selected table, host copy of the folded table)."""
    lib = gpu_ctx._lib
    k = len(ps)
    S = TableLayout()
    _lib.check(lib.pgpu_select_layout_of(C.byref(L), inner, k, C.byref(S)))
    dev = torch.from_numpy(np.array(table).reshape(-1)).cuda()  # (a copy: the shared tables are read-only)
    folded = torch.full(((NSEC + 1) * inner,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    out = torch.full(((NSEC + 1 + k) * inner,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")  # (not the answers)
    nbytes = out.numel() * 8
    assert nbytes == _lib.table_bytes(S)
    pp = (C.c_double * k)(*ps)
    args = (gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner, pp, k, C.c_void_p(out.data_ptr()))
    assert lib.pgpu_table_select(*args, nbytes - 8) == _lib.PGPU_E_INVALID  # too small: refused, nothing enqueued
    _lib.check(lib.pgpu_table_fold(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                                   C.c_void_p(folded.data_ptr()), folded.numel() * 8))
    _lib.check(lib.pgpu_table_select(*args, nbytes))
    torch.cuda.synchronize()
    return S, out, out.cpu().numpy().reshape(NSEC + 1 + k, inner), folded.cpu().numpy().reshape(NSEC + 1, inner)


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


def _check_select(gpu_ctx, rng, t, inner, kind, ps=PS):
    want = _np_select(t, inner, ps)
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(rng, t)
    S, out, got, folded = _select_on_gpu(gpu_ctx, _table_layout(table.shape[1], kind), table, inner, ps)
    # the folded sections: pgpu_table_fold's output bit for bit, and numpy's
    assert np.array_equal(got[: NSEC + 1], folded) and np.array_equal(folded, want[: NSEC + 1])
    assert np.array_equal(got[NSEC + 1:], want[NSEC + 1:]), \
        [(p, int((got[NSEC + 1 + j] != want[NSEC + 1 + j]).sum())) for j, p in enumerate(ps)]
    return S, out, want


# a single cell; a wave boundary either side (a wave per key walks 64 cid a step); many chunks on the wave-per-key
# path with a tail; both lane orientations (inner below and from 64); lanes along g with cid chunks of one, of several
# and with tails ((2100, 1100): five cid per chunk), and with no chunking at all ((70001, 3))
SELECT_SHAPES = [(1, 1), (1, 63), (1, 65), (1, 70001), (3, 5), (64, 257), (257, 64), (5000, 33), (70001, 3),
                 (2100, 1100)]


@functools.lru_cache(maxsize=None)
def _shape_table(inner, card):
    """One table per shape, shared by the dense and the hash case (and left unchanged)."""
    rng = np.random.default_rng(inner * 1000003 + card)
    t = _fill(rng, _random_counts(rng, inner, card))
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card", SELECT_SHAPES, ids=[f"{i}x{c}" for i, c in SELECT_SHAPES])
def test_table_select_against_numpy(gpu_ctx, inner, card, kind):
    t = _shape_table(inner, card)
    S, out, want = _check_select(gpu_ctx, np.random.default_rng(card), t, inner, kind)
    if inner >= 3:  # the empty key holds 0 in every pick; the full key's first and last pick are the ends
        assert not want[NSEC + 1:, 0].any() and want[0, 0] == 0
        assert want[NSEC + 1, inner - 1] == 0 and want[NSEC + 1 + len(PS) - 1, inner - 1] == card - 1
    # compaction of the selected table: the non-empty keys in order, cells row-major
    live = np.flatnonzero(want[0] > 0)
    keys, cells = _compact(gpu_ctx, S, out)
    assert np.array_equal(keys, live) and np.array_equal(cells, want[:, live].T)
    # top 3 by the median's section (aggregation entry n + 1 + j, a LONG SUM), ties with the third kept
    j = PS.index(50.0)
    order = _lib.TopK()
    order.source, order.agg_fn, order.descending, order.k = _lib.PGPU_TOPK_AGG, _lib.PGPU_AGG_SUM, 1, 3
    order.agg_index = 4 + 1 + j
    assert S.agg_section[order.agg_index] == NSEC + 1 + j
    v = want[NSEC + 1 + j, live]
    keep = live if len(live) <= 3 else live[v >= np.sort(v)[-3]]
    keys, cells = _compact(gpu_ctx, S, out, order)
    by = np.argsort(keys)
    assert np.array_equal(keys[by], keep) and np.array_equal(cells[by], want[:, keep].T)


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card", [(2, 1000), (70, 300)], ids=["wave-per-key", "lanes-along-g"])
def test_table_select_one_cid_holds_the_whole_count(gpu_ctx, inner, card, kind):
    rng = np.random.default_rng(inner + card)
    counts = np.zeros(inner * card, dtype=np.int64)
    cid = rng.integers(0, card, inner)
    cid[0], cid[-1] = 0, card - 1
    counts[np.arange(inner) + inner * cid] = rng.integers(1, 1000, inner)
    _, _, want = _check_select(gpu_ctx, rng, _fill(rng, counts), inner, kind)
    assert np.array_equal(want[NSEC + 1:], np.tile(cid, (len(PS), 1)))  # every percentile is that one value


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner", [1, 64], ids=["wave-per-key", "lanes-along-g"])
def test_table_select_rank_at_a_chunk_boundary(gpu_ctx, inner, kind):
    """1,024 cid: a wave per key takes them in chunks of at least 256, lanes along g (64 keys) in chunks of one.  The
    running count is 491 after cid 255, 500 after cid 257 (256 is empty), 600 after 258, N = 1000: rank 490 is the
    last unit of cid 255 -- the last occupied cell of a chunk --, rank 491 the first unit of cid 257 -- the first
    occupied cell of the next --, rank 500 the first of cid 258."""
    card = 1024
    rng = np.random.default_rng(inner)
    c = np.zeros((card, inner), dtype=np.int64)
    c[100], c[255], c[257], c[258], c[1000] = 300, 191, 9, 100, 400
    ps = [49.0, 49.1, 50.0, 0.0, 100.0]
    _, _, want = _check_select(gpu_ctx, rng, _fill(rng, c.reshape(-1)), inner, kind, ps)
    assert want[NSEC + 1:, 0].tolist() == [255, 257, 258, 100, 1000]


def test_table_select_refuses_bad_percentiles(gpu_ctx):
    lib = gpu_ctx._lib
    L = _table_layout(6, PGPU_KEYS_DENSE)
    dev = torch.zeros(NSEC * 6, dtype=torch.int64, device="cuda")
    out = torch.zeros((NSEC + 1 + 8) * 3, dtype=torch.int64, device="cuda")
    for ps in ([-0.5], [100.5], [math.nan], [50.0, math.inf]):
        pp = (C.c_double * len(ps))(*ps)
        assert lib.pgpu_table_select(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, 3, pp, len(ps),
                                     C.c_void_p(out.data_ptr()), out.numel() * 8) == _lib.PGPU_E_INVALID
        assert "percentile" in _lib.last_error()
    pp = (C.c_double * 9)(*([50.0] * 9))
    for k in (0, 9):
        assert lib.pgpu_table_select(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, 3, pp, k,
                                     C.c_void_p(out.data_ptr()), out.numel() * 8) == _lib.PGPU_E_INVALID


# ---- 3. end to end on three segments whose dictionaries overlap only partly ---------------------------------------------
NDOCS = 20_000
C_COLUMNS = ["c_int", "c_long", "c_float", "c_double", "c_raw"]


def _columns(rng, i):
    """Segment i: the percentile columns' values come from [800 i, 800 i + 1400), so the three dictionaries overlap in
    part and the global one has about 3,000 entries.  `u` has 6,000 values (more groups than the server trim keeps)
    and `v` 50 whose spread depends on u, so that the percentiles of v differ from group to group."""
    c = rng.integers(800 * i, 800 * i + 1400, NDOCS).astype(np.int64)
    u = rng.integers(0, 6000, NDOCS).astype(np.int32)
    f = rng.integers(0, 100, NDOCS).astype(np.int32)
    return {"g": (PGPU_INT, rng.integers(0, 7, NDOCS).astype(np.int32) * 11 + 5), "f": (PGPU_INT, f),
            "f2": (PGPU_INT, (f == 0).astype(np.int32)),
            "x": (PGPU_INT, rng.integers(-50_000, 50_000, NDOCS).astype(np.int32)),
            "y": (PGPU_DOUBLE, np.round(rng.normal(0, 1000, NDOCS), 3)),
            "u": (PGPU_INT, u), "v": (PGPU_INT, (rng.integers(0, 1 << 30, NDOCS) % (1 + u % 50)).astype(np.int32) * 3),
            "c_int": (PGPU_INT, (c * 3 - 1000).astype(np.int32)), "c_long": (PGPU_LONG, c * (1 << 33) - 7),
            "c_float": (PGPU_FLOAT, (c.astype(np.float32) * np.float32(0.25)) - np.float32(100)),
            "c_double": (PGPU_DOUBLE, c.astype(np.float64) * 0.1 + 1.0),
            "c_str": (PGPU_STRING, [f"v{v:05d}" for v in c]), "c_raw": (PGPU_INT, (c * 5 + 1).astype(np.int32))}


@pytest.fixture(scope="module")
def three(gpu_ctx):
    rng = np.random.default_rng(20261020)
    cols = [_columns(rng, i) for i in range(3)]
    segs = [build_segment(f"p{i}", c, raw=["c_raw"]) for i, c in enumerate(cols)]
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    host = {k: np.concatenate([np.asarray(c[k][1]) for c in cols]) for k in cols[0] if k != "c_str"}
    yield gs, host
    for g in gs:
        g.release()


def _pct(values, p):
    """PercentileAggregationFunction.java:152-165 over the collected values."""
    if len(values) == 0:
        return -math.inf
    s = np.sort(values)
    return float(s[-1] if p == 100 else s[int(float(len(s)) * p / 100.0)])


def _pct_by(host, col, mask, by, p):
    return {int(k): _pct(host[col][mask & (host[by] == k)], p) for k in np.unique(host[by][mask])}


def _run(pm, q, gs):
    """submit + collect, returning the result and the layout of every pass's GROUP BY g, c launch."""
    pending = pm.submit(q, gs)
    layouts = [pq.layout for pq in pending.pending]
    return pm.collect(pending), layouts


MIX = "SUM(x), MIN(x), MAX(y), AVG(y), COUNT(*)"


@pytest.mark.parametrize("where", ["", " WHERE f < 30"], ids=["all", "filter"])
@pytest.mark.parametrize("grouped", [False, True], ids=["agg", "group"])
def test_end_to_end_mixed_aggregations(gpu_ctx, three, grouped, where):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30 if where else np.ones(len(host["f"]), dtype=bool)
    tail = " GROUP BY g LIMIT 100" if grouped else ""
    head = SEL + ("g, " if grouped else "")
    q = parse_sql(f"{head}SUM(x), PERCENTILE50(c_int), MIN(x), MAX(y), PERCENTILE(c_int, 99.9), AVG(y), COUNT(*), "
                  f"PERCENTILE(c_int, 0), PERCENTILE(c_int, '100') FROM t{where}{tail}")
    res, layouts = _run(pm, q, gs)
    assert len(layouts) == 1 and layouts[0].key_kind == PGPU_KEYS_DENSE  # one pass: 7 x ~3,000 keys
    plain = pm.execute(parse_sql(f"{head}{MIX} FROM t{where}{tail}"), gs)
    pcts = {1: 50, 4: 99.9, 7: 0, 8: 100}  # aggregation index -> percentile
    keep = [0, 2, 3, 5, 6]
    ng = int(grouped)
    if grouped:
        for ai, p in pcts.items():
            assert {r[0]: r[1 + ai] for r in res.group_rows} == _pct_by(host, "c_int", mask, "g", p)
        # the other columns are exactly those of the query without the percentiles
        assert [r[:1] + tuple(r[1 + i] for i in keep) for r in res.group_rows] == plain.group_rows
        assert [r[:1] + tuple(r[1 + i] for i in keep) for r in res.rows] == plain.rows
        assert all(type(r[1 + ai]) is float for r in res.group_rows for ai in pcts)
    else:
        for ai, p in pcts.items():
            assert res.aggregation_result[ai] == _pct(host["c_int"][mask], p)
            assert type(res.aggregation_result[ai]) is float
        assert [res.aggregation_result[i] for i in keep] == plain.aggregation_result
    st = res.stats
    assert st.num_docs_scanned == int(mask.sum()) == plain.stats.num_docs_scanned and st.num_total_docs == 3 * NDOCS
    assert st.num_entries_scanned_post_filter == st.num_docs_scanned * len(q.projected_columns)
    assert len(q.projected_columns) == 3 + ng
    assert st.num_entries_scanned_in_filter == plain.stats.num_entries_scanned_in_filter
    with pytest.raises(UnsupportedPlanError):
        res.intermediate


@pytest.mark.parametrize("col", C_COLUMNS)
def test_end_to_end_column_types(gpu_ctx, three, col):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30
    res = pm.execute(parse_sql(SEL + f"g, PERCENTILE90({col}), PERCENTILE({col}, 33.3), COUNT(*) FROM t WHERE f < 30 "
                               "GROUP BY g LIMIT 100"), gs)
    assert {r[0]: r[1] for r in res.group_rows} == _pct_by(host, col, mask, "g", 90)
    assert {r[0]: r[2] for r in res.group_rows} == _pct_by(host, col, mask, "g", 33.3)
    assert {r[0]: r[3] for r in res.group_rows} == {int(k): int((mask & (host["g"] == k)).sum())
                                                    for k in np.unique(host["g"])}
    res = pm.execute(parse_sql(SEL + f"PERCENTILE90({col}), PERCENTILE({col}, 33.3) FROM t"), gs)  # (never a non-scan plan)
    everything = np.ones(len(host[col]), dtype=bool)
    assert res.aggregation_result == [_pct(host[col][everything], 90), _pct(host[col][everything], 33.3)]
    assert res.stats.num_entries_scanned_post_filter == res.stats.num_docs_scanned == 3 * NDOCS


def test_string_column_raises_before_any_launch(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    with pytest.raises(UnsupportedPlanError, match="STRING"):
        pm.submit(parse_sql(SEL + "PERCENTILE50(c_str) FROM t"), gs)
    with pytest.raises(UnsupportedPlanError, match="STRING"):
        pm.execute(parse_sql(SEL + "g, SUM(x), PERCENTILE50(c_str) FROM t GROUP BY g"), gs)


def test_distinctcount_beside_percentiles_and_two_columns(gpu_ctx, three):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    tail = " FROM t WHERE f < 60 GROUP BY g LIMIT 100"
    both, layouts = _run(pm, parse_sql(SEL + "g, PERCENTILE50(c_int), DISTINCTCOUNT(c_int), PERCENTILE90(c_long), "
                                       "PERCENTILE99(c_int)" + tail), gs)
    assert len(layouts) == 2  # c_int (two picks and the distinct count in one table), c_long
    dc = pm.execute(parse_sql(SEL + "g, DISTINCTCOUNT(c_int)" + tail), gs)
    pc = pm.execute(parse_sql(SEL + "g, PERCENTILE50(c_int), PERCENTILE99(c_int)" + tail), gs)
    pl = pm.execute(parse_sql(SEL + "g, PERCENTILE90(c_long)" + tail), gs)
    assert [(r[0], r[2]) for r in both.group_rows] == dc.group_rows
    assert [(r[0], r[1], r[4]) for r in both.group_rows] == pc.group_rows
    assert [(r[0], r[3]) for r in both.group_rows] == pl.group_rows
    mask = host["f"] < 60
    assert {r[0]: r[1] for r in both.group_rows} == _pct_by(host, "c_int", mask, "g", 50)
    assert {r[0]: r[2] for r in both.group_rows} == {int(k): len(np.unique(host["c_int"][mask & (host["g"] == k)]))
                                                     for k in np.unique(host["g"])}
    assert {r[0]: r[3] for r in both.group_rows} == _pct_by(host, "c_long", mask, "g", 90)
    assert {r[0]: r[4] for r in both.group_rows} == _pct_by(host, "c_int", mask, "g", 99)
    assert both.stats.num_entries_scanned_post_filter == both.stats.num_docs_scanned * 3  # c_int, c_long, g


def test_filter_matching_nothing(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    for where in ("f = 0 AND f2 = 0", "f > 1000"):  # empty at run time / folded to EMPTY at plan time
        res = pm.execute(parse_sql(SEL + f"PERCENTILE50(c_int) FROM t WHERE {where}"), gs)
        assert res.aggregation_result == [-math.inf] and res.stats.num_docs_scanned == 0
        res = pm.execute(parse_sql(SEL + f"COUNT(*), PERCENTILE50(c_int), PERCENTILE(c_double, 100) FROM t WHERE {where}"), gs)
        assert res.aggregation_result == [0, -math.inf, -math.inf]
        res = pm.execute(parse_sql(SEL + f"g, PERCENTILE50(c_int), SUM(x) FROM t WHERE {where} GROUP BY g"), gs)
        assert res.rows == [] and res.group_rows == []


def test_forced_hash_path(gpu_ctx, three):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx, query_flags=PGPU_Q_HASH)
    q = parse_sql(SEL + "g, PERCENTILE50(c_int), SUM(x), PERCENTILE(c_int, 99.9) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    res, layouts = _run(pm, q, gs)
    assert layouts[0].key_kind == PGPU_KEYS_HASH
    mask = host["f"] < 30
    assert {r[0]: r[1] for r in res.group_rows} == _pct_by(host, "c_int", mask, "g", 50)
    assert {r[0]: r[3] for r in res.group_rows} == _pct_by(host, "c_int", mask, "g", 99.9)
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
    g = GpuSegment(gpu_ctx, build_segment("pwide", cols))
    yield g, {k: v[1] for k, v in cols.items()}
    g.release()


def test_partitioned_path(gpu_ctx, wide):
    g, host = wide
    res, layouts = _run(GpuPlanMaker(gpu_ctx), parse_sql(SEL + "PERCENTILE50(c), PERCENTILE(c, 99.9), PERCENTILE(c, 100) "
                                                         "FROM t WHERE f < 50"), [g])
    # 70,000 dense keys: from 65,536 keys up the group-by is partitioned; the pick runs a wave per chunk of cid
    assert layouts[0].key_kind == PGPU_KEYS_DENSE and layouts[0].num_keys == 70_000
    assert res.stats.kernel_variant == _lib.PGPU_KV_PSCAN
    vals = host["c"][host["f"] < 50]
    assert res.aggregation_result == [_pct(vals, 50), _pct(vals, 99.9), _pct(vals, 100)]


def test_hash_path_by_key_space(gpu_ctx, wide):
    g, host = wide
    res, layouts = _run(GpuPlanMaker(gpu_ctx), parse_sql(SEL + "g, PERCENTILE90(c), COUNT(*) FROM t WHERE f < 50 "
                                                         "GROUP BY g LIMIT 100"), [g])
    assert layouts[0].key_kind == PGPU_KEYS_HASH  # 40 x 70,000 keys against 200,000 docs
    assert {r[0]: r[1] for r in res.group_rows} == _pct_by(host, "c", host["f"] < 50, "g", 90)


# ---- 5. ORDER BY PERCENTILE ... LIMIT on more groups than the server trim keeps ---------------------------------------------
def test_order_by_percentile_trimmed_on_the_device(gpu_ctx, three):
    gs, host = three
    q = parse_sql(SEL + "u, PERCENTILE90(v), COUNT(*) FROM t WHERE f < 80 GROUP BY u ORDER BY PERCENTILE90(v) DESC, u "
                  "LIMIT 20")
    mask = host["f"] < 80
    p90 = _pct_by(host, "v", mask, "u", 90)
    cnt = {int(k): int((mask & (host["u"] == k)).sum()) for k in p90}
    full = sorted(((k, p90[k], cnt[k]) for k in p90), key=lambda r: (-r[1], r[0]))
    assert len(full) > 5000
    res = GpuPlanMaker(gpu_ctx).execute(q, gs)  # the default trim: max(5 * 20, 5000) groups, ties with the last kept
    assert res.rows == full[:20]
    assert 5000 <= len(res.group_rows) < len(full) and set(res.group_rows) <= set(full)
    kept = min(r[1] for r in res.group_rows)
    assert all(r in set(res.group_rows) for r in full if r[1] >= kept)  # nothing at or above the cut is missing
    # ascending too, and with the trim off every group comes back
    q2 = parse_sql(SEL + "u, PERCENTILE90(v), COUNT(*) FROM t WHERE f < 80 GROUP BY u ORDER BY PERCENTILE90(v), u LIMIT 20")
    assert GpuPlanMaker(gpu_ctx).execute(q2, gs).rows == sorted(full, key=lambda r: (r[1], r[0]))[:20]
    res = GpuPlanMaker(gpu_ctx, min_server_group_trim_size=-1).execute(q, gs)
    assert res.rows == full[:20] and sorted(res.group_rows, key=lambda r: (-r[1], r[0])) == full


# ---- 6. cancel ----------------------------------------------------------------------------------------------------------------
def test_cancelled_pass_is_not_selected_and_the_context_stays_usable(gpu_ctx, three):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + "g, PERCENTILE50(c_int), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    full = pm.collect(pm.submit(q, gs))
    # at the C ABI: pgpu_query_collect_select passes the wait's status through and releases the query
    pending = pm.submit(q, gs)
    pending.cancel()
    (pq,) = pending.pending
    inner, S = pq.fold.inner_keys, pq.fold.layout
    assert pq.fold.percentiles == [50.0] and S.num_sections == pq.layout.num_sections + 2
    keys = (C.c_int64 * inner)()
    cells = (C.c_int64 * (inner * S.num_sections))()
    n = C.c_uint64()
    st = _lib.QueryStats()
    h, pq.handle = pq.handle, None
    pp = (C.c_double * 1)(50.0)
    rc = gpu_ctx._lib.pgpu_query_collect_select(h, inner, pp, 1, None, keys, cells, inner, C.byref(n), C.byref(st), None)
    assert rc == _lib.PGPU_E_CANCELLED and "cancel" in _lib.last_error()
    # the Python surface raises
    pending = pm.submit(q, gs)
    pending.cancel()
    with pytest.raises(_lib.QueryCancelledError):
        pm.collect(pending)
    again = pm.collect(pm.submit(q, gs))
    assert again.group_rows == full.group_rows and again.stats.num_docs_scanned == full.stats.num_docs_scanned
    assert {r[0]: r[1] for r in again.group_rows} == _pct_by(host, "c_int", host["f"] < 30, "g", 50)
