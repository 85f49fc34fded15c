"""Value runs on the GPU (MI355X only): the mergeable intermediates of DISTINCTCOUNT, PERCENTILE and MODE.
pgpu_table_runs on hand-made tables against numpy, execute_mergeable end to end against numpy over the host columns and
against execute, two servers through DataTables against one, and the contract of pgpu_query_collect_runs."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.segment_writer import build_segment
from pinot_amd import _lib
from pinot_amd._lib import PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_Q_HASH, PGPU_STRING, UnsupportedPlanError
from pinot_amd.datatable import DataTable, reduce_data_tables, server_data_table
from pinot_amd.plan import GpuPlanMaker
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuSegment
from tests.test_gpu_percentile import NSEC, _fill, _random_counts, _table_layout, _to_hash

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEL = "SELECT "  # (the oracle's SQL parser is held against every SELECT literal of the test files: see test_gpu_percentile)
GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A

# ---- 1. pgpu_table_runs alone ------------------------------------------------------------------------------------------
# inner = 1: a wave per key -- one cid, a wave boundary either side, one chunk of 256, two, many with a tail; inner = 3:
# the empty and the full key on that path; 63 / 64 / 65: where the orientation turns to a thread per (g, chunk); 300:
# more than one workgroup of keys; 4095 / 4097: where the chunk prefix goes from a wave to a thread
RUN_SHAPES = ([(1, c) for c in (1, 63, 64, 65, 256, 257, 3000)] + [(3, 300)] + [(i, 70) for i in (63, 64, 65, 300)] +
              [(i, 5) for i in (4095, 4097)])


@functools.lru_cache(maxsize=None)
def _shape(inner, card):
    """(table [NSEC][inner * card], offsets, cids, counts in numpy) of a shape, shared by its cases and left unchanged."""
    rng = np.random.default_rng(inner * 1000003 + card)
    t = _fill(rng, _random_counts(rng, inner, card))
    t.setflags(write=False)
    c = t[0].reshape(card, inner)  # cell = g + inner * cid
    g, cid = np.nonzero(c.T > 0)  # rows of c.T are g: the (g, cid) pairs by g, cid ascending within it
    offsets = np.concatenate([[0], np.cumsum((c > 0).sum(axis=0))]).astype(np.uint64)
    return t, offsets, cid.astype(np.uint32), c.T[g, cid].astype(np.int64)


def _runs_on_gpu(gpu_ctx, L, table, inner, cap):
    """pgpu_table_runs into guard-filled arrays of `cap` + 8 elements: (offsets, cids, counts) on the host."""
    dev = torch.from_numpy(np.array(table).reshape(-1)).cuda()
    off = torch.full((inner + 1 + 8,), GUARD64, dtype=torch.int64, device="cuda")
    cids = torch.full((cap + 8,), GUARD32, dtype=torch.int32, device="cuda")
    cnts = torch.full((cap + 8,), GUARD64, dtype=torch.int64, device="cuda")
    _lib.check(gpu_ctx._lib.pgpu_table_runs(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                                            C.c_void_p(off.data_ptr()), C.c_void_p(cids.data_ptr()),
                                            C.c_void_p(cnts.data_ptr()), cap))
    torch.cuda.synchronize()
    return dev, off.cpu().numpy().view(np.uint64), cids.cpu().numpy().view(np.uint32), cnts.cpu().numpy()


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card", RUN_SHAPES, ids=[f"{i}x{c}" for i, c in RUN_SHAPES])
def test_table_runs_against_numpy(gpu_ctx, inner, card, kind):
    t, offsets, cids, counts = _shape(inner, card)
    total = int(offsets[-1])
    assert total == len(cids) > 0
    if inner >= 3:  # the empty and the full key
        assert offsets[1] == 0 and offsets[inner] - offsets[inner - 1] == card
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(np.random.default_rng(card), t)
    L = _table_layout(table.shape[1], kind)
    dev, off, gc, gn = _runs_on_gpu(gpu_ctx, L, table, inner, total)
    assert np.array_equal(off[: inner + 1], offsets) and (off[inner + 1:] == GUARD64).all()
    assert np.array_equal(gc[:total], cids) and (gc[total:] == GUARD32).all()
    assert np.array_equal(gn[:total], counts) and (gn[total:] == GUARD64).all()
    # the offset differences are the fold's distinct section of the same device table
    folded = torch.zeros((NSEC + 1) * inner, dtype=torch.int64, device="cuda")
    _lib.check(gpu_ctx._lib.pgpu_table_fold(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                                            C.c_void_p(folded.data_ptr()), folded.numel() * 8))
    torch.cuda.synchronize()
    assert np.array_equal(folded.cpu().numpy().reshape(NSEC + 1, inner)[NSEC], np.diff(offsets).astype(np.int64))
    # one element short: offsets complete, the elements below the capacity as before, nothing at or beyond it
    _, off, gc, gn = _runs_on_gpu(gpu_ctx, L, table, inner, total - 1)
    assert np.array_equal(off[: inner + 1], offsets) and (off[inner + 1:] == GUARD64).all()
    assert np.array_equal(gc[: total - 1], cids[:-1]) and (gc[total - 1:] == GUARD32).all()
    assert np.array_equal(gn[: total - 1], counts[:-1]) and (gn[total - 1:] == GUARD64).all()


def test_table_runs_argument_errors(gpu_ctx):
    lib = gpu_ctx._lib
    dev = torch.zeros(NSEC * 6 + 16, dtype=torch.int64, device="cuda")
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, o = C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr())

    def call(L, inner, off=o, cids=o, counts=o):
        return lib.pgpu_table_runs(gpu_ctx.handle, C.byref(L), p, None, inner, off, cids, counts, 4)

    L = _table_layout(6, PGPU_KEYS_DENSE)
    assert call(L, 0) == _lib.PGPU_E_INVALID
    assert call(L, 4) == _lib.PGPU_E_INVALID  # 6 keys are no multiple of 4
    for null in ("off", "cids", "counts"):
        assert call(L, 3, **{null: None}) == _lib.PGPU_E_INVALID
    H = _table_layout(64, PGPU_KEYS_HASH)
    H.key_words = 2
    assert call(H, 3) == _lib.PGPU_E_UNSUPPORTED
    big = _table_layout(2 * ((1 << 26) + 1), PGPU_KEYS_DENSE)
    assert call(big, (1 << 26) + 1) == _lib.PGPU_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any().item()  # nothing was enqueued


# ---- 2. execute_mergeable end to end -----------------------------------------------------------------------------------
from tests.test_gpu_distinct import C_COLUMNS, _columns  # noqa: E402


@pytest.fixture(scope="module")
def three(gpu_ctx):
    """Three 20,000-doc segments whose dictionaries overlap only partly (test_gpu_distinct.py's)."""
    rng = np.random.default_rng(20260119)
    cols = [_columns(rng, i) for i in range(3)]
    gs = [GpuSegment(gpu_ctx, build_segment(f"r{i}", c, raw=["c_raw"])) for i, c in enumerate(cols)]
    hosts = [{k: np.asarray(c[k][1]) for k in c} for c in cols]
    yield gs, hosts
    for g in gs:
        g.release()


def _host(hosts, which=(0, 1, 2)):
    return {k: np.concatenate([hosts[i][k] for i in which]) for k in hosts[0]}


def _runs_of(host, col, mask):
    """numpy: (ascending distinct values, their counts) of `col` over the masked docs, as Python lists."""
    v, c = np.unique(host[col][mask], return_counts=True)
    return v.tolist(), c.tolist()


STATS = ("num_docs_scanned", "num_entries_scanned_in_filter", "num_entries_scanned_post_filter", "num_total_docs",
         "num_segments_processed", "num_segments_matched")


def _check_mergeable(pm, q, gs, host, mask):
    """execute_mergeable against numpy (the intermediates) and against execute (rows, statistics)."""
    from pinot_amd.distinct import ValueList, ValueMap, ValueSet
    res, ref = pm.execute_mergeable(q, gs), pm.execute(q, gs)
    assert res.rows == ref.rows and res.group_rows == ref.group_rows
    assert res.aggregation_result == ref.aggregation_result
    assert [type(v) for v in res.rows[0]] == [type(v) for v in ref.rows[0]]
    for f in STATS:
        assert getattr(res.stats, f) == getattr(ref.stats, f), f
    with pytest.raises(UnsupportedPlanError):
        ref.intermediate  # execute's own result still has none
    inter = res.intermediate
    groups = [(int(k),) for k in np.unique(host["g"][mask])] if q.group_by else [()]
    assert sorted(inter) == groups
    for key in groups:
        m = mask & (host["g"] == key[0]) if key else mask
        for a, got in zip(q.aggregations, inter[key]):
            if a.function == "DISTINCTCOUNT":
                assert type(got) is ValueSet and got.values == _runs_of(host, a.column, m)[0]
                assert got.stored_type == C_COLUMNS[a.column]
            elif a.function == "PERCENTILE":
                v, c = _runs_of(host, a.column, m)
                assert type(got) is ValueList and (got.values, got.counts) == ([float(x) for x in v], c)
            elif a.function == "MODE":
                assert type(got) is ValueMap and (got.values, got.counts) == _runs_of(host, a.column, m)
            elif a.function == "SUM":
                assert got == float(host[a.column][m].astype(np.int64).sum())
            elif a.function == "COUNT":
                assert got == int(m.sum())
    return res


@pytest.mark.parametrize("col", list(C_COLUMNS))
def test_mergeable_column_types(gpu_ctx, three, col):
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30
    more = "" if C_COLUMNS[col] == PGPU_STRING else f", PERCENTILE({col}, 50), MODE({col})"
    _check_mergeable(pm, parse_sql(SEL + f"g, DISTINCTCOUNT({col}){more}, COUNT(*) FROM t WHERE f < 30 GROUP BY g LIMIT 100"),
                     gs, host, mask)
    _check_mergeable(pm, parse_sql(SEL + f"DISTINCTCOUNT({col}){more} FROM t WHERE f < 30"), gs, host, mask)


@pytest.mark.parametrize("flags", [0, PGPU_Q_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("where", ["", " WHERE f < 30"], ids=["all", "filter"])
@pytest.mark.parametrize("grouped", [False, True], ids=["agg", "group"])
def test_mergeable_every_function_of_one_column(gpu_ctx, three, grouped, where, flags):
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx, query_flags=flags)
    mask = host["f"] < 30 if where else np.ones(len(host["f"]), dtype=bool)
    q = parse_sql(SEL + ("g, " if grouped else "") + "DISTINCTCOUNT(c_int), PERCENTILE(c_int, 25), PERCENTILE90(c_int), "
                  "MODE(c_int, 'AVG'), SUM(x) FROM t" + where + (" GROUP BY g LIMIT 100" if grouped else ""))
    pending = pm.submit_mergeable(q, gs)
    kinds = [pq.layout.key_kind for pq in pending.pending]
    pm.collect_mergeable(pending)
    if grouped:
        assert kinds == [PGPU_KEYS_HASH if flags else PGPU_KEYS_DENSE]
    _check_mergeable(pm, q, gs, host, mask)


def test_mergeable_non_scan_segments_contribute_their_dictionaries(gpu_ctx, three):
    """An aggregation-only query whose filter folds to match-all is answered from the dictionary (execute does so
    too): segment 2 holds only c_int >= 3800, segment 0 nothing of it, segment 1 some."""
    from pinot_amd.distinct import ValueSet
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx)
    assert hosts[2]["c_int"].min() >= 3800 > hosts[0]["c_int"].max()
    for where, mask in ((" WHERE c_int >= 3800", host["c_int"] >= 3800), ("", np.ones(len(host["f"]), dtype=bool))):
        q = parse_sql(SEL + "DISTINCTCOUNT(c_int), COUNT(*) FROM t" + where)
        assert any(pm.non_scan_segments(q, gs))
        res, ref = pm.execute_mergeable(q, gs), pm.execute(q, gs)
        assert res.rows == ref.rows == [(len(np.unique(host["c_int"][mask])), int(mask.sum()))]
        for f in STATS:
            assert getattr(res.stats, f) == getattr(ref.stats, f), f
        got = res.intermediate[()]
        assert got[0] == ValueSet(_runs_of(host, "c_int", mask)[0], PGPU_INT) and got[1] == int(mask.sum())


def test_refused_cases_stay_refused(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    for sql in ("g, DISTINCTCOUNT(g) FROM t GROUP BY g", "DISTINCTCOUNT(c_int), SUM(x) FILTER(WHERE f < 3) FROM t",
                "PERCENTILE(c_str, 50) FROM t"):
        with pytest.raises(UnsupportedPlanError):
            pm.execute_mergeable(parse_sql(SEL + sql), gs)
    plain = parse_sql(SEL + "g, SUM(x) FROM t GROUP BY g LIMIT 100")  # a query without folded functions: execute
    assert pm.execute_mergeable(plain, gs).rows == pm.execute(plain, gs).rows


# ---- 3. two servers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sql", [
    "g, DISTINCTCOUNT(c_int), SUM(x), COUNT(*) FROM t WHERE f < 30 GROUP BY g ORDER BY DISTINCTCOUNT(c_int) DESC, g LIMIT 5",
    "g, PERCENTILE(c_double, 50), PERCENTILE99(c_double), MODE(c_int), MODE(c_int, 'MAX'), MODE(c_int, 'AVG') FROM t "
    "GROUP BY g ORDER BY g LIMIT 100",
    "DISTINCTCOUNT(c_str), DISTINCTCOUNT(c_float), PERCENTILE(c_long, 75), MODE(c_raw, 'AVG'), COUNT(*) FROM t WHERE f < 30",
    "DISTINCTCOUNT(c_int) FROM t"], ids=["order-by-distinct", "percentile-mode", "aggregation", "non-scan"])
def test_two_servers_reduce_to_one(gpu_ctx, three, sql):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + sql)
    types = [PGPU_INT] * len(q.group_by)
    wire = [server_data_table(q, pm.execute_mergeable(q, part), types).to_bytes() for part in (gs[:2], gs[2:])]
    got = reduce_data_tables(q, [DataTable.from_bytes(b) for b in wire])
    ref = pm.execute(q, gs)
    assert got.rows == ref.rows and [type(v) for v in got.rows[0]] == [type(v) for v in ref.rows[0]]
    assert got.num_docs_scanned == ref.stats.num_docs_scanned and got.total_docs == ref.stats.num_total_docs
    # each server alone answers differently: the merge did the work
    assert reduce_data_tables(q, [DataTable.from_bytes(wire[0])]).rows != ref.rows


# ---- 4. the collect's contract -----------------------------------------------------------------------------------------
def _raw_collect(gpu_ctx, pq, cap, rcap):
    F = _lib.folded_layout_of(pq.layout, pq.fold.inner_keys, 0, 0)
    keys, cells = np.full(cap, -1, dtype=np.int64), np.full((cap, F.num_sections), -1, dtype=np.int64)
    off, cids, cnts = np.full(cap + 1, 77, dtype=np.uint64), np.full(max(rcap, 1), 77, dtype=np.uint32), \
        np.full(max(rcap, 1), 77, dtype=np.int64)
    n, nr, st = C.c_uint64(), C.c_uint64(), _lib.QueryStats()
    rc = gpu_ctx._lib.pgpu_query_collect_runs(
        pq.handle, pq.fold.inner_keys, keys.ctypes.data_as(C.POINTER(C.c_int64)),
        cells.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n), off.ctypes.data_as(C.POINTER(C.c_uint64)),
        cids.ctypes.data_as(C.POINTER(C.c_uint32)), cnts.ctypes.data_as(C.POINTER(C.c_int64)), rcap, C.byref(nr),
        C.byref(st), None)
    return rc, n.value, nr.value, keys, cells, off, cids, cnts


@pytest.mark.parametrize("flags", [0, PGPU_Q_HASH], ids=["dense", "hash"])
def test_collect_runs_keeps_the_query_when_a_buffer_is_too_small(gpu_ctx, three, flags):
    gs, hosts = three
    host = _host(hosts)
    mask = host["f"] < 30
    pm = GpuPlanMaker(gpu_ctx, query_flags=flags)
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c_int), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    (pq,) = pm.submit_mergeable(q, gs).pending
    want = [_runs_of(host, "c_int", mask & (host["g"] == k)) for k in np.unique(host["g"][mask])]
    total = sum(len(v) for v, _ in want)
    rc, n, nr, keys, cells, off, cids, cnts = _raw_collect(gpu_ctx, pq, 7, total - 1)
    assert rc == _lib.PGPU_E_INVALID and (n, nr) == (7, total)
    assert (keys == -1).all() and (cells == -1).all() and (cids == 77).all() and (cnts == 77).all()  # nothing written
    rc, n, nr, *_ = _raw_collect(gpu_ctx, pq, 6, total)  # too few rows: kept as well
    assert rc == _lib.PGPU_E_INVALID and (n, nr) == (7, total)
    rc, n, nr, keys, cells, off, cids, cnts = _raw_collect(gpu_ctx, pq, 7, total)  # the same query, a second time
    pq.handle = None  # (released by the successful collect)
    assert rc == _lib.PGPU_OK and (n, nr) == (7, total)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(v) for v, _ in want])]).tolist()
    gdict = np.unique(np.concatenate([h["c_int"] for h in hosts]))  # the global dictionary of c_int: cid -> value
    assert gdict[cids].tolist() == [x for v, _ in want for x in v]
    assert cnts.tolist() == [x for _, c in want for x in c]
    assert cells[:, -1].tolist() == [len(v) for v, _ in want]  # the distinct count is the number of runs


def test_collect_runs_passes_a_cancelled_query_through(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + "g, MODE(c_int), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    full = pm.execute_mergeable(q, gs)
    pending = pm.submit_mergeable(q, gs)
    pending.cancel()
    (pq,) = pending.pending
    rc, *_ = _raw_collect(gpu_ctx, pq, 7, 1 << 16)
    pq.handle = None  # released, as pgpu_query_collect_fold releases it
    assert rc == _lib.PGPU_E_CANCELLED and "cancel" in _lib.last_error()
    pending = pm.submit_mergeable(q, gs)
    pending.cancel()
    with pytest.raises(_lib.QueryCancelledError):
        pm.collect_mergeable(pending)
    again = pm.execute_mergeable(q, gs)
    assert again.rows == full.rows and again.intermediate == full.intermediate


def test_python_collect_retries_once_with_the_needed_count(gpu_ctx, three):
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx)
    pm.run_capacity = 16  # far fewer than the ~7 x 900 runs: the first call is refused, the second serves
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c_int), MODE(c_int) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    _check_mergeable(pm, q, gs, host, host["f"] < 30)


# ---- 5. a folded table past 8 MiB: rows compacted on the device ----------------------------------------------------------
def test_many_groups_take_the_device_compaction(gpu_ctx):
    """600,011 group keys: the folded table (count and distinct count, 9.6 MB) is compacted on the device, where up to
    8 MiB it comes back whole.  The filter keeps 30,000 docs, which meet multiples of 3 only; the docs it drops hold
    every key once, so that the dictionary of u has them all."""
    n, nu = 30_000, 600_011
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.integers(0, nu // 3, n) * 3, np.arange(nu)]).astype(np.int32)
    c = np.concatenate([rng.integers(0, 3, n), np.zeros(nu, dtype=np.int64)]).astype(np.int32)
    f = np.concatenate([np.zeros(n, dtype=np.int32), np.ones(nu, dtype=np.int32)])
    g = GpuSegment(gpu_ctx, build_segment("many", {"u": (PGPU_INT, u), "c": (PGPU_INT, c), "f": (PGPU_INT, f)}))
    try:
        pm = GpuPlanMaker(gpu_ctx, num_groups_limit=1 << 20)
        pm.run_capacity = 1000  # (and the retry on this path)
        q = parse_sql(SEL + "u, DISTINCTCOUNT(c), COUNT(*) FROM t WHERE f = 0 GROUP BY u ORDER BY u LIMIT 1000000")
        pending = pm.submit_mergeable(q, [g])
        (pq,) = pending.pending
        inner, L = pq.fold.inner_keys, pq.layout
        res = pm.collect_mergeable(pending)
        assert inner == nu and _lib.table_bytes(_lib.folded_layout_of(L, inner, 0, 0)) > (8 << 20)
        assert res.rows == pm.execute(q, [g]).rows
        pairs = np.unique(u[:n].astype(np.int64) * 3 + c[:n])
        keys, distinct = np.unique(pairs // 3, return_counts=True)
        assert [r[:2] for r in res.rows] == list(zip(keys.tolist(), distinct.tolist())) and len(keys) > 20_000
        inter = res.intermediate
        for k in keys[:50].tolist():
            m = u[:n] == k
            assert inter[(k,)][0].values == np.unique(c[:n][m]).tolist() and inter[(k,)][1] == int(m.sum())
    finally:
        g.release()


# ---- 6. the submit / collect pair on its own ---------------------------------------------------------------------------
@pytest.mark.parametrize("col", [c for c in C_COLUMNS if c != "c_int"])
def test_submit_collect_pair_names_the_wire_type_of_the_column(gpu_ctx, three, col):
    """submit_mergeable / collect_mergeable on a plan maker that has run nothing else: the sets and maps carry the
    column's stored type (LongSet, not IntSet, for a LONG column ...) and go through a DataTable's bytes."""
    from pinot_amd.distinct import ValueMap, ValueSet
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx)
    more = "" if C_COLUMNS[col] == PGPU_STRING else f", MODE({col}, 'MAX')"
    q = parse_sql(SEL + f"g, DISTINCTCOUNT({col}){more} FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    res = pm.collect_mergeable(pm.submit_mergeable(q, gs))
    mask = host["f"] < 30
    for (k,), inter in res.intermediate.items():
        v, c = _runs_of(host, col, mask & (host["g"] == k))
        assert inter[0] == ValueSet(v, C_COLUMNS[col])
        assert not more or inter[1] == ValueMap(v, c, C_COLUMNS[col])
    table = server_data_table(q, res, [PGPU_INT])
    back = DataTable.from_bytes(table.to_bytes())
    assert back.rows == table.rows and len(back.rows) == 7
    assert reduce_data_tables(q, [back]).rows == pm.execute(q, gs).rows


def test_collect_runs_without_a_place_for_the_counts_is_refused(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + "g, DISTINCTCOUNT(c_int) FROM t GROUP BY g LIMIT 100")
    (pq,) = pm.submit_mergeable(q, gs).pending
    n = C.c_uint64()
    rc = gpu_ctx._lib.pgpu_query_collect_runs(pq.handle, pq.fold.inner_keys, None, None, 0, C.byref(n), None, None, None,
                                              0, None, None, None)
    pq.handle = None  # released: only too small a buffer keeps the query
    assert rc == _lib.PGPU_E_INVALID and "null" in _lib.last_error()
    assert len(pm.execute_mergeable(q, gs).rows) == 7  # the context stays usable
