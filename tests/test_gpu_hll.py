"""HyperLogLog sketches on the GPU (MI355X only): DISTINCTCOUNTHLL / DISTINCTCOUNTRAWHLL.
pgpu_table_hll on hand-made tables against hll.sketch_of_lut in numpy -- bit for bit, there is no tolerance on the device
side -- then GpuPlanMaker end to end against hll.sketch_of over the host columns, execute against execute_mergeable,
two servers through DataTables against one, and the contract of pgpu_query_collect_hll."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.segment_writer import build_segment
from pinot_amd import _lib, hll
from pinot_amd._lib import PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_Q_HASH, PGPU_STRING, UnsupportedPlanError
from pinot_amd.datatable import DataTable, reduce_data_tables, server_data_table
from pinot_amd.plan import GpuPlanMaker
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuSegment
from tests.test_gpu_percentile import NSEC, _fill, _random_counts, _table_layout, _to_hash
from tests.test_gpu_value_runs import RUN_SHAPES

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEL = "SELECT "  # (the oracle's SQL parser is held against every SELECT literal of the test files: see test_gpu_percentile)
GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A

# ---- 1. pgpu_table_hll alone -------------------------------------------------------------------------------------------
# RUN_SHAPES for the reasons given there (the wave and the thread orientation, their boundaries, several workgroups of
# keys, chunks with a tail); 400 x 20 at log2m 8 is 68,800 B of registers: past the LDS switch, on HBM atomics; 2 x 40 at
# log2m 16 likewise with the widest row
HLL_SHAPES = [(i, c, m) for i, c in RUN_SHAPES for m in (4, 8, 12)] + [(400, 20, 8), (2, 40, 16)]


@functools.lru_cache(maxsize=None)
def _shape(inner, card):
    rng = np.random.default_rng(inner * 1000003 + card)
    t = _fill(rng, _random_counts(rng, inner, card))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _values(card):
    """The dictionary behind the cid axis of the hand-made tables: distinct LONGs on both sides of 2^32."""
    rng = np.random.default_rng(card)
    return np.unique(rng.integers(-(1 << 40), 1 << 40, 2 * card + 8))[:card]


def _expected_words(t, inner, lut, log2m):
    """[inner][W]: per key the sketch of the LUT entries of its occupied cid, in numpy."""
    occ = np.asarray(t[0]).reshape(-1, inner) > 0  # [cid][g]
    n = min(occ.shape[0], len(lut))
    return np.stack([hll.sketch_of_lut(lut[:n][occ[:n, g]], log2m).words for g in range(inner)])


def _hll_on_gpu(gpu_ctx, L, table, inner, lut, log2m, num_values=None):
    """pgpu_table_hll into guard-filled outputs: (folded table [NSEC + 1][inner], registers [inner][W]) on the host,
    after the guards behind both were checked; the fold of the same device table beside it."""
    lib = gpu_ctx._lib
    W = hll.num_words(log2m)
    dev = torch.from_numpy(np.array(table).reshape(-1)).cuda()
    dlut = torch.from_numpy(np.asarray(lut, dtype=np.uint32).view(np.int32).copy()).cuda()
    nf = (NSEC + 1) * inner
    out = torch.full((nf + 8,), GUARD64, dtype=torch.int64, device="cuda")
    regs = torch.full((inner * W + 8,), GUARD32, dtype=torch.int32, device="cuda")
    _lib.check(lib.pgpu_table_hll(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                                  C.cast(dlut.data_ptr(), C.POINTER(C.c_uint32)),
                                  len(lut) if num_values is None else num_values, log2m, C.c_void_p(out.data_ptr()),
                                  nf * 8, C.c_void_p(regs.data_ptr())))
    folded = torch.zeros(nf, dtype=torch.int64, device="cuda")
    _lib.check(lib.pgpu_table_fold(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                                   C.c_void_p(folded.data_ptr()), nf * 8))
    torch.cuda.synchronize()
    o, r = out.cpu().numpy(), regs.cpu().numpy().view(np.uint32)
    assert (o[nf:] == GUARD64).all() and (r[inner * W:] == GUARD32).all()
    assert np.array_equal(o[:nf], folded.cpu().numpy())  # the folded table is pgpu_table_fold's
    return o[:nf].reshape(NSEC + 1, inner), r[: inner * W].reshape(inner, W)


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card,log2m", HLL_SHAPES, ids=[f"{i}x{c}-m{m}" for i, c, m in HLL_SHAPES])
def test_table_hll_against_numpy(gpu_ctx, inner, card, log2m, kind):
    t = _shape(inner, card)
    lut = hll.lut(_values(card), _lib.PGPU_LONG, log2m)
    want = _expected_words(t, inner, lut, log2m)
    assert want.any()
    if inner >= 3:  # the empty key keeps W zero words
        assert not want[0].any()
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(np.random.default_rng(card), t)
    folded, regs = _hll_on_gpu(gpu_ctx, _table_layout(table.shape[1], kind), table, inner, lut, log2m)
    assert np.array_equal(regs, want)
    assert np.array_equal(folded[NSEC], (np.asarray(t[0]).reshape(-1, inner) > 0).sum(axis=0))
    if (inner, card, log2m) in ((400, 20, 8), (2, 40, 16)):
        assert inner * hll.num_words(log2m) * 4 > 64 * 1024


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card", [(1, 3000), (3, 300), (300, 70)])
def test_table_hll_crafted_luts(gpu_ctx, inner, card, kind):
    """Register 7 offered by the first and the last cid (different chunks of the dense kernels) with different ranks,
    the larger first in one LUT and last in the other; then every cid in one register, with ranks cycling 1..24."""
    t = np.array(_shape(inner, card))
    t[0, :inner] = 5  # every key meets cid 0 and the last cid
    t[0, -inner:] = 5
    t[0, inner: 2 * inner] = 0  # ... and no key cid 1
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(np.random.default_rng(card), t)
    L = _table_layout(table.shape[1], kind)
    base = hll.lut(_values(card), _lib.PGPU_LONG, 8)
    base = np.where((base & 0xFFFF) == 7, base + 1, base).astype(np.uint32)  # no other cid in register 7
    for first, last in ((19, 3), (3, 19)):
        lut = base.copy()
        lut[0], lut[-1] = 7 | first << 16, 7 | last << 16
        lut[1] = 7 | 25 << 16  # (the unoccupied cid: never offered)
        want = _expected_words(t, inner, lut, 8)
        assert all(hll.HyperLogLog(8, w).registers()[7] == 19 for w in want)
        _, regs = _hll_on_gpu(gpu_ctx, L, table, inner, lut, 8)
        assert np.array_equal(regs, want)
    one = (200 | ((np.arange(card) % 24 + 1) << 16)).astype(np.uint32)
    want = _expected_words(t, inner, one, 8)
    _, regs = _hll_on_gpu(gpu_ctx, L, table, inner, one, 8)
    assert np.array_equal(regs, want)
    assert all(np.count_nonzero(hll.HyperLogLog(8, w).registers()) <= 1 for w in regs)


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
def test_table_hll_reads_no_lut_entry_past_num_values(gpu_ctx, kind):
    """A cid >= num_values offers nothing; an entry that names no register of the sketch, or no 5-bit rank, is skipped."""
    inner, card = 3, 300
    t = _shape(inner, card)
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(np.random.default_rng(card), t)
    L = _table_layout(table.shape[1], kind)
    lut = hll.lut(_values(card), _lib.PGPU_LONG, 8)
    _, regs = _hll_on_gpu(gpu_ctx, L, table, inner, lut, 8, num_values=100)
    assert np.array_equal(regs, _expected_words(t, inner, lut[:100], 8))
    bad = lut.copy()
    bad[::3] = 256 | 4 << 16  # register 256 of 256
    bad[1::3] = 9 | 32 << 16  # rank 32
    _, regs = _hll_on_gpu(gpu_ctx, L, table, inner, bad, 8)
    keep = np.arange(card) % 3 == 2
    occ = np.asarray(t[0]).reshape(-1, inner) > 0
    want = np.stack([hll.sketch_of_lut(lut[keep & occ[:, g]], 8).words for g in range(inner)])
    assert np.array_equal(regs, want)


def test_table_hll_argument_errors(gpu_ctx):
    lib = gpu_ctx._lib
    dev = torch.zeros(NSEC * 6 + 16, dtype=torch.int64, device="cuda")
    out = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p, o = C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr())
    lut_t = torch.zeros(16, dtype=torch.int32, device="cuda")
    lp = C.cast(lut_t.data_ptr(), C.POINTER(C.c_uint32))

    def call(L, inner, log2m=8, lut=lp, nv=2, dst=o, nbytes=4096 * 8, regs=o):
        return lib.pgpu_table_hll(gpu_ctx.handle, C.byref(L), p, None, inner, lut, nv, log2m, dst, nbytes, regs)

    L = _table_layout(6, PGPU_KEYS_DENSE)
    assert lib.pgpu_hll_words(3) == 0 == lib.pgpu_hll_words(17)
    assert [lib.pgpu_hll_words(m) for m in (4, 8, 12, 16)] == [3, 43, 683, 10923]
    assert call(L, 3, log2m=3) == _lib.PGPU_E_INVALID and "log2m" in _lib.last_error()
    assert call(L, 3, log2m=17) == _lib.PGPU_E_INVALID
    assert call(L, 0) == _lib.PGPU_E_INVALID
    assert call(L, 4) == _lib.PGPU_E_INVALID  # 6 keys are no multiple of 4
    assert call(L, 3, dst=None) == _lib.PGPU_E_INVALID
    assert call(L, 3, regs=None) == _lib.PGPU_E_INVALID
    assert call(L, 3, lut=None) == _lib.PGPU_E_INVALID
    assert call(L, 3, nv=0) == _lib.PGPU_E_INVALID
    assert call(L, 3, nbytes=(NSEC + 1) * 3 * 8 - 1) == _lib.PGPU_E_INVALID
    H = _table_layout(64, PGPU_KEYS_HASH)
    H.key_words = 2
    assert call(H, 3) == _lib.PGPU_E_UNSUPPORTED
    # the byte cap: 24,576 keys x 10,923 words x 4 B at log2m 16 are just past 1 GiB; 2^26 keys at log2m 8 far past it
    big = _table_layout(2 * 24576, PGPU_KEYS_DENSE)
    assert 24575 * 10923 * 4 <= _lib.PGPU_HLL_MAX_BYTES < 24576 * 10923 * 4
    assert call(big, 24576, log2m=16) == _lib.PGPU_E_UNSUPPORTED and "bytes" in _lib.last_error()
    assert call(_table_layout(2 << 26, PGPU_KEYS_DENSE), 1 << 26) == _lib.PGPU_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any().item()  # nothing was enqueued


# ---- 2. end to end through GpuPlanMaker --------------------------------------------------------------------------------
from tests.test_gpu_distinct import C_COLUMNS, _columns  # noqa: E402
from tests.test_gpu_value_runs import STATS, _host  # noqa: E402


@pytest.fixture(scope="module")
def three(gpu_ctx):
    """Three 20,000-doc segments whose dictionaries overlap only partly (test_gpu_distinct.py's)."""
    rng = np.random.default_rng(20260119)
    cols = [_columns(rng, i) for i in range(3)]
    gs = [GpuSegment(gpu_ctx, build_segment(f"h{i}", c, raw=["c_raw"])) for i, c in enumerate(cols)]
    hosts = [{k: np.asarray(c[k][1]) for k in c} for c in cols]
    yield gs, hosts
    for g in gs:
        g.release()


def _want(host, col, mask, log2m=8):
    """The sketch the reference builds of the column's values over the masked docs."""
    return hll.sketch_of(np.unique(host[col][mask]), C_COLUMNS.get(col, PGPU_INT), log2m)


def _final(a, sk):
    return sk.to_bytes().hex() if a.function == "DISTINCTCOUNTRAWHLL" else sk.cardinality()


def _check(pm, q, gs, host, mask):
    """execute and execute_mergeable against numpy: every sketch bit for bit, the finals from it, the plain aggregations
    and the statistics as the same query without the sketch functions gives them."""
    res, mer = pm.execute(q, gs), pm.execute_mergeable(q, gs)
    assert res.rows == mer.rows and res.group_rows == mer.group_rows
    assert res.aggregation_result == mer.aggregation_result
    for f in STATS:
        assert getattr(res.stats, f) == getattr(mer.stats, f), f
    inter = mer.intermediate
    groups = [(int(k),) for k in np.unique(host["g"][mask])] if q.group_by else [()]
    assert sorted(inter) == groups
    finals = {tuple(r[: len(q.group_by)]): r[len(q.group_by):] for r in res.group_rows} if q.group_by else \
        {(): res.aggregation_result}
    for key in groups:
        m = mask & (host["g"] == key[0]) if key else mask
        for a, got, fin in zip(q.aggregations, inter[key], finals[key]):
            if a.function in ("DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL"):
                want = _want(host, a.column, m, a.log2m)
                assert type(got) is hll.HyperLogLog and got == want  # bit for bit
                assert fin == _final(a, want) and type(fin) is (str if a.function.endswith("RAWHLL") else int)
            elif a.function == "DISTINCTCOUNT":
                assert fin == len(np.unique(host[a.column][m]))
            elif a.function == "SUM":
                assert fin == float(host[a.column][m].astype(np.int64).sum())
            elif a.function == "COUNT":
                assert fin == int(m.sum())
    return res


@pytest.mark.parametrize("col", list(C_COLUMNS))
def test_hll_column_types(gpu_ctx, three, col):
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30
    _check(pm, parse_sql(SEL + f"g, DISTINCTCOUNTHLL({col}), COUNT(*) FROM t WHERE f < 30 GROUP BY g LIMIT 100"), gs, host, mask)
    _check(pm, parse_sql(SEL + f"DISTINCTCOUNTHLL({col}, 12) FROM t WHERE f < 30"), gs, host, mask)


@pytest.mark.parametrize("flags", [0, PGPU_Q_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("where", ["", " WHERE f < 30"], ids=["all", "filter"])
@pytest.mark.parametrize("grouped", [False, True], ids=["agg", "group"])
def test_hll_with_rawhll_exact_and_plain_aggregations(gpu_ctx, three, grouped, where, flags):
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx, query_flags=flags)
    mask = host["f"] < 30 if where else np.ones(len(host["f"]), dtype=bool)
    # (grouped: SUM(x) keeps the all-docs query from the non-scan plan, which has a test of its own)
    q = parse_sql(SEL + ("g, " if grouped else "") + "DISTINCTCOUNTHLL(c_int), DISTINCTCOUNTRAWHLL(c_int), SUM(x), "
                  "DISTINCTCOUNT(c_int), DISTINCTCOUNTHLL(c_str, 12), COUNT(*) FROM t" + where +
                  (" GROUP BY g LIMIT 100" if grouped else ""))
    pending = pm.submit(q, gs)
    assert [(p.column, bool(p.sketch)) for p in pending.passes] == [("c_int", False), ("c_int", True), ("c_str", True)]
    kinds = [pq.layout.key_kind for pq in pending.pending]
    pm.collect(pending)
    if grouped:
        assert kinds == [PGPU_KEYS_HASH if flags else PGPU_KEYS_DENSE] * 3
    res = _check(pm, q, gs, host, mask)
    # the exact count is today's answer, and the estimate is within the reference's bound of it (20 % at log2m 8)
    exact = pm.execute(parse_sql(SEL + ("g, " if grouped else "") + "DISTINCTCOUNT(c_int) FROM t" + where +
                                 (" GROUP BY g LIMIT 100" if grouped else "")), gs)
    rows = res.group_rows if grouped else [tuple(res.aggregation_result)]
    ng = int(grouped)
    assert [r[ng + 3] for r in rows] == [r[ng] for r in (exact.group_rows if grouped else [tuple(exact.aggregation_result)])]
    for r in rows:
        print(f"exact {r[ng + 3]} estimated {r[ng]}")
        assert abs(r[ng] - r[ng + 3]) <= 0.20 * r[ng + 3]


def test_hll_order_by_the_estimate_and_by_a_plain_aggregation(gpu_ctx, three):
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30
    est = {int(k): _want(host, "a", mask & (host["w"] == k)).cardinality() for k in np.unique(host["w"][mask])}
    q = parse_sql(SEL + "w, DISTINCTCOUNTHLL(a) FROM t WHERE f < 30 GROUP BY w ORDER BY DISTINCTCOUNTHLL(a) DESC, w LIMIT 5")
    want = sorted(est.items(), key=lambda kv: (-kv[1], kv[0]))[:5]
    assert pm.execute(q, gs).rows == want == pm.execute_mergeable(q, gs).rows
    q = parse_sql(SEL + "w, DISTINCTCOUNTHLL(a), COUNT(*) FROM t WHERE f < 30 GROUP BY w ORDER BY COUNT(*) DESC, w LIMIT 5")
    cnt = {int(k): int((mask & (host["w"] == k)).sum()) for k in est}
    want = [(k, est[k], c) for k, c in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))[:5]]
    assert pm.execute(q, gs).rows == want


def test_hll_non_scan_segments_offer_their_dictionaries(gpu_ctx, three):
    """An aggregation-only query whose filter folds to match-all offers the dictionary on the host: segment 2 holds only
    c_int >= 3800, segment 0 nothing of it, segment 1 some."""
    gs, hosts = three
    host = _host(hosts)
    pm = GpuPlanMaker(gpu_ctx)
    for where, mask in ((" WHERE c_int >= 3800", host["c_int"] >= 3800), ("", np.ones(len(host["f"]), dtype=bool))):
        q = parse_sql(SEL + "DISTINCTCOUNTHLL(c_int), COUNT(*), DISTINCTCOUNTRAWHLL(c_str, 12) FROM t" + where)
        assert any(pm.non_scan_segments(q, gs))
        want = [_want(host, "c_int", mask), _want(host, "c_str", mask, 12)]
        for res in (pm.execute(q, gs), pm.execute_mergeable(q, gs)):
            assert res.rows == [(want[0].cardinality(), int(mask.sum()), want[1].to_bytes().hex())]
            assert res.intermediate[()][0] == want[0] and res.intermediate[()][2] == want[1]
            assert res.stats.num_docs_scanned == int(mask.sum())


def test_hll_refused_cases(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    for sql in ("g, DISTINCTCOUNTHLL(g) FROM t GROUP BY g", "DISTINCTCOUNTHLL(c_int), SUM(x) FILTER(WHERE f < 3) FROM t",
                "DISTINCTCOUNTHLL(c_int, 3) FROM t", "DISTINCTCOUNTHLL(c_int, 17) FROM t",
                "DISTINCTCOUNTHLL(c_int, 8), DISTINCTCOUNTRAWHLL(c_int, 9) FROM t"):
        for run in (pm.execute, pm.execute_mergeable):
            with pytest.raises(UnsupportedPlanError):
                run(parse_sql(SEL + sql), gs)


# ---- 3. two servers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sql", [
    "g, DISTINCTCOUNTHLL(c_int), SUM(x), COUNT(*) FROM t WHERE f < 30 GROUP BY g ORDER BY DISTINCTCOUNTHLL(c_int) DESC, g LIMIT 5",
    "DISTINCTCOUNTHLL(c_str, 12), DISTINCTCOUNTRAWHLL(c_float), DISTINCTCOUNT(c_long), COUNT(*) FROM t WHERE f < 30",
    "DISTINCTCOUNTHLL(c_int) FROM t"], ids=["order-by-estimate", "aggregation", "non-scan"])
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
def _raw_collect(gpu_ctx, pq, cap):
    F, W = pq.fold.layout, hll.num_words(pq.fold.log2m)
    keys, cells = np.full(max(cap, 1), -1, dtype=np.int64), np.full((max(cap, 1), F.num_sections), -1, dtype=np.int64)
    words = np.full((max(cap, 1), W), 77, dtype=np.uint32)
    n, st = C.c_uint64(), _lib.QueryStats()
    lut = pq.fold.lut
    rc = gpu_ctx._lib.pgpu_query_collect_hll(
        pq.handle, pq.fold.inner_keys, lut.ctypes.data_as(C.POINTER(C.c_uint32)), len(lut), pq.fold.log2m,
        keys.ctypes.data_as(C.POINTER(C.c_int64)), cells.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n),
        words.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st), None)
    return rc, n.value, keys, cells, words


@pytest.mark.parametrize("flags", [0, PGPU_Q_HASH], ids=["dense", "hash"])
def test_collect_hll_keeps_the_query_when_the_capacity_is_too_small(gpu_ctx, three, flags):
    gs, hosts = three
    host = _host(hosts)
    mask = host["f"] < 30
    pm = GpuPlanMaker(gpu_ctx, query_flags=flags)
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c_int), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    (pq,) = pm.submit(q, gs).pending
    rc, n, keys, cells, words = _raw_collect(gpu_ctx, pq, 6)
    assert rc == _lib.PGPU_E_INVALID and n == 7
    assert (keys == -1).all() and (cells == -1).all() and (words == 77).all()  # nothing written
    rc, n, keys, cells, words = _raw_collect(gpu_ctx, pq, 7)  # the same query, a second time
    pq.handle = None  # (released by the successful collect)
    assert rc == _lib.PGPU_OK and n == 7 and keys.tolist() == list(range(7))
    ks = np.unique(host["g"][mask])
    assert [hll.HyperLogLog(8, w) for w in words] == [_want(host, "c_int", mask & (host["g"] == k)) for k in ks]
    assert cells[:, -1].tolist() == [len(np.unique(host["c_int"][mask & (host["g"] == k)])) for k in ks]


def test_collect_hll_passes_a_cancelled_query_through(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c_int), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    full = pm.execute(q, gs)
    pending = pm.submit(q, gs)
    pending.cancel()
    (pq,) = pending.pending
    rc, *_ = _raw_collect(gpu_ctx, pq, 7)
    pq.handle = None  # released, as pgpu_query_collect_fold releases it
    assert rc == _lib.PGPU_E_CANCELLED and "cancel" in _lib.last_error()
    pending = pm.submit(q, gs)
    pending.cancel()
    with pytest.raises(_lib.QueryCancelledError):
        pm.collect(pending)
    assert pm.execute(q, gs).rows == full.rows


def test_collect_hll_argument_errors_release_the_query(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + "g, DISTINCTCOUNTHLL(c_int) FROM t GROUP BY g LIMIT 100")
    lib = gpu_ctx._lib
    (pq,) = pm.submit(q, gs).pending
    lut = pq.fold.lut.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = lib.pgpu_query_collect_hll(pq.handle, pq.fold.inner_keys, lut, len(pq.fold.lut), 8, None, None, 0, None, None,
                                    None, None)
    pq.handle = None  # released: only too small a capacity keeps the query
    assert rc == _lib.PGPU_E_INVALID and "null" in _lib.last_error()
    (pq,) = pm.submit(q, gs).pending
    n = C.c_uint64()
    rc = lib.pgpu_query_collect_hll(pq.handle, pq.fold.inner_keys, lut, len(pq.fold.lut), 17, None, None, 0, C.byref(n),
                                    None, None, None)
    pq.handle = None
    assert rc == _lib.PGPU_E_INVALID and "log2m" in _lib.last_error()
    assert len(pm.execute(q, gs).rows) == 7  # the context stays usable
