"""Prepared queries in the C ABI (pgpu_query_prepare / pgpu_prepared_submit): a query planned once and submitted many
times returns what pgpu_query_submit_ordered returns, re-plans exactly when a fresh plan could differ -- a per-plan
switch changed, a segment's presence rows became ready, a segment or remap buffer went away -- and never otherwise.

Shapes are the smallest at which each path exists: the three presence-row segments of tests/test_gpu_presence.py
(6,149 / 70,001 / 67,584 docs: a partial tile, 35 tiles, a row-word boundary), two candidate-path segments of
tests/test_gpu_cand.py, and three 20,000-doc random segments whose two group columns span a dense table past 8 MiB for
the eager trim.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import engine
from pinot_amd import _lib
from pinot_amd._lib import QueryStats
from pinot_amd.plan import GpuPlanMaker, PendingQuery, key_words_out
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuSegment
from tests.test_gpu_lead_planes import DAY, _sql
from tests.test_gpu_parity import _assert_same, _oracle, _random_segment
from tests.test_gpu_presence import AFTER, LEAD, SWITCH, T31, T32, _acct, _check_oracle, _segments

pytestmark = pytest.mark.gpu
CHUNK = "PGPU_PRESENCE_CHUNK_WORDS"
STAT_FIELDS = [n for n, _ in QueryStats._fields_ if n != "kernel_ms"]


# ---- the C ABI, called directly ---------------------------------------------------------------------------------
def _args(prep):
    _, expr, desc, _, _, _, order, _ = prep
    return (C.byref(desc), expr[0] if expr is not None else None, expr[1] if expr is not None else 0,
            C.byref(order) if order is not None else None)


def _prepare(ctx, prep):
    h = C.c_void_p()
    _lib.check(ctx._lib.pgpu_query_prepare(ctx.handle, *_args(prep), C.byref(h)))
    return h


def _counts(ctx, h):
    c = _lib.PreparedCounts()
    _lib.check(ctx._lib.pgpu_prepared_counts(h, C.byref(c)))
    return c.plans, c.hits, c.uncached


def _submit_plain(ctx, prep, nseg):
    h = C.c_void_p()
    _lib.check(ctx._lib.pgpu_query_submit_ordered(ctx.handle, *_args(prep), C.byref(h)))
    matched = np.full(max(1, nseg), 9, dtype=np.uint8)
    _lib.check(ctx._lib.pgpu_query_matched_segments(h, matched.ctypes.data_as(C.POINTER(C.c_uint8)), nseg))
    return h, matched


def _submit_prepared(ctx, ph, nseg, deadline_ms=0):
    h = C.c_void_p()
    matched = np.full(max(1, nseg), 9, dtype=np.uint8)
    _lib.check(ctx._lib.pgpu_prepared_submit(ph, deadline_ms, matched.ctypes.data_as(C.POINTER(C.c_uint8)), nseg,
                                             C.byref(h)))
    return h, matched


def _collect_raw(ctx, prep, sub):
    """(status, keys, cells, stats without kernel_ms, matched flags): rows in key order (a hash table's slot order
    is not fixed from run to run)."""
    h, matched = sub
    L, order = prep[5], prep[6]
    cap, kw = int(min(L.num_keys, 1 << 26)), key_words_out(L)
    keys = np.zeros(max(cap, 1) * kw, dtype=np.int64)
    cells = np.zeros((max(cap, 1), L.num_sections), dtype=np.int64)
    n, st = C.c_uint64(), QueryStats()
    rc = ctx._lib.pgpu_query_collect_topk(h, C.byref(order) if order is not None else None,
                                          keys.ctypes.data_as(C.POINTER(C.c_int64)),
                                          cells.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n), C.byref(st))
    k = keys[: n.value * kw].reshape(-1, kw)
    by_key = np.lexsort(k.T[::-1]) if len(k) else np.arange(0)
    return (rc, k[by_key].tolist(), cells[: n.value][by_key].tolist(), tuple(getattr(st, f) for f in STAT_FIELDS),
            matched.tolist())


def _collect_result(pm, prep, nseg, sub):
    """The same handle finished by GpuPlanMaker.collect: a QueryResult to hold against the oracle."""
    pq = PendingQuery(pm, prep[0], nseg, sub[0], prep[5], prep[4])
    pq.order, pq.matched = prep[6], sub[1]
    return pm.collect(pq)


def _knobs(monkeypatch, after="-1", switch="0", lead="0"):
    monkeypatch.setenv(AFTER, after)
    monkeypatch.setenv(SWITCH, switch)
    monkeypatch.setenv(LEAD, lead)


@pytest.fixture(scope="module")
def presence_segs(gpu_ctx):
    segs, _ = _segments()
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    yield segs, gs
    for g in gs:
        g.release()


@pytest.fixture(scope="module")
def cand_segs(gpu_ctx):
    from tests.test_gpu_cand import _segments as cand_segments
    segs = cand_segments(nseg=2)
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    yield segs, gs
    for g in gs:
        g.release()


@pytest.fixture(scope="module")
def wide_segs(gpu_ctx):
    rng = np.random.default_rng(909)
    segs = [_random_segment(rng, 20_000 + 17 * i, f"wide{i}") for i in range(3)]
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    yield segs, gs
    for g in gs:
        g.release()


POINT = [DAY, _acct(T32)]
CAND_SQL = "SELECT g, SUM(m), COUNT(*), AVG(x) FROM t WHERE a IN (77, 1234) AND d > 3 GROUP BY g"
SHAPES = {
    # name: (segments fixture, sql, GpuPlanMaker options, oracle options)
    "fused_agg": ("presence", _sql(POINT, "agg"), dict(collect_stats=True), {}),
    "fused_lds": ("presence", _sql([DAY], "lds"), dict(collect_stats=True), {}),
    "split_exact_filter_stats": ("presence", _sql(POINT, "agg"), dict(exact_filter_stats=True), {}),
    "cand_inverted_lead": ("cand", CAND_SQL, {}, {}),
    "hash_groupby": ("cand", CAND_SQL, dict(query_flags=_lib.PGPU_Q_HASH), {}),
    # 47,994 x 7 keys in 8 sections: a dense table of 21 MB (past the 8 MiB a submit exports whole), trimmed to 5,000
    "eager_ordered_trim": ("wide", "SELECT d, a, COUNT(*), SUM(m), MIN(m), MAX(m), SUM(c), MAX(c), MIN(f), SUM(f) "
                                   "FROM t WHERE g > 5 GROUP BY d, a ORDER BY SUM(m) DESC LIMIT 10",
                           dict(num_groups_limit=5_000_000), dict(num_groups_limit=5_000_000)),
}


@pytest.fixture
def shape_segs(request, gpu_ctx):
    def get(kind):
        return request.getfixturevalue(f"{kind}_segs")
    return get


# ---- 1, 2: same answers, counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_same_answers_as_the_plain_path(gpu_ctx, shape_segs, monkeypatch, shape):
    kind, sql, opts, ref_opts = SHAPES[shape]
    segs, gs = shape_segs(kind)
    _knobs(monkeypatch)
    q = parse_sql(sql)
    pm = GpuPlanMaker(gpu_ctx, **opts)
    prep = pm._prepare(q, gs)
    L, order = prep[5], prep[6]
    if shape == "hash_groupby":
        assert L.key_kind == _lib.PGPU_KEYS_HASH
    if shape == "eager_ordered_trim":
        assert order is not None and L.num_keys > order.k and _lib.table_bytes(L) > (8 << 20)
        assert L.key_kind == _lib.PGPU_KEYS_DENSE
    plain = _collect_raw(gpu_ctx, prep, _submit_plain(gpu_ctx, prep, len(gs)))
    assert plain[0] == 0
    if shape.startswith("cand"):
        assert plain[3][STAT_FIELDS.index("kernel_variant")] == _lib.PGPU_KV_CAND
    if shape == "split_exact_filter_stats":
        assert plain[3][STAT_FIELDS.index("filter_stats_exact")] == 1
    ph = _prepare(gpu_ctx, prep)
    try:
        inflight = [_submit_prepared(gpu_ctx, ph, len(gs)) for _ in range(3)]
        for sub in inflight:
            assert _collect_raw(gpu_ctx, prep, sub) == plain
        # a settled shape: planned once, by the prepare; the first submit takes that plan, the other two reuse it
        assert _counts(gpu_ctx, ph) == (1, 2, 0)
        res = _collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs)))
    finally:
        gpu_ctx._lib.pgpu_prepared_release(ph)
    ref = _oracle(q, segs, **ref_opts)
    _assert_same(res, ref)
    assert res.stats.segment_matched.tolist() == plain[4][: len(gs)]
    print(f"{shape}: variant {res.stats.kernel_variant}, {len(plain[1])} rows, matched {plain[4]}")


# ---- 3: switches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,values", [(LEAD, ("0", "-1")), (CHUNK, ("64", "1"))])
def test_a_changed_switch_plans_again(gpu_ctx, presence_segs, monkeypatch, knob, values):
    segs, gs = presence_segs
    _knobs(monkeypatch, after="0" if knob == CHUNK else "-1")
    monkeypatch.setenv(knob, values[0])
    q = parse_sql(_sql(POINT, "agg"))
    pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
    prep = pm._prepare(q, gs)
    ref = engine.execute(q, segs)
    ph = _prepare(gpu_ctx, prep)
    try:
        # (with PGPU_PRESENCE_AFTER=0 on segments sealed without rows the first plans ask for them: run until the
        # plan is settled, as test_built_on_use does)
        for _ in range(200):
            before = _counts(gpu_ctx, ph)
            first = _collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs)))
            if _counts(gpu_ctx, ph)[1] > before[1]:
                break
        _check_oracle(first, ref, q)
        settled = _counts(gpu_ctx, ph)
        same = _collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs)))
        assert _counts(gpu_ctx, ph) == (settled[0], settled[1] + 1, settled[2])   # unchanged switches: no re-plan
        monkeypatch.setenv(knob, values[1])
        changed = _collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs)))
        assert _counts(gpu_ctx, ph) == (settled[0] + 1, settled[1] + 1, settled[2])
        again = _collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs)))
        assert _counts(gpu_ctx, ph) == (settled[0] + 1, settled[1] + 2, settled[2])
    finally:
        gpu_ctx._lib.pgpu_prepared_release(ph)
    for r in (same, changed, again):
        _check_oracle(r, ref, q)
        assert r.group_rows == first.group_rows and r.aggregation_result == first.aggregation_result
    # the change is seen: the plain path under the new switch reports the same figures
    plain = GpuPlanMaker(gpu_ctx, collect_stats=True).execute(q, gs)
    assert (changed.stats.num_entries_scanned_in_filter, changed.stats.dense_bytes) == \
           (plain.stats.num_entries_scanned_in_filter, plain.stats.dense_bytes)


# ---- 4: presence rows through a prepared handle -------------------------------------------------------------------
def test_presence_rows_through_a_prepared_handle(gpu_ctx, monkeypatch):
    """Two identical sets of fresh segments, PGPU_PRESENCE_AFTER=2: the plain path on one, one prepared handle on the
    other.  Submit by submit the same dense_bytes and the same moment at which the rows' bytes are reserved (the build
    starts at the second collect); the handle's first submits are uncached, and hits only start once the skip is in
    the plan."""
    import torch
    segs, _ = _segments()
    _knobs(monkeypatch, after="2")
    q = parse_sql(_sql(POINT, "agg"))
    pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
    runs = {}
    for path in ("plain", "prepared"):
        gs = [GpuSegment(gpu_ctx, s) for s in segs]
        ph = None
        try:
            prep = pm._prepare(q, gs)
            base = gpu_ctx.derived_bytes()[0]
            if path == "prepared":
                ph = _prepare(gpu_ctx, prep)
            trace = []
            for i in range(7):
                sub = _submit_prepared(gpu_ctx, ph, len(gs)) if ph else _submit_plain(gpu_ctx, prep, len(gs))
                res = _collect_result(pm, prep, len(gs), sub)
                if i == 1:
                    torch.cuda.synchronize()   # (the builds the second collect started are done: the third submit skips)
                trace.append((res.stats.dense_bytes, gpu_ctx.derived_bytes()[0] - base,
                              _counts(gpu_ctx, ph) if ph else None, tuple(res.aggregation_result)))
            runs[path] = trace
        finally:
            if ph:
                gpu_ctx._lib.pgpu_prepared_release(ph)
            for g in gs:
                g.release()
    plain, prepared = runs["plain"], runs["prepared"]
    print("plain   ", [(t[0], t[1]) for t in plain])
    print("prepared", [(t[0], t[1], t[2]) for t in prepared])
    assert [t[0] for t in prepared] == [t[0] for t in plain]      # dense_bytes, submit by submit
    assert [t[1] for t in prepared] == [t[1] for t in plain]      # bytes reserved for rows, collect by collect
    assert [t[3] for t in prepared] == [t[3] for t in plain]
    full, skipping = plain[0][0], plain[-1][0]
    assert plain[0][1] == 0 and plain[1][1] > 0                   # the build starts at the second collect
    assert plain[1][0] == full and skipping < full and plain[2][0] == skipping
    counts = [t[2] for t in prepared]
    assert counts[0] == (1, 0, 1) and counts[1] == (2, 0, 2)      # uncached, not skipping
    assert counts[2][1] == 0                                      # the first skipping submit planned for itself
    assert counts[-1][1] >= 2 and counts[-1][2] == 2              # ... and from then on the plan is reused
    for before, after, t in zip(counts, counts[1:], prepared[1:]):
        if after[1] > before[1]:
            assert t[0] == skipping


def test_a_declined_model_settles_at_once(gpu_ctx, monkeypatch):
    """A two-id IN on the 1,024-value column: its rows would keep every tile, the model declines, nothing is asked
    of any segment -- the prepare's plan is kept from the first submit on."""
    segs, _ = _segments()
    _knobs(monkeypatch, after="2")
    q = parse_sql(_sql([DAY, ("s10", "in", [3 * 5, 3 * 900])], "agg"))
    ref = engine.execute(q, segs)
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    try:
        pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
        prep = pm._prepare(q, gs)
        base = gpu_ctx.derived_bytes()[0]
        ph = _prepare(gpu_ctx, prep)
        try:
            for _ in range(3):
                _check_oracle(_collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs))), ref, q)
            assert _counts(gpu_ctx, ph) == (1, 2, 0)
        finally:
            gpu_ctx._lib.pgpu_prepared_release(ph)
        assert gpu_ctx.derived_bytes()[0] == base
    finally:
        for g in gs:
            g.release()


# ---- 5: invalidation ------------------------------------------------------------------------------------------------
def test_set_derived_and_buffer_release_plan_again(gpu_ctx, presence_segs, monkeypatch):
    segs, gs = presence_segs
    _knobs(monkeypatch)
    q = parse_sql(_sql(POINT, "global"))
    ref = engine.execute(q, segs)
    pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
    prep = pm._prepare(q, gs)
    lib = gpu_ctx._lib
    ph = _prepare(gpu_ctx, prep)
    try:
        for _ in range(2):
            _check_oracle(_collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs))), ref, q)
        assert _counts(gpu_ctx, ph) == (1, 1, 0)
        # (refused on a sealed segment; the call alone says that the segment's derived copies are being touched)
        assert lib.pgpu_segment_set_derived(gs[1].handle, 0, _lib.PGPU_DERIVE_ALL) == _lib.PGPU_E_INVALID
        _check_oracle(_collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs))), ref, q)
        assert _counts(gpu_ctx, ph) == (2, 1, 0)
        # a remap buffer beside the query's own is released: any plan may have named it
        table = np.arange(16, dtype=np.int32)
        buf = C.c_void_p()
        _lib.check(lib.pgpu_remap_upload(gpu_ctx.handle, table.ctypes.data_as(C.POINTER(C.c_int32)), 16, C.byref(buf)))
        _check_oracle(_collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs))), ref, q)
        assert _counts(gpu_ctx, ph) == (2, 2, 0)
        _lib.check(lib.pgpu_buffer_release(buf))
        _check_oracle(_collect_result(pm, prep, len(gs), _submit_prepared(gpu_ctx, ph, len(gs))), ref, q)
        assert _counts(gpu_ctx, ph) == (3, 2, 0)
    finally:
        lib.pgpu_prepared_release(ph)


def test_released_segment_drops_the_native_handles(gpu_ctx, monkeypatch):
    _knobs(monkeypatch)
    rng = np.random.default_rng(31)
    segs = [_random_segment(rng, 4_096 + 5 * i, f"drop{i}") for i in range(3)]
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    lib = gpu_ctx._lib
    try:
        q = parse_sql("SELECT b, COUNT(*), SUM(m) FROM t WHERE c < 1500 GROUP BY b")
        live0 = lib.pgpu_prepared_live()
        pm = GpuPlanMaker(gpu_ctx)
        assert lib.pgpu_prepared_live() == live0
        ref = _oracle(q, segs)
        for _ in range(3):
            _assert_same(pm.collect(pm.submit(q, gs)), ref)
        assert len(pm._prepared) == 1 and lib.pgpu_prepared_live() == live0 + 1
        native = next(iter(pm._prepared.values()))[-1]
        c = native.counts()
        assert (c.plans, c.hits, c.uncached) == (1, 2, 0)
        del native, c
        gs[2].release()
        assert not pm._prepared and lib.pgpu_prepared_live() == live0
        _assert_same(pm.collect(pm.submit(q, gs[:2])), _oracle(q, segs[:2]))
        assert lib.pgpu_prepared_live() == live0 + 1
        pm._prepared.clear()
        assert lib.pgpu_prepared_live() == live0
    finally:
        for g in gs:
            g.release()


# ---- 6: deadline per submit -------------------------------------------------------------------------------------------
def test_deadline_is_per_submit(gpu_ctx, presence_segs, monkeypatch):
    segs, gs = presence_segs
    _knobs(monkeypatch)
    q = parse_sql(_sql(POINT, "agg"))
    pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
    prep = pm._prepare(q, gs)
    want = _collect_raw(gpu_ctx, prep, _submit_plain(gpu_ctx, prep, len(gs)))
    prep[2].deadline_ms = 1   # 1 ms past the epoch
    late_plain = _collect_raw(gpu_ctx, prep, _submit_plain(gpu_ctx, prep, len(gs)))
    prep[2].deadline_ms = 0
    assert late_plain[0] == _lib.PGPU_E_TIMEOUT
    ph = _prepare(gpu_ctx, prep)
    try:
        late = _collect_raw(gpu_ctx, prep, _submit_prepared(gpu_ctx, ph, len(gs), deadline_ms=1))
        assert late[0] == _lib.PGPU_E_TIMEOUT and "deadline" in _lib.last_error()
        assert _collect_raw(gpu_ctx, prep, _submit_prepared(gpu_ctx, ph, len(gs), deadline_ms=0)) == want
        assert _counts(gpu_ctx, ph) == (1, 1, 0)
    finally:
        gpu_ctx._lib.pgpu_prepared_release(ph)


# ---- 7: two threads ---------------------------------------------------------------------------------------------------
def test_two_threads_on_one_handle(gpu_ctx, presence_segs, monkeypatch):
    """50 submits + collects from each of two threads on one handle; between their halves, while both wait at a
    barrier, the main thread changes a switch.  Every result is the single-threaded one."""
    segs, gs = presence_segs
    _knobs(monkeypatch)
    q = parse_sql(_sql(POINT, "global"))
    pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
    prep = pm._prepare(q, gs)

    def answer(raw):   # (the two plans read different entries and bytes, maybe through different kernels)
        return (raw[0], raw[1], raw[2], raw[4])

    want = _collect_raw(gpu_ctx, prep, _submit_plain(gpu_ctx, prep, len(gs)))
    monkeypatch.setenv(LEAD, "-1")
    want_off = _collect_raw(gpu_ctx, prep, _submit_plain(gpu_ctx, prep, len(gs)))
    monkeypatch.setenv(LEAD, "0")
    assert answer(want) == answer(want_off)
    ph = _prepare(gpu_ctx, prep)
    barrier = threading.Barrier(3)
    got, errors = {0: [], 1: []}, []

    def worker(k):
        try:
            for half in range(2):
                for _ in range(25):
                    got[k].append(_collect_raw(gpu_ctx, prep, _submit_prepared(gpu_ctx, ph, len(gs))))
                if half == 0:
                    barrier.wait(timeout=60)
                    barrier.wait(timeout=60)
        except Exception as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(k,)) for k in (0, 1)]
    try:
        for t in threads:
            t.start()
        barrier.wait(timeout=60)
        monkeypatch.setenv(LEAD, "-1")
        barrier.wait(timeout=60)
        for t in threads:
            t.join(timeout=120)
        assert not errors, errors
        for k in (0, 1):
            assert len(got[k]) == 50
            assert all(r == want for r in got[k][:25]) and all(r == want_off for r in got[k][25:])
        plans, hits, uncached = _counts(gpu_ctx, ph)
        assert uncached == 0 and plans + hits >= 100 and 2 <= plans <= 3   # (both threads may meet the change at once)
    finally:
        gpu_ctx._lib.pgpu_prepared_release(ph)


# ---- 8: release while in flight ---------------------------------------------------------------------------------------
def test_release_while_in_flight(gpu_ctx, wide_segs, monkeypatch):
    segs, gs = wide_segs
    _knobs(monkeypatch)
    _, sql, opts, _ = SHAPES["eager_ordered_trim"]
    pm = GpuPlanMaker(gpu_ctx, **opts)
    prep = pm._prepare(parse_sql(sql), gs)
    want = _collect_raw(gpu_ctx, prep, _submit_plain(gpu_ctx, prep, len(gs)))
    ph = _prepare(gpu_ctx, prep)
    subs = [_submit_prepared(gpu_ctx, ph, len(gs)) for _ in range(2)]
    assert gpu_ctx._lib.pgpu_prepared_release(ph) == 0
    for sub in subs:
        assert _collect_raw(gpu_ctx, prep, sub) == want


# ---- 9: errors ----------------------------------------------------------------------------------------------------------
def _both_refuse(gpu_ctx, call_plain, call_prepare):
    rc_plain = call_plain()
    msg_plain = _lib.last_error()
    sentinel = C.c_void_p(0xBAD0)
    rc = call_prepare(C.byref(sentinel))
    assert rc != 0 and (rc, _lib.last_error()) == (rc_plain, msg_plain)
    assert sentinel.value == 0xBAD0
    return rc, msg_plain


def test_errors_are_the_plain_path_s(gpu_ctx, presence_segs, monkeypatch):
    segs, gs = presence_segs
    _knobs(monkeypatch)
    lib = gpu_ctx._lib
    q = parse_sql(_sql(POINT, "agg"))
    pm = GpuPlanMaker(gpu_ctx)
    prep = pm._prepare(q, gs)
    desc, expr, order = prep[2], prep[1], prep[6]
    assert expr is not None
    o = C.byref(order) if order is not None else None
    out = C.c_void_p()
    # an unsupported plan: an aggregation function the descriptor does not know
    fn0 = desc.aggs[1].fn
    desc.aggs[1].fn = 9
    try:
        rc, msg = _both_refuse(
            gpu_ctx, lambda: lib.pgpu_query_submit_ordered(gpu_ctx.handle, C.byref(desc), expr[0], expr[1], o, C.byref(out)),
            lambda h: lib.pgpu_query_prepare(gpu_ctx.handle, C.byref(desc), expr[0], expr[1], o, h))
    finally:
        desc.aggs[1].fn = fn0
    assert rc == _lib.PGPU_E_UNSUPPORTED, (rc, msg)
    # null arguments
    rc, msg = _both_refuse(gpu_ctx, lambda: lib.pgpu_query_submit_ordered(None, C.byref(desc), expr[0], expr[1], o, C.byref(out)),
                           lambda h: lib.pgpu_query_prepare(None, C.byref(desc), expr[0], expr[1], o, h))
    assert rc == _lib.PGPU_E_INVALID and msg == "null argument"
    rc, msg = _both_refuse(gpu_ctx, lambda: lib.pgpu_query_submit_ordered(gpu_ctx.handle, None, expr[0], expr[1], o, C.byref(out)),
                           lambda h: lib.pgpu_query_prepare(gpu_ctx.handle, None, expr[0], expr[1], o, h))
    assert rc == _lib.PGPU_E_INVALID and msg == "null argument"
    assert lib.pgpu_query_prepare(gpu_ctx.handle, C.byref(desc), expr[0], expr[1], o, None) == _lib.PGPU_E_INVALID
    # an expression with a trailing node (the last node of a prefix-order program is a leaf: once more)
    n = expr[1]
    longer = (_lib.ExprNode * (n + 1))()
    for i in range(n):
        longer[i] = expr[0][i]
    longer[n] = expr[0][n - 1]
    rc, msg = _both_refuse(gpu_ctx, lambda: lib.pgpu_query_submit_ordered(gpu_ctx.handle, C.byref(desc), longer, n + 1, o, C.byref(out)),
                           lambda h: lib.pgpu_query_prepare(gpu_ctx.handle, C.byref(desc), longer, n + 1, o, h))
    assert rc == _lib.PGPU_E_INVALID and "1 trailing nodes" in msg
    # a matched-segments buffer of another length
    ph = _prepare(gpu_ctx, prep)
    try:
        matched = np.zeros(8, dtype=np.uint8)
        h = C.c_void_p()
        rc = lib.pgpu_prepared_submit(ph, 0, matched.ctypes.data_as(C.POINTER(C.c_uint8)), len(gs) + 1, C.byref(h))
        assert rc == _lib.PGPU_E_INVALID and not h.value
        assert f"{len(gs) + 1} entries for a {len(gs)}-segment query" in _lib.last_error()
        assert lib.pgpu_prepared_submit(None, 0, None, 0, C.byref(h)) == _lib.PGPU_E_INVALID
        assert _counts(gpu_ctx, ph) == (1, 0, 0)
    finally:
        lib.pgpu_prepared_release(ph)
