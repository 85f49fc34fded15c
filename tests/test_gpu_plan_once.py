"""One analysis per segment and submit, in reused scratch (pgpu_segplan.h, Packer::clear, PlanScratch in
pgpu_runtime.cpp): results on the GPU against the oracle where the plans of one query's segments differ, at and past
the inline capacity of the top-level AND, and across submits that reuse one thread's scratch or run on two threads.

Three segments of 3 * 2048 + 17 docs (the last tile is partial).  `acct` is 20 bits wide everywhere; segment 0's
dictionary ends below the literal ABSENT's id, so a filter on it folds to EMPTY there; segment 2 is loaded without
acct's bit-sliced copy, so it can take no lead leaf and is charged the prefix planes it loses (prefix_loss).
"""
import threading
from collections import deque

import numpy as np
import pytest

from oracle import engine
from oracle.segment_writer import bits_per_value, build_segment, dictionary_bytes, pack_fixed_bit
from pinot_amd._lib import PGPU_DERIVE_VALUE_PLANES, PGPU_INT
from pinot_amd.query import parse_sql
from pinot_amd.segment import ColumnIndexes
from tests.helpers import check_groups, close

N = 3 * 2048 + 17
NSEG = 3
DAY0 = 17000
DAY_LO, DAY_HI = DAY0 + 300, DAY0 + 307
KIDS_CAP = 8  # segplan::kKidsCap: the top-level AND's children held inline
NF = KIDS_CAP + 1
CARDS = ((1 << 19) + 100, (1 << 19) + 400, (1 << 19) + 400)   # 20 bits each
ABSENT = (1 << 19) + 250   # an id past segment 0's dictionary
COMMON = 4242
NINE = [COMMON, 11, 70_000, 140_001, 210_002, 280_003, 350_004, 420_005, 500_006]
KNOB = "PGPU_LEAD_SWITCH_BYTES"


def _segment(k, rng):
    day = (DAY0 + rng.permutation(np.arange(N) % 1024)).astype(np.int32)
    inside = (day >= DAY_LO) & (day <= DAY_HI)
    cols = {"day": (PGPU_INT, day), "clicks": (PGPU_INT, rng.integers(0, 1 << 20, N).astype(np.int32))}
    for j in range(NF):
        cols[f"f{j}"] = (PGPU_INT, rng.integers(0, 50, N).astype(np.int32))
    seg = build_segment(f"once{k}", cols, sorted_columns=())
    card = CARDS[k]
    ids = rng.integers(0, card, N)
    for lit in [ABSENT] + NINE:
        if lit >= card:
            continue
        ids[inside & (rng.random(N) < 0.15)] = lit
        ids[~inside & (rng.random(N) < 0.01)] = lit
    assert bits_per_value(card) == 20
    col = ColumnIndexes("acct", PGPU_INT, card, dictionary=dictionary_bytes(3 * np.arange(card), PGPU_INT))
    col.forward = pack_fixed_bit(ids, 20)
    seg.columns["acct"] = col
    return seg


@pytest.fixture(scope="module")
def segs():
    rng = np.random.default_rng(77)
    return [_segment(k, rng) for k in range(NSEG)]


@pytest.fixture(scope="module")
def gpu_segs(gpu_ctx, segs):
    from pinot_amd.segment import GpuSegment
    gs = [GpuSegment(gpu_ctx, s, derived={"acct": PGPU_DERIVE_VALUE_PLANES} if k == 2 else None)
          for k, s in enumerate(segs)]
    yield gs
    for g in gs:
        g.release()


def _day():
    return f"day BETWEEN {DAY_LO} AND {DAY_HI}"


def _acct(ids):
    return f"acct IN ({', '.join(str(3 * i) for i in ids)})"


GROUPED = "SELECT day, COUNT(*), SUM(clicks) FROM t WHERE {} AND {} GROUP BY day LIMIT 2000"
SQL_AND = GROUPED.format(_day(), _acct([COMMON]))
SQL_OR = "SELECT COUNT(*), SUM(clicks), MIN(clicks) FROM t WHERE {} OR {}".format(_day(), _acct(NINE))
SQL_ABSENT = GROUPED.format(_day(), _acct([ABSENT]))


def _sql_kids(n):
    where = " AND ".join(f"f{j} < {45 - j}" for j in range(n))
    return "SELECT COUNT(*), SUM(clicks), MAX(clicks) FROM t WHERE {}".format(where)


def _image(res):
    rows = sorted(res.group_rows) if res.query.group_by else [tuple(res.aggregation_result)]
    return rows, res.stats.num_docs_scanned, res.stats.num_entries_scanned_in_filter


def _check(res, ref):
    if res.query.group_by:
        check_groups(res, ref)
    else:
        assert all(close(a, b) for a, b in zip(res.aggregation_result, ref.aggregation_result))
    assert res.stats.num_docs_scanned == ref.num_docs_scanned


@pytest.mark.gpu
def test_segments_that_plan_differently(gpu_ctx, segs, gpu_segs, monkeypatch):
    """EMPTY fold in segment 0, a lead leaf in segment 1, no bit-sliced copy in segment 2 (no lead; prefix_loss)."""
    from pinot_amd.plan import GpuPlanMaker
    q = parse_sql(SQL_ABSENT)
    ref = engine.execute(q, segs)
    assert ref.num_docs_scanned > 0
    images = []
    for knob in ("-1", "0"):   # the segments in query order, then switched wherever the model says cheaper
        monkeypatch.setenv(KNOB, knob)
        res = GpuPlanMaker(gpu_ctx, collect_stats=True).execute(q, gpu_segs)
        _check(res, ref)
        images.append(_image(res)[:2])
    assert images[0] == images[1]
    # the same filter with a literal every dictionary holds: no segment folds
    q2 = parse_sql(SQL_AND)
    ref2 = engine.execute(q2, segs)
    _check(GpuPlanMaker(gpu_ctx, collect_stats=True).execute(q2, gpu_segs), ref2)


@pytest.mark.gpu
@pytest.mark.parametrize("nkids", [KIDS_CAP - 1, KIDS_CAP, KIDS_CAP + 1])
def test_top_level_and_at_the_inline_capacity(gpu_ctx, segs, gpu_segs, nkids):
    """cap + 1 children spill the analysis' child lists to the heap; the plan and the result are what they were."""
    from pinot_amd.plan import GpuPlanMaker
    q = parse_sql(_sql_kids(nkids))
    ref = engine.execute(q, segs)
    assert 0 < ref.num_docs_scanned < NSEG * N
    pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
    first = pm.execute(q, gpu_segs)
    _check(first, ref)
    # once more, behind a small query on the same thread's scratch
    _check(pm.execute(parse_sql(SQL_AND), gpu_segs), engine.execute(parse_sql(SQL_AND), segs))
    assert _image(pm.execute(q, gpu_segs)) == _image(first)


@pytest.mark.gpu
def test_scratch_reuse_between_alternating_queries(gpu_ctx, segs, gpu_segs):
    """A two-leaf AND and a nine-id IN under an OR (different instruction counts), submitted alternately 40 times
    with three in flight: every result equals its first, which equals the oracle's."""
    from pinot_amd.plan import GpuPlanMaker
    pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
    qs = [parse_sql(SQL_AND), parse_sql(SQL_OR)]
    first = [None, None]
    pending = deque()

    def collect_one():
        k, pq = pending.popleft()
        res = pm.collect(pq)
        if first[k] is None:
            _check(res, engine.execute(qs[k], segs))
            first[k] = _image(res)
        else:
            assert _image(res) == first[k], (k,)

    for i in range(40):
        pending.append((i % 2, pm.submit(qs[i % 2], gpu_segs)))
        if len(pending) == 3:
            collect_one()
    while pending:
        collect_one()
    assert first[0] is not None and first[1] is not None


@pytest.mark.gpu
def test_two_threads_submit_at_once(gpu_ctx, segs, gpu_segs):
    """The same two queries from two threads on one context: each thread's results equal the single-threaded one."""
    from pinot_amd.plan import GpuPlanMaker
    qs = [parse_sql(SQL_AND), parse_sql(SQL_OR)]
    want = []
    for q in qs:
        res = GpuPlanMaker(gpu_ctx, collect_stats=True).execute(q, gpu_segs)
        _check(res, engine.execute(q, segs))
        want.append(_image(res))
    errors = []
    start = threading.Barrier(2)

    def worker(k):
        try:
            pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
            start.wait(timeout=30)
            for _ in range(20):
                pq = pm.submit(qs[k], gpu_segs)
                got = _image(pm.collect(pq))
                if got != want[k]:
                    errors.append((k, got, want[k]))
                    return
        except Exception as e:  # noqa: BLE001 -- reported by the assertion below
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    assert not errors, errors[:2]
