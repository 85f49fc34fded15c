"""Fused single-launch path of submitted register-direct queries (launch_impl / fused_finalize) against the
three-launch path (PGPU_Q_SPLIT_LAUNCH) and the oracle.

A query submitted through pgpu_query_submit* that runs query_kernel_rdirect with a small table is one launch: the
kernel's last workgroup (a ticket drawn after the epilogue) reduces the per-wave statistics and the AGG slabs with
finalize_kernel's tree, writes the matched-segment flags and exports the table; the metadata arena is copied only when
its bytes changed, and a table that needs identities is the workspace's spare table when the previous fused query
wrote them.  Both paths must give the same bits: group rows, aggregation values (floats by their bits),
num_docs_scanned, num_entries_scanned_in_filter, num_segments_matched and dense_bytes.

Shapes: segments of 1, 2,048, 4,097 and 5,000 docs (tile = 2,048 docs: a lone doc, one exact tile, partial tiles; all
of these run as one workgroup) and one of 150,001 docs (several workgroups, so the ticket is drawn more than once).
Every query reads three segments: one with matches, one whose literal is absent from its dictionary (no tiles) and one
where the literal exists but no doc matches.

numEntriesScannedInFilter: the filters here are ANDs of two scan leaves, where the GPU's own count is not the
reference's leap-frogging count (pgpu_query_stats.filter_stats_exact = 0); it is compared with the oracle only when
the runtime says it is exact, and between the two launch paths always.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from oracle import engine
from oracle.segment_writer import build_segment
from pinot_amd import _lib
from pinot_amd._lib import PGPU_DOUBLE, PGPU_INT
from pinot_amd.query import parse_sql
from tests.helpers import check_groups, close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY0 = 17000
V = 3 * 777          # the residual leaf's literal
ACCT_MID = 3 << 19   # half of the residual column's values lie below
ACCT_MOST = 3_000_000  # ... and 95 % below this
BIG = 150_001
# (docs per segment, fast-leaf width in bits): a width needs more than 2^(bits - 1) distinct values, so the wide
# leaves come with the segments that can hold them
SHAPES = [(1, 6), (2048, 6), (2048, 10), (4097, 10), (4097, 12), (5000, 6), (5000, 12), (BIG, 10), (BIG, 16)]


def _card(n, bits):
    return max(1, min(n, (1 << bits) - 3))


def _window(n, bits):
    """The fast leaf's BETWEEN bounds: about 1/64 of the day values.  The planner streams a filter column densely
    while half of its 32-B sectors would be touched anyway; behind a leaf this selective the 11- to 18-bit acct
    column is not, so its leaf is the residual one, gathered per candidate -- and selective not so far that the
    prefix planes would cost more than the gathers they save."""
    c = _card(n, bits)
    return DAY0 + c // 4, DAY0 + c // 4 + max(0, c // 64 - 1)


def _segment(name, n, bits, rng, kind):
    """kind 'match': docs inside the window carry V; 'absent': no doc carries V; 'nomatch': only docs outside the
    window carry V."""
    c = _card(n, bits)
    day = DAY0 + rng.permutation(np.arange(n) % c)
    lo, hi = _window(n, bits)
    inside = (day >= lo) & (day <= hi)
    acct = 3 * rng.integers(0, 1 << 20, n)
    acct[acct == V] += 3
    if kind == "match":
        acct[inside & (rng.random(n) < 0.5)] = V
        if n == 1:
            day[0], acct[0] = lo, V
    elif kind == "nomatch":
        acct[~inside & (rng.random(n) < 0.3)] = V
        if not np.any(acct == V):
            day[0], acct[0] = hi + 1, V
    cols = {"day": (PGPU_INT, day.astype(np.int32)),
            "acct": (PGPU_INT, acct.astype(np.int32)),
            "g1k": (PGPU_INT, rng.integers(0, 1024, n).astype(np.int32)),
            "g4": (PGPU_INT, rng.integers(0, 4, n).astype(np.int32) * 11),
            "clicks": (PGPU_INT, rng.integers(0, 1 << 20, n).astype(np.int32)),
            # magnitudes over ~100 binary orders: past the fixed-point window (126 bits less 40 of tolerance), so
            # SUM(dbl) is a double sum whose bits depend on the order of the additions
            "dbl": (PGPU_DOUBLE, rng.standard_normal(n) * 10.0 ** rng.integers(-15, 16, n))}
    return build_segment(name, cols, sorted_columns=())


_SEGS = {}


def _segments(n, bits):
    if (n, bits) not in _SEGS:
        rng = np.random.default_rng(1000 * bits + n % 997)
        _SEGS[(n, bits)] = [_segment(f"f{n}_{bits}_{k}", n, bits, rng, k) for k in ("match", "absent", "nomatch")]
    return _SEGS[(n, bits)]


def _sql(kind, n, bits):
    lo, hi = _window(n, bits)
    where = f"day BETWEEN {lo} AND {hi} AND acct IN ({V})"
    if kind == "global":   # 1,024 keys: HBM atomics on the table from the first tile
        return f"SELECT g1k, COUNT(*), SUM(clicks), MAX(clicks) FROM t WHERE {where} GROUP BY g1k LIMIT 2000"
    if kind == "lds":      # 4 keys and a wide residual range: many matches per key, the table is privatised in LDS
        return (f"SELECT g4, COUNT(*), SUM(clicks) FROM t WHERE day BETWEEN {lo} AND {hi} AND acct < {ACCT_MOST} "
                f"GROUP BY g4 LIMIT 100")
    return f"SELECT COUNT(*), SUM(clicks), SUM(dbl), MIN(clicks) FROM t WHERE {where}"


def _bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def _image(res):
    """Everything the two launch paths must agree on, floats by their bits."""
    rows = res.group_rows if res.query.group_by else [tuple(res.aggregation_result)]
    st = res.stats
    return ([tuple(_bits(v) for v in r) for r in rows], st.num_docs_scanned, st.num_entries_scanned_in_filter,
            st.num_segments_matched, st.dense_bytes, None if st.segment_matched is None else st.segment_matched.tolist())


def _check_oracle(res, ref):
    if res.query.group_by:
        check_groups(res, ref)
    else:
        assert all(close(a, b) for a, b in zip(res.aggregation_result, ref.aggregation_result)), \
            (res.aggregation_result, ref.aggregation_result)
    assert res.stats.num_docs_scanned == ref.num_docs_scanned
    assert res.stats.num_segments_matched == ref.num_segments_matched
    if res.stats.filter_stats_exact:
        assert res.stats.num_entries_scanned_in_filter == ref.num_entries_scanned_in_filter


def _gpu_segments(ctx, segs, prefix=True):
    from pinot_amd.segment import GpuSegment
    # prefix off: no bit-sliced copy of the residual column, so its top planes cannot be streamed
    return [GpuSegment(ctx, s, derived=None if prefix else {"acct": 0}) for s in segs]


def _makers(ctx, **kw):
    from pinot_amd.plan import GpuPlanMaker
    return (GpuPlanMaker(ctx, collect_stats=True, **kw),
            GpuPlanMaker(ctx, collect_stats=True, query_flags=_lib.PGPU_Q_SPLIT_LAUNCH, **kw))


@pytest.mark.parametrize("kind", ["global", "lds", "agg"])
@pytest.mark.parametrize("n,bits", SHAPES, ids=[f"{n}x{b}b" for n, b in SHAPES])
def test_fused_equals_split_and_oracle(gpu_ctx, n, bits, kind):
    segs = _segments(n, bits)
    q = parse_sql(_sql(kind, n, bits))
    ref = engine.execute(q, segs)
    for prefix in (True, False):
        gs = _gpu_segments(gpu_ctx, segs, prefix)
        try:
            fused_pm, split_pm = _makers(gpu_ctx)
            split = split_pm.execute(q, gs)
            # three times: the first copies the arena and initialises the table, the later ones may find both ready
            fused = [fused_pm.execute(q, gs) for _ in range(3)]
        finally:
            for g in gs:
                g.release()
        # (one-doc segments have one-value dictionaries: their range leaf folds away and with it the fast leaf)
        assert n == 1 or split.stats.kernel_variant == _lib.PGPU_KV_RDIRECT
        want = _image(split)
        for r in fused:
            assert r.stats.kernel_variant == split.stats.kernel_variant
            assert _image(r) == want
        _check_oracle(split, ref)
        _check_oracle(fused[-1], ref)
        if kind != "lds":
            assert ref.num_segments_matched == 1  # (the absent-literal and the no-match segments)


def test_prefix_planes_are_streamed_on_both_paths(gpu_ctx):
    """With the residual column bit-sliced the prefix planes are read (3 more planes per doc under collect_stats),
    without the copy they are not: both launch paths count the same bytes in either case."""
    n, bits = 5000, 10
    segs = _segments(n, bits)
    q = parse_sql(_sql("global", n, bits))
    dense = {}
    for prefix in (True, False):
        gs = _gpu_segments(gpu_ctx, segs, prefix)
        try:
            fused_pm, split_pm = _makers(gpu_ctx)
            a, b = fused_pm.execute(q, gs), split_pm.execute(q, gs)
        finally:
            for g in gs:
                g.release()
        assert _image(a) == _image(b)
        dense[prefix] = a.stats.dense_bytes
    assert dense[True] > dense[False] > 0


def test_same_query_six_times_three_in_flight(gpu_ctx):
    n, bits = BIG, 10
    segs = _segments(n, bits)
    gs = _gpu_segments(gpu_ctx, segs)
    try:
        for kind in ("global", "lds", "agg"):
            q = parse_sql(_sql(kind, n, bits))
            fused_pm, split_pm = _makers(gpu_ctx)
            want = _image(split_pm.execute(q, gs))
            pending = [fused_pm.submit(q, gs) for _ in range(3)]
            got = []
            for _ in range(3):
                got.append(fused_pm.collect(pending.pop(0)))
                pending.append(fused_pm.submit(q, gs))
            got += [fused_pm.collect(p) for p in pending]
            assert len(got) == 6
            for r in got:
                assert _image(r) == want
    finally:
        for g in gs:
            g.release()


def test_alternating_layouts(gpu_ctx):
    """Two layouts taking turns on the same workspaces: every submit misses the spare table's signature and the
    arena shadow, or hits them when the rotation lines up; the results never change."""
    n, bits = 5000, 12
    segs = _segments(n, bits)
    gs = _gpu_segments(gpu_ctx, segs)
    lo, hi = _window(n, bits)
    sqls = [_sql("global", n, bits),
            # 4 x 1,024 keys x (count, MIN) = 8,192 cells: the largest table the fused path takes
            f"SELECT g4, g1k, MIN(clicks) FROM t WHERE day BETWEEN {lo} AND {hi} AND acct IN ({V}) "
            f"GROUP BY g4, g1k LIMIT 5000"]
    try:
        qs = [parse_sql(s) for s in sqls]
        fused_pm, split_pm = _makers(gpu_ctx)
        want = [_image(split_pm.execute(q, gs)) for q in qs]
        for q, w in zip(qs, want):
            _check_oracle(fused_pm.execute(q, gs), engine.execute(q, segs))
        for depth in (1, 2):
            pending = []
            for i in range(8):
                pending.append((i % 2, fused_pm.submit(qs[i % 2], gs)))
                if len(pending) > depth:
                    k, p = pending.pop(0)
                    assert _image(fused_pm.collect(p)) == want[k]
            for k, p in pending:
                assert _image(fused_pm.collect(p)) == want[k]
    finally:
        for g in gs:
            g.release()


def test_order_by_trim_reads_the_device_table(gpu_ctx):
    """A small-table query collected with an ORDER BY ... LIMIT trim selects from the device copy of the table, which
    must be intact after the fused epilogue (and after the spare table took its place)."""
    n, bits = 5000, 10
    segs = _segments(n, bits)
    lo, hi = _window(n, bits)
    q = parse_sql(f"SELECT g1k, SUM(clicks) FROM t WHERE day BETWEEN {lo} AND {hi} AND acct < {ACCT_MID} "
                  f"GROUP BY g1k ORDER BY SUM(clicks) DESC LIMIT 5")
    ref = engine.execute(q, segs)
    assert len(ref.group_rows) > 25  # (the trim below keeps max(5 * 5, 10) groups)
    gs = _gpu_segments(gpu_ctx, segs)
    try:
        fused_pm, split_pm = _makers(gpu_ctx, min_server_group_trim_size=10)
        split = split_pm.execute(q, gs)
        for _ in range(3):
            fused = fused_pm.execute(q, gs)
            assert _image(fused) == _image(split)
            assert [tuple(_bits(v) for v in r) for r in fused.rows] == [tuple(_bits(v) for v in r) for r in split.rows]
    finally:
        for g in gs:
            g.release()
    assert len(fused.group_rows) < len(ref.group_rows)  # trimmed on the device
    assert all(close(a, b) for r, s in zip(fused.rows, ref.rows) for a, b in zip(r, s)), (fused.rows, ref.rows)


@pytest.mark.parametrize("kind", ["global", "agg"])
def test_expired_deadline_then_next_query(gpu_ctx, kind):
    from pinot_amd.plan import GpuPlanMaker
    n, bits = BIG, 10
    segs = _segments(n, bits)
    q = parse_sql(_sql(kind, n, bits))
    gs = _gpu_segments(gpu_ctx, segs)
    try:
        fused_pm, split_pm = _makers(gpu_ctx)
        want = _image(split_pm.execute(q, gs))
        assert _image(fused_pm.execute(q, gs)) == want
        for _ in range(2):
            with pytest.raises(_lib.QueryTimeoutError):
                GpuPlanMaker(gpu_ctx, collect_stats=True, timeout_ms=-1).execute(q, gs)
            # the ticket, the matched-segment words and the spare table are as a finished query leaves them
            assert _image(fused_pm.execute(q, gs)) == want
            assert _image(fused_pm.execute(q, gs)) == want
    finally:
        for g in gs:
            g.release()


_TRACE_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
from tests.test_gpu_fused_launch import _segments, _sql, _gpu_segments, _makers
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuContext
ctx = GpuContext(0)
segs = _segments(5000, 10)
gs = _gpu_segments(ctx, segs)
fused_pm, split_pm = _makers(ctx)
for kind in ("global", "lds", "agg"):
    q = parse_sql(_sql(kind, 5000, 10))
    for _ in range(3):
        fused_pm.execute(q, gs)
    split_pm.execute(q, gs)
for g in gs:
    g.release()
ctx.close()
"""


def test_plan_trace_names_the_path():
    """PGPU_PLAN_TRACE=1 (read once per process, hence the child) says which launch path ran: a repeated query
    finds its arena resident and its table in the spare; PGPU_Q_SPLIT_LAUNCH takes the three launches."""
    env = dict(os.environ, PGPU_PLAN_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _TRACE_SCRIPT.format(root=ROOT)], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("[pgpu plan] launch ")]
    assert len(lines) == 12, lines
    for k in (0, 4):  # GLOBAL, then LDS
        assert lines[k] == "[pgpu plan] launch fused: arena copied, table initialised"
        assert lines[k + 2] == "[pgpu plan] launch fused: arena resident, table spare"
        assert lines[k + 3] == "[pgpu plan] launch split (forced): prologue, query kernels, finalize"
    assert lines[8] == "[pgpu plan] launch fused: arena copied, table needs no identities"
    assert lines[10] == "[pgpu plan] launch fused: arena resident, table needs no identities"
    assert lines[11].startswith("[pgpu plan] launch split")
    # the three queries ran in the GLOBAL (2), LDS (1) and AGG (0) modes of the register-direct kernel (direct 2)
    modes = [l.split()[3] for l in r.stderr.splitlines() if l.startswith("[pgpu plan] mode ") and " direct 2 " in l]
    assert modes == ["2"] * 4 + ["1"] * 4 + ["0"] * 4, modes
