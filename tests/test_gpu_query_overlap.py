"""Two query streams: neighbouring fused (one-launch) queries run on alternate streams and may share the GPU.

A submitted query that takes the fused path runs on the stream the previous fused query did not use; every other pair of
neighbours in submit order is ordered by a wait for the earlier query's completion event.  Whatever is in flight
together, every query must give the bits it gives alone: "expected" is always the `_image` of the same query run alone
through the PGPU_Q_SPLIT_LAUNCH maker.

Shapes: 150,001 docs with a 10-bit fast leaf (several workgroups, so two kernels really are co-resident) and 5,000
docs with a 12-bit one (one workgroup).  Segments and helpers are those of tests/test_gpu_fused_launch.py.
"""
import math
import os
import subprocess
import sys
import time

import pytest

from pinot_amd import _lib
from pinot_amd.query import parse_sql
from tests.test_gpu_fused_launch import BIG, _gpu_segments, _image, _makers, _segments, _sql

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("global", "lds", "agg")
SHAPES = [(BIG, 10), (5000, 12)]


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """Per shape: the GPU segments, the three queries, and each query's image when it runs alone and split (computed
    once, never changed)."""
    out = {}
    for n, bits in SHAPES:
        gs = _gpu_segments(gpu_ctx, _segments(n, bits))
        qs = [parse_sql(_sql(k, n, bits)) for k in KINDS]
        split_pm = _makers(gpu_ctx)[1]
        out[(n, bits)] = (gs, qs, [_image(split_pm.execute(q, gs)) for q in qs])
    yield out
    for gs, _, _ in out.values():
        for g in gs:
            g.release()


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("n,bits", SHAPES, ids=[f"{n}x{b}b" for n, b in SHAPES])
def test_three_kinds_rotating(gpu_ctx, world, n, bits, depth):
    """Different layouts, tables and workspaces on the two streams at once."""
    gs, qs, want = world[(n, bits)]
    pm = _makers(gpu_ctx)[0]
    pending, done = [], 0
    for i in range(12):
        pending.append((i % 3, pm.submit(qs[i % 3], gs)))
        if len(pending) > depth - 1:
            k, p = pending.pop(0)
            assert _image(pm.collect(p)) == want[k], (i, k)
            done += 1
    for k, p in pending:
        assert _image(pm.collect(p)) == want[k], k
        done += 1
    assert done == 12


@pytest.mark.parametrize("n,bits", SHAPES, ids=[f"{n}x{b}b" for n, b in SHAPES])
def test_fused_and_split_mixed(gpu_ctx, world, n, bits):
    gs, qs, want = world[(n, bits)]
    fused_pm, split_pm = _makers(gpu_ctx)
    pending, got = [], []
    for i, c in enumerate("FFSFSSFF"):
        pm = fused_pm if c == "F" else split_pm
        pending.append((i % 3, pm, pm.submit(qs[i % 3], gs)))
        if len(pending) > 2:  # three in flight
            k, m, p = pending.pop(0)
            got.append((k, _image(m.collect(p))))
    got += [(k, _image(m.collect(p))) for k, m, p in pending]
    assert len(got) == 8
    for k, im in got:
        assert im == want[k], k


def test_collect_out_of_submit_order(gpu_ctx, world):
    gs, qs, want = world[(BIG, 10)]
    pm = _makers(gpu_ctx)[0]
    pending = [pm.submit(qs[i % 3], gs) for i in range(4)]
    for i in (2, 0, 3, 1):
        r = pm.collect(pending[i])
        assert _image(r) == want[i % 3], i
        print(f"collect {i}: kernel_ms {r.stats.kernel_ms}")
        assert math.isfinite(r.stats.kernel_ms) and r.stats.kernel_ms >= 0, (i, r.stats.kernel_ms)


@pytest.mark.parametrize("victim", [1, 0], ids=["later", "earlier"])
def test_cancel_one_of_two_in_flight(gpu_ctx, world, victim):
    """The cancelled query skips its tiles and still runs its epilogue: the ticket and the matched-segment words of
    both workspaces are zero again, whichever stream they were last used on."""
    gs, qs, want = world[(BIG, 10)]
    pm = _makers(gpu_ctx)[0]
    pending = [pm.submit(qs[0], gs), pm.submit(qs[1], gs)]
    pending[victim].cancel()
    for i in (0, 1):
        if i == victim:
            with pytest.raises(_lib.QueryCancelledError) as ei:
                pm.collect(pending[i])
            assert ei.value.code == _lib.PGPU_E_CANCELLED
        else:
            assert _image(pm.collect(pending[i])) == want[i]
    nxt = [pm.submit(qs[0], gs), pm.submit(qs[1], gs)]
    for i, p in enumerate(nxt):
        assert _image(pm.collect(p)) == want[i], i


def test_kernel_ms_sums_to_no_more_than_the_wall_time(gpu_ctx, world):
    """kernel_ms of a fused query is the time its kernel held the GPU that no earlier fused query's kernel also held,
    so the sum over queries is the GPU's busy time, which the host's wall time around them bounds.

    Each figure is also held against the same query alone: a kernel that shares the CUs with one other kernel of the
    same work runs at most twice as long as alone, and the part of that it does not share is no longer than that, so
    kernel_ms <= 2 x alone (the largest of three runs alone) + 0.01 ms for the timestamps' resolution.  At this size
    (25 us of kernel against some hundred us of host time per submit) the GPU is idle between queries, so neither
    assertion can tell the accounting from the raw ev0 .. ev1 span; they bound it, and the period-long figures of the
    benchmark are checked there (roofline.kernel_ms_avg against ms_per_step)."""
    gs, qs, want = world[(BIG, 10)]
    pm = _makers(gpu_ctx)[0]
    alone = max(pm.collect(pm.submit(qs[0], gs)).stats.kernel_ms for _ in range(3))
    ms = []
    t0 = time.perf_counter()
    pending = [pm.submit(qs[0], gs) for _ in range(3)]
    for _ in range(3):
        ms.append(pm.collect(pending.pop(0)).stats.kernel_ms)
        pending.append(pm.submit(qs[0], gs))
    ms += [pm.collect(p).stats.kernel_ms for p in pending]
    wall_ms = (time.perf_counter() - t0) * 1e3
    print(f"kernel_ms {ms} sum {sum(ms)} wall_ms {wall_ms} alone {alone}")
    assert len(ms) == 6 and all(math.isfinite(m) and m >= 0 for m in ms), ms
    assert sum(ms) <= wall_ms, (ms, wall_ms)
    assert all(m <= 2 * alone + 0.01 for m in ms), (ms, alone)


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
from tests.test_gpu_fused_launch import _segments, _sql, _gpu_segments, _makers, _image
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuContext
ctx = GpuContext(0)
gs = _gpu_segments(ctx, _segments(5000, 12))
fused_pm, split_pm = _makers(ctx)
q = parse_sql(_sql("global", 5000, 12))
want = _image(split_pm.execute(q, gs))                 # S
pending = [fused_pm.submit(q, gs) for _ in range(3)]   # F F F
got = [_image(fused_pm.collect(p)) for p in pending]
got.append(_image(split_pm.execute(q, gs)))            # S
got.append(_image(fused_pm.execute(q, gs)))            # F
assert all(g == want for g in got), (got, want)
print(repr(got))
for g in gs:
    g.release()
ctx.close()
"""


def test_trace_names_the_stream_and_the_knob_keeps_one():
    """PGPU_PLAN_TRACE and PGPU_QUERY_STREAMS are read once per process, hence the children."""
    def run(**extra):
        env = {k: v for k, v in os.environ.items() if k != "PGPU_QUERY_STREAMS"}
        env.update(PGPU_PLAN_TRACE="1", **extra)
        r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, env=env,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        err = r.stderr.splitlines()
        launches = [l.split()[3].rstrip(":") for l in err if l.startswith("[pgpu plan] launch ")]
        assert launches == ["split", "fused", "fused", "fused", "split", "fused"], launches
        return [l for l in err if l.startswith("[pgpu plan] stream ")], r.stdout

    two, images = run()
    # fused queries alternate (the first takes stream 0); a split query is on stream 0 and does not change whose turn
    # it is
    assert two == [f"[pgpu plan] stream {s} of 2" for s in (0, 0, 1, 0, 0, 1)], two
    one, images_one = run(PGPU_QUERY_STREAMS="1")
    assert one == ["[pgpu plan] stream 0 of 1"] * 6, one
    assert images_one == images


_ORDER_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
from tests.test_gpu_fused_launch import BIG, _segments, _sql, _gpu_segments, _makers, _image
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuContext
ctx = GpuContext(0)
gs = _gpu_segments(ctx, _segments(BIG, 10))
fused_pm, split_pm = _makers(ctx)
q = parse_sql(_sql("global", BIG, 10))
want = _image(split_pm.execute(q, gs))
sys.stderr.write("[test] begin\n")
sys.stderr.flush()
for order in ("SFF", "FFSFF"):
    pending = [(split_pm if c == "S" else fused_pm) for c in order]
    pending = [(pm, pm.submit(q, gs)) for pm in pending]   # all in flight
    for pm, p in pending:
        assert _image(pm.collect(p)) == want
for g in gs:
    g.release()
ctx.close()
"""


def test_a_split_query_shares_the_gpu_with_no_later_fused_query():
    """S F F and F F S F F, each all in flight.  The first fused query after a split one may land on the split query's
    own stream, behind it; the next one, on the other stream, must then wait for the split query too, or it would run
    beside it.  Which waits are enqueued is read from the trace: at these sizes a kernel (25 us) ends long before the
    host has submitted the next query (some hundred us), so no timing could show a missing wait."""
    env = {k: v for k, v in os.environ.items() if k != "PGPU_QUERY_STREAMS"}
    env.update(PGPU_PLAN_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _ORDER_CHILD.format(root=ROOT)], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    err = r.stderr.splitlines()
    err = err[err.index("[test] begin") + 1:]
    got = []
    for l in err:
        if l.startswith("[pgpu plan] stream "):
            got.append(l.split()[3])
        elif l.startswith("[pgpu plan] order: "):
            assert l.startswith("[pgpu plan] order: waits for the last query on stream "), l
            got[-1] += " behind " + l.split()[-1]
    # S F F: the second F, on stream 1, waits for S.  Then F F S F F: nothing is in flight on stream 1 for the first
    # two; S waits for the F on stream 1; the F after it is behind it on stream 0; the last F waits for S.
    assert got == ["0", "0", "1 behind 0"] + ["0", "1", "0 behind 1", "0", "1 behind 0"], got
