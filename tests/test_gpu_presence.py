"""Tile presence rows (pgpu_presence.hip, plan_presence in pgpu_runtime.cpp, rdirect_consumer's skip loop): a point
predicate on a wide dictionary column lets the register-direct kernel stream only the tiles whose presence rows can
hold one of its ids.  PGPU_PRESENCE_AFTER=0 builds the rows inside seal, -1 never builds nor skips, and
PGPU_PRESENCE_SWITCH_BYTES=0 skips whenever the model says it saves a byte (the default keeps queries this small on
their full scan).  PGPU_LEAD_SWITCH_BYTES=0 puts the point leaf in front, as the lead plan does at full size.

Three segments of 3 * 2048 + 5, 70,001 and 2048 * 33 docs: a partial last tile, 35 tiles across a word boundary of
the rows, and exactly one word more.  The point column is 20 bits wide with uniformly random ids; literals are
planted in tile 0, tile 31, tile 32 and the last tile only, in every tile, and in none.  Each case equals the
oracle and the -1 run bit for bit, agrees across fused, split and overlapped launches, and reports the
numEntriesScannedInFilter computed here from the data: the tiles kept by pgpu_presence_rows times the lead plan's
entry rule -- one number that shows both that exactly the predicted tiles were skipped and that none holding a match
was.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import engine
from oracle.segment_writer import bits_per_value, build_segment, dictionary_bytes, pack_fixed_bit
from pinot_amd import _lib
from pinot_amd._lib import PGPU_INT
from pinot_amd.query import parse_sql
from pinot_amd.segment import ColumnIndexes
from tests.helpers import check_groups, close
from tests.test_gpu_lead_planes import DAY, DAY0, DAY_HI, DAY_LO, _image, _mask, _rows, _run_all_paths, _sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (3 * 2048 + 5, 70_001, 2048 * 33)
WT = 2048
T0, T31, T32, LAST, NODOC, ALL = 1000, 2000, 3000, 4000, 5000, 6000   # dict ids of the planted literals
PLANTED = (T0, T31, T32, LAST, NODOC, ALL)
ABSENT_VALUE = 3 * 7000 + 1   # the dictionaries hold multiples of 3 only
AFTER, SWITCH, LEAD = "PGPU_PRESENCE_AFTER", "PGPU_PRESENCE_SWITCH_BYTES", "PGPU_LEAD_SWITCH_BYTES"


def _card(k):
    return (1 << 19) + 100 + 7 * k   # 20 bits, different per segment (as test_gpu_lead_planes._card)


def _segment(k, n, rng):
    day = (DAY0 + rng.permutation(np.arange(n) % 1024)).astype(np.int32)
    tile = np.arange(n) // WT
    ntiles = int(tile[-1]) + 1
    card = _card(k)
    ids = rng.integers(0, card, n)
    ids[np.isin(ids, PLANTED)] += 10_000
    where = {T0: [0], T31: [31], T32: [32], LAST: [ntiles - 1], ALL: list(range(ntiles))}
    for lit, tiles in where.items():
        for t in tiles:
            docs = np.flatnonzero(tile == t)
            if len(docs) == 0:
                continue
            pick = rng.choice(docs, size=min(4, len(docs)), replace=False)
            ids[pick] = lit
            day[pick[: (len(pick) + 1) // 2]] = DAY_LO   # half of them match behind the day window
    cols = {"day": (PGPU_INT, day), "g16": (PGPU_INT, rng.integers(0, 16, n).astype(np.int32)),
            "g1": (PGPU_INT, np.full(n, 7, np.int32)), "clicks": (PGPU_INT, rng.integers(0, 1 << 20, n).astype(np.int32))}
    seg = build_segment(f"presence{k}", cols, sorted_columns=())
    raw = {c: v for c, (_, v) in cols.items()}
    small = rng.integers(0, 1024, n)
    for name, c_ids, c_card in (("acct", ids, card), ("s10", small, 1024)):
        col = ColumnIndexes(name, PGPU_INT, c_card, dictionary=dictionary_bytes(3 * np.arange(c_card), PGPU_INT))
        col.forward = pack_fixed_bit(c_ids, bits_per_value(c_card))
        seg.columns[name] = col
        raw[name] = (3 * c_ids).astype(np.int64)
    return seg, raw


_BUILT = {}


def _segments():
    if not _BUILT:
        rng = np.random.default_rng(77)
        built = [_segment(k, n, rng) for k, n in enumerate(SIZES)]
        _BUILT["segs"], _BUILT["raws"] = [s for s, _ in built], [r for _, r in built]
        assert bits_per_value(_card(0)) == 20
    return _BUILT["segs"], _BUILT["raws"]


_ROWS = {}


def _rows_of(x):
    if x not in _ROWS:
        _ROWS[x] = _lib.presence_rows(int(x))
    return _ROWS[x]


_SIGS = {}


def _signatures(k, raw):
    """Per tile of segment k: the set of presence rows its docs' ids set (the rows' definition, from the library's
    hash)."""
    if k not in _SIGS:
        ids = raw["acct"] // 3
        _SIGS[k] = [set(r for x in np.unique(ids[t0:t0 + WT]) for r in _rows_of(x)) for t0 in range(0, len(ids), WT)]
    return _SIGS[k]


def _kept_docs(k, raw, lits, has_rows=True):
    """Doc mask of the tiles the rows keep for the ids `lits`: OR over ids of AND over the four probes."""
    n = len(raw["acct"])
    if not has_rows:
        return np.ones(n, bool)
    kept = np.array([any(all(r in sig for r in _rows_of(x)) for x in lits) for sig in _signatures(k, raw)])
    return np.repeat(kept, WT)[:n]


def _point_ids(values, card):
    return [v // 3 for v in values if v % 3 == 0 and v // 3 < card]


def _planes(lits, card):
    runs = [(x, x + 1) for x in sorted(lits)]
    return _lib.lead_model(10, 8 / 1024, _lib.PGPU_LEAD_RESID_B, 1, 20, len(lits) / card, runs).planes


def _entries(segs, raws, children, lead, skip=True, no_rows=()):
    """numEntriesScannedInFilter under the lead plan (test_gpu_lead_planes._lead_entries) over the kept tiles only:
    every doc of a kept tile once for the lead leaf, the exact leaf for the docs whose top P id bits can match, then
    the other children for the docs every leaf before kept.  A skipped tile adds nothing."""
    total = 0
    for k, (seg, raw) in enumerate(zip(segs, raws)):
        card = seg.column("acct").cardinality
        lits = _point_ids(children[lead][2], card)
        if not lits:
            continue   # the segment's filter folds to EMPTY
        P, bits = _planes(lits, card), 20
        kd = _kept_docs(k, raw, lits, has_rows=skip and k not in no_rows)
        total += int(kd.sum())
        reach = kd & np.isin((raw["acct"] // 3) >> (bits - P), np.asarray(lits) >> (bits - P))
        for c in [lead] + [j for j in range(len(children)) if j != lead]:
            total += int(reach.sum())
            reach = reach & _mask(raw, children[c])
    return total


def _acct(*ids, extra=()):
    return ("acct", "in", [3 * x for x in ids] + list(extra))


# (id, children, skips)
CASES = [
    ("eq_tile0", [DAY, _acct(T0)], True),
    ("eq_tile31", [DAY, _acct(T31)], True),
    ("eq_last", [DAY, _acct(LAST)], True),
    ("in2_word_boundary", [DAY, _acct(T31, T32)], True),
    ("in4", [DAY, _acct(T0, T31, T32, LAST)], True),
    ("every_tile", [DAY, _acct(ALL)], True),
    ("absent_from_dictionary", [DAY, _acct(T32, extra=[ABSENT_VALUE])], True),
    ("in5", [DAY, _acct(T0, T31, T32, LAST, ALL)], False),
    ("not_in", [DAY, ("acct", "not in", [3 * T0])], False),
    ("range", [DAY, ("acct", "between", 3 * (T0 - 20), 3 * (T0 + 20))], False),
    ("small_dictionary", [DAY, ("s10", "in", [3 * 5, 3 * 900])], False),
]


@pytest.fixture(scope="module")
def seal_env():
    """The module's segments are sealed with PGPU_PRESENCE_AFTER=0 (rows built inside seal)."""
    old = os.environ.get(AFTER)
    os.environ[AFTER] = "0"
    yield
    if old is None:
        os.environ.pop(AFTER, None)
    else:
        os.environ[AFTER] = old


@pytest.fixture(scope="module")
def gpu_segs(gpu_ctx, seal_env):
    from pinot_amd.segment import GpuSegment
    segs, raws = _segments()
    used0 = gpu_ctx.derived_bytes()[0]
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    yield segs, raws, gs
    for g in gs:
        g.release()
    assert gpu_ctx.derived_bytes()[0] == used0


def _knobs(monkeypatch, after):
    monkeypatch.setenv(AFTER, after)
    monkeypatch.setenv(SWITCH, "0")
    monkeypatch.setenv(LEAD, "0")


def _check_oracle(r, ref, q):
    if q.group_by:
        check_groups(r, ref)
    else:
        assert all(close(a, b) for a, b in zip(r.aggregation_result, ref.aggregation_result))
    assert r.stats.num_docs_scanned == ref.num_docs_scanned
    assert r.stats.num_segments_matched == ref.num_segments_matched


@pytest.mark.gpu
def test_rows_are_accounted(gpu_ctx, gpu_segs):
    segs, _, gs = gpu_segs
    for s, g in zip(segs, gs):
        b = g.device_bytes_by_kind()
        ntiles = (s.num_docs + WT - 1) // WT
        # every column with a bit-sliced copy (six at most): 16,384 rows of ceil(ntiles / 32) words each
        unit = 16384 * 4 * ((ntiles + 31) // 32)
        assert b["presence"] % unit == 0 and unit <= b["presence"] <= 6 * unit
        assert b["total"] == g.device_bytes() == sum(v for k, v in b.items() if k != "total")


@pytest.mark.gpu
@pytest.mark.parametrize("name,children,skips", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("mode", ["agg", "global"])
def test_skip_vs_oracle_and_never(gpu_ctx, gpu_segs, monkeypatch, name, children, skips, mode):
    from pinot_amd.plan import GpuPlanMaker
    segs, raws, gs = gpu_segs
    q = parse_sql(_sql(children, mode))
    ref = engine.execute(q, segs)
    _knobs(monkeypatch, "-1")
    off = GpuPlanMaker(gpu_ctx, collect_stats=True).execute(q, gs)
    _knobs(monkeypatch, "0")
    res = _run_all_paths(gpu_ctx, q, gs)
    for r in (res, off):
        _check_oracle(r, ref, q)
    assert ref.num_docs_scanned > 0
    assert _rows(res) == _rows(off)
    if not skips:   # nothing to skip by: the -1 run in every figure
        assert _image(res) == _image(off)
        return
    assert res.stats.kernel_variant == _lib.PGPU_KV_RDIRECT
    want, full = _entries(segs, raws, children, 1), _entries(segs, raws, children, 1, skip=False)
    print(f"{name}: entries {res.stats.num_entries_scanned_in_filter} (model {want}), full scan "
          f"{off.stats.num_entries_scanned_in_filter} (model {full})")
    assert off.stats.num_entries_scanned_in_filter == full
    assert res.stats.num_entries_scanned_in_filter == want
    assert want <= full and (want < full or name == "every_tile")
    # the stats pass counts the kept tiles' planes plus the row words read: fewer bytes wherever tiles were skipped, a
    # few more where every tile is kept
    if name == "every_tile":
        assert off.stats.dense_bytes < res.stats.dense_bytes < 1.01 * off.stats.dense_bytes
    else:
        assert res.stats.dense_bytes < off.stats.dense_bytes


@pytest.mark.gpu
def test_literal_in_no_doc_matches_nothing(gpu_ctx, gpu_segs, monkeypatch):
    segs, raws, gs = gpu_segs
    children = [DAY, _acct(NODOC)]
    q = parse_sql(_sql(children, "agg"))
    ref = engine.execute(q, segs)
    _knobs(monkeypatch, "0")
    res = _run_all_paths(gpu_ctx, q, gs)
    assert ref.num_docs_scanned == 0 == res.stats.num_docs_scanned
    assert res.stats.num_segments_matched == 0
    assert res.stats.num_entries_scanned_in_filter == _entries(segs, raws, children, 1)


@pytest.mark.gpu
def test_or_and_exact_filter_stats_do_not_skip(gpu_ctx, gpu_segs, monkeypatch):
    from pinot_amd.plan import GpuPlanMaker
    segs, _, gs = gpu_segs
    q_or = parse_sql(f"SELECT COUNT(*), SUM(clicks) FROM t WHERE day BETWEEN {DAY_LO} AND {DAY_HI} OR acct IN ({3 * T0})")
    q_and = parse_sql(_sql([DAY, _acct(T0)], "agg"))
    for q, kw in ((q_or, {}), (q_and, dict(exact_filter_stats=True))):
        images = []
        for after in ("-1", "0"):
            _knobs(monkeypatch, after)
            images.append(_image(GpuPlanMaker(gpu_ctx, collect_stats=not kw, **kw).execute(q, gs)))
        assert images[0] == images[1]
    ref = engine.execute(q_and, segs, iterator_stats=True)
    assert images[1][2] == ref.num_entries_scanned_in_filter


@pytest.mark.gpu
def test_segment_without_rows_beside_two_with(gpu_ctx, monkeypatch):
    """The 70,001-doc segment is sealed without rows and the budget is used up when a query asks for them: it is
    declined for good and scanned in full, in the launch that skips through the other two."""
    from pinot_amd.segment import GpuSegment
    segs, raws = _segments()
    children = [DAY, _acct(T31, T32)]
    q = parse_sql(_sql(children, "global"))
    ref = engine.execute(q, segs)
    used0, budget0 = gpu_ctx.derived_bytes()
    gs = []
    try:
        for k, s in enumerate(segs):
            monkeypatch.setenv(AFTER, "2" if k == 1 else "0")
            gs.append(GpuSegment(gpu_ctx, s))
        gpu_ctx.set_derived_budget(gpu_ctx.derived_bytes()[0])
        _knobs(monkeypatch, "0")
        for _ in range(2):   # (the second run finds the column declined)
            res = _run_all_paths(gpu_ctx, q, gs)
            _check_oracle(res, ref, q)
            assert res.stats.num_entries_scanned_in_filter == _entries(segs, raws, children, 1, no_rows=(1,))
        assert gs[1].device_bytes_by_kind()["presence"] == 0
    finally:
        gpu_ctx.set_derived_budget(budget0)
        for g in gs:
            g.release()
    assert gpu_ctx.derived_bytes()[0] == used0


@pytest.mark.gpu
def test_built_on_use(gpu_ctx, monkeypatch):
    """PGPU_PRESENCE_AFTER=2: the first query scans in full, the second asks for the rows, and once they are built
    the same query skips and returns the same rows; release gives the bytes back."""
    import torch
    from pinot_amd.plan import GpuPlanMaker
    from pinot_amd.segment import GpuSegment
    segs, raws = _segments()
    children = [DAY, _acct(T32)]
    q = parse_sql(_sql(children, "agg"))
    want, full = _entries(segs, raws, children, 1), _entries(segs, raws, children, 1, skip=False)
    used0 = gpu_ctx.derived_bytes()[0]
    _knobs(monkeypatch, "2")
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    try:
        sealed = gpu_ctx.derived_bytes()[0]
        assert all(g.device_bytes_by_kind()["presence"] == 0 for g in gs)
        pm = GpuPlanMaker(gpu_ctx, collect_stats=True)
        first = pm.execute(q, gs)
        assert first.stats.num_entries_scanned_in_filter == full
        assert gpu_ctx.derived_bytes()[0] == sealed
        second = pm.execute(q, gs)   # the trigger: it may or may not see the rows itself
        assert gpu_ctx.derived_bytes()[0] > sealed
        torch.cuda.synchronize()
        later = second
        for _ in range(200):   # no submit waits for a build: ask until one finds the rows
            later = pm.execute(q, gs)
            if later.stats.num_entries_scanned_in_filter != full:
                break
        assert later.stats.num_entries_scanned_in_filter == want < full
        assert _rows(later) == _rows(first) == _rows(second)
        assert all(g.device_bytes_by_kind()["presence"] > 0 for g in gs)
    finally:
        for g in gs:
            g.release()
    assert gpu_ctx.derived_bytes()[0] == used0


@pytest.mark.gpu
def test_release_right_after_the_triggering_submit(gpu_ctx, monkeypatch):
    from pinot_amd.plan import GpuPlanMaker
    from pinot_amd.segment import GpuSegment
    segs, _ = _segments()
    q = parse_sql(_sql([DAY, _acct(T0)], "agg"))
    used0 = gpu_ctx.derived_bytes()[0]
    _knobs(monkeypatch, "1")
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    pm = GpuPlanMaker(gpu_ctx)
    pending = pm.submit(q, gs)   # the trigger: its builds start when it is collected
    for g in gs:
        g.release()              # ... and the segments are gone by then: nothing is built, nothing dangles
    pm.collect(pending)
    assert gpu_ctx.derived_bytes()[0] == used0


@pytest.mark.gpu
def test_release_while_the_build_is_in_flight(gpu_ctx, monkeypatch):
    """Collecting the trigger query enqueues the build (here of a 2^24-doc segment: 256 row words walked by a quarter
    of the CUs); the release right behind it waits for the build before the planes and the rows are freed."""
    from pinot_amd.plan import GpuPlanMaker
    from pinot_amd.synth import WORKLOADS, build_segments_gpu
    w = WORKLOADS["adanalytics"]
    used0 = gpu_ctx.derived_bytes()[0]
    _knobs(monkeypatch, "1")
    gs = build_segments_gpu(gpu_ctx, w, [0], 1 << 24)
    try:
        sealed = gpu_ctx.derived_bytes()[0]
        pm = GpuPlanMaker(gpu_ctx, num_groups_limit=w.options.get("num_groups_limit", 100_000))
        pm.collect(pm.submit(parse_sql(w.sql), gs))
        assert gpu_ctx.derived_bytes()[0] == sealed + 16384 * 4 * 256   # reserved when the build was enqueued
        assert gs[0].device_bytes_by_kind()["presence"] == 16384 * 4 * 256
    finally:
        for g in gs:
            g.release()
    assert gpu_ctx.derived_bytes()[0] == used0


_CHILD = r"""
import json, os, sys
sys.path.insert(0, {root!r})
from pinot_amd.plan import GpuPlanMaker
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuContext
from tests.test_gpu_lead_planes import _image
mode = sys.argv[1]
ctx = GpuContext(0)
out = []
if mode == "synth":   # 256 workgroups over 2 x 8,192 tiles: 64 tiles = two row words of one segment each
    from pinot_amd.synth import WORKLOADS, build_segments_gpu
    w = WORKLOADS["adanalytics"]
    gs = build_segments_gpu(ctx, w, [0, 1], 1 << 24)
    q = parse_sql(w.sql)
    pm = GpuPlanMaker(ctx, collect_stats=True, num_groups_limit=w.options.get("num_groups_limit", 100000))
    im = _image(pm.execute(q, gs))
    out += [repr((im[0], im[1], im[3], im[5])), im[2]]
    os.environ["PGPU_PRESENCE_AFTER"] = "0"   # built on use from the first asking submit on
    for _ in range(50):                       # (no submit waits for the build)
        im = _image(pm.execute(q, gs))
        if im[2] < 0.1 * out[1]:              # (both segments' rows are there)
            break
    out += [repr((im[0], im[1], im[3], im[5])), im[2]]
else:                 # plan lines of the small segments, rows built on use
    from tests.test_gpu_presence import CASES, _segments
    from tests.test_gpu_lead_planes import _sql
    from pinot_amd.segment import GpuSegment
    segs, _ = _segments()
    gs = [GpuSegment(ctx, s) for s in segs]
    pm = GpuPlanMaker(ctx, collect_stats=True)
    for name, children, skips in CASES:
        q = parse_sql(_sql(children, "agg"))
        for _ in range(3):
            pm.execute(q, gs)
            sys.stderr.write("[case] %s\n" % name)
for g in gs:
    g.release()
ctx.close()
print(json.dumps(out))
"""


def _child(mode, **env):
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), mode], capture_output=True, text=True,
                       env=dict(os.environ, PGPU_PLAN_TRACE="1", **env), timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr.splitlines()


@pytest.mark.gpu
def test_ranges_of_two_chunks():
    """PGPU_DIRECT_WGS is read once per process, hence the child: one workgroup per CU over two 2^24-doc segments gives
    every workgroup 64 tiles, two row words of one segment, and with PGPU_PRESENCE_CHUNK_WORDS=1 a chunk of keep bits
    is one word: every wave steps from its range's first chunk to its second (at the default 64 words a range would
    have to pass 2,048 tiles of one segment for that)."""
    out, err = _child("synth", PGPU_DIRECT_WGS="1", PGPU_PRESENCE_CHUNK_WORDS="1",
                      **{SWITCH: "0", LEAD: "0", AFTER: "-1"})
    never, never_entries, skip, skip_entries = out
    assert never == skip
    heads = [l for l in err if l.startswith("[pgpu plan] mode ")]
    assert " grid 256 " in heads[0] and " tiles 16384 " in heads[0]
    assert " skip col " not in heads[0] and " skip col " not in heads[1]
    assert re.search(r" skip col \d+ ids 1 keep 0\.0259$", heads[-1]), heads[-1]
    assert skip_entries < 0.1 * never_entries


@pytest.mark.gpu
def test_plan_lines():
    """The first query on fresh segments never skips; once the rows are there a skipping query's line ends in its
    skip field, and no other line changes."""
    _, err = _child("small", **{SWITCH: "0", LEAD: "0", AFTER: "1"})
    heads, case = {}, []
    for l in err:
        if l.startswith("[pgpu plan] mode "):
            case.append(l)
        elif l.startswith("[case] "):
            heads.setdefault(l.split()[1], []).extend(case)
            case = []
    first = CASES[0][0]
    assert " skip col " not in heads[first][0]
    for name, children, skips in CASES:
        lines = heads[name]
        assert len(lines) == 3
        if not skips:
            assert not any(" skip col " in l for l in lines), (name, lines)
            continue
        n = len([v for v in children[1][2] if v % 3 == 0])
        if name != first:   # (the first case's own queries may all run before its rows are built)
            assert any(re.search(rf" skip col \d+ ids {n} keep [01]\.\d+$", l) for l in lines), (name, lines)
        # the line up to the skip field is the line without it
        assert len(set(l.split(" skip col ")[0] for l in lines)) == 1, (name, lines)
