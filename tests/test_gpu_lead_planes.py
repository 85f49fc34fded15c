"""Lead leaf of the register-direct kernel (lead_model / lead_choice in pgpu_runtime.cpp, DevSeg::f_plane0): a
top-level AND whose later child is far more selective than its first streams only the top P bit planes of that
child's column, gathers the child's exact id for the docs whose prefix can match, and gathers the former first
child only for the exact matches.  PGPU_LEAD_SWITCH_BYTES=0 switches whenever the model says cheaper (the default
threshold keeps queries this small on their own order), -1 never.

Three segments of 1, 3 * 2048 + 5 and 70,001 docs; the lead column's width comes from a dictionary padded with
values no doc holds (9, 11, 17, 20, 24 bits), so the plane offset bits - P takes odd, even and zero values.  Each
case: fused, split and overlapped launches agree bit for bit, equal the oracle and the switch-off run, the stats pass
shows P bits per doc streamed, and the GPU's own numEntriesScannedInFilter is every doc once for the lead leaf plus
one per residual leaf per doc that reached it -- which also pins the residual children's order.
"""
import json
import os
import re
import struct
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3 * 2048 + 5, 70_001)
# lead columns: a<bits> is <bits> wide in both large segments; a17f fills its 17 bits (ids up to the last prefix);
# amix is 11 bits wide in the 6,149-doc segment and 20 in the 70,001-doc one, so the two take different P
COLUMNS = ("a9", "a11", "a17", "a20", "a24", "a17f", "amix")
DAY0 = 17000
DAY_LO, DAY_HI = DAY0 + 300, DAY0 + 307   # 8 of 1024 days: the acct columns are gathered per candidate behind it
KNOB = "PGPU_LEAD_SWITCH_BYTES"
A17F_TOP = 131_000   # ids from here up lie in the last 10-bit prefix of a17f
AMIX_ID = 256


def _card(bits, k):
    """Dictionary size of the `bits`-wide column in segment k: past 2^(bits - 1), different per segment."""
    return (1 << (bits - 1)) + 100 + 7 * (k - 1)


def _col_card(name, k):
    if name == "a17f":
        return (1 << 17) - 5 - 7 * (k - 1)
    if name == "amix":
        return _card(11 if k == 1 else 20, k)
    return _card(int(name[1:]), k)


def _lits(bits):
    """Dict ids (value = 3 * id) planted in the docs: one in the middle, two in other prefixes, one that only
    the last segment's dictionary holds."""
    h = 1 << (bits - 1)
    return {"mid": h // 2, "low": 5, "high": h + 9, "last_only": h + 103}


def _col_lits(name):
    if name == "a17f":
        return [A17F_TOP + 40]
    if name == "amix":
        return [AMIX_ID]
    return list(_lits(int(name[1:])).values())


def _segment(k, n, rng, columns):
    # The 1-doc segment's filter folds to EMPTY in every case (its one value is no multiple of 3).  It cannot take
    # part in a register-direct launch otherwise: a one-value dictionary folds each leaf to ALL or EMPTY, and a
    # segment left without a streamed leaf keeps the whole query off this kernel, with a lead leaf or without.
    if n == 1:
        cols = {"day": (PGPU_INT, np.array([DAY_LO], np.int32)), "g16": (PGPU_INT, np.array([3], np.int32)),
                "g1": (PGPU_INT, np.array([7], np.int32)), "clicks": (PGPU_INT, np.array([17], np.int32))}
        cols.update({c: (PGPU_INT, np.array([1], np.int32)) for c in columns})
        return build_segment(f"lead{k}", cols, sorted_columns=()), {c: v for c, (_, v) in cols.items()}
    day = (DAY0 + rng.permutation(np.arange(n) % 1024)).astype(np.int32)
    inside = (day >= DAY_LO) & (day <= DAY_HI)
    cols = {"day": (PGPU_INT, day), "g16": (PGPU_INT, rng.integers(0, 16, n).astype(np.int32)),
            "g1": (PGPU_INT, np.full(n, 7, np.int32)), "clicks": (PGPU_INT, rng.integers(0, 1 << 20, n).astype(np.int32))}
    seg = build_segment(f"lead{k}", cols, sorted_columns=())
    raw = {c: v for c, (_, v) in cols.items()}
    for name in columns:
        card = _col_card(name, k)
        ids = rng.integers(0, card, n)
        for lit in _col_lits(name):
            if lit >= card:
                continue
            ids[inside & (rng.random(n) < 0.2)] = lit      # matches behind the day window
            ids[~inside & (rng.random(n) < 0.01)] = lit    # ... and docs only this leaf keeps
        col = ColumnIndexes(name, PGPU_INT, card, dictionary=dictionary_bytes(3 * np.arange(card), PGPU_INT))
        col.forward = pack_fixed_bit(ids, bits_per_value(card))
        seg.columns[name] = col
        raw[name] = (3 * ids).astype(np.int64)
    return seg, raw


_SEGS = {}


def _segments(columns=COLUMNS):
    if columns not in _SEGS:
        rng = np.random.default_rng(20 + len(columns))
        built = [_segment(k, n, rng, columns) for k, n in enumerate(SIZES)]
        _SEGS[columns] = ([s for s, _ in built], [r for _, r in built])
        for name in columns:
            if name[1:].isdigit():
                assert all(bits_per_value(s.column(name).cardinality) == int(name[1:]) for s in _SEGS[columns][0][1:])
    return _SEGS[columns]


# ---- cases: (id, WHERE children in query order, lead child or None, expected P or None, table mode) ----------------
DAY = ("day", "between", DAY_LO, DAY_HI)


def _in(bits, *names):
    return (f"a{bits}", "in", [3 * _lits(bits)[n] for n in names])


A20_MID = _lits(20)["mid"]
CASES = [
    ("a9_in1", [DAY, _in(9, "mid")], 1, 9, "agg"),               # P = bits: a plain reorder
    ("a11_in1", [DAY, _in(11, "mid")], 1, 11, "day"),
    ("a17_in1", [DAY, _in(17, "mid")], 1, 10, "global"),         # bits - P = 7
    ("a20_in1", [DAY, _in(20, "mid")], 1, 10, "agg"),
    ("a24_in1", [DAY, _in(24, "mid")], 1, 10, "day"),
    ("a20_in3", [DAY, _in(20, "mid", "low", "high")], 1, 12, "global"),   # three prefixes: 12 planes are cheapest
    # 6 ids in 6 prefixes that are no neighbours at any width: more than PGPU_SLICE_RANGES ranges, no switch
    ("a20_in6", [DAY, ("a20", "in", [3 * A20_MID] + [3 * ((j << 16) + 1) for j in (0, 1, 2, 3, 6)])], None, None, "agg"),
    # ids [mid - 20, mid + 20]: mid is a multiple of every 2^(20 - P), so the range straddles a prefix boundary
    ("a20_range", [DAY, ("a20", "between", 3 * (A20_MID - 20), 3 * (A20_MID + 20))], 1, 10, "day"),
    ("a20_absent", [DAY, _in(20, "last_only")], 1, 10, "agg"),   # EMPTY fold in the 6,149-doc segment too
    ("a20_not_in", [DAY, ("a20", "not in", [3 * A20_MID])], None, None, "agg"),
    ("three_mid", [DAY, _in(20, "mid"), ("a11", "lt", 3 * 600)], 1, 10, "global"),
    ("three_last", [DAY, ("a11", "lt", 3 * 600), _in(20, "mid")], 2, 10, "agg"),
    # half of the days and 3,001 ids (0.57 % of the docs): today both leaves stream (30 planes); the ids share one
    # 8-bit prefix, so 8 planes lead, and enough docs match one key for the LDS table
    ("lds_mode", [("day", "between", DAY0, DAY0 + 511), ("a20", "between", 3 * A20_MID, 3 * (A20_MID + 3000))],
     1, 8, "lds"),
    # ids from 131,000 to the end of a dictionary that fills its 17 bits: the last 10-bit prefix, range [1023, 2^10)
    ("a17f_top", [DAY, ("a17f", "between", 3 * A17F_TOP, 3 * (1 << 17))], 1, 10, "agg"),
    # 11 bits in one segment (exact lead leaf, P = 11, no offset), 20 in the other (P = 10, offset 10): the launch
    # holds 12 planes, and the 10-plane segment's upper two read as 0
    ("mixed_p", [DAY, ("amix", "in", [3 * AMIX_ID])], 1, (0, 11, 10), "day"),
]


def _where(children):
    out = []
    for col, op, *args in children:
        if op == "between":
            out.append(f"{col} BETWEEN {args[0]} AND {args[1]}")
        elif op == "lt":
            out.append(f"{col} < {args[0]}")
        else:
            out.append(f"{col} {op.upper()} ({', '.join(str(v) for v in args[0])})")
    return " AND ".join(out)


def _sql(children, mode):
    where = _where(children)
    if mode == "day":     # 1,024 keys on the 10-bit column: a table the LDS could hold, but a filter this selective
        # matches too few docs to pay for a copy per workgroup, so the table stays in HBM (GLOBAL)
        return f"SELECT day, COUNT(*), SUM(clicks) FROM t WHERE {where} GROUP BY day LIMIT 2000"
    if mode == "global":  # 16,384 keys: past the LDS table, GLOBAL whatever matches
        return f"SELECT day, g16, COUNT(*), SUM(clicks), MAX(clicks) FROM t WHERE {where} GROUP BY day, g16 LIMIT 100000"
    if mode == "lds":     # one key: the LDS table pays from ~160 matches on
        return f"SELECT g1, COUNT(*), SUM(clicks) FROM t WHERE {where} GROUP BY g1 LIMIT 10"
    return f"SELECT COUNT(*), SUM(clicks), MIN(clicks) FROM t WHERE {where}"


def _mask(raw, child):
    col, op, *args = child
    v = raw[col]
    if op == "between":
        return (v >= args[0]) & (v <= args[1])
    if op == "lt":
        return v < args[0]
    m = np.isin(v, args[0])
    return ~m if op == "not in" else m


def _folds_empty(seg, children):
    """A child whose literals the segment's dictionary cannot match folds the segment's filter to EMPTY."""
    for col, op, *args in children:
        d = np.frombuffer(seg.column(col).dictionary, dtype=">i4")
        if op == "in" and not np.isin(args[0], d).any():
            return True
        if op == "between" and not ((d >= args[0]) & (d <= args[1])).any():
            return True
    return False


def _p_of(Ps, k):
    """Planes of segment k: one figure for all, or one per segment (None: the segment keeps its order)."""
    return Ps[k] if isinstance(Ps, tuple) else Ps


def _streamed_bytes(segs, children, Ps, stay_bits=10):
    """dense_bytes of the stats pass: P bits per doc of a switched segment, the day planes of one that stays."""
    return sum(s.num_docs * (stay_bits if _p_of(Ps, k) is None else _p_of(Ps, k)) / 8
               for k, s in enumerate(segs) if not _folds_empty(s, children))


def _lead_entries(segs, raws, children, lead, Ps):
    """The GPU's numEntriesScannedInFilter under the lead plan: every doc of a scanned segment once for the lead
    leaf; then the lead child's exact leaf (unless P is its full width) for the docs whose top P id bits can match,
    and the other children in query order, each for the docs every leaf before it kept."""
    total = 0
    col = children[lead][0]
    for k_seg, (seg, raw) in enumerate(zip(segs, raws)):
        if _folds_empty(seg, children):
            continue
        P = _p_of(Ps, k_seg)
        if P is None:  # this segment keeps its order: the first child over every doc, the rest per candidate
            total += seg.num_docs
            reach = _mask(raw, children[0])
            for k in range(1, len(children)):
                total += int(reach.sum())
                reach = reach & _mask(raw, children[k])
            continue
        card = seg.column(col).cardinality
        bits = bits_per_value(card)
        _, op, *args = children[lead]
        lits = np.arange(args[0] // 3, args[1] // 3 + 1) if op == "between" else np.asarray(args[0]) // 3
        lits = lits[lits < card]  # (dict id = value / 3)
        reach = np.isin((raw[col] // 3) >> (bits - P), lits >> (bits - P))
        total += seg.num_docs
        rest = ([lead] if P < bits else []) + [k for k in range(len(children)) if k != lead]
        if P >= bits:
            reach = _mask(raw, children[lead])
        for k in rest:
            total += int(reach.sum())
            reach = reach & _mask(raw, children[k])
    return total


def _bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def _rows(res):
    rows = res.group_rows if res.query.group_by else [tuple(res.aggregation_result)]
    return [tuple(_bits(v) for v in r) for r in rows]


def _image(res):
    st = res.stats
    return (_rows(res), st.num_docs_scanned, st.num_entries_scanned_in_filter, st.num_segments_matched, st.dense_bytes,
            st.kernel_variant)


def _gpu_segments(ctx, segs):
    from pinot_amd.segment import GpuSegment
    return [GpuSegment(ctx, s) for s in segs]


@pytest.fixture(scope="module")
def gpu_segs(gpu_ctx):
    segs, raws = _segments()
    gs = _gpu_segments(gpu_ctx, segs)
    yield segs, raws, gs
    for g in gs:
        g.release()


def _run_all_paths(ctx, q, gs):
    """The query through the fused launch, the three-launch path and two overlapping submits: one image."""
    from pinot_amd.plan import GpuPlanMaker
    fused_pm = GpuPlanMaker(ctx, collect_stats=True)
    split_pm = GpuPlanMaker(ctx, collect_stats=True, query_flags=_lib.PGPU_Q_SPLIT_LAUNCH)
    res = fused_pm.execute(q, gs)
    want = _image(res)
    assert _image(split_pm.execute(q, gs)) == want
    pending = [fused_pm.submit(q, gs) for _ in range(2)]
    for pq in pending:
        assert _image(fused_pm.collect(pq)) == want
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name,children,lead,P,mode", CASES, ids=[c[0] for c in CASES])
def test_lead_plan_vs_oracle_and_switch_off(gpu_ctx, gpu_segs, monkeypatch, name, children, lead, P, mode):
    from pinot_amd.plan import GpuPlanMaker
    segs, raws, gs = gpu_segs
    q = parse_sql(_sql(children, mode))
    ref = engine.execute(q, segs)
    monkeypatch.setenv(KNOB, "-1")
    off = GpuPlanMaker(gpu_ctx, collect_stats=True).execute(q, gs)
    monkeypatch.setenv(KNOB, "0")
    res = _run_all_paths(gpu_ctx, q, gs)
    for r in (res, off):
        if q.group_by:
            check_groups(r, ref)
        else:
            assert all(close(a, b) for a, b in zip(r.aggregation_result, ref.aggregation_result))
        assert r.stats.num_docs_scanned == ref.num_docs_scanned
        assert r.stats.num_segments_matched == ref.num_segments_matched
    assert ref.num_docs_scanned > 0
    assert _rows(res) == _rows(off)
    scanned = sum(s.num_docs for s in segs if not _folds_empty(s, children))
    assert scanned >= SIZES[2]
    if lead is None:  # the query keeps its order: the switch-off run in every figure
        assert _image(res) == _image(off)
        return
    assert res.stats.kernel_variant == _lib.PGPU_KV_RDIRECT
    # the stats pass streamed P planes per doc of the lead column and nothing else
    assert res.stats.dense_bytes == pytest.approx(_streamed_bytes(segs, children, P), rel=0.02)
    assert off.stats.dense_bytes >= scanned * 10 / 8 * 0.98
    assert res.stats.num_entries_scanned_in_filter == _lead_entries(segs, raws, children, lead, P)


@pytest.mark.gpu
def test_one_segment_switches_beside_one_that_keeps_its_order(gpu_ctx, monkeypatch):
    """The 6,149-doc segment has no bit-sliced copy of a20, so it has no lead leaf and keeps the day planes in front
    (and, with a lead leaf elsewhere in the launch, no prefix planes); the 70,001-doc segment leads with 10 a20
    planes.  One launch of the register-direct kernel runs both."""
    from pinot_amd.plan import GpuPlanMaker
    from pinot_amd.segment import GpuSegment
    segs, raws = _segments()
    children = [DAY, _in(20, "mid")]
    q = parse_sql(_sql(children, "day"))
    ref = engine.execute(q, segs)
    gs = [GpuSegment(gpu_ctx, s, derived={"a20": 0} if k == 1 else None) for k, s in enumerate(segs)]
    try:
        monkeypatch.setenv(KNOB, "-1")
        off = GpuPlanMaker(gpu_ctx, collect_stats=True).execute(q, gs)
        monkeypatch.setenv(KNOB, "0")
        res = _run_all_paths(gpu_ctx, q, gs)
    finally:
        for g in gs:
            g.release()
    for r in (res, off):
        check_groups(r, ref)
        assert r.stats.num_docs_scanned == ref.num_docs_scanned > 0
        assert r.stats.kernel_variant == _lib.PGPU_KV_RDIRECT
    assert _rows(res) == _rows(off)
    Ps = (None, None, 10)
    assert res.stats.dense_bytes == pytest.approx(_streamed_bytes(segs, children, Ps), rel=0.02)
    assert res.stats.num_entries_scanned_in_filter == _lead_entries(segs, raws, children, 1, Ps)
    # switched off, both segments keep their order: every doc for the day leaf, every candidate for the a20 leaf
    assert off.stats.num_entries_scanned_in_filter == _lead_entries(segs, raws, children, 1, (None, None, None))


@pytest.mark.gpu
def test_exact_filter_stats_keep_their_plan(gpu_ctx, gpu_segs, monkeypatch):
    """rfsm streams both leaves in full for the reference's count: no lead leaf, with the knob or without."""
    from pinot_amd.plan import GpuPlanMaker
    segs, _, gs = gpu_segs
    segs, gs = segs[1:], gs[1:]  # (rfsm wants two leaves in every segment: not the one whose filter folds to EMPTY)
    q = parse_sql(_sql([DAY, _in(20, "mid")], "agg"))
    ref = engine.execute(q, segs, iterator_stats=True)
    images = []
    for knob in ("-1", "0"):
        monkeypatch.setenv(KNOB, knob)
        r = GpuPlanMaker(gpu_ctx, exact_filter_stats=True).execute(q, gs)
        assert r.stats.kernel_variant == _lib.PGPU_KV_RFSM
        assert r.stats.filter_stats_exact
        assert r.stats.num_entries_scanned_in_filter == ref.num_entries_scanned_in_filter
        assert r.stats.num_docs_scanned == ref.num_docs_scanned
        images.append(_image(r))
    assert images[0] == images[1]


_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
from tests.test_gpu_lead_planes import CASES, _segments, _sql, _gpu_segments, _image
from pinot_amd.plan import GpuPlanMaker
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuContext
ctx = GpuContext(0)
segs, _ = _segments(("a11", "a20"))
gs = _gpu_segments(ctx, segs)
out = []
for name, children, lead, P, mode in CASES:
    if name in ("a20_in1", "a20_range", "three_mid", "lds_mode"):
        r = GpuPlanMaker(ctx, collect_stats=True).execute(parse_sql(_sql(children, mode)), gs)
        out.append(repr(_image(r)))
for g in gs:
    g.release()
ctx.close()
print(json.dumps(out))
"""


def _child(**env):
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True,
                       env=dict(os.environ, PGPU_PLAN_TRACE="1", **env), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    plan = [l for l in r.stderr.splitlines() if l.startswith("[pgpu plan] mode ") or l.startswith("[pgpu plan]  seg ")]
    return json.loads(r.stdout.strip().splitlines()[-1]), plan


@pytest.mark.gpu
def test_without_the_register_direct_kernel_nothing_changes():
    """PGPU_NO_RDIRECT and PGPU_PLAN_TRACE are read once per process, hence the children.  A query that does not end
    on the register-direct kernel is packed again in query order: plan lines and results are those of the switch-off
    run.  With the kernel, the switched query's plan line carries the lead field and no prefix planes."""
    on, plan_on = _child(PGPU_NO_RDIRECT="1", **{KNOB: "0"})
    off, plan_off = _child(PGPU_NO_RDIRECT="1", **{KNOB: "-1"})
    assert plan_on == plan_off and len(plan_on) == 4 * 4
    assert on == off
    assert not any(" lead col " in l or " direct 2 " in l for l in plan_on)
    _, plan = _child(**{KNOB: "0"})
    heads = [l for l in plan if l.startswith("[pgpu plan] mode ")]
    assert len(heads) == 4
    for l, planes in zip(heads, (10, 10, 10, 8)):  # a20_in1, a20_range, three_mid, lds_mode
        assert " direct 2 " in l and f" rd_planes {planes} rd_pfx 0 " in l and " lead col " in l and \
            f" P {planes} bytes " in l, l
    assert [l.split()[3] for l in heads] == ["0", "2", "2", "1"]  # AGG, GLOBAL, GLOBAL, LDS
    # query order: 10 day planes, 3 prefix planes and 2 lines per tile; lead: 10 account planes, 2 lines and the
    # day gather of the exact matches (the model itself: tests/test_lead_model.py)
    today = lead = 0.0
    for k in (1, 2):
        m = _lib.lead_model(10, 8 / 1024, _lib.PGPU_LEAD_RESID_B, 1, 20, 1 / _card(20, k), [(A20_MID, A20_MID + 1)])
        assert m.planes == 10 and m.today_bytes == 3584 and round(m.lead_bytes) == 2816
        today += (SIZES[k] + 2047) // 2048 * m.today_bytes
        lead += (SIZES[k] + 2047) // 2048 * m.lead_bytes
    assert re.search(rf" nwaves \d+ lead col \d+ P 10 bytes {today:.0f}->{lead:.0f}$", heads[0]), heads[0]
