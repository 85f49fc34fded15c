"""Exact MODE measurement ("MODE"): the device fold + mode reduction against the only way to get the same
answer without it -- GROUP BY ..., c with COUNT(*), every row collected, argmax in numpy.

Setup: synthetic AdAnalytics segments (pinot_amd/synth.py) plus a 64-value column `region`, as
tools/percentile_bench.py.  Query: MODE(clicks), MODE(clicks, 'AVG') under a filter, aggregation-only and grouped by
`region`.  Per query it reports

  new      submit + collect of the MODE query, warm, median (host clock around work that ends in the collect's device
           synchronise)
  emulated the same answer by SELECT [region,] clicks, COUNT(*) ... GROUP BY [region,] clicks with the trim off and no
           numGroupsLimit, every row collected, the largest count per region and its values found with numpy (the two
           runs alternate)
  mode     pgpu_table_mode alone (the fold and the reduction behind it, every reducer) on the query's own GROUP BY
           table, HIP events, beside pgpu_table_fold alone, with the bytes the call must move: section 0 twice (the
           fold, then the reduction), the other sections where count > 0, and the mode table written
  hash     mode / fold alone once more on the same query's table built with PGPU_Q_HASH, beside pgpu_table_select of one
           percentile on the same slots: the reduction's two atomic passes against the selection's sort and scan

One JSON line per query on stdout.  Needs an MI355X; there is no CPU fallback.

    python tools/mode_bench.py [--segments 4] [--docs 33554432] [--iters 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILTERS = {
    # the headline query's filter (README): 8 of 1,024 days and one of 2^20 accounts
    "headline": "daysSinceEpoch BETWEEN 17849 AND 17856 AND accountId IN (123456789)",
    # its day range alone: 1 / 128 of the docs
    "days": "daysSinceEpoch BETWEEN 17849 AND 17856",
}


def workload():
    from pinot_amd.synth import WORKLOADS, SynthColumn
    w = WORKLOADS["adanalytics"]
    region = SynthColumn("region", 64, lambda: np.arange(64, dtype=np.int32) * 10)
    return dataclasses.replace(w, name="adanalytics_mode", columns=list(w.columns) + [region])


def median_ms(fn, iters: int, warmup: int):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def modes(values: np.ndarray, counts: np.ndarray, starts: np.ndarray) -> list:
    """[MODE(c), MODE(c, 'AVG')] of each run of rows [starts[i], starts[i + 1]) (values ascending within a run):
    ModeAggregationFunction.java:463-672 over the counts."""
    if len(counts) == 0:
        return [[-float("inf")] * 2]
    top = np.maximum.reduceat(counts, starts)
    tied = counts == np.repeat(top, np.diff(np.append(starts, len(counts))))
    lo = np.minimum.reduceat(np.where(tied, values, values.max()), starts)
    s = np.add.reduceat(np.where(tied, values.astype(np.float64), 0.0), starts)
    t = np.add.reduceat(tied.astype(np.int64), starts)
    return [[float(a), float(b)] for a, b in zip(lo, s / t)]


def timed(run, iters: int, warmup: int) -> list:
    """HIP-event milliseconds of `run` on the default stream."""
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def mode_alone(ctx, pm, query, gs, iters: int, warmup: int) -> dict:
    """pgpu_table_mode, pgpu_table_fold and pgpu_table_select (one percentile) on the table of the query's lowered
    pass, launched into torch tensors."""
    import torch
    from pinot_amd import _lib
    from pinot_amd._lib import QueryStats, TableLayout
    lib = ctx._lib
    (p,) = pm.distinct_passes(query)
    expr = pm.filter_expr(p.query, gs)
    desc, keep, globals_ = pm.build_desc(p.query, gs, plan_filters=expr is None, num_groups_limit=0)
    L = pm.layout(desc)
    nbytes = _lib.table_bytes(L)
    table = torch.empty(nbytes // 8, dtype=torch.int64, device="cuda")
    h = C.c_void_p()
    if expr is not None:
        _lib.check(lib.pgpu_query_launch_expr(ctx.handle, C.byref(desc), expr[0], expr[1], None,
                                              C.c_void_p(table.data_ptr()), nbytes, C.byref(h)))
    else:
        _lib.check(lib.pgpu_query_launch(ctx.handle, C.byref(desc), None, C.c_void_p(table.data_ptr()), nbytes,
                                         C.byref(h)))
    st = QueryStats()
    try:
        _lib.check(lib.pgpu_query_wait(h, C.byref(st)))
    finally:
        lib.pgpu_query_release(h)
    inner = 1
    for g in globals_[:-1]:
        inner *= len(g[0])
    reducers = _lib.PGPU_MODE_MIN | _lib.PGPU_MODE_MAX | _lib.PGPU_MODE_AVG
    M = TableLayout()
    _lib.check(lib.pgpu_mode_layout_of(C.byref(L), inner, 1, reducers, C.byref(M)))  # (room for the select run too)
    out = torch.empty(_lib.table_bytes(M) // 8, dtype=torch.int64, device="cuda")
    values = torch.from_numpy(np.ascontiguousarray(globals_[-1][0], dtype=np.float64)).cuda()
    pp = (C.c_double * 1)(50.0)

    def fold():
        _lib.check(lib.pgpu_table_fold(ctx.handle, C.byref(L), C.c_void_p(table.data_ptr()), None, inner,
                                       C.c_void_p(out.data_ptr()), out.numel() * 8))

    def mode():
        _lib.check(lib.pgpu_table_mode(ctx.handle, C.byref(L), C.c_void_p(table.data_ptr()), None, inner, None, 0,
                                       reducers, C.c_void_p(values.data_ptr()), values.numel(),
                                       C.c_void_p(out.data_ptr()), out.numel() * 8))

    def select():
        _lib.check(lib.pgpu_table_select(ctx.handle, C.byref(L), C.c_void_p(table.data_ptr()), None, inner, pp, 1,
                                         C.c_void_p(out.data_ptr()), out.numel() * 8))

    tf = timed(fold, iters, warmup)
    tm = timed(mode, iters, warmup)
    ts = timed(select, iters, warmup)
    n = int(L.num_keys)
    occupied = int((table[:n] > 0).sum().item())
    hash_words = L.key_words if L.key_kind == _lib.PGPU_KEYS_HASH else 0
    must = 2 * 8 * n + 8 * occupied * (L.num_sections - 1 + hash_words) + 8 * (L.num_sections + 6) * inner
    ms, fms, sms = statistics.median(tm), statistics.median(tf), statistics.median(ts)
    return {"mode_ms": ms, "mode_min_ms": min(tm), "fold_ms": fms, "reduce_ms": ms - fms, "select_ms": sms,
            "picks_ms": sms - fms, "table_keys": n, "table_bytes": nbytes,
            "table_kind": "hash" if hash_words else "dense", "occupied": occupied, "inner": inner,
            "num_values": values.numel(), "must_bytes": must, "mode_gbps": must / ms / 1e6}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--docs", type=int, default=1 << 25)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--filters", default="headline,days")
    args = ap.parse_args()

    import torch
    torch.cuda.init()  # torch initialises HIP first when both runtimes share the process
    from pinot_amd._lib import PGPU_Q_HASH
    from pinot_amd.plan import GpuPlanMaker
    from pinot_amd.query import parse_sql
    from pinot_amd.segment import GpuContext
    from pinot_amd.synth import build_segments_gpu

    w = workload()
    ctx = GpuContext(0)
    gs = build_segments_gpu(ctx, w, list(range(args.segments)), args.docs)
    try:
        pm = GpuPlanMaker(ctx)
        em = GpuPlanMaker(ctx, num_groups_limit=0, min_server_group_trim_size=-1)
        aggs = "MODE(clicks), MODE(clicks, 'AVG')"
        for fname in args.filters.split(","):
            where = FILTERS[fname]
            for grouped in (False, True):
                head, tail = ("region, ", " GROUP BY region LIMIT 100") if grouped else ("", "")
                q = parse_sql(f"SELECT {head}{aggs} FROM {w.table} WHERE {where}{tail}")
                qe = parse_sql(f"SELECT {head}clicks, COUNT(*) FROM {w.table} WHERE {where} "
                               f"GROUP BY {head}clicks LIMIT 1000000000")

                def new():
                    return pm.collect(pm.submit(q, gs))

                def emulated():
                    cols = em.collect(em.submit(qe, gs))._columns
                    if not grouped:
                        return modes(cols.value(0), cols.count, np.zeros(1, dtype=np.int64))[0]
                    reg, clk, cnt = cols.value(0), cols.value(1), cols.count
                    o = np.lexsort((clk, reg))
                    reg, clk, cnt = reg[o], clk[o], cnt[o]
                    starts = np.concatenate([[0], np.flatnonzero(np.diff(reg)) + 1]).astype(np.int64)
                    return {int(r): m for r, m in zip(reg[starts], modes(clk, cnt, starts))}

                got = new()
                want = emulated()
                if grouped:
                    assert {r[0]: list(r[1:]) for r in got.group_rows} == want, "the two paths disagree"
                else:
                    assert got.aggregation_result == want, (got.aggregation_result, want)
                # alternate the two paths so that drift of the shared host hits both alike
                half = max(10, args.iters // 2)
                n1 = median_ms(new, half, args.warmup)
                e1 = median_ms(emulated, half, args.warmup)
                n2 = median_ms(new, half, 1)
                e2 = median_ms(emulated, half, 1)
                line = {"filter": fname, "grouped": grouped, "segments": args.segments, "docs_per_segment": args.docs,
                        "docs_matched": got.stats.num_docs_scanned, "kernel_ms": got.stats.kernel_ms,
                        "new_ms": statistics.median([n1[0], n2[0]]), "new_ms_runs": [n1[0], n2[0]],
                        "emulated_ms": statistics.median([e1[0], e2[0]]), "emulated_ms_runs": [e1[0], e2[0]]}
                line["new_over_emulated"] = line["new_ms"] / line["emulated_ms"]
                line.update(mode_alone(ctx, pm, q, gs, args.iters, args.warmup))
                # the same table built as a hash table (PGPU_Q_HASH): two atomic passes against a sort and a scan
                hm = GpuPlanMaker(ctx, query_flags=PGPU_Q_HASH)
                line["hash"] = {k: v for k, v in mode_alone(ctx, hm, q, gs, args.iters, args.warmup).items()
                                if k in ("mode_ms", "fold_ms", "reduce_ms", "select_ms", "picks_ms", "table_keys",
                                         "table_bytes", "table_kind", "occupied")}
                print(json.dumps(line), flush=True)
    finally:
        for g in gs:
            g.release()
        ctx.close()


if __name__ == "__main__":
    main()
