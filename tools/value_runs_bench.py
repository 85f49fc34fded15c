"""Value-runs measurement: the mergeable intermediates of DISTINCTCOUNT / PERCENTILE / MODE collected
as value runs from the device, against the only way to get them without that stage -- GROUP BY [region,] clicks with
COUNT(*), every row collected and grouped in numpy (§4.26's "emulated" path).

Setup and the four shapes are tools/distinct_bench.py's.  Per shape it reports

  new      submit_mergeable + pgpu_query_collect_runs of DISTINCTCOUNT(clicks) (the rows and the CSR of runs as numpy
           arrays; the decoding into Python values is the same work behind either path and is not timed), warm, median
  emulated SELECT [region,] clicks, COUNT(*) ... GROUP BY [region,] clicks with the trim off and no numGroupsLimit,
           every row collected, sorted by (region, clicks) and cut into the same CSR with numpy; the two alternate
  runs     pgpu_table_runs alone on the query's own GROUP BY table, HIP events, with the bytes it must move: section 0
           once per pass over it (the count and the emit: twice for dense input; the hash input's slots once, and its
           pairs through the sort), plus 12 B per run and the offsets

One JSON line per shape on stdout.  Needs an MI355X; there is no CPU fallback.

    python tools/value_runs_bench.py [--segments 4] [--docs 33554432] [--iters 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from distinct_bench import FILTERS, median_ms, workload  # noqa: E402


def runs_alone(ctx, pm, query, gs, iters: int, warmup: int) -> dict:
    """pgpu_table_runs on the table of the query's lowered pass, launched into torch tensors; HIP events on the
    default stream, which the stage is enqueued on."""
    import torch
    from pinot_amd import _lib
    from pinot_amd._lib import QueryStats
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
    n = int(L.num_keys)
    occupied = int((table[:n] > 0).sum().item())
    off = torch.empty(inner + 1, dtype=torch.int64, device="cuda")
    cids = torch.empty(max(occupied, 1), dtype=torch.int32, device="cuda")
    cnts = torch.empty(max(occupied, 1), dtype=torch.int64, device="cuda")

    def run():
        _lib.check(lib.pgpu_table_runs(ctx.handle, C.byref(L), C.c_void_p(table.data_ptr()), None, inner,
                                       C.c_void_p(off.data_ptr()), C.c_void_p(cids.data_ptr()),
                                       C.c_void_p(cnts.data_ptr()), occupied))

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    assert int(off[inner].item()) == occupied
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    hashed = L.key_kind == _lib.PGPU_KEYS_HASH
    # dense: section 0 in the count and again in the emit; hash: the slots once (counts, and keys where occupied)
    must = (8 * n + 8 * occupied if hashed else 2 * 8 * n) + 12 * occupied + 8 * (inner + 1)
    ms = statistics.median(ts)
    return {"runs_ms": ms, "runs_min_ms": min(ts), "table_keys": n, "table_kind": "hash" if hashed else "dense",
            "occupied": occupied, "inner": inner, "must_bytes": must, "runs_gbps": must / ms / 1e6}


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
        for fname in args.filters.split(","):
            where = FILTERS[fname]
            for grouped in (False, True):
                head, tail = ("region, ", " GROUP BY region LIMIT 100") if grouped else ("", "")
                q = parse_sql(f"SELECT {head}DISTINCTCOUNT(clicks) FROM {w.table} WHERE {where}{tail}")
                qe = parse_sql(f"SELECT {head}clicks, COUNT(*) FROM {w.table} WHERE {where} "
                               f"GROUP BY {head}clicks LIMIT 1000000000")

                def new():
                    pending = pm.submit_mergeable(q, gs)
                    (pr,) = [pm._collect_runs(pq) for pq in pending.pending]
                    pending.pending = []
                    return pr

                def emulated():
                    cols = em.collect(em.submit(qe, gs))._columns
                    clicks, counts = cols.value(1 if grouped else 0), cols.count
                    if not grouped:  # rows come ascending by key: the one group's runs as they are
                        return np.array([0, len(clicks)]), clicks, counts
                    region = cols.value(0)
                    order = np.lexsort((clicks, region))
                    _, sizes = np.unique(region, return_counts=True)
                    return np.concatenate([[0], np.cumsum(sizes)]), clicks[order], counts[order]

                pr = new()
                off, values, counts = emulated()
                assert np.array_equal(pr.offsets.astype(np.int64), off), "the two paths disagree"
                assert np.array_equal(np.asarray(pr.dictionary)[pr.cids], values) and np.array_equal(pr.counts, counts)
                # alternate the two paths so that drift of the shared host hits both alike
                half = max(10, args.iters // 2)
                n1 = median_ms(new, half, args.warmup)
                e1 = median_ms(emulated, half, args.warmup)
                n2 = median_ms(new, half, 1)
                e2 = median_ms(emulated, half, 1)
                line = {"filter": fname, "grouped": grouped, "segments": args.segments, "docs_per_segment": args.docs,
                        "docs_matched": pr.result.stats.num_docs_scanned, "kernel_ms": pr.result.stats.kernel_ms,
                        "groups": len(pr.offsets) - 1, "runs": len(pr.cids),
                        "new_ms": statistics.median([n1[0], n2[0]]), "new_ms_runs": [n1[0], n2[0]],
                        "emulated_ms": statistics.median([e1[0], e2[0]]), "emulated_ms_runs": [e1[0], e2[0]]}
                line["new_over_emulated"] = line["new_ms"] / line["emulated_ms"]
                line.update(runs_alone(ctx, pm, q, gs, args.iters, args.warmup))
                print(json.dumps(line), flush=True)
    finally:
        for g in gs:
            g.release()
        ctx.close()


if __name__ == "__main__":
    main()
