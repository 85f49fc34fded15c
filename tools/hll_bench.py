"""DISTINCTCOUNTHLL measurement: the device sketch stage against the only way to get the same
sketches without it -- GROUP BY ..., c with COUNT(*), every row collected, each group's values sketched on the host.

Setup and shapes are tools/distinct_bench.py's: synthetic AdAnalytics segments plus a 64-value column `region`;
DISTINCTCOUNTHLL(clicks) under the two filters, aggregation-only and grouped by `region`.  Per query it reports

  new      submit + collect (pgpu_query_collect_hll) up to the sketches, warm, median (host clock around work that ends
           in the collect's device synchronise; the LUT of the global dictionary is cached by the plan maker)
  emulated SELECT [region,] clicks, COUNT(*) ... GROUP BY [region,] clicks with the trim off and no numGroupsLimit,
           every row collected and hll.sketch_of per group (the two runs alternate)
  stage    pgpu_table_hll and pgpu_table_fold alone on the query's own GROUP BY table, HIP events; the stage is their
           difference, held against the bytes it must move: section 0 once (and the key word of the occupied slots of
           a hash table), the LUT, and inner x W x 4 B of registers

and once the host cost of hll.lut for a 2^20-value INT dictionary.  One JSON line each on stdout.  Needs an MI355X; there
is no CPU fallback.

    python tools/hll_bench.py [--segments 4] [--docs 33554432] [--iters 30] [--warmup 5] [--log2m 8]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from distinct_bench import FILTERS, median_ms, workload  # noqa: E402


def stage_alone(ctx, pm, query, gs, iters: int, warmup: int) -> dict:
    """pgpu_table_hll and pgpu_table_fold on the table of the query's lowered pass, launched into torch tensors; HIP
    events on the default stream, which both are enqueued on."""
    import torch
    from pinot_amd import _lib, hll
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
    F = TableLayout()
    _lib.check(lib.pgpu_fold_layout_of(C.byref(L), inner, C.byref(F)))
    out = torch.empty(_lib.table_bytes(F) // 8, dtype=torch.int64, device="cuda")
    W = hll.num_words(p.log2m)
    lut = pm.hll_lut(globals_[-1][0], gs[0].column(p.column).data_type, p.log2m)
    dlut = torch.from_numpy(lut.view(np.int32).copy()).cuda()
    regs = torch.empty(inner * W, dtype=torch.int32, device="cuda")

    def run_hll():
        _lib.check(lib.pgpu_table_hll(ctx.handle, C.byref(L), C.c_void_p(table.data_ptr()), None, inner,
                                      C.cast(dlut.data_ptr(), C.POINTER(C.c_uint32)), len(lut), p.log2m,
                                      C.c_void_p(out.data_ptr()), out.numel() * 8, C.c_void_p(regs.data_ptr())))

    def run_fold():
        _lib.check(lib.pgpu_table_fold(ctx.handle, C.byref(L), C.c_void_p(table.data_ptr()), None, inner,
                                       C.c_void_p(out.data_ptr()), out.numel() * 8))

    def timed(run):
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
        return statistics.median(ts), min(ts)

    hll_ms, hll_min = timed(run_hll)
    fold_ms, fold_min = timed(run_fold)
    n = int(L.num_keys)
    occupied = int((table[:n] > 0).sum().item())
    hash_words = L.key_words if L.key_kind == _lib.PGPU_KEYS_HASH else 0
    must = 8 * n + 8 * occupied * hash_words + 4 * len(lut) + 4 * inner * W
    stage = max(hll_ms - fold_ms, 1e-6)
    return {"hll_and_fold_ms": hll_ms, "hll_and_fold_min_ms": hll_min, "fold_ms": fold_ms, "fold_min_ms": fold_min,
            "stage_ms": stage, "table_keys": n, "table_kind": "hash" if hash_words else "dense", "occupied": occupied,
            "inner": inner, "num_values": len(lut), "words": W, "must_bytes": must, "stage_gbps": must / stage / 1e6}


def lut_cost(log2m: int) -> dict:
    from pinot_amd import hll
    from pinot_amd._lib import PGPU_INT
    d = np.arange(1 << 20, dtype=np.int32) * 7 - (1 << 21)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        hll.lut(d, PGPU_INT, log2m)
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"lut_values": len(d), "lut_type": "INT", "log2m": log2m, "lut_ms": statistics.median(ts), "lut_min_ms": min(ts)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--docs", type=int, default=1 << 25)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--log2m", type=int, default=8)
    ap.add_argument("--filters", default="headline,days")
    args = ap.parse_args()

    import torch
    torch.cuda.init()  # torch initialises HIP first when both runtimes share the process
    from pinot_amd import hll
    from pinot_amd.plan import GpuPlanMaker
    from pinot_amd.query import parse_sql
    from pinot_amd.segment import GpuContext
    from pinot_amd.synth import build_segments_gpu

    print(json.dumps(lut_cost(args.log2m)), flush=True)
    w = workload()
    ctx = GpuContext(0)
    gs = build_segments_gpu(ctx, w, list(range(args.segments)), args.docs)
    try:
        pm = GpuPlanMaker(ctx)
        em = GpuPlanMaker(ctx, num_groups_limit=0, min_server_group_trim_size=-1)
        stored = gs[0].column("clicks").data_type
        for fname in args.filters.split(","):
            where = FILTERS[fname]
            for grouped in (False, True):
                head, tail = ("region, ", " GROUP BY region LIMIT 100") if grouped else ("", "")
                q = parse_sql(f"SELECT {head}DISTINCTCOUNTHLL(clicks, {args.log2m}) FROM {w.table} WHERE {where}{tail}")
                qe = parse_sql(f"SELECT {head}clicks, COUNT(*) FROM {w.table} WHERE {where} "
                               f"GROUP BY {head}clicks LIMIT 1000000000")

                def new():
                    return pm.collect(pm.submit(q, gs))

                def emulated():
                    cols = em.collect(em.submit(qe, gs))._columns
                    if not grouped:
                        return {(): hll.sketch_of(cols.value(0), stored, args.log2m).cardinality()}
                    r, c = cols.value(0), cols.value(1)
                    order = np.argsort(r, kind="stable")
                    r, c = r[order], c[order]
                    cuts = np.flatnonzero(np.diff(r)) + 1
                    return {int(k[0]): hll.sketch_of(v, stored, args.log2m).cardinality()
                            for k, v in zip(np.split(r, cuts), np.split(c, cuts)) if len(k)}

                got = new()
                want = emulated()
                if grouped:
                    assert {r[0]: r[1] for r in got.group_rows} == want, "the two paths disagree"
                else:
                    assert got.aggregation_result == [want.get((), 0)], (got.aggregation_result, want)
                # alternate the two paths so that drift of the shared host hits both alike
                half = max(10, args.iters // 2)
                n1 = median_ms(new, half, args.warmup)
                e1 = median_ms(emulated, half, args.warmup)
                n2 = median_ms(new, half, 1)
                e2 = median_ms(emulated, half, 1)
                line = {"filter": fname, "grouped": grouped, "segments": args.segments, "docs_per_segment": args.docs,
                        "log2m": args.log2m, "docs_matched": got.stats.num_docs_scanned, "kernel_ms": got.stats.kernel_ms,
                        "new_ms": statistics.median([n1[0], n2[0]]), "new_ms_runs": [n1[0], n2[0]],
                        "emulated_ms": statistics.median([e1[0], e2[0]]), "emulated_ms_runs": [e1[0], e2[0]]}
                line["new_over_emulated"] = line["new_ms"] / line["emulated_ms"]
                line.update(stage_alone(ctx, pm, q, gs, args.iters, args.warmup))
                print(json.dumps(line), flush=True)
    finally:
        for g in gs:
            g.release()
        ctx.close()


if __name__ == "__main__":
    main()
