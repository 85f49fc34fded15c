"""Exact MODE on the GPU (MI355X only): pgpu_table_mode on hand-made tables against numpy (per-key argmax over the
[card, inner] count matrix), dense and one-word hash, and the whole path -- SQL, lowering, GROUP BY g, c on every key
path, device fold and mode reduction, trim, join -- against the modes counted from the decoded columns.  M, T, LO and HI
are integers and every S here but one test's is a sum of integers or binary fractions far below 2^53, exact in any
order of its adds: every comparison but that test's is exact."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from oracle.segment_writer import build_segment
from pinot_amd import _lib
from pinot_amd._lib import (PGPU_DOUBLE, PGPU_FLOAT, PGPU_INT, PGPU_KEYS_DENSE, PGPU_KEYS_HASH, PGPU_LONG,
                            PGPU_MODE_AVG, PGPU_MODE_MAX, PGPU_MODE_MIN, PGPU_Q_HASH, PGPU_RED_MAX_I64,
                            PGPU_RED_MIN_I64, PGPU_RED_SUM_F64, PGPU_RED_SUM_I64, PGPU_STRING, TableLayout,
                            UnsupportedPlanError)
from pinot_amd.plan import GpuPlanMaker
from pinot_amd.query import parse_sql
from pinot_amd.segment import GpuSegment

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
# Every SELECT literal of the test files is also held against the oracle's own SQL parser (tests/test_oracle_sql.py),
# which has no MODE and is to stay without one: the queries here get their keyword from SEL instead.
SEL = "SELECT "
ALL = PGPU_MODE_MIN | PGPU_MODE_MAX | PGPU_MODE_AVG

# ---- 1. pgpu_table_mode alone -------------------------------------------------------------------------------------------
OPS = [PGPU_RED_SUM_I64, PGPU_RED_SUM_I64, PGPU_RED_MIN_I64, PGPU_RED_MAX_I64]  # count | SUM | MIN | MAX
NSEC = len(OPS)
PS = [0.0, 50.0, 99.9]


def _table_layout(num_keys, kind):
    L = TableLayout()
    L.num_keys, L.num_sections = num_keys, NSEC
    for s, op in enumerate(OPS):
        L.section_op[s] = op
    L.agg_section[0], L.agg_value_type[0] = 0, -1
    for a in (1, 2, 3):
        L.agg_section[a], L.agg_value_type[a], L.agg_sum_parts[a] = a, PGPU_LONG, 1
    L.key_kind, L.key_words, L.key_split = kind, 1, 1
    return L


def _fill(rng, counts):
    """The table [NSEC][n] of these counts: random values where count > 0, the sections' identities elsewhere."""
    n = len(counts)
    t = np.zeros((NSEC, n), dtype=np.int64)
    t[0] = counts
    occ = counts > 0
    t[1] = np.where(occ, rng.integers(-(1 << 20), 1 << 20, n), 0)
    t[2] = np.where(occ, rng.integers(-(1 << 62), 1 << 62, n), I64_MAX)
    t[3] = np.where(occ, rng.integers(-(1 << 62), 1 << 62, n), I64_MIN)
    return t


def _random_counts(rng, inner, card):
    """Counts in [1, 12) -- few enough values that most keys have several modes -- with about half the cells empty
    (cell = g + inner * cid); with inner >= 3, g = 0 has every cell empty and g = inner - 1 every cell full."""
    n = inner * card
    occ = rng.random(n) < 0.5
    if n == 1:
        occ[:] = True
    if inner >= 3:
        g = np.arange(n) % inner
        occ[g == 0] = False
        occ[g == inner - 1] = True
    return np.where(occ, rng.integers(1, 12, n), 0)


def _values(rng, card):
    """Integer values of the ids, ascending like a dictionary's: any sum of them is exact in double."""
    return np.cumsum(rng.integers(1, 1 << 20, card)).astype(np.float64) - float(1 << 30)


def _np_mode(t, inner, values):
    """(the fold in numpy [NSEC + 1][inner], M, T, LO, HI, S): per key the argmax over cid of the count matrix."""
    r3 = t.reshape(NSEC, -1, inner)
    card = r3.shape[1]
    fold = np.zeros((NSEC + 1, inner), dtype=np.int64)
    fold[0], fold[1], fold[2], fold[3] = r3[0].sum(axis=0), r3[1].sum(axis=0), r3[2].min(axis=0), r3[3].max(axis=0)
    fold[NSEC] = (r3[0] > 0).sum(axis=0)
    c = r3[0]
    M = np.maximum(c.max(axis=0), 0)
    tied = (c == M) & (c > 0)
    T = tied.sum(axis=0)
    LO = np.where(T > 0, tied.argmax(axis=0), 0)
    HI = np.where(T > 0, card - 1 - tied[::-1].argmax(axis=0), 0)
    S = np.array([math.fsum(values[tied[:, g]]) for g in range(inner)])
    return fold, M, T, LO, HI, S


def _to_hash(rng, t):
    """The same cells as a one-word hash table: occupied cells in random slots, the key word section after the value
    sections, -1 in empty slots."""
    keys = np.flatnonzero(t[0] > 0)
    slots = 64
    while slots < 2 * len(keys):
        slots <<= 1
    h = np.zeros((NSEC + 1, slots), dtype=np.int64)
    h[2], h[3], h[NSEC] = I64_MAX, I64_MIN, -1
    at = rng.permutation(slots)[: len(keys)]
    h[:NSEC, at] = t[:, keys]
    h[NSEC, at] = keys
    return h


def _mode_on_gpu(gpu_ctx, L, table, inner, values, ps=(), reducers=ALL):
    """pgpu_table_mode of a device table: (mode layout, device output, its host copy [sections][inner])."""
    lib = gpu_ctx._lib
    k = len(ps)
    F = TableLayout()
    _lib.check(lib.pgpu_mode_layout_of(C.byref(L), inner, k, reducers, C.byref(F)))
    nsec = NSEC + 1 + k + (5 if reducers & PGPU_MODE_AVG else 4)
    assert F.num_sections == nsec
    dev = torch.from_numpy(np.array(table).reshape(-1)).cuda()  # (a copy: the shared tables are read-only)
    dval = torch.from_numpy(np.array(values, dtype=np.float64)).cuda()
    out = torch.full((nsec * inner,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")  # (not the answers)
    nbytes = out.numel() * 8
    assert nbytes == _lib.table_bytes(F)
    pp = (C.c_double * max(k, 1))(*ps)
    args = (gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner, pp, k, reducers,
            C.c_void_p(dval.data_ptr()), len(values), C.c_void_p(out.data_ptr()))
    assert lib.pgpu_table_mode(*args, nbytes - 8) == _lib.PGPU_E_INVALID  # too small: refused, nothing enqueued
    _lib.check(lib.pgpu_table_mode(*args, nbytes))
    torch.cuda.synchronize()
    return F, out, out.cpu().numpy().reshape(nsec, inner)


def _fold_on_gpu(gpu_ctx, L, table, inner):
    dev = torch.from_numpy(np.array(table).reshape(-1)).cuda()
    folded = torch.full(((NSEC + 1) * inner,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    _lib.check(gpu_ctx._lib.pgpu_table_fold(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner,
                                            C.c_void_p(folded.data_ptr()), folded.numel() * 8))
    torch.cuda.synchronize()
    return folded.cpu().numpy().reshape(NSEC + 1, inner)


def _check_mode(gpu_ctx, rng, t, inner, kind, values):
    """pgpu_table_mode with every reducer against numpy, every section exactly.  Returns (layout, device output, the
    expected table)."""
    fold, M, T, LO, HI, S = _np_mode(t, inner, values)
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(rng, t)
    L = _table_layout(table.shape[1], kind)
    F, out, got = _mode_on_gpu(gpu_ctx, L, table, inner, values)
    # the folded sections: pgpu_table_fold's output bit for bit, and numpy's
    assert np.array_equal(got[: NSEC + 1], _fold_on_gpu(gpu_ctx, L, table, inner)) and np.array_equal(got[: NSEC + 1], fold)
    for name, sec, want in (("M", 0, M), ("T", 1, T), ("LO", 2, LO), ("HI", 3, HI)):
        assert np.array_equal(got[NSEC + 1 + sec], want), (name, int((got[NSEC + 1 + sec] != want).sum()))
    assert np.array_equal(got[NSEC + 5].view(np.float64), S)  # sums of integers below 2^53: exact in any order
    assert list(F.section_op)[NSEC + 1: NSEC + 6] == [PGPU_RED_SUM_I64] * 4 + [PGPU_RED_SUM_F64]
    want = np.concatenate([fold, np.stack([M, T, LO, HI, S.view(np.int64)])])
    return F, out, want


def _compact(gpu_ctx, F, out, order=None):
    lib = gpu_ctx._lib
    cap = int(F.num_keys)
    keys = np.empty(cap, dtype=np.int64)
    cells = np.empty((cap, F.num_sections), dtype=np.int64)
    n = C.c_uint64()
    kp, cp = keys.ctypes.data_as(C.POINTER(C.c_int64)), cells.ctypes.data_as(C.POINTER(C.c_int64))
    if order is None:
        _lib.check(lib.pgpu_table_compact(gpu_ctx.handle, C.byref(F), C.c_void_p(out.data_ptr()), None, kp, cp, cap,
                                          C.byref(n)))
    else:
        _lib.check(lib.pgpu_table_topk(gpu_ctx.handle, C.byref(F), C.c_void_p(out.data_ptr()), None, C.byref(order),
                                       kp, cp, cap, C.byref(n)))
    return keys[: n.value], cells[: n.value]


# a single cell; a wave boundary either side (a wave per key walks 64 cid a step); many chunks on the wave-per-key
# path with a tail; both lane orientations (inner below and from 64); lanes along g with cid chunks of one; the chunk
# tuples merged by a wave per key (inner below 4,096) and by a thread per key ((5000, 33), (70001, 3))
MODE_SHAPES = [(1, 1), (1, 63), (1, 65), (1, 70001), (3, 5), (64, 257), (257, 64), (5000, 33), (70001, 3)]


@functools.lru_cache(maxsize=None)
def _shape_table(inner, card):
    """One table and value list per shape, shared by the dense and the hash case (and left unchanged)."""
    rng = np.random.default_rng(inner * 1000003 + card)
    t = _fill(rng, _random_counts(rng, inner, card))
    v = _values(rng, card)
    t.setflags(write=False)
    v.setflags(write=False)
    return t, v


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card", MODE_SHAPES, ids=[f"{i}x{c}" for i, c in MODE_SHAPES])
def test_table_mode_against_numpy(gpu_ctx, inner, card, kind):
    t, values = _shape_table(inner, card)
    F, out, want = _check_mode(gpu_ctx, np.random.default_rng(card), t, inner, kind, values)
    M, T, LO, HI = want[NSEC + 1: NSEC + 5]
    if inner >= 3:  # the empty key holds 0 in all five cells
        assert not want[NSEC + 1:, 0].any() and want[0, 0] == 0
    if card > 100:
        assert (T > 1).any()  # some key has several modes, or the tie handling is not looked at
    # compaction of the mode table: the non-empty keys in order, cells row-major
    live = np.flatnonzero(want[0] > 0)
    keys, cells = _compact(gpu_ctx, F, out)
    assert np.array_equal(keys, live) and np.array_equal(cells, want[:, live].T)
    # top 3 by HI (aggregation entry n + 2, a LONG SUM), ties with the third kept; LO is the entry before it
    order = _lib.TopK()
    order.source, order.agg_fn, order.descending, order.k = _lib.PGPU_TOPK_AGG, _lib.PGPU_AGG_SUM, 1, 3
    order.agg_index = 4 + 1 + 1
    assert F.agg_section[order.agg_index] == NSEC + 4 and F.agg_section[order.agg_index - 1] == NSEC + 3
    v = HI[live]
    keep = live if len(live) <= 3 else live[v >= np.sort(v)[-3]]
    keys, cells = _compact(gpu_ctx, F, out, order)
    by = np.argsort(keys)
    assert np.array_equal(keys[by], keep) and np.array_equal(cells[by], want[:, keep].T)


def _targeted(case, rng, inner, card):
    """Count matrix [card, inner] of one targeted case and what it is to show as (key, M, T, LO, HI) rows."""
    c = rng.integers(1, 100, (card, inner)).astype(np.int64)
    if case == "all-tied":
        c[:] = 5
        return c, [(g, 5, card, 0, card - 1) for g in (0, inner - 1)]
    if case == "last-cid":
        c[card - 1] = 1000
        return c, [(g, 1000, 1, card - 1, card - 1) for g in (0, inner - 1)]
    if case == "ties-across-chunks":
        # a wave per key takes 1,024 cid in chunks of 256, lanes along g in chunks of one: 255 | 256 are adjacent cells
        # either side of a chunk boundary on both, 100 and 900 lie in different chunks
        c[[255, 256], 0] = 500
        c[[100, 900], inner - 1] = 500
        return c, [(0, 500, 2, 255, 256), (inner - 1, 500, 2, 100, 900)]
    if case == "beyond-32-bits":
        # compared by their low words 2^40 is 0 and 2^40 + 1 is 1: every other count of the key would beat them
        c[300, 0], c[700, 0] = (1 << 40) + 1, 1 << 40
        c[[10, 20], inner - 1] = 1 << 40
        c[1000, inner - 1] = (1 << 40) - 1
        return c, [(0, (1 << 40) + 1, 1, 300, 300), (inner - 1, 1 << 40, 2, 10, 20)]
    if case == "empty-keys":
        c[:, 0::2] = 0  # every even key has no count at all, every odd one a count in every cell
        return c, [(0, 0, 0, 0, 0)]
    if case == "count-one":
        c[:] = 0
        c[[3, 511, 512, card - 1], 0] = 1
        c[77, inner - 1] = 1
        return c, [(0, 1, 4, 3, card - 1), (inner - 1, 1, 1, 77, 77)]
    raise ValueError(case)


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner", [2, 70], ids=["wave-per-key", "lanes-along-g"])
@pytest.mark.parametrize("case", ["all-tied", "last-cid", "ties-across-chunks", "beyond-32-bits", "empty-keys",
                                  "count-one"])
def test_table_mode_targeted(gpu_ctx, case, inner, kind):
    card = 1024
    rng = np.random.default_rng(inner + len(case))
    c, rows = _targeted(case, rng, inner, card)
    values = _values(rng, card)
    _, _, want = _check_mode(gpu_ctx, rng, _fill(rng, c.reshape(-1)), inner, kind, values)
    for g, m, t, lo, hi in rows:  # numpy agrees with the case's intent (the device agrees with numpy: _check_mode)
        assert want[NSEC + 1: NSEC + 5, g].tolist() == [m, t, lo, hi], (case, g)


@pytest.mark.parametrize("inner", [1, 70], ids=["wave-per-key", "lanes-along-g"])
def test_table_mode_single_chunk_and_one_key_orientations(gpu_ctx, inner):
    """inner = 1 (aggregation only) on the wave-per-key path with one chunk (card 200 < 256) and with several, and
    every cell tied on both orientations with T = card."""
    for card in (200, 3000):
        rng = np.random.default_rng(card + inner)
        c = np.full((card, inner), 9, dtype=np.int64)
        _, _, want = _check_mode(gpu_ctx, rng, _fill(rng, c.reshape(-1)), inner, PGPU_KEYS_DENSE, _values(rng, card))
        assert want[NSEC + 1: NSEC + 5, 0].tolist() == [9, card, 0, card - 1]
    if inner >= 64:  # lanes along g write the output directly only when cid is not cut at all: one cid
        rng = np.random.default_rng(inner)
        _check_mode(gpu_ctx, rng, _fill(rng, rng.integers(0, 3, 300)), 300, PGPU_KEYS_DENSE, _values(rng, 1))


@pytest.mark.parametrize("inner,card", [(1, 70001), (70, 300), (5000, 33)], ids=["wave-per-key", "lanes-along-g", "by-thread"])
def test_table_mode_dense_sum_of_doubles_is_bounded_and_reproducible(gpu_ctx, inner, card):
    """Non-integer values on dense input: S is within the bound of its T - 1 rounded adds of the exact sum,
    |S - fsum| <= (T - 1) 2^-53 sum|v|, and two runs give the same bits (one writer per cell, a fixed order of adds)."""
    rng = np.random.default_rng(card)
    c = np.where(rng.random((card, inner)) < 0.7, 3, rng.integers(0, 3, (card, inner))).astype(np.int64)  # most cells tied
    values = np.sort(rng.normal(0.0, 1e6, card))
    t = _fill(rng, c.reshape(-1))
    _, M, T, LO, HI, S = _np_mode(t, inner, values)
    L = _table_layout(t.shape[1], PGPU_KEYS_DENSE)
    runs = [_mode_on_gpu(gpu_ctx, L, t, inner, values)[2] for _ in range(2)]
    assert np.array_equal(runs[0], runs[1])
    got = runs[0]
    assert np.array_equal(got[NSEC + 1: NSEC + 5], np.stack([M, T, LO, HI])) and T.max() > card // 2
    tied = (c == M) & (c > 0)
    bound = np.maximum(T - 1, 0) * 2.0 ** -53 * np.array([math.fsum(np.abs(values[tied[:, g]])) for g in range(inner)])
    err = np.abs(got[NSEC + 5].view(np.float64) - S)
    print("largest |S - fsum| / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
    assert (err <= bound).all()


@pytest.mark.parametrize("kind", [PGPU_KEYS_DENSE, PGPU_KEYS_HASH], ids=["dense", "hash"])
@pytest.mark.parametrize("inner,card", [(1, 70001), (257, 64)], ids=["1x70001", "257x64"])
def test_table_mode_with_percentiles_equals_table_select(gpu_ctx, inner, card, kind):
    t, values = _shape_table(inner, card)
    rng = np.random.default_rng(card)
    table = t if kind == PGPU_KEYS_DENSE else _to_hash(rng, t)
    L = _table_layout(table.shape[1], kind)
    lib = gpu_ctx._lib
    k = len(PS)
    dev = torch.from_numpy(np.array(table).reshape(-1)).cuda()
    sel = torch.full(((NSEC + 1 + k) * inner,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    pp = (C.c_double * k)(*PS)
    _lib.check(lib.pgpu_table_select(gpu_ctx.handle, C.byref(L), C.c_void_p(dev.data_ptr()), None, inner, pp, k,
                                     C.c_void_p(sel.data_ptr()), sel.numel() * 8))
    torch.cuda.synchronize()
    sel = sel.cpu().numpy().reshape(NSEC + 1 + k, inner)
    _, M, T, LO, HI, S = _np_mode(t, inner, values)
    for reducers in (ALL, PGPU_MODE_MAX):
        F, _, got = _mode_on_gpu(gpu_ctx, L, table, inner, values, PS, reducers)
        assert np.array_equal(got[: NSEC + 1 + k], sel)  # the selected sections bit for bit
        assert np.array_equal(got[NSEC + 1 + k: NSEC + 5 + k], np.stack([M, T, LO, HI]))
        if reducers & PGPU_MODE_AVG:
            assert np.array_equal(got[NSEC + 5 + k].view(np.float64), S)
        # the entries: 4 of the table, the distinct count, the percentiles, then LO and HI
        assert (F.agg_section[5 + k], F.agg_section[6 + k]) == (NSEC + 3 + k, NSEC + 4 + k)


def test_table_mode_refusals(gpu_ctx):
    lib = gpu_ctx._lib
    L = _table_layout(6, PGPU_KEYS_DENSE)
    dev = torch.zeros(NSEC * 6, dtype=torch.int64, device="cuda")
    dval = torch.zeros(2, dtype=torch.float64, device="cuda")
    out = torch.zeros((NSEC + 1 + 5) * 3, dtype=torch.int64, device="cuda")

    def call(layout, reducers, values, nv):
        return lib.pgpu_table_mode(gpu_ctx.handle, C.byref(layout), C.c_void_p(dev.data_ptr()), None, 3, None, 0,
                                   reducers, values, nv, C.c_void_p(out.data_ptr()), out.numel() * 8)
    vp = C.c_void_p(dval.data_ptr())
    for reducers in (0, 8, 15, -1):
        assert call(L, reducers, vp, 2) == _lib.PGPU_E_INVALID and "reducers" in _lib.last_error()
    for reducers in (PGPU_MODE_AVG, ALL):  # the AVG bit needs the values
        assert call(L, reducers, None, 2) == _lib.PGPU_E_INVALID and "values" in _lib.last_error()
        assert call(L, reducers, vp, 0) == _lib.PGPU_E_INVALID
    H = _table_layout(64, PGPU_KEYS_HASH)
    H.key_words = 2
    assert call(H, PGPU_MODE_MIN, None, 0) == _lib.PGPU_E_UNSUPPORTED and "two key words" in _lib.last_error()
    # without the AVG bit no values are needed
    _lib.check(call(L, PGPU_MODE_MIN | PGPU_MODE_MAX, None, 0))
    torch.cuda.synchronize()
    assert not out.cpu().numpy()[: (NSEC + 1 + 4) * 3].reshape(-1, 3)[NSEC + 1:].any()  # an all-empty table: zeros


# ---- 2. end to end on three segments whose dictionaries overlap only partly ---------------------------------------------
NDOCS = 20_000
C_COLUMNS = ["c_int", "c_long", "c_float", "c_double", "c_raw"]
# planted (g, c, docs per segment): values no random doc has, so their counts are exactly these -- g = 5 has one mode,
# g = 16 two and g = 27 three, each spread over the segments so that no segment's own counts give the answer
PLANTED = [(5, 5000, (10, 25, 5)), (16, 5001, (15, 0, 25)), (16, 5003, (20, 20, 0)),
           (27, 5000, (0, 30, 10)), (27, 5002, (40, 0, 0)), (27, 5004, (13, 13, 14))]


def _columns(rng, i):
    """Segment i: the mode columns' values come from [800 i, 800 i + 1400), so the three dictionaries overlap in part
    and the global one has about 3,000 entries, plus the planted docs (f = 0: every filter here keeps them).  Every
    typed column is an increasing function of c whose values and sums are exact in double.  `u` has 6,000 values
    (more groups than the server trim keeps) and `v` up to 50 values whose spread depends on u: a group's handful of docs
    mostly tie at one doc per value, and the largest mode differs from group to group."""
    c = rng.integers(800 * i, 800 * i + 1400, NDOCS).astype(np.int64)
    g = rng.integers(0, 7, NDOCS).astype(np.int32) * 11 + 5
    u = rng.integers(0, 6000, NDOCS).astype(np.int32)
    f = rng.integers(0, 100, NDOCS).astype(np.int32)
    at = 0
    for pg, pc, per in PLANTED:
        g[at: at + per[i]], c[at: at + per[i]], f[at: at + per[i]] = pg, pc, 0
        at += per[i]
    return {"g": (PGPU_INT, g), "f": (PGPU_INT, f), "f2": (PGPU_INT, (f == 0).astype(np.int32)),
            "x": (PGPU_INT, rng.integers(-50_000, 50_000, NDOCS).astype(np.int32)),
            "y": (PGPU_DOUBLE, np.round(rng.normal(0, 1000, NDOCS), 3)),
            "u": (PGPU_INT, u), "v": (PGPU_INT, (rng.integers(0, 1 << 30, NDOCS) % (1 + u % 50)).astype(np.int32) * 3),
            "c_int": (PGPU_INT, (c * 3 - 1000).astype(np.int32)), "c_long": (PGPU_LONG, c * (1 << 33) - 7),
            "c_float": (PGPU_FLOAT, (c.astype(np.float32) * np.float32(0.25)) - np.float32(100)),
            "c_double": (PGPU_DOUBLE, c.astype(np.float64) * 0.125 + 1.0),
            "c_str": (PGPU_STRING, [f"v{v:05d}" for v in c]), "c_raw": (PGPU_INT, (c * 5 + 1).astype(np.int32))}


@pytest.fixture(scope="module")
def three(gpu_ctx):
    rng = np.random.default_rng(20261021)
    cols = [_columns(rng, i) for i in range(3)]
    segs = [build_segment(f"m{i}", c, raw=["c_raw"]) for i, c in enumerate(cols)]
    gs = [GpuSegment(gpu_ctx, s) for s in segs]
    host = {k: np.concatenate([np.asarray(c[k][1]) for c in cols]) for k in cols[0] if k != "c_str"}
    yield gs, host
    for g in gs:
        g.release()


def _modes(values):
    """The tied values of ModeAggregationFunction's map: those of the largest count."""
    vals, counts = np.unique(values, return_counts=True)
    return vals[counts == counts.max()]


def _mode(values, reducer):
    """ModeAggregationFunction.java:463-672 over the collected values: min / max / mean of the modes as doubles."""
    if len(values) == 0:
        return -math.inf
    tied = [float(v) for v in _modes(values)]
    return {"MIN": min(tied), "MAX": max(tied), "AVG": math.fsum(tied) / len(tied)}[reducer]


def _mode_by(host, col, mask, by, reducer):
    return {int(k): _mode(host[col][mask & (host[by] == k)], reducer) for k in np.unique(host[by][mask])}


def _run(pm, q, gs):
    """submit + collect, returning the result and the layout of every pass's GROUP BY g, c launch."""
    pending = pm.submit(q, gs)
    layouts = [pq.layout for pq in pending.pending]
    return pm.collect(pending), layouts


def test_the_data_holds_one_two_and_three_modes(three):
    _, host = three
    for mask in (np.ones(len(host["f"]), dtype=bool), host["f"] < 30):
        n = {int(k): len(_modes(host["c_int"][mask & (host["g"] == k)])) for k in np.unique(host["g"])}
        assert (n[5], n[16], n[27]) == (1, 2, 3), n
        assert len(_modes(host["c_int"][mask])) == 1  # aggregation only: 5000, planted in two groups


MIX = "SUM(x), MIN(x), MAX(y), AVG(y), COUNT(*)"


@pytest.mark.parametrize("where", ["", " WHERE f < 30"], ids=["all", "filter"])
@pytest.mark.parametrize("grouped", [False, True], ids=["agg", "group"])
def test_end_to_end_reducers_beside_plain_aggregations(gpu_ctx, three, grouped, where):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30 if where else np.ones(len(host["f"]), dtype=bool)
    tail = " GROUP BY g LIMIT 100" if grouped else ""
    head = SEL + ("g, " if grouped else "")
    q = parse_sql(f"{head}SUM(x), MODE(c_int), MIN(x), MAX(y), MODE(c_int, 'MAX'), AVG(y), COUNT(*), "
                  f"MODE(c_int, 'AVG'), MODE(c_int, 'MIN') FROM t{where}{tail}")
    res, layouts = _run(pm, q, gs)
    assert len(layouts) == 1 and layouts[0].key_kind == PGPU_KEYS_DENSE  # one pass: 7 x ~3,000 keys
    plain = pm.execute(parse_sql(f"{head}{MIX} FROM t{where}{tail}"), gs)
    modes = {1: "MIN", 4: "MAX", 7: "AVG", 8: "MIN"}  # aggregation index -> reducer
    keep = [0, 2, 3, 5, 6]
    ng = int(grouped)
    if grouped:
        for ai, r in modes.items():
            assert {row[0]: row[1 + ai] for row in res.group_rows} == _mode_by(host, "c_int", mask, "g", r), r
        by_g = {row[0]: row for row in res.group_rows}
        assert by_g[16][2] < by_g[16][8] < by_g[16][5] and by_g[5][2] == by_g[5][5] == by_g[5][8]  # two modes / one
        # the other columns are exactly those of the query without the modes
        assert [row[:1] + tuple(row[1 + i] for i in keep) for row in res.group_rows] == plain.group_rows
        assert [row[:1] + tuple(row[1 + i] for i in keep) for row in res.rows] == plain.rows
        assert all(type(row[1 + ai]) is float for row in res.group_rows for ai in modes)
    else:
        for ai, r in modes.items():
            assert res.aggregation_result[ai] == _mode(host["c_int"][mask], r)
            assert type(res.aggregation_result[ai]) is float
        assert [res.aggregation_result[i] for i in keep] == plain.aggregation_result
    st = res.stats
    assert st.num_docs_scanned == int(mask.sum()) == plain.stats.num_docs_scanned and st.num_total_docs == 3 * NDOCS
    assert st.num_entries_scanned_post_filter == st.num_docs_scanned * len(q.projected_columns)
    assert len(q.projected_columns) == 3 + ng  # x, c_int, y (and g): the mode column included
    assert st.num_entries_scanned_in_filter == plain.stats.num_entries_scanned_in_filter
    with pytest.raises(UnsupportedPlanError):
        res.intermediate


@pytest.mark.parametrize("col", C_COLUMNS)
def test_end_to_end_column_types(gpu_ctx, three, col):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    mask = host["f"] < 30
    res = pm.execute(parse_sql(SEL + f"g, MODE({col}), MODE({col}, 'MAX'), MODE({col}, 'AVG'), COUNT(*) FROM t "
                               "WHERE f < 30 GROUP BY g LIMIT 100"), gs)
    for j, r in enumerate(("MIN", "MAX", "AVG")):
        assert {row[0]: row[1 + j] for row in res.group_rows} == _mode_by(host, col, mask, "g", r), r
    assert {row[0]: row[4] for row in res.group_rows} == {int(k): int((mask & (host["g"] == k)).sum())
                                                          for k in np.unique(host["g"])}
    res = pm.execute(parse_sql(SEL + f"MODE({col}, 'AVG'), MODE({col}) FROM t"), gs)  # (never a non-scan plan)
    assert res.aggregation_result == [_mode(host[col], "AVG"), _mode(host[col], "MIN")]
    assert res.stats.num_entries_scanned_post_filter == res.stats.num_docs_scanned == 3 * NDOCS


def test_string_column_raises_before_any_launch(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    with pytest.raises(UnsupportedPlanError, match="MODE over the STRING column 'c_str'"):
        pm.submit(parse_sql(SEL + "MODE(c_str) FROM t"), gs)
    with pytest.raises(UnsupportedPlanError, match="MODE over the STRING column 'c_str'"):
        pm.execute(parse_sql(SEL + "g, SUM(x), MODE(c_str, 'MAX') FROM t GROUP BY g"), gs)


def test_beside_distinctcount_and_percentiles_of_the_same_and_another_column(gpu_ctx, three):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    tail = " FROM t WHERE f < 60 GROUP BY g LIMIT 100"
    both, layouts = _run(pm, parse_sql(SEL + "g, PERCENTILE50(c_int), MODE(c_int, 'AVG'), DISTINCTCOUNT(c_int), "
                                       "PERCENTILE90(c_long), MODE(c_long, 'MAX'), PERCENTILE99(c_int), "
                                       "DISTINCTCOUNT(c_double)" + tail), gs)
    assert len(layouts) == 3  # c_int (two picks, the distinct count and the mode in one table), c_long, c_double
    dc = pm.execute(parse_sql(SEL + "g, DISTINCTCOUNT(c_int), DISTINCTCOUNT(c_double)" + tail), gs)
    pc = pm.execute(parse_sql(SEL + "g, PERCENTILE50(c_int), PERCENTILE99(c_int), PERCENTILE90(c_long)" + tail), gs)
    assert [(r[0], r[3], r[7]) for r in both.group_rows] == dc.group_rows
    assert [(r[0], r[1], r[6], r[4]) for r in both.group_rows] == pc.group_rows
    mask = host["f"] < 60
    assert {r[0]: r[2] for r in both.group_rows} == _mode_by(host, "c_int", mask, "g", "AVG")
    assert {r[0]: r[5] for r in both.group_rows} == _mode_by(host, "c_long", mask, "g", "MAX")
    assert both.stats.num_entries_scanned_post_filter == both.stats.num_docs_scanned * 4  # c_int, c_long, c_double, g


def test_filter_matching_nothing(gpu_ctx, three):
    gs, _ = three
    pm = GpuPlanMaker(gpu_ctx)
    for where in ("f = 0 AND f2 = 0", "f > 1000"):  # empty at run time / folded to EMPTY at plan time
        res = pm.execute(parse_sql(SEL + f"MODE(c_int) FROM t WHERE {where}"), gs)
        assert res.aggregation_result == [-math.inf] and res.stats.num_docs_scanned == 0
        res = pm.execute(parse_sql(SEL + f"COUNT(*), MODE(c_int, 'AVG'), MODE(c_double, 'MAX'), PERCENTILE50(c_int) "
                                         f"FROM t WHERE {where}"), gs)
        assert res.aggregation_result == [0, -math.inf, -math.inf, -math.inf]
        res = pm.execute(parse_sql(SEL + f"g, MODE(c_int, 'AVG'), SUM(x) FROM t WHERE {where} GROUP BY g"), gs)
        assert res.rows == [] and res.group_rows == []


def test_forced_hash_path(gpu_ctx, three):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx, query_flags=PGPU_Q_HASH)
    q = parse_sql(SEL + "g, MODE(c_int), SUM(x), MODE(c_int, 'AVG'), MODE(c_int, 'MAX'), PERCENTILE50(c_int) FROM t "
                  "WHERE f < 30 GROUP BY g LIMIT 100")
    res, layouts = _run(pm, q, gs)
    assert layouts[0].key_kind == PGPU_KEYS_HASH
    mask = host["f"] < 30
    for col, r in ((1, "MIN"), (3, "AVG"), (4, "MAX")):
        assert {row[0]: row[col] for row in res.group_rows} == _mode_by(host, "c_int", mask, "g", r), r
    assert [(r[0], r[2], r[5]) for r in res.group_rows] == GpuPlanMaker(gpu_ctx).execute(
        parse_sql(SEL + "g, SUM(x), PERCENTILE50(c_int) FROM t WHERE f < 30 GROUP BY g LIMIT 100"), gs).group_rows


def _pct(values, p):
    """PercentileAggregationFunction.java:152-165 over the collected values (p < 100)."""
    s = np.sort(values)
    return float(s[int(float(len(s)) * p / 100.0)])


def _avg_bound(values):
    """test_table_mode_dense_sum_of_doubles_is_bounded_and_reproducible's bound on S, (T - 1) 2^-53 sum|v| over the T
    tied values, carried to the reducer's S / T.  (c_int's values and their sums are integers exact in double, so S / T
    is the same division on both sides and the bound covers the adds alone.)"""
    tied = _modes(values).astype(np.float64)
    return (len(tied) - 1) * 2.0 ** -53 * math.fsum(np.abs(tied)) / len(tied)


@pytest.mark.parametrize("hashed", [False, True], ids=["dense", "hash"])
@pytest.mark.parametrize("grouped", [False, True], ids=["agg", "group"])
def test_selection_and_mode_reduction_share_the_collect_temporary(gpu_ctx, three, grouped, hashed):
    """The selection and the mode reduction of one collect take their temporaries from one workspace buffer, one after
    the other on the stream.  Aggregation only (inner = 1) and GROUP BY g (inner = 7) cut the ~3,000 ids into several
    chunks, so on dense input both stages use it (chunk prefixes, then chunk tuples); on hash input the selection's
    sort buffers fill it and the mode reduction needs none.  Twice on one plan maker: the second collect meets what
    the first left in the buffer."""
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx, query_flags=PGPU_Q_HASH) if hashed else GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + ("g, " if grouped else "") + "DISTINCTCOUNT(c_int), PERCENTILE(c_int, 50), "
                  "PERCENTILE(c_int, 99), MODE(c_int), MODE(c_int, 'AVG') FROM t" +
                  (" GROUP BY g LIMIT 100" if grouped else ""))
    c = host["c_int"]
    groups = {int(k): c[host["g"] == k] for k in np.unique(host["g"])} if grouped else {None: c}
    exact = {k: (len(np.unique(v)), _pct(v, 50), _pct(v, 99), _mode(v, "MIN")) for k, v in groups.items()}
    for _ in range(2):
        res, layouts = _run(pm, q, gs)
        assert len(layouts) == 1 and layouts[0].key_kind == (PGPU_KEYS_HASH if hashed else PGPU_KEYS_DENSE)
        rows = {r[0]: r[1:] for r in res.group_rows} if grouped else {None: tuple(res.aggregation_result)}
        assert {k: r[:4] for k, r in rows.items()} == exact
        for k, v in groups.items():
            assert abs(rows[k][4] - _mode(v, "AVG")) <= _avg_bound(v), k


# ---- 3. the large key paths -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(gpu_ctx):
    rng = np.random.default_rng(7)
    n = 200_000
    # every value of 70,000 once, random ones on top (a handful of docs per value), and three values of their own with
    # 30 docs each that every filter here keeps (f = 0): the three modes of the whole column
    c = np.concatenate([np.arange(70_000), rng.integers(0, 70_000, n - 70_000 - 90),
                        np.repeat([70_000, 70_001, 70_002], 30)]).astype(np.int32)
    f = rng.integers(0, 100, n).astype(np.int32)
    f[-90:] = 0
    at = rng.permutation(n)
    cols = {"c": (PGPU_INT, c[at] * 2), "g": (PGPU_INT, rng.integers(0, 40, n).astype(np.int32)), "f": (PGPU_INT, f[at])}
    g = GpuSegment(gpu_ctx, build_segment("mwide", cols))
    yield g, {k: v[1] for k, v in cols.items()}
    g.release()


def test_partitioned_path(gpu_ctx, wide):
    g, host = wide
    res, layouts = _run(GpuPlanMaker(gpu_ctx), parse_sql(SEL + "MODE(c), MODE(c, 'MAX'), MODE(c, 'AVG') "
                                                         "FROM t WHERE f < 50"), [g])
    # 70,003 dense keys: from 65,536 keys up the group-by is partitioned; the reduction runs a wave per chunk of cid
    assert layouts[0].key_kind == PGPU_KEYS_DENSE and layouts[0].num_keys == 70_003
    assert res.stats.kernel_variant == _lib.PGPU_KV_PSCAN
    vals = host["c"][host["f"] < 50]
    assert _modes(vals).tolist() == [140_000, 140_002, 140_004]
    assert res.aggregation_result == [_mode(vals, "MIN"), _mode(vals, "MAX"), _mode(vals, "AVG")]


def test_hash_path_by_key_space(gpu_ctx, wide):
    g, host = wide
    res, layouts = _run(GpuPlanMaker(gpu_ctx), parse_sql(SEL + "g, MODE(c), MODE(c, 'MAX'), MODE(c, 'AVG'), COUNT(*) "
                                                         "FROM t WHERE f < 50 GROUP BY g LIMIT 100"), [g])
    assert layouts[0].key_kind == PGPU_KEYS_HASH  # 40 x 70,003 keys against 200,000 docs
    for j, r in enumerate(("MIN", "MAX", "AVG")):
        assert {row[0]: row[1 + j] for row in res.group_rows} == _mode_by(host, "c", host["f"] < 50, "g", r), r


# ---- 4. ORDER BY MODE ... LIMIT on more groups than the server trim keeps ---------------------------------------------------
def test_order_by_mode_trimmed_on_the_device(gpu_ctx, three):
    gs, host = three
    q = parse_sql(SEL + "u, MODE(v), MODE(v, 'MAX'), COUNT(*) FROM t WHERE f < 80 GROUP BY u "
                  "ORDER BY MODE(v, 'MAX') DESC, u LIMIT 20")
    mask = host["f"] < 80
    lo, hi = _mode_by(host, "v", mask, "u", "MIN"), _mode_by(host, "v", mask, "u", "MAX")
    cnt = {int(k): int((mask & (host["u"] == k)).sum()) for k in hi}
    full = sorted(((k, lo[k], hi[k], cnt[k]) for k in hi), key=lambda r: (-r[2], r[0]))
    assert len(full) > 5000 and any(r[1] != r[2] for r in full)  # (ordering by the first mode(v) would differ)
    res = GpuPlanMaker(gpu_ctx).execute(q, gs)  # the default trim: max(5 * 20, 5000) groups, ties with the last kept
    assert res.rows == full[:20]
    assert 5000 <= len(res.group_rows) < len(full) and set(res.group_rows) <= set(full)
    kept = min(r[2] for r in res.group_rows)
    assert all(r in set(res.group_rows) for r in full if r[2] >= kept)  # nothing at or above the cut is missing
    # ascending by the MIN reducer too, and with the trim off every group comes back
    q2 = parse_sql(SEL + "u, MODE(v), MODE(v, 'MAX'), COUNT(*) FROM t WHERE f < 80 GROUP BY u ORDER BY MODE(v), u LIMIT 20")
    assert GpuPlanMaker(gpu_ctx).execute(q2, gs).rows == sorted(full, key=lambda r: (r[1], r[0]))[:20]
    res = GpuPlanMaker(gpu_ctx, min_server_group_trim_size=-1).execute(q, gs)
    assert res.rows == full[:20] and sorted(res.group_rows, key=lambda r: (-r[2], r[0])) == full
    with pytest.raises(UnsupportedPlanError, match="AVG"):
        GpuPlanMaker(gpu_ctx).execute(parse_sql(SEL + "u, MODE(v, 'AVG') FROM t GROUP BY u ORDER BY MODE(v, 'AVG') LIMIT 5"), gs)


# ---- 5. cancel ----------------------------------------------------------------------------------------------------------------
def test_cancelled_pass_is_not_reduced_and_the_context_stays_usable(gpu_ctx, three):
    gs, host = three
    pm = GpuPlanMaker(gpu_ctx)
    q = parse_sql(SEL + "g, MODE(c_int, 'AVG'), SUM(x) FROM t WHERE f < 30 GROUP BY g LIMIT 100")
    full = pm.collect(pm.submit(q, gs))
    # at the C ABI: pgpu_query_collect_mode passes the wait's status through and releases the query
    pending = pm.submit(q, gs)
    pending.cancel()
    (pq,) = pending.pending
    inner, F = pq.fold.inner_keys, pq.fold.layout
    assert pq.fold.reducers == ALL and F.num_sections == pq.layout.num_sections + 1 + 5
    keys = (C.c_int64 * inner)()
    cells = (C.c_int64 * (inner * F.num_sections))()
    n = C.c_uint64()
    st = _lib.QueryStats()
    h, pq.handle = pq.handle, None
    vals = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    rc = gpu_ctx._lib.pgpu_query_collect_mode(h, inner, None, 0, ALL, vals, 4, None, keys, cells, inner, C.byref(n),
                                              C.byref(st), None)
    assert rc == _lib.PGPU_E_CANCELLED and "cancel" in _lib.last_error()
    # the Python surface raises
    pending = pm.submit(q, gs)
    pending.cancel()
    with pytest.raises(_lib.QueryCancelledError):
        pm.collect(pending)
    again = pm.collect(pm.submit(q, gs))
    assert again.group_rows == full.group_rows and again.stats.num_docs_scanned == full.stats.num_docs_scanned
    assert {r[0]: r[1] for r in again.group_rows} == _mode_by(host, "c_int", host["f"] < 30, "g", "AVG")
