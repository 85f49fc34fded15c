"""The HyperLogLog of DISTINCTCOUNTHLL on the host (pinot_amd/hll.py), CPU only.

Held against: the register words and byte sizes the reference's tests assert (DistinctCountQueriesTest.java:291-350),
its estimate bounds (:296,380), a scalar second implementation written here from the published algorithm in plain
Python integers, a hand-built byte layout, and a file of (value, hash) pairs that pins this restatement."""
import json
import math
import os
import struct

import numpy as np
import pytest

from pinot_amd import hll
from pinot_amd._lib import PGPU_DOUBLE, PGPU_FLOAT, PGPU_INT, PGPU_LONG, PGPU_STRING, UnsupportedPlanError

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hll_kat.json")
M32 = 0xFFFFFFFF
MUL = 0x5BD1E995


# ---- the second implementation: scalar, Python integers, every step masked to 32 bits ------------------------------
def ref_hash_long(x: int) -> int:
    x &= (1 << 64) - 1
    h = 0
    k = ((x & M32) * MUL) & M32
    k ^= k >> 24
    h ^= (k * MUL) & M32
    k = ((x >> 32) * MUL) & M32
    k ^= k >> 24
    h = (h * MUL) & M32
    h ^= (k * MUL) & M32
    h ^= h >> 13
    h = (h * MUL) & M32
    h ^= h >> 15
    return h


def ref_hash_bytes(data: bytes) -> int:
    n = len(data)
    h = (M32 ^ n) & M32  # seed -1
    n4 = n >> 2
    for i in range(n4):
        k = data[4 * i] | data[4 * i + 1] << 8 | data[4 * i + 2] << 16 | data[4 * i + 3] << 24
        k = (k * MUL) & M32
        k ^= k >> 24
        k = (k * MUL) & M32
        h = (h * MUL) & M32
        h ^= k
    left = n - 4 * n4
    if left:
        def sbyte(b):  # a Java byte cast to int
            return (b - 256 if b >= 128 else b) & M32
        if left >= 3:
            h ^= (sbyte(data[n - left + 2]) << 16) & M32
        if left >= 2:
            h ^= (sbyte(data[n - left + 1]) << 8) & M32
        h ^= sbyte(data[n - left])
        h = (h * MUL) & M32
    h ^= h >> 13
    h = (h * MUL) & M32
    h ^= h >> 15
    return h


def ref_hash(v, stored_type: int) -> int:
    if stored_type == PGPU_STRING:
        return ref_hash_bytes(v.encode("utf-8"))
    if stored_type in (PGPU_INT, PGPU_LONG):
        return ref_hash_long(int(v))
    if stored_type == PGPU_FLOAT:
        return ref_hash_long(struct.unpack("<i", struct.pack("<f", v))[0])
    return ref_hash_long(struct.unpack("<q", struct.pack("<d", v))[0])


def ref_offer(h: int, log2m: int):
    j = h >> (32 - log2m)
    w = ((h << log2m) & M32) | ((1 << (log2m - 1)) + 1)
    return j, (32 - w.bit_length()) + 1


def ref_words(log2m: int) -> int:
    b = (1 << log2m) // 6
    return 1 if b == 0 else (b if b % 32 == 0 else b + 1)


def ref_sketch(values, stored_type, log2m):
    words = [0] * ref_words(log2m)
    for v in values:
        j, r = ref_offer(ref_hash(v, stored_type), log2m)
        w, sh = j // 6, 5 * (j % 6)
        if (words[w] >> sh) & 31 < r:
            words[w] = (words[w] & ~(31 << sh)) | (r << sh)
    return words


def ref_cardinality(words, log2m):
    m = 1 << log2m
    regs = [(words[p // 6] >> (5 * (p % 6))) & 31 for p in range(m)]
    total = sum(2.0 ** -r for r in regs)
    zeros = regs.count(0)
    a = {4: 0.673, 5: 0.697, 6: 0.709}.get(log2m, 0.7213 / (1 + 1.079 / m))
    e = a * m * m / total
    return math.floor(m * math.log(m / zeros) + 0.5) if e <= 2.5 * m else math.floor(e + 0.5)


F32 = lambda x: float(np.float32(x))  # noqa: E731
CASES = {
    PGPU_INT: [0, 1, -1, 7, 123456789, -123456789, 2**31 - 1, -2**31],
    PGPU_LONG: [0, 1, -1, 2**32, 2**32 + 1, 2**40 + 12345, -2**32 - 7, 2**63 - 1, -2**63],
    PGPU_FLOAT: [0.0, -0.0, F32(1.5), F32(-1.5), F32(3.4e38), F32(-1e-30), float("inf")],
    PGPU_DOUBLE: [0.0, -0.0, 1.5, -1.5, 1e300, float("nan"), float("-inf")],
    # lengths 0..9; bytes >= 0x80 (two- and three-byte UTF-8 sequences) in each of the three tail positions
    PGPU_STRING: ["", "a", "ab", "abc", "abcd", "abcde", "abcdef", "abcdefg", "abcdefgh", "abcdefghi",
                  "abcdé", "abcdeé", "abcd€", "é", "aé", "€", "abcdéz",
                  "abcdefghé", "ééééé", "abcé"],
}
NP_TYPE = {PGPU_INT: np.int32, PGPU_LONG: np.int64, PGPU_FLOAT: np.float32, PGPU_DOUBLE: np.float64}


def _array(values, stored_type):
    return list(values) if stored_type == PGPU_STRING else np.array(values, dtype=NP_TYPE[stored_type])


def test_string_cases_cover_every_tail_position_with_a_high_byte():
    seen = set()
    for s in CASES[PGPU_STRING]:
        b = s.encode("utf-8")
        tail = b[len(b) - len(b) % 4:]
        seen |= {(len(tail), k) for k, x in enumerate(tail) if x >= 0x80}
    assert {(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)} <= seen
    assert {len(s.encode("utf-8")) for s in CASES[PGPU_STRING]} >= set(range(10))


@pytest.mark.parametrize("log2m,words,nbytes", [(4, 3, 12), (8, 43, 172), (12, 683, 2732), (16, 10923, 43692)])
def test_words_and_byte_length(log2m, words, nbytes):
    """172 and 2,732 are the reference's own sizeof() asserts (DistinctCountQueriesTest.java:291-350)."""
    assert hll.num_words(log2m) == words == ref_words(log2m)
    s = hll.HyperLogLog.empty(log2m)
    assert len(s.words) == words and 4 * words == nbytes
    b = s.to_bytes()
    assert len(b) == 8 + nbytes and struct.unpack(">ii", b[:8]) == (log2m, nbytes)
    assert s.cardinality() == 0


def test_byte_layout_of_a_hand_built_sketch():
    """Registers 0, 5, 6 and 255 of a log2m = 8 sketch: words 0 (bits 0 and 25), 1 (bit 0) and 42 (bit 15)."""
    regs = np.zeros(256, dtype=np.uint32)
    regs[0], regs[5], regs[6], regs[255] = 3, 31, 1, 17
    s = hll.HyperLogLog(8, hll.pack_registers(regs, 8))
    want = [0] * 43
    want[0] = 3 | 31 << 25
    want[1] = 1
    want[42] = 17 << 15  # 255 = 6 * 42 + 3
    assert s.words.tolist() == want
    assert s.to_bytes() == struct.pack(">ii", 8, 172) + b"".join(struct.pack(">I", w) for w in want)
    back = hll.HyperLogLog.from_bytes(s.to_bytes())
    assert back == s and back.registers().tolist() == regs.tolist()
    with pytest.raises(ValueError):
        hll.HyperLogLog.from_bytes(struct.pack(">ii", 8, 168) + bytes(168))


@pytest.mark.parametrize("stored_type", list(CASES), ids=["int", "long", "float", "double", "string"])
def test_agrees_with_the_scalar_implementation(stored_type):
    values = CASES[stored_type]
    arr = _array(values, stored_type)
    want = [ref_hash(v, stored_type) for v in values]
    assert hll.hash_values(arr, stored_type).tolist() == want
    for log2m in (4, 8, 12, 16):
        j, r = hll.offers(np.array(want, dtype=np.uint32), log2m)
        assert list(zip(j.tolist(), r.tolist())) == [ref_offer(h, log2m) for h in want]
        assert int(r.max()) <= 33 - log2m <= 29
        assert hll.lut(arr, stored_type, log2m).tolist() == [jj | rr << 16 for jj, rr in (ref_offer(h, log2m) for h in want)]
        s = hll.sketch_of(arr, stored_type, log2m)
        words = ref_sketch(values, stored_type, log2m)
        assert s.words.tolist() == words
        assert s.cardinality() == ref_cardinality(words, log2m)


def test_float_zero_signs_and_int_widths_hash_apart():
    f = hll.hash_values(np.array([0.0, -0.0], dtype=np.float32), PGPU_FLOAT)
    assert f[0] != f[1]
    # an INT is offered as its sign-extended long: the same hash as the LONG of that value
    assert hll.hash_values(np.array([-5], dtype=np.int32), PGPU_INT)[0] == hll.hash_values(np.array([-5]), PGPU_LONG)[0]


def test_known_answers():
    """tests/golden/hll_kat.json pins this restatement (its hashes came from the scalar implementation above), not the
    library: a change to either implementation that moves a hash shows here."""
    with open(KAT) as f:
        kat = json.load(f)
    assert len(kat["pairs"]) >= 36
    types = {"INT": PGPU_INT, "LONG": PGPU_LONG, "FLOAT": PGPU_FLOAT, "DOUBLE": PGPU_DOUBLE, "STRING": PGPU_STRING}
    for e in kat["pairs"]:
        t = types[e["type"]]
        if t == PGPU_STRING:
            v = e["value"]
        elif t in (PGPU_INT, PGPU_LONG):
            v = int(e["value"])
        else:  # floating values are stored by their bits
            v = struct.unpack("<f", struct.pack("<I", int(e["bits"])))[0] if t == PGPU_FLOAT else \
                struct.unpack("<d", struct.pack("<Q", int(e["bits"])))[0]
        assert ref_hash(v, t) == e["hash"], e
        assert int(hll.hash_values(_array([v], t), t)[0]) == e["hash"], e


@pytest.mark.parametrize("log2m,bound", [(8, 0.20), (12, 0.05)])
def test_estimates_are_within_the_reference_bounds(log2m, bound):
    """Within 20 % at log2m 8 and 5 % at 12 (DistinctCountQueriesTest.java:296,380); exact up to 10 values."""
    rng = np.random.default_rng(20260101)
    pool = rng.permutation(np.arange(-(1 << 30), (1 << 30), 1 << 11, dtype=np.int64))[:100000].astype(np.int32)
    assert len(np.unique(pool)) == 100000
    for n in (1, 10, 100, 1000, 5000, 100000):
        est = hll.sketch_of(pool[:n], PGPU_INT, log2m).cardinality()
        print(f"log2m {log2m}: {n} distinct values estimated as {est}")
        if n <= 10:
            assert est == n
        assert abs(est - n) <= bound * n, (n, est)


def test_estimate_ignores_repeats_and_order():
    v = np.arange(3000, dtype=np.int32) * 17
    a = hll.sketch_of(v, PGPU_INT, 8)
    b = hll.sketch_of(np.concatenate([v[::-1], v, v[:100]]), PGPU_INT, 8)
    assert a == b


def test_merge():
    rng = np.random.default_rng(3)
    v = rng.integers(-(1 << 31), 1 << 31, 4000).astype(np.int32)
    a, b = hll.sketch_of(v[:2500], PGPU_INT, 8), hll.sketch_of(v[1500:], PGPU_INT, 8)
    both = hll.sketch_of(v, PGPU_INT, 8)
    assert a.merge(b) == both == b.merge(a)
    assert a.merge(b).registers().tolist() == np.maximum(a.registers(), b.registers()).tolist()
    assert a.merge(hll.HyperLogLog.empty(8)) == a
    # unequal sizes (DistinctCountHLLAggregationFunction.java:332-349): the empty one yields, two non-empty are refused
    big = hll.sketch_of(v, PGPU_INT, 12)
    assert hll.HyperLogLog.empty(8).merge(big) == big and big.merge(hll.HyperLogLog.empty(8)) == big
    with pytest.raises(ValueError):
        a.merge(big)


@pytest.mark.parametrize("log2m", [3, 17, 0, 32])
def test_unserved_log2m_keeps_the_cpu_plan(log2m):
    with pytest.raises(UnsupportedPlanError):
        hll.lut(np.arange(4, dtype=np.int32), PGPU_INT, log2m)
    with pytest.raises(UnsupportedPlanError):
        hll.HyperLogLog.empty(log2m)
