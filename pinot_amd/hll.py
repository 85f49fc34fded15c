"""HyperLogLog as DISTINCTCOUNTHLL / DISTINCTCOUNTRAWHLL use it: the sketch on the host.

The reference keeps a bitmap of the column's dictionary ids per group and makes the sketch only at extract time
(DistinctCountHLLAggregationFunction.java:104-110,176-184,438-447: ``hll.offer(dictionary.get(id))`` for every id of the
bitmap), so a group's sketch is a pure function of which ids it met.  This module is a numpy restatement of what
``com.clearspring.analytics.stream.cardinality.HyperLogLog``, ``RegisterSet`` and ``MurmurHash`` (stream-lib, a
third-party library whose source is not part of the reference tree) do with the values offered to them, written from
the published algorithm.  What the reference tree itself pins -- the register count and byte size per ``log2m``
(DistinctCountQueriesTest.java:291-350), the serialised form being ``hll.getBytes()`` (ObjectSerDeUtils
.HYPER_LOG_LOG_SER_DE), the default ``log2m`` 8 (CommonConstants.java:85), the merge rule
(DistinctCountHLLAggregationFunction.java:332-349) and the estimate bounds its tests assert -- is held by
tests/test_hll_sketch.py; wire compatibility with a Java server's sketches rests on those facts and on round trips only.

Hash of a value, all arithmetic 32-bit wrapping with ``m = 0x5bd1e995``:
  hashLong(x)   h = 0; k = (int)x * m; k ^= k >>> 24; h ^= k * m; k = (int)(x >> 32) * m; k ^= k >>> 24; h *= m;
                h ^= k * m; h ^= h >>> 13; h *= m; h ^= h >>> 15
  INT, LONG     hashLong of the (sign-extended) value;  FLOAT: of the sign-extended floatToRawIntBits;  DOUBLE: of
                doubleToRawLongBits
  STRING        MurmurHash2 of the UTF-8 bytes with seed -1: h = seed ^ length; per 4 little-endian bytes k *= m;
                k ^= k >>> 24; k *= m; h *= m; h ^= k; the 1-3 tail bytes xor-ed in at shifts 16 / 8 / 0 sign-extended
                (a Java byte cast to int), then h *= m; the same final mix
Offer: register ``j = h >>> (32 - log2m)`` takes ``r = nlz((h << log2m) | ((1 << (log2m - 1)) + 1)) + 1`` when larger.
Registers are 5 bits each, six per int32 word (register p in word p / 6 at bit 5 * (p mod 6)).
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import UnsupportedPlanError

DEFAULT_LOG2M = 8  # CommonConstants.java:85
MIN_LOG2M, MAX_LOG2M = 4, 16  # r <= 33 - log2m fits the 5 bits, j the low 16 bits of a LUT entry
_M = np.uint32(0x5BD1E995)


def check_log2m(log2m: int) -> int:
    if not MIN_LOG2M <= int(log2m) <= MAX_LOG2M:
        raise UnsupportedPlanError(_lib.PGPU_E_UNSUPPORTED,
                                   f"HyperLogLog with log2m {log2m} (served: {MIN_LOG2M}..{MAX_LOG2M})")
    return int(log2m)


def num_words(log2m: int) -> int:
    """RegisterSet's int32 words for 2^log2m registers (pgpu_hll_words)."""
    b = (1 << log2m) // 6
    if b == 0:
        return 1
    return b if b % 32 == 0 else b + 1


def _mix_k(k: np.ndarray) -> np.ndarray:
    k = k * _M
    k ^= k >> np.uint32(24)
    return k * _M


def _final_mix(h: np.ndarray) -> np.ndarray:
    h ^= h >> np.uint32(13)
    h *= _M
    h ^= h >> np.uint32(15)
    return h


def hash_longs(x) -> np.ndarray:
    """MurmurHash.hashLong of int64 values: uint32[n]."""
    u = np.ascontiguousarray(x, dtype=np.int64).view(np.uint64)
    lo = (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (u >> np.uint64(32)).astype(np.uint32)
    h = _mix_k(lo)  # (h = 0 ^ k * m)
    h *= _M
    h ^= _mix_k(hi)
    return _final_mix(h)


def hash_strings(values) -> np.ndarray:
    """MurmurHash.hash(bytes, length, -1) of the UTF-8 bytes of every string: uint32[n].  Strings of one byte length
    are hashed together."""
    enc = [v if isinstance(v, (bytes, bytearray)) else str(v).encode("utf-8") for v in values]
    out = np.zeros(len(enc), dtype=np.uint32)
    by_len: dict = {}
    for i, b in enumerate(enc):
        by_len.setdefault(len(b), []).append(i)
    for n, idx in by_len.items():
        rows = np.frombuffer(b"".join(enc[i] for i in idx), dtype=np.uint8).reshape(len(idx), n) if n else \
            np.zeros((len(idx), 0), dtype=np.uint8)
        h = np.full(len(idx), 0xFFFFFFFF ^ n, dtype=np.uint32)
        n4 = n // 4
        if n4:
            words = np.ascontiguousarray(rows[:, : 4 * n4]).view("<u4").astype(np.uint32)
            for w in range(n4):
                h *= _M
                h ^= _mix_k(words[:, w])
        tail = n - 4 * n4
        if tail:
            # a Java byte is signed: the cast to int sign-extends, so a byte >= 0x80 also sets every bit above its own
            t = rows[:, 4 * n4:].astype(np.int8).astype(np.int32).view(np.uint32)
            for k in range(tail - 1, -1, -1):
                h ^= t[:, k] << np.uint32(8 * k)
            h *= _M
        out[np.asarray(idx, dtype=np.int64)] = _final_mix(h)
    return out


def hash_values(values, stored_type: int) -> np.ndarray:
    """The 32-bit hash the reference's ``hll.offer(value)`` takes of every value of a column of ``stored_type``
    (PGPU_INT .. PGPU_STRING): uint32[n]."""
    if stored_type == _lib.PGPU_STRING:
        return hash_strings(list(values))
    if stored_type == _lib.PGPU_INT:
        return hash_longs(np.asarray(values, dtype=np.int32).astype(np.int64))
    if stored_type == _lib.PGPU_LONG:
        return hash_longs(np.asarray(values, dtype=np.int64))
    if stored_type == _lib.PGPU_FLOAT:
        return hash_longs(np.ascontiguousarray(values, dtype=np.float32).view(np.int32).astype(np.int64))
    if stored_type == _lib.PGPU_DOUBLE:
        return hash_longs(np.ascontiguousarray(values, dtype=np.float64).view(np.int64))
    raise UnsupportedPlanError(_lib.PGPU_E_UNSUPPORTED, f"HyperLogLog over a column of stored type {stored_type}")


def offers(hashes: np.ndarray, log2m: int):
    """(j, r) of HyperLogLog.offerHashed per hash: the register and the rank it is raised to."""
    log2m = check_log2m(log2m)
    h = np.asarray(hashes, dtype=np.uint32)
    j = h >> np.uint32(32 - log2m)
    w = (h << np.uint32(log2m)) | np.uint32((1 << (log2m - 1)) + 1)
    # nlz of a non-zero 32-bit word: 32 - its bit length, the exponent frexp gives of the exact double
    r = (33 - np.frexp(w.astype(np.float64))[1]).astype(np.uint32)
    return j, r


def lut(dictionary, stored_type: int, log2m: int) -> np.ndarray:
    """uint32[card]: lut[cid] = j | r << 16 of the dictionary's value cid -- what the device stage reads per occupied
    cell (pgpu_table_hll)."""
    j, r = offers(hash_values(dictionary, stored_type), log2m)
    return np.ascontiguousarray(j | (r << np.uint32(16)), dtype=np.uint32)


def pack_registers(regs: np.ndarray, log2m: int) -> np.ndarray:
    """2^log2m register values -> the RegisterSet words."""
    w = num_words(log2m)
    padded = np.zeros(6 * w, dtype=np.uint32)
    padded[: 1 << log2m] = regs
    shifts = (np.uint32(5) * np.arange(6, dtype=np.uint32))[None, :]
    return np.bitwise_or.reduce(padded.reshape(w, 6) << shifts, axis=1).astype(np.uint32)


def unpack_registers(words: np.ndarray, log2m: int) -> np.ndarray:
    shifts = (np.uint32(5) * np.arange(6, dtype=np.uint32))[None, :]
    regs = (np.asarray(words, dtype=np.uint32)[:, None] >> shifts) & np.uint32(31)
    return regs.reshape(-1)[: 1 << log2m]


@dataclass
class HyperLogLog:
    """A sketch: ``words`` are the RegisterSet's int32 words as uint32[num_words(log2m)]."""
    log2m: int
    words: np.ndarray

    @staticmethod
    def empty(log2m: int = DEFAULT_LOG2M) -> "HyperLogLog":
        return HyperLogLog(check_log2m(log2m), np.zeros(num_words(log2m), dtype=np.uint32))

    def registers(self) -> np.ndarray:
        return unpack_registers(self.words, self.log2m)

    def cardinality(self) -> int:
        """HyperLogLog.cardinality(): a LONG.  Java's Math.log and libm may differ in the last ulp, which could only
        show where m * ln(m / Z) falls on an exact .5; Math.round is floor(x + 0.5)."""
        m = 1 << self.log2m
        regs = self.registers()
        total = float(np.sum(np.ldexp(1.0, -regs.astype(np.int64))))
        zeros = int(np.count_nonzero(regs == 0))
        a = {4: 0.673, 5: 0.697, 6: 0.709}.get(self.log2m, 0.7213 / (1 + 1.079 / m))
        e = a * m * m / total
        if e <= 2.5 * m:
            if zeros == 0:  # (m * ln(m / 0.0) is +Infinity in Java, which Math.round saturates)
                return (1 << 63) - 1
            return int(math.floor(m * math.log(m / float(zeros)) + 0.5))
        return int(math.floor(e + 0.5))

    def to_bytes(self) -> bytes:
        """hll.getBytes(): big-endian int32 log2m, int32 4 * W, the W words."""
        w = np.asarray(self.words, dtype=np.uint32)
        return struct.pack(">ii", self.log2m, 4 * len(w)) + w.astype(">u4").tobytes()

    @staticmethod
    def from_bytes(data: bytes, offset: int = 0) -> "HyperLogLog":
        log2m, nbytes = struct.unpack_from(">ii", data, offset)
        if not MIN_LOG2M <= log2m <= MAX_LOG2M or nbytes != 4 * num_words(log2m) or len(data) < offset + 8 + nbytes:
            raise ValueError(f"not a HyperLogLog of log2m {MIN_LOG2M}..{MAX_LOG2M}: log2m {log2m}, {nbytes} bytes")
        return HyperLogLog(log2m, np.frombuffer(data, dtype=">u4", count=nbytes // 4, offset=offset + 8).astype(np.uint32))

    def merge(self, other: "HyperLogLog") -> "HyperLogLog":
        """DistinctCountHLLAggregationFunction.merge (:332-349): sketches of one size unite register by register; of
        two sizes the one of cardinality 0 yields; anything else is refused."""
        if self.log2m == other.log2m:
            return HyperLogLog(self.log2m, pack_registers(np.maximum(self.registers(), other.registers()), self.log2m))
        if self.cardinality() == 0:
            return other
        if other.cardinality() == 0:
            return self
        raise ValueError(f"cannot merge HyperLogLogs of log2m {self.log2m} and {other.log2m}")

    def __eq__(self, other) -> bool:
        return isinstance(other, HyperLogLog) and self.log2m == other.log2m and \
            np.array_equal(np.asarray(self.words, dtype=np.uint32), np.asarray(other.words, dtype=np.uint32))


def sketch_of_lut(entries: np.ndarray, log2m: int) -> HyperLogLog:
    """The sketch of the values whose LUT entries are given."""
    log2m = check_log2m(log2m)
    e = np.asarray(entries, dtype=np.uint32)
    regs = np.zeros(1 << log2m, dtype=np.uint32)
    np.maximum.at(regs, (e & np.uint32(0xFFFF)).astype(np.int64), e >> np.uint32(16))
    return HyperLogLog(log2m, pack_registers(regs, log2m))


def sketch_of(values, stored_type: int, log2m: int = DEFAULT_LOG2M) -> HyperLogLog:
    """The sketch the reference builds by offering every value of ``values``."""
    return sketch_of_lut(lut(values, stored_type, log2m), log2m)
