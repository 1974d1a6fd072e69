"""The reference's `State` case classes, backed by the C-ABI's state algebra.

Every `sum` and `metricValue` goes through `dq_state_merge` / `dq_state_metric`
(deequ_amd/csrc/dq_api.cpp), which restate each Scala `State.sum` exactly, so states produced
on different GPUs, batches or runs (or loaded from a StateProvider) combine the way Spark
partial states do.

* NumMatches -- Size.scala:23-31
* NumMatchesAndCount -- Analyzer.scala:230-244
* SumState -- Sum.scala:25-33;  MeanState -- Mean.scala:25-34
* StandardDeviationState -- StandardDeviation.scala:25-45
* MinState / MaxState -- Minimum.scala:25-33 / Maximum.scala:25-33
* ApproxCountDistinctState -- ApproxCountDistinct.scala:26-40
* DataTypeHistogram -- DataType.scala:40-52
* CorrelationState -- Correlation.scala:26-57
* KLLState, QuantileNonSample, NonSampleCompactor -- KLLSketch.scala:42-74, QuantileNonSample.scala,
  NonSampleCompactor.scala (pure Python: the sketch is variable-size and has no POD image)
* ApproxQuantileState, PercentileDigest -- ApproxQuantile.scala:29-37 over this project's
  Greenwald-Khanna digest (ApproxQuantile; pure Python, the mirror of dq_quantile.cpp)
"""
from __future__ import annotations

import ctypes
import math
import struct
from typing import Dict, List, Optional, Sequence, Tuple

from . import _lib as L


class State:
    KIND = 0

    def to_dq(self) -> L.DqState:
        raise NotImplementedError

    @classmethod
    def from_dq(cls, s: L.DqState) -> "State":
        raise NotImplementedError

    def sum(self, other: "State") -> "State":
        if type(other) is not type(self):
            raise TypeError("cannot sum %s with %s" % (type(self).__name__, type(other).__name__))
        a, b, out = self.to_dq(), other.to_dq(), L.DqState()
        L.check(L.lib().dq_state_merge(ctypes.byref(a), ctypes.byref(b), ctypes.byref(out)))
        return type(self).from_dq(out)

    __add__ = sum

    def metricValue(self) -> float:
        s, out = self.to_dq(), ctypes.c_double()
        L.check(L.lib().dq_state_metric(ctypes.byref(s), ctypes.byref(out)))
        return out.value

    def _dq(self, **fields) -> L.DqState:
        s = L.DqState()
        s.kind = self.KIND
        s.has_value = 1
        for k, v in fields.items():
            setattr(s, k, v)
        return s


class NumMatches(State):
    KIND = L.DQ_OP_SIZE

    def __init__(self, numMatches: int):
        self.numMatches = int(numMatches)

    def to_dq(self):
        return self._dq(num_matches=self.numMatches)

    @classmethod
    def from_dq(cls, s):
        return cls(s.num_matches)

    def __eq__(self, o):
        return isinstance(o, NumMatches) and o.numMatches == self.numMatches

    def __hash__(self):
        return hash(("NumMatches", self.numMatches))

    def __repr__(self):
        return "NumMatches(%d)" % self.numMatches


class NumMatchesAndCount(State):
    KIND = L.DQ_OP_COMPLETENESS

    def __init__(self, numMatches: int, count: int):
        self.numMatches = int(numMatches)
        self.count = int(count)

    def to_dq(self):
        return self._dq(num_matches=self.numMatches, count=self.count)

    @classmethod
    def from_dq(cls, s):
        return cls(s.num_matches, s.count)

    def __eq__(self, o):
        return isinstance(o, NumMatchesAndCount) and (o.numMatches, o.count) == (self.numMatches, self.count)

    def __hash__(self):
        return hash(("NumMatchesAndCount", self.numMatches, self.count))

    def __repr__(self):
        return "NumMatchesAndCount(%d,%d)" % (self.numMatches, self.count)


class SumState(State):
    KIND = L.DQ_OP_SUM

    def __init__(self, sum: float):  # noqa: A002 - mirrors the Scala field name
        self.sum_value = float(sum)

    def to_dq(self):
        return self._dq(sum=self.sum_value)

    @classmethod
    def from_dq(cls, s):
        return cls(s.sum)

    def __eq__(self, o):
        return isinstance(o, SumState) and o.sum_value == self.sum_value

    def __hash__(self):
        return hash(("SumState", self.sum_value))

    def __repr__(self):
        return "SumState(%r)" % self.sum_value


class MeanState(State):
    KIND = L.DQ_OP_MEAN

    def __init__(self, sum: float, count: int):  # noqa: A002
        self.sum_value = float(sum)
        self.count = int(count)

    def to_dq(self):
        return self._dq(sum=self.sum_value, count=self.count)

    @classmethod
    def from_dq(cls, s):
        return cls(s.sum, s.count)

    def __eq__(self, o):
        return isinstance(o, MeanState) and (o.sum_value, o.count) == (self.sum_value, self.count)

    def __hash__(self):
        return hash(("MeanState", self.sum_value, self.count))

    def __repr__(self):
        return "MeanState(%r,%d)" % (self.sum_value, self.count)


class StandardDeviationState(State):
    KIND = L.DQ_OP_STDDEV

    def __init__(self, n: float, avg: float, m2: float):
        if not n > 0.0:  # StandardDeviation.scala:31
            raise ValueError("requirement failed: Standard deviation is undefined for n = 0.")
        self.n, self.avg, self.m2 = float(n), float(avg), float(m2)

    def to_dq(self):
        return self._dq(n=self.n, avg=self.avg, m2=self.m2)

    @classmethod
    def from_dq(cls, s):
        return cls(s.n, s.avg, s.m2)

    def __eq__(self, o):
        return isinstance(o, StandardDeviationState) and (o.n, o.avg, o.m2) == (self.n, self.avg, self.m2)

    def __hash__(self):
        return hash(("StandardDeviationState", self.n, self.avg, self.m2))

    def __repr__(self):
        return "StandardDeviationState(%r,%r,%r)" % (self.n, self.avg, self.m2)


class MinState(State):
    KIND = L.DQ_OP_MINIMUM

    def __init__(self, minValue: float):
        self.minValue = float(minValue)

    def to_dq(self):
        return self._dq(value=self.minValue)

    @classmethod
    def from_dq(cls, s):
        return cls(s.value)

    def __eq__(self, o):
        return isinstance(o, MinState) and o.minValue == self.minValue

    def __hash__(self):
        return hash(("MinState", self.minValue))

    def __repr__(self):
        return "MinState(%r)" % self.minValue


class MaxState(State):
    KIND = L.DQ_OP_MAXIMUM

    def __init__(self, maxValue: float):
        self.maxValue = float(maxValue)

    def to_dq(self):
        return self._dq(value=self.maxValue)

    @classmethod
    def from_dq(cls, s):
        return cls(s.value)

    def __eq__(self, o):
        return isinstance(o, MaxState) and o.maxValue == self.maxValue

    def __hash__(self):
        return hash(("MaxState", self.maxValue))

    def __repr__(self):
        return "MaxState(%r)" % self.maxValue


class ApproxCountDistinctState(State):
    KIND = L.DQ_OP_APPROX_COUNT_DISTINCT

    def __init__(self, words: Sequence[int]):
        words = tuple(map(int, words))
        if len(words) != L.DQ_HLL_NUM_WORDS:
            raise ValueError("requirement failed: expected %d words" % L.DQ_HLL_NUM_WORDS)
        self.words: Tuple[int, ...] = words

    def to_dq(self):
        s = self._dq()
        s.words[:] = self.words
        return s

    @classmethod
    def from_dq(cls, s):
        return cls(s.words[:])

    def to_bytes(self) -> bytes:
        """DeequHyperLogLogPlusPlusUtils.wordsToBytes (StatefulHyperloglogPlus.scala:170-178)."""
        w = (ctypes.c_int64 * L.DQ_HLL_NUM_WORDS)(*self.words)
        out = (ctypes.c_uint8 * 416)()
        L.lib().dq_hll_words_to_bytes(w, out)
        return bytes(out)

    @classmethod
    def from_bytes(cls, b: bytes) -> "ApproxCountDistinctState":
        if len(b) != 416:
            raise ValueError("requirement failed: expected 416 bytes")
        buf = (ctypes.c_uint8 * 416)(*b)
        w = (ctypes.c_int64 * L.DQ_HLL_NUM_WORDS)()
        L.lib().dq_hll_words_from_bytes(buf, w)
        return cls(list(w))

    def __eq__(self, o):
        return isinstance(o, ApproxCountDistinctState) and o.words == self.words

    def __hash__(self):
        return hash(("ApproxCountDistinctState", self.words))

    def __repr__(self):
        return "ApproxCountDistinctState(%s)" % ",".join(str(w) for w in self.words)


class DataTypeHistogram(State):
    """DataTypeHistogram(numNull, numFractional, numIntegral, numBoolean, numString)
    (DataType.scala:40-52); sum adds the counts.  Not a DoubleValuedState."""
    KIND = L.DQ_OP_DATATYPE
    SIZE_IN_BYTES = 40

    def __init__(self, numNull: int, numFractional: int, numIntegral: int, numBoolean: int, numString: int):
        self.numNull, self.numFractional, self.numIntegral = int(numNull), int(numFractional), int(numIntegral)
        self.numBoolean, self.numString = int(numBoolean), int(numString)

    def counts(self) -> Tuple[int, int, int, int, int]:
        return (self.numNull, self.numFractional, self.numIntegral, self.numBoolean, self.numString)

    def to_dq(self):
        s = self._dq()
        for i, c in enumerate(self.counts()):
            s.words[i] = c
        return s

    @classmethod
    def from_dq(cls, s):
        return cls(*[s.words[i] for i in range(5)])

    def metricValue(self):
        raise TypeError("DataTypeHistogram is not a DoubleValuedState")

    def toBytes(self) -> bytes:
        """DataTypeHistogram.toBytes (DataType.scala:75-96): five big-endian longs."""
        import struct
        return struct.pack(">5q", *self.counts())

    @classmethod
    def fromBytes(cls, b: bytes) -> "DataTypeHistogram":
        import struct
        if len(b) != cls.SIZE_IN_BYTES:
            raise ValueError("requirement failed")
        return cls(*struct.unpack(">5q", b))

    def __eq__(self, o):
        return isinstance(o, DataTypeHistogram) and o.counts() == self.counts()

    def __hash__(self):
        return hash(("DataTypeHistogram",) + self.counts())

    def __repr__(self):
        return "DataTypeHistogram(%d,%d,%d,%d,%d)" % self.counts()


class CorrelationState(State):
    """CorrelationState(n, xAvg, yAvg, ck, xMk, yMk) (Correlation.scala:26-57)."""
    KIND = L.DQ_OP_CORRELATION

    def __init__(self, n: float, xAvg: float, yAvg: float, ck: float, xMk: float, yMk: float):
        if not n > 0.0:  # Correlation.scala:35
            raise ValueError("requirement failed: Correlation undefined for n = 0.")
        self.n, self.xAvg, self.yAvg = float(n), float(xAvg), float(yAvg)
        self.ck, self.xMk, self.yMk = float(ck), float(xMk), float(yMk)

    def fields(self) -> Tuple[float, ...]:
        return (self.n, self.xAvg, self.yAvg, self.ck, self.xMk, self.yMk)

    def to_dq(self):
        return self._dq(n=self.n, avg=self.xAvg, y_avg=self.yAvg, ck=self.ck, x_mk=self.xMk, y_mk=self.yMk)

    @classmethod
    def from_dq(cls, s):
        return cls(s.n, s.avg, s.y_avg, s.ck, s.x_mk, s.y_mk)

    def __eq__(self, o):
        return isinstance(o, CorrelationState) and o.fields() == self.fields()

    def __hash__(self):
        return hash(("CorrelationState",) + self.fields())

    def __repr__(self):
        return "CorrelationState(%r,%r,%r,%r,%r,%r)" % self.fields()


# ---------------------------------------------------------------- KLL sketches
def _java_sort_key(x: float):
    """Sort key with java.lang.Double.compare's order: -0.0 before 0.0, every NaN equal and last
    (Python's stable sort then keeps NaNs in arrival order, as java.util.Arrays.sort of objects)."""
    if x != x:
        return (1, 0.0, 0.0)
    return (0, x, math.copysign(1.0, x))


def java_min(a: float, b: float) -> float:
    """java.lang.Math.min(double, double): NaN if either is, -0.0 below 0.0."""
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, b) < 0:
        return b
    return a if a <= b else b


def java_max(a: float, b: float) -> float:
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, a) < 0:
        return b
    return a if a >= b else b


def _to_int(x: float) -> int:
    """Scala's Double.toInt: NaN -> 0, saturating."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)


def _wrap_int(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


class NonSampleCompactor:
    """NonSampleCompactor[Double] (NonSampleCompactor.scala:29-69).  The random offset of the
    original KLL is commented out there (:49-51), so `compact` is deterministic."""

    __slots__ = ("numOfCompress", "offset", "buffer")

    def __init__(self):
        self.numOfCompress = 0
        self.offset = 0
        self.buffer: List[float] = []

    def compact(self) -> List[float]:
        items = len(self.buffer)
        n = items - (items % 2)
        if self.numOfCompress % 2 == 1:
            self.offset = 1 - self.offset
        ordered = sorted(self.buffer[:n], key=_java_sort_key)
        output = ordered[self.offset:n:2]
        self.buffer = [self.buffer[items - 1]] if items % 2 == 1 else []  # the odd tail: the last appended item
        self.numOfCompress += 1
        return output


class QuantileNonSample:
    """QuantileNonSample[Double] (QuantileNonSample.scala:25-305): the reference's KLL sketch,
    restated; the oracle the C++ host sketch (dq_kll.cpp) and the GPU kernels (dq_kll.hip) are
    checked against level for level."""

    def __init__(self, sketchSize: int, shrinkingFactor: float = 0.64):
        self.sketchSize = int(sketchSize)
        self.shrinkingFactor = float(shrinkingFactor)
        self.curNumOfCompactors = 0
        self.compactorActualSize = 0
        self.compactorTotalSize = 0
        self.compactors: List[NonSampleCompactor] = []
        self.expand()

    def reconstruct(self, sketchSize: int, shrinkingFactor: float, data) -> None:
        self.sketchSize = int(sketchSize)
        self.shrinkingFactor = float(shrinkingFactor)
        self.compactors = [NonSampleCompactor() for _ in data]
        for c, level in zip(self.compactors, data):
            c.buffer = [float(v) for v in level]
        self.curNumOfCompactors = len(self.compactors)
        self.compactorActualSize = self.getCompactorItemsCount()
        self.compactorTotalSize = self.getCompactorCapacityCount()

    def getCompactorItems(self) -> List[List[float]]:
        return [list(c.buffer) for c in self.compactors]

    def expand(self) -> None:
        self.compactors.append(NonSampleCompactor())
        self.curNumOfCompactors = len(self.compactors)
        self.compactorTotalSize = self.getCompactorCapacityCount()

    def capacity(self, height: int) -> int:
        """2 * (ceil(sketchSize * pow(shrinkingFactor, height) / 2).toInt + 1) (:78-80)."""
        try:
            p = math.pow(self.shrinkingFactor, height)
        except (OverflowError, ValueError):
            p = float("inf")
        x = self.sketchSize * p / 2
        c = _to_int(math.ceil(x) if x == x and abs(x) != float("inf") else x)
        return _wrap_int(2 * _wrap_int(c + 1))

    def update(self, item: float) -> None:
        self.compactors[0].buffer.append(float(item))
        self.compactorActualSize += 1
        if self.compactorActualSize > self.compactorTotalSize:
            self.condense()

    def updateAll(self, items) -> None:
        """`update` for every item in order, in bulk: the items up to the one that makes
        actual > total are appended at once, then one condense -- what the GPU kernel does."""
        items = [float(v) for v in items]
        at = 0
        while at < len(items):
            room = self.compactorTotalSize - self.compactorActualSize
            take = items[at:at + room + 1]
            at += len(take)
            self.compactors[0].buffer.extend(take)
            self.compactorActualSize += len(take)
            if self.compactorActualSize > self.compactorTotalSize:
                self.condense()

    def condense(self) -> None:
        for height in range(len(self.compactors)):
            if len(self.compactors[height].buffer) >= self.capacity(height):
                if height + 1 >= self.curNumOfCompactors:
                    self.expand()
                self.compactors[height + 1].buffer.extend(self.compactors[height].compact())
                self.compactorActualSize = self.getCompactorItemsCount()
                break

    def _output(self):
        return [(v, 1 << i) for i, c in enumerate(self.compactors[:self.curNumOfCompactors]) for v in c.buffer]

    def getRank(self, item: float, rankMap: Optional[Dict[float, int]] = None) -> int:
        """Weight of the items not greater than `item` (:163-171; Ordering.Double.gt is `>`).
        With `rankMap` (getRankMap's result) the reference's second overload (:194-205): the rank
        of the last entry before the first one greater than `item`."""
        if rankMap is not None:
            cur = 0
            for v, r in rankMap.items():
                if v > item:
                    break
                cur = r
            return cur
        return sum(w for v, w in self._output() if not v > item)

    def getRankExclusive(self, item: float) -> int:
        return sum(w for v, w in self._output() if v < item)

    def getRankMap(self) -> Dict[float, int]:
        """Item -> running rank, ascending by item (:126-139).  The reference first puts the
        sorted (item, weight) pairs into a ListMap, which keeps one entry per item -- the last of
        several equal items, with its weight alone -- and only then accumulates the weights."""
        last: Dict[float, int] = {}
        for v, w in sorted(self._output(), key=lambda iw: _java_sort_key(iw[0])):
            last.pop(v, None)  # (ListMap.updated: the entry moves to the end)
            last[v] = w
        ranks: Dict[float, int] = {}
        running = 0
        for v, w in last.items():
            running += w
            ranks[v] = running
        return dict(sorted(ranks.items(), key=lambda iw: _java_sort_key(iw[0])))

    def getCDF(self) -> List[Tuple[float, float]]:
        """(item, rank / total weight) per entry of the rank map (:146-155)."""
        rankMap = self.getRankMap()
        if not rankMap:
            raise ValueError("getCDF of an empty sketch (the reference's `last` of an empty map throws)")
        total = float(list(rankMap.values())[-1])
        return [(v, float(r) / total) for v, r in rankMap.items()]


    def merge(self, that: "QuantileNonSample") -> "QuantileNonSample":
        """:215-230.  Mutates and returns self, as the reference does."""
        while self.curNumOfCompactors < that.curNumOfCompactors:
            self.expand()
        for i in range(that.curNumOfCompactors):
            self.compactors[i].buffer = self.compactors[i].buffer + that.compactors[i].buffer
        self.compactorActualSize = self.getCompactorItemsCount()
        while self.compactorActualSize >= self.compactorTotalSize:
            before = (self.compactorActualSize, self.curNumOfCompactors)
            self.condense()
            if before == (self.compactorActualSize, self.curNumOfCompactors):
                break  # (no level at its capacity: the reference would spin)
        return self

    def quantiles(self, q: int) -> List[float]:
        """The quantiles 1/q .. (q-1)/q (:246-278)."""
        output = self._output()
        if not output:
            return []
        sortedItems = sorted(output, key=lambda iw: _java_sort_key(iw[0]))
        totalWeight = sum(w for _, w in sortedItems)
        nextThresh = totalWeight // q
        curq, i, sumSoFar = 1, 0, 0
        quantiles = [sortedItems[0][0]] * (q - 1)
        while i < len(sortedItems) and curq < q:
            while sumSoFar < nextThresh:
                sumSoFar += sortedItems[i][1]
                i += 1
            quantiles[curq - 1] = sortedItems[min(i, len(sortedItems) - 1)][0]
            curq += 1
            nextThresh = curq * totalWeight // q
        return quantiles

    def getCompactorItemsCount(self) -> int:
        return sum(len(c.buffer) for c in self.compactors[:self.curNumOfCompactors])

    def getCompactorCapacityCount(self) -> int:
        return sum(self.capacity(h) for h in range(self.curNumOfCompactors))

    def copy(self) -> "QuantileNonSample":
        out = QuantileNonSample.__new__(QuantileNonSample)
        out.sketchSize, out.shrinkingFactor = self.sketchSize, self.shrinkingFactor
        out.curNumOfCompactors = self.curNumOfCompactors
        out.compactorActualSize, out.compactorTotalSize = self.compactorActualSize, self.compactorTotalSize
        out.compactors = []
        for c in self.compactors:
            d = NonSampleCompactor()
            d.numOfCompress, d.offset, d.buffer = c.numOfCompress, c.offset, list(c.buffer)
            out.compactors.append(d)
        return out

    def weight(self) -> int:
        """Sum of len(level i) * 2^i: the number of updates the sketch stands for."""
        return sum(len(c.buffer) << i for i, c in enumerate(self.compactors))

    def levels(self) -> List[tuple]:
        """Per level (numOfCompress, offset, the items' bit patterns): what the parity tests compare."""
        return [(c.numOfCompress, c.offset, struct.pack("<%dd" % len(c.buffer), *c.buffer)) for c in self.compactors]


KLL_INIT_MIN = 2147483647.0   # Int.MaxValue.toDouble (KLLRunner.scala:28)
KLL_INIT_MAX = -2147483648.0  # Int.MinValue.toDouble (KLLRunner.scala:29)


class KLLState(State):
    """KLLState(qSketch, globalMax, globalMin) (KLLSketch.scala:42-74)."""

    def __init__(self, qSketch: QuantileNonSample, globalMax: float, globalMin: float):
        self.qSketch = qSketch
        self.globalMax = float(globalMax)
        self.globalMin = float(globalMin)

    def sum(self, other: "KLLState") -> "KLLState":
        if not isinstance(other, KLLState):
            raise TypeError("cannot sum KLLState with %s" % type(other).__name__)
        # (the reference merges into this.qSketch in place; a copy keeps a persisted state intact)
        merged = self.qSketch.copy().merge(other.qSketch)
        return KLLState(merged, java_max(self.globalMax, other.globalMax), java_min(self.globalMin, other.globalMin))

    __add__ = sum

    def metricValue(self):
        raise TypeError("KLLState is not a DoubleValuedState")

    def to_dq(self):
        raise TypeError("KLLState has no POD image: it travels through dq_kll_export")

    def to_bytes(self) -> bytes:
        """The UDAF's buffer (StatefulKLLSketch: min, max, then KLLSketchSerializer.serialize,
        KLLSketchSerializer.scala:58-81), big-endian -- what KLLState.fromBytes reads."""
        q = self.qSketch
        out = [struct.pack(">dd", self.globalMin, self.globalMax),
               struct.pack(">idiiii", q.sketchSize, q.shrinkingFactor, q.curNumOfCompactors, q.compactorActualSize,
                           q.compactorTotalSize, len(q.compactors))]
        for c in q.compactors:
            out.append(struct.pack(">iii%dd" % len(c.buffer), c.numOfCompress, c.offset, len(c.buffer), *c.buffer))
        return b"".join(out)

    @classmethod
    def from_bytes(cls, b: bytes) -> "KLLState":
        """KLLState.fromBytes (KLLSketch.scala:64-72) over KLLSketchSerializer.deserialize (:83-115)."""
        lo, hi = struct.unpack_from(">dd", b, 0)
        k, c, cur, actual, total, n = struct.unpack_from(">idiiii", b, 16)
        at = 16 + 28
        q = QuantileNonSample(k, c)
        q.compactors = []
        for _ in range(n):
            comp = NonSampleCompactor()
            comp.numOfCompress, comp.offset, m = struct.unpack_from(">iii", b, at)
            at += 12
            comp.buffer = list(struct.unpack_from(">%dd" % m, b, at))
            at += 8 * m
            q.compactors.append(comp)
        q.curNumOfCompactors, q.compactorActualSize, q.compactorTotalSize = cur, actual, total
        return cls(q, hi, lo)

    @classmethod
    def from_export(cls, buf: bytes, sketchSize: int, shrinkingFactor: float) -> "KLLState":
        """From the words of dq_kll_export / dq_diag_kll_sketch (include/deequ_amd.h)."""
        (n,) = struct.unpack_from("<q", buf, 0)
        lo, hi = struct.unpack_from("<dd", buf, 8)
        heads = struct.unpack_from("<%dq" % (3 * n), buf, 24)
        at = 24 + 24 * n
        q = QuantileNonSample(sketchSize, shrinkingFactor)
        q.compactors = []
        for i in range(n):
            comp = NonSampleCompactor()
            m, comp.numOfCompress, comp.offset = heads[3 * i:3 * i + 3]
            comp.buffer = list(struct.unpack_from("<%dd" % m, buf, at))
            at += 8 * m
            q.compactors.append(comp)
        q.curNumOfCompactors = n
        q.compactorActualSize = q.getCompactorItemsCount()
        q.compactorTotalSize = q.getCompactorCapacityCount()
        return cls(q, hi, lo)

    def signature(self) -> tuple:
        """Everything parity is pinned on, bit for bit: levels, numOfCompress, offset, min, max."""
        return (tuple(self.qSketch.levels()), struct.pack("<dd", self.globalMin, self.globalMax))

    def __eq__(self, o):
        return isinstance(o, KLLState) and o.signature() == self.signature() and \
            (o.qSketch.sketchSize, o.qSketch.shrinkingFactor) == (self.qSketch.sketchSize, self.qSketch.shrinkingFactor)

    def __hash__(self):
        return hash(self.signature())

    def __repr__(self):
        return "KLLState(levels=%s,max=%r,min=%r)" % ([len(c.buffer) for c in self.qSketch.compactors],
                                                    self.globalMax, self.globalMin)


DEFAULT_KLL_SLAB_ROWS = 1 << 16  # kDefaultSlabRows (deequ_amd/csrc/dq_kll.h)


def kll_sketch_slabs(values, sketchSize: int, shrinkingFactor: float, slab_rows: int = DEFAULT_KLL_SLAB_ROWS) -> KLLState:
    """The library's partitioning (KLLSketch) on the CPU mirror: `values` is one batch, a
    sequence of floats with None for NULL; slabs of slab_rows rows each sketched as one reference
    partition (KLLRunner.scala:150-177), merged by the balanced tree in slab order."""
    values = list(values)
    slabs = []
    for r0 in range(0, max(len(values), 1), slab_rows):
        q = QuantileNonSample(sketchSize, shrinkingFactor)
        lo, hi = KLL_INIT_MIN, KLL_INIT_MAX
        rows = [float(v) for v in values[r0:r0 + slab_rows] if v is not None]
        for v in rows:
            lo, hi = java_min(lo, v), java_max(hi, v)
        q.updateAll(rows)
        slabs.append([q, lo, hi])
    step = 1
    while step < len(slabs):
        for j in range(0, len(slabs) - step, 2 * step):
            a, b = slabs[j], slabs[j + step]
            a[0].merge(b[0])
            a[1], a[2] = java_min(a[1], b[1]), java_max(a[2], b[2])
        step *= 2
    return KLLState(slabs[0][0], slabs[0][2], slabs[0][1])


# ---------------------------------------------------------------- ApproxQuantile
_CANONICAL_NAN = 0x7FF8000000000000
DIGEST_COMPRESS_THRESHOLD = 10000  # written into the serialised form, not used here


def double_sort_key(x: float) -> int:
    """The 64-bit key whose unsigned order is java.lang.Double.compare's: -0.0 before 0.0, every NaN
    (canonicalised first) last (ApproxQuantile)."""
    (b,) = struct.unpack("<Q", struct.pack("<d", x))
    if (b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000:
        b = _CANONICAL_NAN
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | (1 << 63))


class PercentileDigest:
    """The digest of ApproxQuantile(s): a Greenwald-Khanna summary, `sampled` = [(value, g, delta)] in
    value order over `count` values, for `relativeError`.  The reference keeps Spark's
    PercentileDigest, whose content depends on insertion order and partitioning; this one is
    defined by DESIGN.md (ApproxQuantile): exact-rank batch summaries, merged in arrival order."""

    def __init__(self, relativeError: float):
        self.relativeError = float(relativeError)
        self.count = 0
        self.sampled: List[Tuple[float, int, int]] = []

    @classmethod
    def from_entries(cls, relativeError: float, count: int, entries) -> "PercentileDigest":
        d = cls(relativeError)
        d.count = int(count)
        d.sampled = [(float(v), int(g), int(delta)) for v, g, delta in entries]
        return d

    def copy(self) -> "PercentileDigest":
        return PercentileDigest.from_entries(self.relativeError, self.count, self.sampled)

    def merge(self, that: "PercentileDigest") -> "PercentileDigest":
        """In place, as the reference's digest.merge; `that` is left unchanged."""
        if that.relativeError != self.relativeError:
            raise ValueError("cannot merge digests of relativeError %r and %r" % (self.relativeError, that.relativeError))
        if not that.sampled:
            return self
        if not self.sampled:
            self.sampled, self.count = list(that.sampled), that.count
            return self
        a, b = self.sampled, that.sampled
        merged, side = [], []
        i = j = 0
        while i < len(a) or j < len(b):  # by key; this side first on ties
            take_a = j == len(b) or (i < len(a) and double_sort_key(a[i][0]) <= double_sort_key(b[j][0]))
            if take_a:
                merged.append(a[i])
                i += 1
            else:
                merged.append(b[j])
                j += 1
            side.append(0 if take_a else 1)
        nxt = [None, None]
        grown = [0] * len(merged)
        for k in range(len(merged) - 1, -1, -1):  # delta grows by g + delta - 1 of the other side's next entry
            s = nxt[1 - side[k]]
            grown[k] = merged[k][2] + (s[1] + s[2] - 1 if s is not None else 0)
            nxt[side[k]] = merged[k]
        merged = [(v, g, grown[k]) for k, (v, g, _) in enumerate(merged)]
        self.count += that.count
        threshold = int(math.floor(2.0 * self.relativeError * float(self.count)))
        kept = []
        head = merged[-1]
        for k in range(len(merged) - 2, 0, -1):  # compress from the right; first and last stay
            v, g, delta = merged[k]
            if g + head[1] + head[2] <= threshold:
                head = (head[0], head[1] + g, head[2])
            else:
                kept.append(head)
                head = merged[k]
        kept.append(head)
        if len(merged) > 1:
            kept.append(merged[0])
        kept.reverse()
        self.sampled = kept
        return self

    def getPercentiles(self, quantiles: Sequence[float]) -> List[float]:
        """[] on an empty digest; else per q the entry that minimises max(t - rmin, rmax - t) for
        t = ceil(q * count), the first on ties."""
        if not self.sampled:
            return []
        out = []
        for q in quantiles:
            t = int(math.ceil(float(q) * float(self.count)))
            rmin, best, at = 0, None, 0
            for k, (_, g, delta) in enumerate(self.sampled):
                rmin += g
                err = max(t - rmin, rmin + delta - t)
                if best is None or err < best:
                    best, at = err, k
            out.append(self.sampled[at][0])
        return out

    def serialize(self) -> bytes:
        """Big-endian: int32 compressThreshold, float64 relativeError, int64 count, int32 len, then
        float64 value, int32 g, int32 delta per entry (unverified against Spark)."""
        out = [struct.pack(">idqi", DIGEST_COMPRESS_THRESHOLD, self.relativeError, self.count, len(self.sampled))]
        for v, g, delta in self.sampled:
            out.append(struct.pack(">dii", v, g, delta))
        return b"".join(out)

    @classmethod
    def deserialize(cls, b: bytes) -> "PercentileDigest":
        _, eps, count, n = struct.unpack_from(">idqi", b, 0)
        entries = [struct.unpack_from(">dii", b, 24 + 16 * k) for k in range(n)]
        return cls.from_entries(eps, count, entries)

    def signature(self) -> tuple:
        """Bit for bit: relativeError, count and every entry (values as their bits, so NaN and -0.0
        compare as what they are)."""
        return (struct.pack("<d", self.relativeError), self.count,
                tuple((struct.pack("<d", v), g, delta) for v, g, delta in self.sampled))

    def __eq__(self, o):
        return isinstance(o, PercentileDigest) and o.signature() == self.signature()

    def __hash__(self):
        return hash(self.signature())

    def __repr__(self):
        return "PercentileDigest(relativeError=%r,count=%d,entries=%d)" % (self.relativeError, self.count,
                                                                           len(self.sampled))


class ApproxQuantileState(State):
    """ApproxQuantileState(percentileDigest) (ApproxQuantile.scala:29-37)."""

    def __init__(self, percentileDigest: PercentileDigest):
        self.percentileDigest = percentileDigest

    def sum(self, other: "ApproxQuantileState") -> "ApproxQuantileState":
        if not isinstance(other, ApproxQuantileState):
            raise TypeError("cannot sum ApproxQuantileState with %s" % type(other).__name__)
        # (the reference merges into this.percentileDigest in place; a copy keeps a persisted state intact)
        return ApproxQuantileState(self.percentileDigest.copy().merge(other.percentileDigest))

    __add__ = sum

    def metricValue(self):
        raise TypeError("ApproxQuantileState is not a DoubleValuedState")

    def to_dq(self):
        raise TypeError("ApproxQuantileState has no POD image: it travels through dq_aq_export")

    def __eq__(self, o):
        return isinstance(o, ApproxQuantileState) and o.percentileDigest == self.percentileDigest

    def __hash__(self):
        return hash(self.percentileDigest)

    def __repr__(self):
        return "ApproxQuantileState(%r)" % self.percentileDigest


_BY_KIND = {
    L.DQ_OP_SIZE: NumMatches,
    L.DQ_OP_COMPLETENESS: NumMatchesAndCount,
    L.DQ_OP_COMPLIANCE: NumMatchesAndCount,
    L.DQ_OP_SUM: SumState,
    L.DQ_OP_MEAN: MeanState,
    L.DQ_OP_STDDEV: StandardDeviationState,
    L.DQ_OP_MINIMUM: MinState,
    L.DQ_OP_MAXIMUM: MaxState,
    L.DQ_OP_APPROX_COUNT_DISTINCT: ApproxCountDistinctState,
    L.DQ_OP_DATATYPE: DataTypeHistogram,
    L.DQ_OP_MIN_LENGTH: MinState,  # MinLength's state is a MinState (MinLength.scala:26)
    L.DQ_OP_MAX_LENGTH: MaxState,
    L.DQ_OP_CORRELATION: CorrelationState,
    L.DQ_OP_PATTERN_MATCH: NumMatchesAndCount,  # PatternMatch.scala:38
}


def state_from_dq(s: L.DqState) -> Optional[State]:
    """POD state from dq_plan_finish -> Option[State] (has_value = 0 is None)."""
    if not s.has_value:
        return None
    return _BY_KIND[s.kind].from_dq(s)


def merge(*states: Optional[State]) -> Optional[State]:
    """Analyzers.merge (Analyzer.scala:367-386)."""
    acc = None
    for s in states:
        if acc is None:
            acc = s
        elif s is not None:
            acc = acc.sum(s)
    return acc
