"""Shared by the edge-value tests (ORDER BY, expressions, aggregates): the value pools at the null,
NaN and Long edges, and a pure-Python ORDER BY that shares nothing with the device kernels or with
oracle/relational.py.

The reference sort follows DESIGN.md "Value semantics at the edges":
  - ASC puts nulls first, DESC last; a null ties with every other null on that key, whatever word
    lies under it, so the next key decides and then the input order (the sort is stable);
  - Doubles order as -inf < .. < -0.0 < 0.0 < .. < +inf < NaN, and every NaN bit pattern is one value.
Each key column is mapped to dense integer ranks with an explicit comparator over its distinct
values; the ranks are negated for DESC, the null rank goes in front, and Python's stable ``sorted``
orders the row numbers by the tuples.
"""
import functools
import math
import struct

import numpy as np

I64, BOOL, F64, STR = 0, 1, 2, 3

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1

# quiet NaN, the sign-bit NaN x86 makes of inf - inf, a signalling payload, all ones
NAN_BITS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF)


def f64_bits(bits) -> np.ndarray:
    """float64 array holding exactly these 64-bit patterns"""
    return np.array(list(bits), dtype=np.uint64).view(np.float64)


def f64_pool_sort() -> np.ndarray:
    """ORDER BY's Double edges"""
    plain = np.array([0.0, -0.0, np.inf, -np.inf, 1e300, -1e300, 5e-324], dtype=np.float64)
    return np.concatenate([plain, f64_bits(NAN_BITS)])


def f64_pool_expr() -> np.ndarray:
    plain = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 63, -(2.0 ** 63), 1e300, -1e300,
                      5e-324, np.inf, -np.inf], dtype=np.float64)
    return np.concatenate([plain, f64_bits(NAN_BITS)])


def i64_pool() -> np.ndarray:
    return np.array([0, 1, -1, 2 ** 31 - 1, 2 ** 31, -(2 ** 31), 2 ** 53, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62,
                     INT64_MAX, INT64_MAX - 1, INT64_MIN, 3, -7, 18, 64, 65], dtype=np.int64)


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def compare(ty: int, a, b) -> int:
    """-1 / 0 / 1 under the type's total order (Python ints, or floats for F64)"""
    if ty == F64:
        an, bn = math.isnan(a), math.isnan(b)
        if an or bn:
            return 0 if (an and bn) else (1 if an else -1)
        if a < b:
            return -1
        if a > b:
            return 1
        sa, sb = math.copysign(1.0, a), math.copysign(1.0, b)  # -0.0 below 0.0
        return -1 if sa < sb else (1 if sa > sb else 0)
    return -1 if a < b else (1 if a > b else 0)


def dense_ranks(ty: int, values, valid):
    """rank (>= 1) of each valid row's value among the column's distinct values; 0 under a null"""
    n = len(values)
    ok = [True] * n if valid is None else [bool(x) for x in valid]
    py = [(float(v) if ty == F64 else int(v)) for v in values]
    ident = (lambda x: bits_of(x)) if ty == F64 else (lambda x: x)
    distinct = {}
    for r in range(n):
        if ok[r]:
            distinct.setdefault(ident(py[r]), py[r])
    ordered = sorted(distinct.items(), key=functools.cmp_to_key(lambda p, q: compare(ty, p[1], q[1])))
    rank_of, rank, prev = {}, 0, None
    for key, v in ordered:
        if prev is None or compare(ty, prev, v) != 0:
            rank += 1
        rank_of[key] = rank
        prev = v
    return [rank_of[ident(py[r])] if ok[r] else 0 for r in range(n)]


def reference_order(columns, items):
    """Row permutation of ORDER BY ``items`` ((name, "asc" | "desc"), ...) over ``columns`` (objects with
    name, type, values, valid): position i of the result holds the input row that sorts i-th."""
    by_name = {c.name: c for c in columns}
    n = len(columns[0].values) if columns else 0
    parts = []
    for name, order in items:
        c = by_name[name]
        desc = order.lower().startswith("desc")
        ranks = dense_ranks(c.type, c.values, c.valid)
        if desc:  # nulls last, values descending
            parts.append([(1, 0) if r == 0 else (0, -r) for r in ranks])
        else:  # nulls first
            parts.append([(0, 0) if r == 0 else (1, r) for r in ranks])
    return sorted(range(n), key=lambda r: tuple(p[r] for p in parts))


def hidden_words(rng, n, ty):
    """random non-zero words to lie under nulls"""
    w = rng.integers(1, 1 << 62, n, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), n)
    return w.view(np.float64) if ty == F64 else w


def _nullable(rng, vals, ty, frac):
    n = len(vals)
    valid = rng.random(n) >= frac
    return np.where(valid, vals, hidden_words(rng, n, ty)), valid


N_ORDER = 10_007  # crosses the 4096-key sort tile, ragged


def order_cases(dictionary):
    """[(case id, columns, items)]: host tables for ORDER BY, each with the row-id column ``i``."""
    from capsmi import ColumnData
    n = N_ORDER
    cases = []

    def ids():
        return ColumnData("i", I64, np.arange(n, dtype=np.int64), None)

    for ty, tname in ((I64, "long"), (F64, "double")):
        rng = np.random.default_rng(100 + ty)
        if ty == I64:
            k = rng.integers(-3, 4, n).astype(np.int64)
        else:
            k = rng.choice(np.concatenate([f64_pool_sort(), [-2.5, 0.25, 7.0]]), n)
        kv, kvalid = _nullable(rng, k, ty, 0.3)
        v = rng.integers(0, 40, n).astype(np.int64)
        cols = [ColumnData("k", ty, kv, kvalid), ColumnData("v", I64, v, None), ids()]
        for ko in ("asc", "desc"):
            for vo in ("asc", "desc"):
                cases.append((f"hidden_{tname}_{ko}_{vo}", cols, [("k", ko), ("v", vo)]))

    rng = np.random.default_rng(7)
    strings = ["", "a", "ab", "b", "zz"]
    dictionary.extend(strings)
    codes = np.array([dictionary.encode(s) for s in strings], dtype=np.int64)
    kk, kkv = _nullable(rng, rng.choice(np.array([INT64_MIN, -1, 0, 5, INT64_MAX], dtype=np.int64), n), I64, 0.2)
    ff, ffv = _nullable(rng, rng.choice(np.concatenate([f64_bits(NAN_BITS[:2]), [-0.0, 0.0, 1.5, -np.inf]]), n), F64, 0.2)
    ss, ssv = _nullable(rng, codes[rng.integers(0, len(codes), n)], STR, 0.2)
    bb, bbv = _nullable(rng, rng.integers(0, 2, n).astype(np.int64), BOOL, 0.2)
    mixed = [ColumnData("k", I64, kk, kkv), ColumnData("f", F64, ff, ffv), ColumnData("s", STR, ss, ssv),
             ColumnData("b", BOOL, bb, bbv), ids()]
    cases.append(("mixed_s_f_b", mixed, [("s", "asc"), ("f", "desc"), ("b", "asc")]))
    cases.append(("mixed_k_b_f", mixed, [("k", "desc"), ("b", "desc"), ("f", "asc")]))
    cases.append(("mixed_b_s_k", mixed, [("b", "asc"), ("s", "desc"), ("k", "asc")]))

    rng = np.random.default_rng(11)
    pool = f64_pool_sort()
    e = rng.choice(pool, n)  # every edge value many times over
    ev, evalid = _nullable(rng, e, F64, 0.1)
    for cname, col in (("edges_double", ColumnData("k", F64, e, None)),
                       ("edges_double_nullable", ColumnData("k", F64, ev, evalid))):
        for o in ("asc", "desc"):
            cases.append((f"{cname}_{o}", [col, ids()], [("k", o)]))

    ext = np.array([INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX], dtype=np.int64)
    lk = rng.choice(ext, n)
    for o in ("asc", "desc"):
        cases.append((f"edges_long_{o}", [ColumnData("k", I64, lk, None), ids()], [("k", o)]))
    return cases


# ---- the NaN truth table of comparisons, written out by hand (Spark SQL "NaN Semantics") ----------------
T, F, N = True, False, None
NAN, NEG_NAN, SNAN, ONES = (float(x) for x in f64_bits(NAN_BITS))
INF = math.inf


def _keep_bits(values):
    """float64 column that keeps each NaN's bits"""
    return np.array([np.float64(v) for v in values], dtype=np.float64)


# (a, b) -> = <> < <= > >=
NAN_TRUTH = [
    (NAN, NEG_NAN, (T, F, F, T, F, T)),   # NaN = NaN whatever its bits
    (SNAN, ONES, (T, F, F, T, F, T)),
    (NEG_NAN, 2.0, (F, T, F, F, T, T)),   # NaN is greater than any number, sign bit or not
    (NAN, INF, (F, T, F, F, T, T)),
    (1.0, NAN, (F, T, T, T, F, F)),
    (INF, NEG_NAN, (F, T, T, T, F, F)),
    (-INF, NAN, (F, T, T, T, F, F)),
    (None, NAN, (N, N, N, N, N, N)),      # a null operand still gives NULL
    (NEG_NAN, None, (N, N, N, N, N, N)),
    (-0.0, 0.0, (T, F, F, T, F, T)),      # comparisons go by value: the sort alone tells the zeros apart
]
OPS = ("=", "<>", "<", "<=", ">", ">=")


def nan_truth_columns():
    a = _keep_bits([0.0 if x is None else x for x, _, _ in NAN_TRUTH])
    b = _keep_bits([0.0 if y is None else y for _, y, _ in NAN_TRUTH])
    av = np.array([x is not None for x, _, _ in NAN_TRUTH], bool)
    bv = np.array([y is not None for _, y, _ in NAN_TRUTH], bool)
    return [("a", F64, a, av), ("b", F64, b, bv)]
