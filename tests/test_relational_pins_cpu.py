"""Literal pins of the edge semantics the checker (oracle/relational.py) must have -- DESIGN.md "Value
semantics at the edges".  Every expected value below is written out by hand from Spark SQL 2.2.1's rules
(nulls first ascending / last descending; doubleToLongBits + nanSafeCompareDoubles in the sort; the SQL
programming guide's "NaN Semantics" for comparisons and Min / Max), never computed.  The last test checks
the oracle's orderBy against the pure-Python reference sort of tests/edge_ref.py on the tables the GPU
tests use, so the two CPU implementations vouch for each other before any kernel is compared."""
import math

import numpy as np
import pytest

from edge_ref import (F64, I64, INT64_MAX, NAN_BITS, NAN_TRUTH, OPS, f64_bits, nan_truth_columns, order_cases,
                      reference_order)

NAN, NEG_NAN, SNAN, ONES = f64_bits(NAN_BITS)
INF = math.inf
T, F, N = True, False, None


def _table(cols):
    from capsmi import ColumnData, StringDictionary
    from oracle.relational import NumpyBackend
    return NumpyBackend(StringDictionary()).table([ColumnData(*c) for c in cols])


def _f(values):
    """float64 column that keeps each NaN's bits"""
    return np.array([np.float64(v) for v in values], dtype=np.float64)


def _order(t, *items):
    return [int(x) for x in t.orderBy(*items).cols["i"].values]


def test_order_by_null_keys_tie_whatever_lies_under_them():
    k = np.array([5, 9, 1, 7], dtype=np.int64)
    t = _table([("k", I64, k, np.array([1, 0, 0, 1], bool)), ("v", I64, np.array([0, 1, 2, 3])),
                ("i", I64, np.arange(4))])
    assert [int(x) for x in t.orderBy(("k", "asc"), ("v", "asc")).cols["v"].values] == [1, 2, 0, 3]
    assert _order(t, ("k", "asc"), ("v", "desc")) == [2, 1, 0, 3]
    assert _order(t, ("k", "desc"), ("v", "asc")) == [3, 0, 1, 2]
    assert _order(t, ("k", "desc"), ("v", "desc")) == [3, 0, 2, 1]
    assert _order(t, ("k", "asc")) == [1, 2, 0, 3]  # one key: the nulls keep their input order
    assert _order(t, ("k", "desc")) == [3, 0, 1, 2]
    assert _order(t) == [0, 1, 2, 3]


def test_order_by_null_double_keys_tie():
    k = _f([2.0, NEG_NAN, -INF, 1.0, 1e300, NAN])
    valid = np.array([1, 0, 0, 1, 0, 0], bool)
    t = _table([("k", F64, k, valid), ("v", I64, np.array([0, 3, 2, 1, 1, 0])), ("i", I64, np.arange(6))])
    assert _order(t, ("k", "asc"), ("v", "asc")) == [5, 4, 2, 1, 3, 0]
    assert _order(t, ("k", "desc"), ("v", "desc")) == [0, 3, 1, 2, 4, 5]


def test_order_by_double_total_order_nan_greatest():
    #          0    1    2     3     4        5    6    7    8     9
    k = _f([NAN, 1.0, -INF, -0.0, NEG_NAN, 0.0, INF, NAN, SNAN, -1e300])
    valid = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1, 1], bool)  # row 7: a null with a NaN under it
    t = _table([("k", F64, k, valid), ("i", I64, np.arange(10))])
    assert _order(t, ("k", "asc")) == [7, 2, 9, 3, 5, 1, 6, 0, 4, 8]
    assert _order(t, ("k", "desc")) == [0, 4, 8, 6, 1, 5, 3, 9, 2, 7]


def test_order_by_nans_tie_and_fall_to_the_next_key():
    k = _f([ONES, NAN, 3.0, NEG_NAN, SNAN])
    t = _table([("k", F64, k, None), ("v", I64, np.array([4, 3, 9, 2, 1])), ("i", I64, np.arange(5))])
    assert _order(t, ("k", "asc"), ("v", "asc")) == [2, 4, 3, 1, 0]
    assert _order(t, ("k", "desc"), ("v", "asc")) == [4, 3, 1, 0, 2]


def test_order_by_long_extremes():
    k = np.array([0, INT64_MAX, -(1 << 63), -1, INT64_MAX - 1, -(1 << 63) + 1, 1], dtype=np.int64)
    t = _table([("k", I64, k, None), ("i", I64, np.arange(7))])
    assert _order(t, ("k", "asc")) == [2, 5, 3, 0, 6, 4, 1]
    assert _order(t, ("k", "desc")) == [1, 4, 6, 0, 3, 5, 2]


def _tv(t, e):
    """three-valued result of a predicate: True / False / None per row"""
    from oracle.relational import BOOL, evaluate
    ty, v, m = evaluate(e, t)
    assert ty == BOOL
    return [(bool(x) if ok else None) for x, ok in zip(v, m)]


def test_comparisons_with_nan():
    from capsmi.expr import BinOp, Col, Lit
    t = _table(nan_truth_columns())
    for j, op in enumerate(OPS):
        assert _tv(t, BinOp(op, Col("a"), Col("b"))) == [row[2][j] for row in NAN_TRUTH], op
    # the same against literals
    assert _tv(t, BinOp("=", Col("a"), Lit(float("nan")))) == [T, T, T, T, F, F, F, N, T, F]
    assert _tv(t, BinOp("<", Col("a"), Lit(float("nan")))) == [F, F, F, F, T, T, T, N, F, T]
    assert _tv(t, BinOp(">", Lit(float("nan")), Col("a"))) == [F, F, F, F, T, T, T, N, F, T]


def test_in_with_nan_and_mixed_numbers():
    from capsmi.expr import Col, In, Lit
    x = _f([NAN, 1.0, 0.0, NEG_NAN, 2.0])
    t = _table([("x", F64, x, np.array([1, 1, 0, 1, 1], bool)),
                ("l", I64, np.array([1, 2, 2 ** 53 + 1, 0, -1], dtype=np.int64), None)])
    nan = Lit(float("nan"))
    assert _tv(t, In(Col("x"), (nan, Lit(2.0)))) == [T, F, N, T, T]
    assert _tv(t, In(Col("x"), (nan, Lit(None, F64)))) == [T, N, N, T, N]
    assert _tv(t, In(Col("x"), ())) == [F, F, N, F, F]
    assert _tv(t, In(Col("x"), (Lit(1), Lit(2)))) == [F, T, N, F, T]  # Long elements against a Double
    assert _tv(t, In(Col("l"), (Lit(1.0), Lit(2.0 ** 53)))) == [T, F, T, F, F]
    assert _tv(t, In(Col("l"), (nan,))) == [F, F, F, F, F]
    # Long against Long compares exactly: 2^53 + 1 is not in (2^53), though both are one Double
    assert _tv(t, In(Col("l"), (Lit(2 ** 53), Lit(2)))) == [F, T, F, F, F]
    assert _tv(t, In(Col("l"), (Lit(2 ** 53 + 1),))) == [F, F, T, F, F]


def test_collect_set_holds_one_nan_and_both_zeros():
    """collect(DISTINCT): every NaN is one element (Double.equals goes by doubleToLongBits); -0.0 and 0.0
    are two; nulls are skipped.  collect without DISTINCT keeps every NaN."""
    g = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2], dtype=np.int64)
    v = _f([NAN, NEG_NAN, 1.0, NAN, 1.0, 0.0, -0.0, SNAN, NEG_NAN, ONES, 7.0])
    valid = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0], bool)
    t = _table([("g", I64, g, None), ("v", F64, v, valid)])
    out = t.group(["g"], [("collect", "v", True, "set"), ("collect", "v", False, "all")])

    def show(name):
        return {int(k): [("NaN" if math.isnan(x) else (str(float(x)))) for x in xs]
                for k, xs in zip(out.cols["g"].values, out.cols[name].values)}

    assert show("set") == {0: ["-0.0", "0.0", "1.0", "NaN"], 1: ["NaN"], 2: []}
    assert {k: sorted(xs) for k, xs in show("all").items()} == \
        {0: ["-0.0", "0.0", "1.0", "1.0", "NaN", "NaN", "NaN"], 1: ["NaN", "NaN"], 2: []}
    assert show("all")[0][-3:] == ["NaN", "NaN", "NaN"]


def test_long_versus_double_compares_as_double():
    from capsmi.expr import BinOp, Col
    t = _table([("l", I64, np.array([2 ** 53 + 1, INT64_MAX, 3, -(1 << 63)], dtype=np.int64), None),
                ("d", F64, _f([2.0 ** 53, 2.0 ** 63, 3.5, NAN]), None)])
    assert _tv(t, BinOp("=", Col("l"), Col("d"))) == [T, T, F, F]  # the Long is cast to Double first
    assert _tv(t, BinOp("<", Col("l"), Col("d"))) == [F, F, T, T]
    assert _tv(t, BinOp(">=", Col("d"), Col("l"))) == [T, T, T, T]


def test_min_max_over_doubles_nan_greatest():
    g = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 4], dtype=np.int64)
    v = _f([1.0, NEG_NAN, -INF, NAN, NEG_NAN, SNAN, 7.0, INF, -INF, 0.0, ONES])
    valid = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1], bool)  # group 2: only nulls (with words under them)
    t = _table([("g", I64, g, None), ("v", F64, v, valid)])
    out = t.group(["g"], [("min", "v", False, "mn"), ("max", "v", False, "mx"), ("count", "v", False, "c")])

    def show(name):
        c = out.cols[name]
        by = {}
        for key, x, ok in zip(out.cols["g"].values, c.values, c.valid):
            by[int(key)] = None if not ok else ("NaN" if math.isnan(x) else float(x))
        return by

    assert show("mn") == {0: -INF, 1: "NaN", 2: None, 3: -INF, 4: "NaN"}
    assert show("mx") == {0: "NaN", 1: "NaN", 2: None, 3: INF, 4: "NaN"}
    assert show("c") == {0: 3.0, 1: 2.0, 2: 0.0, 3: 2.0, 4: 1.0}


def test_min_max_over_longs_unchanged():
    g = np.array([0, 0, 1, 1, 1], dtype=np.int64)
    v = np.array([INT64_MAX, -(1 << 63), 5, -5, 77], dtype=np.int64)
    t = _table([("g", I64, g, None), ("v", I64, v, np.array([1, 1, 1, 1, 0], bool))])
    out = t.group(["g"], [("min", "v", False, "mn"), ("max", "v", False, "mx")])
    assert [int(x) for x in out.cols["mn"].values] == [-(1 << 63), -5]
    assert [int(x) for x in out.cols["mx"].values] == [INT64_MAX, 5]


_CASES = []


def _cases():
    if not _CASES:
        from capsmi import StringDictionary
        d = StringDictionary()
        _CASES.extend([d, order_cases(d)])
    return _CASES


@pytest.mark.parametrize("case", range(17))
def test_oracle_order_by_equals_the_pure_python_reference(case):
    from oracle.relational import NumpyBackend
    d, cases = _cases()
    assert len(cases) == 17
    name, cols, items = cases[case]
    got = NumpyBackend(d).table(cols).orderBy(*items).cols["i"].values
    np.testing.assert_array_equal(got, np.array(reference_order(cols, items), dtype=np.int64), err_msg=name)
