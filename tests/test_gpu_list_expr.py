"""List expressions on the device: size(), list[i], x IN list-column (CAPSMI_X_SIZE / INDEX / IN_LIST) and
range() (capsmi_with_range_column).  The golden cases of tests/golden/list_expr.json run through the planner;
the operators are compared, exactly and in row order, with the pure-Python restatement of list_expr_ref.py over
the rows the table exports.  Shapes are built around T, the tile of virtual (row, position) slots."""
import json
import math
import zlib

import numpy as np
import pytest

from golden_util import load_cases, run_planner, same_rows
from list_expr_ref import T, ref_in_list, ref_index, ref_range, ref_size

pytestmark = pytest.mark.gpu

CASES = load_cases("list_expr.json")
PY = {"I64": int, "F64": float, "BOOL": bool, "STR": str}


# ---- golden cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["routed", "unfused"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden(session, case, fused):
    session.set_fused(fused)
    try:
        got = run_planner(session, case)
    finally:
        session.set_fused(True)
    assert same_rows(got, case["expected"]), json.dumps(got)


# ---- helpers ---------------------------------------------------------------------------------------
def _words(session, elem_name, values):
    if elem_name == "F64":
        return np.asarray(values, dtype=np.float64).view(np.int64)
    if elem_name == "STR":
        session.dictionary.extend(sorted(set(values)))
        return np.array([session.dictionary.encode(x) for x in values], dtype=np.int64)
    return np.asarray([int(x) for x in values], dtype=np.int64)


def _table(session, lists, valid, elem_name, cols=()):
    """A table of len(lists) rows: id, the columns `cols`, and the list column xs.  `lists` are the stored lists
    (a null row may store elements: they must not be seen)."""
    from capsmi import ColumnData, expr
    n = len(lists)
    offs = np.zeros(n + 1, dtype=np.int64)
    if n:
        np.cumsum([len(x) for x in lists], out=offs[1:])
    flat = [v for x in lists for v in x]
    t = session.table([ColumnData("id", expr.I64, np.arange(n, dtype=np.int64))] + list(cols))
    return t.add_list_column_csr("xs", getattr(expr, elem_name), offs, _words(session, elem_name, flat),
                                 None if valid is None else np.asarray(valid, dtype=np.uint8))


def _values(session, t, name):
    """Column `name` as Python values, None for NULL."""
    from capsmi.table import decode_value
    c = t.column(name)
    return [None if (c.valid is not None and not c.valid[r]) else decode_value(c.type, c.values[r], session.dictionary)
            for r in range(len(c.values))]


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return type(a) is type(b) and a == b


def _assert_same(got, want):
    assert len(got) == len(want)
    bad = [(r, g, w) for r, (g, w) in enumerate(zip(got, want)) if not _same(g, w)]
    assert not bad, bad[:10]


def _i64(name, values, valid=None):
    from capsmi import ColumnData, expr
    return ColumnData(name, expr.I64, np.asarray(values, dtype=np.int64), None if valid is None else np.asarray(valid, dtype=bool))


# ---- size() and list[i] ------------------------------------------------------------------------------
def _random_lists(rng, elem_name, n, maxlen=6):
    pool = {"I64": lambda: int(rng.integers(-(1 << 40), 1 << 40)), "F64": lambda: float(np.round(rng.standard_normal(), 3)),
            "BOOL": lambda: bool(rng.integers(0, 2)), "STR": lambda: f"s{int(rng.integers(0, 30)):02d}"}[elem_name]
    return [[pool() for _ in range(int(rng.integers(0, maxlen + 1)))] for _ in range(n)]


def _check_size_index(session, t):
    """Size / Index over the materialised table t (columns id, xs, i) against the restatement of its rows."""
    from capsmi.expr import BinOp, Col, Index, Lit, Size
    t.size  # materialise: the row order is fixed from here on
    xs, idx = _values(session, t, "xs"), _values(session, t, "i")
    out = t.withColumns((Size(Col("xs")), "s"), (Index(Col("xs"), Col("i")), "e"),
                        (Index(Col("xs"), BinOp("+", Col("i"), Lit(1))), "e1"), (Index(Col("xs"), Lit(0)), "e0"))
    assert out.columnType["s"] == 0 and out.columnType["e"] == t.columnType["xs"] - 8
    _assert_same(_values(session, out, "id"), _values(session, t, "id"))
    _assert_same(_values(session, out, "s"), [ref_size(x) for x in xs])
    _assert_same(_values(session, out, "e"), [ref_index(x, i) for x, i in zip(xs, idx)])
    _assert_same(_values(session, out, "e1"), [ref_index(x, None if i is None else i + 1) for x, i in zip(xs, idx)])
    _assert_same(_values(session, out, "e0"), [ref_index(x, 0) for x in xs])
    return len(xs)


def _index_table(session, rng, elem_name, n):
    lists = _random_lists(rng, elem_name, n)
    lists[0], lists[1] = [], lists[1] or lists[2] or _random_lists(rng, elem_name, 1, 1)[0]
    valid = rng.random(n) >= 0.25  # null rows keep their stored elements
    valid[0] = True
    sizes = np.array([len(x) for x in lists])
    idx = np.select([np.arange(n) % 5 == k for k in range(5)], [np.full(n, -1), np.zeros(n, dtype=np.int64), sizes - 1, sizes,
                                                                 rng.integers(-2, 8, n)])
    iv = rng.random(n) >= 0.15  # a NULL index
    return _table(session, lists, valid, elem_name, [_i64("i", idx, iv)])


@pytest.mark.parametrize("elem_name", ["I64", "F64", "BOOL", "STR"])
def test_size_and_index(session, elem_name):
    rng = np.random.default_rng(zlib.crc32(elem_name.encode()))
    assert _check_size_index(session, _index_table(session, rng, elem_name, 700)) == 700


def test_size_and_index_without_rows(session):
    from capsmi.expr import Col, Index, Lit, Size
    t = _table(session, [], None, "I64", [_i64("i", [])])
    out = t.withColumns((Size(Col("xs")), "s"), (Index(Col("xs"), Lit(0)), "e"))
    assert out.size == 0 and out.physicalColumns == ["id", "i", "xs", "s", "e"]


def test_size_and_index_after_filter_and_order(session):
    from capsmi.expr import BinOp, Col, Lit
    rng = np.random.default_rng(5)
    t = _index_table(session, rng, "I64", 900)
    assert 0 < _check_size_index(session, t.filter(BinOp(">", Col("i"), Lit(-1)))) < 900
    assert _check_size_index(session, t.orderBy(("i", "desc"), ("id", "asc")).skip(3)) == 897


def test_size_and_index_after_union_of_two_stores(session):
    rng = np.random.default_rng(6)
    a, b = _index_table(session, rng, "F64", 300), _index_table(session, rng, "F64", 200)
    assert _check_size_index(session, a.unionAll(b)) == 500


def test_size_and_index_after_a_join_that_repeats_list_rows(session):
    from capsmi import ColumnData, expr
    rng = np.random.default_rng(7)
    t = _index_table(session, rng, "STR", 60).drop("i")
    left = session.table([ColumnData("k", expr.I64, rng.integers(0, 70, 500).astype(np.int64)),
                          _i64("i", rng.integers(-1, 7, 500), rng.random(500) >= 0.1)])
    j = left.join(t, "inner", ("k", "id"))
    assert _check_size_index(session, j) > 300


# ---- x IN list-column: shapes ------------------------------------------------------------------------
def _check_in(session, t, elem_name="I64", probe=None, restate=None):
    """InList(probe, xs) over the materialised table t (columns id, p, xs), exact and in row order."""
    from capsmi.expr import Col, InList
    t.size
    xs, p = _values(session, t, "xs"), _values(session, t, "p")
    want = [ref_in_list((restate or (lambda v: v))(x), lst, PY[elem_name]) for x, lst in zip(p, xs)]
    out = t.withColumns((InList(probe if probe is not None else Col("p"), Col("xs")), "m"))
    assert out.columnType["m"] == 1
    _assert_same(_values(session, out, "id"), _values(session, t, "id"))
    _assert_same(_values(session, out, "m"), want)
    return want


def _distinct_list(k, base=0):
    return list(range(base, base + 2 * k, 2))  # k even numbers: an odd probe is absent


IN_SHAPES = ["no_rows", "all_empty_or_null", "long_list_last_first_none", "tile_boundaries", "one_4T_among_empty"]


@pytest.mark.parametrize("shape", IN_SHAPES)
def test_in_list_shapes(session, shape):
    rng = np.random.default_rng(zlib.crc32(shape.encode()))
    valid = None
    if shape == "no_rows":
        lists, probes = [], []
    elif shape == "all_empty_or_null":
        lists = [[], [2, 4, 6], [], [], [8, 10], [], [0] * 7, []]
        valid = [len(x) == 0 for x in lists]  # every non-empty row is null
        probes = [2, 2, 0, 1, 8, 3, 0, 5]
    elif shape == "long_list_last_first_none":
        k = 3 * T + 5
        lists = [_distinct_list(k), _distinct_list(k), _distinct_list(k)]
        probes = [2 * (k - 1), 0, 2 * k]  # the only match is the last element, the first, none
    elif shape == "tile_boundaries":  # list boundaries at T, T + 1, 2T - 1, 2T, 3T, ...; row 1 starts at a tile's slot 0
        lens = [T, 1, T - 2, 1, T, 1, T - 2, 2 * T, 1, 9]
        lists = [_distinct_list(l, 10 * i) for i, l in enumerate(lens)]
        # alternately the list's last element (present) and an odd number (absent)
        probes = [x[-1] if i % 2 == 0 else x[0] + 1 for i, x in enumerate(lists)]
    else:  # one list of 4T elements among 2000 empty rows
        lists = [[] for _ in range(1000)] + [_distinct_list(4 * T)] + [[] for _ in range(1000)]
        probes = rng.integers(0, 100, 2001).tolist()
        probes[1000] = 2 * (4 * T - 1)
    t = _table(session, lists, valid, "I64", [_i64("p", probes)])
    want = _check_in(session, t)
    if shape == "long_list_last_first_none":
        assert want == [True, True, False]
    if shape == "tile_boundaries":
        assert want == [i % 2 == 0 for i in range(10)]
    if shape == "one_4T_among_empty":
        assert want[1000] is True and not any(want[:1000]) and not any(want[1001:])
    if shape == "all_empty_or_null":
        assert want == [False, None, False, False, None, False, None, False]


def test_in_list_one_list_referenced_by_300_rows(session):
    """A join repeats one list index in 300 rows with different probes, half present and half absent."""
    from capsmi import ColumnData, expr
    one = _table(session, [_distinct_list(T + 77)], None, "I64")
    probes = [2 * i if i % 2 == 0 else 2 * i + 1 for i in range(300)]
    left = session.table([ColumnData("k", expr.I64, np.zeros(300, dtype=np.int64)), _i64("p", probes)])
    want = _check_in(session, left.join(one, "inner", ("k", "id")))
    assert sorted(want) == [False] * 150 + [True] * 150


def test_in_list_after_union_and_filter(session):
    from capsmi.expr import BinOp, Col, Lit
    rng = np.random.default_rng(8)
    mk = lambda n: _table(session, [rng.integers(0, 20, int(rng.integers(0, 9))).tolist() for _ in range(n)],  # noqa: E731
                          rng.random(n) >= 0.2, "I64", [_i64("p", rng.integers(0, 20, n), rng.random(n) >= 0.1)])
    u = mk(600).unionAll(mk(500)).filter(BinOp("<>", Col("p"), Lit(3)))
    want = _check_in(session, u)
    assert {True, False, None} == set(want)


def test_in_list_in_a_table_at_the_column_limit(session):
    """70 columns: the temporary membership column cannot be appended below the interpreter's 64-column limit."""
    from capsmi.expr import Ands, BinOp, Col, InList, Lit
    rng = np.random.default_rng(14)
    n = 300
    fill = [_i64(f"f{k}", np.full(n, k)) for k in range(70)]
    lists = [rng.integers(0, 9, int(rng.integers(0, 6))).tolist() for _ in range(n)]
    t = _table(session, lists, None, "I64", [_i64("p", rng.integers(0, 9, n))] + fill)
    t = t.select("id", "p", "xs", *[f"f{k}" for k in range(70)])
    want = [ref_in_list(x, lst, int) for x, lst in zip(_values(session, t, "p"), _values(session, t, "xs"))]
    out = t.withColumns((Ands((InList(Col("p"), Col("xs")), BinOp("=", Col("f0"), Lit(0)))), "m"))
    assert len(out.physicalColumns) == 74
    _assert_same(_values(session, out, "m"), want)
    for k in (0, 1, 60, 61, 69):  # the input columns are what they were
        assert _values(session, out, f"f{k}") == [k] * n


# ---- x IN list-column: value semantics ---------------------------------------------------------------
def test_in_list_null_probe_null_list_and_computed_probe(session):
    from capsmi.expr import BinOp, Col, Lit
    lists = [[2, 4], [2, 4], [2, 4], [], [6]]
    t = _table(session, lists, [True, True, False, True, True], "I64", [_i64("p", [1, 2, 1, 1, 3], [True, False, True, True, True])])
    assert _check_in(session, t) == [False, None, None, False, False]
    want = _check_in(session, t, probe=BinOp("*", Col("p"), Lit(2)), restate=lambda v: None if v is None else 2 * v)
    assert want == [True, None, None, False, True]


def test_in_list_nan_and_long_against_double(session):
    from capsmi import ColumnData, expr
    nan = float("nan")
    lists = [[1.5, nan], [1.5, 2.5], [float(2 ** 53)], [float(2 ** 53)], [-0.0]]
    pf = ColumnData("p", expr.F64, np.array([nan, nan, 1.0, 2.0 ** 53, 0.0]))
    assert _check_in(session, _table(session, lists, None, "F64", [pf]), "F64") == [True, False, False, True, True]
    # a Long probe against a Double list compares as doubles: 2^53 + 1 = 2^53.0
    pl = _i64("p", [1, 2, 2 ** 53 + 1, 2 ** 53 + 2, 0])
    assert _check_in(session, _table(session, lists, None, "F64", [pl]), "F64") == [False, False, True, False, True]
    # a Double probe against a Long list
    t = _table(session, [[1, 2], [3]], None, "I64", [ColumnData("p", expr.F64, np.array([2.0, 3.5]))])
    assert _check_in(session, t) == [True, False]


def test_in_list_strings_and_incomparable_types(session):
    from capsmi import ColumnData, expr
    lists = [["a", "b"], ["c"], [], ["b"]]
    session.dictionary.extend(["a", "b", "c", "zz"])
    codes = np.array([session.dictionary.encode(x) for x in ["b", "a", "a", "zz"]], dtype=np.int64)
    t = _table(session, lists, None, "STR", [ColumnData("p", expr.STR, codes)])
    assert _check_in(session, t, "STR") == [True, False, False, False]
    # a Long probe against a STR list is NULL, as `=` gives -- for an empty list too
    t = _table(session, lists, None, "STR", [_i64("p", [1, 2, 3, 4])])
    assert _check_in(session, t, "STR") == [None, None, None, None]


def test_in_list_as_a_filter_and_inside_ands_and_not(session):
    from capsmi.expr import Ands, BinOp, Col, InList, Lit, Not
    rng = np.random.default_rng(9)
    n = 1500
    lists = [rng.integers(0, 12, int(rng.integers(0, 7))).tolist() for _ in range(n)]
    t = _table(session, lists, rng.random(n) >= 0.2, "I64", [_i64("p", rng.integers(0, 12, n), rng.random(n) >= 0.1)])
    t.size
    xs, p, ids = _values(session, t, "xs"), _values(session, t, "p"), _values(session, t, "id")
    m = [ref_in_list(x, lst, int) for x, lst in zip(p, xs)]
    member = InList(Col("p"), Col("xs"))
    keep = t.filter(member)  # NULL and FALSE rows are dropped
    assert _values(session, keep, "id") == [i for i, v in zip(ids, m) if v is True]
    both = t.filter(Ands((member, BinOp(">", Col("p"), Lit(5)))))
    assert _values(session, both, "id") == [i for i, v, x in zip(ids, m, p) if v is True and x > 5]
    neg = t.filter(Not(member))  # NOT NULL is NULL: only the FALSE rows
    assert _values(session, neg, "id") == [i for i, v in zip(ids, m) if v is False]
    two = t.withColumns((Ands((member, Not(InList(BinOp("+", Col("p"), Lit(1)), Col("xs"))))), "b"))
    m1 = [ref_in_list(None if x is None else x + 1, lst, int) for x, lst in zip(p, xs)]
    want = [False if (a is False or b is True) else (None if a is None or b is None else True) for a, b in zip(m, m1)]
    _assert_same(_values(session, two, "b"), want)


# ---- what stays unimplemented ------------------------------------------------------------------------
def test_list_operands_of_other_operators_are_not_implemented(session):
    from capsmi._lib import IllegalArgumentException, NotImplementedException
    from capsmi.expr import BinOp, Coalesce, Col, In, Index, Lit
    t = _table(session, [[1], [2, 3]], None, "I64", [_i64("p", [1, 2])])
    for e in (BinOp("=", Col("xs"), Lit(1)), BinOp("+", Col("xs"), Lit(1)), In(Col("xs"), (Lit(1),)),
              In(Col("p"), (Col("xs"),)), Coalesce((Col("xs"), Col("xs")))):
        with pytest.raises(NotImplementedException):
            t.withColumns((e, "x"))
    with pytest.raises(NotImplementedException):
        t.filter(BinOp("=", Col("xs"), Lit(1)))
    with pytest.raises(IllegalArgumentException):
        t.withColumns((Index(Col("xs"), Lit(1.0)), "x"))
    with pytest.raises(IllegalArgumentException):
        t.withColumns((Index(Col("p"), Lit(0)), "x"))


# ---- range() -----------------------------------------------------------------------------------------
def _check_range(session, t, start, end, step, py):
    """withRangeColumn over the materialised table t against ref_range of py(row) = (start, end, step)."""
    t.size
    cols = {c: _values(session, t, c) for c in t.physicalColumns}
    rows = [{c: cols[c][r] for c in cols} for r in range(t.size)]
    want = []
    for row in rows:
        opd = py(row)
        want.append(None if any(x is None for x in opd) else ref_range(*opd))
    out = t.withRangeColumn(start, end, step, "rg")
    assert out.columnType["rg"] == 8 and out.physicalColumns == t.physicalColumns + ["rg"]
    assert _values(session, out, "rg") == want
    return want


def test_range_columns_literals_negative_steps_and_nulls(session):
    from capsmi.expr import BinOp, Col, Lit
    rng = np.random.default_rng(10)
    n = 1200
    a, b = rng.integers(-20, 20, n), rng.integers(-20, 20, n)
    st = rng.integers(1, 5, n) * rng.choice([-1, 1], n)
    t = session.table([_i64("id", np.arange(n)), _i64("a", a, rng.random(n) >= 0.1), _i64("b", b, rng.random(n) >= 0.1),
                       _i64("st", st, rng.random(n) >= 0.1)])
    want = _check_range(session, t, Col("a"), Col("b"), Col("st"), lambda r: (r["a"], r["b"], r["st"]))
    assert any(w == [] for w in want) and any(w is None for w in want) and any(w and len(w) > 3 for w in want)
    _check_range(session, t, Col("a"), Col("b"), None, lambda r: (r["a"], r["b"], 1))
    _check_range(session, t, Lit(3), Col("b"), Lit(-2), lambda r: (3, r["b"], -2))
    _check_range(session, t, BinOp("+", Col("a"), Lit(1)), 7, 3, lambda r: (None if r["a"] is None else r["a"] + 1, 7, 3))


def test_range_replaces_a_column_of_its_name(session):
    from capsmi.expr import Col
    t = session.table([_i64("a", [1, 2]), _i64("rg", [5, 6]), _i64("z", [0, 0])])
    out = t.withRangeColumn(Col("a"), Col("rg"), None, "rg")
    assert out.physicalColumns == ["a", "rg", "z"] and _values(session, out, "rg") == [[1, 2, 3, 4, 5], [2, 3, 4, 5, 6]]


def test_range_step_zero_raises_at_the_action(session):
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Col
    st = np.ones(1000, dtype=np.int64)
    st[613] = 0
    t = session.table([_i64("a", np.zeros(1000)), _i64("st", st)])
    lazy = t.withRangeColumn(Col("a"), 3, Col("st"), "rg")  # building the node is fine
    with pytest.raises(IllegalArgumentException, match="step 0"):
        lazy.size
    with pytest.raises(IllegalArgumentException):  # a non-Long operand: when the node is built
        t.withRangeColumn(Col("a"), 2.5, None, "rg")


def test_range_beyond_the_device_is_unsupported(session):
    """Counts no device holds are refused with the count, not by the allocator."""
    from capsmi._lib import NotImplementedException, UnsupportedOperationException
    from capsmi.expr import Col, Range
    t = session.table([_i64("a", [0, 0, 0, 5]), _i64("b", [2 ** 62, 2 ** 62, 2 ** 62, 4])])
    with pytest.raises(UnsupportedOperationException, match=r"range: \d+ or more elements") as e:
        t.withRangeColumn(Col("a"), Col("b"), None, "rg").size
    assert int(str(e.value).split("range: ")[1].split()[0]) == 3 * 2 ** 40  # three saturated rows, one empty
    one = session.table([_i64("a", [-2 ** 63]), _i64("b", [2 ** 63 - 1])])
    with pytest.raises(UnsupportedOperationException, match="or more elements"):
        one.withRangeColumn(Col("a"), Col("b"), None, "rg").size
    # below the per-row cap, above the device: the exact count
    big = session.table([_i64("a", [0, 0]), _i64("b", [2 ** 39 - 1, 2 ** 39 - 1])])
    with pytest.raises(UnsupportedOperationException, match=rf"range: {2 ** 40} elements"):
        big.withRangeColumn(Col("a"), Col("b"), None, "rg").size
    assert t.withRangeColumn(Col("a"), 3, None, "rg").size == 4  # the session goes on working
    with pytest.raises(NotImplementedException, match="Range"):
        t.filter(Range(Col("a"), Col("b")))


def test_range_long_edges(session):
    from capsmi.expr import Col
    lo, hi = -2 ** 63, 2 ** 63 - 1
    t = session.table([_i64("a", [lo, hi - 2, hi, lo]), _i64("b", [hi, hi, hi - 2, lo]), _i64("st", [2 ** 62, 1, -1, lo])])
    want = _check_range(session, t, Col("a"), Col("b"), Col("st"), lambda r: (r["a"], r["b"], r["st"]))
    assert [len(w) for w in want] == [4, 3, 3, 1]


@pytest.mark.parametrize("shape", ["one_long_among_empty_and_null", "multiple_of_tile"])
def test_range_tiles(session, shape):
    from capsmi.expr import Col
    if shape == "one_long_among_empty_and_null":
        n = 1500
        a, b = np.full(n, 5), np.full(n, 4)  # empty
        b[700] = 5 + 3 * T + 4               # one range of 3T + 5
        ok = np.arange(n) % 3 != 0
        ok[700] = True
    else:  # totals T, then more rows to 3T
        lens = [700, 1348, T, 1, T - 1]
        n = len(lens)
        a = np.arange(n) * 10
        b = a + np.array(lens) - 1
        ok = np.ones(n, dtype=bool)
    t = session.table([_i64("a", a, ok), _i64("b", b)])
    want = _check_range(session, t, Col("a"), Col("b"), None, lambda r: (r["a"], r["b"], 1))
    total = sum(len(w) for w in want if w)
    assert total == (3 * T + 5 if shape == "one_long_among_empty_and_null" else 3 * T)


def test_explode_of_range_is_the_concatenated_aranges(session):
    from capsmi.expr import Col, Explode, Range
    rng = np.random.default_rng(11)
    n = 800
    a, b = rng.integers(-10, 10, n), rng.integers(-10, 30, n)
    st = rng.integers(1, 4, n)
    t = session.table([_i64("id", np.arange(n)), _i64("a", a), _i64("b", b), _i64("st", st)])
    out = t.withColumns((Explode(Range(Col("a"), Col("b"), Col("st"))), "x"))
    assert out.physicalColumns == ["id", "a", "b", "st", "x"]  # the temporary list column is gone
    pieces = [np.arange(a[r], b[r] + 1, st[r]) for r in range(n)]
    assert np.array_equal(out.column("x").values, np.concatenate(pieces))
    assert np.array_equal(out.column("id").values, np.repeat(np.arange(n), [len(p) for p in pieces]))
    assert out.size > T


def test_size_and_in_list_of_range(session):
    from capsmi.expr import BinOp, Col, InList, Lit, Range, Size
    from capsmi._lib import NotImplementedException
    rng = np.random.default_rng(12)
    n = 900
    a, b, p = rng.integers(-10, 10, n), rng.integers(-10, 30, n), rng.integers(-12, 32, n)
    t = session.table([_i64("id", np.arange(n)), _i64("a", a), _i64("b", b, rng.random(n) >= 0.1), _i64("p", p)])
    bv = _values(session, t, "b")
    out = t.withColumns((Size(Range(Col("a"), Col("b"))), "s"), (InList(Col("p"), Range(Col("a"), Col("b"), Lit(3))), "m"),
                        (Range(Col("a"), Lit(2)), "r"), (Size(Col("r")), "sr"))  # the columns after a Range see it
    assert out.physicalColumns == ["id", "a", "b", "p", "s", "m", "r", "sr"]
    _assert_same(_values(session, out, "s"), [None if y is None else len(ref_range(int(x), y)) for x, y in zip(a, bv)])
    _assert_same(_values(session, out, "m"),
                 [None if y is None else int(q) in ref_range(int(x), y, 3) for x, y, q in zip(a, bv, p)])
    _assert_same(_values(session, out, "sr"), [len(ref_range(int(x), 2)) for x in a])
    kept = t.filter(InList(Col("p"), Range(Col("a"), Col("b"))))
    assert kept.physicalColumns == ["id", "a", "b", "p"]
    assert _values(session, kept, "id") == [r for r in range(n) if bv[r] is not None and a[r] <= p[r] <= bv[r]]
    with pytest.raises(NotImplementedException):
        t.withColumns((BinOp("=", Range(Col("a"), Col("b")), Lit(1)), "x"))


# ---- routing and determinism -------------------------------------------------------------------------
@pytest.mark.parametrize("where", [["in_list", ["prop", "b", "k"], ["prop", "a", "xs"]],
                                   ["in_list", ["prop", "a", "k"], ["prop", "a", "xs"]]], ids=["two_nodes", "one_node"])
def test_in_list_filter_keeps_the_expand_route(session, where):
    """A filter with InList above MATCH (a)-[r]->(b): the plan under it is routed as it is without it."""
    create = "CREATE (:A {xs: [1, 3], k: 1})-[:T]->(:B {xs: [7], k: 3})-[:T]->(:C {xs: [5], k: 4})"
    ret = {"items": [["a", ["entity", "a"]]]}
    plain = {"create": create, "query": {"clauses": [{"match": "(a)-[r]->(b)"}], "return": ret}}
    filt = {"create": create, "query": {"clauses": [{"match": "(a)-[r]->(b)", "where": where}], "return": ret}}
    names = ("expand", "expand_count", "two_hop", "triangle", "var_length", "miss")

    def routes(c):
        before = [session.route_count(n) for n in names]
        rows = run_planner(session, c)
        return [session.route_count(n) - b for n, b in zip(names, before)], rows

    d_plain, rows_plain = routes(plain)
    d_filter, rows_filter = routes(filt)
    assert d_filter == d_plain
    assert len(rows_plain) == 2
    assert [r["a"]["labels"] for r in rows_filter] == [["A"]]  # (A)->(B): 3 IN [1, 3], and 1 IN [1, 3]; B's own 3 is not in [7]


def test_fingerprint_is_equal_across_two_runs(session):
    from capsmi.expr import Col, Index, InList, Lit, Range, Size

    def run():
        rng = np.random.default_rng(13)
        n = 3000
        lists = [rng.integers(0, 50, int(rng.integers(0, 40))).tolist() for _ in range(n)]
        t = _table(session, lists, rng.random(n) >= 0.2, "I64",
                   [_i64("p", rng.integers(0, 50, n), rng.random(n) >= 0.1), _i64("i", rng.integers(-1, 40, n))])
        out = t.withColumns((Size(Col("xs")), "s"), (Index(Col("xs"), Col("i")), "e"), (InList(Col("p"), Col("xs")), "m"),
                            (Size(Range(Lit(0), Col("p"), Lit(2))), "rs"), (InList(Col("i"), Range(Col("p"), Lit(45))), "rm"))
        return out.fingerprint(["id", "s", "e", "m", "rs", "rm"])

    a, b = run(), run()
    assert a == b and a[0] == 3000
