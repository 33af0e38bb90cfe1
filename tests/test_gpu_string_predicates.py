"""STARTS WITH / ENDS WITH / CONTAINS on the device (CAPSMI_X_STARTS_WITH / ENDS_WITH / CONTAINS over the session's
string store).  The golden cases of tests/golden/string_predicates.json run through the planner; the operators are
compared, exactly and in row order, with the pure-Python restatement of str_match_ref.py, on the row side and on the
dictionary side (CAPSMI_STR_MATCH).  CONTAINS's shapes are built around T, the tile of candidate slots.

One pattern of the random comparison is the second byte of "é" alone: no UTF-8, so it travels through the binding as
a surrogate escape (PEP 383), which StringDictionary.arrays() stores as that one byte."""
import ctypes
import json

import numpy as np
import pytest

from golden_util import load_cases, run_planner, same_rows
from str_match_ref import OPS, T, ref_match, slots

pytestmark = pytest.mark.gpu

CASES = load_cases("string_predicates.json")
MODES = ["rows", "dict"]


def _cls(op):
    from capsmi.expr import Contains, EndsWith, StartsWith
    return {"starts_with": StartsWith, "ends_with": EndsWith, "contains": Contains}[op]


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
def _str_col(session, name, values):
    """A String ColumnData of Python strings, None for NULL."""
    from capsmi import ColumnData, expr
    session.dictionary.extend(sorted({v for v in values if v is not None}))
    codes = np.array([0 if v is None else session.dictionary.encode(v) for v in values], dtype=np.int64)
    return ColumnData(name, expr.STR, codes, np.array([v is not None for v in values], dtype=bool))


def _table(session, **cols):
    from capsmi import ColumnData, expr
    n = len(next(iter(cols.values())))
    return session.table([ColumnData("id", expr.I64, np.arange(n, dtype=np.int64))] +
                         [_str_col(session, k, v) for k, v in cols.items()])


def _values(session, t, name):
    from capsmi.table import decode_value
    c = t.column(name)
    return [None if (c.valid is not None and not c.valid[r]) else decode_value(c.type, c.values[r], session.dictionary)
            for r in range(len(c.values))]


def _assert_same(got, want):
    assert len(got) == len(want)
    bad = [(r, g, w) for r, (g, w) in enumerate(zip(got, want)) if not (type(g) is type(w) and g == w)]
    assert not bad, bad[:10]


def _timer(session, name):
    from capsmi import _lib
    launches, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", session.handle, name.encode(), ctypes.byref(launches), ctypes.byref(ms))
    return launches.value


# ---- random comparison -----------------------------------------------------------------------------
LONE = b"\xa9".decode("utf-8", "surrogateescape")  # the second byte of é alone
PATTERNS = ["", "a", "ab", "aba", "é", LONE, "ababababababa"]  # the last: 13 characters, longer than every string
RANDOM = {}


def _random_rows():
    """700 strings over {a, b, é} of 0 to 12 characters and 700 patterns from PATTERNS, a quarter of each NULL."""
    if not RANDOM:
        rng = np.random.default_rng(29)
        alpha = ["a", "b", "é"]
        s = ["".join(alpha[k] for k in rng.integers(0, 3, int(rng.integers(0, 13)))) for _ in range(700)]
        p = [PATTERNS[k] for k in rng.integers(0, len(PATTERNS), 700)]
        RANDOM["s"] = [None if x else v for v, x in zip(s, rng.random(700) < 0.25)]
        RANDOM["p"] = [None if x else v for v, x in zip(p, rng.random(700) < 0.25)]
    return RANDOM["s"], RANDOM["p"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", OPS)
def test_random_strings_against_the_restatement(session, knobs, op, mode):
    from capsmi.expr import Col, Lit
    knobs(session, CAPSMI_STR_MATCH=mode)
    s, p = _random_rows()
    assert s.count(None) > 100 and "" in s and max(len(x) for x in s if x is not None) == 12
    t = _table(session, s=s, p=p)
    out = t.withColumns(*[(_cls(op)(Col("s"), Lit(pat)), f"m{k}") for k, pat in enumerate(PATTERNS)],
                        (_cls(op)(Col("s"), Col("p")), "mc"))
    assert out.columnType["m0"] == 1 and out.columnType["mc"] == 1  # BOOL
    for k, pat in enumerate(PATTERNS):
        want = [ref_match(op, x, pat) for x in s]
        if pat != PATTERNS[-1] and not (pat == LONE and op == "starts_with"):  # nothing starts with a continuation byte
            assert want.count(True) > 10  # matches are common
        _assert_same(_values(session, out, f"m{k}"), want)
    _assert_same(_values(session, out, "mc"), [ref_match(op, x, y) for x, y in zip(s, p)])
    _assert_same(_values(session, out, "id"), list(range(700)))


@pytest.mark.parametrize("mode", MODES)
def test_two_string_nodes_and_a_case(session, knobs, mode):
    from capsmi.expr import Ands, Case, Col, Contains, EndsWith, Lit, Not, StartsWith
    knobs(session, CAPSMI_STR_MATCH=mode)
    s, p = _random_rows()
    t = _table(session, s=s, p=p)
    both = Ands((Contains(Col("s"), Lit("a")), Not(EndsWith(Col("s"), Lit("b")))))
    case = Case(((StartsWith(Col("s"), Col("p")), Lit("yes")), (Contains(Col("s"), Lit("é")), Lit("é"))), Lit("no"))
    out = t.withColumns((both, "x"), (case, "c"))

    def and3(a, b):
        return False if a is False or b is False else None if a is None or b is None else True

    def not3(a):
        return None if a is None else not a

    want = [and3(ref_match("contains", x, "a"), not3(ref_match("ends_with", x, "b"))) for x in s]
    _assert_same(_values(session, out, "x"), want)
    _assert_same(_values(session, out, "c"),
                 ["yes" if ref_match("starts_with", x, y) is True else "é" if ref_match("contains", x, "é") is True else "no"
                  for x, y in zip(s, p)])
    kept = t.filter(both)
    assert _values(session, kept, "id") == [r for r in range(700) if want[r] is True]


# ---- tile edges of CONTAINS ------------------------------------------------------------------------
LONG = 3 * T + 5


def _long(at):
    """LONG bytes of x with the only xyz at candidate slot `at` (None: nowhere)."""
    return "x" * LONG if at is None else "x" * at + "xyz" + "x" * (LONG - at - 3)


EDGE = {
    "at_0": ["", None, "xy", _long(0), "x", None, ""],
    "across_the_first_tile_boundary": ["", None, "xy", _long(T - 1), "x", None, ""],
    "at_the_last_candidate": ["", None, "xy", _long(LONG - 3), "x", None, ""],
    "nowhere": ["", None, "xy", _long(None), "x", None, ""],
    "slots_exactly_T": ["x" * (T - 98), None, "x" * 99 + "xyz"],
    "slots_T_plus_1": ["x" * (T - 98), None, "x" * 99 + "xyz", "", "xyz"],
    "one_row": ["wxyz"],
    "no_rows": [],
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(EDGE))
def test_contains_tile_edges(session, knobs, shape, mode):
    from capsmi.expr import Col, Contains, Lit
    knobs(session, CAPSMI_STR_MATCH=mode)
    s = EDGE[shape]
    total = sum(slots(x, "xyz") for x in s)
    assert total == {"slots_exactly_T": T, "slots_T_plus_1": T + 1, "one_row": 2, "no_rows": 0}.get(shape, LONG - 2)
    if shape == "across_the_first_tile_boundary":  # the long string's slots start the first tile: bytes T-1 .. T+1
        assert s[3].index("xyz") == T - 1 and all(slots(x, "xyz") == 0 for x in s[:3])
    t = _table(session, s=s)
    out = t.withColumns((Contains(Col("s"), Lit("xyz")), "m"))
    want = [ref_match("contains", x, "xyz") for x in s]
    if shape not in ("nowhere", "no_rows"):
        assert want.count(True) == (2 if shape == "slots_T_plus_1" else 1)
    _assert_same(_values(session, out, "m"), want)
    assert out.physicalColumns == ["id", "s", "m"]


def test_constant_haystack_and_column_pattern(session):
    from capsmi.expr import Col, Contains, EndsWith, Lit, StartsWith
    r = ["foo", "", None, "bar", "foobar", "foobarx", "oba", "f"]
    t = _table(session, r=r)
    out = t.withColumns((StartsWith(Lit("foobar"), Col("r")), "a"), (EndsWith(Lit("foobar"), Col("r")), "b"),
                        (Contains(Lit("foobar"), Col("r")), "c"), (Contains(Lit(None), Col("r")), "n"),
                        (StartsWith(Col("r"), Lit(None, 3)), "n3"), (Contains(Lit("foobar"), Lit("oba")), "k"))
    for name, op in (("a", "starts_with"), ("b", "ends_with"), ("c", "contains")):
        _assert_same(_values(session, out, name), [ref_match(op, "foobar", x) for x in r])
    _assert_same(_values(session, out, "n"), [None] * len(r))
    _assert_same(_values(session, out, "n3"), [None] * len(r))
    _assert_same(_values(session, out, "k"), [True] * len(r))


@pytest.mark.parametrize("mode", MODES)
def test_operands_that_are_expressions(session, knobs, mode):
    """A bound parameter (a constant by the time the node runs), coalesce, CASE and list[i] of a String list: the
    operand sub-programs are evaluated into temporary columns first."""
    from capsmi import expr
    from capsmi.expr import BinOp, Case, Coalesce, Col, Contains, EndsWith, Index, Lit, Param, StartsWith
    knobs(session, CAPSMI_STR_MATCH=mode)
    s, p = _random_rows()
    s, p = s[:300], p[:300]
    firsts = [None if x is None or not x else x[0] for x in s]  # xs = [first character of s] (empty for "" and NULL)
    session.dictionary.extend(sorted({c for c in firsts if c is not None}))
    offs = np.cumsum([0] + [0 if c is None else 1 for c in firsts])
    words = [session.dictionary.encode(c) for c in firsts if c is not None]
    t = _table(session, s=s, p=p).add_list_column_csr("xs", expr.STR, offs, words)
    session.set_params(["ab"])
    try:
        out = t.withColumns((Contains(Col("s"), Param(0)), "par"),
                            (EndsWith(Col("s"), Coalesce((Col("p"), Lit("a")))), "co"),
                            (StartsWith(Col("s"), Index(Col("xs"), Lit(0))), "ix"),
                            (StartsWith(Case(((BinOp("<", Col("id"), Lit(150)), Col("s")),), Lit("ba")), Col("p")), "ca"))
        got = {k: _values(session, out, k) for k in ("par", "co", "ix", "ca")}
    finally:
        session.set_params([])
    _assert_same(got["par"], [ref_match("contains", x, "ab") for x in s])
    _assert_same(got["co"], [ref_match("ends_with", x, "a" if y is None else y) for x, y in zip(s, p)])
    _assert_same(got["ix"], [ref_match("starts_with", x, c) for x, c in zip(s, firsts)])  # TRUE wherever xs[0] exists
    assert got["ix"].count(True) == sum(c is not None for c in firsts) > 100
    _assert_same(got["ca"], [ref_match("starts_with", x if r < 150 else "ba", y) for r, (x, y) in enumerate(zip(s, p))])


def test_in_list_and_contains_in_a_table_at_the_column_limit(session):
    """64 columns, the interpreter's limit, and 300 rows (one block of 256 and a part of one): x IN xs and s CONTAINS 'a'
    under one AND whose third operand reads the other 61 columns.  Neither lowered node can append its result
    column, so each borrows a slot the rest of the program does not read (its own operands' columns)."""
    from functools import reduce
    from capsmi import ColumnData, expr
    from capsmi.expr import Ands, BinOp, Col, Contains, InList, Lit
    from list_expr_ref import ref_in_list
    rng = np.random.default_rng(64)
    n = 300
    s, _ = _random_rows()
    s = s[:n]
    pv = rng.random(n) >= 0.2
    p = [int(x) if ok else None for x, ok in zip(rng.integers(0, 9, n), pv)]
    lists = [rng.integers(0, 9, int(rng.integers(0, 6))).tolist() for _ in range(n)]
    lv = rng.random(n) >= 0.2
    offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    cols = [ColumnData("id", expr.I64, np.arange(n, dtype=np.int64)), _str_col(session, "s", s),
            ColumnData("p", expr.I64, np.array([0 if x is None else x for x in p], dtype=np.int64), pv)]
    cols += [ColumnData(f"f{k}", expr.I64, np.full(n, k, dtype=np.int64)) for k in range(60)]
    t = session.table(cols).add_list_column_csr("xs", expr.I64, offs, np.array([v for x in lists for v in x], dtype=np.int64),
                                                lv.astype(np.uint8))
    assert len(t.physicalColumns) == 64
    others = reduce(lambda a, b: BinOp("+", a, b), [Col("id")] + [Col(f"f{k}") for k in range(60)])  # id + 0 + .. + 59
    pred = Ands((InList(Col("p"), Col("xs")), Contains(Col("s"), Lit("a")), BinOp(">=", others, Lit(1770 + 40))))

    def and3(*v):
        return False if False in v else None if None in v else True

    want = [and3(ref_in_list(p[r], lists[r] if lv[r] else None, int), ref_match("contains", s[r], "a"), r >= 40)
            for r in range(n)]
    assert want.count(True) > 10 and want.count(None) > 10 and want[:40].count(False) == 40
    out = t.withColumns((pred, "m"))
    _assert_same(_values(session, out, "m"), want)
    assert _values(session, out, "f59") == [59] * n and _values(session, out, "s") == s  # the lent slots are the view's
    assert _values(session, t.filter(pred), "id") == [r for r in range(n) if want[r] is True]


# ---- the side taken under auto ---------------------------------------------------------------------
def test_auto_takes_the_dictionary_side_from_as_many_rows_as_strings(session):
    from capsmi import _lib
    from capsmi.expr import Col, Contains, Lit
    pool = ["alpha", "beta", "gamma", None]
    session.dictionary.extend(["alpha", "beta", "gamma", "a"])
    ns = len(session.dictionary)
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        for n, lookups in ((ns, 1), (ns - 1, 0)):
            s = [pool[r % 4] for r in range(n)]
            t = _table(session, s=s)
            _timer(session, "str_match_lookup")  # reset
            _timer(session, "str_index")
            out = t.withColumns((Contains(Col("s"), Lit("a")), "m"))
            _assert_same(_values(session, out, "m"), [ref_match("contains", x, "a") for x in s])
            assert len(session.dictionary) == ns
            assert _timer(session, "str_index") == 1
            assert _timer(session, "str_match_lookup") == lookups, n
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)


# ---- errors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_a_coalesce_of_string_and_long_is_no_string_operand(session, op):
    """Whichever alternative comes first: the typed alternatives disagree, so the operand has no one type."""
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Coalesce, Col, Lit
    t = _table(session, s=["a", "b"])
    for alts in ((Col("s"), Col("id")), (Col("id"), Col("s"))):
        with pytest.raises(IllegalArgumentException):
            t.withColumns((_cls(op)(Coalesce(alts), Lit("a")), "x"))
        with pytest.raises(IllegalArgumentException):
            t.filter(_cls(op)(Col("s"), Coalesce(alts)))
    t.withColumns((Coalesce((Col("s"), Col("id"))), "x"))  # a value like any other where no type is demanded


@pytest.mark.parametrize("op", OPS)
def test_operand_types_are_checked_when_the_node_is_built(session, op):
    from capsmi import expr
    from capsmi._lib import IllegalArgumentException, NotImplementedException
    from capsmi.expr import Col, Lit
    t = _table(session, s=["a", "b"]).add_list_column_csr("xs", expr.STR, [0, 1, 1], [session.dictionary.encode("a")])
    with pytest.raises(IllegalArgumentException):
        t.withColumns((_cls(op)(Col("id"), Lit("a")), "x"))
    with pytest.raises(IllegalArgumentException):
        t.filter(_cls(op)(Col("s"), Lit(3)))
    with pytest.raises(IllegalArgumentException):
        t.withColumns((_cls(op)(Col("s"), Lit(None, expr.I64)), "x"))
    with pytest.raises(NotImplementedException):
        t.withColumns((_cls(op)(Col("xs"), Lit("a")), "x"))
    with pytest.raises(NotImplementedException):
        t.withColumns((_cls(op)(Col("s"), Col("xs")), "x"))


@pytest.mark.parametrize("mode", MODES)
def test_a_code_outside_the_store_fails_the_action(session, knobs, mode):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Col, Contains, Lit
    knobs(session, CAPSMI_STR_MATCH=mode)
    good = session.dictionary.encode("abc")
    raw = np.array([good, 12345, good, -7], dtype=np.int64)  # words that are no codes of the dictionary
    with pytest.raises(KeyError):
        session.dictionary.decode(12345)
    t = session.table([ColumnData("s", expr.STR, raw, np.array([True, True, False, True]))])
    out = t.withColumns((Contains(Col("s"), Lit("b")), "m"))  # the node is built
    with pytest.raises(IllegalArgumentException, match="registered"):
        out.size
    ok = _table(session, s=["abc", None, "ac"])  # the session goes on
    _assert_same(_values(session, ok.withColumns((Contains(Col("s"), Lit("b")), "m")), "m"), [True, None, False])


# ---- pushdown --------------------------------------------------------------------------------------
def test_contains_filter_on_a_node_scan_under_an_expand(session):
    create = ("CREATE (:P {name: 'xavier'})-[:T]->(:P {name: 'bob'})-[:T]->(:P {name: 'alex'})-[:T]->(:P {name: 'max'}), "
              "(:P {name: 'ann'})-[:T]->(:P)")
    case = {"create": create,
            "query": {"clauses": [{"match": "(n)-[r]->(m)", "where": ["contains", ["prop", "n", "name"], ["lit", "x"]]}],
                      "return": {"items": [["n.name", ["prop", "n", "name"]], ["m.name", ["prop", "m", "name"]]]}}}
    got = {}
    for fused in (True, False):
        session.set_fused(fused)
        try:
            got[fused] = run_planner(session, case)
        finally:
            session.set_fused(True)
    want = [{"n.name": "xavier", "m.name": "bob"}, {"n.name": "alex", "m.name": "max"}]
    assert same_rows(got[True], want) and same_rows(got[False], want), json.dumps(got)
