"""Division, the math functions, toFloat and toInteger on the device (CAPSMI_X_DIV .. CAPSMI_X_TO_INTEGER, the kMath
instantiation of k_expr.hip's interpreter).  The golden cases of tests/golden/math_functions.json run through the
planner; every edge the header names is compared bit for bit -- type, validity, the sign of zero -- with the
pure-Python restatement of math_ref.py, but for the finite non-zero results of log, log10 and exp, which are held to
2 ULP of numpy's: OCML and glibc each document at most 1 ULP for these functions, so two correct implementations
differ by at most 2.  (That bound cannot tell log(x) / log(10.0) from log10(x); the kernel's source does.)"""
import ctypes
import json
import math

import numpy as np
import pytest

import math_ref as mr
from golden_util import load_cases, run_planner, same_rows

pytestmark = pytest.mark.gpu

CASES = load_cases("math_functions.json")
INF, NAN = math.inf, math.nan
LMAX, LMIN = mr.LONG_MAX, mr.LONG_MIN
ULP_BOUND = 2


def _cls(op):
    from capsmi import expr
    return {"sqrt": expr.Sqrt, "log": expr.Log, "log10": expr.Log10, "exp": expr.Exp, "abs": expr.Abs, "ceil": expr.Ceil,
            "floor": expr.Floor, "round": expr.Round, "sign": expr.Sign, "tofloat": expr.ToFloat,
            "tointeger": expr.ToInteger}[op]


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
def _col(name, ty, values):
    """A Long or Double ColumnData of Python values, None for NULL."""
    from capsmi import ColumnData, expr
    dt = np.float64 if ty == expr.F64 else np.int64
    return ColumnData(name, ty, np.array([0 if v is None else v for v in values], dtype=dt),
                      np.array([v is not None for v in values], dtype=bool))


def _values(t, name):
    """The column as Python values: int for Long and for BOOL words, float for Double, None for NULL."""
    from capsmi import expr
    c = t.column(name)
    conv = float if c.type == expr.F64 else bool if c.type == expr.BOOL else int
    return [None if (c.valid is not None and not c.valid[r]) else conv(c.values[r]) for r in range(len(c.values))]


def _ordered(x: float) -> int:
    b = mr.bits(x)
    return b if b >= 0 else -(b & LMAX)


def _ulps(a: float, b: float) -> int:
    return abs(_ordered(a) - _ordered(b))


def _assert_exact(got, want, what=""):
    assert len(got) == len(want)
    bad = [(r, g, w) for r, (g, w) in enumerate(zip(got, want)) if not mr.same_value(g, w)]
    assert not bad, (what, bad[:10])


def _assert_within_ulps(got, want, what=""):
    """Validity, NaN, the infinities and zeros exactly; finite non-zero results within ULP_BOUND."""
    assert len(got) == len(want)
    worst, bad = 0, []
    for r, (g, w) in enumerate(zip(got, want)):
        if w is not None and g is not None and math.isfinite(w) and w != 0.0 and math.isfinite(g):
            d = _ulps(g, w)
            worst = max(worst, d)
            if d > ULP_BOUND:
                bad.append((r, g, w, d))
        elif not mr.same_value(g, w):
            bad.append((r, g, w, None))
    print(f"{what}: max distance {worst} ULP over {len(want)} rows")
    assert not bad, (what, bad[:10])


# ---- the edge tables -------------------------------------------------------------------------------
LONGS = [None, 0, 1, -1, 2, 9, 100, 1000, -23, 2 ** 31, 2 ** 31 - 1, -2 ** 31, -2 ** 31 - 1, 2 ** 32 + 5, 2 ** 53 + 1, LMAX,
         LMIN, LMIN + 1, 710, -746]
DOUBLES = [None, 0.0, -0.0, 0.5, -0.5, 2.5, -2.5, 0.49999999999999994, -0.4, 0.1, 1.9, -1.1, 1.0, 12.96, -12.96, 1.337, 82.9,
           2.0 ** 52 + 1, 2.0 ** 53, 1e300, -1e300, 3e9, -3e9, 2147483647.5, -2147483648.5, 2.0 ** 63, -(2.0 ** 63), 5e-324,
           710.0, -746.0, 709.0, INF, -INF, NAN, 1000.0, 100.0, 9.0, -1.0]
APPROX = ("log", "log10", "exp")


@pytest.mark.parametrize("op", mr.OPS)
def test_unary_edges(session, op):
    from capsmi import expr
    from capsmi.expr import Col
    n = max(len(LONGS), len(DOUBLES))
    assert n <= 64
    xi = LONGS + [None] * (n - len(LONGS))
    xf = DOUBLES + [None] * (n - len(DOUBLES))
    t = session.table([_col("xi", expr.I64, xi), _col("xf", expr.F64, xf)])
    out = t.withColumns((_cls(op)(Col("xi")), "ri"), (_cls(op)(Col("xf")), "rf"), (_cls(op)(expr.Lit(None)), "rn"))
    long_valued = op in ("sign", "tointeger")
    assert out.columnType["ri"] == (expr.F64 if not long_valued and op != "abs" else expr.I64)
    assert out.columnType["rf"] == (expr.I64 if long_valued else expr.F64)
    check = _assert_within_ulps if op in APPROX else _assert_exact
    check(_values(out, "ri"), [mr.FUNCS[op](v) for v in xi], f"{op}(Long)")
    check(_values(out, "rf"), [mr.FUNCS[op](v) for v in xf], f"{op}(Double)")
    _assert_exact(_values(out, "rn"), [None] * n)


DIV_ROWS = [(9, 3), (3, 2), (-7, 2), (7, -2), (LMIN, -1), (2 ** 53 + 1, 1), (0, 0), (5, 0), (0, 5), (LMAX, 1), (LMAX, -1),
            (LMIN, 1), (1, LMIN), (None, 2), (2, None), (None, None),
            (1.0, -0.0), (1.0, 0.0), (INF, INF), (INF, 2.0), (-1.0, INF), (NAN, 2.0), (2.0, NAN), (1.0, 3.0), (9.0, 4.5),
            (1e308, 1e-308), (5e-324, 2.0), (-0.0, 5.0), (0.0, -5.0), (None, 1.0), (1.0, None)]


def test_division_edges(session):
    from capsmi import expr
    from capsmi.expr import BinOp, Col
    assert len(DIV_ROWS) <= 64
    longs = [not isinstance(a, float) and not isinstance(b, float) for a, b in DIV_ROWS]  # the rows of the Long columns
    ai = [a if ok else None for (a, _), ok in zip(DIV_ROWS, longs)]
    bi = [b if ok else None for (_, b), ok in zip(DIV_ROWS, longs)]
    af = [None if a is None else float(a) for a, _ in DIV_ROWS]
    bf = [None if b is None else float(b) for _, b in DIV_ROWS]
    t = session.table([_col("ai", expr.I64, ai), _col("bi", expr.I64, bi), _col("af", expr.F64, af), _col("bf", expr.F64, bf)])
    pairs = {"ll": ("ai", "bi"), "ff": ("af", "bf"), "lf": ("ai", "bf"), "fl": ("af", "bi")}
    out = t.withColumns(*[(BinOp("/", Col(a), Col(b)), k) for k, (a, b) in pairs.items()])
    assert [out.columnType[k] for k in pairs] == [expr.I64, expr.F64, expr.F64, expr.F64]
    data = {"ai": ai, "bi": bi, "af": af, "bf": bf}
    for k, (a, b) in pairs.items():
        _assert_exact(_values(out, k), [mr.div(p, q) for p, q in zip(data[a], data[b])], k)
    ll = _values(out, "ll")
    assert ll[:8] == [3, 1, -3, -3, LMAX, 2 ** 53, None, None]  # as the header states them


# ---- log, log10 and exp against numpy ------------------------------------------------------------------
def test_log_log10_exp_within_two_ulps_of_numpy(session):
    """4096 random doubles (log: 10^u over the whole normal range, a tenth of them negated, which gives NULL; exp: the
    range whose results are normal) plus the edges of the table above."""
    from capsmi import expr
    from capsmi.expr import Col, Exp, Log, Log10
    rng = np.random.default_rng(41)
    edges = np.array([v for v in DOUBLES if v is not None], dtype=np.float64)
    xl = np.concatenate([10.0 ** rng.uniform(-307, 308, 4096) * np.where(rng.random(4096) < 0.1, -1.0, 1.0), edges])
    xe = np.concatenate([rng.uniform(-700, 700, 4096), edges])
    t = session.table([_col("xl", expr.F64, xl.tolist()), _col("xe", expr.F64, xe.tolist())])
    out = t.withColumns((Log(Col("xl")), "log"), (Log10(Col("xl")), "log10"), (Exp(Col("xe")), "exp"))
    with np.errstate(all="ignore"):
        ln = np.log(xl)
        want = {"log": [None if x <= 0.0 else float(v) for x, v in zip(xl, ln)],
                "log10": [None if x <= 0.0 else float(v) for x, v in zip(xl, ln / np.log(10.0))],
                "exp": [float(v) for v in np.exp(xe)]}
    assert want["log"].count(None) > 300
    for k in ("log", "log10", "exp"):
        _assert_within_ulps(_values(out, k), want[k], k)


# ---- grid edges of the math instantiation --------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 8192 * 256 + 1])
def test_grid_edges(session, n):
    """sqrt(toFloat(x)) / y: one row, around one block, and one row more than the capped grid covers in one stride."""
    from capsmi import ColumnData, expr
    from capsmi.expr import BinOp, Col, Sqrt, ToFloat
    rng = np.random.default_rng(n)
    x = rng.integers(0, 1 << 40, n).astype(np.int64)
    x = np.where(rng.random(n) < 0.05, -x - 1, x)  # sqrt of a negative Long: NaN
    y = np.where(rng.random(n) < 0.1, 0.0, rng.standard_normal(n))
    yv = rng.random(n) >= 0.2
    t = session.table([ColumnData("x", expr.I64, x), ColumnData("y", expr.F64, y, yv)])
    out = t.withColumns((BinOp("/", Sqrt(ToFloat(Col("x"))), Col("y")), "r"))
    assert out.columnType["r"] == expr.F64 and out.size == n
    c = out.column("r")
    with np.errstate(all="ignore"):
        want = np.sqrt(x.astype(np.float64)) / y  # sqrt and / are correctly rounded on both sides
    want_valid = yv & (y != 0.0)
    got_valid = np.ones(n, dtype=bool) if c.valid is None else c.valid
    assert np.array_equal(got_valid, want_valid)
    g, w = c.values[want_valid], want[want_valid]
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)].view(np.int64), w[~np.isnan(w)].view(np.int64))
    if n >= 255:
        assert np.isnan(w).any() and (~yv).any() and (yv & (y == 0.0)).any()


# ---- composition ---------------------------------------------------------------------------------------
def _random_table(session, n=300):
    from capsmi import expr
    rng = np.random.default_rng(7)
    x = [None if rng.random() < 0.1 else int(v) for v in rng.integers(-20, 20, n)]
    y = [None if rng.random() < 0.1 else int(v) for v in rng.integers(-3, 4, n)]
    f = [None if rng.random() < 0.1 else float(v) for v in np.round(rng.uniform(-2, 6, n), 2)]
    lists = [rng.integers(-5, 6, int(rng.integers(0, 6))).tolist() for _ in range(n)]
    offs = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    t = session.table([_col("id", expr.I64, list(range(n))), _col("x", expr.I64, x), _col("y", expr.I64, y), _col("f", expr.F64, f)])
    t = t.add_list_column_csr("xs", expr.I64, offs, np.array([v for l in lists for v in l], dtype=np.int64))
    return t, x, y, f, lists


def test_under_case_coalesce_in_and_index(session):
    from capsmi import expr
    from capsmi.expr import BinOp, Case, Coalesce, Col, In, Index, InList, Lit, Sqrt, ToInteger
    t, x, y, f, lists = _random_table(session)
    div = BinOp("/", Col("x"), Col("y"))
    out = t.withColumns((Case(((BinOp(">=", Col("f"), Lit(0.0)), Sqrt(Col("f"))),), Lit(-1.0)), "case"),
                        (Coalesce((div, Lit(99))), "co"),
                        (In(div, (Lit(1), Lit(-2), Lit(0))), "in"),
                        (InList(div, Col("xs")), "inl"),
                        (Index(Col("xs"), ToInteger(Col("f"))), "ix"))
    assert [out.columnType[k] for k in ("case", "co", "in", "inl", "ix")] == [expr.F64, expr.I64, expr.BOOL, expr.BOOL, expr.I64]
    q = [mr.div(a, b) for a, b in zip(x, y)]
    assert q.count(None) > 40 and len({v for v in q if v is not None}) > 10
    _assert_exact(_values(out, "case"), [mr.sqrt(v) if v is not None and v >= 0.0 else -1.0 for v in f])
    _assert_exact(_values(out, "co"), [99 if v is None else v for v in q])
    _assert_exact(_values(out, "in"), [None if v is None else v in (1, -2, 0) for v in q])
    _assert_exact(_values(out, "inl"), [None if v is None else v in l for v, l in zip(q, lists)])

    def index(l, v):
        i = mr.tointeger(v)
        return None if i is None or not 0 <= i < len(l) else l[i]

    want_ix = [index(l, v) for l, v in zip(lists, f)]
    assert sum(v is not None for v in want_ix) > 50
    _assert_exact(_values(out, "ix"), want_ix)


def test_in_a_filter(session):
    from capsmi.expr import Ands, BinOp, Col, Floor, Lit
    t, x, y, f, _ = _random_table(session)
    pred = Ands((BinOp("=", BinOp("/", Col("x"), Col("y")), Lit(-2)), BinOp("<", Floor(Col("f")), Lit(3.0))))
    want = [r for r in range(len(x)) if mr.div(x[r], y[r]) == -2 and f[r] is not None and mr.floor(f[r]) < 3.0]
    assert len(want) > 3
    assert _values(t.filter(pred), "id") == want


def test_a_string_match_and_log_in_one_program(session):
    """The string match runs as a pass of its own; the rest of the program, which holds the Log, is evaluated by the
    recursion, which has to take the math instantiation for it."""
    from capsmi import ColumnData, expr
    from capsmi.expr import Ands, BinOp, Col, Lit, Log, StartsWith
    names = ["alpha", "beta", None, "alto", "gamma", "al", "albert", None]
    f = [2.5, 3.0, 4.0, 0.5, 9.0, -1.0, None, 0.0]
    session.dictionary.extend(sorted({v for v in names if v is not None} | {"al"}))
    codes = np.array([0 if v is None else session.dictionary.encode(v) for v in names], dtype=np.int64)
    t = session.table([_col("id", expr.I64, list(range(8))), ColumnData("s", expr.STR, codes, np.array([v is not None for v in names])),
                       _col("f", expr.F64, f)])
    pred = Ands((StartsWith(Col("s"), Lit("al")), BinOp(">", Log(Col("f")), Lit(0.0))))
    out = t.withColumns((pred, "m"))
    # log(f) > 0 iff f > 1; NULL for f <= 0 or NULL.  AND: FALSE wins over NULL
    _assert_exact(_values(out, "m"), [True, False, None, False, False, None, None, None])
    assert _values(t.filter(pred), "id") == [0]


def test_the_stack_limit_under_a_division(session):
    """a / (b + (b + .. + b)), 31 b's: 32 values on the stack before the first ADD, DIV last.  One more is refused."""
    from capsmi import expr
    from capsmi._lib import NotImplementedException
    from capsmi.expr import BinOp, Col, compile_program
    a = [1000, -1000, 30, 31, None, 5, LMIN]
    b = [1, 3, 1, 1, 2, 0, -1]
    t = session.table([_col("a", expr.I64, a), _col("b", expr.I64, b)])

    def chain(k):
        e = Col("b")
        for _ in range(k - 1):
            e = BinOp("+", Col("b"), e)
        return BinOp("/", Col("a"), e)

    prog = compile_program(chain(31), {"a": 0, "b": 1}.__getitem__, None)
    assert [p[0] for p in prog] == [expr.X_COL] * 32 + [expr.X_ADD] * 30 + [expr.X_DIV]
    _assert_exact(_values(t.withColumns((chain(31), "r")), "r"), [mr.div(p, 31 * q) for p, q in zip(a, b)])
    with pytest.raises(NotImplementedException, match="too deep"):
        t.withColumns((chain(32), "r"))


# ---- refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ("/",) + mr.OPS)
def test_operand_types_are_checked_when_the_node_is_built(session, op):
    from capsmi import ColumnData, expr
    from capsmi._lib import NotImplementedException
    from capsmi.expr import BinOp, Coalesce, Col, Lit
    code = session.dictionary.encode("a")
    t = session.table([_col("x", expr.I64, [1, 2]), ColumnData("b", expr.BOOL, np.array([1, 0], dtype=np.int64)),
                       ColumnData("s", expr.STR, np.array([code, code], dtype=np.int64))])
    t = t.add_list_column_csr("xs", expr.I64, [0, 1, 1], [5])
    make = (lambda e: BinOp("/", Col("x"), e)) if op == "/" else _cls(op)
    for bad, word in ((Col("b"), "BOOL"), (Col("s"), "STR"), (Lit(True), "BOOL"), (Lit("a"), "STR"), (Col("xs"), "list")):
        with pytest.raises(NotImplementedException, match=word):
            t.withColumns((make(bad), "r"))
        with pytest.raises(NotImplementedException, match=word):
            t.filter(BinOp("=", make(bad), Lit(1)))
    # a value of no one type is taken; the row that holds no number gives NULL
    out = t.withColumns((make(Coalesce((Lit(None, expr.STR), Col("s"), Col("x")))), "r"))
    assert _values(out, "r") == [None, None]


@pytest.mark.parametrize("with_param", [False, True], ids=["plain", "with_a_parameter"])
def test_an_unassigned_opcode_through_the_abi(session, with_param):
    from capsmi import _lib, expr
    from capsmi._lib import NotImplementedException
    from capsmi.table import _EXPR_PTR
    t = session.table([_col("x", expr.I64, [1, 2])])
    first = (expr.X_PARAM, 0, 0, 0) if with_param else (expr.X_COL, 0, 0, 0)
    session.set_params([4])
    try:
        for op in (32, 39, 52):
            prog = expr.to_ctypes([first, (op, 0, 0, 0)])
            cols = (_lib.ExprColumn * 1)()
            cols[0].name, cols[0].nnodes, cols[0].prog = b"r", 2, ctypes.cast(prog, _EXPR_PTR)
            out = ctypes.c_void_p()
            with pytest.raises(NotImplementedException, match=f"unknown expression op {op}"):
                _lib.call("capsmi_with_columns", t._h, 1, cols, ctypes.byref(out))
            with pytest.raises(NotImplementedException, match=f"unknown expression op {op}"):
                _lib.call("capsmi_filter", t._h, 2, prog, ctypes.byref(out))
    finally:
        session.set_params([])


# ---- routing -------------------------------------------------------------------------------------------
def test_a_division_filter_keeps_the_expand_route(session):
    """MATCH (a)-[r]->(b) WHERE a.k / 2 = 0 RETURN a: the filter is pushed down like any conjunct, so the plan is
    routed as the plain match is, and gives the rows of the unrouted run."""
    create = ("CREATE (:A {k: 0})-[:R]->(:B {k: 5}), (:A {k: 1})-[:R]->(:B {k: 0}), (:A {k: 2})-[:R]->(:B {k: 1}), "
              "(:A {k: -1})-[:R]->(:A {k: 7})-[:R]->(:B), (:A)-[:R]->(:B {k: 1})")
    ret = {"items": [["a", ["entity", "a"]]]}
    plain = {"create": create, "query": {"clauses": [{"match": "(a)-[r]->(b)"}], "return": ret}}
    where = ["=", ["/", ["prop", "a", "k"], ["lit", 2]], ["lit", 0]]
    case = {"create": create, "query": {"clauses": [{"match": "(a)-[r]->(b)", "where": where}], "return": ret}}
    names = ("expand", "expand_count", "two_hop", "triangle", "var_length", "miss")

    def routes(c):
        before = [session.route_count(n) for n in names]
        rows = run_planner(session, c)
        return [session.route_count(n) - b for n, b in zip(names, before)], rows

    d_plain, rows_plain = routes(plain)
    d_where, rows_where = routes(case)
    session.set_fused(False)
    try:
        rows_unfused = run_planner(session, case)
    finally:
        session.set_fused(True)
    assert d_where == d_plain
    assert len(rows_plain) == 6 and sorted(r["a"]["props"]["k"] for r in rows_where) == [-1, 0, 1]
    assert same_rows(rows_where, rows_unfused)
