"""toString() and string concatenation on the device (CAPSMI_X_TO_STRING, CAPSMI_X_CONCAT, k_strmake.hip): the strings
are made from the distinct operand tuples, the session's string sink gives them codes from the dictionary, and the new
entries are merged into the string store.  The golden cases of tests/golden/string_make.json run through the planner;
everything else is decoded through the dictionary and compared, exactly and in row order, with the pure-Python
restatement of str_make_ref.py."""
import ctypes
import json
from collections import Counter

import numpy as np
import pytest

import str_make_ref as mr
from golden_util import load_cases, run_planner, same_rows

pytestmark = pytest.mark.gpu

CASES = load_cases("string_make.json")
T = 2048  # a tile of output bytes (kExplodeTile)
TIMERS = ("str_index", "str_make_lengths", "str_make_starts", "str_make", "str_store_merge", "str_make_gather")


@pytest.fixture
def fresh():
    """A session of its own, so that the test decides what the string store holds and which sink is registered."""
    from capsmi import Session
    s = Session(0)
    yield s
    s.close()


# ---- helpers ---------------------------------------------------------------------------------------
def _str_col(session, name, values):
    from capsmi import ColumnData, expr
    session.dictionary.extend(sorted({v for v in values if v is not None}))
    codes = np.array([0 if v is None else session.dictionary.encode(v) for v in values], dtype=np.int64)
    return ColumnData(name, expr.STR, codes, np.array([v is not None for v in values], dtype=bool))


def _long_col(name, values):
    from capsmi import ColumnData, expr
    return ColumnData(name, expr.I64, np.array([0 if v is None else v for v in values], dtype=np.int64),
                      np.array([v is not None for v in values], dtype=bool))


def _table(session, **cols):
    """id plus one column per keyword: s.., u.. and name are String columns (str / None), the others Long columns."""
    from capsmi import ColumnData, expr
    n = len(next(iter(cols.values())))
    out = [ColumnData("id", expr.I64, np.arange(n, dtype=np.int64))]
    for k, v in cols.items():
        out.append(_str_col(session, k, v) if k[0] in "su" or k == "name" else _long_col(k, v))
    return session.table(out)


def _codes(t, name):
    c = t.column(name)
    w = np.ascontiguousarray(c.values).astype(np.int64)
    ok = np.ones(len(w), dtype=bool) if c.valid is None else np.asarray(c.valid, dtype=bool)
    return w, ok


def _decoded(session, t, name):
    from capsmi import expr
    assert t.columnType[name] == expr.STR, t.columnType
    w, ok = _codes(t, name)
    return [session.dictionary.decode(int(x)) if v else None for x, v in zip(w, ok)]


def _timer(session, name):
    from capsmi import _lib
    launches, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", session.handle, name.encode(), ctypes.byref(launches), ctypes.byref(ms))
    return launches.value


def _bytes(session, name):
    from capsmi import _lib
    b = ctypes.c_double()
    _lib.call("capsmi_session_kernel_bytes", session.handle, name.encode(), ctypes.byref(b))
    return b.value


def _profiled(session, fn):
    """fn() with profiling on: (its result, {timer: launches}, the write pass's declared bytes)."""
    from capsmi import _lib
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        for k in TIMERS:
            _timer(session, k)  # reset
        _bytes(session, "str_make")
        res = fn()
        return res, {k: _timer(session, k) for k in TIMERS}, _bytes(session, "str_make")
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)


class Spy:
    """The session's own sink behind a wrapper that records every call: the strings of each."""

    def __init__(self, session, sink=None):
        from capsmi import _lib
        self.session, self.calls = session, []

        def fn(ctx, n, offsets, data, out):
            off = [offsets[i] for i in range(n + 1)]
            raw = ctypes.string_at(data, off[n])
            self.calls.append([raw[off[i]:off[i + 1]] for i in range(n)])
            return (sink or session._string_sink)(ctx, n, offsets, data, out)

        self.cb = _lib.STRING_SINK_FN(fn)

    def __enter__(self):
        self.session.set_string_sink(self.cb)
        return self

    def __exit__(self, *exc):
        self.session.set_string_sink(self.session._sink_cb)


# ---- golden cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["routed", "unfused"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden(session, case, fused):
    from capsmi._lib import NotImplementedException
    session.set_fused(fused)
    try:
        if case["expected"] == "NotImplemented":
            with pytest.raises(NotImplementedException, match="Double.toString"):
                run_planner(session, case)
            return
        got = run_planner(session, case)
    finally:
        session.set_fused(True)
    assert same_rows(got, case["expected"]), json.dumps(got)
    assert all(v is None or isinstance(v, str) for g in got for v in g.values()), got


# ---- toString --------------------------------------------------------------------------------------
def test_edge_longs_exact_and_in_row_order(session):
    from capsmi.expr import Col, ToString
    x = []
    for i, v in enumerate(mr.edge_longs() * 2):  # every edge twice, a quarter of the rows NULL
        x += [v, None] if i % 3 == 0 else [v]
    assert x.count(None) * 4 >= len(x) - 8 and mr.LONG_MIN in x and mr.LONG_MAX in x
    t = _table(session, x=x)
    with Spy(session) as spy:
        got = _decoded(session, t.withColumns((ToString(Col("x")), "r")), "r")
    assert got == [mr.to_string(v) for v in x]
    assert len(spy.calls) == 1 and sorted(spy.calls[0]) == sorted({str(v).encode() for v in x if v is not None})
    assert b"-9223372036854775808" in spy.calls[0]


def test_booleans_and_the_identity_on_strings(session):
    from capsmi import ColumnData, expr
    from capsmi.expr import Col, Lit, ToString
    b = ColumnData("b", expr.BOOL, np.array([1, 0, 0, 1, 1], dtype=np.int64), np.array([True, True, False, True, False]))
    s = _str_col(session, "s", ["true", None, "", "é", "x"])
    t = session.table([b, s])
    with Spy(session) as spy:
        out = t.withColumns((ToString(Col("b")), "rb"))
        assert _decoded(session, out, "rb") == ["true", "false", None, "true", None]
        assert len(spy.calls) == 1 and sorted(spy.calls[0]) == [b"false", b"true"]
        del spy.calls[:]
        out = t.withColumns((ToString(Col("s")), "rs"), (ToString(Lit("lit")), "rl"))
        assert _decoded(session, out, "rs") == ["true", None, "", "é", "x"]
        assert _decoded(session, out, "rl") == ["lit"] * 5
        assert np.array_equal(_codes(out, "rs")[0][[0, 2, 3, 4]], _codes(t, "s")[0][[0, 2, 3, 4]])
        assert spy.calls == []  # toString of a String: no sink call


# ---- concatenation ---------------------------------------------------------------------------------
def _random_rows():
    rng = np.random.default_rng(65)
    alphabet = ["a", "b", "é"]

    def strings():
        out = ["".join(alphabet[k] for k in rng.integers(0, 3, rng.integers(0, 7))) for _ in range(700)]
        return [None if rng.integers(0, 4) == 0 else v for v in out]

    s, u = strings(), strings()
    s[:4] = ["a", "ab", "", "b"]
    u[:4] = ["bc", "c", "b", ""]
    longs = mr.edge_longs()
    x = [None if rng.integers(0, 4) == 0 else int(longs[rng.integers(0, len(longs))]) for _ in range(700)]
    return s, u, x


def test_random_concatenations_in_every_shape(session):
    from capsmi.expr import BinOp, Col, Concat, Lit
    s, u, x = _random_rows()
    assert 120 < s.count(None) < 230 and "" in s and any("é" in v for v in s if v)
    t = _table(session, s=s, u=u, x=x)
    shapes = {"cl": (Concat(Col("s"), Lit("é!")), [mr.concat(a, "é!") for a in s]),
              "lc": (Concat(Lit("<"), Col("s")), [mr.concat("<", a) for a in s]),
              "cc": (Concat(Col("s"), Col("u")), [mr.concat(a, b) for a, b in zip(s, u)]),
              "ls": (Concat(Col("x"), Col("s")), [mr.concat(a, b) for a, b in zip(x, s)]),
              "sl": (Concat(Col("s"), Col("x")), [mr.concat(a, b) for a, b in zip(s, x)]),
              "le": (Concat(Col("s"), Lit("")), list(s)),
              "el": (BinOp("+", Lit(""), Col("u")), list(u)),
              "ln": (Concat(Col("s"), Lit(-7)), [mr.concat(a, -7) for a in s]),
              "nl": (Concat(Lit(mr.LONG_MIN), Col("s")), [mr.concat(mr.LONG_MIN, a) for a in s])}
    with Spy(session) as spy:
        out = t.withColumns(*[(e, k) for k, (e, _) in shapes.items()])
        for k, (_, want) in shapes.items():
            assert _decoded(session, out, k) == want, k
        names = list(shapes)
        first = [out.fingerprint(names[:5]), out.fingerprint(names[5:])]  # a fingerprint takes at most 8 columns
    assert len(spy.calls) == len(shapes)  # one sink call per lowered node
    for call in spy.calls:
        assert len(call) <= 700
    # "a" + "bc" and "ab" + "c": two tuples, one string, one code; the empty string on either side
    cc, ok = _codes(out, "cc")
    assert ok[:4].all() and cc[0] == cc[1] and session.dictionary.decode(int(cc[0])) == "abc"
    assert session.dictionary.decode(int(cc[2])) == "b" == session.dictionary.decode(int(cc[3]))
    assert np.array_equal(_codes(out, "le")[0][_codes(out, "le")[1]], _codes(t, "s")[0][_codes(t, "s")[1]])  # s + "" is s
    # determinism: the same shapes again give the same codes
    again = t.withColumns(*[(e, k) for k, (e, _) in shapes.items()])
    assert [again.fingerprint(names[:5]), again.fingerprint(names[5:])] == first


# ---- the write pass at its tile edges --------------------------------------------------------------------
def _strings_of(out_lengths):
    """Distinct strings s_i with len(s_i + "!") = out_lengths[i]."""
    assert all(n >= 1 for n in out_lengths) and len(out_lengths) <= 26
    return [chr(ord("a") + i) * (n - 1) for i, n in enumerate(out_lengths)]


@pytest.mark.parametrize("shape", ["T", "T+1", "3T+5", "one_row"])
def test_write_pass_tile_edges(fresh, shape):
    from capsmi.expr import Col, Concat, Lit
    lengths = {"T": [5, T - 5 - 40, 40], "T+1": [T - 2, 2, 1], "3T+5": [2, 3 * T + 5 - 2 - 7, 7], "one_row": [T + 3]}[shape]
    s = _strings_of(lengths)
    rows = (s + [None] + s[::-1]) if shape != "one_row" else s
    t = _table(fresh, s=rows)
    out, launches, declared = _profiled(fresh, lambda: _decoded(fresh, t.withColumns((Concat(Col("s"), Lit("!")), "r")), "r"))
    assert out == [mr.concat(v, "!") for v in rows]
    assert launches["str_make"] == 1 and launches["str_make_gather"] == 1 and launches["str_store_merge"] == 1, launches
    assert declared == sum(lengths) + 16 * len(lengths)  # the output bytes once, two offsets per String operand and group
    assert sum(lengths) == {"T": T, "T+1": T + 1, "3T+5": 3 * T + 5, "one_row": T + 3}[shape]


def test_all_rows_null_and_no_rows(fresh):
    from capsmi.expr import BinOp, Col, Concat, Lit, ToString
    t = _table(fresh, s=[None, None, None], x=[None, None, None])
    with Spy(fresh) as spy:
        def run():
            out = t.withColumns((Concat(Col("s"), Lit("!")), "r"), (ToString(Col("x")), "q"), (Concat(Col("s"), Col("x")), "p"))
            return [_codes(out, k)[1].tolist() for k in ("r", "q", "p")]
        valid, launches, declared = _profiled(fresh, run)
        assert valid == [[False] * 3] * 3
        assert launches["str_make"] == launches["str_store_merge"] == launches["str_make_lengths"] == 0 and declared == 0
        empty = _table(fresh, s=["a"], x=[1]).filter(BinOp(">", Col("x"), Lit(5)))
        out = empty.withColumns((Concat(Col("s"), Col("x")), "r"))
        assert out.size == 0 and out.columnType["r"] == 3
    assert spy.calls == []


def test_one_mebibyte_string_among_ten_thousand_short_rows(fresh):
    from capsmi.expr import Col, Concat
    big = "x" * (1 << 20)
    s = [("r%d" % (i % 1000)) for i in range(10000)]
    s[5000] = big
    d = [i % 10 for i in range(10000)]
    t = _table(fresh, s=s, d=d)
    with Spy(fresh) as spy:
        w, ok = _codes(t.withColumns((Concat(Col("s"), Col("d")), "r")), "r")
    assert ok.all() and len(spy.calls) == 1 and len(spy.calls[0]) == len({(a, b) for a, b in zip(s, d)})
    assert fresh.dictionary.decode(int(w[5000])) == big + "0"
    for r in (0, 1, 4999, 5001, 9999):
        assert fresh.dictionary.decode(int(w[r])) == s[r] + str(d[r])
    uniq = {int(c): fresh.dictionary.decode(int(c)) for c in np.unique(w)}
    assert [uniq[int(c)] for c in w[:5000]] == [a + str(b) for a, b in zip(s[:5000], d[:5000])]
    # the merged store is readable at once: the big entry ends with its digit
    from capsmi.expr import EndsWith, Lit, StrSize
    out = t.withColumns((Concat(Col("s"), Col("d")), "r")).withColumns((StrSize(Col("r")), "n"), (EndsWith(Col("r"), Lit("x0")), "e"))
    assert int(_codes(out, "n")[0][5000]) == (1 << 20) + 1 and int(_codes(out, "e")[0].sum()) == 1


# ---- the distinct tuples ---------------------------------------------------------------------------------
def test_the_sink_sees_each_distinct_tuple_once(session):
    from capsmi import ColumnData, expr
    from capsmi.expr import Col, ToString
    rng = np.random.default_rng(300)
    vals = np.unique(np.concatenate([rng.integers(-2 ** 62, 2 ** 62, 297), [0, mr.LONG_MIN, mr.LONG_MAX]]))
    assert len(vals) == 300
    n = 8192 * 256 + 1  # one row more than one pass of the largest grid
    pick = rng.integers(0, 300, n)
    t = session.table([ColumnData("x", expr.I64, vals[pick])])
    with Spy(session) as spy:
        w, ok = _codes(t.withColumns((ToString(Col("x")), "r")), "r")
    assert len(spy.calls) == 1 and len(spy.calls[0]) <= 300 and sorted(spy.calls[0]) == sorted(str(int(v)).encode() for v in vals)
    code_of = np.array([session.dictionary.encode(str(int(v))) for v in vals], dtype=np.int64)
    assert ok.all() and np.array_equal(w, code_of[pick])


def test_seventy_thousand_distinct_longs(session):
    from capsmi import ColumnData, expr
    from capsmi.expr import Col, ToString
    x = np.arange(70000, dtype=np.int64) * 1000003 - 35_000_000_000
    t = session.table([ColumnData("x", expr.I64, x)])
    with Spy(session) as spy:
        got = _decoded(session, t.withColumns((ToString(Col("x")), "r")), "r")
    assert got == [str(int(v)) for v in x]
    assert len(spy.calls) == 1 and len(spy.calls[0]) == 70000


# ---- composition in one program --------------------------------------------------------------------------
def _mixed(n=400):
    rng = np.random.default_rng(7)
    x = [None if i % 5 == 4 else int(v) for i, v in enumerate(rng.integers(-2 ** 31, 2 ** 31, n))]
    x[:6] = [1, 10, -1, 0, 19, 2 ** 31 - 1]
    s = [None if i % 7 == 3 else "k%d" % (i % 9) for i in range(n)]
    return x, s


def test_the_result_feeds_string_opcodes_in_the_same_program(session):
    from capsmi.expr import BinOp, Col, Lit, StartsWith, StrSize, StrToInteger, ToString
    x, s = _mixed()
    t = _table(session, x=x, s=s)
    kept = t.filter(StartsWith(ToString(Col("x")), Lit("1")))
    assert _codes(kept, "id")[0].tolist() == [i for i, v in enumerate(x) if v is not None and str(v).startswith("1")]
    out = t.withColumns((StrSize(ToString(Col("x"))), "n"), (BinOp("=", StrToInteger(ToString(Col("x"))), Col("x")), "same"))
    n, nok = _codes(out, "n")
    assert nok.tolist() == [v is not None for v in x] and n[nok].tolist() == [len(str(v)) for v in x if v is not None]
    same, sok = _codes(out, "same")
    assert sok.tolist() == nok.tolist() and same[sok].all()  # toInteger(toString(x)) = x over the Int range


def test_three_operands_case_and_coalesce(session):
    from capsmi.expr import BinOp, Case, Coalesce, Col, Concat, Lit, ToString
    x, s = _mixed()
    t = _table(session, x=x, s=s)
    out = t.withColumns((Concat(Concat(Col("s"), Lit("-")), Col("x")), "abc"),
                        (BinOp("+", BinOp("+", Col("s"), Lit("-")), Col("x")), "plus"),
                        (Coalesce((Concat(Col("s"), Col("x")), Lit("none"))), "co"),
                        (Case(((BinOp(">", Col("x"), Lit(0)), ToString(Col("x"))),), Concat(Lit("neg"), Col("s"))), "ca"))
    want = [None if a is None or b is None else f"{a}-{b}" for a, b in zip(s, x)]
    assert _decoded(session, out, "abc") == want == _decoded(session, out, "plus")
    assert _decoded(session, out, "co") == ["none" if a is None or b is None else f"{a}{b}" for a, b in zip(s, x)]
    assert _decoded(session, out, "ca") == [str(b) if b is not None and b > 0 else mr.concat("neg", a) for a, b in zip(s, x)]


def test_in_a_table_at_the_column_limit(session):
    from capsmi import ColumnData, expr
    from capsmi.expr import Col, Concat, StartsWith, Lit
    x, s = _mixed(100)
    cols = [ColumnData("id", expr.I64, np.arange(100, dtype=np.int64)), _str_col(session, "s", s), _long_col("x", x)]
    cols += [ColumnData(f"f{k}", expr.I64, np.full(100, k, dtype=np.int64)) for k in range(61)]
    t = session.table(cols)
    assert len(t.physicalColumns) == 64
    kept = t.filter(StartsWith(Concat(Col("s"), Col("x")), Lit("k1")))
    assert _codes(kept, "id")[0].tolist() == [i for i in range(100) if s[i] is not None and x[i] is not None and s[i] == "k1"]


def test_a_tostring_filter_keeps_the_expand_route(session):
    create = ("CREATE (:A {age: 41})-[:R]->(:B {age: 5}), (:A {age: 40})-[:R]->(:B {age: 0}), (:A {age: 14})-[:R]->(:B), "
              "(:A {age: 7})-[:R]->(:A {age: 477})-[:R]->(:B), (:A)-[:R]->(:B {age: 49})")
    ret = {"items": [["a", ["entity", "a"]]]}
    plain = {"create": create, "query": {"clauses": [{"match": "(a)-[r]->(b)"}], "return": ret}}
    where = ["starts_with", ["tostring", ["prop", "a", "age"]], ["lit", "4"]]
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
    assert len(rows_plain) == 6 and sorted(r["a"]["props"]["age"] for r in rows_where) == [40, 41, 477]
    assert same_rows(rows_where, rows_unfused)


# ---- the codes are real codes ----------------------------------------------------------------------------
def test_order_group_distinct_and_join_on_the_produced_column(session):
    from capsmi.expr import Col, Concat
    rng = np.random.default_rng(11)
    s = [["Hello", "b", "é", "a", "ab"][k] for k in rng.integers(0, 5, 300)]
    x = [int(v) for v in rng.integers(-3, 45, 300)]
    s[0], x[0] = "Hello", 42
    before = _table(session, name=["Hello42", "zzz", "a-1"])  # a String column ingested before anything is made
    t = _table(session, s=s, x=x).withColumns((Concat(Col("s"), Col("x")), "r"))
    want = [a + str(b) for a, b in zip(s, x)]
    assert _decoded(session, t.orderBy(("r", "asc")), "r") == sorted(want)
    g = t.group(["r"], [("count_star", None, False, "n")])
    assert dict(zip(_decoded(session, g, "r"), _codes(g, "n")[0].tolist())) == dict(Counter(want))
    assert sorted(_decoded(session, t.select("r").distinct(), "r")) == sorted(set(want))
    j = before.select("name").join(t.select("r", "x"), "inner", ("name", "r"))
    assert sorted(_decoded(session, j, "name")) == sorted(w for w in want if w in ("Hello42", "zzz", "a-1")) and j.size >= 1


# ---- the store grows by what is new ------------------------------------------------------------------------
def test_store_growth_and_the_repeated_query(fresh):
    from capsmi.expr import Col, Concat, Lit, StartsWith, ToString
    t = _table(fresh, x=[1, 2, 3, 2, 1, None], s=["k", "k", "m", None, "k", "m"])
    fresh.sync_strings()
    assert fresh.string_count() == len(fresh.dictionary) == 2
    assert _decoded(fresh, t.withColumns((ToString(Col("x")), "r")), "r") == ["1", "2", "3", "2", "1", None]
    assert fresh.string_count() == 5 == len(fresh.dictionary) and fresh._strings_at == fresh.dictionary.growth
    q = lambda: _decoded(fresh, t.withColumns((Concat(Col("s"), Col("x")), "r")), "r")  # noqa: E731
    assert q() == ["k1", "k2", "m3", None, "k1", None]
    assert fresh.string_count() == 8 == len(fresh.dictionary)
    at = fresh._strings_at
    got, launches, _ = _profiled(fresh, q)  # the same query again: nothing is new
    assert got == ["k1", "k2", "m3", None, "k1", None]
    assert launches["str_store_merge"] == 0 and launches["str_make"] == 1, launches
    assert fresh.string_count() == 8 and fresh._strings_at == at == fresh.dictionary.growth
    uploads = []
    from capsmi import _lib
    real = _lib.call
    try:
        _lib.call = lambda name, *a: (uploads.append(name) if name == "capsmi_session_set_strings" else None, real(name, *a))[1]
        fresh.sync_strings()
        kept = t.filter(StartsWith(Concat(Col("s"), Col("x")), Lit("k")))  # "k" is known: no upload either
        assert _codes(kept, "id")[0].tolist() == [0, 1, 4]
    finally:
        _lib.call = real
    assert uploads == []


def test_tostring_of_a_long_needs_no_store_beforehand(fresh):
    from capsmi import ColumnData, _lib, expr
    from capsmi.table import GpuTable, _EXPR_PTR
    assert fresh.string_count() == 0
    t = fresh.table([ColumnData("x", expr.I64, np.array([5, -5, 5], dtype=np.int64))])
    prog = expr.to_ctypes([(expr.X_COL, 0, 0, 0), (expr.X_TO_STRING, 0, 0, 0)])  # no sync_strings before the action
    cols = (_lib.ExprColumn * 1)()
    cols[0].name, cols[0].nnodes, cols[0].prog = b"r", 2, ctypes.cast(prog, _EXPR_PTR)
    h = ctypes.c_void_p()
    _lib.call("capsmi_with_columns", t._h, 1, cols, ctypes.byref(h))
    assert _decoded(fresh, GpuTable(fresh, h), "r") == ["5", "-5", "5"]
    assert fresh.string_count() == 2


# ---- errors ------------------------------------------------------------------------------------------------
def _bad_sinks(session, taken_code):
    def refuses(ctx, n, offsets, data, out):
        return 7

    def one_code(ctx, n, offsets, data, out):
        for i in range(n):
            out[i] = 123456789
        return 0

    def taken(ctx, n, offsets, data, out):
        for i in range(n):
            out[i] = taken_code + i * 1000
        return 0

    return {"non-zero": (refuses, "sink failed"), "one code": (one_code, "two different strings"), "taken": (taken, "other bytes")}


@pytest.mark.parametrize("which", ["none", "non-zero", "one code", "taken"])
def test_what_a_sink_may_not_do_leaves_the_store_as_it_was(fresh, which):
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Col, Lit, StartsWith, ToString
    t = _table(fresh, x=[1, 2, 3], s=["abc", "b", None])
    fresh.sync_strings()
    n0 = fresh.string_count()
    assert n0 == 2
    out = t.withColumns((ToString(Col("x")), "r"))  # the node is built
    if which == "none":
        fresh.set_string_sink(None)
        with pytest.raises(IllegalArgumentException, match="no string sink"):
            out.size
    else:
        fn, msg = _bad_sinks(fresh, fresh.dictionary.encode("abc"))[which]
        with Spy(fresh, sink=fn) as spy:
            with pytest.raises(IllegalArgumentException, match=msg):
                out.size
        assert len(spy.calls) == 1 and sorted(spy.calls[0]) == [b"1", b"2", b"3"]
    fresh.set_string_sink(fresh._sink_cb)
    assert fresh.string_count() == n0 and len(fresh.dictionary) == 2
    w, ok = _codes(t.withColumns((StartsWith(Col("s"), Lit("ab")), "m")), "m")  # "ab" is new: the store is uploaded whole
    assert w.tolist() == [1, 0, 0] and ok.tolist() == [True, True, False]
    assert _decoded(fresh, t.withColumns((ToString(Col("x")), "r")), "r") == ["1", "2", "3"]  # and the session goes on


def test_operand_types_are_checked_when_the_node_is_built(session):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException, NotImplementedException
    from capsmi.expr import Coalesce, Col, Concat, Lit, ToString
    t = session.table([ColumnData("x", expr.I64, np.array([1, 2], dtype=np.int64)), ColumnData("f", expr.F64, np.array([1.0, 2.0])),
                       ColumnData("b", expr.BOOL, np.array([1, 0], dtype=np.int64)), _str_col(session, "s", ["a", "b"])])
    t = t.add_list_column_csr("xs", expr.STR, [0, 1, 1], [session.dictionary.encode("a")])
    for e in (ToString(Col("f")), ToString(Lit(2.5)), Concat(Col("s"), Col("f")), Concat(Col("f"), Col("s")), Concat(Lit(1.5), Col("s"))):
        with pytest.raises(NotImplementedException, match="Double.toString"):
            t.withColumns((e, "r"))
    mixed = Coalesce((Col("s"), Col("x")))
    for e in (Concat(Col("b"), Col("s")), Concat(Col("s"), Lit(True)), Concat(Col("x"), Col("x")), Concat(Lit(1), Col("x")),
              ToString(mixed), Concat(mixed, Col("s"))):
        with pytest.raises(IllegalArgumentException):
            t.withColumns((e, "r"))
    for e in (ToString(Col("xs")), Concat(Col("xs"), Col("s"))):
        with pytest.raises(NotImplementedException, match="list"):
            t.withColumns((e, "r"))


def test_a_code_outside_the_store_fails_the_action(session):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Col, Concat, Lit
    good = session.dictionary.encode("42")
    raw = np.array([good, 12345, good, -7], dtype=np.int64)  # words that are no codes of the dictionary
    t = session.table([ColumnData("s", expr.STR, raw, np.array([True, True, False, True]))])
    out = t.withColumns((Concat(Col("s"), Lit("!")), "r"))
    with Spy(session) as spy:
        with pytest.raises(IllegalArgumentException, match="registered"):
            out.size
    assert spy.calls == []
    ok = _table(session, s=["42", None, "x"])  # the session goes on
    assert _decoded(session, ok.withColumns((Concat(Col("s"), Lit("!")), "r")), "r") == ["42!", None, "x!"]


def test_without_a_string_store_a_string_column_operand_fails(fresh):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Col, Concat
    t = fresh.table([ColumnData("s", expr.STR, np.array([5, 6], dtype=np.int64)), ColumnData("x", expr.I64, np.array([1, 2], dtype=np.int64))])
    assert len(fresh.dictionary) == 0
    out = t.withColumns((Concat(Col("s"), Col("x")), "r"))
    with pytest.raises(IllegalArgumentException, match="no string store"):
        out.size


def test_literal_operands_are_folded_and_a_null_literal_runs_nothing(session):
    from capsmi import expr
    from capsmi.expr import Col, Concat, Lit, ToString
    t = _table(session, s=["a", None, "b"], x=[1, 2, None])
    with Spy(session) as spy:
        def folded():
            out = t.withColumns((Concat(Lit("Hello"), Lit("World")), "hw"), (Concat(Lit("n"), Lit(-5)), "n5"), (ToString(Lit(mr.LONG_MIN)), "mn"),
                                (ToString(Lit(True)), "tt"), (ToString(Lit(None)), "un"), (Concat(Col("s"), Lit(None)), "cn"),
                                (Concat(Lit(None, expr.STR), Col("x")), "nc"))
            return out, out.size

        (out, n), launches, _ = _profiled(session, folded)
        merges = launches.pop("str_store_merge")  # a folded string that is new to the store is merged like any other
        assert n == 3 and launches == {k: 0 for k in TIMERS if k != "str_store_merge"} and merges <= 4, (launches, merges)
        assert spy.calls == [[b"HelloWorld"], [b"n-5"], [b"-9223372036854775808"], [b"true"]]  # one call, one string each
    for k, word in (("hw", "HelloWorld"), ("n5", "n-5"), ("mn", str(mr.LONG_MIN)), ("tt", "true")):
        assert _decoded(session, out, k) == [word] * 3, k
    for k in ("un", "cn", "nc"):
        assert out.columnType[k] == expr.STR and not _codes(out, k)[1].any(), k
    _, launches, _ = _profiled(session, lambda: t.withColumns((Concat(Col("s"), Col("x")), "r")).size)  # columns do launch
    assert launches["str_index"] == 1 and launches["str_make"] == 1 and launches["str_make_gather"] == 1
