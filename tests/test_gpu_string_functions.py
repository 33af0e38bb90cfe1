"""size(), toInteger(), toFloat() and toBoolean() of Strings on the device (CAPSMI_X_STR_SIZE .. CAPSMI_X_TO_BOOLEAN over
the session's string store, k_strconv.hip).  The golden cases of tests/golden/string_functions.json run through the
planner; everything else is compared bit for bit -- the value word, the sign of zero and the validity -- with the
pure-Python restatement of str_conv_ref.py, on the rows side and on the dictionary side (CAPSMI_STR_MATCH)."""
import ctypes
import json

import numpy as np
import pytest

import str_conv_ref as sr
from golden_util import load_cases, run_planner, same_rows

pytestmark = pytest.mark.gpu

CASES = load_cases("string_functions.json")
EDGES = load_cases("str_conv_cases.json")
MODES = ["rows", "dict"]
OPS = ("str_size", "str_tointeger", "str_tofloat", "toboolean")
T = 2048  # a tile of byte slots (kExplodeTile)


def _cls(op):
    from capsmi import expr
    return {"str_size": expr.StrSize, "str_tointeger": expr.StrToInteger, "str_tofloat": expr.StrToFloat,
            "toboolean": expr.ToBoolean}[op]


def _type(op):
    from capsmi import expr
    return {"str_size": expr.I64, "str_tointeger": expr.I64, "str_tofloat": expr.F64, "toboolean": expr.BOOL}[op]


@pytest.fixture
def fresh():
    """A session of its own, so that the test decides what the string store holds."""
    from capsmi import Session
    s = Session(0)
    yield s
    s.close()


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
    for g in got:
        for k, v in g.items():
            assert v is None or type(v) in {type(e[k]) for e in case["expected"] if e[k] is not None}, got


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


def _words(t, name):
    """(value words int64, validity bool) of a column; the word of a NULL row is set to 0."""
    c = t.column(name)
    v = np.ascontiguousarray(c.values)
    w = v.view(np.int64) if v.dtype == np.float64 else v.astype(np.int64)
    ok = np.ones(len(w), dtype=bool) if c.valid is None else np.asarray(c.valid, dtype=bool)
    return np.where(ok, w, 0), ok


def _want(op, strings):
    pairs = [sr.word_of(op, None if s is None else s.encode("utf-8", "surrogateescape")) for s in strings]
    return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=bool)


def _assert_bits(t, name, op, strings, what=""):
    (gw, gok), (ww, wok) = _words(t, name), _want(op, strings)
    assert len(gw) == len(ww), (what, len(gw), len(ww))
    bad = [(r, strings[r][:40] if strings[r] else strings[r], int(gw[r]), bool(gok[r]), int(ww[r]), bool(wok[r]))
           for r in np.flatnonzero((gw != ww) | (gok != wok))[:10]]
    assert not bad, (what, op, bad)


def _timer(session, name):
    from capsmi import _lib
    launches, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", session.handle, name.encode(), ctypes.byref(launches), ctypes.byref(ms))
    return launches.value


TIMERS = ("str_index", "str_conv", "str_conv_starts", "str_conv_lookup")


def _profiled(session, fn):
    """fn() with profiling on: (its result, {timer: launches})."""
    from capsmi import _lib
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        for k in TIMERS:
            _timer(session, k)  # reset
        res = fn()
        return res, {k: _timer(session, k) for k in TIMERS}
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)


# ---- the edge tables -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", OPS)
def test_edge_table(session, knobs, op, mode):
    """The inputs of tests/golden/str_conv_cases.json that are text (the ill-formed entry has a test of its own)."""
    from capsmi import expr
    from capsmi.expr import Col
    knobs(session, CAPSMI_STR_MATCH=mode)
    cases = [c for c in EDGES if c["op"] == op and not c["raw"]]
    s = [None if c["in"] is None else bytes.fromhex(c["in"]).decode("utf-8") for c in cases]
    assert 8 <= len(s) <= 80 and None in s
    t = _table(session, s=s)
    out = t.withColumns((_cls(op)(Col("s")), "r"))
    assert out.columnType["r"] == _type(op)
    gw, gok = _words(out, "r")
    bad = [(c["in"][:60], int(gw[r]), bool(gok[r]), c["word"], c["ok"]) for r, c in enumerate(cases)
           if int(gw[r]) != int(c["word"]) or bool(gok[r]) != bool(c["ok"])]
    assert not bad, bad[:10]
    _assert_bits(out, "r", op, s)  # the fixture is what the restatement gives


def test_toboolean_of_a_boolean_column_is_the_identity(session):
    from capsmi import ColumnData, expr
    from capsmi.expr import Col, Lit, ToBoolean
    b = ColumnData("b", expr.BOOL, np.array([1, 0, 0, 1, 1], dtype=np.int64), np.array([True, True, False, True, False]))
    out = session.table([b]).withColumns((ToBoolean(Col("b")), "r"), (ToBoolean(Lit(True)), "t"), (ToBoolean(Lit(None, expr.BOOL)), "n"))
    assert [out.columnType[k] for k in ("r", "t", "n")] == [expr.BOOL] * 3
    w, ok = _words(out, "r")
    assert w.tolist() == [1, 0, 0, 1, 0] and ok.tolist() == [True, True, False, True, False]
    assert _words(out, "t")[0].tolist() == [1] * 5 and not _words(out, "n")[1].any()


@pytest.mark.parametrize("mode", MODES)
def test_size_of_ill_formed_bytes_through_the_raw_store_call(fresh, knobs, mode):
    """A store registered with capsmi_session_set_strings itself: one entry is no UTF-8.  The count is that of the
    bytes that are not 10xxxxxx."""
    from capsmi import ColumnData, _lib, expr
    from capsmi.table import GpuTable, _EXPR_PTR
    knobs(fresh, CAPSMI_STR_MATCH=mode)
    (raw,) = [c for c in EDGES if c["raw"]]
    entries = [b"", bytes.fromhex(raw["in"]), "日本語".encode(), b"\xbf\xbf\xbf"]
    codes = np.array([10, 20, 30, 40], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in entries])]).astype(np.int64)
    _lib.call("capsmi_session_set_strings", fresh.handle, 4, codes.ctypes.data, offsets.ctypes.data, b"".join(entries))
    rows = [1, 0, 3, 2, 1, 1]
    t = fresh.table([ColumnData("s", expr.STR, codes[rows], np.array([True, True, True, True, False, True]))])
    prog = expr.to_ctypes([(expr.X_COL, 0, 0, 0), (expr.X_STR_SIZE, 0, 0, 0)])
    cols = (_lib.ExprColumn * 1)()
    cols[0].name, cols[0].nnodes, cols[0].prog = b"r", 2, ctypes.cast(prog, _EXPR_PTR)
    h = ctypes.c_void_p()
    _lib.call("capsmi_with_columns", t._h, 1, cols, ctypes.byref(h))
    w, ok = _words(GpuTable(fresh, h), "r")
    want = [sr.size(entries[k]) for k in rows]
    assert want[0] == int(raw["word"]) == 4 and want[2] == 0
    assert ok.tolist() == [True, True, True, True, False, True]
    assert w.tolist() == [x if v else 0 for x, v in zip(want, ok)]


# ---- random numbers ----------------------------------------------------------------------------------
RANDOM = {}


def _random_numbers():
    """2000 random doubles (any bit pattern that is finite) printed at 17 significant digits, which identify a double,
    and 2000 random 25-digit decimals with exponents in [-340, 310]."""
    if not RANDOM:
        rng = np.random.default_rng(58)
        d = rng.integers(-2 ** 63, 2 ** 63 - 1, 2600, dtype=np.int64).view(np.float64)
        d = d[np.isfinite(d)][:2000]
        RANDOM["d"] = d
        RANDOM["s17"] = ["%.17g" % x for x in d]
        RANDOM["s25"] = ["".join(map(str, rng.integers(0, 10, 25))) + "e" + str(int(rng.integers(-340, 311))) for _ in range(2000)]
    return RANDOM


@pytest.mark.parametrize("mode", MODES)
def test_random_doubles_and_long_decimals_bit_for_bit(session, knobs, mode):
    from capsmi.expr import Col, StrToFloat
    knobs(session, CAPSMI_STR_MATCH=mode)
    r = _random_numbers()
    assert len(r["d"]) == 2000 and len(set(r["s25"])) == 2000
    t = _table(session, a=r["s17"], b=r["s25"])
    out = t.withColumns((StrToFloat(Col("a")), "fa"), (StrToFloat(Col("b")), "fb"))
    w, ok = _words(out, "fa")
    assert ok.all() and np.array_equal(w, r["d"].view(np.int64))  # 17 digits read back give the double itself
    _assert_bits(out, "fa", "str_tofloat", r["s17"])
    _assert_bits(out, "fb", "str_tofloat", r["s25"])
    want = _want("str_tofloat", r["s25"])[0].view(np.float64)
    assert np.isinf(want).any() and (np.abs(want) < 2.2e-308).any()  # overflow, and subnormals


# ---- shapes ------------------------------------------------------------------------------------------
def _pool():
    """300 distinct strings: numbers of every form, the boolean words, text of 1 to 4 bytes per character."""
    rng = np.random.default_rng(300)
    pool = ["", "true", "FALSE", "y", "No", "0", "1", "é", "日本語", "\U0001F600x", "-0", "1e5", ".5", "0x1p3", "NaN", "-Infinity",
            "2147483647", "2147483648", "-2147483648", "82.9", " 1", "12345678901234567890123", "4.9e-324", "1e400"]
    k = 0
    while len(pool) < 300:
        v = [str(int(rng.integers(-3000, 3000))), "%.17g" % float(rng.standard_normal() * 10.0 ** int(rng.integers(-30, 30))),
             "ab" * int(rng.integers(1, 9)) + "é" * int(rng.integers(0, 3)), str(int(rng.integers(0, 99))) + "." + str(k)][k % 4]
        if v not in pool:
            pool.append(v)
        k += 1
    return pool


SHAPES = [0, 1, 255, 256, 257, 8192 * 256 + 1]


@pytest.mark.parametrize("mode", ["auto"] + MODES)
@pytest.mark.parametrize("n", SHAPES)
def test_shapes_over_a_300_entry_dictionary(fresh, n, mode):
    """One row, around one block, and one row more than the capped grid covers in one stride; under auto the rows side
    below 300 rows and the store from there on, seen in the launches of the lookup.  Every shape runs twice."""
    from capsmi.expr import Col
    fresh.set_config("CAPSMI_STR_MATCH", mode)
    pool = _pool()
    fresh.dictionary.extend(pool)
    assert len(fresh.dictionary) == 300
    rng = np.random.default_rng(n + 1)
    pick = rng.integers(0, 300, n)
    null = rng.random(n) < 0.1
    s = [None if z else pool[k] for k, z in zip(pick, null)]
    t = _table(fresh, s=s)
    cols = [(_cls(op)(Col("s")), op) for op in OPS]

    def twice():
        a, b = t.withColumns(*cols), t.withColumns(*cols)
        return a, b, a.size, b.size  # the actions run here

    out, launches = _profiled(fresh, twice)
    assert out[2] == out[3] == n and out[0].fingerprint(list(OPS)) == out[1].fingerprint(list(OPS))
    per = {op: _want(op, pool) for op in OPS}  # the reference once per entry, gathered
    for op in OPS:
        gw, gok = _words(out[0], op)
        wok = per[op][1][pick] & ~null
        assert np.array_equal(gok, wok), op
        assert np.array_equal(gw, np.where(wok, per[op][0][pick], 0)), op
    dict_side = n > 0 and (mode == "dict" or (mode == "auto" and n >= 300))
    assert launches["str_conv_lookup"] == (2 * len(OPS) if dict_side else 0), launches
    assert launches["str_index"] == (2 * len(OPS) if n > 0 else 0), launches
    assert len(fresh.dictionary) == 300


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ["no_bytes", "one_tile", "one_tile_and_a_byte", "more_tiles_than_blocks"])
def test_size_tile_edges(fresh, shape, mode):
    """The size pass over a byte array of 0 bytes, of one tile exactly, of one byte more, and of more tiles than the
    grid has blocks (so a block walks several).  The table holds every store entry once and a NULL row, so both sides
    see these totals."""
    from capsmi.expr import Col, StrSize
    fresh.set_config("CAPSMI_STR_MATCH", mode)
    if shape == "no_bytes":
        s = ["", None]
    elif shape == "more_tiles_than_blocks":
        import torch
        cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
        big = ("aé日\U0001F600" * (1 << 16))  # 10 bytes, 4 characters a piece: 640 KiB
        s = [big + "x" * k for k in range(-(-(cap * T + 1) // len(big.encode())) + 1)] + ["", None, "tail"]
        assert sum(len(x.encode()) for x in s if x) > cap * T
    else:
        total = T if shape == "one_tile" else T + 1
        s = ["é" * 500, "", "ab", None, "日本語" * 100, "q" * 7]
        s.append("z" * (total - sum(len(x.encode()) for x in s if x)))
        assert sum(len(x.encode()) for x in s if x) == total
    t = _table(fresh, s=s)
    out = (t.withColumns((StrSize(Col("s")), "r")), t.withColumns((StrSize(Col("s")), "r")))
    w, ok = _words(out[0], "r")
    assert ok.tolist() == [x is not None for x in s]
    assert w.tolist() == [0 if x is None else len(x) for x in s]  # code points are what Python's str counts
    assert out[0].fingerprint(["r"]) == out[1].fingerprint(["r"])


# ---- skew --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_mebibyte_of_digits_among_ten_thousand_short_strings(fresh, mode):
    from capsmi.expr import Col
    fresh.set_config("CAPSMI_STR_MATCH", mode)
    long = "0" * ((1 << 20) - 20) + "12345678901234567891"
    assert len(long) == 1 << 20
    s = [str(k) for k in range(5000)] + [long] + [str(k) + ".5" for k in range(5000)]
    t = _table(fresh, s=s)
    out = t.withColumns(*[(_cls(op)(Col("s")), op) for op in OPS[:3]])
    for op in OPS[:3]:
        _assert_bits(out, op, op, s, mode)
    w, ok = _words(out, "str_tointeger")
    assert not ok[5000] and ok[:5000].all()  # out of range
    f = _words(out, "str_tofloat")[0].view(np.float64)[5000]
    assert f == 1.2345678901234567891e19
    assert _words(out, "str_size")[0][5000] == 1 << 20


# ---- composition ---------------------------------------------------------------------------------------
def _mixed_rows(n=300):
    rng = np.random.default_rng(17)
    pool = ["42", "7", "41", "40", "-3", "82.9", "1e3", "", "true", "No", "x", "é", "0", "1", "3", "2", "100", "abc", " 5", "y", "F"]
    s = [None if rng.random() < 0.15 else pool[int(k)] for k in rng.integers(0, len(pool), n)]
    return s


def test_under_case_and_coalesce(session):
    from capsmi import expr
    from capsmi.expr import BinOp, Case, Coalesce, Col, Lit, StrSize, StrToFloat, StrToInteger, ToBoolean
    s = _mixed_rows()
    t = _table(session, s=s)
    early = BinOp("<", Col("id"), Lit(150))
    out = t.withColumns((Coalesce((StrToInteger(Col("s")), Lit(-1))), "ci"), (Coalesce((StrToFloat(Col("s")), Lit(-1.0))), "cf"),
                        (Coalesce((ToBoolean(Col("s")), Lit(False))), "cb"), (Coalesce((StrSize(Col("s")), Lit(-1))), "cs"),
                        (Case(((early, StrToInteger(Col("s"))),), Lit(-7)), "ki"), (Case(((early, StrToFloat(Col("s"))),), Lit(0.5)), "kf"),
                        (Case(((ToBoolean(Col("s")), StrSize(Col("s"))),), Lit(-9)), "kb"))
    assert [out.columnType[k] for k in ("ci", "cf", "cb", "cs", "ki", "kf", "kb")] == \
        [expr.I64, expr.F64, expr.BOOL, expr.I64, expr.I64, expr.F64, expr.I64]

    def col(name):
        w, ok = _words(out, name)
        return [int(x) if v else None for x, v in zip(w, ok)]

    i, f, b, z = ([fn(x) for x in s] for fn in (sr.to_integer, sr.to_float_bits, sr.to_boolean, sr.size))
    assert sum(v is not None for v in i) > 50 and sum(v is not None for v in b) > 50 and i.count(None) > 50
    assert col("ci") == [-1 if v is None else v for v in i]
    assert col("cf") == [sr.bits_of(-1.0) if v is None else v for v in f]
    assert col("cb") == [0 if v is None else int(v) for v in b]
    assert col("cs") == [-1 if v is None else v for v in z]
    assert col("ki") == [v if r < 150 else -7 for r, v in enumerate(i)]
    assert col("kf") == [v if r < 150 else sr.bits_of(0.5) for r, v in enumerate(f)]
    assert col("kb") == [zz if bb is True else -9 for zz, bb in zip(z, b)]


@pytest.mark.parametrize("mode", MODES)
def test_in_a_filter_as_an_in_probe_and_as_a_list_index(session, knobs, mode):
    from capsmi import expr
    from capsmi.expr import BinOp, Col, In, Index, InList, Lit, StrToInteger
    knobs(session, CAPSMI_STR_MATCH=mode)
    s = _mixed_rows()
    n = len(s)
    rng = np.random.default_rng(5)
    lists = [rng.integers(0, 50, int(rng.integers(0, 5))).tolist() for _ in range(n)]
    offs = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    t = _table(session, s=s).add_list_column_csr("xs", expr.I64, offs, np.array([v for l in lists for v in l], dtype=np.int64))
    i = [sr.to_integer(x) for x in s]
    kept = t.filter(BinOp(">", StrToInteger(Col("s")), Lit(40)))
    want = [r for r in range(n) if i[r] is not None and i[r] > 40]
    assert len(want) > 20 and _words(kept, "id")[0].tolist() == want
    out = t.withColumns((In(StrToInteger(Col("s")), (Lit(42), Lit(7), Lit(0))), "in"), (InList(StrToInteger(Col("s")), Col("xs")), "inl"),
                        (Index(Col("xs"), StrToInteger(Col("s"))), "ix"))

    def col(name):
        w, ok = _words(out, name)
        return [int(x) if v else None for x, v in zip(w, ok)]

    assert col("in") == [None if v is None else int(v in (42, 7, 0)) for v in i]
    assert col("inl") == [None if v is None else int(v in l) for v, l in zip(i, lists)]
    want_ix = [None if v is None or not 0 <= v < len(l) else l[v] for v, l in zip(i, lists)]
    assert sum(v is not None for v in want_ix) > 5 and col("ix") == want_ix


def test_beside_a_contains_and_a_log_in_one_program(session):
    """Three kinds of node in one program: the string match and the conversion run as passes of their own, one after
    the other, and the rest, which holds the Log, takes the interpreter's math instantiation."""
    from capsmi.expr import Ands, BinOp, Col, Contains, Lit, Log, StrToFloat
    s = ["2.5", "a3.0", "4.0a", "0.5", "9a", "-1.0a", None, "a", "1e1a", "0xap2"]
    t = _table(session, s=s + ["a"])
    pred = Ands((Contains(Col("s"), Lit("a")), BinOp(">", Log(StrToFloat(Col("s"))), Lit(0.0))))
    w, ok = _words(t.withColumns((pred, "m")), "m")
    # contains 'a' and log(toFloat) > 0: toFloat is NULL for every string that holds an 'a' but the hex float's; AND:
    # FALSE wins over NULL
    got = [int(x) if v else None for x, v in zip(w, ok)]
    assert got == [0, None, None, 0, None, None, None, None, None, 1, None]
    assert _words(t.filter(pred), "id")[0].tolist() == [9]


def test_in_a_table_at_the_column_limit(session):
    """64 columns: the lowered node cannot append its result column and borrows a slot the rest does not read."""
    from functools import reduce
    from capsmi import ColumnData, expr
    from capsmi.expr import Ands, BinOp, Col, Lit, StrToInteger, ToBoolean
    s = _mixed_rows()
    n = len(s)
    cols = [ColumnData("id", expr.I64, np.arange(n, dtype=np.int64)), _str_col(session, "s", s), _str_col(session, "u", s[::-1])]
    cols += [ColumnData(f"f{k}", expr.I64, np.full(n, k, dtype=np.int64)) for k in range(61)]
    t = session.table(cols)
    assert len(t.physicalColumns) == 64
    others = reduce(lambda a, b: BinOp("+", a, b), [Col("id")] + [Col(f"f{k}") for k in range(61)])  # id + 0 + .. + 60
    pred = Ands((BinOp(">", StrToInteger(Col("s")), Lit(2)), ToBoolean(Col("u")), BinOp(">=", others, Lit(1830 + 40))))

    def and3(*v):
        return False if False in v else None if None in v else True

    i, b = [sr.to_integer(x) for x in s], [sr.to_boolean(x) for x in s[::-1]]
    want = [and3(None if i[r] is None else i[r] > 2, b[r], r >= 40) for r in range(n)]
    assert want.count(True) > 3 and want.count(None) > 10
    w, ok = _words(t.withColumns((pred, "m")), "m")
    assert [bool(x) if v else None for x, v in zip(w, ok)] == want
    assert _words(t.filter(pred), "id")[0].tolist() == [r for r in range(n) if want[r] is True]


def test_a_tointeger_filter_keeps_the_expand_route(session):
    """MATCH (a)-[r]->(b) WHERE toInteger(a.age) > 40 RETURN a: pushed down like any conjunct, so the plan is routed as
    the plain match is, and gives the rows of the unrouted run."""
    create = ("CREATE (:A {age: '41'})-[:R]->(:B {age: '5'}), (:A {age: '40'})-[:R]->(:B {age: '0'}), (:A {age: '82.9'})-[:R]->(:B), "
              "(:A {age: 'old'})-[:R]->(:A {age: '77'})-[:R]->(:B), (:A)-[:R]->(:B {age: '99'})")
    ret = {"items": [["a", ["entity", "a"]]]}
    plain = {"create": create, "query": {"clauses": [{"match": "(a)-[r]->(b)"}], "return": ret}}
    where = [">", ["str_tointeger", ["prop", "a", "age"]], ["lit", 40]]
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
    assert len(rows_plain) == 6 and sorted(r["a"]["props"]["age"] for r in rows_where) == ["41", "77", "82.9"]
    assert same_rows(rows_where, rows_unfused)


# ---- refusals and errors -------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
def test_operand_types_are_checked_when_the_node_is_built(session, op):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException, NotImplementedException
    from capsmi.expr import BinOp, Coalesce, Col, Lit
    t = session.table([ColumnData("x", expr.I64, np.array([1, 2], dtype=np.int64)), ColumnData("f", expr.F64, np.array([1.0, 2.0])),
                       ColumnData("b", expr.BOOL, np.array([1, 0], dtype=np.int64)), _str_col(session, "s", ["a", "b"])])
    t = t.add_list_column_csr("xs", expr.STR, [0, 1, 1], [session.dictionary.encode("a")])
    bad = [Col("x"), Col("f"), Lit(3), Lit(2.5), Lit(None, expr.I64), Coalesce((Col("s"), Col("x"))), Coalesce((Col("x"), Col("s")))]
    if op != "toboolean":
        bad += [Col("b"), Lit(True), Lit(None, expr.BOOL)]
    for e in bad:
        with pytest.raises(IllegalArgumentException):
            t.withColumns((_cls(op)(e), "r"))
        with pytest.raises(IllegalArgumentException):
            t.filter(BinOp("=", _cls(op)(e), Lit(1)))
    with pytest.raises(NotImplementedException, match="list"):
        t.withColumns((_cls(op)(Col("xs")), "r"))
    out = t.withColumns((_cls(op)(Lit(None)), "u"), (_cls(op)(Lit(None, expr.STR)), "n"))
    assert out.columnType["u"] == out.columnType["n"] == _type(op)
    assert not _words(out, "u")[1].any() and not _words(out, "n")[1].any()


@pytest.mark.parametrize("op", OPS)
def test_without_a_string_store_the_action_fails(fresh, op):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Col
    t = fresh.table([ColumnData("s", expr.STR, np.array([5, 6], dtype=np.int64))])
    assert len(fresh.dictionary) == 0
    out = t.withColumns((_cls(op)(Col("s")), "r"))  # the node is built
    with pytest.raises(IllegalArgumentException, match="no string store"):
        out.size


@pytest.mark.parametrize("mode", MODES)
def test_a_code_outside_the_store_fails_the_action(session, knobs, mode):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException
    from capsmi.expr import Col, StrToInteger
    knobs(session, CAPSMI_STR_MATCH=mode)
    good = session.dictionary.encode("42")
    raw = np.array([good, 12345, good, -7], dtype=np.int64)  # words that are no codes of the dictionary
    t = session.table([ColumnData("s", expr.STR, raw, np.array([True, True, False, True]))])
    out = t.withColumns((StrToInteger(Col("s")), "r"))
    with pytest.raises(IllegalArgumentException, match="registered"):
        out.size
    ok = _table(session, s=["42", None, "x"])  # the session goes on
    w, v = _words(ok.withColumns((StrToInteger(Col("s")), "r")), "r")
    assert w.tolist() == [42, 0, 0] and v.tolist() == [True, False, False]


def test_literal_operands_are_folded_and_a_null_literal_runs_nothing(session):
    from capsmi import expr
    from capsmi.expr import Col, Lit, StrSize, StrToFloat, StrToInteger, ToBoolean
    t = _table(session, s=["a", None, "b"])

    def folded():
        out = t.withColumns((StrSize(Lit("日本語")), "z"), (StrToInteger(Lit("-82.9")), "i"), (StrToInteger(Lit("1e3")), "ni"),
                            (StrToFloat(Lit("-0")), "f"), (ToBoolean(Lit("YES")), "b"), (ToBoolean(Lit("maybe")), "nb"),
                            (StrSize(Lit(None)), "nz"), (StrToFloat(Lit(None, expr.STR)), "nf"))
        return out, out.size

    (out, n), launches = _profiled(session, folded)
    assert n == 3 and launches == {k: 0 for k in TIMERS}, launches
    assert [out.columnType[k] for k in ("z", "i", "ni", "f", "b", "nb", "nz", "nf")] == \
        [expr.I64, expr.I64, expr.I64, expr.F64, expr.BOOL, expr.BOOL, expr.I64, expr.F64]
    for k, word in (("z", 3), ("i", -82), ("f", sr.bits_of(-0.0)), ("b", 1)):
        w, ok = _words(out, k)
        assert ok.all() and w.tolist() == [word] * 3, k
    for k in ("ni", "nb", "nz", "nf"):
        assert not _words(out, k)[1].any(), k
    # a column operand does launch
    _, launches = _profiled(session, lambda: t.withColumns((StrToInteger(Col("s")), "r")).size)
    assert launches["str_index"] == 1 and launches["str_conv"] == 1
