"""UNWIND on the device (capsmi_explode / capsmi_explode_values / capsmi_table_add_list_column):
the golden cases of UnwindBehaviour.scala through the planner, and the operators against a NumPy
restatement kept in this file (np.repeat of the row index by list length plus the concatenated lists).
Exact equality, row order included: the header fixes the order as (input row, element position)."""
import json
import zlib

import numpy as np
import pytest

from golden_util import load_cases, run_planner, same_rows

pytestmark = pytest.mark.gpu

T = 2048  # kExplodeTile, the expansion kernel's tile of output rows (csrc/capsmi_impl.h; pinned by test_unwind_cpu)

CASES = load_cases("unwind.json")


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


def test_unwind_keeps_the_expand_route(session):
    """MATCH (a)-[r]->(b) UNWIND ...: the plan under the explode is routed as it is without the UNWIND."""
    case = next(c for c in CASES if c["name"] == "unwind after match")
    plain = dict(case, query={"clauses": [{"match": "(a)-[r]->(b)"}], "return": {"items": [["a", ["entity", "a"]]]}})
    names = ("expand", "expand_count", "two_hop", "triangle", "var_length", "miss")

    def routes(c):
        before = [session.route_count(n) for n in names]
        rows = run_planner(session, c)
        return [session.route_count(n) - b for n, b in zip(names, before)], rows

    d_plain, rows_plain = routes(plain)
    d_unwind, rows_unwind = routes(case)
    assert d_unwind == d_plain
    assert len(rows_unwind) == 3 * len(rows_plain)


# ---- the column form against the restatement --------------------------------------------------------
def _words(rng, elem, m, session):
    from capsmi.expr import BOOL, F64, STR
    if elem == F64:
        return np.round(rng.standard_normal(m), 3).view(np.int64)
    if elem == BOOL:
        return rng.integers(0, 2, m).astype(np.int64)
    if elem == STR:
        strings = [f"u{i:02d}" for i in range(30)]
        session.dictionary.extend(strings)
        codes = np.array([session.dictionary.encode(x) for x in strings], dtype=np.int64)
        return codes[rng.integers(0, 30, m)]
    return rng.integers(-(1 << 40), 1 << 40, m).astype(np.int64)


def _shape(name, rng):
    """(stored list lengths, validity or None).  A null row may store elements: they must not come out."""
    z = lambda k: [0] * k  # noqa: E731
    if name == "no_rows":
        return [], None
    if name == "all_empty_or_null":
        lens = [0, 3, 0, 0, 2, 0, 7, 0]
        return lens, [l == 0 and i % 2 == 0 for i, l in enumerate(lens)]
    if name == "one_row_one_element":
        return [1], None
    if name == "identity":
        return [1] * 5000, None
    if name == "one_long_list":
        return [3 * T + 5], None
    if name == "tile_edges":  # list boundaries at T, T + 1, 2T - 1, 2T, 3T, 3T + 1, 4T - 1, 6T - 1, 6T
        return [T, 1, T - 2, 1, T, 1, T - 2, 2 * T, 1, 9], None
    if name == "multiple_of_tile":
        return [700, 1348, T, 1, T - 1], None
    if name == "zero_runs":
        lens = z(T + 10) + [5] + z(2 * T + 3) + [T + 7] + [4] * (T + 1) + [1] + z(T + 5)
        valid = [True] * len(lens)
        for i in range(3 * T + 15, 3 * T + 15 + T + 1):  # the run of 4-element rows is null
            valid[i] = False
        valid[3] = valid[T + 40] = False  # and a few of the empty ones
        return lens, valid
    if name == "general":
        n = 200_000
        return (rng.geometric(1 / 8.0, n) - 1).tolist(), (rng.random(n) >= 0.3).tolist()
    raise KeyError(name)


def _restate(lens, valid, vals):
    """np.repeat of the row index by effective length, and the concatenation of the non-null rows' lists."""
    lens = np.asarray(lens, dtype=np.int64)
    ok = np.ones(len(lens), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    src = np.repeat(np.arange(len(lens), dtype=np.int64), np.where(ok, lens, 0))
    item = vals[np.repeat(ok, lens)]
    return src, item


def _list_table(session, rng, lens, valid, elem):
    from capsmi import ColumnData
    from capsmi.expr import F64, I64
    n = len(lens)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=offs[1:])
    vals = _words(rng, elem, int(offs[-1]), session)
    p = rng.integers(-50, 50, n).astype(np.int64)
    q = np.round(rng.standard_normal(n), 2)
    qv = rng.random(n) >= 0.25
    t = session.table([ColumnData("id", I64, np.arange(n, dtype=np.int64)), ColumnData("p", I64, p),
                       ColumnData("q", F64, q, qv)])
    t = t.add_list_column_csr("xs", elem, offs, vals, None if valid is None else np.asarray(valid, dtype=np.uint8))
    return t, vals, p, q, qv


def _col_words(c):
    return np.asarray(c.values).view(np.int64) if np.asarray(c.values).dtype == np.float64 else np.asarray(c.values)


SHAPES = ["no_rows", "all_empty_or_null", "one_row_one_element", "identity", "one_long_list", "tile_edges",
          "multiple_of_tile", "zero_runs"]


@pytest.mark.parametrize("elem_name", ["I64", "F64", "BOOL", "STR"])
@pytest.mark.parametrize("shape", SHAPES)
def test_explode_shapes(session, shape, elem_name):
    from capsmi import expr
    elem = getattr(expr, elem_name)
    rng = np.random.default_rng(zlib.crc32(f"{shape}/{elem_name}".encode()))
    lens, valid = _shape(shape, rng)
    t, vals, p, q, qv = _list_table(session, rng, lens, valid, elem)
    src, item = _restate(lens, valid, vals)
    out = t.explode("xs", "item")
    assert out.physicalColumns == ["id", "p", "q", "xs", "item"]
    assert out.columnType["item"] == elem and out.columnType["xs"] == expr.LIST + elem
    assert out.size == len(src)
    if shape == "multiple_of_tile":
        assert len(src) % T == 0 and len(src) > 0
    cols = {c.name: c for c in out.select("id", "p", "q", "item").to_columns()}
    assert cols["item"].valid is None  # non-nullable
    assert np.array_equal(_col_words(cols["item"]), item)
    assert np.array_equal(cols["id"].values, src)
    assert np.array_equal(cols["p"].values, p[src])
    if lens:  # (a table without rows stores no validity)
        assert np.array_equal(cols["q"].valid, qv[src])
        assert np.array_equal(_col_words(cols["q"])[qv[src]], q.view(np.int64)[src][qv[src]])
    if len(src) <= 64:  # withColumn keeps the list column: every output row still holds its whole list
        xs = out.column("xs")
        offs = np.concatenate([[0], np.cumsum(lens)])
        for j, r in enumerate(src):
            assert np.array_equal(np.asarray(xs.values[j]).view(np.int64), vals[offs[r]:offs[r + 1]])


@pytest.mark.parametrize("elem_name", ["I64", "STR"])
def test_explode_general(session, elem_name):
    """Geometric lengths, 30 % null rows, n = 2 * 10^5, m ~ 10^6."""
    from capsmi import expr
    rng = np.random.default_rng(77)
    lens, valid = _shape("general", rng)
    t, vals, p, _, _ = _list_table(session, rng, lens, valid, getattr(expr, elem_name))
    src, item = _restate(lens, valid, vals)
    assert 800_000 < len(src) < 1_200_000
    out = t.explode("xs", "item").select("id", "p", "item")
    assert out.size == len(src)
    assert np.array_equal(out.column("item").values, item)
    assert np.array_equal(out.column("id").values, src)
    assert np.array_equal(out.column("p").values, p[src])


# ---- arbitrary row words: any materialised table with a list column ------------------------------------
def _check(t, list_col):
    """Explode `t` (materialised here first, so its row order is fixed) and compare with the restatement
    over its exported rows."""
    cols = t.to_columns()
    n = t.size
    lc = next(c for c in cols if c.name == list_col)
    ok = np.ones(n, dtype=bool) if lc.valid is None else lc.valid
    rows = [np.asarray(lc.values[i]).view(np.int64) if ok[i] else np.empty(0, dtype=np.int64) for i in range(n)]
    src = np.repeat(np.arange(n, dtype=np.int64), [len(r) for r in rows])
    item = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
    out = t.explode(list_col, "item")
    assert out.size == len(src)
    assert np.array_equal(_col_words(out.column("item")), item)
    for c in cols:
        if c.name == list_col:
            continue
        g = out.column(c.name)
        v = np.ones(n, dtype=bool) if c.valid is None else c.valid
        assert (g.valid is None) == (c.valid is None), c.name
        if g.valid is not None:
            assert np.array_equal(g.valid, v[src]), c.name
        assert np.array_equal(_col_words(g)[v[src]], _col_words(c)[src][v[src]]), c.name
    return len(src)


def _grouped(session, seed, n=4000, keys=40):
    from capsmi import ColumnData
    from capsmi.expr import I64
    rng = np.random.default_rng(seed)
    k = rng.integers(0, keys, n).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    ok = rng.random(n) >= 0.2
    t = session.table([ColumnData("k", I64, k), ColumnData("v", I64, v, ok)])
    return t.group(["k"], [("collect", "v", False, "lv"), ("count_star", None, False, "n")]), k, v, ok


def test_explode_after_filter(session):
    from capsmi.expr import BinOp, Col, I64, Lit
    rng = np.random.default_rng(3)
    lens = (rng.geometric(0.15, 1500) - 1).tolist() + [0] * (T + 3) + (rng.geometric(0.15, 1500) - 1).tolist()
    t, *_ = _list_table(session, rng, lens, (rng.random(len(lens)) >= 0.2).tolist(), I64)
    assert _check(t.filter(BinOp(">", Col("p"), Lit(0))), "xs") > T


def test_explode_after_duplicating_join(session):
    """Each list row is matched by several probe rows: the same list index in many rows."""
    from capsmi import ColumnData
    from capsmi.expr import I64
    rng = np.random.default_rng(4)
    lens = (rng.geometric(0.2, 300) - 1).tolist()
    t, *_ = _list_table(session, rng, lens, (rng.random(300) >= 0.2).tolist(), I64)
    left = session.table([ColumnData("lid", I64, np.arange(2000, dtype=np.int64)),
                          ColumnData("k", I64, rng.integers(0, 350, 2000).astype(np.int64))])
    assert _check(left.join(t, "inner", ("k", "id")), "xs") > 2 * T


def test_explode_after_union_of_collects(session):
    """unionAll of two collect results: row words point into a merged store."""
    g1, *_ = _grouped(session, 11)
    g2, *_ = _grouped(session, 12, n=3000, keys=25)
    assert _check(g1.unionAll(g2), "lv") > T


def test_explode_after_order_skip_limit(session):
    """A skipped table: Column::offset is non-zero."""
    g, *_ = _grouped(session, 13)
    assert _check(g.orderBy(("n", "desc"), ("k", "asc")).skip(3).limit(20), "lv") > 0


def test_explode_of_collect_gives_the_groups_values(session):
    g, k, v, ok = _grouped(session, 14)
    out = g.explode("lv", "x").select("k", "x")
    gk, gx = out.column("k").values, out.column("x").values
    order = np.lexsort((v[ok], k[ok]))  # by group, the non-null values ascending (sort_array)
    by_group = np.argsort(gk, kind="stable")  # the group rows come in any order, their elements in list order
    assert np.array_equal(gk[by_group], k[ok][order])
    assert np.array_equal(gx[by_group], v[ok][order])


# ---- the constant form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 100_000])
@pytest.mark.parametrize("values", [[], [7], [3, None, -5], [1.5, 2, None], ["b", "a", "b"], [True, False]],
                         ids=["count0", "count1", "null_element", "doubles", "strings", "booleans"])
def test_explode_values(session, n, values):
    from capsmi import ColumnData, expr
    rng = np.random.default_rng(n + len(values))
    p = rng.integers(-9, 9, n).astype(np.int64)
    t = session.table([ColumnData("id", expr.I64, np.arange(n, dtype=np.int64)), ColumnData("p", expr.I64, p)])
    out = t.explodeValues(values, "item")
    c = len(values)
    assert out.physicalColumns == ["id", "p", "item"]
    assert out.size == n * c
    src = np.repeat(np.arange(n, dtype=np.int64), c)
    assert np.array_equal(out.column("id").values, src)
    assert np.array_equal(out.column("p").values, p[src])
    item = out.column("item")
    nulls = np.array([x is None for x in values], dtype=bool)
    assert (item.valid is not None) == bool(nulls.any())  # nullable exactly when a value is null
    if item.valid is not None:
        assert np.array_equal(item.valid, np.tile(~nulls, n))
    ty = expr.STR if "a" in values else expr.F64 if 1.5 in values else expr.BOOL if True in values and c == 2 else expr.I64
    assert out.columnType["item"] == ty
    if ty == expr.STR:
        want = np.array([session.dictionary.encode(x) for x in values], dtype=np.int64)
    elif ty == expr.F64:
        want = np.array([0.0 if x is None else float(x) for x in values], dtype=np.float64)
    else:
        want = np.array([0 if x is None else int(x) for x in values], dtype=np.int64)
    got, exp = np.asarray(item.values), np.tile(want, n)
    keep = np.tile(~nulls, n)
    assert np.array_equal(got[keep], exp[keep])


# ---- list ingest ---------------------------------------------------------------------------------------
def test_list_ingest_round_trip(session):
    from capsmi import ColumnData, expr
    rows = np.empty(5, dtype=object)
    data = [[1, 2, 3], [], [4], [9, 9], [5]]
    for i, r in enumerate(data):
        rows[i] = np.array(r, dtype=np.int64)
    valid = np.array([True, True, True, False, True])
    frows = np.empty(5, dtype=object)
    for i, r in enumerate(data):
        frows[i] = np.array(r, dtype=np.float64) / 2
    t = session.table([ColumnData("id", expr.I64, np.arange(5)), ColumnData("xs", expr.LIST + expr.I64, rows, valid),
                       ColumnData("fs", expr.LIST + expr.F64, frows)])
    assert t.physicalColumns == ["id", "xs", "fs"]
    assert t.columnType == {"id": expr.I64, "xs": expr.LIST + expr.I64, "fs": expr.LIST + expr.F64}
    back = {c.name: c for c in t.to_columns()}
    assert np.array_equal(back["xs"].valid, valid) and back["fs"].valid is None
    for i in range(5):
        if valid[i]:
            assert np.array_equal(back["xs"].values[i], rows[i])
        assert np.array_equal(back["fs"].values[i], frows[i])
    assert t.explode("xs", "x").column("x").values.tolist() == [1, 2, 3, 4, 5]
    alone = session.table([ColumnData("xs", expr.LIST + expr.I64, rows, valid)])  # no plain column at all
    assert alone.physicalColumns == ["xs"] and alone.explode("xs", "x").size == 5


@pytest.mark.parametrize("offsets", [[0, 2, 1, 3], [1, 2, 3, 3], [0, 2, 3]], ids=["decreasing", "not_from_zero", "too_few"])
def test_malformed_list_offsets_are_refused(session, offsets):
    from capsmi import ColumnData, expr
    from capsmi._lib import IllegalArgumentException
    t = session.table([ColumnData("id", expr.I64, np.arange(3))])
    with pytest.raises(IllegalArgumentException):
        t.add_list_column_csr("xs", expr.I64, offsets, np.arange(3))
    with pytest.raises(IllegalArgumentException):  # offsets that end past the values
        t.add_list_column_csr("xs", expr.I64, [0, 1, 2, 5], np.arange(3))
    with pytest.raises(IllegalArgumentException):  # an existing name
        t.add_list_column_csr("id", expr.I64, [0, 1, 2, 3], np.arange(3))


# ---- semantics -----------------------------------------------------------------------------------------
def _small(session, seed=21):
    from capsmi.expr import I64
    rng = np.random.default_rng(seed)
    lens = (rng.geometric(0.15, 1500) - 1).tolist()
    t, vals, p, _, _ = _list_table(session, rng, lens, (rng.random(1500) >= 0.2).tolist(), I64)
    return t, lens, vals, p


def test_filter_on_item_stays_above_the_explode(session):
    """A lazy filter that reads the item (alone, and together with a payload column whose conjunct may go
    below) gives the rows of filtering the materialised explode."""
    from capsmi.expr import Ands, BinOp, Col, Lit
    t, *_ = _small(session)
    preds = [BinOp(">", Col("item"), Lit(0)),
             Ands((BinOp(">", Col("p"), Lit(0)), BinOp("<", Col("item"), Lit(1 << 39)))),
             BinOp("<", Col("item"), Col("p"))]
    for pred in preds:
        lazy = t.explode("xs", "item").filter(pred).select("id", "p", "item")
        first = t.explode("xs", "item")
        assert first.size > T  # materialised before the filter is planned
        eager = first.filter(pred).select("id", "p", "item")
        assert 0 < lazy.size == eager.size < first.size
        for name in ("id", "p", "item"):
            assert np.array_equal(lazy.column(name).values, eager.column(name).values), name


def test_explode_twice_gives_one_fingerprint(session):
    t, *_ = _small(session)
    a = t.explode("xs", "item").fingerprint(["id", "p", "item"])
    b = t.explode("xs", "item").fingerprint(["id", "p", "item"])
    assert a == b and a[0] > T


def test_item_replaces_a_column_of_its_name(session):
    from capsmi import expr
    t, lens, vals, _ = _small(session)
    full = t.explode("xs", "item")
    over_p = t.explode("xs", "p")
    assert over_p.physicalColumns == ["id", "p", "q", "xs"]
    assert np.array_equal(over_p.column("p").values, full.column("item").values)
    over_xs = t.explode("xs", "xs")  # the item may take the list column's own name
    assert over_xs.physicalColumns == ["id", "p", "q", "xs"] and over_xs.columnType["xs"] == expr.I64
    assert np.array_equal(over_xs.column("xs").values, full.column("item").values)
    assert np.array_equal(over_xs.column("id").values, full.column("id").values)


def test_non_list_column_is_refused(session):
    from capsmi._lib import IllegalArgumentException
    t, *_ = _small(session)
    with pytest.raises(IllegalArgumentException):
        t.explode("p", "item")
    with pytest.raises(IllegalArgumentException):
        t.explode("nope", "item")


def test_explode_expression_in_with_columns(session):
    from capsmi._lib import NotImplementedException
    from capsmi.expr import BinOp, Col, Explode, ListLit, Lit, Param
    t, *_ = _small(session)
    want = t.explode("xs", "item")
    got = t.withColumns((Explode(Col("xs")), "item"))
    assert got.physicalColumns == want.physicalColumns
    assert np.array_equal(got.column("item").values, want.column("item").values)
    assert np.array_equal(got.column("id").values, want.column("id").values)
    # other columns of the same call are added around the generator, in order
    both = t.withColumns((BinOp("+", Col("p"), Lit(1)), "p1"), (Explode(Col("xs")), "item"),
                         (BinOp("+", Col("item"), Col("p1")), "s"))
    assert both.physicalColumns == ["id", "p", "q", "xs", "p1", "item", "s"]
    assert np.array_equal(both.column("s").values, want.column("item").values + want.column("p").values + 1)
    lit = t.limit(4).withColumns((Explode(ListLit((1, 2))), "item"))
    assert lit.column("item").values.tolist() == [1, 2] * 4
    session.set_params([5, [4, 5, 6]])
    try:
        par = t.limit(2).withColumns((Explode(Param(1)), "item"))
        assert par.column("item").values.tolist() == [4, 5, 6] * 2
        with pytest.raises(Exception):
            t.withColumns((Explode(Param(0)), "item"))  # a scalar parameter
    finally:
        session.set_params([])
    with pytest.raises(NotImplementedException):
        t.withColumns((Explode(Col("xs")), "a"), (Explode(Col("xs")), "b"))
    with pytest.raises(NotImplementedException):
        t.withColumns((BinOp("+", Explode(Col("xs")), Lit(1)), "a"))
    with pytest.raises(NotImplementedException):
        t.withColumns((Explode(Explode(Col("xs"))), "a"))


def test_schema_is_known_before_any_row(session):
    """Lazy like every Table[T] operator: names and types at once, errors at once."""
    from capsmi import expr
    t, *_ = _small(session)
    out = t.filter(expr.BinOp(">", expr.Col("p"), expr.Lit(0))).explode("xs", "item").explodeValues([None, 2.5], "w")
    assert out.physicalColumns == ["id", "p", "q", "xs", "item", "w"]
    assert out.columnType["item"] == expr.I64 and out.columnType["w"] == expr.F64
    assert out.select("w").column("w").valid is not None


def test_kernel_timers_and_bytes(session):
    """The `explode` timer declares 8 B x (n starts + n row words + m values + m items + m source rows)."""
    import ctypes
    from capsmi import _lib
    t, lens, *_ = _small(session)
    n = t.size
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        m = t.explode("xs", "item").size
        launches, ms, nbytes = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _lib.call("capsmi_session_kernel_bytes", session.handle, b"explode", ctypes.byref(nbytes))
        _lib.call("capsmi_session_kernel_time", session.handle, b"explode", ctypes.byref(launches), ctypes.byref(ms))
        assert launches.value == 1 and ms.value > 0
        assert nbytes.value == 8.0 * (2 * n + 3 * m)
        assert t.limit(10).explodeValues([1, 2, 3], "w").size == 30
        _lib.call("capsmi_session_kernel_time", session.handle, b"explode_values", ctypes.byref(launches),
                  ctypes.byref(ms))
        assert launches.value == 1
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)


def test_only_the_payload_columns_read_above_are_gathered(session):
    """Column pruning through the explode: the `explode_gather` timer declares 24 B per output row and
    gathered column, so its bytes tell how many payload columns a plan gathered."""
    import ctypes
    from capsmi import _lib
    t, *_ = _small(session)
    m = t.explode("xs", "item").size

    def gathered(plan):
        nbytes = ctypes.c_double()
        _lib.call("capsmi_session_kernel_bytes", session.handle, b"explode_gather", ctypes.byref(nbytes))  # reset
        assert plan.size == m
        _lib.call("capsmi_session_kernel_bytes", session.handle, b"explode_gather", ctypes.byref(nbytes))
        return nbytes.value / (24.0 * m)

    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        assert gathered(t.explode("xs", "item")) == 4  # id, p, q and the list column itself
        assert gathered(t.explode("xs", "item").select("item")) == 0
        assert gathered(t.explode("xs", "item").select("p", "item")) == 1
        assert gathered(t.explode("xs", "item").drop("xs", "q")) == 2
        assert gathered(t.explode("xs", "p")) == 3  # the replaced column is not gathered
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)
