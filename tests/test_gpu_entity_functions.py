"""labels(), keys() and type() on the device: capsmi_with_mask_list_column (k_masklist.hip) and the expressions
Labels / Keys / RelType.  The golden cases of tests/golden/entity_functions.json run through the planner, routed
and unfused; the operator is compared, exactly and in row order, with the pure-Python restatement of
entity_fn_ref.py over the rows the input table exports.  Shapes are built around T, the tile of (row, position)
slots, and K = 64, the columns one mask word holds."""
import json
import zlib

import numpy as np
import pytest

from entity_fn_ref import MASK_NOT_NULL, MASK_TRUE, ref_keys, ref_labels, ref_mask_list, ref_rel_type
from golden_util import load_cases, run_planner, same_rows
from list_expr_ref import T, ref_in_list, ref_index, ref_size

pytestmark = pytest.mark.gpu

CASES = load_cases("entity_functions.json")
MODES = [MASK_TRUE, MASK_NOT_NULL]
MODE_IDS = ["true", "not_null"]
LIST_STR = 11


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
def _col(name, ty, values, valid=None):
    from capsmi import ColumnData
    return ColumnData(name, ty, np.asarray(values), None if valid is None else np.asarray(valid, dtype=bool))


def _names(k):
    return [f"N{k - 1 - i:02d}" for i in range(k)]  # descending: the library keeps the order given


def _build(session, mode, passes, rng):
    """A table id, c00 .. whose column i passes in row r exactly where passes[i, r].  MASK_TRUE: Boolean flags,
    the even columns nullable -- a cell that does not pass is FALSE, NULL over a FALSE word or NULL over a TRUE
    word -- the odd ones not.  MASK_NOT_NULL: Long / Double / Boolean / String columns whose validity is `passes`;
    a column that passes everywhere has no validity bytes unless its number is a multiple of 3."""
    from capsmi import expr
    k, n = passes.shape
    cols = [_col("id", expr.I64, np.arange(n, dtype=np.int64))]
    code = session.encode_str("stored")
    for i in range(k):
        p = passes[i]
        if mode == MASK_TRUE:
            if i % 2 == 0:
                kind = rng.integers(0, 3, n)
                word = np.where(p, 1, (kind == 1).astype(np.int64))
                valid = p | (kind == 0)
                cols.append(_col(f"c{i:02d}", expr.BOOL, word, valid))
            else:
                cols.append(_col(f"c{i:02d}", expr.BOOL, p.astype(np.int64)))
        else:
            ty = (expr.I64, expr.F64, expr.BOOL, expr.STR)[i % 4]
            vals = {expr.I64: rng.integers(-5, 5, n), expr.F64: rng.standard_normal(n), expr.BOOL: rng.integers(0, 2, n),
                    expr.STR: np.full(n, code, dtype=np.int64)}[ty]
            cols.append(_col(f"c{i:02d}", ty, vals, None if (p.all() and i % 3) else p))
    return session.table(cols), [f"c{i:02d}" for i in range(k)]


def _exported(t, cols):
    """(value, valid) per row of the materialised table's columns: what the restatement reads."""
    out = []
    for c in cols:
        cd = t.column(c)
        n = len(cd.values)
        valid = np.ones(n, dtype=bool) if cd.valid is None else cd.valid
        vals = [None] * n if cd.type >= 8 else cd.values.tolist()
        out.append(list(zip(vals, valid.tolist())))
    return out


def _lists(session, t, name):
    """A non-nullable String list column as Python lists."""
    c = t.column(name)
    assert c.type == LIST_STR and c.valid is None
    return [[session.dictionary.decode(int(w)) for w in row] for row in c.values]


def _check(session, t, mode, cols, names, name="out"):
    """withMaskListColumn over t against the restatement of t's own rows; returns the expected lists."""
    n = t.size  # materialise: the row order is fixed from here on
    want = ref_mask_list(mode, _exported(t, cols), names) if cols else [[] for _ in range(n)]
    out = t.withMaskListColumn(mode, cols, names, name)
    assert out.columnType[name] == LIST_STR
    assert _lists(session, out, name) == want
    if "id" in t.physicalColumns and name != "id":
        assert np.array_equal(out.column("id").values, t.column("id").values)
    return want


# ---- shapes, in both modes ---------------------------------------------------------------------------
SHAPES = ["no_rows", "one_row_one_column", "no_columns", "full_32_rows_one_tile", "full_33_rows", "full_65_rows",
          "random_64_columns", "random_3_columns", "empty_rows_then_one_full", "one_full_then_empty_rows", "no_empty_row",
          "bit_63_only_and_bit_0_only"]


def _passes(shape, rng):
    full = lambda n: np.ones((64, n), dtype=bool)  # noqa: E731
    if shape == "no_rows":
        return np.zeros((3, 0), dtype=bool)
    if shape == "one_row_one_column":
        return np.ones((1, 1), dtype=bool)
    if shape == "no_columns":
        return np.zeros((0, 10), dtype=bool)
    if shape == "full_32_rows_one_tile":
        assert 32 * 64 == T  # m = T exactly
        return full(32)
    if shape == "full_33_rows":
        return full(33)
    if shape == "full_65_rows":  # two tiles and one row
        return full(64 + 1)
    if shape == "random_64_columns":
        return rng.random((64, 5000)) < 0.5
    if shape == "random_3_columns":
        return rng.random((3, 3 * T + 1)) < 0.5
    if shape in ("empty_rows_then_one_full", "one_full_then_empty_rows"):  # the compacted path
        p = np.zeros((64, 2 * T + 6), dtype=bool)
        p[:, -1 if shape == "empty_rows_then_one_full" else 0] = True
        return p
    if shape == "no_empty_row":  # the path without compaction
        p = rng.random((5, 3000)) < 0.4
        p[rng.integers(0, 5, 3000), np.arange(3000)] = True
        return p
    p = full(40)
    p[:, 7] = False
    p[63, 7] = True
    p[:, 23] = False
    p[0, 23] = True
    return p


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(session, shape, mode):
    rng = np.random.default_rng(zlib.crc32(f"{shape}{mode}".encode()))
    passes = _passes(shape, rng)
    t, cols = _build(session, mode, passes, rng)
    names = _names(len(cols))
    want = _check(session, t, mode, cols, names)
    assert [len(w) for w in want] == passes.sum(axis=0).tolist()  # the table holds what the shape says
    if shape == "bit_63_only_and_bit_0_only":
        assert want[7] == [names[63]] and want[23] == [names[0]] and want[8] == names


# ---- MASK_TRUE ---------------------------------------------------------------------------------------
def test_true_words_under_null_rows_are_not_seen(session):
    from capsmi import expr
    a = _col("a", expr.BOOL, [1, 1, 0, 1, 0], [1, 0, 1, 0, 0])   # nullable, NULLs over TRUE and FALSE words
    b = _col("b", expr.BOOL, [0, 1, 1, 1, 1])                     # non-nullable
    c = _col("c", expr.BOOL, [1, 1, 1, 1, 1], [0, 0, 0, 0, 1])   # TRUE everywhere, NULL but once
    t = session.table([_col("id", expr.I64, np.arange(5)), a, b, c])
    want = _check(session, t, MASK_TRUE, ["a", "b", "c"], ["A", "B", "C"])
    assert want == [["A"], ["B"], ["B"], ["B"], ["B", "C"]]
    assert _check(session, t, MASK_TRUE, ["c", "a"], ["C", "A"]) == [["A"], [], [], [], ["C"]]  # the order given


# ---- MASK_NOT_NULL -----------------------------------------------------------------------------------
def test_keys_over_mixed_types_and_a_list_column(session):
    from capsmi import expr
    n = 6
    code = session.encode_str("x")
    t = session.table([_col("id", expr.I64, np.arange(n)),
                       _col("i", expr.I64, np.arange(n), [1, 0, 1, 1, 0, 1]),
                       _col("f", expr.F64, np.full(n, np.nan)),                    # NaN is a value; non-nullable
                       _col("s", expr.STR, np.full(n, code), [0, 0, 1, 1, 1, 0]),
                       _col("b", expr.BOOL, np.zeros(n, dtype=np.int64), [1, 1, 0, 1, 1, 1])])  # FALSE is a value
    # a null list row that stores elements, a non-null empty list, and lists of one and two elements
    t = t.add_list_column_csr("xs", expr.I64, [0, 2, 2, 3, 3, 5, 5], [1, 2, 3, 4, 5], np.array([0, 1, 1, 0, 1, 1], dtype=np.uint8))
    cols = ["xs", "s", "i", "f", "b"]
    want = _check(session, t, MASK_NOT_NULL, cols, ["xs", "s", "i", "f", "b"])
    assert want[0] == ["i", "f", "b"]               # the null list row does not pass
    assert want[1] == ["xs", "f", "b"]              # the empty list passes
    assert want[5] == ["xs", "i", "f", "b"]
    assert all("f" in w for w in want)


# ---- errors and the replace-or-append rule ------------------------------------------------------------
def test_more_than_64_columns_is_unsupported(session):
    from capsmi import expr
    from capsmi._lib import UnsupportedOperationException
    t = session.table([_col(f"c{i:02d}", expr.BOOL, [1, 0]) for i in range(65)])
    cols = [f"c{i:02d}" for i in range(65)]
    for mode in MODES:
        with pytest.raises(UnsupportedOperationException, match=r"65 columns, at most 64"):
            t.withMaskListColumn(mode, cols, cols, "out")  # when the node is built
    assert t.withMaskListColumn(MASK_TRUE, cols[:64], cols[:64], "out").size == 2


def test_bad_arguments(session):
    from capsmi import expr
    from capsmi._lib import IllegalArgumentException
    t = session.table([_col("flag", expr.BOOL, [1, 0]), _col("k", expr.I64, [1, 2], [1, 0])])
    with pytest.raises(IllegalArgumentException, match="'k' is not Boolean"):
        t.withMaskListColumn(MASK_TRUE, ["flag", "k"], ["F", "K"], "out")
    with pytest.raises(IllegalArgumentException, match="no column named 'nope'"):
        t.withMaskListColumn(MASK_NOT_NULL, ["k", "nope"], ["K", "N"], "out")
    with pytest.raises(IllegalArgumentException):
        t.withMaskListColumn(MASK_TRUE, ["flag"], ["F", "G"], "out")
    with pytest.raises(IllegalArgumentException, match="mode"):
        t.withMaskListColumn(2, ["flag"], ["F"], "out")
    assert _check(session, t, MASK_NOT_NULL, ["flag", "k"], ["F", "K"]) == [["F", "K"], ["F"]]


def test_name_of_an_existing_column_replaces_it_in_place(session):
    from capsmi import expr
    t = session.table([_col("a", expr.BOOL, [1, 0, 1]), _col("out", expr.I64, [7, 8, 9]), _col("b", expr.BOOL, [0, 0, 1], [1, 0, 1])])
    out = t.withMaskListColumn(MASK_TRUE, ["a", "b"], ["A", "B"], "out")
    assert out.physicalColumns == ["a", "out", "b"] and _lists(session, out, "out") == [["A"], [], ["A", "B"]]
    # the name of one of the mask's own columns
    own = t.withMaskListColumn(MASK_TRUE, ["a", "b"], ["A", "B"], "b")
    assert own.physicalColumns == ["a", "out", "b"] and own.columnType["b"] == LIST_STR
    assert _lists(session, own, "b") == [["A"], [], ["A", "B"]]
    assert own.select("b").size == 3 and _lists(session, own.select("b"), "b") == [["A"], [], ["A", "B"]]


# ---- views and lazy plans ------------------------------------------------------------------------------
def _flag_table(session, rng, n, k=5):
    passes = rng.random((k, n)) < 0.45
    passes[:, : n // 7] = False
    return _build(session, MASK_TRUE, passes, rng)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_skip_limit_filter_and_join_inputs(session, mode):
    from capsmi import expr
    from capsmi.expr import BinOp, Col, Lit
    rng = np.random.default_rng(31 + mode)
    t, cols = _build(session, mode, rng.random((6, 2500)) < 0.5, rng)
    names = _names(6)
    assert len(_check(session, t.skip(777).limit(1500), mode, cols, names)) == 1500  # a zero-copy row offset
    assert 0 < len(_check(session, t.filter(BinOp("=", BinOp("&", Col("id"), Lit(3)), Lit(1))), mode, cols, names)) < 2500
    left = session.table([_col("k", expr.I64, rng.integers(0, 2600, 4000).astype(np.int64))])
    assert len(_check(session, left.join(t, "inner", ("k", "id")), mode, cols, names)) > 3000  # rows repeat
    assert any(w == [] for w in _check(session, left.join(t, "left_outer", ("k", "id")), mode, cols, names))  # misses: []


def test_union_of_two_tables_that_carry_mask_lists(session):
    from capsmi.expr import Col, Size
    rng = np.random.default_rng(33)
    (a, cols), (b, _) = _flag_table(session, rng, 900), _flag_table(session, rng, 400)
    names = _names(5)
    u = a.withMaskListColumn(MASK_TRUE, cols, names, "l").unionAll(b.withMaskListColumn(MASK_TRUE, cols, names, "l"))
    assert u.size == 1300
    want = ref_mask_list(MASK_TRUE, _exported(u, cols), names)
    assert _lists(session, u, "l") == want  # the second store's lists follow the first's
    sized = u.withColumns((Size(Col("l")), "s"))
    assert sized.column("s").values.tolist() == [len(w) for w in want]


def test_select_of_the_list_alone_prunes_the_flags_above_the_node(session):
    rng = np.random.default_rng(34)
    t, cols = _flag_table(session, rng, 1200)
    names = _names(5)
    want = ref_mask_list(MASK_TRUE, _exported(t, cols), names)
    only = t.withMaskListColumn(MASK_TRUE, cols, names, "l").select("l")
    assert only.physicalColumns == ["l"] and _lists(session, only, "l") == want
    # under a lazy projection that renames and drops around the node
    lazy = t.withColumnRenamed("id", "key").withMaskListColumn(MASK_TRUE, cols, names, "l").drop(*cols)
    assert lazy.physicalColumns == ["key", "l"] and _lists(session, lazy, "l") == want


def test_filter_on_another_column_above_the_node(session):
    from capsmi.expr import BinOp, Col, Lit, Size
    rng = np.random.default_rng(35)
    t, cols = _flag_table(session, rng, 2000)
    names = _names(5)
    want = ref_mask_list(MASK_TRUE, _exported(t, cols), names)
    got = {}
    for fused in (True, False):
        session.set_fused(fused)
        try:
            out = t.withMaskListColumn(MASK_TRUE, cols, names, "l").filter(BinOp("<", Col("id"), Lit(500)))
            got[fused] = (out.column("id").values.tolist(), _lists(session, out, "l"))
            both = t.withMaskListColumn(MASK_TRUE, cols, names, "l").filter(
                BinOp(">", BinOp("+", Size(Col("l")), Col("id")), Lit(1998)))  # reads the new column: stays above
            assert both.column("id").values.tolist() == [r for r in range(2000) if len(want[r]) + r > 1998]
        finally:
            session.set_fused(True)
    assert got[True] == got[False] == (list(range(500)), want[:500])


# ---- composition with the list expressions -------------------------------------------------------------
def test_size_index_in_list_and_explode_of_labels_and_keys(session):
    from capsmi.expr import BinOp, Col, Explode, Index, InList, Keys, Labels, Lit, Size
    rng = np.random.default_rng(36)
    n = 1500
    t, cols = _build(session, MASK_TRUE, rng.random((4, n)) < 0.5, rng)
    t = t.withColumns((BinOp("-", BinOp("&", Col("id"), Lit(7)), Lit(2)), "i"))  # -2 .. 5: both sides out of range
    t.size
    given = ["D", "A", "C", "B"]  # the expression sorts them, and the columns with them
    lab = Labels(tuple(cols), tuple(given))
    want = ref_labels(_exported(t, cols), given)
    assert max(len(w) for w in want) == 4 and [] in want and all(w == sorted(w) for w in want)
    idx = t.column("i").values.tolist()
    out = t.withColumns((Size(lab), "s"), (Index(lab, Col("i")), "e"), (Index(lab, Lit(9)), "e9"), (InList(Lit("A"), lab), "m"),
                        (lab, "l"), (Size(Col("l")), "sl"))
    assert out.physicalColumns == t.physicalColumns + ["s", "e", "e9", "m", "l", "sl"]  # no temporary is left
    rows = out.rows()
    assert [r["s"] for r in rows] == [ref_size(w) for w in want] == [r["sl"] for r in rows]
    assert [r["e"] for r in rows] == [ref_index(w, i) for w, i in zip(want, idx)]
    assert [r["e9"] for r in rows] == [None] * n
    assert [r["m"] for r in rows] == [ref_in_list("A", w, str) for w in want]
    assert [r["l"] for r in rows] == want
    ex = t.withColumns((Explode(lab), "x"))
    assert ex.physicalColumns == t.physicalColumns + ["x"]
    assert [(r["id"], r["x"]) for r in ex.rows()] == [(r, x) for r, w in enumerate(want) for x in w]
    # keys over nullable property columns
    k, kcols = _build(session, MASK_NOT_NULL, rng.random((4, n)) < 0.6, rng)
    kwant = ref_keys(_exported(k, kcols), ["z", "y", "x", "w"])
    kex = k.withColumns((Explode(Keys(tuple(kcols), ("z", "y", "x", "w"))), "key"))
    assert [(r["id"], r["key"]) for r in kex.rows()] == [(r, x) for r, w in enumerate(kwant) for x in w]
    kept = k.filter(InList(Lit("y"), Keys(tuple(kcols), ("z", "y", "x", "w"))))
    assert kept.physicalColumns == k.physicalColumns
    assert kept.column("id").values.tolist() == [r for r, w in enumerate(kwant) if "y" in w]


# ---- routing ---------------------------------------------------------------------------------------------
ROUTES = ("expand", "expand_count", "two_hop", "triangle", "var_length", "miss")
PATTERN = "CREATE (:A {k: 1})-[:T]->(:B:C {k: 2})-[:T]->(:C {k: 3})-[:T]->()"


def _routes(session, items, where=None):
    clause = {"match": "(a)-[r]->(b)"}
    if where is not None:
        clause["where"] = where
    case = {"create": PATTERN, "query": {"clauses": [clause], "return": {"items": items}}}
    before = [session.route_count(n) for n in ROUTES]
    rows = run_planner(session, case)
    delta = [session.route_count(n) - b for n, b in zip(ROUTES, before)]
    print("route deltas", dict(zip(ROUTES, delta)), "for", json.dumps(items))
    return delta, rows


def test_labels_above_an_expand_adds_one_expand_route(session):
    """MATCH (a)-[r]->(b) RETURN labels(b) through the planner adds exactly one to route_count("expand"): the
    pattern's projection on b's id takes the Expand route, b's label flags are joined back by id."""
    delta, rows = _routes(session, [["l", ["labels", "b"]]])
    assert same_rows(rows, [{"l": ["B", "C"]}, {"l": ["C"]}, {"l": []}])
    assert delta == [1, 0, 0, 0, 0, 0]


def test_node_columns_of_both_ends_are_joined_back_to_the_routed_pattern(session):
    """labels() and keys() of both ends, relationship columns beside them, and a node predicate inside the
    pattern: one Expand route each, the rows those of the unfused plan."""
    both = [["la", ["labels", "a"]], ["lb", ["labels", "b"]], ["kb", ["keys", "b"]], ["r", ["id", "r"]]]
    delta, rows = _routes(session, both)
    want = [{"la": ["A"], "lb": ["B", "C"], "kb": ["k"], "r": 2}, {"la": ["B", "C"], "lb": ["C"], "kb": ["k"], "r": 4},
            {"la": ["C"], "lb": [], "kb": [], "r": 6}]
    assert same_rows(rows, want)
    assert delta == [1, 0, 0, 0, 0, 0]
    delta, rows = _routes(session, both, where=[">", ["prop", "a", "k"], ["lit", 1]])
    assert same_rows(rows, want[1:])
    assert delta == [1, 0, 0, 0, 0, 0]
    session.set_fused(False)
    try:
        delta, rows = _routes(session, both)
    finally:
        session.set_fused(True)
    assert same_rows(rows, want) and delta[:5] == [0, 0, 0, 0, 0]
    # every entity function of the pattern's variables in one RETURN
    _, rows = _routes(session, [["l", ["labels", "b"]], ["k", ["keys", "b"]], ["t", ["type", "r"]], ["s", ["startnode", "r"]],
                                ["e", ["endnode", "r"]], ["n", ["size", ["labels", "a"]]]])
    assert same_rows(rows, [{"l": ["B", "C"], "k": ["k"], "t": "T", "s": 0, "e": 1, "n": 1},
                            {"l": ["C"], "k": ["k"], "t": "T", "s": 1, "e": 3, "n": 2},
                            {"l": [], "k": [], "t": "T", "s": 3, "e": 5, "n": 1}])


def test_rel_type_is_the_first_true_flag_or_null(session):
    from capsmi import expr
    from capsmi.expr import RelType
    rng = np.random.default_rng(37)
    n = 500
    flags = rng.random((3, n)) < 0.3
    flags[:, 0] = False  # a row of no TRUE flag
    t = session.table([_col("t0", expr.BOOL, flags[0].astype(np.int64)),
                       _col("t1", expr.BOOL, np.ones(n, dtype=np.int64), flags[1]),  # NULL over a TRUE word
                       _col("t2", expr.BOOL, flags[2].astype(np.int64))])
    cols, names = ["t2", "t0", "t1"], ["ZED", "KNOWS", "A"]  # not sorted: the order given decides
    out = t.withColumns((RelType(tuple(cols), tuple(names)), "ty"))
    assert out.columnType["ty"] == expr.STR
    got = [r["ty"] for r in out.rows()]
    assert got == ref_rel_type(_exported(t, cols), names)
    assert got[0] is None and {"ZED", "KNOWS", "A", None} == set(got)
