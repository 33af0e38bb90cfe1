"""CPU checks of the list expressions (size(), list[i], IN over a list column, range()): the transcription of
tests/golden/list_expr.json (a pure-Python evaluation of the literal-sourced cases reproduces their bags), the
opcodes and operand order of compile_program against the header, the ctypes declaration of
capsmi_with_range_column, the planner DSL, the binding's rewrites, and the range restatement the GPU tests use."""
import os
import re

import pytest

from golden_util import load_cases, same_rows
from list_expr_ref import T, ref_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("list_expr.json")


def test_golden_file_shape_and_refs():
    assert len(CASES) == 10
    assert [c["name"] for c in CASES if c.get("upstream_ignored")] == ["size() on null"]
    assert [c["name"] for c in CASES if c.get("project_case")] == ["IN over a collected list"]
    refs = [c["ref"] for c in CASES if not c.get("project_case")]
    assert sum(r.startswith("ExpressionBehaviour.scala:") for r in refs) == 3  # ContainerIndex
    assert sum(r.startswith("FunctionsBehaviour.scala:") for r in refs) == 6   # four range, two size
    for r in refs:
        assert re.fullmatch(r"(Expression|Functions)Behaviour\.scala:\d+-\d+", r), r
    for c in CASES:
        assert c["expected"] and "clauses" in c["query"] and c["cypher"]


# ---- a pure-Python evaluation of the cases whose lists are literals, properties or ranges ---------------
def _eval(spec, row):
    op = spec[0]
    if op == "var":
        return row[spec[1]]
    if op == "lit":
        return spec[1]
    if op == "prop":
        return row[spec[1]]["props"].get(spec[2])
    if op == "listlit":
        return list(spec[1])
    if op == "range":
        opd = [_eval(s, row) if isinstance(s, list) else s for s in spec[1:]]
        return None if any(x is None for x in opd) else ref_range(*opd)
    if op == "size":
        lst = _eval(spec[1], row)
        return None if lst is None else len(lst)
    if op == "index":
        lst, i = _eval(spec[1], row), _eval(spec[2], row)
        return None if lst is None or i is None or not 0 <= i < len(lst) else lst[i]
    raise NotImplementedError(op)


def _literal_sourced(case):
    return not case.get("project_case")


def _run(case):
    from oracle.create_graph import create_graph
    g = create_graph(case["create"])
    rows = [{}]
    for cl in case["query"]["clauses"]:
        if "match" in cl:
            (var,) = re.fullmatch(r"\((\w*)\)", cl["match"]).groups()
            rows = [dict(row, **{var or "_": n}) for row in rows for n in g["nodes"]]
        else:
            rows = [dict(row, **{cl["as"]: x}) for row in rows for x in _eval(cl["unwind"], row)]
    return [{alias: _eval(spec, row) for alias, spec in case["query"]["return"]["items"]} for row in rows]


@pytest.mark.parametrize("case", [c for c in CASES if _literal_sourced(c)],
                         ids=[c["name"] for c in CASES if _literal_sourced(c)])
def test_pure_python_evaluation_reproduces_the_expected_bag(case):
    assert same_rows(_run(case), case["expected"])


def test_the_project_case_by_hand():
    """The bag the file's `about` derives: collect per start node, then membership over all five nodes."""
    from oracle.create_graph import create_graph
    case = next(c for c in CASES if c.get("project_case"))
    g = create_graph(case["create"])
    val = {n["id"]: n["props"]["val"] for n in g["nodes"]}
    assert len(val) == 5
    vs = {}
    for r in g["rels"]:
        vs.setdefault(r["src"], []).append(val[r["dst"]])
    rows = [{"a.val": val[a], "c.val": val[c]} for a, lst in vs.items() for c in val if val[c] in lst]
    assert same_rows(rows, case["expected"]) and len(rows) == 5


# ---- the binding against the header ---------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "capsmi.h")).read()


def test_opcode_values_match_the_header():
    from capsmi import expr
    text = _header()
    for name, want in (("SIZE", 26), ("INDEX", 27), ("IN_LIST", 28)):
        (v,) = re.findall(rf"CAPSMI_X_{name} = (\d+)", text)
        assert int(v) == want == getattr(expr, f"X_{name}")


def test_compile_program_operand_order():
    from capsmi.expr import (BinOp, Col, Index, InList, Lit, Size, X_COL, X_IN_LIST, X_INDEX, X_LIT, X_MUL, X_SIZE,
                             columns_of, compile_program)
    idx = {"a": 0, "xs": 1, "i": 2}.__getitem__
    assert compile_program(Size(Col("xs")), idx, None) == [(X_COL, 1, 0, 0), (X_SIZE, 0, 0, 0)]
    # [list, i]
    assert compile_program(Index(Col("xs"), Col("i")), idx, None) == [(X_COL, 1, 0, 0), (X_COL, 2, 0, 0), (X_INDEX, 0, 0, 0)]
    # [x, list]
    prog = compile_program(InList(BinOp("*", Col("a"), Lit(2)), Col("xs")), idx, None)
    assert [p[0] for p in prog] == [X_COL, X_LIT, X_MUL, X_COL, X_IN_LIST]
    assert prog[0][1] == 0 and prog[3][1] == 1
    assert (X_SIZE, X_INDEX, X_IN_LIST) == (26, 27, 28)
    from capsmi.expr import Range
    assert columns_of(InList(Col("a"), Col("xs"))) == {"a", "xs"}
    assert columns_of(Size(Range(Col("a"), BinOp("+", Col("i"), Lit(1)), Col("xs")))) == {"a", "i", "xs"}
    assert columns_of(Index(Col("xs"), Col("i"))) == {"xs", "i"}


def test_ctypes_declares_the_range_entry_point():
    from capsmi import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    (args,) = re.findall(r"^capsmi_status\s+capsmi_with_range_column\s*\((.*?)\)\s*;", text, re.S | re.M)
    res, sig = _lib._SIGS["capsmi_with_range_column"]
    assert len(sig) == " ".join(args.split()).count(",") + 1
    assert hasattr(_lib.load(), "capsmi_with_range_column")


def test_tile_constant_matches_the_kernel():
    text = open(os.path.join(ROOT, "cypher-for-apache-spark_amd", "csrc", "capsmi_impl.h")).read()
    (tile,) = re.findall(r"constexpr int kExplodeTile = (\d+);", text)
    assert int(tile) == T


# ---- planner DSL and the binding's rewrites -------------------------------------------------------------
def test_planner_parses_the_new_forms():
    from capsmi import planner
    from capsmi.expr import BinOp, Col, Index, InList, ListLit, Lit, Range, Size
    h = ["n", "n.xs", "n.k", "i"]
    assert planner.to_expr(["size", ["prop", "n", "xs"]], h) == Size(Col("n.xs"))
    assert planner.to_expr(["size", ["listlit", ["a", "b"]]], h) == Size(ListLit(("a", "b")))
    assert planner.to_expr(["index", ["prop", "n", "xs"], ["var", "i"]], h) == Index(Col("n.xs"), Col("i"))
    assert planner.to_expr(["index", ["listlit", [4, 5]], ["lit", 1]], h) == Index(ListLit((4, 5)), Lit(1))
    assert planner.to_expr(["in_list", ["prop", "n", "k"], ["prop", "n", "xs"]], h) == InList(Col("n.k"), Col("n.xs"))
    assert planner.to_expr(["in_list", ["var", "i"], ["listlit", [1, 2]]], h) == InList(Col("i"), ListLit((1, 2)))
    assert planner.to_expr(["range", 1, 3], h) == Range(Lit(1), Lit(3), None)
    assert planner.to_expr(["range", ["prop", "n", "k"], ["+", ["var", "i"], ["lit", 1]], -2], h) == \
        Range(Col("n.k"), BinOp("+", Col("i"), Lit(1)), Lit(-2))
    assert planner.to_expr(["size", ["range", 1, ["var", "i"]]], h) == Size(Range(Lit(1), Col("i"), None))
    with pytest.raises(planner.PlanningError):
        planner.to_expr(["range", 1], h)


class _FakeTable:
    """The part of GpuTable that _lower_lists reads."""
    columnType = {"xs": 8, "s": 3, "a": 0}


def _lower(e):
    from capsmi.table import GpuTable
    return GpuTable._lower_lists(_FakeTable(), e)


def test_in_rewrite_and_size_fold():
    from capsmi import _lib
    from capsmi.expr import Case, Col, Explode, In, Index, InList, ListLit, Lit, Not, Param, Range, Size
    assert _lower(InList(Col("a"), ListLit((1, 2)))) == (In(Col("a"), (Lit(1), Lit(2))), [])
    assert _lower(Not(InList(Col("a"), Param(0)))) == (Not(In(Col("a"), (Param(0),))), [])
    assert _lower(Size(ListLit(("x", "y", "z")))) == (Lit(3), [])
    assert _lower(InList(Col("a"), Col("xs"))) == (InList(Col("a"), Col("xs")), [])
    e, temps = _lower(Index(ListLit((7, 8)), Col("a")))
    assert isinstance(e, Case) and len(e.alternatives) == 2 and temps == []
    with pytest.raises(_lib.NotImplementedException, match="string"):
        _lower(Size(Col("s")))
    with pytest.raises(_lib.NotImplementedException, match="string"):
        _lower(Size(Lit("Alice")))
    # a Range below Size / Index / InList / Explode becomes a temporary column
    for wrap in (Size, lambda r: Index(r, Lit(0)), lambda r: InList(Col("a"), r), Explode):
        e, temps = _lower(wrap(Range(Lit(1), Col("a"))))
        assert len(temps) == 1 and temps[0][1] == Range(Lit(1), Col("a"))
    e, temps = _lower(Range(Lit(1), Col("a")))  # the whole column stays
    assert e == Range(Lit(1), Col("a")) and temps == []
    from capsmi.expr import BinOp
    with pytest.raises(_lib.NotImplementedException):
        _lower(BinOp("=", Range(Lit(1), Lit(2)), Lit(1)))


# ---- the range restatement ------------------------------------------------------------------------------
def test_range_restatement_table():
    assert ref_range(1, 3) == [1, 2, 3]
    assert ref_range(1, 7, 3) == [1, 4, 7]
    assert ref_range(1, 4, 2) == [1, 3]
    assert ref_range(1, 4, 3) == [1, 4]
    assert ref_range(3, 1) == []
    assert ref_range(3, 1, -1) == [3, 2, 1]
    big = ref_range(-2 ** 63, 2 ** 63 - 1, 2 ** 62)
    assert len(big) == 4 and big == [-2 ** 63, -2 ** 62, 0, 2 ** 62]
    assert ref_range(2 ** 63 - 3, 2 ** 63 - 1) == [2 ** 63 - 3, 2 ** 63 - 2, 2 ** 63 - 1]
    with pytest.raises(ValueError):
        ref_range(1, 2, 0)
