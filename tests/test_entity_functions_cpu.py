"""CPU checks of the entity functions (labels(), keys(), type(), startNode(), endNode(), exists()): the
transcription of tests/golden/entity_functions.json (a pure-Python evaluation of every case reproduces its bag),
the planner DSL's new forms, the name sorting and temporary-column lowering of the binding, and the ctypes
declaration of capsmi_with_mask_list_column against the header."""
import os
import re

import pytest

from entity_fn_ref import MASK_NOT_NULL, MASK_TRUE, ref_keys, ref_labels, ref_mask_list, ref_rel_type
from golden_util import load_cases, same_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("entity_functions.json")


def test_golden_file_shape_and_refs():
    assert len(CASES) == 10
    assert [c["name"] for c in CASES] == [
        "exists()", "type()", "labels: get single label", "labels: get multiple labels", "labels: unlabeled nodes",
        "size() on constructed list", "keys()", "keys() does not return keys of unset properties", "startNode()",
        "endNode()"]
    assert [c["ref"] for c in CASES] == [f"FunctionsBehaviour.scala:{r}" for r in (
        "40-52", "57-68", "93-103", "105-115", "117-128", "167-179", "193-204", "206-219", "237-248", "252-263")]
    for c in CASES:
        assert re.fullmatch(r"FunctionsBehaviour\.scala:\d+-\d+", c["ref"]), c["ref"]
        assert c["expected"] and "clauses" in c["query"] and c["cypher"] and c["create"]


# ---- a pure-Python evaluation of every case -----------------------------------------------------------------
def _eval(spec, row, g):
    op = spec[0]
    if op == "lit":
        return spec[1]
    if op == "prop":
        return row[spec[1]]["props"].get(spec[2])
    if op == "=":
        a, b = _eval(spec[1], row, g), _eval(spec[2], row, g)
        return None if a is None or b is None else a == b
    if op == "isnotnull":
        return _eval(spec[1], row, g) is not None
    if op == "type":
        names = sorted({r["type"] for r in g["rels"]})
        return ref_rel_type([[(row[spec[1]]["type"] == t, True)] for t in names], names)[0]
    if op == "startnode":
        return row[spec[1]]["src"]
    if op == "endnode":
        return row[spec[1]]["dst"]
    if op == "labels":  # one flag column per label of the graph, as the scan's header has them
        names = sorted({l for n in g["nodes"] for l in n["labels"]}, reverse=True)  # the restatement sorts
        return ref_labels([[(l in row[spec[1]]["labels"], True)] for l in names], names)[0]
    if op == "keys":  # one property column per key of the graph, null where the node has none
        names = sorted({k for n in g["nodes"] for k in n["props"]}, reverse=True)
        props = row[spec[1]]["props"]
        return ref_keys([[(props.get(k), k in props)] for k in names], names)[0]
    if op == "size":
        lst = _eval(spec[1], row, g)
        return None if lst is None else len(lst)
    raise NotImplementedError(op)


_NODE = r"\((\w*)(?::(\w+))?\)"


def _match(pattern, g):
    m = re.fullmatch(_NODE, pattern)
    if m:
        var, label = m.groups()
        return [{var or "_": n} for n in g["nodes"] if label is None or label in n["labels"]]
    m = re.fullmatch(_NODE + r"-\[(\w+)(?::(\w+))?\]->" + _NODE, pattern)
    a, la, r, ty, b, lb = m.groups()
    assert la is None and lb is None
    by_id = {n["id"]: n for n in g["nodes"]}
    return [{a or "_a": by_id[x["src"]], r: x, b or "_b": by_id[x["dst"]]} for x in g["rels"] if ty is None or x["type"] == ty]


def _run(case):
    from oracle.create_graph import create_graph
    g = create_graph(case["create"])
    (cl,) = case["query"]["clauses"]
    rows = _match(cl["match"], g)
    if "where" in cl:
        rows = [row for row in rows if _eval(cl["where"], row, g) is True]
    return [{alias: _eval(spec, row, g) for alias, spec in case["query"]["return"]["items"]} for row in rows]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pure_python_evaluation_reproduces_the_expected_bag(case):
    assert same_rows(_run(case), case["expected"])


def test_restatement_table():
    t, f, null = (True, True), (False, True), (True, False)  # a TRUE word under validity 0 is a NULL flag
    assert ref_mask_list(MASK_TRUE, [[t, f, null], [f, f, t]], ["x", "y"]) == [["x"], [], ["y"]]
    assert ref_mask_list(MASK_NOT_NULL, [[t, f, null], [(None, False), (0.0, True), ([], True)]], ["x", "y"]) == \
        [["x"], ["x", "y"], ["y"]]
    assert ref_mask_list(MASK_TRUE, [], []) == []
    assert ref_labels([[t], [t]], ["B", "A"]) == [["A", "B"]] and ref_keys([[t], [null]], ["b", "a"]) == [["b"]]
    assert ref_rel_type([[f, t], [t, t]], ["Z", "A"]) == ["A", "Z"]  # the first TRUE flag in the order given
    assert ref_rel_type([[f], [null]], ["Z", "A"]) == [None]


# ---- planner DSL ------------------------------------------------------------------------------------------
def test_planner_builds_the_entity_nodes_from_a_header():
    from capsmi import planner
    from capsmi.expr import Col, Explode, Index, InList, IsNotNull, Keys, Labels, Lit, Size
    h = ["n", "n:B", "n:A", "n.name", "n.age", "r", "r.__src", "r.__dst", "r.__type", "r.w", "nn", "nn:C", "nn.z"]
    lab = planner.to_expr(["labels", "n"], h)
    assert lab == Labels(("n:A", "n:B"), ("A", "B")) and lab.flag_cols == ("n:A", "n:B")
    assert planner.to_expr(["labels", "nn"], h) == Labels(("nn:C",), ("C",))
    assert planner.to_expr(["labels", "r"], h) == Labels((), ())  # no label column: the reference's array()
    keys = planner.to_expr(["keys", "n"], h)
    assert keys == Keys(("n.age", "n.name"), ("age", "name"))
    assert planner.to_expr(["keys", "r"], h) == Keys(("r.w",), ("w",))  # without the r.__* columns
    assert planner.to_expr(["startnode", "r"], h) == Col("r.__src")
    assert planner.to_expr(["endnode", "r"], h) == Col("r.__dst")
    assert planner.to_expr(["type", "r"], h) == Col("r.__type")
    assert planner.to_expr(["isnotnull", ["prop", "n", "age"]], h) == IsNotNull(Col("n.age"))
    # valid wherever _list_operand takes a list
    assert planner.to_expr(["size", ["labels", "n"]], h) == Size(lab)
    assert planner.to_expr(["index", ["keys", "n"], ["lit", 0]], h) == Index(keys, Lit(0))
    assert planner.to_expr(["in_list", ["lit", "A"], ["labels", "n"]], h) == InList(Lit("A"), lab)
    assert Explode(lab) == Explode(planner.to_expr(["labels", "n"], list(reversed(h))))


# ---- the binding: sorting, columns_of, lowering -------------------------------------------------------------
def test_labels_and_keys_sort_by_name_and_rel_type_does_not():
    from capsmi.expr import (Case, Col, Keys, Labels, Lit, RelType, STR, X_CASE, X_COL, X_LIT, X_NULL, columns_of,
                             compile_program, mask_list_args, needs_list_lowering)
    lab = Labels(("f2", "f0", "f1"), ("C", "A", "B"))
    assert (lab.flag_cols, lab.names) == (("f0", "f1", "f2"), ("A", "B", "C"))
    assert mask_list_args(lab) == (MASK_TRUE, ("f0", "f1", "f2"), ("A", "B", "C"))
    keys = Keys(["p.z", "p.a"], ["z", "a"])
    assert mask_list_args(keys) == (MASK_NOT_NULL, ("p.a", "p.z"), ("a", "z"))
    with pytest.raises(ValueError):
        Labels(("f0",), ("A", "B"))
    rt = RelType(("t1", "t0"), ("Z", "A"))
    assert rt.to_case() == Case(((Col("t1"), Lit("Z")), (Col("t0"), Lit("A"))), Lit(None, STR))
    prog = compile_program(rt, {"t0": 0, "t1": 1}.__getitem__, {"A": 10, "Z": 20}.__getitem__)
    assert prog == [(X_COL, 1, 0, 0), (X_LIT, 0, STR, 20), (X_COL, 0, 0, 0), (X_LIT, 0, STR, 10), (X_NULL, STR + 1, 0, 0),
                    (X_CASE, 2, 0, 0)]
    assert columns_of(lab) == {"f0", "f1", "f2"} and columns_of(keys) == {"p.a", "p.z"} and columns_of(rt) == {"t0", "t1"}
    assert needs_list_lowering(lab) and needs_list_lowering(keys) and not needs_list_lowering(rt)


class _FakeTable:
    """The part of GpuTable that _lower_lists reads."""
    columnType = {"xs": 8, "s": 3, "a": 0}


def _lower(e):
    from capsmi.table import GpuTable
    return GpuTable._lower_lists(_FakeTable(), e)


def test_temporary_column_lowering():
    from capsmi import _lib
    from capsmi.expr import BinOp, Col, Explode, Index, InList, Keys, Labels, Lit, Not, Range, Size
    lab, keys = Labels(("f",), ("A",)), Keys(("p",), ("k",))
    for src in (lab, keys):
        for wrap in (Size, lambda x: Index(x, Lit(0)), lambda x: InList(Col("a"), x), Explode):
            e, temps = _lower(wrap(src))
            assert len(temps) == 1 and temps[0][1] == src
            assert wrap(Col(temps[0][0])) == e
        assert _lower(src) == (src, [])  # the whole column stays
        with pytest.raises(_lib.NotImplementedException, match=type(src).__name__):  # misplaced
            _lower(BinOp("=", src, Lit(1)))
        with pytest.raises(_lib.NotImplementedException, match=type(src).__name__):
            _lower(Not(src))
    # two sources in one expression get two temporaries; a Range still gets its own
    e, temps = _lower(BinOp("+", Size(lab), BinOp("+", Size(keys), Size(Range(Lit(1), Col("a"))))))
    assert [t[1] for t in temps] == [lab, keys, Range(Lit(1), Col("a"))] and len({t[0] for t in temps}) == 3
    with pytest.raises(_lib.NotImplementedException, match="nested"):  # a list source inside a Range operand
        _lower(Size(Range(Lit(1), Size(Range(Lit(1), Lit(2))))))


def test_with_columns_dispatches_list_sources_to_their_nodes():
    """_with_list_columns on a recording stub: a whole column and a temporary both reach withMaskListColumn with
    the sorted names, and the temporary is dropped."""
    from capsmi.expr import Col, Keys, Labels, Size
    from capsmi.table import GpuTable

    class Rec:
        columnType = {}
        calls = []
        _lower_lists = GpuTable._lower_lists
        _with_list_source = GpuTable._with_list_source

        def withMaskListColumn(self, mode, cols, names, name):
            self.calls.append(("mask", mode, tuple(cols), tuple(names), name))
            return self

        def _with_columns(self, cols):
            self.calls.append(("cols", tuple(cols)))
            return self

        def drop(self, *names):
            self.calls.append(("drop", names))
            return self

    r = Rec()
    GpuTable._with_list_columns(r, [(Labels(("n:B", "n:A"), ("B", "A")), "l"), (Size(Keys(("n.y", "n.x"), ("y", "x"))), "s")])
    assert r.calls[0] == ("mask", MASK_TRUE, ("n:A", "n:B"), ("A", "B"), "l")
    kind, mode, cols, names, tmp = r.calls[1]
    assert (kind, mode, cols, names) == ("mask", MASK_NOT_NULL, ("n.x", "n.y"), ("x", "y"))
    assert r.calls[2] == ("cols", ((Size(Col(tmp)), "s"),)) and r.calls[3] == ("drop", (tmp,))


# ---- the binding against the header -----------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "capsmi.h")).read()


def test_header_declares_the_entry_point_and_both_modes():
    from capsmi import expr
    text = _header()
    assert "capsmi_status capsmi_with_mask_list_column(" in text
    for name, want in (("TRUE", 0), ("NOT_NULL", 1)):
        (v,) = re.findall(rf"CAPSMI_MASK_{name} = (\d+)", text)
        assert int(v) == want == getattr(expr, f"MASK_{name}")
    assert "CAPSFunctions.scala:73-91" in text and "not an observation of a run" in " ".join(text.split())


def test_ctypes_declares_the_mask_list_entry_point():
    import ctypes
    from capsmi import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    (args,) = re.findall(r"^capsmi_status\s+capsmi_with_mask_list_column\s*\((.*?)\)\s*;", text, re.S | re.M)
    res, sig = _lib._SIGS["capsmi_with_mask_list_column"]
    assert len(sig) == " ".join(args.split()).count(",") + 1 == 7
    assert res is ctypes.c_int32 and sig[1] is ctypes.c_int32 and sig[2] is ctypes.c_int32
    assert sig[4] is ctypes.POINTER(ctypes.c_int64) and sig[5] is ctypes.c_char_p
    assert hasattr(_lib.load(), "capsmi_with_mask_list_column")
