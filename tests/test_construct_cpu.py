"""CPU checks of MonotonicallyIncreasingId (CAPSMI_X_ROW_ID) and of CONSTRUCT in the planner mirror: the opcode against
the header and the JVM shim, compile_program / columns_of, check_program over tests/golden/row_id_programs.json in a
stand-alone ASan + UBSan program (tests/sanitize/expr_san.cpp, unchanged), generateId's offsets, the tag strategies the
reference's tests pin, the pure-Python restatement (construct_ref.py) over tests/golden/construct.json, and the
validation of construct specs.  No GPU."""
import json
import os
import re

import pytest

import construct_ref as cr
from capsmi import construct, expr, tagging
from capsmi.expr import MonotonicallyIncreasingId
from golden_util import load_cases
from test_sanitizers import ASAN, SAN, _build, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("construct.json")


# ---- the opcode against the header and the front ends ---------------------------------------------------
def test_opcode_value_matches_the_header_and_the_jvm_shim():
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    (v,) = re.findall(r"CAPSMI_X_ROW_ID = (\d+)", text)
    assert int(v) == 68 == expr.X_ROW_ID
    assert not re.search(r"CAPSMI_X_[A-Z0-9_]+ = 6[67]\b", text)  # 66..67 stay unassigned
    block = re.sub(r"\s+", " ", text[text.index("66..67"):text.index("CAPSMI_X_ROW_ID = 68")])
    for words in ("SparkSQLExprMapper.scala:189", "Legal only in a program of capsmi_with_columns", "is pinned",
                  "no filter conjunct is pushed below it", "computed whole", "keeps its rows", "never matched as part of a fused",
                  "distributed CONSTRUCT is not implemented"):
        assert words in block, words
    scala = os.path.join(ROOT, "jvm", "src", "main", "scala", "org", "opencypher", "capsmi")
    assert re.search(r"final val X_ROW_ID = 68\b", open(os.path.join(scala, "CapsmiLib.scala")).read())
    assert re.search(r"case _: MonotonicallyIncreasingId => out \+= \(\(Capsmi\.X_ROW_ID, 0, 0, 0L\)\)",
                     open(os.path.join(scala, "GpuTable.scala")).read())


def test_compile_program_and_columns_of():
    from capsmi.expr import BinOp, Col, Lit, X_ADD, X_COL, X_LIT, X_ROW_ID, columns_of, compile_program
    idx = {"x": 0, "y": 1}.__getitem__
    rid = MonotonicallyIncreasingId()
    assert compile_program(rid, idx, None) == [(X_ROW_ID, 0, 0, 0)]
    assert compile_program(BinOp("+", rid, Col("y")), idx, None) == [(X_ROW_ID, 0, 0, 0), (X_COL, 1, 0, 0), (X_ADD, 0, 0, 0)]
    tagged = compile_program(tagging.expr_set_tag(BinOp("+", rid, Lit(1 << 32)), 3), idx, None)
    assert [n[0] for n in tagged] == [X_ROW_ID, X_LIT, X_ADD, X_LIT, expr.X_BITAND, X_LIT, X_LIT, expr.X_SHL, expr.X_BITOR]
    assert columns_of(rid) == set() and columns_of(BinOp("+", rid, Col("y"))) == {"y"}
    assert rid == MonotonicallyIncreasingId() and hash(rid) == hash(MonotonicallyIncreasingId()) and rid != Lit(0)
    assert "SparkSQLExprMapper.scala:189" in MonotonicallyIncreasingId.__doc__
    assert not expr.needs_list_lowering(rid) and not expr.contains_explode(rid) and not expr.is_string_typed(rid)


def test_row_id_programs_under_asan_ubsan(tmp_path):
    """Accepted: alone and under ADD / BITOR / SHL / DIV / EQ / CASE / the set_tag shape / TO_STRING, typed I64 (BOOL under
    EQ, STR under TO_STRING, F64 added to a Double).  Refused with ILLEGAL_ARGUMENT: as the operand of an opcode that
    demands a String, and a non-zero arg.  66, 67 and 69 stay unknown."""
    fixture = os.path.join(ROOT, "tests", "golden", "row_id_programs.json")
    with open(fixture) as f:
        records = json.load(f)["records"]
    by_why = {r["why"]: r for r in records}
    assert len(by_why) == len(records)
    accepted = [r for r in records if r["status"] == 0]
    for why, ty in (("ROW_ID", 0), ("ADD(ROW_ID,litI64)", 0), ("ADD(ROW_ID,F64)", 2), ("BITOR(ROW_ID,I64)", 0),
                    ("SHL(ROW_ID,litI64)", 0), ("DIV(ROW_ID,litI64)", 0), ("EQ(ROW_ID,I64)", 1),
                    ("CASE(EQ(ROW_ID,lit),ROW_ID,lit)", 0), ("set_tag(ADD(ROW_ID,offset),tag)", 0), ("TO_STRING(ROW_ID)", 3)):
        assert (by_why[why]["status"], by_why[why]["type"]) == (0, ty), why
        assert any(n[0] == 68 for n in by_why[why]["prog"]), why
    for why in ("STARTS_WITH(ROW_ID,litSTR)", "CONTAINS(STR,ROW_ID)", "STR_SIZE(ROW_ID)"):
        assert by_why[why]["status"] == 1 and "String" in by_why[why]["message"], why
    for why in ("ROW_ID with arg 1", "ROW_ID with arg -1 under ADD"):
        assert by_why[why]["status"] == 1 and "CAPSMI_X_ROW_ID takes no argument" in by_why[why]["message"], why
    for op in (66, 67, 69):
        r = by_why[f"op {op} is unknown"]
        assert r["status"] == 2 and r["message"] == f"unknown expression op {op}"
    exe = str(tmp_path / "expr_san")
    _build(["g++", *ASAN, "-std=c++17", os.path.join(SAN, "expr_san.cpp"), "-o", exe], tmp_path)
    out = _run(exe, fixture)
    assert f"{len(records)} records, {len(accepted)} accepted" in out, out
    assert "\n0 mixed refused" in out and "\n0 mismatches" in out, out


# ---- generateId and the tag strategies --------------------------------------------------------------------
@pytest.mark.parametrize("k,n,want", [(0, 1, 0), (1, 2, 1 << 32), (2, 3, 2 << 31), (7, 8, 7 << 30)])
def test_generate_id_offsets(k, n, want):
    """ConstructGraphPlanner.generateId: k << (33 - (floor(ln n) + 1)), the natural log being the reference's own."""
    assert construct.id_offset(k, n) == want == cr.id_offset(k, n)
    from capsmi.expr import BinOp, Lit
    assert construct.generate_id(k, n) == BinOp("+", MonotonicallyIncreasingId(), Lit(want))


def test_tag_strategies_of_the_pinned_cases():
    # ON graphs first, their retaggings fixed; match graphs after them
    assert construct.tag_strategy([("one", {0})], [("one", {0})]) == ({"one": {0: 0}}, {"one": {0: 0}})
    on, strat = construct.tag_strategy([("one", {0}), ("two", {0})], [])
    assert on == {"one": {0: 0}, "two": {0: 1}} == strat
    assert tagging.pick_free_tag({t for m in strat.values() for t in m.values()}) == 2
    on, strat = construct.tag_strategy([], [("g", {0})])
    assert on == {} and strat == {"g": {0: 0}}
    on, strat = construct.tag_strategy([], [("g", {0}), ("h", {0})])
    assert strat == {"g": {0: 0}, "h": {0: 1}}
    on, strat = construct.tag_strategy([("one", {0})], [("m", {0, 1})])
    assert strat == {"one": {0: 0}, "m": {0: 2, 1: 1}}
    assert construct.tag_strategy([("a", {0})], [("a", {0})]) == cr.tag_strategy([("a", {0})], [("a", {0})])


# ---- the restatement over the golden cases ----------------------------------------------------------------
def test_golden_file_shape():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) >= 12
    for c in CASES:
        assert c["ref"].startswith("MultipleGraphBehaviour.scala:") and c["cypher"].strip(), c["name"]
        assert c["query"]["return"] == "graph" or c["query"]["return"]["items"], c["name"]
    assert sum(1 for c in CASES if "construct" in json.dumps(c["query"])) >= 40


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_reproduces_the_expected_graph(case):
    got = cr.run_case(case)
    cr.assert_graph(got, case["expected"])


# ---- spec validation ---------------------------------------------------------------------------------------
def _validate(spec, node_vars=("a", "b"), rel_vars=("r",)):
    return construct.validate(spec, set(node_vars), set(rel_vars))


def test_spec_validation():
    from capsmi.planner import PlanningError
    ok = {"on": [], "clones": [["a", "a"], ["x", "b"]],
          "creates": [{"node": "n", "labels": ["L"]}, {"rel": "e", "src": "a", "dst": "n", "type": "T"},
                      {"rel": "f", "src": "x", "dst": "a", "copy_of": "r"}],
          "sets": [["prop", "n", "k", ["lit", 1]], ["label", "a", ["M"]]]}
    _validate(ok)
    bad = [
        (dict(ok, clones=[["a", "zz"]]), "unknown clone original"),
        (dict(ok, creates=[{"rel": "e", "src": "a", "dst": "b", "type": "T"}]), "neither cloned nor created"),
        (dict(ok, creates=[{"node": "n", "labels": [], "copy_of": "gone"}]), "copy_of"),
        (dict(ok, creates=[{"rel": "e", "src": "a", "dst": "x"}]), "type"),
        (dict(ok, sets=[["prop", "b", "k", ["lit", 1]]]), "dropped variable"),
        (dict(ok, sets=[["label", "e", ["M"]]]), "label on"),
    ]
    for spec, words in bad:
        with pytest.raises(PlanningError, match=words):
            _validate(spec)
