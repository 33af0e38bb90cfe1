"""CPU checks of toString() and string concatenation (CAPSMI_X_TO_STRING, CAPSMI_X_CONCAT): the restatement of
str_make_ref.py over the transcription of tests/golden/string_make.json, the opcodes of compile_program against the
header, the planner DSL, StringDictionary.intern_batch (what the session's string sink runs), csrc/str_make.h under
ASan + UBSan in a stand-alone program (tests/sanitize/strmake_san.cpp over tests/golden/str_make_cases.json), and
check_program over tests/golden/string_make_programs.json (tests/sanitize/expr_san.cpp, unchanged).  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import str_make_ref as mr
from golden_util import load_cases, same_rows
from test_sanitizers import ASAN, SAN, _build, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("string_make.json")
EDGES = load_cases("str_make_cases.json")
OPCODES = {"TO_STRING": 64, "CONCAT": 65}


# ---- the restatement -------------------------------------------------------------------------------------
def test_restatement_at_the_edges_the_header_names():
    assert mr.to_string(mr.LONG_MIN) == "-9223372036854775808" and len(mr.to_string(mr.LONG_MIN)) == 20
    assert [mr.to_string(v) for v in (0, -1, 7, 10, -100, mr.LONG_MAX)] == ["0", "-1", "7", "10", "-100", "9223372036854775807"]
    assert [mr.to_string(v) for v in (True, False, "x", "", None)] == ["true", "false", "x", "", None]
    assert mr.concat("Hello", 42) == "Hello42" and mr.concat(42, "Hello") == "42Hello" and mr.concat("", "") == ""
    assert mr.concat("a", "bc") == mr.concat("ab", "c") == "abc"
    assert mr.concat(None, "x") is None and mr.concat("x", None) is None and mr.concat(None, 1) is None
    assert mr.concat("é", -5).encode() == b"\xc3\xa9-5"
    for bad in (lambda: mr.to_string(1.0), lambda: mr.concat("a", 1.5), lambda: mr.concat(2.0, "a")):
        with pytest.raises(NotImplementedError):
            bad()
    for bad in (lambda: mr.concat(True, "a"), lambda: mr.concat(1, 2)):
        with pytest.raises(ValueError):
            bad()


def test_the_edge_fixture_is_what_the_restatement_gives():
    longs = [c for c in EDGES if c["kind"] == "long"]
    assert [int(c["value"]) for c in longs] == mr.edge_longs() and len(longs) == 59
    assert {0, 1, -1, 9, 10, 99, 100, 10 ** 18, -10 ** 18, 10 ** 18 - 1, mr.LONG_MAX, mr.LONG_MIN} <= set(mr.edge_longs())
    for c in longs:
        assert c["text"] == mr.to_string(int(c["value"])) and 1 <= len(c["text"]) <= 20, c
    assert [(c["value"], c["text"]) for c in EDGES if c["kind"] == "bool"] == [("true", "true"), ("false", "false")]
    assert {len(c["text"]) for c in longs} == set(range(1, 21))  # every length the lengths pass can give


# ---- the golden file -------------------------------------------------------------------------------------
def test_golden_file_shape_and_refs():
    assert len(CASES) == 9
    assert sum(1 for c in CASES if c["ref"].startswith("FunctionsBehaviour")) == 5
    assert sum(1 for c in CASES if c["ref"].startswith("ExpressionBehaviour")) == 4
    for c in CASES:
        assert re.fullmatch(r"(Functions|Expression)Behaviour\.scala:\d+-\d+", c["ref"]), c["ref"]
        assert c["expected"] and len(c["query"]["clauses"]) == 1 and c["cypher"]
    refused = [c for c in CASES if c["expected"] == "NotImplemented"]
    assert len(refused) == 2 and all("float" in c["name"] and c["reference_expected"] for c in refused)
    assert {i[1][0] for c in CASES for i in c["query"]["return"]["items"]} == {"tostring", "concat"}


def _eval(spec, binding):
    if spec[0] == "lit":
        return spec[1]
    if spec[0] == "prop":
        return binding[spec[1]]["props"].get(spec[2])
    return mr.FUNCS[spec[0]](*[_eval(s, binding) for s in spec[1:]])


def _bindings(case):
    from oracle.create_graph import create_graph
    nodes = create_graph(case["create"])["nodes"]
    pats = re.findall(r"\((\w*)(?::(\w+))?\)", case["query"]["clauses"][0]["match"])
    out = [{}]
    for var, label in pats:  # the patterns of these cases are node patterns joined by a cross product
        out = [dict(b, **{var or "_": n}) for b in out for n in nodes if not label or label in n["labels"]]
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pure_python_evaluation_reproduces_the_expected_bag(case):
    items = case["query"]["return"]["items"]
    if case["expected"] == "NotImplemented":
        with pytest.raises(NotImplementedError):
            [{alias: _eval(spec, b) for alias, spec in items} for b in _bindings(case)]
        return
    got = [{alias: _eval(spec, b) for alias, spec in items} for b in _bindings(case)]
    assert same_rows(got, case["expected"]), got


# ---- the binding against the header ----------------------------------------------------------------------
def test_opcode_values_match_the_header():
    from capsmi import expr
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    for name, want in OPCODES.items():
        (v,) = re.findall(rf"CAPSMI_X_{name} = (\d+)", text)
        assert int(v) == want == getattr(expr, f"X_{name}"), name
    assert not re.search(r"CAPSMI_X_[A-Z0-9_]+ = 6[0-3]\b", text)  # 60..63 stay unassigned
    assert expr.STRING_MAKE_OPS == (64, 65)
    assert expr.STRING_SYNC_OPS == expr.STRING_STORE_OPS + expr.STRING_MAKE_OPS
    tail = re.sub(r"\s+", " ", text[text.index("60..63"):])
    assert "stated from knowledge of Spark's source, not from a run" in tail and "Double.toString" in tail
    assert "capsmi_string_sink_fn" in text and "capsmi_session_string_count" in text
    from capsmi import _lib
    assert {"capsmi_session_set_string_sink", "capsmi_session_string_count"} <= set(_lib.EXPORTED)


def test_compile_program_and_columns_of():
    from capsmi import expr
    from capsmi.expr import (BinOp, Coalesce, Col, Concat, Lit, STR, ToString, X_ADD, X_COL, X_CONCAT, X_LIT, X_NULL, X_TO_STRING,
                             columns_of, compile_program)
    idx = {"x": 0, "y": 1}.__getitem__
    assert compile_program(ToString(Col("y")), idx, None) == [(X_COL, 1, 0, 0), (X_TO_STRING, 0, 0, 0)]
    assert compile_program(ToString(Lit(5)), idx, None) == [(X_LIT, 0, expr.I64, 5), (X_TO_STRING, 0, 0, 0)]
    assert compile_program(ToString(Lit(None, STR)), idx, None) == [(X_NULL, STR + 1, 0, 0), (X_TO_STRING, 0, 0, 0)]
    assert compile_program(Concat(Col("x"), Col("y")), idx, None) == [(X_COL, 0, 0, 0), (X_COL, 1, 0, 0), (X_CONCAT, 0, 0, 0)]
    assert compile_program(Concat(Lit("a"), Lit(7)), idx, lambda s: 77) == \
        [(X_LIT, 0, STR, 77), (X_LIT, 0, expr.I64, 7), (X_CONCAT, 0, 0, 0)]
    # Add: the concatenation when the tree types an operand as String, else the addition it was
    assert compile_program(BinOp("+", Col("x"), Lit("a")), idx, lambda s: 77)[-1] == (X_CONCAT, 0, 0, 0)
    assert compile_program(BinOp("+", Lit("a"), Col("x")), idx, lambda s: 77)[-1] == (X_CONCAT, 0, 0, 0)
    assert compile_program(BinOp("+", ToString(Col("x")), Col("y")), idx, None)[-1] == (X_CONCAT, 0, 0, 0)
    assert [n[0] for n in compile_program(BinOp("+", BinOp("+", Col("x"), Lit("-")), Col("y")), idx, lambda s: 77)] == \
        [X_COL, X_LIT, X_CONCAT, X_COL, X_CONCAT]
    assert compile_program(BinOp("+", Col("x"), Col("y")), idx, None)[-1] == (X_ADD, 0, 0, 0)
    assert compile_program(BinOp("+", Col("x"), Lit(1)), idx, None)[-1] == (X_ADD, 0, 0, 0)
    assert compile_program(BinOp("-", Col("x"), Lit("a")), idx, lambda s: 77)[-1] == (expr.X_SUB, 0, 0, 0)
    for cls in (ToString, Concat):
        assert "SparkSQLExprMapper.scala" in cls.__doc__
    assert columns_of(Concat(ToString(Col("x")), Coalesce((Col("y"), Lit("z"))))) == {"x", "y"}
    assert ToString(Col("x")) == ToString(Col("x")) != ToString(Col("y"))
    assert Concat(Col("x"), Col("y")) != Concat(Col("y"), Col("x"))


def test_planner_parses_the_new_words():
    from capsmi import planner
    from capsmi.expr import BinOp, Col, Concat, Lit, ToString
    h = ["n", "n.val", "n.name"]
    x, s = ["prop", "n", "val"], ["prop", "n", "name"]
    assert planner.to_expr(["tostring", x], h) == ToString(Col("n.val"))
    assert planner.to_expr(["tostring", ["prop", "n", "gone"]], h) == ToString(Lit(None))
    assert planner.to_expr(["concat", s, x], h) == Concat(Col("n.name"), Col("n.val"))
    assert planner.to_expr(["concat", ["concat", s, ["lit", "-"]], x], h) == Concat(Concat(Col("n.name"), Lit("-")), Col("n.val"))
    assert planner.to_expr(["+", x, ["lit", 1]], h) == BinOp("+", Col("n.val"), Lit(1))  # the addition is what it was


# ---- the dictionary side of the sink -----------------------------------------------------------------------
def _batch(strings):
    enc = [x if isinstance(x, bytes) else x.encode("utf-8") for x in strings]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in enc], out=off[1:])
    return off, b"".join(enc)


def test_intern_batch():
    from capsmi.table import StringDictionary
    d = StringDictionary(["b", "d", "f"])
    known = {x: d.encode(x) for x in ("b", "d", "f")}
    g0 = d.growth
    batch = ["d", "a", "c", "a", "zz", "", "d", b"\xffx", "c"]  # known and new, duplicates, the empty string, no UTF-8
    codes = d.intern_batch(*_batch(batch))
    assert codes.dtype == np.int64 and len(codes) == len(batch)
    assert d.growth == g0 + 1  # one extend for the batch
    assert codes[0] == codes[6] == known["d"] and codes[1] == codes[3] and codes[2] == codes[8]
    assert len(set(codes.tolist())) == 6 and len(d) == 3 + 5
    assert {x: d.encode(x) for x in known} == known  # codes are stable
    assert d.decode(int(codes[7])) == b"\xffx".decode("utf-8", "surrogateescape")
    assert d.decode(int(codes[5])) == "" and d.decode(int(codes[4])) == "zz"
    # code order is string order afterwards, and arrays() gives the bytes back
    cs, off, data = d.arrays()
    strs = [data[off[i]:off[i + 1]].decode("utf-8", "surrogateescape") for i in range(len(cs))]
    assert strs == sorted(strs) and (np.diff(cs) > 0).all() and b"\xffx" in data
    # a batch of known strings moves nothing
    again = d.intern_batch(*_batch(batch))
    assert again.tolist() == codes.tolist() and d.growth == g0 + 1
    assert d.intern_batch(np.zeros(1, dtype=np.int64), b"").tolist() == []


# ---- the formatting code under ASan + UBSan, stand-alone ------------------------------------------------------
def test_str_make_under_asan_ubsan(tmp_path):
    """csrc/str_make.h compiled for the host into a program of its own, every output in a heap block of exactly the
    computed length: lengths and bytes are the fixture's, with no sanitizer finding."""
    exe = str(tmp_path / "strmake_san")
    _build(["g++", *ASAN, "-std=c++17", os.path.join(SAN, "strmake_san.cpp"), "-o", exe], tmp_path)
    out = _run(exe, os.path.join(ROOT, "tests", "golden", "str_make_cases.json"))
    assert f"{len(EDGES)} cases" in out, out
    assert "\n0 mismatches" in out, out


# ---- check_program over the recorded programs, under ASan + UBSan ------------------------------------------
def test_string_make_programs_under_asan_ubsan(tmp_path):
    """Accepted: STR, I64, untyped-NULL, typed-NULL and literal operands per opcode, BOOL too for TO_STRING.  Refused
    with NOT_IMPLEMENTED: an F64 operand (the message names Double.toString) and a list; with ILLEGAL_ARGUMENT: a BOOL in
    CONCAT, I64 + I64 and a mixed operand.  60..63 stay unknown."""
    fixture = os.path.join(ROOT, "tests", "golden", "string_make_programs.json")
    with open(fixture) as f:
        records = json.load(f)["records"]
    by_why = {r["why"]: r for r in records}
    assert len(by_why) == len(records)
    accepted = [r for r in records if r["status"] == 0 and not r["mixed_demand"]]
    for why in ("TO_STRING(STR)", "TO_STRING(I64)", "TO_STRING(BOOL)", "TO_STRING(NULL)", "TO_STRING(nullSTR)", "TO_STRING(litI64)",
                "TO_STRING(litSTR)", "CONCAT(STR,STR)", "CONCAT(STR,I64)", "CONCAT(I64,STR)", "CONCAT(STR,NULL)", "CONCAT(NULL,I64)",
                "CONCAT(nullSTR,STR)", "CONCAT(litSTR,litI64)", "CONCAT(litSTR,STR)"):
        assert by_why[why]["status"] == 0 and by_why[why]["type"] == 3, why
    for why in ("TO_STRING(F64)", "TO_STRING(litF64)", "CONCAT(F64,STR)", "CONCAT(STR,F64)"):
        assert by_why[why]["status"] == 2 and "Double.toString" in by_why[why]["message"], why
    for why in ("CONCAT(BOOL,STR)", "CONCAT(STR,BOOL)", "CONCAT(I64,I64)", "CONCAT(litI64,litI64)"):
        assert by_why[why]["status"] == 1, why
    for why in ("TO_STRING(LIST)", "CONCAT(LIST,STR)", "CONCAT(STR,LIST)"):
        assert by_why[why]["status"] == 2 and "a list value" in by_why[why]["message"], why
    for op in OPCODES.values():
        assert sum(1 for r in records if r["mixed_demand"] and r["prog"][-1][0] == op) >= 1
    assert by_why["STARTS_WITH(TO_STRING(I64),litSTR)"]["type"] == 1 and by_why["STR_SIZE(TO_STRING(I64))"]["type"] == 0
    assert by_why["ADD(I64,I64) stays ADD"]["type"] == 0
    for op in (60, 61, 62, 63):
        r = by_why[f"op {op} is unknown"]
        assert r["status"] == 2 and r["message"] == f"unknown expression op {op}"
    mixed = sum(1 for r in records if r["mixed_demand"])
    exe = str(tmp_path / "expr_san")
    _build(["g++", *ASAN, "-std=c++17", os.path.join(SAN, "expr_san.cpp"), "-o", exe], tmp_path)
    out = _run(exe, fixture)
    assert f"{len(records)} records, {len(accepted)} accepted" in out, out
    assert f"\n{mixed} mixed refused" in out, out
    assert "\n0 mismatches" in out, out
