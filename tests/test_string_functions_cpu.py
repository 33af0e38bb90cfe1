"""CPU checks of size(), toInteger(), toFloat() and toBoolean() of a String (CAPSMI_X_STR_SIZE .. CAPSMI_X_TO_BOOLEAN):
the restatement of str_conv_ref.py over the transcription of tests/golden/string_functions.json and over the edge
inputs of tests/golden/str_conv_cases.json, the opcodes of compile_program against the header, the planner DSL,
csrc/str_conv.h under ASan + UBSan in a stand-alone program over those edge inputs (tests/sanitize/strconv_san.cpp),
and check_program over tests/golden/string_function_programs.json (tests/sanitize/expr_san.cpp, unchanged).  No GPU."""
import json
import math
import os
import re

import pytest

import str_conv_ref as sr
from golden_util import load_cases, same_rows
from test_sanitizers import ASAN, SAN, _build, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("string_functions.json")
EDGES = load_cases("str_conv_cases.json")
OPCODES = {"STR_SIZE": 56, "STR_TO_INTEGER": 57, "STR_TO_FLOAT": 58, "TO_BOOLEAN": 59}
WORDS = {"str_size": "StrSize", "str_tointeger": "StrToInteger", "str_tofloat": "StrToFloat", "toboolean": "ToBoolean"}


# ---- the restatement -------------------------------------------------------------------------------------
def test_restatement_at_the_edges_the_header_names():
    assert [sr.size(s) for s in ("", "Alice", "é", "日本語", "\U0001F600", None)] == [0, 5, 1, 3, 1, None]
    assert sr.size(bytes([0x80, 0xC3, 0x41, 0xFF, 0xBF])) == 3  # ill-formed: still the bytes that are not 10xxxxxx
    ints = {"": None, "+": None, "-": None, ".": 0, "+.": 0, "-.": 0, ".5": 0, "5.": 5, "-0": 0, "+7": 7, "007": 7,
            "2147483647": 2 ** 31 - 1, "2147483648": None, "-2147483648": -2 ** 31, "-2147483649": None, "9" * 20: None,
            "0" * 40 + "5": 5, "1e3": None, " 1": None, "1 ": None, "1.2.3": None, "1.x": None, "--1": None, "1-": None,
            "٣": None, "82.9": 82, "-82.9": -82, "0.999999": 0}
    for s, want in ints.items():
        assert sr.to_integer(s) == want, s
    floats = {"42": 42.0, "1.": 1.0, ".5": 0.5, ".": None, "": None, "1e": None, "1e+": None, "1e5": 1e5, "1E-5": 1e-5,
              "Infinity": math.inf, "-Infinity": -math.inf, "infinity": None, "Inf": None, "nan": None, "1d": 1.0, "1F": 1.0,
              "1dd": None, "d": None, " 1.5 ": 1.5, "\t1.5\n": 1.5, "1 .5": None, "1_0": None, "0x1p3": 8.0, "0X1.8P1": 3.0,
              "0x1": None, "0x.8p0": 0.5, "0xp0": None, "0x1p-1075": 0.0, "1e400": math.inf, "-1e400": -math.inf,
              "4.9e-324": 5e-324, "2.4703282292062327e-324": 0.0, "2.4703282292062328e-324": 5e-324,
              "1.7976931348623158e308": 1.7976931348623157e308, "1.7976931348623159e308": math.inf,
              "9007199254740993": 2.0 ** 53, "9007199254740993." + "0" * 30 + "1": 2.0 ** 53 + 2,
              "1e99999999999999999999": math.inf, "0e99999999999999999999": 0.0, "1e-99999999999999999999": 0.0, "1٣": None}
    for s, want in floats.items():
        got = sr.to_float(s)
        assert (got is None) == (want is None) and (want is None or sr.bits_of(got) == sr.bits_of(want)), (s, got)
    assert sr.to_float_bits("NaN") == sr.to_float_bits("-NaN") == sr.NAN_BITS
    assert sr.bits_of(sr.to_float("-0")) == sr.bits_of(-0.0) != sr.bits_of(0.0)
    assert sr.to_float("0x1.0000000000000800p0") == 1.0 and sr.to_float("0x1.0000000000000801p0") == 1.0 + 2.0 ** -52
    for w in ("t", "true", "y", "yes", "1"):
        assert sr.to_boolean(w) is True and sr.to_boolean(w.upper()) is True
    for w in ("f", "false", "n", "no", "0"):
        assert sr.to_boolean(w) is False and sr.to_boolean(w.upper()) is False
    for w in ("tr ue", " true", "true ", "", "2", "yes!", "on", "ｔ", None):
        assert sr.to_boolean(w) is None, w
    assert sr.to_boolean(True) is True and sr.to_boolean(False) is False


def test_the_edge_fixture_is_what_the_restatement_gives():
    per_op = {op: [c for c in EDGES if c["op"] == op] for op in WORDS}
    assert sum(len(v) for v in per_op.values()) == len(EDGES)
    for op, cases in per_op.items():
        assert 8 <= len(cases) <= 80, op  # one table per opcode on the device
        assert any(c["in"] is None for c in cases), op
        for c in cases:
            s = None if c["in"] is None else bytes.fromhex(c["in"])
            assert sr.word_of(op, s) == (int(c["word"]), c["ok"]), c
    longest = max(len(c["in"]) // 2 for c in per_op["str_tofloat"] if c["in"])
    assert longest > sr_digits()  # a mantissa longer than the slow path's digit buffer
    assert [c["raw"] for c in EDGES].count(True) == 1


def sr_digits():
    text = open(os.path.join(ROOT, "cypher-for-apache-spark_amd", "csrc", "str_conv.h")).read()
    (n,) = re.findall(r"constexpr int kDecDigits = (\d+);", text)
    return int(n)


# ---- the golden file -------------------------------------------------------------------------------------
def test_golden_file_shape_and_refs():
    assert len(CASES) == 11
    for c in CASES:
        assert re.fullmatch(r"FunctionsBehaviour\.scala:\d+-\d+", c["ref"]), c["ref"]
        assert c["expected"] and len(c["query"]["clauses"]) == 1 and c["cypher"]
    assert {c["query"]["return"]["items"][0][1][0] for c in CASES} == set(WORDS)


def _eval(spec, node):
    if spec[0] == "lit":
        return spec[1]
    if spec[0] == "prop":
        return node["props"].get(spec[2])
    return sr.FUNCS[spec[0]](_eval(spec[1], node))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pure_python_evaluation_reproduces_the_expected_bag(case):
    from oracle.create_graph import create_graph
    nodes = create_graph(case["create"])["nodes"]
    got = [{alias: _eval(spec, n) for alias, spec in case["query"]["return"]["items"]} for n in nodes]
    assert same_rows(got, case["expected"]), got
    for g in got:  # the types too: a Long is no Double, a Boolean no Long
        for v in g.values():
            assert v is None or type(v) in {type(e[k]) for e in case["expected"] for k in e if e[k] is not None}


# ---- the binding against the header ----------------------------------------------------------------------
def test_opcode_values_match_the_header():
    from capsmi import expr
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    for name, want in OPCODES.items():
        (v,) = re.findall(rf"CAPSMI_X_{name} = (\d+)", text)
        assert int(v) == want == getattr(expr, f"X_{name}"), name
    assert not re.search(r"CAPSMI_X_[A-Z0-9_]+ = 5[2-5]\b", text)  # 52..55 stay unassigned
    assert expr.STRING_CONV_OPS == (56, 57, 58, 59)
    assert expr.STRING_STORE_OPS == expr.STRING_MATCH_OPS + expr.STRING_CONV_OPS
    assert "stated from knowledge of Spark's source, not from a run" in re.sub(r"\s+", " ", text[text.index("52..55"):])


def test_compile_program_and_columns_of():
    from capsmi import expr
    from capsmi.expr import BinOp, Coalesce, Col, Lit, X_COL, X_LIT, X_NULL, STR, columns_of, compile_program
    idx = {"x": 0, "y": 1}.__getitem__
    for name, op in zip(WORDS.values(), OPCODES.values()):
        cls = getattr(expr, name)
        assert compile_program(cls(Col("y")), idx, None) == [(X_COL, 1, 0, 0), (op, 0, 0, 0)], name
        assert compile_program(cls(Lit("abc")), idx, lambda s: 77) == [(X_LIT, 0, STR, 77), (op, 0, 0, 0)]
        assert compile_program(cls(Lit(None, STR)), idx, None) == [(X_NULL, STR + 1, 0, 0), (op, 0, 0, 0)]
        assert "SparkSQLExprMapper.scala" in cls.__doc__
        assert columns_of(cls(Coalesce((Col("x"), Col("y"))))) == {"x", "y"}
        assert cls(Col("x")) == cls(Col("x")) != cls(Col("y"))
    assert compile_program(BinOp(">", expr.StrToInteger(Col("x")), Lit(40)), idx, None) == \
        [(X_COL, 0, 0, 0), (57, 0, 0, 0), (X_LIT, 0, 0, 40), (expr.X_GT, 0, 0, 0)]
    # the list and number forms are what they were
    assert compile_program(expr.Size(Col("x")), idx, None)[-1][0] == 26
    assert compile_program(expr.ToFloat(Col("x")), idx, None)[-1][0] == 50
    assert compile_program(expr.ToInteger(Col("x")), idx, None)[-1][0] == 51


def test_planner_parses_the_new_words():
    from capsmi import expr, planner
    from capsmi.expr import BinOp, Col, Lit
    h = ["n", "n.val", "xs"]
    x = ["prop", "n", "val"]
    for word, name in WORDS.items():
        assert planner.to_expr([word, x], h) == getattr(expr, name)(Col("n.val")), word
        assert planner.to_expr([word, ["prop", "n", "gone"]], h) == getattr(expr, name)(Lit(None))
    assert planner.to_expr([">", ["str_tointeger", x], ["lit", 40]], h) == BinOp(">", expr.StrToInteger(Col("n.val")), Lit(40))
    # the words of the list and number forms build what they built
    assert planner.to_expr(["size", ["var", "xs"]], h) == expr.Size(Col("xs"))
    assert planner.to_expr(["tofloat", x], h) == expr.ToFloat(Col("n.val"))
    assert planner.to_expr(["tointeger", x], h) == expr.ToInteger(Col("n.val"))


# ---- the parsers under ASan + UBSan, stand-alone -------------------------------------------------------------
def test_str_conv_under_asan_ubsan(tmp_path):
    """csrc/str_conv.h compiled for the host into a program of its own, every input in a heap block of exactly its
    length: the count and the three parsers give the fixture's words and validities, with no sanitizer finding."""
    exe = str(tmp_path / "strconv_san")
    _build(["g++", *ASAN, "-std=c++17", os.path.join(SAN, "strconv_san.cpp"), "-o", exe], tmp_path)
    out = _run(exe, os.path.join(ROOT, "tests", "golden", "str_conv_cases.json"))
    nulls = sum(1 for c in EDGES if c["in"] is None)
    assert f"{len(EDGES)} cases, {nulls} null operands" in out, out
    assert "\n0 mismatches" in out, out


# ---- check_program over the recorded programs, under ASan + UBSan ------------------------------------------
def test_string_function_programs_under_asan_ubsan(tmp_path):
    """Accepted: STR, untyped-NULL and typed-NULL operands per opcode, BOOL too for TO_BOOLEAN.  Refused with
    ILLEGAL_ARGUMENT: I64, F64 and BOOL operands (but BOOL for TO_BOOLEAN) and a mixed operand; with NOT_IMPLEMENTED:
    a list, and the opcodes 52..55."""
    fixture = os.path.join(ROOT, "tests", "golden", "string_function_programs.json")
    with open(fixture) as f:
        records = json.load(f)["records"]
    ops = lambda r: {row[0] for row in r["prog"]}  # noqa: E731
    accepted = [r for r in records if r["status"] == 0 and not r["mixed_demand"]]
    for name, op in OPCODES.items():
        for operand in ("(STR)", "(NULL)", "(nullSTR)", "(litSTR)"):
            assert any(r["why"] == name + operand for r in accepted), (name, operand)
        for operand in ("I64", "F64", "BOOL"):
            want = 0 if (name, operand) == ("TO_BOOLEAN", "BOOL") else 1
            hits = [r for r in records if op in ops(r) and r["why"].startswith(f"{name}({operand})")]
            assert hits and all(r["status"] == want for r in hits), (name, operand)
        assert any(op in ops(r) and "LIST" in r["why"] and r["status"] == 2 for r in records), name
        assert sum(1 for r in records if op in ops(r) and r["mixed_demand"]) == 2, name
    for op in (52, 53, 54, 55):
        assert any(op in ops(r) and r["message"] == f"unknown expression op {op}" and r["status"] == 2 for r in records)
    mixed = sum(1 for r in records if r["mixed_demand"])
    exe = str(tmp_path / "expr_san")
    _build(["g++", *ASAN, "-std=c++17", os.path.join(SAN, "expr_san.cpp"), "-o", exe], tmp_path)
    out = _run(exe, fixture)
    assert f"{len(records)} records, {len(accepted)} accepted" in out, out
    assert f"\n{mixed} mixed refused" in out, out
    assert "\n0 mismatches" in out, out
