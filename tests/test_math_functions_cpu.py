"""CPU checks of division, the math functions, toFloat and toInteger (CAPSMI_X_DIV .. CAPSMI_X_TO_INTEGER): the
restatement of math_ref.py at the edges the header names and over the transcription of tests/golden/math_functions.json,
the opcodes and operand order of compile_program against the header, the planner DSL, check_program over
tests/golden/math_programs.json under ASan + UBSan (tests/sanitize/expr_san.cpp, built as test_sanitizers.py builds
it), and the registers of the two k_eval instantiations in the built object.  No GPU."""
import json
import math
import os
import re
import subprocess

import pytest

import math_ref as mr
from golden_util import load_cases, same_rows
from test_kernel_resources import LLVM
from test_sanitizers import ASAN, SAN, _build, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("math_functions.json")
OPCODES = {"DIV": 40, "SQRT": 41, "LOG": 42, "LOG10": 43, "EXP": 44, "ABS": 45, "CEIL": 46, "FLOOR": 47, "ROUND": 48,
           "SIGN": 49, "TO_FLOAT": 50, "TO_INTEGER": 51}
INF, NAN = math.inf, math.nan


# ---- the restatement -------------------------------------------------------------------------------------
def _same(got, want):
    assert mr.same_value(got, want), (got, want)


def test_restatement_division():
    for a, b, want in ((9, 3, 3), (3, 2, 1), (-7, 2, -3), (7, -2, -3), (mr.LONG_MIN, -1, mr.LONG_MAX),
                       (2 ** 53 + 1, 1, 2 ** 53), (0, 0, None), (5, 0, None), (5.0, -0.0, None), (1.0, -0.0, None),
                       (9, 4.5, 2.0), (1.0, 4, 0.25), (INF, INF, NAN), (NAN, 2, NAN), (1.0, INF, 0.0), (-1, INF, -0.0),
                       (INF, 2, INF), (None, 2, None), (2, None, None), (True, 2, None), (2.0, "x", None)):
        _same(mr.div(a, b), want)


def test_restatement_functions():
    table = {
        "sqrt": ((12.96, 3.6), (9, 3.0), (-1.0, NAN), (-0.0, -0.0), (INF, INF), (NAN, NAN), (None, None)),
        "log": ((0, None), (0.0, None), (-0.0, None), (-1, None), (NAN, NAN), (INF, INF), (1, 0.0), (None, None),
                (12.96, 2.561867690924129), (9, 2.1972245773362196)),
        "log10": ((1000, 2.9999999999999996), (12.96, 1.1126050015345745), (100, 2.0), (0, None), (-0.0, None),
                  (NAN, NAN), (None, None)),
        "exp": ((0, 1.0), (710, INF), (-746, 0.0), (1.337, 3.8076035433731965), (2, 7.38905609893065), (NAN, NAN),
                (-INF, 0.0), (None, None)),
        "abs": ((mr.LONG_MIN, mr.LONG_MIN), (-23, 23), (-12.96, 12.96), (-0.0, 0.0), (-INF, INF), (None, None)),
        "ceil": ((-0.5, 0.0), (0.1, 1.0), (1, 1.0), (1e300, 2.0 ** 63), (-1e300, -(2.0 ** 63)), (NAN, 0.0), (INF, 2.0 ** 63),
                 (2 ** 53 + 1, 2.0 ** 53), (None, None)),
        "floor": ((-0.0, 0.0), (1.9, 1.0), (-0.5, -1.0), (1, 1.0), (NAN, 0.0), (-INF, -(2.0 ** 63)), (None, None)),
        "round": ((0.5, 1.0), (-0.5, -1.0), (2.5, 3.0), (-2.5, -3.0), (0.49999999999999994, 0.0), (-0.4, 0.0), (-0.0, 0.0),
                  (2.0 ** 52 + 1, 2.0 ** 52 + 1), (1.9, 2.0), (1, 1.0), (NAN, NAN), (INF, INF), (-INF, -INF), (None, None)),
        "sign": ((-1.1, -1), (1, 1), (0, 0), (-0.0, 0), (0.0, 0), (NAN, 0), (-INF, -1), (mr.LONG_MIN, -1), (None, None)),
        "tofloat": ((1, 1.0), (1.0, 1.0), (2 ** 53 + 1, 2.0 ** 53), (-0.0, -0.0), (None, None)),
        "tointeger": ((2 ** 31, -2 ** 31), (2 ** 32 + 5, 5), (-1, -1), (3e9, 2 ** 31 - 1), (-3e9, -2 ** 31), (NAN, 0),
                      (82.9, 82), (-82.9, -82), (INF, 2 ** 31 - 1), (None, None)),
    }
    assert sorted(table) == sorted(mr.OPS)
    for op, rows in table.items():
        for x, want in rows:
            assert mr.same_value(mr.FUNCS[op](x), want), (op, x, mr.FUNCS[op](x), want)
        assert mr.FUNCS[op](True) is None and mr.FUNCS[op]("1") is None  # no numbers
    assert [mr.sat_i64(d) for d in (NAN, 2.0 ** 63, -(2.0 ** 63), 1e300, -1.9, 1.9)] == [0, mr.LONG_MAX, mr.LONG_MIN, mr.LONG_MAX, -1, 1]
    assert mr.LN10 == math.log(10.0)


# ---- the golden file -------------------------------------------------------------------------------------
def test_golden_file_shape_and_refs():
    assert len(CASES) == 32
    for c in CASES:
        assert re.fullmatch(r"(Expression|Functions)Behaviour\.scala:\d+-\d+", c["ref"]), c["ref"]
        assert c["expected"] and "clauses" in c["query"] and c["cypher"]
    words = {c["query"]["return"]["items"][0][1][0] for c in CASES}
    assert words == {"/", "e", "sqrt", "log", "log10", "exp", "abs", "ceil", "floor", "round", "sign", "tofloat"}
    assert not any("tointeger" in json.dumps(c["query"]) for c in CASES)  # the reference's are all over strings


def _rows(case):
    from oracle.create_graph import create_graph
    g = create_graph(case["create"])
    clauses = case["query"]["clauses"]
    if not clauses:
        return [{}]  # no clause: the unit row
    (cl,) = clauses
    one = re.fullmatch(r"\((\w+)\)", cl["match"])
    if one:
        return [{one.group(1): n} for n in g["nodes"]]
    a, la, b, lb = re.fullmatch(r"\((\w+):(\w+)\)-->\((\w+):(\w+)\)", cl["match"]).groups()
    by_id = {n["id"]: n for n in g["nodes"]}
    return [{a: by_id[r["src"]], b: by_id[r["dst"]]} for r in g["rels"]
            if la in by_id[r["src"]]["labels"] and lb in by_id[r["dst"]]["labels"]]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pure_python_evaluation_reproduces_the_expected_bag(case):
    got = [{alias: mr.eval_spec(spec, row) for alias, spec in case["query"]["return"]["items"]} for row in _rows(case)]
    assert same_rows(got, case["expected"]), got
    if len(got) == 1:  # one row: the value itself, type and bits
        (g,), (e,) = got, case["expected"]
        assert all(mr.same_value(g[k], e[k]) for k in e), (g, e)


# ---- the binding against the header ----------------------------------------------------------------------
def test_opcode_values_match_the_header():
    from capsmi import expr
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    for name, want in OPCODES.items():
        (v,) = re.findall(rf"CAPSMI_X_{name} = (\d+)", text)
        assert int(v) == want == getattr(expr, f"X_{name}"), name
    assert expr.BIN_OPS["/"] == 40
    assert not re.search(r"CAPSMI_X_[A-Z0-9_]+ = 3[2-9]\b", text)  # 32..39 stay unassigned
    assert expr.E == expr.Lit(math.e) and expr.E.resolved_type() == expr.F64


def test_compile_program_operand_order():
    from capsmi import expr
    from capsmi.expr import BinOp, Col, Lit, X_COL, X_LIT, F64, columns_of, compile_program
    idx = {"x": 0, "y": 1}.__getitem__
    assert compile_program(BinOp("/", Col("x"), Col("y")), idx, None) == [(X_COL, 0, 0, 0), (X_COL, 1, 0, 0), (40, 0, 0, 0)]
    assert compile_program(BinOp("/", Col("y"), Col("x")), idx, None) == [(X_COL, 1, 0, 0), (X_COL, 0, 0, 0), (40, 0, 0, 0)]
    classes = {"Sqrt": 41, "Log": 42, "Log10": 43, "Exp": 44, "Abs": 45, "Ceil": 46, "Floor": 47, "Round": 48, "Sign": 49,
               "ToFloat": 50, "ToInteger": 51}
    for name, op in classes.items():
        cls = getattr(expr, name)
        assert compile_program(cls(Col("y")), idx, None) == [(X_COL, 1, 0, 0), (op, 0, 0, 0)], name
        assert "SparkSQLExprMapper.scala" in cls.__doc__
        assert columns_of(cls(BinOp("/", Col("x"), Col("y")))) == {"x", "y"}
        assert cls(Col("x")) == cls(Col("x")) != cls(Col("y"))
    e_bits = mr.bits(math.e)
    assert compile_program(expr.Log(expr.E), idx, None) == [(X_LIT, 0, F64, e_bits), (42, 0, 0, 0)]
    assert compile_program(expr.Sqrt(expr.ToFloat(BinOp("/", Col("x"), Lit(2)))), idx, None) == \
        [(X_COL, 0, 0, 0), (X_LIT, 0, 0, 2), (40, 0, 0, 0), (50, 0, 0, 0), (41, 0, 0, 0)]


def test_planner_parses_the_new_forms():
    from capsmi import expr, planner
    from capsmi.expr import BinOp, Col, Lit
    h = ["n", "n.val", "m", "m.val"]
    x = ["prop", "n", "val"]
    assert planner.to_expr(["/", x, ["prop", "m", "val"]], h) == BinOp("/", Col("n.val"), Col("m.val"))
    words = {"sqrt": "Sqrt", "log": "Log", "log10": "Log10", "exp": "Exp", "abs": "Abs", "ceil": "Ceil", "floor": "Floor",
             "round": "Round", "sign": "Sign", "tofloat": "ToFloat", "tointeger": "ToInteger"}
    assert sorted(words) == sorted(mr.OPS)
    for word, name in words.items():
        assert planner.to_expr([word, x], h) == getattr(expr, name)(Col("n.val")), word
    assert planner.to_expr(["e"], h) == expr.E
    assert planner.to_expr(["sqrt", ["prop", "n", "gone"]], h) == expr.Sqrt(Lit(None))
    assert planner.to_expr(["index", ["var", "xs"], ["tointeger", x]], h + ["xs"]) == expr.Index(Col("xs"), expr.ToInteger(Col("n.val")))


# ---- check_program over the recorded programs, under ASan + UBSan ------------------------------------------
def test_math_programs_under_asan_ubsan(tmp_path):
    """Accepted programs for every new opcode over I64, F64, untyped-NULL and mixed operands with their static types;
    BOOL, STR and list operands, opcodes 32, 39 and 52 and a DIV with one operand refused, message for message."""
    fixture = os.path.join(ROOT, "tests", "golden", "math_programs.json")
    with open(fixture) as f:
        records = json.load(f)["records"]
    ops = lambda r: {row[0] for row in r["prog"]}  # noqa: E731
    accepted = [r for r in records if r["status"] == 0 and not r["mixed_demand"]]
    for op in OPCODES.values():
        for operand in ("(I64", "(F64", "(NULL", "(mixed"):
            assert any(op in ops(r) and operand in r["why"] for r in accepted), (op, operand)
        for operand in ("BOOL", "STR", "LIST"):
            assert any(op in ops(r) and operand in r["why"] and r["status"] == 2 for r in records), (op, operand)
    for op in (32, 39, 52):
        assert any(op in ops(r) and r["message"] == f"unknown expression op {op}" and r["status"] == 2 for r in records)
    assert any(r["why"] == "DIV with one operand" and r["status"] == 1 and "underflow" in r["message"] for r in records)
    mixed = sum(1 for r in records if r["mixed_demand"])
    assert mixed == 2
    exe = str(tmp_path / "expr_san")
    _build(["g++", *ASAN, "-std=c++17", os.path.join(SAN, "expr_san.cpp"), "-o", exe], tmp_path)
    out = _run(exe, fixture)
    assert f"{len(records)} records, {len(accepted)} accepted" in out, out
    assert f"\n{mixed} mixed refused" in out, out
    assert "\n0 mismatches" in out, out


# ---- the two instantiations of the interpreter -------------------------------------------------------------
OBJ = os.path.join(ROOT, "cypher-for-apache-spark_amd", "build", "k_expr.o")
# k_eval of the parent commit 6fc3be8, built with the same compiler: the program that holds none of the new opcodes
# runs a kernel that is no larger
PARENT_VGPRS, PARENT_PRIVATE_BYTES = 22, 544


def _k_eval(obj, tmp):
    """{False / True: (vgpr_count, private_segment_fixed_size)} of k_eval<false> / k_eval<true>."""
    fat, co = os.path.join(tmp, "k.fatbin"), os.path.join(tmp, "k.co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, obj, os.path.join(tmp, "o")],
                   check=True, capture_output=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", notes)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", block).group(1)
        m = re.search(r"6k_evalILb([01])EE", name)
        if m:
            out[m.group(1) == "1"] = (int(re.search(r"\n    \.vgpr_count:\s+(\d+)", block).group(1)),
                                      int(re.search(r"\n    \.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")),
                    reason="k_expr.o not built or no ROCm llvm tools")
def test_the_plain_interpreter_is_no_larger_than_the_parents(tmp_path):
    ks = _k_eval(OBJ, str(tmp_path))
    assert sorted(ks) == [False, True], ks  # both instantiations exist
    vgprs, private = ks[False]
    print(f"k_eval<false>: {vgprs} VGPRs, {private} B private; k_eval<true>: {ks[True][0]} VGPRs, {ks[True][1]} B private")
    assert vgprs <= PARENT_VGPRS and private <= PARENT_PRIVATE_BYTES, ks
