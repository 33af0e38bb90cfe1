"""CPU checks of STARTS WITH / ENDS WITH / CONTAINS: the opcodes and operand order of compile_program against the
header, the planner DSL, StringDictionary.arrays() (the arrays of capsmi_session_set_strings), the entry point's null
check and the CAPSMI_STR_MATCH knob, and the transcription of tests/golden/string_predicates.json (a pure-Python
evaluation with str_match_ref reproduces every expected bag).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from golden_util import load_cases, same_rows
from str_match_ref import OPS, T, ref_match, slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases("string_predicates.json")


# ---- the binding against the header ---------------------------------------------------------------------
def test_opcode_values_match_the_header():
    from capsmi import expr
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    for name, want in (("STARTS_WITH", 29), ("ENDS_WITH", 30), ("CONTAINS", 31)):
        (v,) = re.findall(rf"CAPSMI_X_{name} = (\d+)", text)
        assert int(v) == want == getattr(expr, f"X_{name}")
    assert expr.STRING_MATCH_OPS == (29, 30, 31)


def test_compile_program_operand_order():
    from capsmi.expr import (Col, Contains, EndsWith, Lit, Not, StartsWith, X_COL, X_CONTAINS, X_ENDS_WITH, X_LIT, X_NOT,
                             X_STARTS_WITH, STR, columns_of, compile_program)
    idx = {"s": 0, "p": 1}.__getitem__
    enc = {"Al": 77}.__getitem__
    # [s, p]: left operand, right operand, opcode
    assert compile_program(StartsWith(Col("s"), Lit("Al")), idx, enc) == \
        [(X_COL, 0, 0, 0), (X_LIT, 0, STR, 77), (X_STARTS_WITH, 0, 0, 0)]
    assert compile_program(EndsWith(Col("s"), Col("p")), idx, enc) == [(X_COL, 0, 0, 0), (X_COL, 1, 0, 0), (X_ENDS_WITH, 0, 0, 0)]
    assert compile_program(Not(Contains(Lit("Al"), Col("p"))), idx, enc) == \
        [(X_LIT, 0, STR, 77), (X_COL, 1, 0, 0), (X_CONTAINS, 0, 0, 0), (X_NOT, 0, 0, 0)]
    assert columns_of(Contains(Col("s"), Col("p"))) == {"s", "p"}
    assert StartsWith(Col("s"), Lit("x")) == StartsWith(Col("s"), Lit("x")) != EndsWith(Col("s"), Lit("x"))


def test_planner_parses_the_new_forms():
    from capsmi import planner
    from capsmi.expr import Col, Contains, EndsWith, Lit, StartsWith
    h = ["n", "n.name", "n.r"]
    assert planner.to_expr(["starts_with", ["prop", "n", "name"], ["lit", "Al"]], h) == StartsWith(Col("n.name"), Lit("Al"))
    assert planner.to_expr(["ends_with", ["prop", "n", "name"], ["prop", "n", "r"]], h) == EndsWith(Col("n.name"), Col("n.r"))
    assert planner.to_expr(["contains", ["lit", "foobar"], ["prop", "n", "r"]], h) == Contains(Lit("foobar"), Col("n.r"))
    assert planner.to_expr(["not", ["contains", ["prop", "n", "gone"], ["lit", "x"]]], h).arg == Contains(Lit(None), Lit("x"))


def test_ctypes_declares_the_entry_point():
    from capsmi import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "capsmi.h")).read(), flags=re.S)
    (args,) = re.findall(r"^capsmi_status\s+capsmi_session_set_strings\s*\((.*?)\)\s*;", text, re.S | re.M)
    res, sig = _lib._SIGS["capsmi_session_set_strings"]
    assert len(sig) == " ".join(args.split()).count(",") + 1 == 5
    assert hasattr(_lib.load(), "capsmi_session_set_strings")


def test_set_strings_refuses_a_null_session():
    from capsmi import _lib
    lib = _lib.load()
    codes = np.array([1, 2], dtype=np.int64)
    offs = np.array([0, 1, 2], dtype=np.int64)
    assert lib.capsmi_session_set_strings(None, 2, codes.ctypes.data, offs.ctypes.data, b"ab") == _lib.ERR_ILLEGAL_ARGUMENT
    assert "null argument" in _lib.last_error()
    assert lib.capsmi_session_set_strings(None, 0, None, None, None) == _lib.ERR_ILLEGAL_ARGUMENT


def test_str_match_knob_is_checked():
    from capsmi import _lib
    lib = _lib.load()
    for v in (b"auto", b"rows", b"dict", None):
        assert lib.capsmi_config_check(b"CAPSMI_STR_MATCH", v) == _lib.OK, v
    assert lib.capsmi_config_check(b"CAPSMI_STR_MATCH", b"both") == _lib.ERR_ILLEGAL_ARGUMENT
    assert "configuration" in _lib.last_error()


def test_tile_constant_matches_the_kernel():
    text = open(os.path.join(ROOT, "cypher-for-apache-spark_amd", "csrc", "capsmi_impl.h")).read()
    (tile,) = re.findall(r"constexpr int kExplodeTile = (\d+);", text)
    assert int(tile) == T


# ---- StringDictionary.arrays() --------------------------------------------------------------------------
def _check_arrays(d, strings):
    codes, offsets, data = d.arrays()
    n = len(d)
    assert codes.dtype == np.int64 and offsets.dtype == np.int64 and isinstance(data, bytes)
    assert len(codes) == n == len(set(strings)) and len(offsets) == n + 1
    assert offsets[0] == 0 and offsets[-1] == len(data) and np.all(np.diff(offsets) >= 0)
    assert np.all(np.diff(codes) > 0)  # strictly ascending
    decoded = [data[offsets[i]:offsets[i + 1]].decode("utf-8") for i in range(n)]
    assert decoded == sorted(set(strings))  # code order is string order
    for i, x in enumerate(decoded):
        assert d.encode(x) == codes[i] and d.decode(int(codes[i])) == x


def test_dictionary_arrays():
    from capsmi import StringDictionary
    first = ["b", "", "é", "日本", "abc", "zz"]
    d = StringDictionary(first)
    _check_arrays(d, first)
    _, offsets, data = d.arrays()
    lens = {data[offsets[i]:offsets[i + 1]].decode(): int(offsets[i + 1] - offsets[i]) for i in range(len(d))}
    assert lens[""] == 0 and lens["é"] == 2 and lens["日本"] == 6
    before = {x: d.encode(x) for x in first}
    g = d.growth
    d.extend(["a", "abd", "c", "日"])  # between known strings
    assert d.growth == g + 1
    _check_arrays(d, first + ["a", "abd", "c", "日"])
    assert {x: d.encode(x) for x in first} == before  # codes are stable
    d.extend(["a", "zz"])  # nothing new: no growth
    assert d.growth == g + 1
    d.encode("new")  # an encoded literal is inserted, and counted
    assert d.growth == g + 2
    assert StringDictionary().arrays()[1].tolist() == [0] and StringDictionary().growth == 0
    # bytes that are no UTF-8 travel as surrogate escapes: the second byte of é alone is one byte in the store
    lone = b"\xa9".decode("utf-8", "surrogateescape")
    r = StringDictionary(["é", lone])
    codes, offsets, data = r.arrays()
    assert sorted(data[offsets[i]:offsets[i + 1]] for i in range(2)) == [b"\xa9", b"\xc3\xa9"] and np.all(np.diff(codes) > 0)
    assert data[offsets[0]:offsets[1]] == "é".encode() and r.decode(int(codes[1])) == lone


# ---- the restatement and the golden file ----------------------------------------------------------------
def test_restatement_table():
    assert ref_match("starts_with", "foobar", "foo") is True and ref_match("starts_with", "foobar", "bar") is False
    assert ref_match("ends_with", "foobar", "bar") is True and ref_match("ends_with", "foobar", "foo") is False
    assert ref_match("contains", "foobarbaz", "baz") is True and ref_match("contains", "foobarbaz", "abc") is False
    for op in OPS:
        assert ref_match(op, None, "a") is None and ref_match(op, "a", None) is None and ref_match(op, None, None) is None
        assert ref_match(op, "", "") is True and ref_match(op, "abc", "") is True  # the empty pattern
        assert ref_match(op, "ab", "abc") is False and ref_match(op, "", "a") is False  # longer than the string
        assert ref_match(op, "abc", "abc") is True
    # bytes, not characters: the second byte of é is a suffix of it and occurs in it
    assert ref_match("ends_with", "é", b"\xa9") is True and ref_match("contains", "aéb", b"\xa9") is True
    assert ref_match("starts_with", "é", b"\xa9") is False
    assert ref_match("ends_with", "é", b"\xa9".decode("utf-8", "surrogateescape")) is True  # as the dictionary holds it
    assert slots("abcde", "abc") == 3 and slots("ab", "abc") == 0 and slots("abc", "") == 0 and slots(None, "a") == 0


def test_golden_file_shape_and_refs():
    ref = [c for c in CASES if not c.get("project_case")]
    assert len(ref) == 9 and len(CASES) == 12
    for c in ref:
        assert re.fullmatch(r"ExpressionBehaviour\.scala:\d+-\d+", c["ref"]), c["ref"]
    nulls = [c for c in ref if c["name"].endswith("can handle nulls")]
    assert len(nulls) == 3 and all("STARTS WITh" in c["cypher"] for c in nulls)  # as the reference has them
    assert [c["name"] for c in CASES if c.get("project_case")] == \
        ["ENDS WITH over the null graph", "CONTAINS over the null graph", "CONTAINS as a filter over four names"]
    for c in CASES:
        assert c["expected"] and "clauses" in c["query"] and c["cypher"]


def _eval(spec, row):
    op = spec[0]
    if op == "lit":
        return spec[1]
    if op == "prop":
        return row[spec[1]]["props"].get(spec[2])
    if op in OPS:
        return ref_match(op, _eval(spec[1], row), _eval(spec[2], row))
    raise NotImplementedError(op)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pure_python_evaluation_reproduces_the_expected_bag(case):
    from oracle.create_graph import create_graph
    g = create_graph(case["create"])
    (cl,) = case["query"]["clauses"]
    (var,) = re.fullmatch(r"\((\w*)\)", cl["match"]).groups()
    rows = [{var or "_": n} for n in g["nodes"]]
    if "where" in cl:
        rows = [r for r in rows if _eval(cl["where"], r) is True]
    got = [{alias: _eval(spec, row) for alias, spec in case["query"]["return"]["items"]} for row in rows]
    assert same_rows(got, case["expected"])
