"""CPU checks of the var-length count(DISTINCT b) route's yardstick: the walk BFS of varlen_distinct_ref.py equals
relationship-distinct path enumeration for lower <= 1 (the lemma the route rests on), the lower = 2 counterexample
that keeps lower >= 2 on the join plan, the brute-force MATCH enumeration's count_distinct on the same graphs, and
the header's two entry points.  No GPU."""
import os
import re

import numpy as np
import pytest

from varlen_distinct_ref import reach_sets, trail_ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _multigraph(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 9))
    m = int(rng.integers(0, 15))
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 4] = dst[: m // 4]  # a quarter self-loops
    return n, src, dst, rng.random(n) < 0.7, rng.random(n) < 0.6


@pytest.mark.parametrize("seed", range(40))
def test_walk_bfs_equals_trail_enumeration(seed):
    n, src, dst, a_mask, b_mask = _multigraph(seed)
    for lower in (0, 1):
        for upper in (1, 2, 3, 5, 6):
            counts, union = reach_sets(n, src, dst, a_mask, b_mask, lower, upper)
            all_ends = set()
            for a in range(n):
                if not a_mask[a]:
                    assert counts[a] == 0
                    continue
                ends = {b for b in trail_ends(n, src, dst, a, lower, upper) if b_mask[b]}
                if lower == 0:
                    ends.add(a)  # the zero-length path's b is a copy of a, without b's filter
                assert counts[a] == len(ends), (seed, a, lower, upper)
                all_ends |= ends
            assert union == len(all_ends), (seed, lower, upper)


def test_lower_two_counterexample():
    """Two nodes and the relationships 0 -> 1 and 1 -> 0.  The walk 0 -> 1 -> 0 -> 1 of length 3 uses 0 -> 1 twice, so
    node 1 ends a walk of length in [2, 3] from 0 and no relationship-distinct path of that length: walks and
    trails part at lower = 2, and the route refuses it.  At lower = 1 the one-hop path 0 -> 1 is there and they agree."""
    src, dst = np.array([0, 1]), np.array([1, 0])
    assert trail_ends(2, src, dst, 0, 2, 3) == {0}
    level, walk_ends = {0}, set()
    for depth in range(1, 4):
        level = {int(d) for s, d in zip(src, dst) if int(s) in level}
        if depth >= 2:
            walk_ends |= level
    assert walk_ends == {0, 1}
    assert trail_ends(2, src, dst, 0, 1, 3) == {0, 1}
    assert reach_sets(2, src, dst, [True, False], [True, True], 1, 3)[0].tolist() == [2, 0]


@pytest.mark.parametrize("seed", [1, 5, 9, 14])
def test_enumeration_oracle_agrees_for_lower_one(seed):
    """oracle/enumerate.py (the reference's bindings restated) on the same graphs, lower = 1; labelled b."""
    from oracle import enumerate as en
    n, src, dst, a_mask, b_mask = _multigraph(seed)
    g = {"nodes": [{"id": i, "labels": (["A"] if a_mask[i] else []) + (["B"] if b_mask[i] else []), "props": {}}
                   for i in range(n)],
         "rels": [{"id": n + e, "src": int(s), "dst": int(d), "type": "T", "props": {}}
                  for e, (s, d) in enumerate(zip(src, dst))]}
    graph = en.Graph(g)
    for upper in (1, 2, 3, 5):
        q = {"clauses": [{"match": f"(a:A)-[:T*1..{upper}]->(b:B)"}],
             "return": {"items": [["a", ["id", "a"]], ["n", ["count_distinct", ["id", "b"]]]]}}
        rows = en.project(graph, en.match(graph, q), q["return"])
        counts, union = reach_sets(n, src, dst, a_mask, b_mask, 1, upper)
        assert {r["a"]: r["n"] for r in rows} == {int(i): int(counts[i]) for i in np.nonzero(counts)[0]}
        q1 = {"clauses": q["clauses"], "return": {"items": [["n", ["count_distinct", ["id", "b"]]]]}}
        assert en.project(graph, en.match(graph, q1), q1["return"]) == [{"n": union}]


def test_header_declares_both_entries_with_the_lemma():
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    for name in ("capsmi_var_length_count_distinct", "capsmi_var_length_reach_count"):
        (decl,) = re.findall(rf"capsmi_status {name}\(([^;]*)\);", text)
        assert "const capsmi_bitmap* a_ok" in decl and "int32_t lower, int32_t upper" in decl, name
        doc = text[: text.index(f"capsmi_status {name}(")].rsplit("/*", 1)[1]
        assert "count(DISTINCT b)" in doc and "walk" in doc and "relationship-distinct" in doc, name
        assert "CAPSMI_ERR_NOT_IMPLEMENTED" in doc and "lower = 0" in doc, name
    from capsmi import _lib
    assert "capsmi_var_length_count_distinct" in _lib.EXPORTED and "capsmi_var_length_reach_count" in _lib.EXPORTED


def test_reach_words_knob_is_registered():
    from capsmi import _lib
    lib = _lib.load()
    for v in (b"auto", b"1", b"2", b"4", b"8"):
        assert lib.capsmi_config_check(b"CAPSMI_REACH_WORDS", v) == _lib.OK, v
    for v in (b"3", b"16", b"0", b"wide"):
        assert lib.capsmi_config_check(b"CAPSMI_REACH_WORDS", v) == _lib.ERR_ILLEGAL_ARGUMENT, v
    assert lib.capsmi_config_check(b"CAPSMI_REACH", b"flat") == _lib.OK
    assert lib.capsmi_config_check(b"CAPSMI_REACH", b"atomic") == _lib.ERR_ILLEGAL_ARGUMENT
