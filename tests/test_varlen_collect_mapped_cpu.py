"""CPU checks of the yardstick of var-length collect(DISTINCT b) over remapped ids: mapped_lists (reach_lists, then
``sorted(ids[x] for x in list)``) equals relationship-distinct path enumeration on graphs whose node ids are a random
permutation -- oracle/enumerate.py for lower = 1, trail_ends for lower = 0 -- and the header documents the two mapped
entry points.  No GPU."""
import os
import re

import numpy as np
import pytest

from varlen_collect_mapped_ref import id_sets, mapped_lists
from varlen_distinct_ref import trail_ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPPED = ("capsmi_var_length_collect_distinct_mapped", "capsmi_var_length_reach_list_mapped")


def _multigraph(seed):
    rng = np.random.default_rng(2000 + seed)
    n = int(rng.integers(1, 10))
    m = int(rng.integers(0, 15))
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 4] = dst[: m // 4]  # a quarter self-loops
    ids = id_sets()["signed" if seed % 2 else "random"](rng, n)
    return n, src, dst, rng.random(n) < 0.7, rng.random(n) < 0.6, ids


@pytest.mark.parametrize("seed", range(6))
def test_mapped_lists_equal_the_enumeration_oracle(seed):
    """oracle/enumerate.py on the graph in ORIGINAL ids (a random permutation, or signed ids far apart), lower = 1."""
    from oracle import enumerate as en
    n, src, dst, a_mask, b_mask, ids = _multigraph(seed)
    g = {"nodes": [{"id": int(ids[i]), "labels": (["A"] if a_mask[i] else []) + (["B"] if b_mask[i] else []), "props": {}}
                   for i in range(n)],
         "rels": [{"id": (1 << 50) + e, "src": int(ids[s]), "dst": int(ids[d]), "type": "T", "props": {}}
                  for e, (s, d) in enumerate(zip(src, dst))]}
    graph = en.Graph(g)
    for upper in (1, 2, 3, 5):
        lists, union = mapped_lists(n, src, dst, a_mask, b_mask, 1, upper, ids)
        q = {"clauses": [{"match": f"(a:A)-[:T*1..{upper}]->(b:B)"}],
             "return": {"items": [["a", ["id", "a"]], ["ds", ["collect_distinct", ["id", "b"]]],
                                  ["n", ["count_distinct", ["id", "b"]]]]}}
        rows = en.project(graph, en.match(graph, q), q["return"])
        assert {r["a"]: list(r["ds"]) for r in rows} == lists, (seed, upper)
        assert all(r["n"] == len(r["ds"]) for r in rows)
        q1 = {"clauses": q["clauses"], "return": {"items": [["ds", ["collect_distinct", ["id", "b"]]]]}}
        (row,) = en.project(graph, en.match(graph, q1), q1["return"])
        assert list(row["ds"]) == union, (seed, upper)


@pytest.mark.parametrize("seed", range(6, 16))
def test_mapped_lists_equal_trail_enumeration(seed):
    n, src, dst, a_mask, b_mask, ids = _multigraph(seed)
    for lower in (0, 1):
        for upper in (1, 3, 4):
            lists, union = mapped_lists(n, src, dst, a_mask, b_mask, lower, upper, ids)
            all_ends = set()
            for a in range(n):
                if not a_mask[a]:
                    assert int(ids[a]) not in lists
                    continue
                ends = {b for b in trail_ends(n, src, dst, a, lower, upper) if b_mask[b]}
                if lower == 0:
                    ends.add(a)  # the zero-length path's b is a copy of a, without b's filter
                want = sorted(int(ids[b]) for b in ends)
                assert lists.get(int(ids[a]), []) == want, (seed, a, lower, upper)
                all_ends |= ends
            assert union == sorted(int(ids[b]) for b in all_ends)


def test_signed_ids_sort_as_longs():
    rng = np.random.default_rng(3)
    ids = id_sets()["signed"](rng, 64)
    assert (ids < 0).any() and (ids > (1 << 61)).any() and ((ids > (1 << 39)) & (ids < (1 << 41))).any()
    n = len(ids)
    src, dst = np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64)  # a hub: its list is every id
    ones = np.ones(n, bool)
    lists, union = mapped_lists(n, src, dst, ones, ones, 1, 1, ids)
    assert lists == {int(ids[0]): np.sort(ids).tolist()} and union == np.sort(ids).tolist()
    assert union[0] < 0 < union[-1]


def test_header_documents_the_mapped_entries():
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    for name in MAPPED:
        (decl,) = re.findall(rf"capsmi_status {name}\(([^;]*)\);", text)
        assert "const capsmi_bitmap* a_ok" in decl and "int32_t lower, int32_t upper" in decl, name
        assert "const int64_t* orig" in decl and "int64_t orig_len" in decl, name
        assert "const char* list_name" in decl and "capsmi_table** out" in decl, name
        doc = text[: text.index(f"capsmi_status {name}(")].rsplit("/*", 1)[1]
        assert "collect(DISTINCT b)" in doc and "ascending" in doc and "signed" in doc, name
        assert "lemma" in doc and "CAPSMI_ERR_NOT_IMPLEMENTED" in doc and "lower = 0" in doc, name
        assert "CAPSMI_REACH_LIST_LIMIT" in doc and "distinct" in doc and "CAPSMI_ERR_ILLEGAL_ARGUMENT" in doc, name
    from capsmi import _lib
    assert all(name in _lib.EXPORTED for name in MAPPED)
