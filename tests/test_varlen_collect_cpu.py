"""CPU checks of the var-length collect(DISTINCT b) route's yardstick: the per-source BFS of varlen_collect_ref.py
equals relationship-distinct path enumeration for lower <= 1 and agrees with the counts of reach_sets; the header
documents the two entry points; the list limit knob is registered.  No GPU."""
import os
import re

import numpy as np
import pytest

from varlen_collect_ref import reach_lists
from varlen_distinct_ref import reach_sets, trail_ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _multigraph(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 10))
    m = int(rng.integers(0, 15))
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 4] = dst[: m // 4]  # a quarter self-loops
    return n, src, dst, rng.random(n) < 0.7, rng.random(n) < 0.6


@pytest.mark.parametrize("seed", range(40))
def test_lists_equal_trail_enumeration(seed):
    n, src, dst, a_mask, b_mask = _multigraph(seed)
    for lower in (0, 1):
        for upper in (1, 2, 3, 4):
            lists, union = reach_lists(n, src, dst, a_mask, b_mask, lower, upper)
            all_ends = set()
            for a in range(n):
                if not a_mask[a]:
                    assert a not in lists
                    continue
                ends = {b for b in trail_ends(n, src, dst, a, lower, upper) if b_mask[b]}
                if lower == 0:
                    ends.add(a)  # the zero-length path's b is a copy of a, without b's filter
                assert lists.get(a, np.zeros(0, np.int64)).tolist() == sorted(ends), (seed, a, lower, upper)
                assert (a in lists) == bool(ends)
                all_ends |= ends
            assert union.tolist() == sorted(all_ends), (seed, lower, upper)


@pytest.mark.parametrize("seed", range(8))
def test_list_lengths_equal_reach_sets_counts(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 200))
    m = int(rng.integers(0, 1500))
    src = rng.integers(-3, n + 3, m).astype(np.int64)  # some endpoints outside the window
    dst = rng.integers(-3, n + 3, m).astype(np.int64)
    a_mask, b_mask = rng.random(n) < 0.7, rng.random(n) < 0.6
    for lower, upper in [(1, 1), (1, 3), (0, 3), (0, 10)]:
        lists, union = reach_lists(n, src, dst, a_mask, b_mask, lower, upper)
        counts, total = reach_sets(n, src, dst, a_mask, b_mask, lower, upper)
        assert {a: len(v) for a, v in lists.items()} == {int(i): int(counts[i]) for i in np.nonzero(counts)[0]}
        assert len(union) == total
        for v in lists.values():
            assert v.dtype == np.int64 and (np.diff(v) > 0).all()


def test_header_documents_both_entries():
    text = open(os.path.join(ROOT, "include", "capsmi.h")).read()
    for name in ("capsmi_var_length_collect_distinct", "capsmi_var_length_reach_list"):
        (decl,) = re.findall(rf"capsmi_status {name}\(([^;]*)\);", text)
        assert "const capsmi_bitmap* a_ok" in decl and "int32_t lower, int32_t upper" in decl, name
        assert "const char* list_name" in decl and "capsmi_table** out" in decl, name
        doc = text[: text.index(f"capsmi_status {name}(")].rsplit("/*", 1)[1]
        assert "collect(DISTINCT b)" in doc and "ascending" in doc, name
        assert "CAPSMI_ERR_NOT_IMPLEMENTED" in doc and "lower = 0" in doc, name
        assert "CAPSMI_REACH_LIST_LIMIT" in doc, name
    from capsmi import _lib
    assert "capsmi_var_length_collect_distinct" in _lib.EXPORTED and "capsmi_var_length_reach_list" in _lib.EXPORTED


def test_list_limit_knob_is_registered():
    from capsmi import _lib
    lib = _lib.load()
    for v in (b"auto", b"1000"):
        assert lib.capsmi_config_check(b"CAPSMI_REACH_LIST_LIMIT", v) == _lib.OK, v
    for v in (b"-1", b"x"):
        assert lib.capsmi_config_check(b"CAPSMI_REACH_LIST_LIMIT", v) == _lib.ERR_ILLEGAL_ARGUMENT, v
