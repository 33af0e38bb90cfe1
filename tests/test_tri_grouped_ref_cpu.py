"""The two restatements of the per-node triangle counts (tests/tri_grouped_ref.py) against each other and
against the C enumeration of the whole count (oracle/rmat.c), on random multigraphs with self-loops; the
rotation symmetry that lets the planner route a grouping by b or by c; and the hand-built graphs' own claims."""
import itertools

import numpy as np
import pytest

import tri_grouped_ref as tg
from oracle import cpu


def _random(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 15))
    m = int(rng.integers(0, 90))
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 5] = dst[: m // 5]  # a fifth of the relationships are self-loops
    return n, src, dst


@pytest.mark.parametrize("seed", range(40))
def test_restatements_agree(seed):
    n, src, dst = _random(seed)
    by_a = tg.per_node_enumerate(n, src, dst)
    assert by_a.tolist() == tg.per_node_dense(n, src, dst).tolist()
    assert int(by_a.sum()) == cpu.triangle_enumerate(n, src, dst)
    assert tg.per_node_enumerate(n, src, dst, "b").tolist() == by_a.tolist()
    assert tg.per_node_enumerate(n, src, dst, "c").tolist() == by_a.tolist()


def test_reversed_arrows_give_the_same_counts():
    n, src, dst = _random(7)
    assert tg.per_node_enumerate(n, dst, src).tolist() == tg.per_node_enumerate(n, src, dst).tolist()


def test_float_branch_matches_int_branch():
    rng = np.random.default_rng(3)
    n, m = 401, 6000
    src, dst = rng.integers(0, 60, m), rng.integers(0, 60, m)  # the triangles among 60 of the 401 nodes
    assert tg.per_node_dense(n, src, dst)[:60].tolist() == tg.per_node_dense(60, src, dst).tolist()


def test_heavy_triangle_counts():
    n, src, dst = tg.heavy_triangle()
    want = tg.heavy_triangle_counts()
    assert tg.per_node_dense(n, src, dst).tolist() == want.tolist()
    assert want.min() > 2 ** 32


def test_prime_triangle_reaches_every_degree_order():
    """the shared builder's six pendant permutations put the corners into six different degree orders, above
    every leaf; the triangle's own part of every corner's cyclic count is 2*5*13 + 11*7*3"""
    orders = set()
    for pend in itertools.permutations((1, 2, 3)):
        n, src, dst = tg.prime_triangle(pend)
        assert n == 3 + 6 * tg.PENDANT_UNIT
        rid = tg.degree_order(n, src, dst)
        assert sorted(rid[:3].tolist()) == [0, 1, 2]  # the corners outrank every leaf
        orders.add(tuple(rid[:3].tolist()))
        nl = src != dst
        assert tg.per_node_dense(n, src[nl], dst[nl])[:3].tolist() == [361] * 3
    assert len(orders) == 6


def test_built_graphs_sit_on_the_edges():
    for t in (tg.TILE_SLOTS - 1, tg.TILE_SLOTS, tg.TILE_SLOTS + 1):
        slots = tg.walk_slots(*tg.disjoint_triangles(t))
        assert int(slots.sum()) == t and int(slots.max()) == 1
    for total in (2 * tg.TILE_SLOTS, 2 * tg.TILE_SLOTS + 1):
        slots = tg.walk_slots(*tg.clique_and_triangles(total))
        ends = np.cumsum(slots)
        assert int(ends[-1]) == total
        assert ((ends - slots < tg.TILE_SLOTS) & (ends > tg.TILE_SLOTS)).any()  # a row straddles the first tile end
    for f in (tg.BY_NODE_WIN - 1, tg.BY_NODE_WIN):
        (n, src, dst), c = tg.star_behind(f)  # asserts that exactly f nodes outrank the centre
        assert tg.walk_slots(n, src, dst).sum() > 0
