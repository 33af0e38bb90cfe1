"""Without a GPU: the numpy reference of the undirected Expand counts (tests/und_ref.py) against binding enumeration
(oracle/rmat.c orc_two_hop_undirected_enumerate, pinned to oracle/enumerate.py in tests/test_oracle_pins.py) and a
brute-force loop, and every graph of tests/test_gpu_undirected_edges.py against the C closed form
(oracle/closed.c orc_two_hop_undirected_closed_form) with the preconditions it states."""
import numpy as np
import pytest

import und_ref as ur
from oracle import cpu


def _multigraph(seed):
    """5 to 40 nodes, self-loops, parallel and reciprocal pairs, three independent filters"""
    rng = np.random.default_rng(700 + seed)
    n = int(rng.integers(5, 41))
    m = int(rng.integers(1, (4 if seed % 2 else 1) * n + 1))  # even seeds sparse: many middles with one arc
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    loops = rng.random(m) < 0.15
    dst[loops] = src[loops]
    k = m // 4
    src = np.concatenate([src, src[:k], dst[k:2 * k]]).astype(np.int64)  # parallel copies, then reciprocal ones
    dst = np.concatenate([dst, dst[:k], src[k:2 * k]]).astype(np.int64)
    p = float(rng.choice([0.4, 0.7, 0.9]))
    a, b, c = (rng.random(n) < p for _ in range(3))
    return n, src, dst, a, b, c


def _u8(n, m):
    return np.ones(n, np.uint8) if m is None else np.ascontiguousarray(m, dtype=np.uint8)


@pytest.mark.parametrize("seed", range(30))
def test_two_hop_equals_enumeration(seed):
    n, src, dst, a, b, c = _multigraph(seed)
    want = cpu.two_hop_undirected_enumerate(n, src, dst, _u8(n, a), _u8(n, b), _u8(n, c))
    assert ur.two_hop(n, src, dst, a, b, c) == want
    if seed % 5 == 0:  # and with filters that cover the domain
        assert ur.two_hop(n, src, dst) == cpu.two_hop_undirected_enumerate(n, src, dst)
    loose = ur.two_hop(n, src, dst, a, b, c, exclude=False)
    assert loose[0] == want[0] and loose[1] >= want[1] and loose[2] >= want[2]


def test_multigraphs_have_every_feature():
    """taken together: loops, parallel and reciprocal pairs, middles with K = 0, 1, 2, and answers the exclusion
    decides"""
    seen, decided, loops, parallel, reciprocal = set(), 0, 0, 0, 0
    for seed in range(30):
        n, src, dst, a, b, c = _multigraph(seed)
        loops += int((src == dst).any())
        K, _ = ur.reach_state(n, src, dst, a, b)
        seen |= set(np.minimum(K, 2).tolist())
        decided += ur.two_hop(n, src, dst, a, b, c, exclude=False)[1:] != ur.two_hop(n, src, dst, a, b, c)[1:]
        key = set(zip(src.tolist(), dst.tolist()))
        parallel += int(len(key) < len(src))
        reciprocal += int(any(s != t and (t, s) in key for s, t in key))
    assert seen == {0, 1, 2} and decided >= 10 and loops >= 20 and parallel >= 20 and reciprocal >= 20


@pytest.mark.parametrize("seed", range(30))
def test_one_hop_equals_brute_force(seed):
    n, src, dst, a, b, _ = _multigraph(seed)
    rows, ends, starts = 0, set(), set()
    for s, t in zip(src.tolist(), dst.tolist()):
        for x, y in ([(s, t)] if s == t else [(s, t), (t, s)]):
            if a[x] and b[y]:
                rows += 1
                ends.add(y)
                starts.add(x)
    assert ur.one_hop(n, src, dst, a, b) == (rows, len(ends), len(starts))


@pytest.mark.parametrize("seed", range(0, 30, 3))
def test_compact_leaves_the_answers_unchanged(seed):
    n, src, dst, a, b, c = _multigraph(seed)
    big = 1000 * n + 7  # the same graph spread over a larger domain, with relationships that leave it
    up = lambda v: v * 1000 + 3
    s2 = np.concatenate([up(src), [-1, big, 5]])
    t2 = np.concatenate([up(dst), [4, 6, big + 9]])
    sets = [up(np.nonzero(m)[0]) for m in (a, b, c)]
    k, cs, ct, ms = ur.compact(big, s2, t2, sets, id_sets=True)
    assert k == len(np.unique(np.concatenate([src, dst]))) and len(cs) == len(src)
    assert ur.two_hop(k, cs, ct, *ms) == ur.two_hop(n, src, dst, a, b, c)
    assert ur.one_hop(k, cs, ct, ms[0], ms[1]) == ur.one_hop(n, src, dst, a, b)
    k2, cs2, ct2, ms2 = ur.compact(n, src, dst, (a, b, c))  # masks gathered
    assert ur.two_hop(k2, cs2, ct2, *ms2) == ur.two_hop(n, src, dst, a, b, c)
    assert ur.compact(n, src, dst, (None, b, None))[3][0] is None


@pytest.mark.parametrize("name", list(ur.BUILDERS) + list(ur.DEGENERATE))
def test_graph_builders(name):
    """every graph of the GPU file: its preconditions, and the reference against the C closed form"""
    cs = ur.case(name)
    ur.check_preconditions(cs)
    n, s, t, (a, b, c) = cs.dense()
    rows, dc, da = cs.two_hop()
    assert (rows, dc) == cpu.two_hop_undirected_closed_form(n, s, t, _u8(n, a), _u8(n, b), _u8(n, c))
    assert (rows, da) == cpu.two_hop_undirected_closed_form(n, s, t, _u8(n, c), _u8(n, b), _u8(n, a))
    arcs, ends, starts = cs.one_hop()
    assert ends <= arcs and starts <= arcs and (arcs == 0) == (ends == 0)
    for which in range(3):  # the ids a bitmap is built from
        ids = cs.ok_ids(which)
        assert len(ids) == len(np.unique(ids)) and (len(ids) == 0 or (ids.min() >= 0 and ids.max() < cs.n))


def test_issue_figures_hold_for_the_three_slice_graph():
    """the kind of graph the issue describes: dropping the c != x(b) test moves the distinct count by a wide margin"""
    cs = ur.case("three_slices")
    plain, loose = cs.two_hop(), cs.two_hop(exclude=False)
    assert loose[1] > plain[1] + 10_000 and loose[2] > plain[2] + 10_000


def test_walk_order_helpers():
    cnt = np.array([[1, 2], [3, 4]])  # cnt[target slice, source slice]
    # group 0: forwards (0,0) (0,1), backwards (0,0) (1,0); group 1: forwards (1,0) (1,1), backwards (0,1) (1,1)
    assert ur.item_offsets(cnt).tolist() == [0, 1, 3, 4, 7, 10, 14, 16, 20]
    S = ur.SLICE
    assert ur.item_of_arc(2, 5, S + 1, False) == 4 and ur.item_of_arc(2, S + 1, 5, True) == 3
    assert ur.min_distance(ur.item_offsets(cnt), 0, 3) == 4 - 0 and ur.min_distance(ur.item_offsets(cnt), 2, 2) == 0


def test_wrapper_is_declared():
    from capsmi import _lib, graph
    assert hasattr(_lib.load(), "capsmi_undirected_count") and callable(graph.undirected_count)
