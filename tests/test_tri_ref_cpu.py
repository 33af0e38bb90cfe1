"""The reference of the sorted triangle build's device tests (tests/tri_ref.py), pinned on the CPU: both forms
of the plain restatement equal the C enumeration (oracle/rmat.c orc_triangle_enumerate) on random multigraphs
and the C closed form on the hand-built graphs, with and without the dropped relationships and the node
filter; and the builders and placements deliver the shapes they claim.  The shape checks are conditions on the
inputs: they hold or the test fails."""
import numpy as np
import pytest

import tri_ref as tr
from tri_ref import W24


def _compact(c):
    """a Case's kept relationships over compacted ids, as the oracle takes them: (n, src, dst) from the tables
    alone (window, node ids, Long ids) -- not from the core indices the restatement works on"""
    ids = np.sort(c.node_ids)
    in_win = (c.src >= c.lo) & (c.src < c.lo + c.n) & (c.dst >= c.lo) & (c.dst < c.lo + c.n)
    s, d = c.src[in_win], c.dst[in_win]
    ps, pd = np.searchsorted(ids, s), np.searchsorted(ids, d)
    ps, pd = np.minimum(ps, len(ids) - 1), np.minimum(pd, len(ids) - 1)
    keep = (ids[ps] == s) & (ids[pd] == d)
    return len(ids), ps[keep].astype(np.int64), pd[keep].astype(np.int64)


@pytest.mark.parametrize("seed", range(10))
def test_restatements_equal_enumeration(seed):
    from oracle import cpu
    g = tr.random_multigraph(seed)
    want = cpu.triangle_enumerate(g.k, g.src, g.dst)
    assert tr.dense_count(g.k, g.src, g.dst)[0] == want
    assert tr.sparse_count(g.k, g.src, g.dst)[0] == want
    assert tr.dense_count(g.k, g.src, g.dst)[1] == tr.sparse_count(g.k, g.src, g.dst)[1]
    # with a node filter, both against the enumeration of the kept relationships
    ok = np.random.default_rng(1000 + seed).random(g.k) < 0.7
    keep = ok[g.src] & ok[g.dst]
    want = cpu.triangle_enumerate(g.k, g.src[keep], g.dst[keep])
    assert tr.dense_count(g.k, g.src, g.dst, ok)[0] == want
    assert tr.sparse_count(g.k, g.src, g.dst, ok)[0] == want


def test_random_multigraphs_have_loops_and_triangles():
    gs = [tr.random_multigraph(seed) for seed in range(8)]
    assert all(3 <= g.k < 60 and len(g.src) < 600 for g in gs)
    assert sum(bool((g.src == g.dst).any()) for g in gs) >= 6
    assert sum(tr.dense_count(g.k, g.src, g.dst)[0] > 0 for g in gs) >= 6


@pytest.mark.parametrize("dropped", [False, True], ids=["plain", "dropped"])
@pytest.mark.parametrize("graph", ["runs", "all_exceptions", "one_exception", "hub"])
def test_restatements_equal_closed_form(graph, dropped):
    """on the tables the device sees (edge24 / last_far placement), compacted by the node table"""
    from oracle import cpu
    c = tr.case(graph, "last_far" if graph == "hub" else "edge24", dropped)
    n, s, d = _compact(c)
    want = cpu.triangle_closed_form(n, s, d)
    assert want > 0
    g = tr.BUILDERS[graph]()
    ok = tr.node_filter(g.k) if dropped else None
    sparse = tr.sparse_count(g.k, g.src, g.dst, ok)
    assert sparse[0] == want
    if graph != "hub":  # (the dense form is for a few thousand nodes at the most)
        assert tr.dense_count(g.k, g.src, g.dst, ok) == sparse
        assert tr.expected_of(c) == sparse
    assert tr.expected(graph, dropped) == sparse
    # the pairs, from the compacted tables
    assert sparse[1] == len({(min(a, b), max(a, b)) for a, b in zip(s.tolist(), d.tolist()) if a != b})


def test_dense_reference():
    """complete loop-free digraph: every ordered triple of distinct nodes is one binding"""
    g = tr.dense()
    assert len(g.src) == tr.DENSE_K * (tr.DENSE_K - 1) and not (g.src == g.dst).any()
    assert len(set(zip(g.src.tolist(), g.dst.tolist()))) == len(g.src)
    k = tr.DENSE_K
    assert tr.expected("dense") == (k * (k - 1) * (k - 2), k * (k - 1) // 2)
    assert k - 1 > 2048  # one LDS chunk of out-list entries


def test_trivial_inputs():
    from oracle import cpu
    g = tr.no_relationships()
    assert len(g.src) == 0 and tr.dense_count(g.k, g.src, g.dst) == (0, 0)
    g = tr.loops_only()
    assert (g.src == g.dst).all()
    assert sorted(np.bincount(g.src)[[u for u, _ in tr.LOOPS_ONLY]].tolist()) == [1, 2, 3, 40]
    want = sum(s * (s - 1) * (s - 2) for _, s in tr.LOOPS_ONLY)
    assert want == 6 + 40 * 39 * 38
    assert tr.dense_count(g.k, g.src, g.dst) == (want, 0) == tr.sparse_count(g.k, g.src, g.dst)
    assert cpu.triangle_enumerate(g.k, g.src, g.dst) == want
    g, ok = tr.all_dropped()
    assert len(g.src) == 400 and 0 < ok.sum() < g.k and (g.src == g.dst).any()
    assert not (ok[g.src] & ok[g.dst]).any()
    assert tr.dense_count(g.k, g.src, g.dst)[0] > 0  # there would be bindings without the filter
    assert tr.dense_count(g.k, g.src, g.dst, ok) == (0, 0) == tr.sparse_count(g.k, g.src, g.dst, ok)


def _run_table(g):
    """{(lower, upper): (relationships lower -> upper, upper -> lower)} of a graph's non-loop relationships"""
    t = {}
    for a, b in zip(g.src.tolist(), g.dst.tolist()):
        if a != b:
            up, down = t.get((min(a, b), max(a, b)), (0, 0))
            t[(min(a, b), max(a, b))] = (up + (a < b), down + (a > b))
    return t


def test_runs_shape():
    g = tr.runs()
    t = _run_table(g)
    assert g.k == 48 and 5000 < len(g.src) < 7000
    assert sorted(t) == tr.runs_pairs() and 250 < len(t) < 430  # density about 0.3 of 1128 pairs
    spec = tr.runs_spec()
    assert [(i, j) for i, j, _, _ in spec] == sorted(t)[:45]  # the first pairs in (lower, upper) key order
    got = [t[(i, j)] for i, j, _, _ in spec]
    want = []
    for L in tr.RUN_LENGTHS:
        want += [(L, 0), (0, L), ((L + 1) // 2, L // 2)]
    assert got == want
    assert tr.RUN_LENGTHS == (1, 2, 14, 15, 16, 31, 32, 33, 63, 64, 65, 255, 256, 257, 600)
    # every other pair: one relationship, or one each way for about one in ten
    rest = [t[p] for p in sorted(t)[45:]]
    assert set(rest) == {(1, 0), (0, 1), (1, 1)}
    assert 0.03 < rest.count((1, 1)) / len(rest) < 0.25 and rest.count((1, 0)) > 50 and rest.count((0, 1)) > 50
    loops = np.bincount(g.src[g.src == g.dst], minlength=g.k)
    assert [int(loops[v]) for v, _ in tr.RUNS_LOOPS] == [1, 2, 3, 1, 5, 40] and loops.sum() == 52
    # shuffled: the relationships of the longest run are not contiguous
    i, j, _, _ = spec[-1]
    at = np.nonzero((np.minimum(g.src, g.dst) == i) & (np.maximum(g.src, g.dst) == j))[0]
    assert len(at) == 600 and at.max() - at.min() > 3000
    # the node filter leaves a run of every length
    ok = tr.node_filter(g.k)
    assert {sum(t[(i, j)]) for i, j, _, _ in spec if ok[i] and ok[j]} == set(tr.RUN_LENGTHS)
    assert any(not (ok[i] and ok[j]) for i, j, _, _ in spec)


def test_exception_shapes():
    g = tr.all_exceptions()
    t = _run_table(g)
    assert g.k == 70 and len(t) == 2415 and all(up >= 15 and down >= 15 for up, down in t.values())
    assert len(t) > 4 * 64 * 4  # more than one pass of a 256-lane block's four waves at four edges a lane
    g = tr.one_exception()
    t = _run_table(g)
    assert len(t) == 2415
    sat = [p for p in sorted(t) if max(t[p]) >= 15]
    assert sat == [sorted(t)[-1]] == [(68, 69)] and t[(68, 69)] == (15, 15)
    assert all(v == (1, 1) for p, v in t.items() if p != (68, 69))
    assert tr.node_filter(70)[[68, 69]].all()  # the exception survives the node filter


def test_hub_shape():
    g = tr.hub()
    deg = np.bincount(g.src, minlength=g.k) + np.bincount(g.dst, minlength=g.k)
    assert g.k == 70_001 and deg[0] >= 65_536 and deg[1:].max() <= 4
    into = np.sort(g.dst[g.src == 0])
    assert (into == np.arange(1, g.k)).all()  # an in-list of 70,000 at whichever end the hub's edges point to
    back = np.sort(g.src[(g.dst == 0)])
    assert (back == np.arange(1, g.k)[::13]).all()
    assert tr.expected("hub")[0] > 0 and tr.expected("hub", True)[0] > 0
    assert tr.node_filter(g.k)[0]


@pytest.mark.parametrize("k", [48, 70])
def test_placements(k):
    p = tr.place("low", k)
    assert (p.lo, p.n) == (0, k) and (p.rel == np.arange(k)).all()
    p = tr.place("edge24", k)
    assert (p.lo, p.n) == (0, W24) and p.rel[[0, 1, -2, -1]].tolist() == [0, 1, W24 - 2, W24 - 1]
    w = tr.place("wide", k)
    assert (w.lo, w.n) == (0, W24 + 1) and w.rel[[0, -2, -1]].tolist() == [0, W24 - 1, W24]
    f = tr.place("wide_offset", k)
    assert (f.lo, f.n) == ((1 << 40) + 12345, W24 + 1) and (f.rel == w.rel).all()
    q = tr.place("last_far", k)
    assert (q.lo, q.n) == (0, W24 + 1) and q.rel.tolist() == list(range(k - 1)) + [W24]
    for name in tr.PLACEMENTS:
        p = tr.place(name, k)
        assert len(p.rel) == k and (np.diff(p.rel) > 0).all() and p.rel[0] >= 0 and p.rel[-1] < p.n
    # the key layouts' id widths: 24 bits up to 2^24 ids, 25 from 2^24 + 1 (k_tri.hip bits_for)
    assert (W24 - 1).bit_length() == 24 and W24.bit_length() == 25
    # the seeded ids of edge24 fill the high digits: an id in every quarter of the window
    assert len(set((tr.place("edge24", k).rel >> 22).tolist())) == 4


def test_big_placements():
    for k in (tr.HUB_K, tr.DENSE_K):
        p = tr.place("low", k)
        assert (p.lo, p.n) == (0, k)
        q = tr.place("last_far", k)
        assert q.n == W24 + 1 and q.rel[-1] == W24 and (q.rel[:-1] == np.arange(k - 1)).all()


CASES = [(g, p) for g in ("runs", "all_exceptions", "one_exception") for p in ("low", "edge24", "wide", "wide_offset")]
CASES += [("hub", "low"), ("hub", "last_far")]


@pytest.mark.parametrize("graph,placement", CASES)
def test_dropped(graph, placement):
    """at least one relationship dropped for each reason; the filter removes one core node in five; the
    plain case is the same graph with every node and none of the extra relationships"""
    c, plain = tr.case(graph, placement, True), tr.case(graph, placement)
    g = tr.BUILDERS[graph]()
    lo, hi = c.lo, c.lo + c.n
    assert len(plain.src) == len(g.src) and len(c.src) == len(g.src) + tr.N_DROPPED
    assert len(plain.node_ids) == g.k and plain.core_ok.all()
    assert 0.15 < 1 - len(c.node_ids) / g.k <= 0.2
    nodes = set(c.node_ids.tolist())
    assert all(lo <= v < hi for v in nodes) and len(nodes) == len(c.node_ids)
    below = (c.src == lo - 1) | (c.dst == lo - 1)
    above = (c.src == hi) | (c.dst == hi)
    inside = (c.src >= lo) & (c.src < hi) & (c.dst >= lo) & (c.dst < hi)
    no_node = inside & ~(np.isin(c.src, c.node_ids) & np.isin(c.dst, c.node_ids))
    assert below.sum() >= 60 and above.sum() >= 60 and no_node.sum() >= 60
    assert (c.src.min() == lo - 1 or c.dst.min() == lo - 1) and max(c.src.max(), c.dst.max()) == hi
    # the extra relationships are mixed into the row order, and none of them is kept
    extra = below | above
    assert np.nonzero(extra)[0].min() < len(c.src) // 4 and np.nonzero(extra)[0].max() > 3 * len(c.src) // 4
    kept = inside & ~no_node
    assert kept.sum() == (c.core_ok[g.src] & c.core_ok[g.dst]).sum() > 0
    assert kept.sum() < len(g.src)  # the filter drops relationships of the graph itself
    if placement != "low":  # an in-window id that is no core node at all
        core = set((lo + tr.place(placement, g.k).rel).tolist())
        ends = set(c.src[inside].tolist()) | set(c.dst[inside].tolist())
        assert ends - core
