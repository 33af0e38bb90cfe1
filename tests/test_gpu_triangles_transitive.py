"""The transitive triangle (csrc/k_tri_nodes.hip, routes "triangle_transitive" and "triangle_transitive_grouped"):
  MATCH (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a) RETURN count(*)
  MATCH (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a) RETURN id(a), count(*)     (or id(b), or id(c))
through the direct entry points on both trigraph builds and through the planner, against the enumeration and the
closed form of tests/tri_trans_ref.py (pinned against each other in tests/test_tri_trans_ref_cpu.py).  Every row is
compared, with its id; counts are integers and must match exactly."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import tri_trans_ref as tt
from golden_util import same_rows

pytestmark = pytest.mark.gpu

BUILDS = ["direct", "sorted"]
ROLE_NAMES = {tt.SOURCE: "source", tt.MIDDLE: "middle", tt.SINK: "sink"}


def _build(knobs, session, build):
    if build == "sorted":
        knobs(session, CAPSMI_TRI_BUILD="sorted")


def _rows(t):
    ids, cnt = t.column("id").values, t.column("n").values
    assert t.column("id").valid is None and t.column("n").valid is None  # two non-nullable Long columns
    return [{"id": int(i), "n": int(c)} for i, c in zip(ids, cnt)]


def _tables(session, n, src, dst, mask=None, lo=0, ids=None):
    from capsmi import ColumnData, I64, graph
    rels = session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)), ColumnData("source", I64, src),
                          ColumnData("target", I64, dst)])
    if ids is None:
        ids = lo + (np.arange(n) if mask is None else np.nonzero(mask)[0])
    nodes = session.table([ColumnData("id", I64, np.asarray(ids, dtype=np.int64))])
    return rels, graph.NodeBitmap(session, lo, lo + n).add_scan(nodes)


def _all(session, n, src, dst, mask=None, lo=0, ids=None, handle=False):
    """(count(*), rows per role) of the entry points over the window [lo, lo + n)"""
    from capsmi import graph
    rels, ok = _tables(session, n, src, dst, mask, lo, ids)
    if handle:
        g = graph.TriGraph(session, [rels], ok)
        try:
            return g.count_transitive(), [_rows(g.count_transitive_by_node(r, "id", "n")) for r in tt.ROLES]
        finally:
            g.release()
    return (graph.triangle_count_transitive(session, [rels], ok),
            [_rows(graph.triangle_count_transitive_by_node(session, [rels], ok, r, "id", "n")) for r in tt.ROLES])


def _check(got, want, ids=None):
    """got = _all(...); want = the 3 x n counts.  Every role's rows, the count, and the count against each role's
    sum."""
    total, rows = got
    for r in tt.ROLES:
        assert same_rows(rows[r], tt.rows_of(want[r], ids)), f"role {ROLE_NAMES[r]}"
        assert total == sum(x["n"] for x in rows[r]), f"count(*) against the sum over the {ROLE_NAMES[r]}s"
    assert total == int(want[0].sum())


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("seed", range(8))
def test_random_multigraphs(session, knobs, seed, build):
    _build(knobs, session, build)
    n, src, dst = tt.random_multigraph(seed)
    want = tt.per_node_enumerate_all(n, src, dst)
    assert want.tolist() == tt.per_node_dense_all(n, src, dst).tolist()
    _check(_all(session, n, src, dst, handle=seed % 2 == 1), want)


# ---- one triangle, six different multiplicities, every degree order ----------------------------------------------

PRIMES = tt.PRIMES


@functools.lru_cache(maxsize=None)
def _prime_triangle(pendants):
    """the prime triangle of tests/tri_grouped_ref.py with its expected 3 x n counts"""
    n, src, dst = tt.prime_triangle(pendants)
    return n, src, dst, tt.per_node_enumerate_all(n, src, dst)


def test_prime_triangle_reaches_every_degree_order():
    orders = set()
    for pend in itertools.permutations((1, 2, 3)):
        n, src, dst, _ = _prime_triangle(pend)
        rid = tt.degree_order(n, src, dst)
        assert sorted(rid[:3].tolist()) == [0, 1, 2]  # the corners outrank every leaf
        orders.add(tuple(rid[:3].tolist()))
    assert len(orders) == 6


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("pend", list(itertools.permutations((1, 2, 3))))
def test_prime_triangle_under_every_degree_order(session, knobs, pend, build):
    """a swapped payload half, or a role tied to the orientation instead of the direction, shows here: the three
    corners' weights are 2*11*12, 3*5*24, 13*7*5 (source), 3*11*5 + 13*2*7, ... -- no two alike"""
    _build(knobs, session, build)
    n, src, dst, want = _prime_triangle(pend)
    tri = tt.per_node_dense_all(3, *[np.repeat([k[i] for k in PRIMES], list(PRIMES.values())) for i in (0, 1)])
    assert len(set(tri.flatten().tolist())) == 9
    _check(_all(session, n, src, dst), want)


# ---- pair and self terms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", BUILDS)
def test_one_directional_pairs_beside_loops(session, knobs, build):
    """m (m - 1) s terms of pairs with relationships in one direction only (the cyclic pair pass skips those):
    0 has two loops, 3 one; 0 -> 1 twice, 2 -> 0 three times, 1 -> 3 three times, 3 -> 4 twice, 4 <-> 5 without a
    loop (no term), and 5 -> 0 once (m - 1 = 0)"""
    _build(knobs, session, build)
    src = np.array([0, 0, 3, 0, 0, 2, 2, 2, 1, 1, 1, 3, 3, 4, 5, 5], dtype=np.int64)
    dst = np.array([0, 0, 3, 1, 1, 0, 0, 0, 3, 3, 3, 4, 4, 5, 4, 0], dtype=np.int64)
    want = tt.per_node_enumerate_all(6, src, dst)
    assert want.tolist() == tt.per_node_dense_all(6, src, dst).tolist()
    # a = b = 0: 2 * 2 * 1; b = c = 0: 3 * 2 * 2; b = c = 3: 3 * 2 * 1; a = b = 3: 1 * 2 * 1
    assert int(want[0].sum()) == 4 + 12 + 6 + 2
    _check(_all(session, 6, src, dst), want)
    _check(_all(session, 6, src, dst, handle=True), want)


@pytest.mark.parametrize("build", BUILDS)
def test_loops_only(session, knobs, build):
    """s = 0, 1, 2, 3, 4 self-loops and nothing else: s (s - 1) (s - 2) for every role"""
    _build(knobs, session, build)
    v = np.repeat(np.arange(5, dtype=np.int64), np.arange(5))
    want = np.array([[0, 0, 0, 6, 24]] * 3, dtype=np.int64)
    assert want.tolist() == tt.per_node_enumerate_all(5, v, v).tolist()
    _check(_all(session, 5, v, v), want)


# ---- the walk's tiles --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _flipped(name, arg, seed):
    """a builder's graph with every relationship reversed with probability 1/2 (fixed seed): triangles of both
    kinds, and all three roles at corners of every degree rank; (n, src, dst, expected 3 x n)"""
    n, src, dst = getattr(tt, name)(arg)
    flip = np.random.default_rng(seed).random(len(src)) < 0.5
    s, d = np.where(flip, dst, src), np.where(flip, src, dst)
    want = tt.per_node_enumerate_all(n, s, d)
    for r in tt.ROLES:
        assert np.count_nonzero(want[r]) > 0
    return n, s, d, want


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("t", [tt.TILE_SLOTS - 1, tt.TILE_SLOTS, tt.TILE_SLOTS + 1])
def test_one_slot_rows_at_a_tile_end(session, knobs, t, build):
    """t disjoint triangles with random directions: t rows of one slot each, three in four transitive"""
    _build(knobs, session, build)
    n, src, dst, want = _flipped("disjoint_triangles", t, 502)
    assert int(tt.walk_slots(n, src, dst).sum()) == t
    _check(_all(session, n, src, dst), want)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("slots", [2 * tt.TILE_SLOTS, 2 * tt.TILE_SLOTS + 1])
def test_rows_across_tile_ends(session, knobs, slots, build):
    """exactly two tiles / two tiles and one slot; a row of several slots straddles the first tile end"""
    _build(knobs, session, build)
    n, src, dst = tt.clique_and_triangles(slots)
    want = _clique_want(slots)
    _check(_all(session, n, src, dst), want)


@functools.lru_cache(maxsize=None)
def _clique_want(slots):
    return tt.per_node_enumerate_all(*tt.clique_and_triangles(slots))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fillers", [tt.BY_NODE_WIN - 1, tt.BY_NODE_WIN])
def test_hub_at_the_window_edge(session, knobs, fillers, build):
    """the star's centre is the last id of the privatised window / the first id outside it: with the star's
    directions as built (cycles through the centre: its pair terms only), and with one relationship of each of
    its three triangles reversed so that the centre is the source of the first, the middle of the second and the
    sink of the third"""
    _build(knobs, session, build)
    (n, src, dst), c = tt.star_behind(fillers)
    assert c == 0 and tt.degree_order(n, src, dst)[c] == fillers
    want = tt.per_node_enumerate_all(n, src, dst)
    assert want[:, c].sum() > 0
    _check(_all(session, n, src, dst), want)
    # the triangles are c -> x -> y -> c with (x, y) = (1, 2), (3, 4), (5, 6)
    flip = ((src == 2) & (dst == c)) | ((src == 3) & (dst == 4)) | ((src == c) & (dst == 5))
    assert int(flip.sum()) == 3
    s, d = np.where(flip, dst, src), np.where(flip, src, dst)
    assert tt.degree_order(n, s, d)[c] == fillers
    want = tt.per_node_enumerate_all(n, s, d)
    assert all(want[r][c] > 0 for r in tt.ROLES)
    _check(_all(session, n, s, d), want)


@pytest.mark.parametrize("build", BUILDS)
def test_counts_above_2_32_and_exception_payloads(session, knobs, build):
    """multiplicity 1700 on all six directed edges (every coded field an exception: payloads from ov) and three
    self-loops on one corner; expected from the closed form in Python ints, which must fit int64"""
    _build(knobs, session, build)
    n, src, dst = tt.heavy_triangle()
    exact = tt.per_node_dense_all(n, src, dst, dtype=object)
    assert all(2 ** 32 < int(x) < 2 ** 63 for x in exact.flatten()) and int(exact[0].sum()) < 2 ** 63
    want = exact.astype(np.int64)
    m = 1700
    assert int(want[tt.SOURCE][0]) == 2 * m ** 3 + m * (m - 1) * 3  # 0 has no loop: its b = c = 2 term only
    _check(_all(session, n, src, dst), want)
    _check(_all(session, n, src, dst, handle=True), want)


COMPLETE_N = 300


@functools.lru_cache(maxsize=None)
def _complete():
    a, b = np.nonzero(~np.eye(COMPLETE_N, dtype=bool))
    perm = np.random.default_rng(504).permutation(len(a))
    return a[perm].astype(np.int64), b[perm].astype(np.int64)


@pytest.mark.parametrize("build", BUILDS)
def test_complete_digraph(session, knobs, build):
    """K_300, every ordered pair once: every role (n-1)(n-2) per node, n(n-1)(n-2) in all.  The walk has C(300, 3) =
    4,455,100 slots in 2176 tiles of 2048, above tile_grid's cap of 8 workgroups on each of 256 CUs = 2048: the
    block-stride loop takes a second tile in 128 workgroups.  Out-degrees reach 299, ids lie on both sides of the
    window's end."""
    _build(knobs, session, build)
    n = COMPLETE_N
    src, dst = _complete()
    slots = n * (n - 1) * (n - 2) // 6
    assert -(-slots // tt.TILE_SLOTS) > tt.TILE_GRID_CAP
    want = np.full((3, n), (n - 1) * (n - 2), dtype=np.int64)
    got = _all(session, n, src, dst)
    assert got[0] == n * (n - 1) * (n - 2)
    _check(got, want)


def test_complete_digraph_slots():
    """the slot count the test above relies on, from the mirror of the walk's slots"""
    src, dst = _complete()
    assert int(tt.walk_slots(COMPLETE_N, src, dst).sum()) == COMPLETE_N * (COMPLETE_N - 1) * (COMPLETE_N - 2) // 6


# ---- node filter, window, no rows --------------------------------------------------------------------------------

@pytest.mark.parametrize("build", BUILDS)
def test_node_filter_and_window(session, knobs, build):
    """about 70 % of 200 nodes kept (corners of many triangles go), in a window that starts at 5000, and 300
    relationships with an end below or above the window"""
    _build(knobs, session, build)
    rng = np.random.default_rng(42)
    n, m, lo = 200, 4000, 5000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[:300] = dst[:300]
    mask = rng.random(n) < 0.7
    keep = mask[src] & mask[dst]
    want = tt.per_node_dense_all(n, src[keep], dst[keep])
    full = tt.per_node_dense_all(n, src, dst)
    assert 0 < want[0].sum() < full[0].sum()
    inside = rng.integers(0, n, 300) + lo
    outside = np.where(rng.random(300) < 0.5, lo - 1 - rng.integers(0, 50, 300), lo + n + rng.integers(0, 50, 300))
    swap = rng.random(300) < 0.5
    xs = np.concatenate([src + lo, np.where(swap, inside, outside)])
    xd = np.concatenate([dst + lo, np.where(swap, outside, inside)])
    _check(_all(session, n, xs, xd, mask, lo=lo), want, lo + np.arange(n))
    _check(_all(session, n, xs, xd, mask, lo=lo, handle=True), want, lo + np.arange(n))


@pytest.mark.parametrize("build", BUILDS)
def test_no_rows(session, knobs, build):
    """no relationships; relationships, a lone loop and a reciprocal pair, but no binding"""
    _build(knobs, session, build)
    e = np.zeros(0, dtype=np.int64)
    assert _all(session, 48, e, e) == (0, [[], [], []])
    src = np.array([0, 1, 2, 3, 5, 6, 7], dtype=np.int64)  # a path, a directed 3-cycle's two edges, 2-cycle, a loop
    dst = np.array([1, 2, 3, 4, 6, 5, 7], dtype=np.int64)
    assert tt.per_node_enumerate_all(9, src, dst).sum() == 0
    assert _all(session, 9, src, dst) == (0, [[], [], []])
    cyc = np.array([0, 1, 2], dtype=np.int64)  # a directed cycle is no transitive triangle
    assert _all(session, 3, cyc, np.roll(cyc, -1)) == (0, [[], [], []])


# ---- errors ------------------------------------------------------------------------------------------------------

def test_null_arguments(session):
    from capsmi import _lib
    out, v = ctypes.c_void_p(), ctypes.c_int64()
    rels, ok = _tables(session, 3, np.array([0, 1, 0], dtype=np.int64), np.array([1, 2, 2], dtype=np.int64))
    arr = (ctypes.c_void_p * 1)(rels.handle)
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_trigraph_count_transitive", session.handle, None, ctypes.byref(v))
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_trigraph_count_transitive_by_node", session.handle, None, 0, b"id", b"n", ctypes.byref(out))
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_transitive", session.handle, 1, arr, b"source", b"target", None, ctypes.byref(v))
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_transitive_by_node", session.handle, 1, arr, b"source", b"target", ok.handle, 0,
                  b"id", b"n", None)
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_transitive_by_node", session.handle, 1, arr, b"source", b"target", ok.handle, 0,
                  None, b"n", ctypes.byref(out))


@pytest.mark.parametrize("role", [3, -1])
def test_role_out_of_range(session, role):
    from capsmi import _lib, graph
    rels, ok = _tables(session, 3, np.array([0, 1, 0], dtype=np.int64), np.array([1, 2, 2], dtype=np.int64))
    with pytest.raises(_lib.IllegalArgumentException):
        graph.triangle_count_transitive_by_node(session, [rels], ok, role, "id", "n")
    g = graph.TriGraph(session, [rels], ok)
    try:
        with pytest.raises(_lib.IllegalArgumentException):
            g.count_transitive_by_node(role, "id", "n")
        assert g.count_transitive() == 1
    finally:
        g.release()


# ---- the planner routes ------------------------------------------------------------------------------------------

LO = 1000
MIXED = [d for d in itertools.product("><", repeat=3) if len(set(d)) == 2]
UNIFORM = [(">", ">", ">"), ("<", "<", "<")]


@functools.lru_cache(maxsize=None)
def _labelled():
    """60 nodes from LO on, three in four labelled L and the rest M; 420 relationships of two types, self-loops
    and parallel relationships among them (a few thousand bindings at the most)"""
    rng = np.random.default_rng(78)
    n, m = 60, 420
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[:50] = dst[:50]
    is_l = np.arange(n) % 4 != 3
    types = np.where(rng.random(m) < 0.5, "R", "S")
    return n, src, dst, is_l, types


@pytest.fixture(scope="module")
def labelled(session):
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    n, src, dst, is_l, types = _labelled()
    nodes = []
    for lab, sel in (("L", is_l), ("M", ~is_l)):
        t = session.table([ColumnData("id", I64, LO + np.nonzero(sel)[0].astype(np.int64))]).as_node_table("id")
        nodes.append(EntityTable("node", frozenset({lab}), {}, t, id_col="id"))
    rid = np.arange(len(src), dtype=np.int64) + (1 << 50)
    rels = []
    for ty in ("R", "S"):
        k = types == ty
        t = session.table([ColumnData("id", I64, rid[k]), ColumnData("source", I64, src[k] + LO),
                           ColumnData("target", I64, dst[k] + LO)]).as_rel_table("id", "source", "target")
        rels.append(EntityTable("rel", frozenset({ty}), {}, t, id_col="id", src_col="source", dst_col="target"))
    sg = ScanGraph(session, nodes, rels)
    yield sg
    del sg


def _pattern(dirs, labels=("L", "L", "L"), types="R|S"):
    hop = {">": f"-[:{types}]->", "<": f"<-[:{types}]-"}
    la, lb, lc = [f":{x}" if x else "" for x in labels]
    return f"(a{la}){hop[dirs[0]]}(b{lb}){hop[dirs[1]]}(c{lc}){hop[dirs[2]]}(a)"


def _query(dirs=tt.TRANSITIVE, labels=("L", "L", "L"), items=(("k", ["id", "a"]), ("n", ["count*"]))):
    return {"clauses": [{"match": _pattern(dirs, labels)}], "return": {"items": [[k, spec] for k, spec in items]}}


def _run(session, sg, q, fused=True):
    from capsmi.planner import Planner, result_rows
    session.set_fused(fused)
    try:
        t, outs = Planner(sg).run(q)
        return result_rows(t, outs, session.dictionary)
    finally:
        session.set_fused(True)


ROUTES = ("triangle", "triangle_grouped", "triangle_transitive", "triangle_transitive_grouped", "miss")


def _routes(session):
    return {r: session.route_count(r) for r in ROUTES}


def _rose(session, before):
    """the routes that rose since `before`, with by how much"""
    return {r: v - before[r] for r, v in _routes(session).items() if v != before[r]}


@functools.lru_cache(maxsize=None)
def _want_l():
    """3 x n: the transitive pattern's counts per role among the L nodes"""
    n, src, dst, is_l, _ = _labelled()
    cnt = tt.per_node_enumerate_all(n, src, dst, ok=(is_l, is_l, is_l))
    assert 0 < cnt[0].sum() < 20000
    assert len({tuple(cnt[r].tolist()) for r in tt.ROLES}) == 3  # the roles differ: a wrong role shows
    return cnt


def _k_rows(cnt):
    return [{"k": LO + int(i), "n": int(cnt[i])} for i in np.nonzero(cnt)[0]]


@pytest.mark.parametrize("key", ["a", "b", "c"])
@pytest.mark.parametrize("dirs", MIXED, ids=["".join(d) for d in MIXED])
def test_grouped_routed(session, labelled, dirs, key):
    """every mixed spelling, grouped by each position: routed, equal to the unfused run, to the enumeration of that
    spelling and to the enumeration of the transitive pattern for the role the position has"""
    n, src, dst, is_l, _ = _labelled()
    q = _query(dirs, items=(("k", ["id", key]), ("n", ["count*"])))
    before = _routes(session)
    got = _run(session, labelled, q)
    assert _rose(session, before) == {"triangle_transitive_grouped": 1}
    pos = "abc".index(key)
    want = _k_rows(_want_l()[tt.roles_of(dirs)[pos]])
    assert same_rows(got, want)
    assert same_rows(got, _k_rows(_spelled(dirs)[pos]))
    before = _routes(session)
    unfused = _run(session, labelled, q, fused=False)
    assert set(_rose(session, before)) <= {"miss"}  # no fused route took it
    assert same_rows(got, unfused)


@functools.lru_cache(maxsize=None)
def _spelled(dirs):
    n, src, dst, is_l, _ = _labelled()
    return tt.per_node_enumerate_all(n, src, dst, ok=(is_l, is_l, is_l), dirs=dirs)


@pytest.mark.parametrize("dirs", MIXED, ids=["".join(d) for d in MIXED])
def test_count_routed(session, labelled, dirs):
    before = _routes(session)
    got = _run(session, labelled, _query(dirs, items=(("n", ["count*"]),)))
    assert _rose(session, before) == {"triangle_transitive": 1}
    assert got == [{"n": int(_want_l()[0].sum())}]
    assert got == _run(session, labelled, _query(dirs, items=(("n", ["count*"]),)), fused=False)


@pytest.mark.parametrize("dirs", UNIFORM, ids=["".join(d) for d in UNIFORM])
def test_uniform_spellings_stay_on_the_cyclic_routes(session, labelled, dirs):
    import tri_grouped_ref as tg
    n, src, dst, is_l, _ = _labelled()
    cnt = tg.per_node_enumerate(n, src, dst, ok=(is_l, is_l, is_l))
    assert cnt.sum() > 0
    before = _routes(session)
    got = _run(session, labelled, _query(dirs))
    assert _rose(session, before) == {"triangle_grouped": 1}
    assert same_rows(got, _k_rows(cnt))
    before = _routes(session)
    got = _run(session, labelled, _query(dirs, items=(("n", ["count*"]),)))
    assert _rose(session, before) == {"triangle": 1}
    assert got == [{"n": int(cnt.sum())}]


def _generic(session, sg, q):
    before = _routes(session)
    got = _run(session, sg, q)
    rose = _rose(session, before)
    assert set(rose) == {"miss"} and rose["miss"] >= 1
    return got


def test_different_labels_take_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    cnt = tt.per_node_enumerate_all(n, src, dst, ok=(is_l, ~is_l, is_l))[tt.SOURCE]
    assert cnt.sum() > 0
    got = _generic(session, labelled, _query(labels=("L", "M", "L")))
    assert same_rows(got, _k_rows(cnt))


def test_two_keys_take_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    pairs = {}
    for a, b, _ in tt.bindings(src, dst, (is_l, is_l, is_l)):
        pairs[(a, b)] = pairs.get((a, b), 0) + 1
    got = _generic(session, labelled, _query(items=(("k", ["id", "a"]), ("j", ["id", "b"]), ("n", ["count*"]))))
    assert same_rows(got, [{"k": LO + a, "j": LO + b, "n": c} for (a, b), c in pairs.items()])


def test_count_distinct_takes_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    bs = {}
    for a, b, _ in tt.bindings(src, dst, (is_l, is_l, is_l)):
        bs.setdefault(a, set()).add(b)
    got = _generic(session, labelled, _query(items=(("k", ["id", "a"]), ("n", ["count_distinct", ["id", "b"]]))))
    assert same_rows(got, [{"k": LO + a, "n": len(s)} for a, s in bs.items()])


@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_tagged_ids(session, key):
    """ids carrying a graph tag in the top 10 bits (Tags.scala: id | tag << 54), reached through the graph's
    dense id compaction: routed, and the rows carry the tagged ids"""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    ids, src, dst, tags = tt.tagged_graph()
    retag = np.vectorize(lambda v: tags[int(v)], otypes=[np.int64])
    nodes = session.table([ColumnData("id", I64, retag(ids))]).as_node_table("id")
    rels = session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64) * 3 + (1 << 50)),
                          ColumnData("source", I64, retag(src)), ColumnData("target", I64, retag(dst))]).as_rel_table(
        "id", "source", "target")
    assert session.compact_if_sparse([nodes], [rels])
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    q = {"clauses": [{"match": _pattern(tt.TRANSITIVE, labels=("", "", ""), types="R")}],
         "return": {"items": [["k", ["id", key]], ["n", ["count*"]]]}}
    before = _routes(session)
    got = _run(session, sg, q)
    assert _rose(session, before) == {"triangle_transitive_grouped": 1}
    cnt = _tagged_want()["abc".index(key)]
    assert cnt.sum() > 0
    assert same_rows(got, [{"k": tags[int(ids[i])], "n": int(cnt[i])} for i in np.nonzero(cnt)[0]])


@functools.lru_cache(maxsize=None)
def _tagged_want():
    ids, src, dst, _ = tt.tagged_graph()
    return tt.per_node_dense_all(*tt.relabel(ids, src, dst))
