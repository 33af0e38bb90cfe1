"""The cyclic triangle grouped by its start (csrc/k_tri_nodes.hip, route "triangle_grouped"):
  MATCH (a)-[r1]->(b)-[r2]->(c)-[r3]->(a) RETURN id(a), count(*)
through the direct entry points on both trigraph builds and through the planner, against the plain restatements
of tests/tri_grouped_ref.py (pinned against the C enumeration in tests/test_tri_grouped_ref_cpu.py).  Every row
is compared, with its id; counts are integers and must match exactly."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import tri_grouped_ref as tg
from golden_util import same_rows

pytestmark = pytest.mark.gpu

BUILDS = ["direct", "sorted"]


def _build(knobs, session, build):
    if build == "sorted":
        knobs(session, CAPSMI_TRI_BUILD="sorted")


def _rows(t):
    ids, cnt = t.column("id").values, t.column("n").values
    assert t.column("id").valid is None and t.column("n").valid is None  # two non-nullable Long columns
    return [{"id": int(i), "n": int(c)} for i, c in zip(ids, cnt)]


def _by_node(session, n, src, dst, mask=None, lo=0, ids=None, handle=False):
    """rows of the direct entry point over the window [lo, lo + n)"""
    from capsmi import ColumnData, I64, graph
    rels = session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)), ColumnData("source", I64, src),
                          ColumnData("target", I64, dst)])
    if ids is None:
        ids = lo + (np.arange(n) if mask is None else np.nonzero(mask)[0])
    nodes = session.table([ColumnData("id", I64, np.asarray(ids, dtype=np.int64))])
    ok = graph.NodeBitmap(session, lo, lo + n).add_scan(nodes)
    if handle:
        g = graph.TriGraph(session, [rels], ok)
        try:
            rows = _rows(g.count_by_node("id", "n"))
            assert g.count() == sum(r["n"] for r in rows)  # the ungrouped count of the same handle
            return rows
        finally:
            g.release()
    return _rows(graph.triangle_count_by_node(session, [rels], ok, "id", "n"))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("seed", range(8))
def test_random_multigraphs(session, knobs, seed, build):
    import tri_ref
    _build(knobs, session, build)
    n, src, dst = tri_ref.random_multigraph(seed)
    want = tg.per_node_enumerate(n, src, dst)
    assert want.tolist() == tg.per_node_dense(n, src, dst).tolist()
    assert same_rows(_by_node(session, n, src, dst, handle=seed % 2 == 1), tg.rows_of(want))


# ---- one triangle, six different multiplicities, every degree order ----------------------------------------------

def _cycle_weight(puv, pvw, puw):
    """tri_weight (csrc/tri_code.h) of the payloads (f, b) of u -> v, v -> w, u -> w"""
    return puv[0] * pvw[0] * puw[1] + puw[0] * pvw[1] * puv[1]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("pend", list(itertools.permutations((1, 2, 3))))
def test_prime_triangle_under_every_degree_order(session, knobs, pend, build):
    """The walk hands tri_weight the payloads of u -> v, v -> w and u -> w (u > v > w as degree-order ids), the
    latter two in an order that depends on which list it walked.  Every corner's weight is 2*5*13 + 11*7*3 = 361;
    with u -> w exchanged for u -> v or for v -> w, or the halves of any one payload flipped, it is 347, 349 or 383
    under each of the six orders.  (Exchanging u -> v with v -> w leaves the cyclic weight as it is: that one
    cannot show here; the transitive test catches it.)"""
    _build(knobs, session, build)
    n, src, dst = tg.prime_triangle(pend)
    rid = tg.degree_order(n, src, dst)
    w, v, u = sorted(range(3), key=lambda x: rid[x])
    pay = {(x, y): (tg.PRIMES[x, y], tg.PRIMES[y, x]) for x, y in tg.PRIMES}
    puv, pvw, puw = pay[u, v], pay[v, w], pay[u, w]
    assert _cycle_weight(puv, pvw, puw) == 361
    wrong = [_cycle_weight(puw, pvw, puv), _cycle_weight(puv, puw, pvw), _cycle_weight(puv[::-1], pvw, puw),
             _cycle_weight(puv, pvw[::-1], puw), _cycle_weight(puv, pvw, puw[::-1])]
    assert set(wrong) <= {347, 349, 383}
    want = tg.per_node_enumerate(n, src, dst)
    assert want.tolist() == tg.per_node_dense(n, src, dst).tolist() and want[3:].sum() == 0
    assert same_rows(_by_node(session, n, src, dst), tg.rows_of(want))


# ---- pair and self terms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", BUILDS)
def test_one_directional_pairs_beside_loops(session, knobs, build):
    """the graph of tests/test_gpu_triangles_transitive.py: 0 has two loops, 3 one; 0 -> 1 twice, 2 -> 0 three
    times, 1 -> 3 three times, 3 -> 4 twice, 5 -> 0 once: pairs in one direction beside a loop, which have no term
    in the cycle (the pair pass leaves them on their coded word), and 4 <-> 5 without a loop: no row at all.  With
    1 -> 0 added, {0, 1} is reciprocated beside the loops of 0 and alone contributes: 2 * 1 * (2 * 2 + 0) to 0 and
    2 * 1 * (0 + 2) to 1."""
    _build(knobs, session, build)
    src = np.array([0, 0, 3, 0, 0, 2, 2, 2, 1, 1, 1, 3, 3, 4, 5, 5], dtype=np.int64)
    dst = np.array([0, 0, 3, 1, 1, 0, 0, 0, 3, 3, 3, 4, 4, 5, 4, 0], dtype=np.int64)
    want = tg.per_node_enumerate(6, src, dst)
    assert want.tolist() == tg.per_node_dense(6, src, dst).tolist() == [0] * 6
    assert _by_node(session, 6, src, dst) == []
    assert _by_node(session, 6, src, dst, handle=True) == []
    src, dst = np.append(src, 1), np.append(dst, 0)
    want = tg.per_node_enumerate(6, src, dst)
    assert want.tolist() == tg.per_node_dense(6, src, dst).tolist() == [8, 4, 0, 0, 0, 0]
    assert same_rows(_by_node(session, 6, src, dst), tg.rows_of(want))
    assert same_rows(_by_node(session, 6, src, dst, handle=True), tg.rows_of(want))


@pytest.mark.parametrize("build", BUILDS)
def test_loops_only(session, knobs, build):
    """s = 0, 1, 2, 3, 4 self-loops and nothing else: s (s - 1) (s - 2)"""
    _build(knobs, session, build)
    v = np.repeat(np.arange(5, dtype=np.int64), np.arange(5))
    want = tg.per_node_enumerate(5, v, v)
    assert want.tolist() == tg.per_node_dense(5, v, v).tolist() == [0, 0, 0, 6, 24]
    assert same_rows(_by_node(session, 5, v, v), tg.rows_of(want))


@pytest.mark.parametrize("build", BUILDS)
def test_node_filter_and_window(session, knobs, build):
    """about 70 % of 200 nodes kept, in a window that starts at 5000"""
    _build(knobs, session, build)
    rng = np.random.default_rng(42)
    n, m, lo = 200, 4000, 5000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[:300] = dst[:300]
    mask = rng.random(n) < 0.7
    keep = mask[src] & mask[dst]
    want = tg.per_node_dense(n, src[keep], dst[keep])
    assert same_rows(_by_node(session, n, src + lo, dst + lo, mask, lo=lo), tg.rows_of(want, lo + np.arange(n)))


@pytest.mark.parametrize("build", BUILDS)
def test_no_rows(session, knobs, build):
    """no relationships; relationships, self-loops and reciprocal pairs, but no closed triangle"""
    _build(knobs, session, build)
    e = np.zeros(0, dtype=np.int64)
    assert _by_node(session, 48, e, e) == []
    src = np.array([0, 1, 2, 3, 3, 5, 6, 7, 7], dtype=np.int64)  # a path, a 2-cycle without loops, lone loops
    dst = np.array([1, 2, 3, 4, 5, 3, 6, 7, 7], dtype=np.int64)
    assert tg.per_node_enumerate(9, src, dst).sum() == 0
    assert _by_node(session, 9, src, dst) == []


@pytest.mark.parametrize("build", BUILDS)
def test_counts_above_2_32_and_exception_payloads(session, knobs, build):
    _build(knobs, session, build)
    n, src, dst = tg.heavy_triangle()
    want = tg.heavy_triangle_counts()
    assert want.min() > 2 ** 32
    assert same_rows(_by_node(session, n, src, dst), tg.rows_of(want))
    assert same_rows(_by_node(session, n, src, dst, handle=True), tg.rows_of(want))


@functools.lru_cache(maxsize=None)
def _complete_2200():
    n = 2200
    rng = np.random.default_rng(5)
    M = rng.integers(1, 4, (n, n))
    np.fill_diagonal(M, 0)
    a, b = np.nonzero(M)
    reps = M[a, b]
    src, dst = np.repeat(a, reps).astype(np.int64), np.repeat(b, reps).astype(np.int64)
    return n, src, dst, tg.rows_of(tg.per_node_dense(n, src, dst))


@pytest.mark.parametrize("build", BUILDS)
def test_complete_digraph(session, knobs, build):
    """out-degrees up to 2199, ids on both sides of the window's end, against the float64 diag(M^3)"""
    _build(knobs, session, build)
    n, src, dst, want = _complete_2200()
    assert same_rows(_by_node(session, n, src, dst), want)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fillers", [tg.BY_NODE_WIN - 1, tg.BY_NODE_WIN])
def test_hub_at_the_window_edge(session, knobs, fillers, build):
    """the star's centre is the last id of the privatised window / the first id outside it"""
    _build(knobs, session, build)
    (n, src, dst), c = tg.star_behind(fillers)
    core = (src < 2 * tg.STAR_T + 1) & (dst < 2 * tg.STAR_T + 1)
    want = tg.per_node_enumerate(n, src, dst)
    assert want[c] == tg.per_node_dense(2 * tg.STAR_T + 1, src[core], dst[core])[c] > 0
    assert same_rows(_by_node(session, n, src, dst), tg.rows_of(want))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("t", [tg.TILE_SLOTS - 1, tg.TILE_SLOTS, tg.TILE_SLOTS + 1])
def test_one_slot_rows_at_a_tile_end(session, knobs, t, build):
    """t disjoint triangles: t rows of one slot each (a full tile holds as many rows as slots)"""
    _build(knobs, session, build)
    n, src, dst = tg.disjoint_triangles(t)
    assert same_rows(_by_node(session, n, src, dst), [{"id": i, "n": 1} for i in range(n)])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("slots", [2 * tg.TILE_SLOTS, 2 * tg.TILE_SLOTS + 1])
def test_rows_across_tile_ends(session, knobs, slots, build):
    """exactly two tiles / two tiles and one slot; a row of several slots straddles the first tile end"""
    _build(knobs, session, build)
    n, src, dst = tg.clique_and_triangles(slots)
    assert same_rows(_by_node(session, n, src, dst), tg.rows_of(tg.per_node_dense(n, src, dst)))


def test_wide_id_range(session):
    """ids spread over [0, 2^25 + 3): uncoded targets (cb == 0), every payload read from ov; the construction of
    tests/test_gpu_triangles.py test_wide_id_range"""
    rng = np.random.default_rng(21)
    n = (1 << 25) + 3
    ids = np.unique(rng.integers(0, n, 700)).astype(np.int64)
    ids[-1] = n - 1
    k = len(ids)
    a = rng.integers(0, k, 9000)
    b = rng.integers(0, k, 9000)
    b[:300] = a[:300]  # self-loops
    want = tg.rows_of(tg.per_node_dense(k, a, b), ids)
    assert same_rows(_by_node(session, n, ids[a], ids[b], ids=ids), want)


def test_null_arguments(session):
    from capsmi import _lib
    out = ctypes.c_void_p()
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_trigraph_count_by_node", session.handle, None, b"id", b"n", ctypes.byref(out))
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_by_node", session.handle, 0, None, b"source", b"target", None, b"id", b"n",
                  ctypes.byref(out))


# ---- the planner route ------------------------------------------------------------------------------------

LO = 1000


@functools.lru_cache(maxsize=None)
def _labelled():
    """60 nodes from LO on, three in four labelled L and the rest M; 420 relationships of two types, self-loops
    and parallel relationships among them (a few thousand bindings at the most)"""
    rng = np.random.default_rng(77)
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


def _query(labels=("L", "L", "L"), items=(("k", ["id", "a"]), ("n", ["count*"]))):
    la, lb, lc = labels
    return {"clauses": [{"match": f"(a:{la})-[:R|S]->(b:{lb})-[:R|S]->(c:{lc})-[:R|S]->(a)"}],
            "return": {"items": [[k, spec] for k, spec in items]}}


def _run(session, sg, q, fused=True):
    from capsmi.planner import Planner, result_rows
    session.set_fused(fused)
    try:
        t, outs = Planner(sg).run(q)
        return result_rows(t, outs, session.dictionary)
    finally:
        session.set_fused(True)


def _want_l():
    n, src, dst, is_l, _ = _labelled()
    cnt = tg.per_node_enumerate(n, src, dst, ok=(is_l, is_l, is_l))
    assert 0 < cnt.sum() < 5000
    return [{"k": LO + int(i), "n": int(cnt[i])} for i in np.nonzero(cnt)[0]]


@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_routed(session, labelled, key):
    """grouped by a -- the test that fails without the route -- and, by rotation, by b and by c"""
    before = session.route_count("triangle_grouped")
    got = _run(session, labelled, _query(items=(("k", ["id", key]), ("n", ["count*"]))))
    assert session.route_count("triangle_grouped") == before + 1, "plan not routed to 'triangle_grouped'"
    assert same_rows(got, _want_l())


def test_unfused_gives_the_same_rows(session, labelled):
    before = session.route_count("triangle_grouped")
    got = _run(session, labelled, _query(), fused=False)
    assert session.route_count("triangle_grouped") == before
    assert same_rows(got, _want_l())


def test_ungrouped_count_is_the_sum(session, labelled):
    before = session.route_count("triangle"), session.route_count("triangle_grouped")
    got = _run(session, labelled, _query(items=(("n", ["count*"]),)))
    assert (session.route_count("triangle"), session.route_count("triangle_grouped")) == (before[0] + 1, before[1])
    assert got == [{"n": sum(r["n"] for r in _want_l())}]


def _not_routed(session, sg, q):
    before = session.route_count("triangle_grouped")
    got = _run(session, sg, q)
    assert session.route_count("triangle_grouped") == before
    return got


def test_different_labels_take_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    cnt = tg.per_node_enumerate(n, src, dst, ok=(is_l, ~is_l, is_l))
    assert cnt.sum() > 0
    got = _not_routed(session, labelled, _query(labels=("L", "M", "L")))
    assert same_rows(got, [{"k": LO + int(i), "n": int(cnt[i])} for i in np.nonzero(cnt)[0]])


def test_two_keys_take_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    pairs = {}
    for a, b, _ in tg.bindings(src, dst, (is_l, is_l, is_l)):
        pairs[(a, b)] = pairs.get((a, b), 0) + 1
    got = _not_routed(session, labelled, _query(items=(("k", ["id", "a"]), ("j", ["id", "b"]), ("n", ["count*"]))))
    assert same_rows(got, [{"k": LO + a, "j": LO + b, "n": c} for (a, b), c in pairs.items()])


def test_count_distinct_takes_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    bs = {}
    for a, b, _ in tg.bindings(src, dst, (is_l, is_l, is_l)):
        bs.setdefault(a, set()).add(b)
    got = _not_routed(session, labelled, _query(items=(("k", ["id", "a"]), ("n", ["count_distinct", ["id", "b"]]))))
    assert same_rows(got, [{"k": LO + a, "n": len(s)} for a, s in bs.items()])


def test_tagged_ids(session):
    """ids carrying a graph tag in the top 10 bits (Tags.scala: id | tag << 54), reached through the graph's
    dense id compaction: the rows carry the tagged ids"""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    ids, src, dst, tags = tg.tagged_graph()
    retag = np.vectorize(lambda v: tags[int(v)], otypes=[np.int64])
    nodes = session.table([ColumnData("id", I64, retag(ids))]).as_node_table("id")
    rels = session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64) * 3 + (1 << 50)),
                          ColumnData("source", I64, retag(src)), ColumnData("target", I64, retag(dst))]).as_rel_table(
        "id", "source", "target")
    assert session.compact_if_sparse([nodes], [rels])
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    q = {"clauses": [{"match": "(a)-[:R]->(b)-[:R]->(c)-[:R]->(a)"}],
         "return": {"items": [["k", ["id", "a"]], ["n", ["count*"]]]}}
    before = session.route_count("triangle_grouped")
    got = _run(session, sg, q)
    assert session.route_count("triangle_grouped") == before + 1
    cnt = tg.per_node_dense(*tg.relabel(ids, src, dst))
    assert cnt.sum() > 0
    assert same_rows(got, [{"k": tags[int(ids[i])], "n": int(cnt[i])} for i in np.nonzero(cnt)[0]])
