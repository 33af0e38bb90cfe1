"""The undirected triangle (csrc/k_tri_nodes.hip, routes "triangle_undirected" and "triangle_undirected_grouped"):
  MATCH (a)-[r1]-(b)-[r2]-(c)-[r3]-(a) RETURN count(*)
  MATCH (a)-[r1]-(b)-[r2]-(c)-[r3]-(a) RETURN id(a), count(*)     (or id(b), or id(c))
through the direct entry points on both trigraph builds and through the planner, against the enumeration of the
plan and the closed form of tests/tri_und_ref.py (pinned against each other in tests/test_tri_und_ref_cpu.py).
count(*) runs in both of its forms (CAPSMI_TRI_UND_COUNT = hash, walk); both must equal each other and the sums of
the END rows and of the MIDDLE rows.  Every row is compared, with its id; counts are integers and must match
exactly."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import tri_und_ref as tu
from golden_util import same_rows

pytestmark = pytest.mark.gpu

BUILDS = ["direct", "sorted"]
FORMS = ("hash", "walk")
CLASS_NAMES = {tu.END: "end", tu.MIDDLE: "middle"}


def _build(knobs, session, build):
    if build == "sorted":
        knobs(session, CAPSMI_TRI_BUILD="sorted")


def _rows(t):
    ids, cnt = t.column("id").values, t.column("n").values
    assert t.column("id").valid is None and t.column("n").valid is None  # two non-nullable Long columns
    assert ids.dtype == np.int64 and cnt.dtype == np.int64
    return [{"id": int(i), "n": int(c)} for i, c in zip(ids, cnt)]


def _tables(session, n, src, dst, mask=None, lo=0, ids=None):
    from capsmi import ColumnData, I64, graph
    rels = session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)), ColumnData("source", I64, src),
                          ColumnData("target", I64, dst)])
    if ids is None:
        ids = lo + (np.arange(n) if mask is None else np.nonzero(mask)[0])
    nodes = session.table([ColumnData("id", I64, np.asarray(ids, dtype=np.int64))])
    return rels, graph.NodeBitmap(session, lo, lo + n).add_scan(nodes)


def _all(session, n, src, dst, mask=None, lo=0, ids=None, handle=False, forms=FORMS, by_node=True):
    """({form: count(*)}, rows per class) of the entry points over the window [lo, lo + n)"""
    from capsmi import graph
    rels, ok = _tables(session, n, src, dst, mask, lo, ids)
    counts, rows = {}, None
    if handle:
        g = graph.TriGraph(session, [rels], ok)
        try:
            for f in forms:
                with session.configured(CAPSMI_TRI_UND_COUNT=f):
                    counts[f] = g.count_undirected()
            if by_node:
                rows = [_rows(g.count_undirected_by_node(c, "id", "n")) for c in tu.CLASSES]
        finally:
            g.release()
        return counts, rows
    for f in forms:
        with session.configured(CAPSMI_TRI_UND_COUNT=f):
            counts[f] = graph.triangle_count_undirected(session, [rels], ok)
    if by_node:
        rows = [_rows(graph.triangle_count_undirected_by_node(session, [rels], ok, c, "id", "n")) for c in tu.CLASSES]
    return counts, rows


def _check(got, want, ids=None):
    """got = _all(...); want = the 3 x n counts per position.  Every class's rows; hash = walk = the count = the
    sum of the END rows = the sum of the MIDDLE rows."""
    counts, rows = got
    assert want[0].tolist() == want[2].tolist()
    total = int(want[0].sum())
    for f, v in counts.items():
        assert v == total, f"count(*), CAPSMI_TRI_UND_COUNT={f}"
    assert len(set(counts.values())) == 1
    for c in tu.CLASSES:
        assert same_rows(rows[c], tu.rows_of(want[c], ids)), f"class {CLASS_NAMES[c]}"
        assert total == sum(x["n"] for x in rows[c]), f"count(*) against the sum over the {CLASS_NAMES[c]} rows"


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("seed", range(8))
def test_random_multigraphs(session, knobs, seed, build):
    _build(knobs, session, build)
    n, src, dst = tu.random_multigraph(seed)
    want = tu.per_node_enumerate_all(n, src, dst)
    assert want.tolist() == tu.per_node_dense_all(n, src, dst).tolist()
    _check(_all(session, n, src, dst, handle=False), want)
    _check(_all(session, n, src, dst, handle=True), want)


# ---- one triangle, six different multiplicities, every degree order ----------------------------------------------

PRIME_LOOPS = tu.PRIME_LOOPS


@functools.lru_cache(maxsize=None)
def _prime_triangle(pendants):
    """the prime triangle of tests/tri_grouped_ref.py (m = 2, 3, 5, 7, 11, 13 around {0, 1, 2}; 1, 2, 4 self-loops)
    with its expected 3 x n counts"""
    n, src, dst = tu.prime_triangle(pendants)
    return n, src, dst, tu.per_node_dense_all(n, src, dst)


def test_prime_triangle_reference():
    """U = 5, 12, 24: T = 2 * 5 * 12 * 24 at every corner; the pair terms differ per corner and per class, so a
    swapped payload half (U taken as f or b alone) or a wrong class shows; all six degree orders occur"""
    orders = set()
    for pend in itertools.permutations((1, 2, 3)):
        n, src, dst, want = _prime_triangle(pend)
        rid = tu.degree_order(n, src, dst)
        assert sorted(rid[:3].tolist()) == [0, 1, 2]
        orders.add(tuple(rid[:3].tolist()))
        assert len(set(want[:2, :3].flatten().tolist())) == 6
        assert want[:, 3:].sum() == 0
    assert len(orders) == 6
    n, src, dst, want = _prime_triangle((1, 2, 3))
    assert want.tolist() == tu.per_node_enumerate_all(n, src, dst).tolist()
    s, q01, q12, q02 = PRIME_LOOPS, 5 * 4, 12 * 11, 24 * 23
    assert int(want[0][0]) == 2 * 5 * 12 * 24 + (3 * s[0] + s[1]) * q01 + (3 * s[0] + s[2]) * q02 + 0
    assert int(want[1][1]) == 2 * 5 * 12 * 24 + 2 * (s[1] + s[0]) * q01 + 2 * (s[1] + s[2]) * q12 + 0
    assert int(want[0][2]) == 2 * 5 * 12 * 24 + (3 * s[2] + s[0]) * q02 + (3 * s[2] + s[1]) * q12 + 2 * 4 * 3 * 2


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("pend", list(itertools.permutations((1, 2, 3))))
def test_prime_triangle_under_every_degree_order(session, knobs, pend, build):
    _build(knobs, session, build)
    n, src, dst, want = _prime_triangle(pend)
    _check(_all(session, n, src, dst), want)


# ---- pair and self terms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", BUILDS)
def test_loops_only(session, knobs, build):
    """s = 0, 1, 2, 3, 4 self-loops and nothing else: 2 s (s - 1) (s - 2) at every position"""
    _build(knobs, session, build)
    v = np.repeat(np.arange(5, dtype=np.int64), np.arange(5))
    want = np.array([[0, 0, 0, 12, 48]] * 3, dtype=np.int64)
    assert want.tolist() == tu.per_node_enumerate_all(5, v, v).tolist()
    _check(_all(session, 5, v, v), want)


@pytest.mark.parametrize("build", BUILDS)
def test_one_directional_pairs_beside_loops(session, knobs, build):
    """Q s terms of pairs with m(y,x) = 0: 0 has two loops, 3 one; 0 -> 1 twice, 2 -> 0 three times, 1 -> 3 three
    times, 3 -> 4 twice, 4 <-> 5 without a loop (no term), and 5 -> 0 once (Q = 0)"""
    _build(knobs, session, build)
    src = np.array([0, 0, 3, 0, 0, 2, 2, 2, 1, 1, 1, 3, 3, 4, 5, 5], dtype=np.int64)
    dst = np.array([0, 0, 3, 1, 1, 0, 0, 0, 3, 3, 3, 4, 4, 5, 4, 0], dtype=np.int64)
    want = tu.per_node_enumerate_all(6, src, dst)
    assert want.tolist() == tu.per_node_dense_all(6, src, dst).tolist()
    # 4 s Q per looped end of a pair: {0,1} 4*2*2, {0,2} 4*2*6, {1,3} 4*1*6, {3,4} 4*1*2; no triangle ({4,5} and
    # {5,0} close none)
    assert int(want[0].sum()) == 16 + 48 + 24 + 8
    _check(_all(session, 6, src, dst), want)
    _check(_all(session, 6, src, dst, handle=True), want)


@pytest.mark.parametrize("build", BUILDS)
def test_lone_loop_beside_a_double_relationship(session, knobs, build):
    """x -> x, x -> y, y -> x: the a = c term twice, 8 rows"""
    _build(knobs, session, build)
    src, dst = np.array([0, 0, 1], dtype=np.int64), np.array([0, 1, 0], dtype=np.int64)
    want = tu.per_node_enumerate_all(2, src, dst)
    assert int(want[0].sum()) == 8
    _check(_all(session, 2, src, dst), want)


@pytest.mark.parametrize("build", BUILDS)
def test_no_rows(session, knobs, build):
    """no relationships; a path; a lone loop; one pair without a third node"""
    _build(knobs, session, build)
    none = ({"hash": 0, "walk": 0}, [[], []])
    e = np.zeros(0, dtype=np.int64)
    assert _all(session, 48, e, e) == none
    src = np.array([0, 1, 2, 3, 5, 6, 7], dtype=np.int64)  # a path, a reciprocal pair, a loop
    dst = np.array([1, 2, 3, 4, 6, 5, 7], dtype=np.int64)
    assert tu.per_node_enumerate_all(9, src, dst).sum() == 0
    assert _all(session, 9, src, dst) == none
    assert _all(session, 9, src, dst, handle=True) == none
    one = np.array([0], dtype=np.int64)
    assert _all(session, 2, one, one) == none      # a lone loop
    assert _all(session, 2, one, one + 1) == none  # one relationship


# ---- the walk's tiles --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _flipped(name, arg, seed):
    """a builder's graph with every relationship reversed with probability 1/2 (fixed seed): the count does not
    depend on the directions, the payload halves do; (n, src, dst, expected 3 x n)"""
    n, src, dst = getattr(tu, name)(arg)
    flip = np.random.default_rng(seed).random(len(src)) < 0.5
    s, d = np.where(flip, dst, src), np.where(flip, src, dst)
    return n, s, d, tu.per_node_dense_all(n, s, d)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("t", [tu.TILE_SLOTS - 1, tu.TILE_SLOTS, tu.TILE_SLOTS + 1])
def test_one_slot_rows_at_a_tile_end(session, knobs, t, build):
    """t disjoint triangles with random directions: t rows of one slot each, 2 rows per corner and position"""
    _build(knobs, session, build)
    n, src, dst, want = _flipped("disjoint_triangles", t, 502)
    assert int(tu.walk_slots(n, src, dst).sum()) == t
    assert want.tolist() == np.full((3, 3 * t), 2).tolist()
    _check(_all(session, n, src, dst), want)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("slots", [2 * tu.TILE_SLOTS, 2 * tu.TILE_SLOTS + 1])
def test_rows_across_tile_ends(session, knobs, slots, build):
    """exactly two tiles / two tiles and one slot; a row of several slots straddles the first tile end"""
    _build(knobs, session, build)
    n, src, dst = tu.clique_and_triangles(slots)
    assert int(tu.walk_slots(n, src, dst).sum()) == slots
    _check(_all(session, n, src, dst), tu.per_node_dense_all(n, src, dst))


def test_clique_and_triangles_reference():
    n, src, dst = tu.clique_and_triangles(2 * tu.TILE_SLOTS)
    sub = (src < 30) & (dst < 30)  # the large clique (the first CLIQUE_K = 20 ids) and two small ones
    assert tu.per_node_enumerate_all(30, src[sub], dst[sub]).tolist() == \
        tu.per_node_dense_all(30, src[sub], dst[sub]).tolist()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("fillers", [tu.BY_NODE_WIN - 1, tu.BY_NODE_WIN])
def test_hub_at_the_window_edge(session, knobs, fillers, build):
    """the star's centre (two self-loops, three triangles, a reciprocal spoke) is the last id of the privatised
    window / the first id outside it"""
    _build(knobs, session, build)
    (n, src, dst), c = tu.star_behind(fillers)
    assert c == 0 and tu.degree_order(n, src, dst)[c] == fillers
    want = tu.per_node_enumerate_all(n, src, dst)
    assert want.tolist() == tu.per_node_dense_all(n, src, dst).tolist()
    assert want[0][c] > 0 and want[0][c] != want[1][c]
    _check(_all(session, n, src, dst), want)


COMPLETE_N = 300


@functools.lru_cache(maxsize=None)
def _complete():
    a, b = np.nonzero(~np.eye(COMPLETE_N, dtype=bool))
    perm = np.random.default_rng(504).permutation(len(a))
    return a[perm].astype(np.int64), b[perm].astype(np.int64)


@pytest.mark.parametrize("build", BUILDS)
def test_complete_digraph(session, knobs, build):
    """K_300, every ordered pair once, U = 2: 8 (n-1)(n-2) per node and position.  The walk has C(300, 3) slots in
    2176 tiles of 2048, above tile_grid's cap of 2048 workgroups: the block-stride loop takes a second tile in 128
    of them.  Both forms of the count."""
    _build(knobs, session, build)
    n = COMPLETE_N
    src, dst = _complete()
    slots = n * (n - 1) * (n - 2) // 6
    assert -(-slots // tu.TILE_SLOTS) > tu.TILE_GRID_CAP
    want = np.full((3, n), 8 * (n - 1) * (n - 2), dtype=np.int64)
    got = _all(session, n, src, dst)
    assert got[0] == {"hash": 8 * n * (n - 1) * (n - 2), "walk": 8 * n * (n - 1) * (n - 2)}
    _check(got, want)


# ---- the hash walks' edges (CAPSMI_TRI_UND_COUNT=hash) -----------------------------------------------------------

@pytest.mark.parametrize("build", BUILDS)
def test_dense_big_vertices(session, knobs, build):
    """the dense random multigraph of test_gpu_triangles.py::test_dense_big_vertices: oriented out-degrees above
    64, lists in the <= 64, <= 128 and > 128 groups of the item walks"""
    _build(knobs, session, build)
    rng = np.random.default_rng(11)
    n, m = 300, 40000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    od = _oriented_out_degrees(n, src, dst)
    assert (od <= 64).any() and ((od > 64) & (od <= 128)).any() and (od > 128).any()
    want = tu.per_node_dense_all(n, src, dst)
    assert 0 < int(want[0].sum()) < 2 ** 62
    _check(_all(session, n, src, dst, forms=("hash",)), want)


def _oriented_out_degrees(n, src, dst):
    """out-degrees of the degree-ordered orientation (distinct neighbours of a higher degree-order id)"""
    rid = tu.degree_order(n, src, dst)
    nl = src != dst
    a, b = rid[src[nl]], rid[dst[nl]]
    pairs = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)]), axis=1)
    return np.bincount(pairs[0], minlength=n)


ITEM_LANES = 512                    # csrc/k_tri.hip: the u-mode items' workgroup, B
HASH_CHUNK = 2 * ITEM_LANES         # ItemLds<B>::kChunk: out-list entries per hash chunk
CHUNKS_N = HASH_CHUNK + 76          # 1100 nodes: the first node's oriented out-list (n - 1 entries) takes two chunks


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mult", [False, True])
def test_complete_digraph_hash_chunks(session, knobs, mult, build):
    """the complete digraph on 1100 nodes, with and without multiplicities 1..3: oriented out-degrees up to 1099
    exceed one 1024-entry hash chunk of the 512-lane items.  Loop-free, so count(*) = trace(U^3), exact in
    float64 here."""
    _build(knobs, session, build)
    n = CHUNKS_N
    assert n - 1 > HASH_CHUNK
    rng = np.random.default_rng(5)
    M = np.ones((n, n), dtype=np.int64)
    if mult:
        M = rng.integers(1, 4, (n, n)).astype(np.int64)
    np.fill_diagonal(M, 0)
    a, b = np.nonzero(M)
    src, dst = np.repeat(a, M[a, b]).astype(np.int64), np.repeat(b, M[a, b]).astype(np.int64)
    U = (M + M.T).astype(np.float64)
    assert float(n) ** 3 * float(U.max()) ** 3 < 2.0 ** 53
    want = int(np.rint(np.trace(U @ U @ U)))
    if not mult:
        assert want == 8 * n * (n - 1) * (n - 2)
    counts, _ = _all(session, n, src, dst, forms=("hash",), by_node=False)
    assert counts == {"hash": want}


# ---- large counts, node filter, window ---------------------------------------------------------------------------

@pytest.mark.parametrize("build", BUILDS)
def test_counts_above_2_32_and_exception_payloads(session, knobs, build):
    """multiplicity 1700 on all six directed edges (every coded field an exception: payloads from ov) and three
    self-loops on one corner; expected from the closed form in Python ints, which must fit int64"""
    _build(knobs, session, build)
    n, src, dst = tu.heavy_triangle()
    exact = tu.per_node_dense_all(n, src, dst, dtype=object)
    assert all(2 ** 32 < int(x) < 2 ** 63 for x in exact.flatten()) and int(exact[0].sum()) < 2 ** 63
    want = exact.astype(np.int64)
    u = 3400
    assert int(want[0][0]) == 2 * u ** 3 + 3 * u * (u - 1)  # 0 has no loop: s(2) Q(0,2) only
    assert int(want[1][2]) == 2 * u ** 3 + 2 * 2 * 3 * u * (u - 1) + 2 * 3 * 2 * 1
    _check(_all(session, n, src, dst), want)
    _check(_all(session, n, src, dst, handle=True), want)


@pytest.mark.parametrize("build", BUILDS)
def test_node_filter_and_window(session, knobs, build):
    """about 70 % of 200 nodes kept, in a window that starts at 5000, and 300 relationships with an end below or
    above the window"""
    _build(knobs, session, build)
    rng = np.random.default_rng(42)
    n, m, lo = 200, 4000, 5000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[:300] = dst[:300]
    mask = rng.random(n) < 0.7
    keep = mask[src] & mask[dst]
    want = tu.per_node_dense_all(n, src[keep], dst[keep])
    full = tu.per_node_dense_all(n, src, dst)
    assert 0 < want[0].sum() < full[0].sum()
    inside = rng.integers(0, n, 300) + lo
    outside = np.where(rng.random(300) < 0.5, lo - 1 - rng.integers(0, 50, 300), lo + n + rng.integers(0, 50, 300))
    swap = rng.random(300) < 0.5
    xs = np.concatenate([src + lo, np.where(swap, inside, outside)])
    xd = np.concatenate([dst + lo, np.where(swap, outside, inside)])
    _check(_all(session, n, xs, xd, mask, lo=lo), want, lo + np.arange(n))
    _check(_all(session, n, xs, xd, mask, lo=lo, handle=True), want, lo + np.arange(n))


# ---- errors ------------------------------------------------------------------------------------------------------

def test_null_arguments(session):
    from capsmi import _lib
    out, v = ctypes.c_void_p(), ctypes.c_int64()
    rels, ok = _tables(session, 3, np.array([0, 1, 0], dtype=np.int64), np.array([1, 2, 2], dtype=np.int64))
    arr = (ctypes.c_void_p * 1)(rels.handle)
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_trigraph_count_undirected", session.handle, None, ctypes.byref(v))
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_trigraph_count_undirected_by_node", session.handle, None, 0, b"id", b"n", ctypes.byref(out))
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_undirected", session.handle, 1, arr, b"source", b"target", None, ctypes.byref(v))
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_undirected", session.handle, 1, arr, b"source", b"target", ok.handle, None)
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_undirected_by_node", session.handle, 1, arr, b"source", b"target", ok.handle, 0,
                  b"id", b"n", None)
    with pytest.raises(_lib.IllegalArgumentException):
        _lib.call("capsmi_triangle_count_undirected_by_node", session.handle, 1, arr, b"source", b"target", ok.handle, 0,
                  None, b"n", ctypes.byref(out))


@pytest.mark.parametrize("position", [2, -1])
def test_position_out_of_range(session, position):
    from capsmi import _lib, graph
    rels, ok = _tables(session, 3, np.array([0, 1, 0], dtype=np.int64), np.array([1, 2, 2], dtype=np.int64))
    with pytest.raises(_lib.IllegalArgumentException):
        graph.triangle_count_undirected_by_node(session, [rels], ok, position, "id", "n")
    g = graph.TriGraph(session, [rels], ok)
    try:
        with pytest.raises(_lib.IllegalArgumentException):
            g.count_undirected_by_node(position, "id", "n")
        assert g.count_undirected() == 6
    finally:
        g.release()


# ---- the planner routes ------------------------------------------------------------------------------------------

LO = 1000


@functools.lru_cache(maxsize=None)
def _labelled():
    """the labelled two-type graph of test_gpu_triangles_transitive.py: 60 nodes from LO on, three in four labelled
    L and the rest M; 420 relationships of two types, self-loops and parallel relationships among them"""
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


def _pattern(dirs="---", labels=("L", "L", "L"), types="R|S"):
    hop = {">": f"-[:{types}]->", "<": f"<-[:{types}]-", "-": f"-[:{types}]-"}
    la, lb, lc = [f":{x}" if x else "" for x in labels]
    return f"(a{la}){hop[dirs[0]]}(b{lb}){hop[dirs[1]]}(c{lc}){hop[dirs[2]]}(a)"


def _query(dirs="---", labels=("L", "L", "L"), items=(("k", ["id", "a"]), ("n", ["count*"]))):
    return {"clauses": [{"match": _pattern(dirs, labels)}], "return": {"items": [[k, spec] for k, spec in items]}}


def _run(session, sg, q, fused=True):
    from capsmi.planner import Planner, result_rows
    session.set_fused(fused)
    try:
        t, outs = Planner(sg).run(q)
        return result_rows(t, outs, session.dictionary)
    finally:
        session.set_fused(True)


ROUTES = ("triangle", "triangle_grouped", "triangle_transitive", "triangle_transitive_grouped", "triangle_undirected",
          "triangle_undirected_grouped", "undirected", "miss")


def _routes(session):
    return {r: session.route_count(r) for r in ROUTES}


def _rose(session, before):
    """the routes that rose since `before`, with by how much"""
    return {r: v - before[r] for r, v in _routes(session).items() if v != before[r]}


@functools.lru_cache(maxsize=None)
def _want_l():
    """3 x n: the plan's rows per position among the L nodes"""
    n, src, dst, is_l, _ = _labelled()
    cnt = tu.per_node_enumerate_all(n, src, dst, ok=(is_l, is_l, is_l))
    assert 0 < cnt[0].sum() < 200000
    assert cnt[0].tolist() != cnt[1].tolist()  # the classes differ: a wrong class shows
    return cnt


def _k_rows(cnt):
    return [{"k": LO + int(i), "n": int(cnt[i])} for i in np.nonzero(cnt)[0]]


@pytest.mark.parametrize("form", FORMS)
def test_count_routed(session, knobs, labelled, form):
    knobs(session, CAPSMI_TRI_UND_COUNT=form)
    q = _query(items=(("n", ["count*"]),))
    before = _routes(session)
    got = _run(session, labelled, q)
    assert _rose(session, before) == {"triangle_undirected": 1}
    assert got == [{"n": int(_want_l()[0].sum())}]
    before = _routes(session)
    unfused = _run(session, labelled, q, fused=False)
    assert set(_rose(session, before)) <= {"miss"}  # no fused route took it
    assert got == unfused


def test_grouped_routed(session, labelled):
    """grouped by a, by b and by c: routed once each, equal to the unfused run and to the enumeration of the plan;
    the a and c rows are equal"""
    got = {}
    for key in "abc":
        q = _query(items=(("k", ["id", key]), ("n", ["count*"])))
        before = _routes(session)
        got[key] = _run(session, labelled, q)
        assert _rose(session, before) == {"triangle_undirected_grouped": 1}
        assert same_rows(got[key], _k_rows(_want_l()["abc".index(key)])), key
        before = _routes(session)
        unfused = _run(session, labelled, q, fused=False)
        assert set(_rose(session, before)) <= {"miss"}
        assert same_rows(got[key], unfused), key
    assert same_rows(got["a"], got["c"])
    assert not same_rows(got["a"], got["b"])


def _generic(session, sg, q):
    before = _routes(session)
    got = _run(session, sg, q)
    rose = _rose(session, before)
    assert set(rose) == {"miss"} and rose["miss"] >= 1
    return got


@pytest.mark.parametrize("dirs", ["->-", "--<", ">--"])
def test_one_directed_hop_takes_the_generic_plan(session, labelled, dirs):
    got = _generic(session, labelled, _query(dirs, items=(("n", ["count*"]),)))
    assert got == _run(session, labelled, _query(dirs, items=(("n", ["count*"]),)), fused=False)
    assert got[0]["n"] > 0


def test_different_labels_take_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    cnt = tu.per_node_enumerate_all(n, src, dst, ok=(is_l, ~is_l, is_l))[0]
    assert cnt.sum() > 0
    got = _generic(session, labelled, _query(labels=("L", "M", "L")))
    assert same_rows(got, _k_rows(cnt))


def test_two_keys_take_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    pairs = {}
    for a, b, _ in tu.bindings(src, dst, (is_l, is_l, is_l)):
        pairs[(a, b)] = pairs.get((a, b), 0) + 1
    got = _generic(session, labelled, _query(items=(("k", ["id", "a"]), ("j", ["id", "b"]), ("n", ["count*"]))))
    assert same_rows(got, [{"k": LO + a, "j": LO + b, "n": c} for (a, b), c in pairs.items()])


def test_count_distinct_takes_the_generic_plan(session, labelled):
    n, src, dst, is_l, _ = _labelled()
    bs = {}
    for a, b, _ in tu.bindings(src, dst, (is_l, is_l, is_l)):
        bs.setdefault(a, set()).add(b)
    got = _generic(session, labelled, _query(items=(("k", ["id", "a"]), ("n", ["count_distinct", ["id", "b"]]))))
    assert same_rows(got, [{"k": LO + a, "n": len(s)} for a, s in bs.items()])


DIRECTED = ["".join(d) for d in itertools.product("><", repeat=3)]


@pytest.mark.parametrize("dirs", DIRECTED)
def test_directed_spellings_keep_their_routes(session, labelled, dirs):
    """the six mixed spellings take the transitive routes and the two uniform ones the cyclic routes, as before"""
    mixed = len(set(dirs)) == 2
    before = _routes(session)
    _run(session, labelled, _query(dirs))
    assert _rose(session, before) == {"triangle_transitive_grouped" if mixed else "triangle_grouped": 1}
    before = _routes(session)
    _run(session, labelled, _query(dirs, items=(("n", ["count*"]),)))
    assert _rose(session, before) == {"triangle_transitive" if mixed else "triangle": 1}


def test_undirected_two_hop_keeps_its_route(session, labelled):
    q = {"clauses": [{"match": "(a:L)-[:R|S]-(b:L)-[:R|S]-(c:L)"}], "return": {"items": [["n", ["count*"]]]}}
    before = _routes(session)
    got = _run(session, labelled, q)
    assert _rose(session, before) == {"undirected": 1}
    assert got == _run(session, labelled, q, fused=False)


@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_tagged_ids(session, key):
    """ids carrying a graph tag in the top 10 bits (Tags.scala: id | tag << 54), reached through the graph's
    dense id compaction: routed, and the rows carry the tagged ids"""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    ids, src, dst, tags = tu.tagged_graph()
    retag = np.vectorize(lambda v: tags[int(v)], otypes=[np.int64])
    nodes = session.table([ColumnData("id", I64, retag(ids))]).as_node_table("id")
    rels = session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64) * 3 + (1 << 50)),
                          ColumnData("source", I64, retag(src)), ColumnData("target", I64, retag(dst))]).as_rel_table(
        "id", "source", "target")
    assert session.compact_if_sparse([nodes], [rels])
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    q = {"clauses": [{"match": _pattern(labels=("", "", ""), types="R")}],
         "return": {"items": [["k", ["id", key]], ["n", ["count*"]]]}}
    before = _routes(session)
    got = _run(session, sg, q)
    assert _rose(session, before) == {"triangle_undirected_grouped": 1}
    cnt = _tagged_want()["abc".index(key)]
    assert cnt.sum() > 0
    assert same_rows(got, [{"k": tags[int(ids[i])], "n": int(cnt[i])} for i in np.nonzero(cnt)[0]])
    if key == "a":
        q = {"clauses": [{"match": _pattern(labels=("", "", ""), types="R")}], "return": {"items": [["n", ["count*"]]]}}
        before = _routes(session)
        assert _run(session, sg, q) == [{"n": int(cnt.sum())}]
        assert _rose(session, before) == {"triangle_undirected": 1}


@functools.lru_cache(maxsize=None)
def _tagged_want():
    ids, src, dst, _ = tu.tagged_graph()
    return tu.per_node_dense_all(*tu.relabel(ids, src, dst))
