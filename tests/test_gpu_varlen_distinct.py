"""Var-length count(DISTINCT b) on the device (k_reach.hip: k-hop reach by bit-parallel BFS) against the numpy walk
BFS of varlen_distinct_ref.py -- the direct entry points at the kernels' edges (batch widths, slice borders, hubs,
level arithmetic, the zero-length path), and the planner's plans routed to them ("var_length_distinct")."""
import numpy as np
import pytest

from golden_util import same_rows
from varlen_distinct_ref import reach_sets

pytestmark = pytest.mark.gpu

WORDS = ["auto", "1", "2", "4", "8"]
LDS_WORDS = 16384  # k_reach.hip kLdsWords: a target slice is LDS_WORDS / W ids at W words per node


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src))), ColumnData("source", I64, src),
                          ColumnData("target", I64, dst)])


def _bitmaps(session, n, a_mask, b_mask, lo=0):
    from capsmi import ColumnData, I64, graph
    a_nodes = session.table([ColumnData("id", I64, np.nonzero(a_mask)[0].astype(np.int64) + lo)])
    b_nodes = session.table([ColumnData("id", I64, np.nonzero(b_mask)[0].astype(np.int64) + lo)])
    return (graph.NodeBitmap(session, lo, lo + n).add_scan(a_nodes), graph.NodeBitmap(session, lo, lo + n).add_scan(b_nodes))


def _check(session, n, src, dst, a_mask, b_mask, lower, upper, lo=0, rels=None):
    """Both forms against reach_sets (src / dst absolute ids, masks over the window [lo, lo + n)), each run twice."""
    from capsmi import graph
    a_mask, b_mask = np.asarray(a_mask, bool), np.asarray(b_mask, bool)
    rels = rels or [_table(session, src, dst)]
    a_ok, b_ok = _bitmaps(session, n, a_mask, b_mask, lo)
    counts, union = reach_sets(n, src - lo, dst - lo, a_mask, b_mask, lower, upper)
    expect = {int(i) + lo: int(counts[i]) for i in np.nonzero(counts)[0]}
    prints = []
    for _ in range(2):
        out = graph.var_length_count_distinct(session, rels, a_ok, b_ok, lower, upper, "a", "cnt")
        got = dict(zip(out.column("a").values.tolist(), out.column("cnt").values.tolist()))
        assert out.size == len(got)
        assert got == expect, (lower, upper)
        prints.append(out.fingerprint(["a", "cnt"]))
        assert graph.var_length_reach_count(session, rels, a_ok, b_ok, lower, upper) == union, (lower, upper)
    assert prints[0] == prints[1]
    return counts, union


RANGES = [(1, 1), (1, 2), (1, 3), (0, 3), (1, 6), (0, 10)]


@pytest.mark.parametrize("seed", range(6))
def test_random_multigraphs(session, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 300))
    m = int(rng.integers(0, 3000))
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 5] = dst[: m // 5]  # self-loops
    a_mask = rng.random(n) < 0.7
    b_mask = rng.random(n) < 0.6
    for lower, upper in RANGES:
        _check(session, n, src, dst, a_mask, b_mask, lower, upper)


@pytest.mark.parametrize("flat", ["sliced", "flat"])
@pytest.mark.parametrize("words", WORDS)
def test_batch_edges(session, knobs, words, flat):
    """|a_ok| around the batch width 64 W: no source, one, a word's edges, a batch's edges, two batches and a bit --
    scattered ids.  Also through the flat (global OR) level pass."""
    knobs(session, CAPSMI_REACH_WORDS=words, CAPSMI_REACH=flat)
    rng = np.random.default_rng(17)
    n, m = 1500, 6000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    b_mask = rng.random(n) < 0.6
    W = 64 * (8 if words == "auto" else int(words))
    for k in sorted({0, 1, 63, 64, 65, W, W + 1, 2 * W + 3}):
        a_mask = np.zeros(n, bool)
        a_mask[rng.permutation(n)[:k]] = True
        counts, union = _check(session, n, src, dst, a_mask, b_mask, 1, 3)
        if k == 0:
            assert union == 0 and not counts.any()
        _check(session, n, src, dst, a_mask, b_mask, 0, 2)


@pytest.mark.parametrize("words,slices", [("2", 1), ("2", 3), ("8", 1), ("8", 3), ("1", 1)])
@pytest.mark.parametrize("extra", [0, 1, 5])
def test_slice_edges(session, knobs, words, slices, extra):
    """Domains of exactly one target slice, one more id, several slices and five: sources and targets in the top three
    ids of the window, a window that does not start at 0, n no multiple of 64 (extra 1 and 5)."""
    knobs(session, CAPSMI_REACH_WORDS=words)
    w = int(words)
    n = slices * (LDS_WORDS // w) + extra
    lo = 1000
    rng = np.random.default_rng(n)
    m = 4000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    top = np.array([n - 1, n - 2, n - 3])
    src[:60] = rng.choice(top, 60)          # out of the top ids
    dst[60:120] = rng.choice(top, 60)       # into the top ids
    src[120:130], dst[120:130] = top[rng.integers(0, 3, 10)], top[rng.integers(0, 3, 10)]
    a_mask = np.zeros(n, bool)
    a_mask[rng.permutation(n - 3)[: 64 * w + 7]] = True  # more than one batch, and at least w words wide
    a_mask[top] = True
    b_mask = rng.random(n) < 0.5
    b_mask[top[:2]] = True
    for lower, upper in [(1, 3), (0, 4)]:
        _check(session, n, src + lo, dst + lo, a_mask, b_mask, lower, upper, lo=lo)


@pytest.mark.parametrize("reverse", [False, True])
def test_hub(session, reverse):
    """A star whose centre's in-degree is above one partition chunk (8192 pairs), and the reversed star."""
    k = 10_000
    leaves = np.arange(1, k + 1, dtype=np.int64)
    centre = np.zeros(k, dtype=np.int64)
    src, dst = (centre, leaves) if reverse else (leaves, centre)
    ones = np.ones(k + 1, bool)
    a_mask = np.zeros(k + 1, bool)
    a_mask[:: 37] = True
    a_mask[0] = True
    for lower, upper in [(1, 1), (1, 3), (0, 2)]:
        _check(session, k + 1, src, dst, a_mask, ones, lower, upper)


def test_multi_edges_do_not_inflate(session):
    """All relationships are copies of one pair."""
    k = 9000
    src, dst = np.full(k, 3, dtype=np.int64), np.full(k, 5, dtype=np.int64)
    ones = np.ones(8, bool)
    counts, union = _check(session, 8, src, dst, ones, ones, 1, 4)
    assert counts.tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and union == 1


@pytest.mark.parametrize("upper", [39, 40, 41, 10 ** 6])
def test_chain_levels(session, upper):
    """0 -> 1 -> ... -> 40: source a reaches min(upper, 40 - a) nodes; the early exit ends a huge upper."""
    src, dst = np.arange(40, dtype=np.int64), np.arange(1, 41, dtype=np.int64)
    ones = np.ones(41, bool)
    counts, union = _check(session, 41, src, dst, ones, ones, 1, upper)
    assert counts.tolist() == np.minimum(upper, 40 - np.arange(41)).tolist() and union == 40


@pytest.mark.parametrize("upper", [39, 40, 41])
def test_cycle_levels(session, upper):
    """A 40-cycle: a source reaches itself exactly at level 40."""
    src = np.arange(40, dtype=np.int64)
    dst = (src + 1) % 40
    ones = np.ones(40, bool)
    counts, union = _check(session, 40, src, dst, ones, ones, 1, upper)
    assert counts.tolist() == [min(upper, 40)] * 40 and union == 40


def test_zero_length_path_counts_once(session):
    from capsmi import graph
    src, dst = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0, 2], dtype=np.int64)  # a 2-cycle, a self-loop
    for b0 in (True, False):
        b_mask = np.array([b0, True, True])
        a_mask = np.array([True, False, False])
        counts, union = _check(session, 3, src, dst, a_mask, b_mask, 0, 2)
        assert counts.tolist() == [2, 0, 0] and union == 2  # a itself once (through either path), and node 1
    for b2 in (True, False):  # the self-loop-only node, lower = 1: 1 if b_ok, no row otherwise
        b_mask = np.array([True, True, b2])
        a_mask = np.array([False, False, True])
        counts, union = _check(session, 3, src, dst, a_mask, b_mask, 1, 3)
        assert counts.tolist() == [0, 0, 1 if b2 else 0] and union == (1 if b2 else 0)
        a_ok, b_ok = _bitmaps(session, 3, a_mask, b_mask)
        assert graph.var_length_count_distinct(session, [_table(session, src, dst)], a_ok, b_ok, 1, 3).size == (1 if b2 else 0)


def test_empty_b_ok(session):
    rng = np.random.default_rng(4)
    n, m = 200, 900
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    a_mask = rng.random(n) < 0.5
    none = np.zeros(n, bool)
    counts, union = _check(session, n, src, dst, a_mask, none, 1, 3)
    assert not counts.any() and union == 0
    counts, union = _check(session, n, src, dst, a_mask, none, 0, 3)
    assert counts.tolist() == a_mask.astype(int).tolist() and union == int(a_mask.sum())


def test_relationship_tables(session):
    """Two tables whose union is the scan; relationships with an endpoint outside the window are ignored."""
    rng = np.random.default_rng(9)
    n, m, lo = 100, 2000, 50
    src = rng.integers(0, n + 100, m).astype(np.int64)  # absolute ids in [0, 200): the window is [50, 150)
    dst = rng.integers(0, n + 100, m).astype(np.int64)
    a_mask = rng.random(n) < 0.8
    b_mask = rng.random(n) < 0.8
    one = _check(session, n, src, dst, a_mask, b_mask, 1, 3, lo=lo)
    t1, t2 = _table(session, src[:700], dst[:700]), _table(session, src[700:], dst[700:])
    two = _check(session, n, src, dst, a_mask, b_mask, 1, 3, lo=lo, rels=[t1, t2])
    assert one[0].tolist() == two[0].tolist() and one[1] == two[1]
    inside = (src >= lo) & (src < lo + n) & (dst >= lo) & (dst < lo + n)
    kept = _check(session, n, src[inside], dst[inside], a_mask, b_mask, 1, 3, lo=lo)
    assert kept[0].tolist() == one[0].tolist()


@pytest.mark.parametrize("scale", [8, 11])
def test_ldbc_shaped_rmat(session, scale):
    """The C5 generator at small scale: R-MAT (0.45, 0.15, 0.15, 0.25), edge factor 32, all nodes in both masks."""
    from capsmi import graph
    from oracle import cpu
    n, m = 1 << scale, 32 << scale
    rels = graph.rmat_rels(session, scale, 0, m, graph.RMAT_LDBC, 42)
    src, dst = cpu.rmat_edges(scale, 0, m, graph.RMAT_LDBC, 42)
    ones = np.ones(n, dtype=bool)
    for lower, upper in [(1, 3), (1, 6)]:
        _check(session, n, src, dst, ones, ones, lower, upper, rels=[rels])


def test_refusals(session):
    from capsmi import _lib, graph
    src, dst = np.array([0, 1], dtype=np.int64), np.array([1, 2], dtype=np.int64)
    rels = [_table(session, src, dst)]
    ones = np.ones(3, bool)
    a_ok, b_ok = _bitmaps(session, 3, ones, ones)
    for fn in (lambda lo, hi: graph.var_length_count_distinct(session, rels, a_ok, b_ok, lo, hi),
               lambda lo, hi: graph.var_length_reach_count(session, rels, a_ok, b_ok, lo, hi)):
        with pytest.raises(_lib.NotImplementedException, match="join plan"):
            fn(2, 3)
        with pytest.raises(_lib.IllegalArgumentException):
            fn(0, 0)
        with pytest.raises(_lib.IllegalArgumentException):
            fn(1, 0)
    other, _ = _bitmaps(session, 4, np.ones(4, bool), np.ones(4, bool))
    with pytest.raises(_lib.CapsmiError) as mine:
        graph.var_length_count_distinct(session, rels, a_ok, other, 1, 2)
    with pytest.raises(_lib.CapsmiError) as theirs:
        graph.var_length_count(session, rels, a_ok, other, 1, 2)
    assert type(mine.value) is type(theirs.value)


# ---- routed through the planner -------------------------------------------------------------------------
def _graph(session, scale, ef=32, probs=(45, 15, 15), kind="all", rtype="KNOWS"):
    from capsmi import graph
    from capsmi.planner import EntityTable, ScanGraph
    rels = graph.rmat_rels(session, scale, 0, ef << scale, probs, 42)
    k = graph.NODES_ALL if kind == "all" else graph.NODES_PERSON
    nodes = graph.rmat_nodes(session, scale, k, 42)
    props = {"age": 0} if kind == "person" else {}
    return ScanGraph(session, [EntityTable("node", frozenset({"Person"}), props, nodes, id_col="id")],
                     [EntityTable("rel", frozenset({rtype}), {}, rels, id_col="id", src_col="source", dst_col="target")])


def _run(session, sg, q, fused=True):
    from capsmi.planner import Planner, result_rows
    session.set_fused(fused)
    try:
        t, outs = Planner(sg).run(q)
        return result_rows(t, outs, session.dictionary)
    finally:
        session.set_fused(True)


def _routed(session, name, fn):
    before = session.route_count(name)
    out = fn()
    assert session.route_count(name) == before + 1, f"plan not routed to '{name}'"
    return out


def _queries(lo, hi, label="Person", rtype="KNOWS", where=None):
    clause = {"match": f"(a:{label})-[:{rtype}*{lo}..{hi}]->(b:{label})"}
    if where is not None:
        clause["where"] = where
    grouped = {"clauses": [clause], "return": {"items": [["a", ["id", "a"]], ["n", ["count_distinct", ["id", "b"]]]]}}
    alone = {"clauses": [clause], "return": {"items": [["n", ["count_distinct", ["id", "b"]]]]}}
    return grouped, alone


def _want_rows(counts, ids=None):
    return [{"a": int(i if ids is None else ids[i]), "n": int(counts[i])} for i in np.nonzero(counts)[0]]


@pytest.mark.parametrize("lo,hi", [(1, 3), (0, 3), (1, 1), (1, 6), (0, 6)])
def test_routed(session, lo, hi):
    from oracle import cpu
    scale = 8
    sg = _graph(session, scale)
    src, dst = cpu.rmat_edges(scale, 0, 32 << scale, (45, 15, 15), 42)
    ones = np.ones(1 << scale, bool)
    counts, union = reach_sets(1 << scale, src, dst, ones, ones, lo, hi)
    grouped, alone = _queries(lo, hi)
    got = _routed(session, "var_length_distinct", lambda: _run(session, sg, grouped))
    assert same_rows(got, _want_rows(counts))
    if (lo, hi) == (1, 1):
        # one branch and no key is the plain one-hop count(DISTINCT b), which the one-hop route answered before
        # this one existed and still does: the answer is checked, the route's name is not
        assert _run(session, sg, alone) == [{"n": union}]
    else:
        assert _routed(session, "var_length_distinct", lambda: _run(session, sg, alone)) == [{"n": union}]
    if (lo, hi) in ((1, 3), (0, 3)):  # the same plan operator by operator: the reference's plan restated
        assert same_rows(_run(session, sg, grouped, fused=False), _want_rows(counts))
        assert _run(session, sg, alone, fused=False) == [{"n": union}]


def test_routed_with_predicates(session):
    """A label subset (Person = 3/4 of the ids) and a property predicate on a, another on b."""
    from oracle import cpu
    scale = 8
    n = 1 << scale
    sg = _graph(session, scale, kind="person")
    where = ["and", [">=", ["prop", "a", "age"], ["lit", 30]], ["<", ["prop", "b", "age"], ["lit", 60]]]
    src, dst = cpu.rmat_edges(scale, 0, 32 << scale, (45, 15, 15), 42)
    pm = cpu.person_mask(n).astype(bool)
    age = cpu.ages(np.arange(n))
    a_mask, b_mask = pm & (age >= 30), pm & (age < 60)
    for lo, hi in [(1, 3), (1, 5)]:
        counts, union = reach_sets(n, src, dst, a_mask, b_mask, lo, hi)
        grouped, alone = _queries(lo, hi, where=where)
        got = _routed(session, "var_length_distinct", lambda: _run(session, sg, grouped))
        assert same_rows(got, _want_rows(counts))
        assert _routed(session, "var_length_distinct", lambda: _run(session, sg, alone)) == [{"n": union}]
        if hi == 3:
            assert same_rows(_run(session, sg, grouped, fused=False), _want_rows(counts))


def test_routed_on_sparse_ids(session):
    """Ids near 2^40, compacted: the dense remap gives the original ids back."""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    rng = np.random.default_rng(5)
    ids = np.unique(rng.integers(1 << 40, (1 << 40) + (1 << 45), 800))
    n, m = len(ids), 6000
    s_i, d_i = rng.integers(0, n, m), rng.integers(0, n, m)
    s_i[: m // 50] = d_i[: m // 50]
    nodes = session.table([ColumnData("id", I64, ids)]).as_node_table("id")
    rels = session.table([ColumnData("id", I64, np.arange(m, dtype=np.int64) * 3 + (1 << 50)),
                          ColumnData("source", I64, ids[s_i]), ColumnData("target", I64, ids[d_i])]).as_rel_table(
        "id", "source", "target")
    assert session.compact_if_sparse([nodes], [rels])
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    ones = np.ones(n, bool)
    counts, union = reach_sets(n, s_i, d_i, ones, ones, 1, 4)
    grouped, alone = _queries(1, 4, label="N", rtype="R")
    got = _routed(session, "var_length_distinct", lambda: _run(session, sg, grouped))
    assert same_rows(got, _want_rows(counts, ids))
    assert _routed(session, "var_length_distinct", lambda: _run(session, sg, alone)) == [{"n": union}]


def test_lower_two_is_not_routed(session):
    sg = _graph(session, 6)
    clause = {"match": "(a)-[:KNOWS*2..3]->(b)"}
    for items in ([["a", ["id", "a"]], ["n", ["count_distinct", ["id", "b"]]]], [["n", ["count_distinct", ["id", "b"]]]]):
        q = {"clauses": [clause], "return": {"items": items}}
        before = session.route_count("var_length_distinct")
        got = _run(session, sg, q)
        assert session.route_count("var_length_distinct") == before
        assert same_rows(got, _run(session, sg, q, fused=False))


def test_scale_12_answers_where_the_join_plan_is_refused(session):
    """R-MAT LDBC scale 12, *1..6 grouped, under the unrouted limit of the routing tests: the join plan is refused by
    the guard (as it was for this query before the route existed); the route answers."""
    from capsmi import _lib
    from oracle import cpu
    scale = 12
    n = 1 << scale
    sg = _graph(session, scale)
    grouped, _ = _queries(1, 6)
    session.set_unrouted_limit(1 << 30)
    try:
        with pytest.raises(_lib.UnsupportedOperationException, match="estimated"):
            _run(session, sg, grouped, fused=False)
        got = _routed(session, "var_length_distinct", lambda: _run(session, sg, grouped))
    finally:
        session.set_unrouted_limit(0)
    src, dst = cpu.rmat_edges(scale, 0, 32 << scale, (45, 15, 15), 42)
    ones = np.ones(n, bool)
    counts, _ = reach_sets(n, src, dst, ones, ones, 1, 6)
    assert same_rows(got, _want_rows(counts))
