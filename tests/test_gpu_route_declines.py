"""Where the two var-length routes ("var_length": grouped count(*) by the start node; "var_length_distinct": count /
collect(DISTINCT end node)) stop: each plan here sits just outside one route's preconditions, or just inside, on a graph
of 64 nodes and 256 relationships.  A declined plan moves no route's counter, runs operator by operator and counts as
a "miss"; a routed one counts its route once and nothing else.  Either way the rows are those of the same plan with
the fused routes switched off.

"miss" counts materialisations that ran a pattern unrouted, and a sub-plan with two parents is materialised on its
own, in place: in the plan of `*l..2` the chain of one hop feeds both the length-1 branch and the second hop, so a
declined `*0..2` or `*1..2` plan counts two misses (MISSES), the chain's and its own.

The pattern language writes a var-length hop as `*l..u`, so lengths with a gap (1 and 3 without 2) cannot be asked
for, and the hops' interior nodes have no name a WHERE could use: the interior case is the one the language can
express, a node scan (with a label and a property predicate) at an interior position of every branch."""
import numpy as np
import pytest

from golden_util import same_rows

pytestmark = pytest.mark.gpu

SCALE, EF = 6, 4  # R-MAT: 64 nodes, 256 relationships per type
VARLEN = ("var_length", "var_length_distinct")
ROUTES = ("expand", "expand_count", "two_hop", "two_hop_grouped", "undirected", "triangle", "triangle_grouped",
          "triangle_transitive", "triangle_transitive_grouped", "triangle_undirected", "triangle_undirected_grouped",
          "var_length", "var_length_distinct", "miss")


def _graph(session, scale=SCALE, ef=EF, probs=(45, 15, 15), kind="all", second_type=None):
    from capsmi import graph
    from capsmi.planner import EntityTable, ScanGraph
    k = graph.NODES_ALL if kind == "all" else graph.NODES_PERSON
    nodes = graph.rmat_nodes(session, scale, k, 42)
    props = {"age": 0} if kind == "person" else {}
    rels = [("KNOWS", graph.rmat_rels(session, scale, 0, ef << scale, probs, 42))]
    if second_type:
        rels.append((second_type, graph.rmat_rels(session, scale, 0, ef << scale, probs, 7)))
    return ScanGraph(session, [EntityTable("node", frozenset({"Person"}), props, nodes, id_col="id")],
                     [EntityTable("rel", frozenset({t}), {}, r, id_col="id", src_col="source", dst_col="target")
                      for t, r in rels])


def _run(session, sg, q, fused=True):
    from capsmi.planner import Planner, result_rows
    session.set_fused(fused)
    try:
        t, outs = Planner(sg).run(q)
        return result_rows(t, outs, session.dictionary)
    finally:
        session.set_fused(True)


def _routes(session):
    return {r: session.route_count(r) for r in ROUTES}


def _rose(session, before):
    return {r: v - before[r] for r, v in _routes(session).items() if v != before[r]}


def _routed(session, sg, q, name):
    """`q` takes route `name`, once, and no other; its rows are the operator path's"""
    before = _routes(session)
    got = _run(session, sg, q)
    assert _rose(session, before) == {name: 1}, f"plan not routed to '{name}'"
    want = _run(session, sg, q, fused=False)
    assert len(want) > 0 and same_rows(got, want)
    return got


MISSES = 2  # of a declined `*l..2` plan (see above)


def _declined(session, sg, q):
    """no route takes `q`, the var-length ones least of all: the plan's misses, and the operator path's rows"""
    before = _routes(session)
    got = _run(session, sg, q)
    rose = _rose(session, before)
    assert not set(rose) & set(VARLEN), f"routed: {rose}"
    assert rose == {"miss": MISSES}, rose
    want = _run(session, sg, q, fused=False)
    assert len(want) > 0 and same_rows(got, want)
    return got


def _q(pattern, items, where=None):
    clause = {"match": pattern}
    if where is not None:
        clause["where"] = where
    return {"clauses": [clause], "return": {"items": [list(i) for i in items]}}


A, B = ("a", ["id", "a"]), ("b", ["id", "b"])
STAR = ("n", ["count*"])
COUNT_B = ("n", ["count", ["id", "b"]])
DISTINCT_A = ("n", ["count_distinct", ["id", "a"]])
DISTINCT_B = ("n", ["count_distinct", ["id", "b"]])
COLLECT_B = ("ds", ["collect_distinct", ["id", "b"]])


def _pat(lo, hi, label="Person", rtype="KNOWS"):
    return f"(a:{label})-[:{rtype}*{lo}..{hi}]->(b:{label})"


def test_zero_length_branch_takes_count_star_only(session):
    """*0..2 grouped by the start: count(*) is routed, count(b) -- the same numbers -- is not"""
    sg = _graph(session)
    star = _routed(session, sg, _q(_pat(0, 2), [A, STAR]), "var_length")
    col = _declined(session, sg, _q(_pat(0, 2), [A, COUNT_B]))
    assert same_rows(star, col)


def test_one_up_count_of_a_column_is_routed(session):
    """without the zero-length branch count(b) of the non-null end is count(*)"""
    sg = _graph(session)
    _routed(session, sg, _q(_pat(1, 2), [A, COUNT_B]), "var_length")


def test_key_at_the_end_is_declined_by_both(session):
    sg = _graph(session)
    _declined(session, sg, _q(_pat(1, 2), [B, STAR]))
    _declined(session, sg, _q(_pat(1, 2), [B, ("n", ["count_distinct", ["id", "a"]])]))
    _declined(session, sg, _q(_pat(1, 2), [B, ("n", ["count_distinct", ["id", "b"]])]))


def test_distinct_of_the_start_is_declined(session):
    """count(DISTINCT a) keyed by a: the counted column is not the end node's"""
    sg = _graph(session)
    got = _declined(session, sg, _q(_pat(1, 2), [A, DISTINCT_A]))
    assert {r["n"] for r in got} == {1}
    _declined(session, sg, _q(_pat(0, 2), [A, DISTINCT_A]))


@pytest.mark.parametrize("agg", [STAR, ("n", ["count_distinct", ["id", "c"]])], ids=["count_star", "count_distinct"])
def test_scanned_interior_position_is_declined(session, agg):
    """(a)-[:KNOWS*1..2]->(b)-[:LIKES]->(c): chains of 2 and 3 hops whose position before the last is node-scanned,
    labelled and filtered, and whose last hop reads another relationship set"""
    sg = _graph(session, kind="person", second_type="LIKES")
    pattern = "(a:Person)-[:KNOWS*1..2]->(b:Person)-[:LIKES]->(c:Person)"
    where = [">=", ["prop", "b", "age"], ["lit", 30]]
    _declined(session, sg, _q(pattern, [A, agg], where))


def test_three_lengths_with_end_predicates_are_routed(session):
    """*1..3 with predicates on both ends only: both routes take it"""
    sg = _graph(session, kind="person")
    where = ["and", [">=", ["prop", "a", "age"], ["lit", 30]], ["<", ["prop", "b", "age"], ["lit", 60]]]
    _routed(session, sg, _q(_pat(1, 3), [A, STAR], where), "var_length")
    _routed(session, sg, _q(_pat(1, 3), [A, DISTINCT_B], where), "var_length_distinct")


def test_two_aggregates_of_one_kind_are_declined(session):
    sg = _graph(session)
    two = [A, ("n", ["count_distinct", ["id", "b"]]), ("m", ["count_distinct", ["id", "b"]])]
    got = _declined(session, sg, _q(_pat(1, 2), two))
    assert all(r["n"] == r["m"] for r in got)
    _declined(session, sg, _q(_pat(1, 2), two[1:]))
    lists = [A, ("ds", ["collect_distinct", ["id", "b"]]), ("es", ["collect_distinct", ["id", "b"]])]
    _declined(session, sg, _q(_pat(1, 2), lists))


@pytest.mark.parametrize("lo", [0, 1])
@pytest.mark.parametrize("order", ["count_first", "collect_first"])
def test_count_and_collect_follow_the_aggregates(session, order, lo):
    """one count(DISTINCT b) and one collect(DISTINCT b), in both orders, keyed and alone"""
    sg = _graph(session)
    aggs = [DISTINCT_B, COLLECT_B] if order == "count_first" else [COLLECT_B, DISTINCT_B]
    got = _routed(session, sg, _q(_pat(lo, 2), [A] + aggs), "var_length_distinct")
    assert all(r["n"] == len(r["ds"]) and r["ds"] == sorted(set(r["ds"])) for r in got)
    alone = _routed(session, sg, _q(_pat(lo, 2), aggs), "var_length_distinct")
    assert len(alone) == 1 and alone[0]["n"] == len(alone[0]["ds"])


def _sparse_graph(session):
    """64 ids near 2^40 and 256 relationships, compacted"""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    rng = np.random.default_rng(5)
    ids = np.unique(rng.integers(1 << 40, (1 << 40) + (1 << 45), 64))
    n, m = len(ids), 256
    s_i, d_i = rng.integers(0, n, m), rng.integers(0, n, m)
    s_i[:6] = d_i[:6]  # self-loops
    nodes = session.table([ColumnData("id", I64, ids)]).as_node_table("id")
    rels = session.table([ColumnData("id", I64, np.arange(m, dtype=np.int64) * 3 + (1 << 50)),
                          ColumnData("source", I64, ids[s_i]), ColumnData("target", I64, ids[d_i])]).as_rel_table(
        "id", "source", "target")
    assert session.compact_if_sparse([nodes], [rels])
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    return sg, ids


def test_compacted_graph_returns_the_original_ids_from_both_routes(session):
    """*1..3 on a compacted graph: the grouped count(*) and the grouped count(DISTINCT b) name the same start nodes,
    by their original ids"""
    sg, ids = _sparse_graph(session)
    star = _routed(session, sg, _q(_pat(1, 3, "N", "R"), [A, STAR]), "var_length")
    dist = _routed(session, sg, _q(_pat(1, 3, "N", "R"), [A, DISTINCT_B]), "var_length_distinct")
    starts = sorted(r["a"] for r in star)
    assert starts == sorted(r["a"] for r in dist) and len(starts) == len(set(starts))
    assert set(starts) <= set(ids.tolist())
    paths = {r["a"]: r["n"] for r in star}
    assert all(1 <= r["n"] <= paths[r["a"]] for r in dist)
