"""MonotonicallyIncreasingId on the device (CAPSMI_X_ROW_ID, k_expr.hip) and the plan executor's rules for the node
that holds it (plan.hip): the value is the index of the row in the table the withColumns reads, whatever else the
program holds; the node is pinned -- no filter below it, computed whole and once, its rows kept, never part of a fused
pattern; and CONSTRUCT through the planner mirror (capsmi/construct.py) against the pure-Python restatement of
construct_ref.py.  Expected ids are numpy.arange over the rows in the order the table exports."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# around one block of 256 rows, many blocks, and more rows than the grid of 8192 blocks of 256 lanes covers in one
# stride (2 097 152): the second iteration of k_eval's grid-stride loop
SIZES = (0, 1, 255, 256, 257, 70001, 8192 * 256 * 2 + 77)


def _rid():
    from capsmi.expr import MonotonicallyIncreasingId
    return MonotonicallyIncreasingId()


def _longs(session, **cols):
    from capsmi import ColumnData, I64
    return session.table([ColumnData(k, I64, np.asarray(v, dtype=np.int64)) for k, v in cols.items()])


def _col(t, name):
    c = t.column(name)
    assert c.valid is None or np.asarray(c.valid, dtype=bool).all(), f"{name} holds NULLs"
    return np.ascontiguousarray(c.values).astype(np.int64)


def _launches(session, name="expr_eval"):
    from capsmi import _lib
    n, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", session.handle, name.encode(), ctypes.byref(n), ctypes.byref(ms))
    return n.value


@pytest.fixture
def fresh():
    from capsmi import Session
    s = Session(0)
    yield s
    s.close()


# ---- the opcode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_row_id_is_arange(session, n):
    from capsmi import I64
    t = _longs(session, x=np.arange(n)[::-1]).withColumns((_rid(), "i"))
    assert t.columnType["i"] == I64 and t.size == n
    assert np.array_equal(_col(t, "i"), np.arange(n))
    assert np.array_equal(_col(t, "x"), np.arange(n)[::-1])


def test_row_id_under_the_id_formula(session):
    """generateId(k = 2 of n = 3 created entities).setTag(5): ADD, BITAND, BITOR and SHL around the row index."""
    from capsmi import tagging
    from capsmi.expr import BinOp, Lit
    n = 1000
    e = tagging.expr_set_tag(BinOp("+", _rid(), Lit(2 << 31)), 5)
    got = _col(_longs(session, x=np.zeros(n)).withColumns((e, "id")), "id")
    assert got.tolist() == [tagging.set_tag(r + (2 << 31), 5) for r in range(n)]
    assert {tagging.get_tag(int(v)) for v in got} == {5}


def test_row_id_after_filter_skip_limit_union_and_join(session):
    """Below the pinned node anything may stand: the ids count the rows the operator reads."""
    from capsmi.expr import BinOp, Col, Lit
    n = 5000
    x = (np.arange(n) * 7919) % 1000
    base = _longs(session, k=np.arange(n), x=x)
    keep = x >= 300
    f = base.filter(BinOp(">=", Col("x"), Lit(300))).withColumns((_rid(), "i"))
    assert np.array_equal(_col(f, "i"), np.arange(keep.sum())) and np.array_equal(_col(f, "k"), np.arange(n)[keep])
    s = base.skip(37).withColumns((_rid(), "i"))
    assert np.array_equal(_col(s, "i"), np.arange(n - 37)) and np.array_equal(_col(s, "k"), np.arange(37, n))
    lim = base.limit(300).withColumns((_rid(), "i"))
    assert np.array_equal(_col(lim, "i"), np.arange(300)) and np.array_equal(_col(lim, "k"), np.arange(300))
    u = base.unionAll(base.limit(11)).withColumns((_rid(), "i"))
    assert np.array_equal(_col(u, "i"), np.arange(n + 11))
    assert np.array_equal(_col(u, "k"), np.concatenate([np.arange(n), np.arange(11)]))
    other = _longs(session, k2=np.arange(0, n, 3), y=np.arange(0, n, 3) * 2)
    j = base.join(other, "inner", ("k", "k2")).withColumns((_rid(), "i"))
    m = len(range(0, n, 3))
    assert np.array_equal(_col(j, "i"), np.arange(m))
    assert sorted(_col(j, "k").tolist()) == list(range(0, n, 3)) and np.array_equal(_col(j, "y"), _col(j, "k") * 2)


def test_row_id_on_a_64_column_table(session):
    from capsmi.expr import BinOp, Col
    n = 300
    t = _longs(session, **{f"c{q}": np.full(n, q) for q in range(64)})
    out = t.withColumns((BinOp("+", _rid(), Col("c63")), "i"), (_rid(), "c0"))
    assert np.array_equal(_col(out, "i"), np.arange(n) + 63)
    assert np.array_equal(_col(out, "c0"), np.arange(n))  # a replaced column
    assert np.array_equal(_col(out, "c62"), np.full(n, 62))


def test_row_id_beside_the_nodes_that_run_as_passes_of_their_own(fresh):
    """STARTS WITH and toString() are lowered to columns of a view of the table before the interpreter runs: the view
    keeps the rows, so the ids are the ones a program without them gives.  / 2 takes the kMath instantiation."""
    from capsmi import ColumnData, expr
    from capsmi.expr import BinOp, Case, Col, Lit, StartsWith, ToString
    s = fresh
    n = 777
    words = [None if r % 5 == 4 else ("ab" if r % 2 else "ba") + str(r % 3) for r in range(n)]
    s.dictionary.extend(sorted({w for w in words if w is not None}) + ["a"])
    codes = np.array([0 if w is None else s.dictionary.encode(w) for w in words], dtype=np.int64)
    t = s.table([ColumnData("w", expr.STR, codes, np.array([w is not None for w in words], dtype=bool))])
    e = Case(((StartsWith(Col("w"), Lit("a")), _rid()),), BinOp("+", _rid(), Lit(100000)))
    out = t.withColumns((e, "i"), (BinOp("/", _rid(), Lit(2)), "h"), (ToString(_rid()), "txt"), (_rid(), "plain"))
    want = [r if (words[r] is not None and words[r].startswith("a")) else r + 100000 for r in range(n)]
    assert _col(out, "i").tolist() == want
    assert np.array_equal(_col(out, "h"), np.arange(n) // 2)
    assert np.array_equal(_col(out, "plain"), np.arange(n))
    assert out.columnType["txt"] == expr.STR
    assert [s.dictionary.decode(int(c)) for c in _col(out, "txt")] == [str(r) for r in range(n)]


def test_row_id_is_refused_outside_with_columns(session):
    from capsmi import _lib, graph
    from capsmi.expr import BinOp, Lit
    t = _longs(session, id=np.arange(10))
    pred = BinOp(">", _rid(), Lit(3))
    with pytest.raises(_lib.IllegalArgumentException, match="CAPSMI_X_ROW_ID in a capsmi_filter predicate"):
        t.filter(pred)
    with pytest.raises(_lib.IllegalArgumentException, match="CAPSMI_X_ROW_ID in a capsmi_with_range_column operand"):
        t.withRangeColumn(_rid(), 5, None, "l")
    with pytest.raises(_lib.IllegalArgumentException, match="CAPSMI_X_ROW_ID in a capsmi_with_range_column operand"):
        t.withRangeColumn(0, 5, BinOp("+", _rid(), Lit(1)), "l")
    with pytest.raises(_lib.IllegalArgumentException, match="CAPSMI_X_ROW_ID in a capsmi_bitmap_add_scan predicate"):
        graph.NodeBitmap(session, 0, 10).add_scan(t.as_node_table("id"), "id", pred)
    # and the withColumns beside them is taken
    assert np.array_equal(_col(t.withColumns((pred, "p")), "p"), (np.arange(10) > 3).astype(np.int64))


def test_row_id_on_a_session_of_two_ranks_is_refused_when_built(fresh):
    """World size 1 with a collective set runs; world 2 refuses the node when it is built (no collective is called)."""
    from capsmi import _lib
    from capsmi.expr import BinOp, Col, Lit
    calls = []
    fresh.set_ranks(0, 1, lambda *a: calls.append(a))
    t = _longs(fresh, x=np.arange(5))
    assert np.array_equal(_col(t.withColumns((_rid(), "i")), "i"), np.arange(5))
    fresh.set_ranks(0, 2, lambda *a: calls.append(a))
    with pytest.raises(_lib.UnsupportedOperationException, match="distributed CONSTRUCT is not implemented"):
        t.withColumns((_rid(), "i"))
    t.withColumns((BinOp("+", Col("x"), Lit(1)), "y"))  # a program without the opcode is still built
    assert calls == []
    fresh.set_ranks(0, 1, None)


# ---- the plan rules ----------------------------------------------------------------------------------
def test_rule_1_no_filter_is_pushed_below_a_pinned_node(session):
    """The filter reads none of the node's new columns, and drops early rows: pushed down, i would be 0..m-1."""
    from capsmi.expr import BinOp, Col, Lit
    n, k = 4000, 1500
    t = _longs(session, x=np.arange(n), pay=np.arange(n) * 3)
    out = t.withColumns((_rid(), "i")).filter(BinOp(">", Col("x"), Lit(k)))
    assert np.array_equal(_col(out, "i"), np.arange(k + 1, n))
    assert np.array_equal(_col(out, "pay"), np.arange(k + 1, n) * 3)
    # two conjuncts, one over the new column: neither goes below
    both = t.withColumns((_rid(), "i")).filter(BinOp(">", Col("x"), Lit(k))).filter(BinOp("<", Col("i"), Lit(k + 10)))
    assert np.array_equal(_col(both, "i"), np.arange(k + 1, k + 10))


def test_rules_2_and_3_a_pinned_node_is_computed_whole_once_and_keeps_its_rows(session):
    """Two actions over one pinned node read disjoint column subsets.  The first computes the node whole (its other
    program too, which the first action does not read); the second launches no interpreter for the node's programs and
    sees the same ids, row for row, joined back on the payload key."""
    from capsmi import _lib
    from capsmi.expr import BinOp, Col, Lit
    n = 3000
    key = (np.arange(n) * 7 + 3) % n  # a permutation: n and 7 are coprime
    left = _longs(session, key=key, a=key * 2)
    right = _longs(session, key2=np.arange(n), b=np.arange(n) + 5)
    joined = left.join(right, "inner", ("key", "key2"))  # an input whose row order is the join's business
    pinned = joined.withColumns((_rid(), "i"), (BinOp("*", Col("b"), Lit(10)), "b10"))
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        _launches(session)  # reset
        first = pinned.select("i", "key")
        i1, k1 = _col(first, "i"), _col(first, "key")
        assert _launches(session) >= 2  # both programs of the node, though the action reads one
        second = pinned.withColumns((Col("i"), "j")).select("j", "key")
        j2, k2 = _col(second, "j"), _col(second, "key")
        third = pinned.select("b10", "i")
        b3, i3 = _col(third, "b10"), _col(third, "i")
        assert _launches(session) <= 1  # at most the copy j = i: nothing of the pinned node runs again
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)
    assert np.array_equal(i1, np.arange(n)) and sorted(k1.tolist()) == list(range(n))
    by_key = dict(zip(k1.tolist(), i1.tolist()))
    assert [by_key[k] for k in k2.tolist()] == j2.tolist()
    assert np.array_equal(i3, np.arange(n))
    assert b3.tolist() == [(k1[r] + 5) * 10 for r in range(n)]  # the third action's rows are the first's rows


def _rel_graph(session, n=500, m=4000, seed=5):
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    nodes = session.table([ColumnData("id", I64, np.arange(n, dtype=np.int64))]).as_node_table("id")
    rels = session.table([ColumnData("id", I64, np.arange(m, dtype=np.int64) + (1 << 20)), ColumnData("source", I64, src),
                          ColumnData("target", I64, dst)]).as_rel_table("id", "source", "target")
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    return sg, src, dst


def test_rule_4_a_pinned_node_over_a_routed_expand_is_no_part_of_the_pattern(session):
    """MATCH (a:N)-[r:R]->(b:N) below a pinned node still takes the fused Expand route, once; the node itself and what
    stands above it run operator by operator, and a second action routes nothing."""
    from capsmi.expr import BinOp, Col, Lit
    from capsmi.planner import Planner
    sg, src, dst = _rel_graph(session)
    q = {"clauses": [{"match": "(a:N)-[r:R]->(b:N)"}],
         "return": {"items": [["a", ["id", "a"]], ["r", ["id", "r"]], ["b", ["id", "b"]]]}}
    t, outs = Planner(sg).run(q)
    a, r, b = (o[2] for o in outs)
    before, missed, counted = (session.route_count(x) for x in ("expand", "miss", "expand_count"))
    pinned = t.withColumns((_rid(), "i"))
    m = len(src)
    # count(*) over the node: as part of the pattern it would be the fused count, and the node never computed
    assert _col(pinned.group([], [("count_star", None, False, "n")]), "n").tolist() == [m]
    assert session.route_count("expand") == before + 1 and session.route_count("expand_count") == counted
    above = pinned.filter(BinOp(">=", Col("i"), Lit(0))).select(a, r, b, "i")
    assert np.array_equal(_col(above, "i"), np.arange(m))
    assert session.route_count("expand") == before + 1 and session.route_count("miss") == missed
    rid = _col(above, r) - (1 << 20)
    assert sorted(rid.tolist()) == list(range(m))
    assert np.array_equal(_col(above, a), src[rid]) and np.array_equal(_col(above, b), dst[rid])
    again = pinned.select("i", r)
    assert np.array_equal(_col(again, r), _col(above, r)) and session.route_count("expand") == before + 1


# ---- CONSTRUCT through the planner mirror -------------------------------------------------------------
import construct_ref as cr  # noqa: E402
from golden_util import load_cases  # noqa: E402

CASES = load_cases("construct.json")


def _entities(session, g):
    """The graph's nodes and relationships as PGNode / PGRel, read through its own scans."""
    from capsmi.planner import PGNode, PGRel, result_rows
    t, h = g.node_scan("n", [])
    assert t.physicalColumns == h
    rows = result_rows(t, [("entity", "n", (False, [(c[1:], c) for c in h]))], session.dictionary)
    nodes = [PGNode(r["n"]["id"], frozenset(r["n"]["labels"]), r["n"]["props"]) for r in rows]
    t, h = g.rel_scan("r", [])
    assert t.physicalColumns == h
    rows = result_rows(t, [("entity", "r", (True, [(c[1:], c) for c in h]))], session.dictionary)
    rels = [PGRel(r["r"]["id"], r["r"]["src"], r["r"]["dst"], r["r"]["type"], r["r"]["props"]) for r in rows]
    return nodes, rels


def _device_case(session, case):
    from capsmi.planner import Planner, ScanGraph, UnionGraph, result_rows
    catalog = {name: ScanGraph.from_property_graph(session, pg) for name, pg in cr.case_graphs(case).items()}
    ambient = case.get("ambient")
    if ambient is None:
        g = ScanGraph(session, [], [])  # the session's empty graph
    elif isinstance(ambient, list):
        g = UnionGraph.union_all(session, *[catalog[a] for a in ambient])
    else:
        g = catalog[ambient]
    p = Planner(g, catalog)
    out, outs = p.run(case["query"])
    strategies = [{str(k): v for k, v in s.items()} for s in p.tag_strategies]
    if case["query"]["return"] == "graph":
        nodes, rels = _entities(session, out)
        return {"tags": sorted(out.tags), "nodes": nodes, "rels": rels, "strategies": strategies}
    return {"rows": result_rows(out, outs, session.dictionary), "strategies": strategies}


def _same_graph_up_to_created_ids(got, ref, created_tags):
    """Cloned ids exact; created ids as a set exact, and the graph equal up to a bijection of them that keeps the tag and
    is applied to node ids and relationship endpoints alike."""
    assert sorted(n.id for n in got["nodes"]) == sorted(n.id for n in ref["nodes"])
    assert sorted(r.id for r in got["rels"]) == sorted(r.id for r in ref["rels"])
    assert cr.canonical(got["nodes"], got["rels"], created_tags) == cr.canonical(ref["nodes"], ref["rels"], created_tags)
    assert sorted(got["tags"]) == sorted(ref["tags"])


@pytest.mark.parametrize("fused", [True, False], ids=["routed", "unfused"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_case_on_the_device(session, case, fused):
    session.set_fused(fused)
    try:
        got = _device_case(session, case)
    finally:
        session.set_fused(True)
    cr.assert_graph(got, case["expected"])  # what the reference's test states: pinned ids and tags exact
    ref = cr.run_case(case)
    # the construct tag strategies; a graph the session made has a generated name on either side
    assert [sorted(s.values(), key=repr) for s in got["strategies"]] == [sorted(s.values(), key=repr) for s in ref["strategies"]]
    for want in ([case["expected"]["strategy"]] if "strategy" in case["expected"] else []):
        assert {k: {str(f): t for f, t in v.items()} for k, v in got["strategies"][-1].items()} == want
    if "rows" not in case["expected"]:
        created = set(got["tags"]) - {t for s in got["strategies"][-1:] for m in s.values() for t in m.values()}
        _same_graph_up_to_created_ids(got, ref, created)


class _Tags:
    def __init__(self, tags=(0,)):
        self.tags = frozenset(tags)
        self.pg = None


def _bindings_table(session, rows, node_cols, rel_cols=None):
    """A bindings table: per node variable v its id, one flag per label and one Long column per key (NULL where the row
    binds no node); per relationship variable r its id, __src, __dst, __type and one Long column per key.
    node_cols: {v: (labels, keys)}; rel_cols: {r: keys}."""
    from capsmi import BOOL, ColumnData, I64, STR
    cols, header = [], []
    for v, keys in (rel_cols or {}).items():
        ents = [r[v] for r in rows]
        session.dictionary.extend(sorted({e.type for e in ents}))
        cols += [ColumnData(v, I64, np.array([e.id for e in ents], dtype=np.int64)),
                 ColumnData(f"{v}.__src", I64, np.array([e.src for e in ents], dtype=np.int64)),
                 ColumnData(f"{v}.__dst", I64, np.array([e.dst for e in ents], dtype=np.int64)),
                 ColumnData(f"{v}.__type", STR, np.array([session.dictionary.encode(e.type) for e in ents], dtype=np.int64))]
        cols += [ColumnData(f"{v}.{k}", I64, np.array([e.props[k] for e in ents], dtype=np.int64)) for k in keys]
        header += [v, f"{v}.__src", f"{v}.__dst", f"{v}.__type"] + [f"{v}.{k}" for k in keys]
    for v, (labels, keys) in node_cols.items():
        ents = [r.get(v) for r in rows]
        ok = np.array([e is not None for e in ents], dtype=bool)
        valid = None if ok.all() else ok
        cols.append(ColumnData(v, I64, np.array([0 if e is None else e.id for e in ents], dtype=np.int64), valid))
        for l in labels:
            cols.append(ColumnData(f"{v}:{l}", BOOL, np.array([0 if e is None else int(l in e.labels) for e in ents], dtype=np.int64), valid))
        for k in keys:
            has = np.array([e is not None and e.props.get(k) is not None for e in ents], dtype=bool)
            cols.append(ColumnData(f"{v}.{k}", I64, np.array([0 if not h else e.props[k] for e, h in zip(ents, has)], dtype=np.int64),
                                   None if has.all() else has))
        header += [v] + [f"{v}:{l}" for l in labels] + [f"{v}.{k}" for k in keys]
    return session.table(cols), header


def _edge_construct(session, rows, node_cols, spec):
    """plan_construct over hand-made bindings against the restatement over the same rows."""
    from capsmi.construct import plan_construct
    table, header = _bindings_table(session, rows, node_cols)
    graph_of = {v: "g" for v in node_cols}
    catalog = {"g": _Tags()}
    graph, pattern, strategy = plan_construct(session, table, header, set(node_cols), [], graph_of, spec, catalog)
    nodes, rels = _entities(session, graph)
    ref, _, created = cr.construct(rows, {v: "node" for v in node_cols}, graph_of, spec, catalog)
    got = {"tags": sorted(graph.tags), "nodes": nodes, "rels": rels}
    _same_graph_up_to_created_ids(got, {"tags": sorted(ref.tags), "nodes": ref.pg.nodes, "rels": ref.pg.rels},
                                  set() if created is None else {created})
    return got, pattern, created


def _nodes(n, labels=("L",), first=0):
    from capsmi.planner import PGNode
    return [PGNode(first + i, frozenset(labels if i % 2 else labels[:1]), {"v": i * 3}) for i in range(n)]


def test_copy_of_a_null_base_is_no_entity(session):
    """300 bindings, every third base NULL (an OPTIONAL MATCH miss): no copy and no relationship for those rows."""
    a, b = _nodes(300), _nodes(300, ("L", "M"), 1000)
    rows = [{"a": a[i], "b": None if i % 3 == 2 else b[i]} for i in range(300)]
    spec = {"clones": [["a", "a"]], "creates": [{"node": "c", "labels": ["K"], "copy_of": "b"},
                                                 {"rel": "e", "src": "a", "dst": "c", "type": "T"}]}
    got, _, created = _edge_construct(session, rows, {"a": (["L"], ["v"]), "b": (["L", "M"], ["v"])}, spec)
    copies = [n for n in got["nodes"] if cr.get_tag(n.id) == created]
    assert len(copies) == 200 == len(got["rels"]) and len(got["nodes"]) == 500
    assert all("K" in n.labels and "L" in n.labels for n in copies)
    assert sorted(n.id & cr.ID_MASK for n in copies) == [i for i in range(300) if i % 3 != 2]  # the row index counts every row


def test_a_variable_cloned_under_two_aliases_and_a_self_loop(session):
    a = _nodes(40)
    rows = [{"a": a[i % 40]} for i in range(100)]  # every node bound two or three times
    spec = {"clones": [["x", "a"], ["y", "a"]], "creates": [{"rel": "e", "src": "x", "dst": "x", "type": "LOOP"},
                                                           {"rel": "f", "src": "x", "dst": "y", "type": "SAME"}]}
    got, pattern, created = _edge_construct(session, rows, {"a": (["L"], ["v"])}, spec)
    assert pattern.node_vars == ["x", "y"] and sorted(pattern.rel_vars) == ["e", "f"]
    assert len(got["nodes"]) == 40 and len(got["rels"]) == 200  # one copy of a node, a relationship per binding
    assert all(r.src == r.dst for r in got["rels"])
    t, h = pattern.node_scan("n", ["L"])  # no distinct across the variables (SingleTableGraph.scala:99-105)
    assert h == ["n", "n:L", "n.v"] and t.size == 80


def test_nine_created_nodes_change_the_offset_shift(session):
    """n = 9 created nodes: floor(ln 9) + 1 = 3 bits, the shift the reference takes from n = 8 on."""
    rows = [{"a": x} for x in _nodes(5)]
    spec = {"clones": [], "creates": [{"node": f"n{k}", "labels": [f"K{k % 2}"]} for k in range(9)]}
    got, _, created = _edge_construct(session, rows, {"a": (["L"], ["v"])}, spec)
    assert created == 0 and got["tags"] == [0]
    assert sorted(n.id for n in got["nodes"]) == sorted((k << 30) + r for k in range(9) for r in range(5))
    assert cr.id_offset(7, 8) == 7 << 30 and cr.id_offset(6, 7) == 6 << 31


def test_an_empty_binding_table_gives_an_empty_graph(session):
    from capsmi import BOOL, I64, STR
    spec = {"clones": [["a", "a"]], "creates": [{"node": "c", "labels": ["K"], "copy_of": "a"},
                                                 {"rel": "e", "src": "a", "dst": "c", "type": "T"}],
            "sets": [["prop", "e", "w", ["prop", "a", "v"]]]}
    got, pattern, _ = _edge_construct(session, [], {"a": (["L"], ["v"])}, spec)
    assert got["nodes"] == [] and got["rels"] == [] and got["tags"] == [0, 1]
    t, h = pattern.node_scan("n", [])
    assert h == ["n", "n:K", "n:L", "n.v"] == t.physicalColumns and t.size == 0
    assert [t.columnType[c] for c in h] == [I64, BOOL, BOOL, I64]
    t, h = pattern.rel_scan("r", ["T"])
    assert h == ["r", "r.__src", "r.__dst", "r.__type", "r.w"] == t.physicalColumns and t.size == 0
    assert [t.columnType[c] for c in h] == [I64, I64, I64, STR, I64]
    assert pattern.entity_tables() == ([], [])


def test_a_relationship_clone_whose_endpoints_are_clones_with_moved_tags(session):
    """(a)-[r]->(b) matched from a graph with tag 0 and cloned ON a second graph that already holds tag 0: the match
    graph's tag moves to 1, so expr_replace_tags runs over r's id, __src and __dst and over both endpoints' ids.  The
    retagged ids are exact, every endpoint names a retagged node, and the ON graph's entities keep theirs."""
    from capsmi.construct import plan_construct
    from capsmi.planner import PGNode, PGRel, PropertyGraph, ScanGraph
    n, m = 120, 400
    rng = np.random.default_rng(27)
    nodes = _nodes(n, ("L", "M"), 10)
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    src[:20] = dst[:20]  # self-loops among them
    rels = [PGRel(5000 + i, nodes[src[i]].id, nodes[dst[i]].id, "T" if i % 3 else "U", {"w": i}) for i in range(m)]
    rows = [{"a": nodes[src[i]], "r": rels[i], "b": nodes[dst[i]]} for i in range(m)]
    other = PropertyGraph([PGNode(10 + i, frozenset({"L"}), {"v": -i}) for i in range(5)],  # ids that collide untagged
                          [PGRel(5000, 10, 11, "T", {"w": -1})])
    spec = {"on": ["other"], "clones": [["a", "a"], ["r", "r"], ["b", "b"]]}
    node_cols = {"a": (["L", "M"], ["v"]), "b": (["L", "M"], ["v"])}
    table, header = _bindings_table(session, rows, node_cols, {"r": ["w"]})
    graph_of = {v: "g" for v in ("a", "r", "b")}
    graph, pattern, strategy = plan_construct(session, table, header, {"a", "b"}, ["r"], graph_of, spec,
                                              {"g": _Tags(), "other": ScanGraph.from_property_graph(session, other)})
    assert strategy == {"other": {0: 0}, "g": {0: 1}} and graph.tags == frozenset({0, 1})
    got_nodes, got_rels = _entities(session, graph)
    ref, ref_strategy, created = cr.construct(rows, {"a": "node", "r": "rel", "b": "node"}, graph_of, spec,
                                              {"g": cr.RefGraph(None), "other": cr.RefGraph(other)})
    assert created is None and ref_strategy == strategy
    _same_graph_up_to_created_ids({"tags": sorted(graph.tags), "nodes": got_nodes, "rels": got_rels},
                                  {"tags": sorted(ref.tags), "nodes": ref.pg.nodes, "rels": ref.pg.rels}, set())
    # and stated outright, without the restatement
    bound = {r.src for r in rels} | {r.dst for r in rels}
    moved = {cr.set_tag(x.id, 1): x for x in nodes if x.id in bound}
    by_id = {x.id: x for x in got_nodes}
    assert len(by_id) == len(got_nodes) == len(moved) + 5
    assert {i for i in by_id if cr.get_tag(i) == 1} == set(moved) and {i for i in by_id if cr.get_tag(i) == 0} == set(range(10, 15))
    assert all(by_id[i].labels == x.labels and by_id[i].props == x.props for i, x in moved.items())
    want = sorted((cr.set_tag(r.id, 1), cr.set_tag(r.src, 1), cr.set_tag(r.dst, 1), r.type, r.props["w"]) for r in rels) + \
        [(5000, 10, 11, "T", -1)]
    assert sorted((r.id, r.src, r.dst, r.type, r.props["w"]) for r in got_rels) == sorted(want)
    assert all(r.src in by_id and r.dst in by_id for r in got_rels)
    t, h = pattern.rel_scan("x", ["U"])  # the pattern graph's own scan, by type
    assert h == ["x", "x.__src", "x.__dst", "x.__type", "x.w"] and t.size == sum(1 for r in rels if r.type == "U")
    assert {cr.get_tag(int(i)) for c in ("x", "x.__src", "x.__dst") for i in _col(t, c)} == {1}


# ---- stored constructed graphs ----------------------------------------------------------------------------
def _rmat_graph(session, scale=8, ef=12):
    from capsmi import graph
    from capsmi.planner import EntityTable, ScanGraph
    rels = graph.rmat_rels(session, scale, 0, ef << scale, (57, 19, 19), 42)
    nodes = graph.rmat_nodes(session, scale, graph.NODES_ALL, 42)
    return ScanGraph(session, [EntityTable("node", frozenset({"Person"}), {}, nodes, id_col="id")],
                     [EntityTable("rel", frozenset({"FRIEND_OF"}), {}, rels, id_col="id", src_col="source", dst_col="target")])


@pytest.mark.parametrize("on_second", [False, True], ids=["tag0", "on_a_second_graph"])
def test_a_stored_constructed_graph_takes_the_fused_routes(session, on_second):
    """MATCH (a)-[r]->(b) CONSTRUCT CLONE a, b CREATE (a)-[:E]->(b) over a few thousand R-MAT relationships, stored with
    to_scan_graph(): the 2-hop count(DISTINCT c) and the Expand projection each take their route once and equal the
    operator-by-operator answer.  ON a second graph the clones carry tag 1."""
    from capsmi.planner import PGNode, Planner, PropertyGraph, ScanGraph, result_rows
    sg = _rmat_graph(session)
    catalog = {"rmat": sg}
    spec = {"clones": [["a", "a"], ["b", "b"]], "creates": [{"rel": "e", "src": "a", "dst": "b", "type": "E"}]}
    if on_second:
        catalog["other"] = ScanGraph.from_property_graph(session, PropertyGraph([PGNode(7, frozenset({"Other"}), {})], []))
        spec["on"] = ["other"]
    p = Planner(sg, catalog)
    g, _ = p.run({"clauses": [{"match": "(a)-[r]->(b)"}, {"construct": spec}], "return": "graph"})
    stored = g.to_scan_graph()
    ids = np.concatenate([_col(e.table, e.id_col) for e in stored.nodes if "Person" in e.labels])
    assert {cr.get_tag(int(i)) for i in ids} == ({1} if on_second else {0})
    (rel,) = stored.rels
    assert rel.labels == frozenset({"E"}) and rel.table.size == 12 << 8
    two_hop = {"clauses": [{"match": "(a:Person)-[:E]->(b:Person)-[:E]->(c:Person)"}],
               "return": {"items": [["n", ["count_distinct", ["id", "c"]]]]}}
    expand = {"clauses": [{"match": "(a:Person)-[r:E]->(b:Person)"}],
              "return": {"items": [["a", ["id", "a"]], ["b", ["id", "b"]]]}}

    def run(q, fused):
        session.set_fused(fused)
        try:
            t, outs = Planner(stored).run(q)
            return result_rows(t, outs, session.dictionary)
        finally:
            session.set_fused(True)

    for q, route in ((two_hop, "two_hop"), (expand, "expand")):
        before = session.route_count(route)
        routed = run(q, True)
        assert session.route_count(route) == before + 1, route
        plain = run(q, False)
        assert session.route_count(route) == before + 1
        key = lambda r: sorted(r.items())  # noqa: E731
        assert sorted(routed, key=key) == sorted(plain, key=key) and routed
