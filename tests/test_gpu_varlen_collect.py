"""Var-length collect(DISTINCT b) on the device (k_reach.hip: the reach lists read off the BFS bit matrix) against the
per-source BFS of varlen_collect_ref.py -- the two direct entry points at the kernels' edges (batch widths, extraction
tiles, slice borders, dense words, hubs, the zero-length path, the list limit), and the planner's plans routed to them
("var_length_distinct")."""
import numpy as np
import pytest

from varlen_collect_ref import reach_lists

pytestmark = pytest.mark.gpu

WORDS = ["auto", "1", "2", "4", "8"]
LDS_WORDS = 16384  # k_reach.hip kLdsWords: a target slice is LDS_WORDS / W ids at W words per node
LIST_TILE = 256    # k_reach.hip kListTile: a wave of the extraction owns LIST_TILE consecutive nodes (of one source word)


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src))), ColumnData("source", I64, src),
                          ColumnData("target", I64, dst)])


def _bitmaps(session, n, a_mask, b_mask, lo=0):
    from capsmi import ColumnData, I64, graph
    a_nodes = session.table([ColumnData("id", I64, np.nonzero(a_mask)[0].astype(np.int64) + lo)])
    b_nodes = session.table([ColumnData("id", I64, np.nonzero(b_mask)[0].astype(np.int64) + lo)])
    return (graph.NodeBitmap(session, lo, lo + n).add_scan(a_nodes), graph.NodeBitmap(session, lo, lo + n).add_scan(b_nodes))


def _check(session, n, src, dst, a_mask, b_mask, lower, upper, lo=0, rels=None, expect=None):
    """Both entry points against reach_lists (src / dst absolute ids, masks over the window [lo, lo + n)), each run
    twice: the row set and every list exactly equal, the two runs' exported arrays identical, lists strictly
    ascending, count == len(list).  `expect`: the reference's (lists, union), when the caller has it already."""
    from capsmi import graph
    a_mask, b_mask = np.asarray(a_mask, bool), np.asarray(b_mask, bool)
    rels = rels or [_table(session, src, dst)]
    a_ok, b_ok = _bitmaps(session, n, a_mask, b_mask, lo)
    lists, union = expect if expect is not None else reach_lists(n, src - lo, dst - lo, a_mask, b_mask, lower, upper)
    runs = []
    for _ in range(2):
        out = graph.var_length_collect_distinct(session, rels, a_ok, b_ok, lower, upper, "a", "ds", "cnt")
        ids = out.column("a").values
        ds = out.column("ds")
        cnt = out.column("cnt").values
        assert ds.valid is None or ds.valid.all()
        assert out.size == len(ids) == len(set(ids.tolist()))
        assert sorted(ids.tolist()) == sorted(a + lo for a in lists), (lower, upper)
        for a, d, c in zip(ids.tolist(), ds.values, cnt.tolist()):
            assert d.dtype == np.int64 and np.array_equal(d, lists[a - lo] + lo), (a, lower, upper)
            assert (np.diff(d) > 0).all() and c == len(d) > 0
        flat = np.concatenate(list(ds.values)) if out.size else np.zeros(0, np.int64)
        whole = graph.var_length_reach_list(session, rels, a_ok, b_ok, lower, upper)
        assert whole.dtype == np.int64 and np.array_equal(whole, union + lo), (lower, upper)
        runs.append((ids, cnt, flat, whole))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    return lists, union


def _subset(all_lists, a_mask, n):
    """The reference of a source subset from the lists of every source (D(a) does not depend on a_mask)."""
    lists = {a: v for a, v in all_lists.items() if a_mask[a]}
    union = np.zeros(n, bool)
    for v in lists.values():
        union[v] = True
    return lists, np.nonzero(union)[0].astype(np.int64)


RANGES = [(1, 1), (1, 3), (0, 3), (1, 6), (0, 10)]


@pytest.mark.parametrize("seed", range(5))
def test_random_multigraphs(session, seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(5, 300))
    m = int(rng.integers(0, 3000))
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 5] = dst[: m // 5]  # self-loops
    a_mask = rng.random(n) < 0.7
    b_mask = rng.random(n) < 0.6
    for lower, upper in RANGES:
        _check(session, n, src, dst, a_mask, b_mask, lower, upper)


_BATCH = {}


def _batch_graph():
    """One graph and the lists of all its nodes for the batch-edge cases, computed once."""
    if not _BATCH:
        rng = np.random.default_rng(17)
        n, m = 1500, 6000
        src = rng.integers(0, n, m).astype(np.int64)
        dst = rng.integers(0, n, m).astype(np.int64)
        b_mask = rng.random(n) < 0.6
        ones = np.ones(n, bool)
        _BATCH.update(n=n, src=src, dst=dst, b_mask=b_mask,
                      ref={(1, 3): reach_lists(n, src, dst, ones, b_mask, 1, 3)[0],
                           (0, 2): reach_lists(n, src, dst, ones, b_mask, 0, 2)[0]})
    return _BATCH


@pytest.mark.parametrize("words,flat", [(w, "sliced") for w in WORDS] + [("2", "flat")])
def test_batch_edges(session, knobs, words, flat):
    """|a_ok| around the batch width 64 W: no source, one, a word's edges, a batch's edges, two batches and a bit (a
    last batch narrower than W) -- scattered ids.  Once through the flat level pass."""
    knobs(session, CAPSMI_REACH_WORDS=words, CAPSMI_REACH=flat)
    g = _batch_graph()
    n = g["n"]
    rng = np.random.default_rng(18)
    W = 8 if words == "auto" else int(words)
    for k in sorted({0, 1, 63, 64, 65, 64 * W, 64 * W + 1, 128 * W + 3}):
        a_mask = np.zeros(n, bool)
        a_mask[rng.permutation(n)[:k]] = True
        for lower, upper in [(1, 3), (0, 2)]:
            lists, union = _check(session, n, g["src"], g["dst"], a_mask, g["b_mask"], lower, upper,
                                  expect=_subset(g["ref"][(lower, upper)], a_mask, n))
            if k == 0:
                assert not lists and len(union) == 0


@pytest.mark.parametrize("n", [LIST_TILE - 1, LIST_TILE, LIST_TILE + 1, 2 * LIST_TILE + 5, 3 * LIST_TILE + 37])
def test_tile_edges(session, knobs, n):
    """Domains around the extraction tile: one id short of a tile, a tile, one more, two and five, and a size that is
    no multiple of 64; a window starting at 1000, sources and targets among the top three ids, more than one batch."""
    knobs(session, CAPSMI_REACH_WORDS="1")
    lo = 1000
    rng = np.random.default_rng(n)
    m = 5 * n
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    top = np.array([n - 1, n - 2, n - 3])
    src[:40] = rng.choice(top, 40)
    dst[40:80] = rng.choice(top, 40)
    src[80:90], dst[80:90] = top[rng.integers(0, 3, 10)], top[rng.integers(0, 3, 10)]
    a_mask = np.zeros(n, bool)
    a_mask[rng.permutation(n - 3)[:64 + 9]] = True  # two batches at one word
    a_mask[top] = True
    b_mask = rng.random(n) < 0.5
    b_mask[top[:2]] = True
    for lower, upper in [(1, 2), (0, 3)]:
        _check(session, n, src + lo, dst + lo, a_mask, b_mask, lower, upper, lo=lo)


@pytest.mark.parametrize("words,slices", [("2", 1), ("8", 3)])
@pytest.mark.parametrize("extra", [0, 5])
def test_slice_edges(session, knobs, words, slices, extra):
    """Domains of whole target slices and five ids more: sources and targets in the top three ids."""
    knobs(session, CAPSMI_REACH_WORDS=words)
    w = int(words)
    n = slices * (LDS_WORDS // w) + extra
    lo = 1000
    rng = np.random.default_rng(n)
    m = 4000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    top = np.array([n - 1, n - 2, n - 3])
    src[:60] = rng.choice(top, 60)
    dst[60:120] = rng.choice(top, 60)
    src[120:130], dst[120:130] = top[rng.integers(0, 3, 10)], top[rng.integers(0, 3, 10)]
    a_mask = np.zeros(n, bool)
    a_mask[rng.permutation(n - 3)[: 64 * w + 7]] = True  # more than one batch, and at least w words wide
    a_mask[top] = True
    b_mask = rng.random(n) < 0.5
    b_mask[top[:2]] = True
    for lower, upper in [(1, 3), (0, 4)]:
        _check(session, n, src + lo, dst + lo, a_mask, b_mask, lower, upper, lo=lo)


def test_dense_words(session):
    """The complete directed graph on 130 nodes with loops: every bit of every word is set, so every ballot path of a
    word runs, and every list is all 130 ids."""
    n = 130
    src, dst = [x.ravel().astype(np.int64) for x in np.meshgrid(np.arange(n), np.arange(n))]
    ones = np.ones(n, bool)
    lists, union = _check(session, n, src, dst, ones, ones, 1, 2)
    assert len(lists) == n and all(v.tolist() == list(range(n)) for v in lists.values()) and len(union) == n


@pytest.mark.parametrize("reverse", [False, True])
def test_hub(session, reverse):
    """A star with 10 000 leaves: the centre's one list of 10 000 elements, and the reversed star's 10 000 lists of
    one element."""
    k = 10_000
    leaves = np.arange(1, k + 1, dtype=np.int64)
    centre = np.zeros(k, dtype=np.int64)
    src, dst = (leaves, centre) if reverse else (centre, leaves)
    ones = np.ones(k + 1, bool)
    lists, _ = _check(session, k + 1, src, dst, ones, ones, 1, 3)
    if reverse:
        assert len(lists) == k and all(v.tolist() == [0] for v in lists.values())
    else:
        assert list(lists) == [0] and lists[0].tolist() == leaves.tolist()


def test_multi_edges_give_one_element(session):
    k = 9000
    src, dst = np.full(k, 3, dtype=np.int64), np.full(k, 5, dtype=np.int64)
    ones = np.ones(8, bool)
    lists, union = _check(session, 8, src, dst, ones, ones, 1, 4)
    assert {a: v.tolist() for a, v in lists.items()} == {3: [5]} and union.tolist() == [5]


def test_zero_length_path_appears_once_in_place(session):
    """The 2-cycle plus a self-loop: with lower = 0 source 1 holds itself once, between 0 and nothing, whether b_ok(1)
    holds (the cycle returns to it as well) or not (only the zero-length path gives it)."""
    src, dst = np.array([0, 1, 2], dtype=np.int64), np.array([1, 0, 2], dtype=np.int64)
    for b1 in (True, False):
        b_mask = np.array([True, b1, True])
        a_mask = np.array([False, True, False])
        lists, union = _check(session, 3, src, dst, a_mask, b_mask, 0, 2)
        assert {a: v.tolist() for a, v in lists.items()} == {1: [0, 1]} and union.tolist() == [0, 1]
    for b0 in (True, False):
        b_mask = np.array([b0, True, True])
        a_mask = np.array([True, False, False])
        lists, _ = _check(session, 3, src, dst, a_mask, b_mask, 0, 2)
        assert {a: v.tolist() for a, v in lists.items()} == {0: [0, 1]}


def test_empty_b_ok(session):
    import ctypes
    from capsmi import _lib, graph
    from capsmi.table import GpuTable
    rng = np.random.default_rng(4)
    n, m = 200, 900
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    a_mask = rng.random(n) < 0.5
    none = np.zeros(n, bool)
    lists, union = _check(session, n, src, dst, a_mask, none, 1, 3)
    assert not lists and len(union) == 0
    a_ok, b_ok = _bitmaps(session, n, a_mask, none)
    rels = [_table(session, src, dst)]
    assert graph.var_length_collect_distinct(session, rels, a_ok, b_ok, 1, 3).size == 0
    out = ctypes.c_void_p()  # the global form is one row holding the empty list
    _lib.call("capsmi_var_length_reach_list", session.handle, 1, graph._handles(rels), b"source", b"target", a_ok.handle,
              b_ok.handle, 1, 3, b"ds", ctypes.byref(out))
    one = GpuTable(session, out)
    assert one.size == 1 and len(one.column("ds").values[0]) == 0
    lists, union = _check(session, n, src, dst, a_mask, none, 0, 3)
    assert {a: v.tolist() for a, v in lists.items()} == {int(a): [int(a)] for a in np.nonzero(a_mask)[0]}
    assert union.tolist() == np.nonzero(a_mask)[0].tolist()


@pytest.mark.parametrize("upper", [40, 10 ** 6])
def test_chain_levels(session, upper):
    """0 -> 1 -> ... -> 40: the list of source 0 is 1..40; the early exit ends a huge upper."""
    src, dst = np.arange(40, dtype=np.int64), np.arange(1, 41, dtype=np.int64)
    ones = np.ones(41, bool)
    lists, union = _check(session, 41, src, dst, ones, ones, 1, upper)
    assert lists[0].tolist() == list(range(1, 41)) and 40 not in lists and union.tolist() == list(range(1, 41))


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
    _check(session, n, src, dst, a_mask, b_mask, 1, 3, lo=lo, rels=[t1, t2], expect=one)
    inside = (src >= lo) & (src < lo + n) & (dst >= lo) & (dst < lo + n)
    _check(session, n, src[inside], dst[inside], a_mask, b_mask, 1, 3, lo=lo, expect=one)


def test_without_count_and_explode(session):
    """count_name = None leaves the count column out; explode of the list column gives exactly the reference's (a, b)
    pairs."""
    from capsmi import graph
    rng = np.random.default_rng(21)
    n, m = 300, 1200
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    a_mask, b_mask = rng.random(n) < 0.7, rng.random(n) < 0.6
    a_ok, b_ok = _bitmaps(session, n, a_mask, b_mask)
    lists, _ = reach_lists(n, src, dst, a_mask, b_mask, 0, 3)
    out = graph.var_length_collect_distinct(session, [_table(session, src, dst)], a_ok, b_ok, 0, 3, "a", "ds")
    assert list(out.physicalColumns) == ["a", "ds"]
    pairs = out.explode("ds", "b")
    got = sorted(zip(pairs.column("a").values.tolist(), pairs.column("b").values.tolist()))
    assert got == sorted((a, int(b)) for a, v in lists.items() for b in v)


def test_refusals(session, knobs):
    from capsmi import _lib, graph
    src, dst = np.array([0, 1], dtype=np.int64), np.array([1, 2], dtype=np.int64)
    rels = [_table(session, src, dst)]
    ones = np.ones(3, bool)
    a_ok, b_ok = _bitmaps(session, 3, ones, ones)
    for fn in (lambda lo, hi: graph.var_length_collect_distinct(session, rels, a_ok, b_ok, lo, hi),
               lambda lo, hi: graph.var_length_reach_list(session, rels, a_ok, b_ok, lo, hi)):
        with pytest.raises(_lib.NotImplementedException, match="join plan"):
            fn(2, 3)
        with pytest.raises(_lib.IllegalArgumentException):
            fn(0, 0)
        with pytest.raises(_lib.IllegalArgumentException):
            fn(1, 0)
    other, _ = _bitmaps(session, 4, np.ones(4, bool), np.ones(4, bool))
    with pytest.raises(_lib.CapsmiError) as mine:
        graph.var_length_collect_distinct(session, rels, a_ok, other, 1, 2)
    with pytest.raises(_lib.CapsmiError) as theirs:
        graph.var_length_count(session, rels, a_ok, other, 1, 2)
    assert type(mine.value) is type(theirs.value)


def test_list_limit(session, knobs):
    """Over CAPSMI_REACH_LIST_LIMIT the query is refused with the limit in the message; back at auto the same session
    answers."""
    from capsmi import _lib, graph
    rng = np.random.default_rng(33)
    n, m = 400, 3000
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    ones = np.ones(n, bool)
    rels = [_table(session, src, dst)]
    a_ok, b_ok = _bitmaps(session, n, ones, ones)
    lists, union = reach_lists(n, src, dst, ones, ones, 1, 3)
    assert sum(len(v) for v in lists.values()) > 100 and len(union) > 100
    knobs(session, CAPSMI_REACH_LIST_LIMIT="100", CAPSMI_REACH_WORDS="1")  # several batches: the first one crosses it
    with pytest.raises(_lib.UnsupportedOperationException, match="CAPSMI_REACH_LIST_LIMIT = 100"):
        graph.var_length_collect_distinct(session, rels, a_ok, b_ok, 1, 3)
    with pytest.raises(_lib.UnsupportedOperationException, match="CAPSMI_REACH_LIST_LIMIT = 100"):
        graph.var_length_reach_list(session, rels, a_ok, b_ok, 1, 3)
    session.set_config("CAPSMI_REACH_LIST_LIMIT", None)
    _check(session, n, src, dst, ones, ones, 1, 3, rels=rels, expect=(lists, union))


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


COLLECT = ["ds", ["collect_distinct", ["id", "b"]]]
COUNT = ["n", ["count_distinct", ["id", "b"]]]


def _query(lo, hi, items, label="Person", rtype="KNOWS", where=None):
    clause = {"match": f"(a:{label})-[:{rtype}*{lo}..{hi}]->(b:{label})"}
    if where is not None:
        clause["where"] = where
    return {"clauses": [clause], "return": {"items": items}}


def _norm(rows):
    """Rows in a comparable form: sorted by a (if there), lists as plain int lists."""
    out = [{k: ([int(x) for x in v] if k == "ds" else v) for k, v in r.items()} for r in rows]
    return sorted(out, key=lambda r: r.get("a", 0))


def _want(lists, union, grouped, with_list=True, with_count=False, ids=None):
    def ident(i):
        return int(i if ids is None else ids[i])
    rows = []
    for a, v in (sorted(lists.items()) if grouped else [(None, union)]):
        row = {"a": ident(a)} if grouped else {}
        if with_list:
            row["ds"] = [ident(x) for x in v]
        if with_count:
            row["n"] = len(v)
        rows.append(row)
    return sorted(rows, key=lambda r: r.get("a", 0))


def _routed_forms(session, sg, lo, hi, lists, union, where=None):
    """Grouped and alone, collect alone and with count (either order): each routed, each equal to the reference."""
    for grouped in (True, False):
        key = [["a", ["id", "a"]]] if grouped else []
        for items, wc in ((key + [COLLECT], False), (key + [COUNT, COLLECT], True), (key + [COLLECT, COUNT], True)):
            q = _query(lo, hi, items, where=where)
            got = _routed(session, "var_length_distinct", lambda: _run(session, sg, q))
            assert _norm(got) == _want(lists, union, grouped, with_count=wc), (lo, hi, grouped, wc)


@pytest.mark.parametrize("lo,hi", [(1, 3), (0, 3), (1, 6)])
def test_routed(session, lo, hi):
    """R-MAT scale 8, edge factor 32.  For (1, 3) and (0, 3) the same queries run operator by operator as well
    (set_fused(False)) at the same scale 8 and equal the routed rows."""
    from oracle import cpu
    scale = 8
    sg = _graph(session, scale)
    src, dst = cpu.rmat_edges(scale, 0, 32 << scale, (45, 15, 15), 42)
    ones = np.ones(1 << scale, bool)
    lists, union = reach_lists(1 << scale, src, dst, ones, ones, lo, hi)
    _routed_forms(session, sg, lo, hi, lists, union)
    if (lo, hi) in ((1, 3), (0, 3)):  # the reference's plan restated
        key = [["a", ["id", "a"]]]
        for items, grouped, wc in ((key + [COLLECT], True, False), ([COLLECT], False, False),
                                   (key + [COUNT, COLLECT], True, True)):
            q = _query(lo, hi, items)
            plain = _run(session, sg, q, fused=False)
            assert _norm(plain) == _norm(_run(session, sg, q))
            assert _norm(plain) == _want(lists, union, grouped, with_count=wc)


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
        lists, union = reach_lists(n, src, dst, a_mask, b_mask, lo, hi)
        _routed_forms(session, sg, lo, hi, lists, union, where=where)
    # lower = 0 with a predicate on a alone (one on b would also filter the zero-length path's copy of a, which is
    # not the route's rule: such a plan is not routed, for the count either)
    lists, union = reach_lists(n, src, dst, a_mask, pm, 0, 3)
    _routed_forms(session, sg, 0, 3, lists, union, where=where[1])


def test_sparse_ids_equal_the_reference(session):
    """Ids near 2^40, compacted.  The dense ids of a compacted graph are not monotonic in the original ids, so the
    route declines collect there and the operator path answers: the lists are in original ids, ascending.  The count
    alone stays routed."""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    rng = np.random.default_rng(5)
    ids = np.unique(rng.integers(1 << 40, (1 << 40) + (1 << 45), 300))
    n, m = len(ids), 900
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
    lists, union = reach_lists(n, s_i, d_i, ones, ones, 1, 3)
    key = [["a", ["id", "a"]]]
    got = _run(session, sg, _query(1, 3, key + [COLLECT, COUNT], label="N", rtype="R"))
    assert _norm(got) == _want(lists, union, True, with_count=True, ids=ids)
    got = _run(session, sg, _query(1, 3, [COLLECT], label="N", rtype="R"))
    assert _norm(got) == _want(lists, union, False, ids=ids)
    _routed(session, "var_length_distinct", lambda: _run(session, sg, _query(1, 3, key + [COUNT], label="N", rtype="R")))
