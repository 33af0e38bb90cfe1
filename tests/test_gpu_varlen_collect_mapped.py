"""Var-length collect(DISTINCT b) over remapped ids on the device (k_reach.hip "Remapped ids": the hit matrix gathered
in the order of the original ids, so the lists come out sorted without a sort of their elements) against
varlen_collect_mapped_ref.mapped_lists -- the two mapped entry points at the walk's edges (permutations of orig, 64-lane
steps, tiles, batches, widths, the zero-length path, hubs, dense words, the global form's bitmap permutation), and the
planner's plans on compacted graphs, which the route ("var_length_distinct") now takes."""
import ctypes

import numpy as np
import pytest

from varlen_collect_mapped_ref import id_sets, mapped_lists

pytestmark = pytest.mark.gpu

IDS = id_sets()
LIST_TILE = 256  # k_reach.hip kListTile


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src))), ColumnData("source", I64, src),
                          ColumnData("target", I64, dst)])


def _bitmaps(session, n, a_mask, b_mask, lo=0):
    from capsmi import ColumnData, I64, graph
    a_nodes = session.table([ColumnData("id", I64, np.nonzero(a_mask)[0].astype(np.int64) + lo)])
    b_nodes = session.table([ColumnData("id", I64, np.nonzero(b_mask)[0].astype(np.int64) + lo)])
    return (graph.NodeBitmap(session, lo, lo + n).add_scan(a_nodes), graph.NodeBitmap(session, lo, lo + n).add_scan(b_nodes))


def _export(out):
    ids = out.column("a").values
    ds = out.column("ds")
    cnt = out.column("cnt").values
    assert ds.valid is None or ds.valid.all()
    flat = np.concatenate(list(ds.values)) if out.size else np.zeros(0, np.int64)
    return ids, ds.values, cnt, flat


def _check(session, n, src, dst, a_mask, b_mask, lower, upper, ids, lo=0):
    """Both mapped entry points against mapped_lists (src / dst dense ids relative to the window, which starts at
    `lo`), each run twice: the row set, every list exactly and in order, count == len(list), the global list; the two
    runs' exported arrays identical."""
    from capsmi import graph
    a_mask, b_mask = np.asarray(a_mask, bool), np.asarray(b_mask, bool)
    rels = [_table(session, src + lo, dst + lo)]
    a_ok, b_ok = _bitmaps(session, n, a_mask, b_mask, lo)
    lists, union = mapped_lists(n, src, dst, a_mask, b_mask, lower, upper, ids)
    runs = []
    for _ in range(2):
        out = graph.var_length_collect_distinct(session, rels, a_ok, b_ok, lower, upper, "a", "ds", "cnt", orig=ids)
        got_ids, ds, cnt, flat = _export(out)
        assert out.size == len(got_ids) == len(set(got_ids.tolist()))
        assert sorted(got_ids.tolist()) == sorted(lists), (lower, upper)
        for a, d, c in zip(got_ids.tolist(), ds, cnt.tolist()):
            assert d.dtype == np.int64 and d.tolist() == lists[a], (a, lower, upper)
            assert c == len(d) > 0
        whole = graph.var_length_reach_list(session, rels, a_ok, b_ok, lower, upper, orig=ids)
        assert whole.dtype == np.int64 and whole.tolist() == union, (lower, upper)
        runs.append((got_ids, cnt, flat, whole))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    return lists, union


def _random_graph(rng, n, m):
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 5] = dst[: m // 5]  # self-loops
    return src, dst


# ---- the direct entry points ----------------------------------------------------------------------------
@pytest.mark.parametrize("perm", list(IDS))
def test_permutations(session, perm):
    rng = np.random.default_rng(41)
    n, m = 300, 1500
    src, dst = _random_graph(rng, n, m)
    a_mask, b_mask = rng.random(n) < 0.7, rng.random(n) < 0.6
    ids = IDS[perm](rng, n)
    for lower, upper in [(1, 3), (0, 3), (1, 6)]:
        _check(session, n, src, dst, a_mask, b_mask, lower, upper, ids)


def test_identity_is_byte_identical_to_the_unmapped_entry(session):
    """orig[d] = lo + d on a window that starts at 1000: ids, counts, list values and the global list, byte for byte."""
    from capsmi import graph
    rng = np.random.default_rng(42)
    n, m, lo = 700, 3000, 1000
    src, dst = _random_graph(rng, n, m)
    a_mask, b_mask = rng.random(n) < 0.8, rng.random(n) < 0.6  # more than one batch at eight words
    rels = [_table(session, src + lo, dst + lo)]
    a_ok, b_ok = _bitmaps(session, n, a_mask, b_mask, lo)
    ids = lo + np.arange(n, dtype=np.int64)
    for lower, upper in [(1, 3), (0, 2)]:
        plain = _export(graph.var_length_collect_distinct(session, rels, a_ok, b_ok, lower, upper, "a", "ds", "cnt"))
        mapped = _export(graph.var_length_collect_distinct(session, rels, a_ok, b_ok, lower, upper, "a", "ds", "cnt",
                                                           orig=ids))
        for x, y in zip((plain[0], plain[2], plain[3]), (mapped[0], mapped[2], mapped[3])):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        assert len(plain[3]) > n
        whole = graph.var_length_reach_list(session, rels, a_ok, b_ok, lower, upper)
        assert whole.tobytes() == graph.var_length_reach_list(session, rels, a_ok, b_ok, lower, upper, orig=ids).tobytes()


@pytest.mark.parametrize("n", [1, 63, 64, 65, LIST_TILE - 1, LIST_TILE, LIST_TILE + 1, 300, 3 * LIST_TILE + 37])
def test_domain_sizes(session, n):
    """The 64-lane steps and the 256-node tile of the walk, the 64-position words of the global permutation: sources and
    targets among the top ids and the top ranks, a random and a signed permutation."""
    rng = np.random.default_rng(1000 + n)
    m = 5 * n
    src, dst = _random_graph(rng, n, m)
    top = np.arange(max(n - 3, 0), n)
    src[:8] = rng.choice(top, len(src[:8]))
    dst[8:16] = rng.choice(top, len(dst[8:16]))
    for perm in ("random", "signed"):
        ids = IDS[perm](rng, n)
        a_mask, b_mask = rng.random(n) < 0.7, rng.random(n) < 0.6
        by_rank = np.argsort(ids)
        a_mask[by_rank[-1]] = b_mask[by_rank[-1]] = b_mask[by_rank[0]] = True  # the first and the last position
        a_mask[top] = True
        for lower, upper in [(1, 2), (0, 3)]:
            _check(session, n, src, dst, a_mask, b_mask, lower, upper, ids)


def test_65_sources(session):
    rng = np.random.default_rng(43)
    n, m = 400, 1600
    src, dst = _random_graph(rng, n, m)
    a_mask = np.zeros(n, bool)
    a_mask[rng.permutation(n)[:65]] = True  # two words
    ids = IDS["random"](rng, n)
    for lower, upper in [(1, 3), (0, 2)]:
        _check(session, n, src, dst, a_mask, rng.random(n) < 0.6, lower, upper, ids)


def test_two_batches_at_eight_words(session):
    """513 sources over 600 ids: a full batch and a batch of one source; every list belongs to its source."""
    rng = np.random.default_rng(44)
    n, m = 600, 2400
    src, dst = _random_graph(rng, n, m)
    a_mask = np.zeros(n, bool)
    a_mask[rng.permutation(n)[:513]] = True
    ids = IDS["signed"](rng, n)
    for lower, upper in [(1, 3), (0, 2)]:
        lists, _ = _check(session, n, src, dst, a_mask, rng.random(n) < 0.6, lower, upper, ids)
        assert len(lists) > 64 * 8 - 200


@pytest.mark.parametrize("words", ["1", "2", "4", "8"])
def test_forced_widths(session, knobs, words):
    """Each width W through CAPSMI_REACH_WORDS: 64 W + 1 and 128 W + 3 sources (a join of two and of three batches, the
    last narrower than W)."""
    knobs(session, CAPSMI_REACH_WORDS=words)
    w = int(words)
    rng = np.random.default_rng(45 + w)
    n, m = 128 * w + 90, 4 * (128 * w + 90)
    src, dst = _random_graph(rng, n, m)
    ids = IDS["random"](rng, n)
    b_mask = rng.random(n) < 0.6
    for k in (64 * w + 1, 128 * w + 3):
        a_mask = np.zeros(n, bool)
        a_mask[rng.permutation(n)[:k]] = True
        for lower, upper in [(1, 3), (0, 2)]:
            _check(session, n, src, dst, a_mask, b_mask, lower, upper, ids)


def test_zero_length_path(session):
    """lower = 0: sources outside b_ok hold themselves, once; the 2-cycle returns to its source, which appears once; a
    source that reaches nothing holds itself alone; its place in the list is its original id's."""
    ids = np.array([50, -7, 1 << 40, 3, -(1 << 41), 12], dtype=np.int64)
    src, dst = np.array([0, 1, 2, 2], dtype=np.int64), np.array([1, 0, 2, 3], dtype=np.int64)
    a_mask = np.array([True, True, True, False, True, True])
    for b_mask in (np.ones(6, bool), np.array([False, False, False, True, False, True]),
                   np.array([False, True, True, True, True, False])):
        lists, union = _check(session, 6, src, dst, a_mask, b_mask, 0, 2, ids)
        assert sorted(lists) == sorted(ids[a_mask].tolist())
        assert lists[int(ids[4])] == [int(ids[4])] and lists[12] == [12]  # reach nothing
        assert lists[50].count(50) == 1 and lists[-7].count(-7) == 1      # the cycle 0 -> 1 -> 0
        assert (1 << 40) in lists[1 << 40] and lists[1 << 40] == sorted(lists[1 << 40])
    rng = np.random.default_rng(46)
    n = 330
    src, dst = _random_graph(rng, n, 900)
    a_mask = rng.random(n) < 0.7
    b_mask = rng.random(n) < 0.5
    b_mask[np.nonzero(a_mask)[0][::2]] = False  # b_ok(a) false for half the sources
    _check(session, n, src, dst, a_mask, b_mask, 0, 3, IDS["signed"](rng, n))


@pytest.mark.parametrize("reverse", [False, True])
def test_hub(session, reverse):
    """A star with 3000 leaves under a random permutation: the centre's list is every leaf in sorted original order; the
    reversed star gives 3000 lists of one element."""
    k = 3000
    rng = np.random.default_rng(47)
    leaves = np.arange(1, k + 1, dtype=np.int64)
    centre = np.zeros(k, dtype=np.int64)
    src, dst = (leaves, centre) if reverse else (centre, leaves)
    ones = np.ones(k + 1, bool)
    ids = IDS["signed"](rng, k + 1)
    lists, _ = _check(session, k + 1, src, dst, ones, ones, 1, 3, ids)
    if reverse:
        assert len(lists) == k and all(v == [int(ids[0])] for v in lists.values())
    else:
        assert list(lists) == [int(ids[0])] and lists[int(ids[0])] == np.sort(ids[1:]).tolist()


def test_hub_holds_every_id(session):
    """A hub with a loop: its list is every id of the domain."""
    n = 1000
    rng = np.random.default_rng(48)
    src, dst = np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    ids = IDS["random"](rng, n) * 3 - 1500
    a_mask = np.zeros(n, bool)
    a_mask[0] = True
    lists, union = _check(session, n, src, dst, a_mask, np.ones(n, bool), 1, 1, ids)
    assert lists == {int(ids[0]): np.sort(ids).tolist()} and union == np.sort(ids).tolist()


def test_dense_words(session):
    """The complete directed graph on 130 nodes with loops: every bit of every word is set, every ballot path runs, and
    every list is all ids in sorted original order."""
    n = 130
    rng = np.random.default_rng(49)
    src, dst = [x.ravel().astype(np.int64) for x in np.meshgrid(np.arange(n), np.arange(n))]
    ones = np.ones(n, bool)
    ids = IDS["signed"](rng, n)
    lists, union = _check(session, n, src, dst, ones, ones, 1, 2, ids)
    want = np.sort(ids).tolist()
    assert len(lists) == n and all(v == want for v in lists.values()) and union == want


@pytest.mark.parametrize("perm", list(IDS))
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_global_form(session, perm, n):
    from capsmi import graph
    rng = np.random.default_rng(50 + n)
    src, dst = _random_graph(rng, n, 3 * n)
    a_mask, b_mask = rng.random(n) < 0.5, rng.random(n) < 0.7
    a_mask[0] = True
    ids = IDS[perm](rng, n)
    rels = [_table(session, src, dst)]
    a_ok, b_ok = _bitmaps(session, n, a_mask, b_mask)
    for lower, upper in [(1, 1), (1, 4), (0, 2)]:
        _, union = mapped_lists(n, src, dst, a_mask, b_mask, lower, upper, ids)
        one = graph.var_length_reach_list(session, rels, a_ok, b_ok, lower, upper, orig=ids)
        two = graph.var_length_reach_list(session, rels, a_ok, b_ok, lower, upper, orig=ids)
        assert one.tolist() == union and one.tobytes() == two.tobytes(), (lower, upper)


def test_nothing_reached(session):
    """Empty b_ok: no grouped row, and the global form is one row holding the empty list."""
    from capsmi import _lib, graph
    from capsmi.table import GpuTable
    rng = np.random.default_rng(51)
    n = 200
    src, dst = _random_graph(rng, n, 900)
    a_mask, none = rng.random(n) < 0.5, np.zeros(n, bool)
    ids = IDS["signed"](rng, n)
    lists, union = _check(session, n, src, dst, a_mask, none, 1, 3, ids)
    assert not lists and not union
    a_ok, b_ok = _bitmaps(session, n, a_mask, none)
    rels = [_table(session, src, dst)]
    holder, ptr, length = graph._orig_device(session, a_ok, ids)
    out = ctypes.c_void_p()
    _lib.call("capsmi_var_length_reach_list_mapped", session.handle, 1, graph._handles(rels), b"source", b"target",
              a_ok.handle, b_ok.handle, 1, 3, ptr, length, b"ds", ctypes.byref(out))
    one = GpuTable(session, out)
    assert one.size == 1 and len(one.column("ds").values[0]) == 0


def test_list_limit(session, knobs):
    from capsmi import _lib, graph
    rng = np.random.default_rng(52)
    n, m = 400, 3000
    src, dst = _random_graph(rng, n, m)
    ones = np.ones(n, bool)
    ids = IDS["random"](rng, n)
    rels = [_table(session, src, dst)]
    a_ok, b_ok = _bitmaps(session, n, ones, ones)
    knobs(session, CAPSMI_REACH_LIST_LIMIT="100", CAPSMI_REACH_WORDS="1")
    with pytest.raises(_lib.UnsupportedOperationException, match="CAPSMI_REACH_LIST_LIMIT = 100"):
        graph.var_length_collect_distinct(session, rels, a_ok, b_ok, 1, 3, orig=ids)
    with pytest.raises(_lib.UnsupportedOperationException, match="CAPSMI_REACH_LIST_LIMIT = 100"):
        graph.var_length_reach_list(session, rels, a_ok, b_ok, 1, 3, orig=ids)
    session.set_config("CAPSMI_REACH_LIST_LIMIT", None)
    _check(session, n, src, dst, ones, ones, 1, 3, ids)


def test_refusals(session):
    from capsmi import _lib, graph
    src, dst = np.array([0, 1], dtype=np.int64), np.array([1, 2], dtype=np.int64)
    rels = [_table(session, src, dst)]
    ones = np.ones(3, bool)
    a_ok, b_ok = _bitmaps(session, 3, ones, ones)
    good = np.array([9, -4, 5], dtype=np.int64)
    for fn in (lambda lo, hi, o: graph.var_length_collect_distinct(session, rels, a_ok, b_ok, lo, hi, orig=o),
               lambda lo, hi, o: graph.var_length_reach_list(session, rels, a_ok, b_ok, lo, hi, orig=o)):
        with pytest.raises(_lib.NotImplementedException, match="join plan"):
            fn(2, 3, good)
        with pytest.raises(_lib.IllegalArgumentException):
            fn(0, 0, good)
        with pytest.raises(_lib.IllegalArgumentException, match="one original id per id"):
            fn(1, 2, good[:2])
        with pytest.raises(_lib.IllegalArgumentException, match="one original id per id"):
            fn(1, 2, np.arange(4, dtype=np.int64))
        with pytest.raises(_lib.IllegalArgumentException, match="twice"):
            fn(1, 2, np.array([9, -4, 9], dtype=np.int64))
    # the session answers afterwards
    assert graph.var_length_reach_list(session, rels, a_ok, b_ok, 1, 2, orig=good).tolist() == [-4, 5]


# ---- routed through the planner -------------------------------------------------------------------------
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
KEY = [["a", ["id", "a"]]]


def _query(lo, hi, items, label="N", rtype="R"):
    return {"clauses": [{"match": f"(a:{label})-[:{rtype}*{lo}..{hi}]->(b:{label})"}], "return": {"items": items}}


def _norm(rows):
    out = [{k: ([int(x) for x in v] if k == "ds" else v) for k, v in r.items()} for r in rows]
    return sorted(out, key=lambda r: r.get("a", 0))


def _want(lists, union, grouped, with_count=False):
    rows = []
    for a, v in (sorted(lists.items()) if grouped else [(None, union)]):
        row = {"a": a} if grouped else {}
        row["ds"] = list(v)
        if with_count:
            row["n"] = len(v)
        rows.append(row)
    return rows


def _scan_graph(session, ids, s_i, d_i, label="N", rtype="R"):
    """Node ids `ids` (row d holds ids[d]) and relationships ids[s_i] -> ids[d_i] as entity tables, compacted."""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    m = len(s_i)
    nodes = session.table([ColumnData("id", I64, ids)]).as_node_table("id")
    rels = session.table([ColumnData("id", I64, np.arange(m, dtype=np.int64) * 3 + (1 << 50)),
                          ColumnData("source", I64, ids[s_i]), ColumnData("target", I64, ids[d_i])]).as_rel_table(
        "id", "source", "target")
    assert session.compact_if_sparse([nodes], [rels])
    return ScanGraph(session, [EntityTable("node", frozenset({label}), {}, nodes, id_col="id")],
                     [EntityTable("rel", frozenset({rtype}), {}, rels, id_col="id", src_col="source", dst_col="target")])


def _launches(session, name):
    from capsmi import _lib
    n, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", session.handle, name.encode(), ctypes.byref(n), ctypes.byref(ms))
    return n.value


@pytest.mark.parametrize("order", ["sorted", "shuffled_signed"])
def test_sparse_ids_are_routed(session, order):
    """Ids near 2^40, compacted (the construction of test_sparse_ids_equal_the_reference; and the same ids shuffled,
    half of them negated): grouped and ungrouped collect, with and without the count in either order, lower 1 and 0,
    each routed and equal to the reference.  The order of the ids is built once per compacted graph."""
    from capsmi import _lib
    rng = np.random.default_rng(5)
    ids = np.unique(rng.integers(1 << 40, (1 << 40) + (1 << 45), 300))
    if order == "shuffled_signed":
        ids = ids[rng.permutation(len(ids))]
        ids[::2] = -ids[::2]
    n, m = len(ids), 900
    s_i, d_i = rng.integers(0, n, m), rng.integers(0, n, m)
    s_i[: m // 50] = d_i[: m // 50]
    sg = _scan_graph(session, ids, s_i, d_i)
    ones = np.ones(n, bool)
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        _launches(session, "reach_list_order")  # reset
        for lo, hi in [(1, 3), (0, 2)]:
            lists, union = mapped_lists(n, s_i, d_i, ones, ones, lo, hi, ids)
            for grouped in (True, False):
                key = KEY if grouped else []
                for items, wc in ((key + [COLLECT], False), (key + [COUNT, COLLECT], True), (key + [COLLECT, COUNT], True)):
                    q = _query(lo, hi, items)
                    got = _routed(session, "var_length_distinct", lambda: _run(session, sg, q))
                    assert _norm(got) == _want(lists, union, grouped, with_count=wc), (lo, hi, grouped, wc)
        assert _launches(session, "reach_list_order") == 1  # kept with the compacted domain
        assert _launches(session, "reach_list_gather") >= 12
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)
    _routed(session, "var_length_distinct", lambda: _run(session, sg, _query(1, 3, KEY + [COUNT])))


def test_unrouted_limit(session):
    """R-MAT scale 8, ids spread near 2^40 and compacted, *1..3 grouped collect under the 1 GiB unrouted limit: the
    route takes the plan (before it did not: the plan stayed with the operator path and its guard) and equals the
    reference.  Without the limit the operator path gives the same rows."""
    from oracle import cpu
    scale = 8
    n = 1 << scale
    src, dst = cpu.rmat_edges(scale, 0, 32 << scale, (45, 15, 15), 42)
    rng = np.random.default_rng(6)
    ids = (1 << 40) + rng.permutation(n).astype(np.int64) * (1 << 24) + rng.integers(0, 1 << 20, n)
    sg = _scan_graph(session, ids, np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64))
    ones = np.ones(n, bool)
    lists, union = mapped_lists(n, src, dst, ones, ones, 1, 3, ids)
    q = _query(1, 3, KEY + [COLLECT])
    session.set_unrouted_limit(1 << 30)
    try:
        got = _routed(session, "var_length_distinct", lambda: _run(session, sg, q))
    finally:
        session.set_unrouted_limit(0)
    assert _norm(got) == _want(lists, union, True)
    assert _norm(_run(session, sg, q, fused=False)) == _norm(got)


@pytest.mark.parametrize("second_tag", [None, 600])
def test_tagged_union(session, second_tag):
    """Two small graphs with the same ids, retagged (capsmi/tagging.py: the second graph's tag 0 becomes 1, or a fixed
    tag 600, whose ids are negative Longs) and unioned, compacted: collect is routed -- this is the orig-table form, not
    the scrambled one -- and equals the operator path and the reference."""
    from capsmi import tagging
    rng = np.random.default_rng(7)
    k, m = 90, 260
    fixed = {} if second_tag is None else {"g2": {0: second_tag}}
    re = tagging.compute_retaggings({"g1": {0}, "g2": {0}}, fixed=fixed)
    assert re["g2"][0] == (1 if second_tag is None else second_tag)
    base = np.arange(k, dtype=np.int64) * 5 + 2
    ids = np.concatenate([np.array([tagging.replace_tags(int(x), re[g]) for x in base], dtype=np.int64)
                          for g in ("g1", "g2")])
    s_i = np.concatenate([rng.integers(0, k, m), k + rng.integers(0, k, m)])  # no relationship crosses the graphs
    d_i = np.concatenate([rng.integers(0, k, m), k + rng.integers(0, k, m)])
    sg = _scan_graph(session, ids, s_i, d_i)
    ones = np.ones(2 * k, bool)
    for lo, hi in [(1, 3), (0, 2)]:
        lists, union = mapped_lists(2 * k, s_i, d_i, ones, ones, lo, hi, ids)
        for items, grouped, wc in ((KEY + [COLLECT, COUNT], True, True), ([COLLECT], False, False)):
            q = _query(lo, hi, items)
            got = _routed(session, "var_length_distinct", lambda: _run(session, sg, q))
            assert _norm(got) == _want(lists, union, grouped, with_count=wc)
            assert _norm(_run(session, sg, q, fused=False)) == _norm(got)


def test_unremapped_graph_takes_the_old_kernels(session):
    """Plain ids: the same results as before, under the same timer names -- no gather, no order build."""
    from capsmi import _lib, graph
    from capsmi.planner import EntityTable, ScanGraph
    from oracle import cpu
    from varlen_collect_ref import reach_lists
    scale = 6
    n = 1 << scale
    rels = graph.rmat_rels(session, scale, 0, 32 << scale, (45, 15, 15), 42)
    nodes = graph.rmat_nodes(session, scale, graph.NODES_ALL, 42)
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    src, dst = cpu.rmat_edges(scale, 0, 32 << scale, (45, 15, 15), 42)
    ones = np.ones(n, bool)
    lists, union = reach_lists(n, src, dst, ones, ones, 0, 3)
    names = ["reach_list_starts", "reach_list_count", "reach_list_write", "reach_list_gather", "reach_list_order"]
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        for name in names:
            _launches(session, name)  # reset
        got = _routed(session, "var_length_distinct", lambda: _run(session, sg, _query(0, 3, KEY + [COLLECT, COUNT])))
        one = _routed(session, "var_length_distinct", lambda: _run(session, sg, _query(0, 3, [COLLECT])))
        seen = {name: _launches(session, name) for name in names}
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)
    assert _norm(got) == _want({a: v.tolist() for a, v in lists.items()}, union.tolist(), True, with_count=True)
    assert _norm(one) == _want({}, union.tolist(), False)
    # grouped: hit + self, colscan + scan, the final scan (starts x3), count x1, write x1; global: starts x1, write x1
    assert seen == {"reach_list_starts": 4, "reach_list_count": 1, "reach_list_write": 2, "reach_list_gather": 0,
                    "reach_list_order": 0}
