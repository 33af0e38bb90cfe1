"""Endpoint presence words (CAPSMI_PRESENCE=auto, the default: four bitmaps kept with a registered relationship
table -- non-loop targets, non-loop sources, ids with one / two self-loops; plan_entity.hip presence_endpoints) and hop 1
answered from them (k_part.hip k_presence_hop1) in place of k_pool_hop1 / k_hop_2d<HOP1>.

Every 2-hop case registers its tables and runs the cold 2-hop (RelPartition.build_mark_mid + mark_dst) under
CAPSMI_PRESENCE=auto and under off, and compares the mid words (X1, X2), hop 1's scratch S1, the end bitmap and
its popcount with the numpy restatements of pool_split_ref.py / pool_hop2_ref.py (pinned to the oracle in
test_pool_split_cpu.py / test_pool_hop2_cpu.py), and the two settings with each other.  With full masks the
words read back are the stored bitmaps themselves: X1 = in | loop1, X2 = in | loop2, S1 = loop1, and the walk
against the relationships gives out | loop1.

Two temporary mutations of the library, each of which fails this module (run on MI355X, 38 cases):
  - the funnel's shift taken as lo - tlo instead of tlo - lo (k_part.hip presence_hop1): 20 cases fail, every one
    whose table window does not start at the domain's low end;
  - l2 without the cross-table term `l1 & a` (k_presence_hop1): 2 cases fail, test_self_loops_on_one_id[1+1] and
    [1 twice]."""
import numpy as np
import pytest

import pool_hop2_ref as H
import pool_split_ref as R

pytestmark = pytest.mark.gpu

LO = 1000            # the domain's low end in most cases: ids are not word-aligned to zero anywhere by accident
N0 = 2000 + 17       # ids of the small domain: no multiple of 32


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)),
                          ColumnData("source", I64, np.asarray(src, np.int64)),
                          ColumnData("target", I64, np.asarray(dst, np.int64))])


def _reg(session, src, dst, built=1):
    """the registered table; asserts how many registrations made words"""
    before = session.route_count("presence_built")
    t = _table(session, src, dst).as_rel_table("id", "source", "target")
    assert session.route_count("presence_built") == before + built
    return t


def _bitmap(session, lo, n, mask=None):
    from capsmi import ColumnData, I64, graph
    ids = np.arange(n, dtype=np.int64) if mask is None else np.nonzero(mask)[0].astype(np.int64)
    return graph.NodeBitmap(session, lo, lo + n).add_scan(session.table([ColumnData("id", I64, ids + lo)]))


def _cold(session, knobs, mode, tables, a, b, c, n, cols=("source", "target")):
    """one cold 2-hop: words, popcount and what ran"""
    import torch
    from capsmi import graph
    knobs(session, CAPSMI_PRESENCE=mode)
    nw = (n + 31) // 32
    mid = torch.zeros(2 * nw, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(nw, dtype=torch.int32, device="cuda")
    end = torch.zeros(nw, dtype=torch.int32, device="cuda")
    h0, p0 = session.route_count("hop1_presence"), session.route_count("pool_split")
    rp = graph.RelPartition.build_mark_mid(session, tables, a, b, mid.data_ptr(), scratch.data_ptr(), *cols)
    rp.mark_dst(b, c, mid.data_ptr(), end.data_ptr())
    session.sync()
    cnt = graph.words_popcount(session, end.data_ptr(), 0, nw)
    rp.release()
    x = mid.cpu().numpy().view(np.uint32)
    return {"x1": x[:nw], "x2": x[nw:], "s1": scratch.cpu().numpy().view(np.uint32),
            "c": end.cpu().numpy().view(np.uint32), "count": cnt,
            "hop1": session.route_count("hop1_presence") - h0, "split": session.route_count("pool_split") - p0}


def _expect(graphs, lo, n, b=None, c=None):
    src = np.concatenate([g[0] for g in graphs]) - lo
    dst = np.concatenate([g[1] for g in graphs]) - lo
    w1, w2 = R.frontier(n, src, dst, b)
    k = R.inside(n, src, dst)
    loops = np.bincount(dst[k][src[k] == dst[k]], minlength=n) >= 1
    if b is not None:
        loops &= np.asarray(b).astype(bool)
    cb = H.hop2_bits(n, src, dst, b, c)
    return {"x1": R.words(w1), "x2": R.words(w2), "s1": R.words(loops), "c": R.words(cb), "count": int(cb.sum())}


def _check(session, knobs, tables, graphs, lo=LO, n=N0, a=None, b=None, c=None, presence=1, split=1, bm=None,
           cols=("source", "target")):
    """both settings against the restatement and each other; which hop 1 ran"""
    bm = bm or {}
    full = bm["full"] if "full" in bm else _bitmap(session, lo, n)
    am = full if a is None else _bitmap(session, lo, n, a)
    bb = full if b is None else _bitmap(session, lo, n, b)
    cc = full if c is None else _bitmap(session, lo, n, c)
    if cols != ("source", "target"):
        graphs = [(g[1], g[0]) for g in graphs]
    want = _expect(graphs, lo, n, b, c) if a is None else None
    got = {}
    for mode in ("auto", "off"):
        got[mode] = g = _cold(session, knobs, mode, tables, am, bb, cc, n, cols)
        assert g["hop1"] == (presence if mode == "auto" else 0), (mode, g["hop1"])
        assert g["split"] == split, (mode, g["split"])
        if want is not None:
            for k in ("x1", "x2", "s1", "c"):
                np.testing.assert_array_equal(g[k], want[k], err_msg=f"{mode} {k}")
            assert g["count"] == want["count"]
    for k in ("x1", "x2", "s1", "c"):
        np.testing.assert_array_equal(got["auto"][k], got["off"][k], err_msg=k)
    assert got["auto"]["count"] == got["off"]["count"]
    knobs(session, CAPSMI_PRESENCE="auto")  # a later registration of the same test builds its words again
    return got["auto"]


def _graph(seed, rows, tlo, thi, loops=3):
    """`rows` relationships whose endpoints span exactly [tlo, thi), a few self-loops (one id with two)"""
    rng = np.random.default_rng(seed)
    src = rng.integers(tlo, thi, rows).astype(np.int64)
    dst = rng.integers(tlo, thi, rows).astype(np.int64)
    if rows >= 5 and loops:
        at = rng.choice(np.arange(1, rows), min(loops + 1, rows - 1), replace=False)
        src[at] = dst[at]
        src[at[1]] = dst[at[1]] = dst[at[0]]  # a second loop at the first one's id
    if thi - tlo == 1:
        return src, dst
    dst[0], src[0] = tlo, thi - 1  # the window's two ends
    return src, dst


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 8191, 8192, 8193, 2 * 8192 + 5])
def test_rows(session, knobs, rows):
    g = _graph(rows, rows, LO, LO + N0)
    _check(session, knobs, [_reg(session, *g)], [g])


@pytest.mark.parametrize("d", [0, 1, 31, 32, 33])
def test_window_below_the_domains_low_end_by(session, knobs, d):
    """the table's window starts d ids above the domain's low end: the funnel's shift"""
    g = _graph(100 + d, 300, LO + d, LO + d + 700)
    _check(session, knobs, [_reg(session, *g)], [g])


@pytest.mark.parametrize("end", [63, 64, 65, 95, 96, 97])
def test_window_end_at_a_word_boundary(session, knobs, end):
    """the table's own last word: one bit short of full, full, one bit into the next; under two shifts"""
    for d in (0, 7):
        g = _graph(200 + end, 200, LO + d, LO + d + end)
        _check(session, knobs, [_reg(session, *g)], [g])


def test_single_last_id_of_the_domain(session, knobs):
    last = LO + N0 - 1
    g = (np.array([last, last], np.int64), np.array([last, last], np.int64))
    got = _check(session, knobs, [_reg(session, *g)], [g])
    assert got["count"] == 1 and got["x2"][-1] == 1 << ((N0 - 1) & 31)


V = LO + 333  # the id of the self-loop cases; it has one out-relationship, so X1 / X2 at it decide the end bitmap


def _loops(k, extra=True):
    src, dst = [V] * k + [V, LO + 5], [V] * k + [LO + 700, LO + 6]
    if not extra:
        src, dst = src[:-1], dst[:-1]
    return np.array(src, np.int64), np.array(dst, np.int64)


@pytest.mark.parametrize("case", ["1", "2", "3", "1+1", "1+0", "1 twice"])
def test_self_loops_on_one_id(session, knobs, case):
    if case in ("1", "2", "3"):
        graphs = [_loops(int(case))]
        tabs = [_reg(session, *graphs[0])]
    elif case == "1 twice":  # the same table listed twice counts twice
        g = _loops(1)
        t = _reg(session, *g)
        graphs, tabs = [g, g], [t, t]
    else:
        graphs = [_loops(1), _loops(int(case[-1]))]
        tabs = [_reg(session, *g) for g in graphs]
    got = _check(session, knobs, tabs, graphs)
    r = V - LO
    bit = lambda x: (int(x[r >> 5]) >> (r & 31)) & 1  # noqa: E731
    assert bit(got["x1"]) == 1 and bit(got["s1"]) == 1
    assert bit(got["x2"]) == (0 if case in ("1", "1+0") else 1)


def test_two_tables_with_different_windows(session, knobs):
    gs = [_graph(301, 500, LO + 3, LO + 900), _graph(302, 9000, LO + 650, LO + N0)]
    _check(session, knobs, [_reg(session, *g) for g in gs], gs)


def test_one_table_without_words_falls_back(session, knobs):
    gs = [_graph(303, 500, LO + 3, LO + 900), _graph(304, 700, LO + 650, LO + N0)]
    _check(session, knobs, [_reg(session, *gs[0]), _table(session, *gs[1])], gs, presence=0)


def _masks():
    rng = np.random.default_rng(310)
    b = (rng.random(N0) < 0.7).astype(np.uint8)
    b[[0, 5, 31, 32 * 20 + 3, N0 - 1, N0 - 9]] = 0  # off inside the first, a middle and the last word
    b[[1, 32 * 20 + 4, N0 - 2]] = 1
    return b, (rng.random(N0) < 0.6).astype(np.uint8)


def test_partial_b_and_c(session, knobs):
    b, c = _masks()
    g = _graph(311, 6000, LO, LO + N0, loops=40)
    t = _reg(session, *g)
    _check(session, knobs, [t], [g], b=b)
    _check(session, knobs, [t], [g], c=c)
    _check(session, knobs, [t], [g], b=b, c=c)


def test_partial_a_falls_back(session, knobs):
    """a filtered first node: hop 1 needs the sources, no pool hop at all"""
    from oracle import cpu
    b, c = _masks()
    g = _graph(312, 6000, LO, LO + N0, loops=40)
    got = _check(session, knobs, [_reg(session, *g)], [g], a=c, b=b, presence=0, split=0)
    full = np.ones(N0, np.uint8)
    assert got["count"] == cpu.two_hop_enumerate(N0, g[0] - LO, g[1] - LO, c, b, full)[1]


def test_row_outside_the_domain_falls_back(session, knobs):
    """the table's window overhangs the domain on either side: pass 1 drops rows that the words have counted"""
    for out in (LO - 50, LO + N0):
        src, dst = _graph(313, 400, LO, LO + N0)
        src[7] = out
        _check(session, knobs, [_reg(session, src, dst)], [(src, dst)], presence=0)


@pytest.fixture(scope="module")
def wide(session):
    """the widest domain with words: 2^26 ids (128 target slices)"""
    from capsmi import graph
    n = 1 << 26
    return n, graph.NodeBitmap(session, 0, n).add_scan(graph.rmat_nodes(session, 26, graph.NODES_ALL), "id")


def test_widest_domain_rows_at_its_ends(session, knobs, wide):
    """a window of exactly 2^26 ids: built; the last word and the last slice"""
    n, full = wide
    src = np.array([0, 1, n - 1, n - 1, n - 2, 1, n - 1], np.int64)
    dst = np.array([1, n - 1, n - 1, 0, n - 1, 1, n - 2], np.int64)
    got = _check(session, knobs, [_reg(session, src, dst)], [(src, dst)], lo=0, n=n, bm={"full": full})
    assert got["x1"][-1] == 3 << 30 and got["x1"][0] == 3


def test_window_of_one_id_more_is_not_built(session, knobs, wide):
    n, full = wide
    src = np.array([0, 1, 5, n], np.int64)
    dst = np.array([1, 5, 5, 7], np.int64)
    _check(session, knobs, [_reg(session, src, dst, built=0)], [(src, dst)], lo=0, n=n, bm={"full": full}, presence=0)


def test_views(session, knobs):
    src, dst = _graph(320, 3000, LO, LO + N0, loops=20)
    t = _reg(session, src, dst)
    _check(session, knobs, [t], [(src, dst)])
    # registered behind a skip: the words are made under the row offset
    before = session.route_count("presence_built")
    ts = _table(session, src, dst).skip(1).as_rel_table("id", "source", "target")
    assert session.route_count("presence_built") == before + 1
    _check(session, knobs, [ts], [(src[1:], dst[1:])])
    # registered, then skipped or limited: other rows than the words were made from
    _check(session, knobs, [t.skip(1)], [(src[1:], dst[1:])], presence=0)
    _check(session, knobs, [t.limit(2999)], [(src[:2999], dst[:2999])], presence=0)
    # a second handle on the same columns, as the benchmark makes it: reused, not rebuilt
    built, reused = session.route_count("presence_built"), session.route_count("presence_reused")
    t2 = t.select("id", "source", "target").as_rel_table("id", "source", "target").cache()
    assert session.route_count("presence_built") == built and session.route_count("presence_reused") == reused + 1
    _check(session, knobs, [t2], [(src, dst)])
    # renamed endpoint columns carry the words along
    _check(session, knobs, [t.select("source", "target")], [(src, dst)])


def test_walk_against_the_relationships_reads_out(session, knobs):
    """the same table walked from target to source: M is `out`"""
    g = _graph(330, 5000, LO + 33, LO + 1500, loops=30)
    _check(session, knobs, [_reg(session, *g)], [g], cols=("target", "source"))


def test_count_distinct_a_through_the_planner(session, knobs):
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, Planner, ScanGraph, result_rows
    from oracle import cpu
    n = 3000
    src, dst = _graph(331, 20000, 40, n - 100, loops=50)
    nodes = session.table([ColumnData("id", I64, np.arange(n, dtype=np.int64))]).as_node_table("id")
    rels = _reg(session, src, dst)
    sg = ScanGraph(session, [EntityTable("node", frozenset({"N"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"R"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    q = {"clauses": [{"match": "(a:N)-[:R]->(b:N)-[:R]->(c:N)"}],
         "return": {"items": [["a", ["count_distinct", ["id", "a"]]], ["c", ["count_distinct", ["id", "c"]]]]}}
    want = {"a": cpu.two_hop_enumerate(n, dst, src)[1], "c": cpu.two_hop_enumerate(n, src, dst)[1]}
    for mode, hops in (("auto", 2), ("off", 0)):
        knobs(session, CAPSMI_PRESENCE=mode)
        before = session.route_count("hop1_presence")
        t, outs = Planner(sg).run(q)
        assert result_rows(t, outs, session.dictionary) == [want]
        assert session.route_count("hop1_presence") == before + hops  # one from `in`, one from `out`


def test_warm_handle(session, knobs):
    """a layout built once (capsmi_relpart_build keeps the tables' words): mark_mid with a full a reads them,
    with a partial a walks the cells"""
    import torch
    from capsmi import graph
    from oracle import cpu
    b, c = _masks()
    g = _graph(340, 9000, LO + 1, LO + N0 - 40, loops=40)
    t = _reg(session, *g)
    full, bb, am = _bitmap(session, LO, N0), _bitmap(session, LO, N0, b), _bitmap(session, LO, N0, c)
    nw = (N0 + 31) // 32
    rp = graph.RelPartition(session, [t], LO, LO + N0)
    words = {}
    for mode in ("auto", "off"):
        knobs(session, CAPSMI_PRESENCE=mode)
        for name, (a, bx, hops) in {"full": (full, full, 1), "b": (full, bb, 1), "a": (am, bb, 0)}.items():
            mid = torch.zeros(2 * nw, dtype=torch.int32, device="cuda")
            scratch = torch.zeros(nw, dtype=torch.int32, device="cuda")
            before = session.route_count("hop1_presence")
            rp.mark_mid(a, bx, mid.data_ptr(), scratch.data_ptr())
            session.sync()
            assert session.route_count("hop1_presence") == before + (hops if mode == "auto" else 0)
            words[mode, name] = np.concatenate([mid.cpu().numpy().view(np.uint32), scratch.cpu().numpy().view(np.uint32)])
        want = _expect([g], LO, N0)
        np.testing.assert_array_equal(words[mode, "full"], np.concatenate([want["x1"], want["x2"], want["s1"]]))
        want = _expect([g], LO, N0, b)
        np.testing.assert_array_equal(words[mode, "b"], np.concatenate([want["x1"], want["x2"], want["s1"]]))
        assert rp.count_distinct(am, bb, full) == cpu.two_hop_enumerate(N0, g[0] - LO, g[1] - LO, c, b,
                                                                      np.ones(N0, np.uint8))[1]
    for name in ("full", "b", "a"):
        np.testing.assert_array_equal(words["auto", name], words["off", name])
    rp.release()


def test_knob_off_builds_no_words(session, knobs):
    knobs(session, CAPSMI_PRESENCE="off")
    g = _graph(350, 100, LO, LO + N0)
    t = _reg(session, *g, built=0)
    knobs(session, CAPSMI_PRESENCE="auto")
    got = _cold(session, knobs, "auto", [t], *[_bitmap(session, LO, N0)] * 3, N0)
    assert got["hop1"] == 0 and got["count"] == _expect([g], LO, N0)["count"]
