"""The split pass-1 pool (CAPSMI_POOL=split, the default: per chunk an array of target words with the self-loop
flag in bit 31 and an array of source words; k_part.hip k_scatter_l<SPLIT>, k_pool_hop1<true>, k_pool_hop2<true>,
and k_chunk_hist / k_scatter_s2 reading it when a kept handle builds its cells) against the CPU oracle's
enumeration and the numpy restatements of pool_split_ref.py (checked against the oracle in
test_pool_split_cpu.py), under both pool formats."""
import numpy as np
import pytest

import pool_split_ref as R

pytestmark = pytest.mark.gpu

N = R.N
NW = (N + 31) // 32
FORMATS = ("split", "pairs")


@pytest.fixture(scope="module")
def G():
    src, dst, masks = R.main_graph()
    return {"src": src, "dst": dst, "masks": masks, "want": {}}


def _want(G, b, c):
    """enumeration's count(DISTINCT c) with a full a_ok, once per filter pair"""
    from oracle import cpu
    if (b, c) not in G["want"]:
        m, k = G["masks"], R.inside(N, G["src"], G["dst"])
        G["want"][(b, c)] = cpu.two_hop_enumerate(N, G["src"][k], G["dst"][k], m["full"], m[b], m[c])[1]
    return G["want"][(b, c)]


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)),
                          ColumnData("source", I64, np.asarray(src, np.int64)),
                          ColumnData("target", I64, np.asarray(dst, np.int64))])


def _bitmap(session, n, mask):
    from capsmi import ColumnData, I64, graph
    t = session.table([ColumnData("id", I64, np.nonzero(mask)[0].astype(np.int64))])
    return graph.NodeBitmap(session, 0, n).add_scan(t)


@pytest.fixture(scope="module")
def dev(session, G):
    return {"rels": _table(session, G["src"], G["dst"]),
            "bm": {k: _bitmap(session, N, m) for k, m in G["masks"].items()}}


def _hop1(session, knobs, fmt, tables, full, b, n=N):
    """the cold build with a full a_ok over the pool: the handle and hop 1's words (X1, X2)"""
    import torch
    from capsmi import graph
    knobs(session, CAPSMI_HOP2="pool", CAPSMI_POOL=fmt)
    nw = (n + 31) // 32
    mid = torch.zeros(2 * nw, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(nw, dtype=torch.int32, device="cuda")
    before = session.route_count("pool_split")
    rp = graph.RelPartition.build_mark_mid(session, tables, full, b, mid.data_ptr(), scratch.data_ptr())
    session.sync()
    split = session.route_count("pool_split") - before
    x = mid.cpu().numpy().view(np.uint32)
    return rp, x[:nw], x[nw:], split


def _check_frontier(x1, x2, src, dst, b_ok=None, n=N):
    w1, w2 = R.frontier(n, src, dst, b_ok)
    np.testing.assert_array_equal(x1, R.words(w1))
    np.testing.assert_array_equal(x2, R.words(w2))


def _check_digest(rp, src, dst, n=N):
    counts, sums, bad, (ns, sbits, tbits) = rp.digest()
    want_n, want_s, kept = R.np_digest(n, src, dst, len(counts), ns, sbits, tbits)
    assert bad == 0 and rp.size == kept
    np.testing.assert_array_equal(counts, want_n)
    np.testing.assert_array_equal(sums, want_s)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("b", ["full", "b"])
def test_hop1_words(session, knobs, G, dev, fmt, b):
    """hop 1's output itself, and which pool format ran"""
    rp, x1, x2, split = _hop1(session, knobs, fmt, [dev["rels"]], dev["bm"]["full"], dev["bm"][b])
    assert split == (1 if fmt == "split" else 0)
    _check_frontier(x1, x2, G["src"], G["dst"], G["masks"][b])
    rp.release()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("b,c", [("full", "full"), ("b", "c")])
def test_count_distinct(session, knobs, G, dev, fmt, b, c):
    from capsmi import graph
    bm = dev["bm"]
    knobs(session, CAPSMI_HOP2="pool", CAPSMI_POOL=fmt)
    pool, split = session.route_count("hop2_pool"), session.route_count("pool_split")
    assert graph.two_hop_count_distinct(session, [dev["rels"]], bm["full"], bm[b], bm[c]) == _want(G, b, c)
    assert session.route_count("hop2_pool") == pool + 1
    assert session.route_count("pool_split") == split + (1 if fmt == "split" else 0)


def test_cells_from_the_split_pool(session, knobs, G, dev):
    """a kept handle asked for its cells: k_chunk_hist and pass 2 read the two arrays; then a partial a_ok"""
    from oracle import cpu
    bm = dev["bm"]
    rp, _, _, split = _hop1(session, knobs, "split", [dev["rels"]], bm["full"], bm["full"])
    assert split == 1
    _check_digest(rp, G["src"], G["dst"])
    k = R.inside(N, G["src"], G["dst"])
    m = G["masks"]
    want = cpu.two_hop_enumerate(N, G["src"][k], G["dst"][k], m["c"], m["b"], m["c"])[1]
    assert rp.count_distinct(bm["c"], bm["b"], bm["c"]) == want
    rp.release()


@pytest.mark.parametrize("rows", [0, 1, 31, 32, 33, 8191, 8192, 8193])
def test_line_edges_one_slice(session, knobs, dev, rows):
    """a table that ends before, at and after a 32-pair line and a tile, all into one slice"""
    src, dst = R.one_slice_table(rows)
    rp, x1, x2, split = _hop1(session, knobs, "split", [_table(session, src, dst)], dev["bm"]["full"], dev["bm"]["full"])
    assert split == (1 if rows else 0)  # no rows: no pool hop, no pool
    _check_frontier(x1, x2, src, dst)
    _check_digest(rp, src, dst)
    rp.release()


@pytest.mark.parametrize("extra", [(2, R.LINE), (0, 5)], ids=["a-line-per-tile", "held-tail-only"])
def test_line_edges_side_slice(session, knobs, dev, extra):
    """beside a busy slice: one that receives exactly one 32-pair line per tile, and one that only ever holds
    fewer than 32 pairs (flushed at the end of pass 1)"""
    src, dst = R.one_slice_table(4 * R.TILE, extra_per_tile=extra)
    rp, x1, x2, split = _hop1(session, knobs, "split", [_table(session, src, dst)], dev["bm"]["full"], dev["bm"]["full"])
    assert split == 1
    _check_frontier(x1, x2, src, dst)
    _check_digest(rp, src, dst)
    rp.release()


@pytest.mark.parametrize("fmt", FORMATS)
def test_self_loops_and_bit_31(session, knobs, dev, fmt):
    from capsmi import graph
    from oracle import cpu
    src, dst = R.loops_graph()
    full = dev["bm"]["full"]
    tab = _table(session, src, dst)
    rp, x1, x2, _ = _hop1(session, knobs, fmt, [tab], full, full)
    _check_frontier(x1, x2, src, dst)
    bit = lambda x, v: (int(x[v >> 5]) >> (v & 31)) & 1
    assert bit(x1, R.ONE_LOOP_ONLY) and not bit(x2, R.ONE_LOOP_ONLY)
    assert bit(x1, R.TWO_LOOPS_ONLY) and bit(x2, R.TWO_LOOPS_ONLY)
    assert bit(x2, R.ONE_LOOP_ONE_IN) and bit(x2, R.SAME_OFFSET[1])
    _check_digest(rp, src, dst)
    rp.release()
    assert graph.two_hop_count_distinct(session, [tab], full, full, full) == cpu.two_hop_enumerate(N, src, dst)[1]


@pytest.mark.parametrize("fill", [1, R.STEP - 1, R.STEP, R.STEP + 1, R.TILE])
def test_chunk_fill_edges(session, knobs, dev, fill):
    """a chunk that ends before, at and after hop 1's 1024-target wave step, and a full one"""
    from capsmi import graph
    from oracle import cpu
    src, dst = R.fill_table(fill)
    full = dev["bm"]["full"]
    tab = _table(session, src, dst)
    rp, x1, x2, split = _hop1(session, knobs, "split", [tab], full, full)
    assert split == 1
    _check_frontier(x1, x2, src, dst)
    rp.release()
    assert graph.two_hop_count_distinct(session, [tab], full, full, full) == cpu.two_hop_enumerate(N, src, dst)[1]


def test_two_tables_one_off_the_vector_boundary(session, knobs, G, dev):
    """two pass-1 launches into one split pool, the first table's columns 8 bytes off a 16-byte boundary"""
    src, dst = G["src"], G["dst"]
    cut = R.M // 3 + 7
    tabs = [_table(session, src[:cut], dst[:cut]).skip(1), _table(session, src[cut:], dst[cut:])]
    rp, x1, x2, split = _hop1(session, knobs, "split", tabs, dev["bm"]["full"], dev["bm"]["full"])
    assert split == 1
    _check_frontier(x1, x2, src[1:], dst[1:])
    _check_digest(rp, src[1:], dst[1:])
    rp.release()


def test_above_128_target_slices_keeps_pairs(session, knobs):
    """2^27 ids = 256 target slices: pass 1 is k_scatter_c, the pool stays pairs, the pool hops still answer.
    The oracle enumerates the same graph with its ids renumbered densely (the count does not depend on names)."""
    from capsmi import graph
    from oracle import cpu
    logn = 27
    n = 1 << logn
    rng = np.random.default_rng(67)
    m = 5003
    src = rng.integers(0, 1 << 12, m).astype(np.int64)
    dst = np.where(rng.random(m) < 0.5, rng.integers(0, 1 << 12, m), rng.integers(0, n, m)).astype(np.int64)
    src[::101] = dst[::101]
    full = graph.NodeBitmap(session, 0, n).add_scan(graph.rmat_nodes(session, logn, graph.NODES_ALL), "id")
    tab = _table(session, src, dst)
    knobs(session, CAPSMI_HOP2="pool", CAPSMI_POOL="split")
    pool, split = session.route_count("hop2_pool"), session.route_count("pool_split")
    got = graph.two_hop_count_distinct(session, [tab], full, full, full)
    assert session.route_count("hop2_pool") == pool + 1 and session.route_count("pool_split") == split
    ids, dense = np.unique(np.concatenate([src, dst]), return_inverse=True)
    assert got == cpu.two_hop_enumerate(len(ids), dense[:m].astype(np.int64), dense[m:].astype(np.int64))[1]
