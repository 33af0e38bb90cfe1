"""Pass 1 of the relationship partition without the per-chunk cell counts (k_part.hip k_scatter_l / k_scatter_c
with HIST = false: the cold 2-hop over the pool, CAPSMI_HOP2=pool) and k_chunk_hist, which makes those counts
afterwards when a kept handle builds its cells after all.

One graph serves most cases: 3 * 2^19 + 1000 ids (three full target slices and a short fourth), 2^18 + 5
relationships (not a multiple of 16), of which
- about 85 % have their target in slice 1, so a block's tiles put more than one chunk (8192 pairs) there: runs
  cross a chunk boundary and chunks retire full;
- 9 in all have their target in slice 2 (fewer than one 16-pair line: the slice is a held tail only);
- none has its target in the short slice 3;
- a few are self-loops, and a few have an endpoint outside the domain (below 0, at N and far above it).
The layout check is the digest of the cells (per cell the pair count and a wrapping sum of a 64-bit mix of the
pair) against a numpy grouping of the in-domain pairs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S = 1 << 19
N = 3 * S + 1000
M = (1 << 18) + 5


def _mix64(x):
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _np_digest(lo, hi, src, dst, ncells, ns, sbits, tbits):
    keep = (src >= lo) & (src < hi) & (dst >= lo) & (dst < hi)
    x, y = (src[keep] - lo).astype(np.uint64), (dst[keep] - lo).astype(np.uint64)
    cell = (y >> np.uint64(tbits)).astype(np.int64) * ns + (x >> np.uint64(sbits)).astype(np.int64)
    want_n = np.bincount(cell, minlength=ncells)
    want_s = np.zeros(ncells, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(want_s, cell, _mix64((x << np.uint64(32)) | y))
    return want_n, want_s, int(keep.sum())


def _check_digest(digest, size, lo, hi, src, dst):
    counts, sums, bad, (ns, sbits, tbits) = digest
    want_n, want_s, kept = _np_digest(lo, hi, src, dst, len(counts), ns, sbits, tbits)
    assert bad == 0
    assert size == kept
    np.testing.assert_array_equal(counts, want_n)
    np.testing.assert_array_equal(sums, want_s)


def _build_graph():
    rng = np.random.default_rng(41)
    dst = np.where(rng.random(M) < 0.85, S + rng.integers(0, S, M), rng.integers(0, S, M)).astype(np.int64)
    src = rng.integers(0, 2 * S, M).astype(np.int64)  # sources in slices 0 and 1: every middle can have out-rels
    at = rng.choice(M, 9 + 40 + 12, replace=False)
    dst[at[:9]] = 2 * S + rng.integers(0, S, 9)  # slice 2: nine pairs
    src[at[9:49]] = dst[at[9:49]]                # self-loops
    src[at[49:53]] = -3                          # outside the domain
    dst[at[53:57]] = N
    src[at[57:61]] = N + (1 << 33)
    inside = (src >= 0) & (src < N) & (dst >= 0) & (dst < N)
    masks = {"full": np.ones(N, np.uint8), "a": (rng.random(N) < 0.8).astype(np.uint8),
             "b": (rng.random(N) < 0.7).astype(np.uint8), "c": (rng.random(N) < 0.6).astype(np.uint8)}
    return src, dst, inside, masks


@pytest.fixture(scope="module")
def G():
    src, dst, inside, masks = _build_graph()
    return {"src": src, "dst": dst, "inside": inside, "masks": masks, "want": {}}


def _want(G, a, b, c):
    """enumeration's count(DISTINCT c) over the in-domain relationships, once per filter triple"""
    from oracle import cpu
    if (a, b, c) not in G["want"]:
        m, k = G["masks"], G["inside"]
        G["want"][(a, b, c)] = cpu.two_hop_enumerate(N, G["src"][k], G["dst"][k], m[a], m[b], m[c])[1]
    return G["want"][(a, b, c)]


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


def _pool_handle(session, knobs, tables, full):
    """a handle whose pass 1 ran without the cell counts: the cold build with a full a_ok over the pool"""
    import torch
    from capsmi import graph
    knobs(session, CAPSMI_HOP2="pool")
    nw = (N + 31) // 32
    mid = torch.zeros(2 * nw, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(nw, dtype=torch.int32, device="cuda")
    rp = graph.RelPartition.build_mark_mid(session, tables, full, full, mid.data_ptr(), scratch.data_ptr())
    session.sync()
    return rp


def test_graph_has_the_shapes(G):
    """host only: what the cases below rely on"""
    src, dst, k = G["src"], G["dst"], G["inside"]
    per_slice = np.bincount(dst[k] >> 19, minlength=4)
    assert M % 16 != 0 and int(k.sum()) % 16 != 0
    assert per_slice[1] > 0.8 * M and 0 < per_slice[2] < 16 and per_slice[3] == 0
    assert (src[k] == dst[k]).sum() >= 30 and (~k).sum() >= 8
    # a pass-1 block walks two 8192-row tiles of this table (16 blocks): together they bring slice 1 more than a chunk
    tiles = (dst[:32 * 8192] >> 19 == 1).reshape(32, 8192).sum(axis=1)
    assert ((tiles[:16] + tiles[16:]) > 8192).all()


def test_lazy_rows_equal_in_pass_rows(session, knobs, G, dev):
    """the cells of a handle built over the pool (k_chunk_hist makes the rows when digest() asks for the cells)
    against those of a handle whose pass 1 counted them, and against numpy; then the same handle answers a
    query with a partial a_ok (hop 1 over the cells)"""
    from capsmi import graph
    bm = dev["bm"]
    before = session.route_count("chunk_hist")
    rp = _pool_handle(session, knobs, [dev["rels"]], bm["full"])
    assert session.route_count("chunk_hist") == before  # nothing has asked for the cells yet
    lazy = rp.digest()
    assert session.route_count("chunk_hist") == before + 1
    ref = graph.RelPartition(session, [dev["rels"]], 0, N)
    inpass = ref.digest()
    assert session.route_count("chunk_hist") == before + 1  # the cached build counts in pass 1
    assert lazy[3] == inpass[3]
    np.testing.assert_array_equal(lazy[0], inpass[0])
    np.testing.assert_array_equal(lazy[1], inpass[1])
    assert lazy[2] == 0 and inpass[2] == 0
    _check_digest(lazy, rp.size, 0, N, G["src"], G["dst"])
    assert rp.size == ref.size == int(G["inside"].sum())
    assert rp.count_distinct(bm["a"], bm["b"], bm["c"]) == _want(G, "a", "b", "c")
    assert ref.count_distinct(bm["a"], bm["b"], bm["c"]) == _want(G, "a", "b", "c")
    rp.release()
    ref.release()


@pytest.mark.parametrize("b,c", [("full", "full"), ("b", "c")])
def test_answers_pool_and_cells(session, knobs, G, dev, b, c):
    from capsmi import graph
    bm = dev["bm"]
    want = _want(G, "full", b, c)
    for mode in ("pool", "cells"):
        knobs(session, CAPSMI_HOP2=mode)
        name = "hop2_" + mode
        before = session.route_count(name)
        assert graph.two_hop_count_distinct(session, [dev["rels"]], bm["full"], bm[b], bm[c]) == want, mode
        assert session.route_count(name) == before + 1, f"forced {mode} did not run hop 2 over the {mode}"


@pytest.mark.parametrize("rows", [0, 1, 15, 16, 8191, 8192, 8193])
def test_tile_loop_edges(session, knobs, G, dev, rows):
    """a table that ends before, at and after a line and a tile"""
    src, dst = G["src"][:rows], G["dst"][:rows]
    rp = _pool_handle(session, knobs, [_table(session, src, dst)], dev["bm"]["full"])
    _check_digest(rp.digest(), rp.size, 0, N, src, dst)
    rp.release()


def test_two_tables_in_one_build(session, knobs, G, dev):
    """two pass-1 launches into one pool"""
    src, dst = G["src"], G["dst"]
    cut = M // 3 + 7
    tabs = [_table(session, src[:cut], dst[:cut]), _table(session, src[cut:], dst[cut:])]
    rp = _pool_handle(session, knobs, tabs, dev["bm"]["full"])
    _check_digest(rp.digest(), rp.size, 0, N, src, dst)
    rp.release()


def test_columns_off_the_vector_boundary(session, knobs, G, dev):
    """skip(1) is a view one row into the table's columns: they start 8 bytes off a 16-byte boundary, so pass 1
    takes its scalar loads"""
    src, dst = G["src"][:3 * 8192 + 100], G["dst"][:3 * 8192 + 100]
    view = _table(session, src, dst).skip(1)
    rp = _pool_handle(session, knobs, [view], dev["bm"]["full"])
    _check_digest(rp.digest(), rp.size, 0, N, src[1:], dst[1:])
    rp.release()


def test_above_128_target_slices(session):
    """2^27 ids = 256 target slices: k_scatter_c, whose layouts always go on to the cells (cell counts in pass 1)"""
    from capsmi import graph
    n = 1 << 27
    rng = np.random.default_rng(43)
    m = 5003
    src = rng.integers(0, n, m).astype(np.int64)
    dst = np.where(rng.random(m) < 0.5, rng.integers(0, 1 << 12, m), rng.integers(0, n, m)).astype(np.int64)
    src[::101] = dst[::101]
    before = session.route_count("chunk_hist")
    rp = graph.RelPartition(session, [_table(session, src, dst)], 0, n)
    _check_digest(rp.digest(), rp.size, 0, n, src, dst)
    assert session.route_count("chunk_hist") == before
    rp.release()
