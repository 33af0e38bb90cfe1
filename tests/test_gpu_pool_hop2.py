"""Hop 2 over the split pass-1 pool (k_part.hip k_pool_hop2<true>: the pipelined walk of both arrays with the
source lines read on demand, part::walk_chunks_st_pipe) word for word against the numpy restatement of
pool_hop2_ref.py (pinned to the CPU oracle's enumeration in test_pool_hop2_cpu.py): build_mark_mid, then
mark_dst, under CAPSMI_HOP2=pool, and all of the end bitmap compared."""
import numpy as np
import pytest

import pool_hop2_ref as R
import pool_split_ref as P

pytestmark = pytest.mark.gpu

N = R.N
NW = (N + 31) // 32


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)),
                          ColumnData("source", I64, np.asarray(src, np.int64)),
                          ColumnData("target", I64, np.asarray(dst, np.int64))])


def _bitmap(session, mask):
    from capsmi import ColumnData, I64, graph
    t = session.table([ColumnData("id", I64, np.nonzero(mask)[0].astype(np.int64))])
    return graph.NodeBitmap(session, 0, N).add_scan(t)


@pytest.fixture(scope="module")
def main():
    src, dst, masks = P.main_graph()
    return {"src": src, "dst": dst, "masks": masks}


@pytest.fixture(scope="module")
def bm(session, main):
    return {k: _bitmap(session, m) for k, m in main["masks"].items()}


def _end_words(session, knobs, fmt, src, dst, full, b, c):
    """the cold build with a full a_ok and both hops over the pool: hop 2's end bitmap as words"""
    import torch
    from capsmi import graph
    knobs(session, CAPSMI_HOP2="pool", CAPSMI_POOL=fmt)
    mid = torch.zeros(2 * NW, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(NW, dtype=torch.int32, device="cuda")
    dstw = torch.zeros(NW, dtype=torch.int32, device="cuda")
    pool, split = session.route_count("hop2_pool"), session.route_count("pool_split")
    rp = graph.RelPartition.build_mark_mid(session, [_table(session, src, dst)], full, b, mid.data_ptr(),
                                           scratch.data_ptr())
    rp.mark_dst(b, c, mid.data_ptr(), dstw.data_ptr())
    session.sync()
    w = dstw.cpu().numpy().view(np.uint32)
    rp.release()
    assert session.route_count("hop2_pool") == pool + 1
    assert session.route_count("pool_split") == split + (1 if fmt == "split" else 0)
    return w


@pytest.mark.parametrize("fmt", ["split", "pairs"])
@pytest.mark.parametrize("tiles", [1, 4])
def test_hot_and_cold_targets(session, knobs, bm, fmt, tiles):
    """most lanes need nothing; the cold targets whose sources have no in-relationship stay unset"""
    src, dst, ids = R.hot_cold_graph(tiles)
    w = _end_words(session, knobs, fmt, src, dst, bm["full"], bm["full"], bm["full"])
    np.testing.assert_array_equal(w, R.hop2_words(N, src, dst))
    bit = lambda x: (w[np.asarray(x) >> 5] >> (np.asarray(x) & 31).astype(np.uint32)) & 1  # noqa: E731
    assert bit(ids["hot"]).all() and bit(ids["one"]).all() and not bit(ids["none"]).any()


@pytest.mark.parametrize("fill", R.FILLS)
def test_chunk_fills(session, knobs, bm, fill):
    """a chunk that ends before, at and after one and two 512-pair wave steps, and a full one"""
    src, dst = R.fill_graph(fill)
    w = _end_words(session, knobs, "split", src, dst, bm["full"], bm["full"], bm["full"])
    np.testing.assert_array_equal(w, R.hop2_words(N, src, dst))


@pytest.mark.parametrize("fmt", ["split", "pairs"])
@pytest.mark.parametrize("b,c", [("full", "full"), ("b", "c")])
def test_main_graph(session, knobs, main, bm, fmt, b, c):
    """chunks of slice 1 shared by two blocks, nine pairs in slice 2, an empty slice, loops, endpoints outside
    the domain; the partial masks: preset C bits and the masked flush"""
    m = main["masks"]
    w = _end_words(session, knobs, fmt, main["src"], main["dst"], bm["full"], bm[b], bm[c])
    np.testing.assert_array_equal(w, R.hop2_words(N, main["src"], main["dst"], m[b], m[c]))


def test_loops(session, knobs, bm):
    """X2 against X1: one loop, two loops, a loop plus another in-relationship"""
    src, dst = P.loops_graph()
    w = _end_words(session, knobs, "split", src, dst, bm["full"], bm["full"], bm["full"])
    np.testing.assert_array_equal(w, R.hop2_words(N, src, dst))
    bit = lambda v: (int(w[v >> 5]) >> (v & 31)) & 1  # noqa: E731
    assert not bit(P.ONE_LOOP_ONLY) and bit(P.TWO_LOOPS_ONLY) and bit(P.ONE_LOOP_ONE_IN)
