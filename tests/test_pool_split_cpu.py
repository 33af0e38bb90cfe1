"""The numpy restatements of pool_split_ref.py (hop 1's frontier, the cells' digest grouping) against oracle.cpu
on the graphs of test_gpu_pool_split.py, and the shapes those graphs must have.  No GPU."""
import numpy as np
import pytest

import pool_split_ref as R
from oracle import cpu


@pytest.fixture(scope="module")
def G():
    src, dst, masks = R.main_graph()
    return src, dst, masks


def _enumerate(src, dst, b=None, c=None):
    k = R.inside(R.N, src, dst)
    return cpu.two_hop_enumerate(R.N, src[k], dst[k], None, b, c)[1]


def test_main_graph_has_the_shapes(G):
    src, dst, _ = G
    k = R.inside(R.N, src, dst)
    per_slice = np.bincount(dst[k] >> 19, minlength=4)
    assert R.M % R.LINE != 0 and int(k.sum()) % R.LINE != 0
    assert per_slice[1] > 0.8 * R.M and 0 < per_slice[2] < R.LINE and per_slice[3] == 0
    assert (src[k] == dst[k]).sum() >= 30 and (~k).sum() >= 8
    # a pass-1 block walks two 8192-row tiles of this table (16 blocks): together they bring slice 1 more than a chunk
    tiles = (dst[:32 * R.TILE] >> 19 == 1).reshape(32, R.TILE).sum(axis=1)
    assert ((tiles[:16] + tiles[16:]) > R.TILE).all()


@pytest.mark.parametrize("b,c", [("full", "full"), ("b", "c"), ("b", "full")])
def test_frontier_gives_the_oracles_count(G, b, c):
    src, dst, masks = G
    assert R.distinct_from_frontier(R.N, src, dst, masks[b], masks[c]) == _enumerate(src, dst, masks[b], masks[c])


def test_loops_graph_frontier():
    src, dst = R.loops_graph()
    x1, x2 = R.frontier(R.N, src, dst)
    for v in R.LOOP_IDS:  # one loop each and no other in-relationship
        assert x1[v] and not x2[v]
    assert x1[R.TWO_LOOPS_ONLY] and x2[R.TWO_LOOPS_ONLY]
    assert x1[R.ONE_LOOP_ONLY] and not x2[R.ONE_LOOP_ONLY]
    assert x1[R.ONE_LOOP_ONE_IN] and x2[R.ONE_LOOP_ONE_IN]
    a, b = R.SAME_OFFSET
    assert a != b and (a & (R.S - 1)) == (b & (R.S - 1)) and x1[b] and x2[b]
    assert R.distinct_from_frontier(R.N, src, dst) == _enumerate(src, dst)
    # the count depends on the X1 / X2 distinction: taking X1 for the loops' test as well changes it
    loop = src == dst
    c = np.zeros(R.N, bool)
    c[dst[x1[src]]] = True
    assert int(c.sum()) != _enumerate(src, dst) and loop.sum() >= 8


def test_digest_grouping_counts(G):
    """per cell, the restated pair count against the oracle's expand with slice masks as node filters"""
    src, dst, _ = G
    ns, bits = 4, 19
    want_n, _, kept = R.np_digest(R.N, src, dst, 16, ns, bits, bits)
    k = R.inside(R.N, src, dst)
    assert kept == int(k.sum()) == int(want_n.sum())
    ids = np.arange(R.N)
    for j in range(4):
        for i in range(4):
            a_ok, b_ok = (ids >> bits == i).astype(np.uint8), (ids >> bits == j).astype(np.uint8)
            assert cpu.expand_filter(src[k], dst[k], a_ok, b_ok)[0] == want_n[j * ns + i], (j, i)


def test_words_bit_order():
    bits = np.zeros(70, bool)
    bits[[0, 31, 32, 69]] = True
    np.testing.assert_array_equal(R.words(bits), np.array([0x80000001, 1, 1 << 5], np.uint32))


@pytest.mark.parametrize("rows", [0, 1, 31, 32, 33, 8191, 8192, 8193])
def test_one_slice_tables(rows):
    src, dst = R.one_slice_table(rows)
    assert len(src) == rows and ((dst >> 19) == 1).all()


def test_line_tables():
    src, dst = R.one_slice_table(4 * R.TILE, extra_per_tile=(2, R.LINE))  # exactly a line per tile
    assert (np.bincount((dst >> 19)[:R.TILE], minlength=4)[2] == R.LINE
            and ((dst >> 19) == 2).reshape(4, R.TILE).sum(axis=1).tolist() == [R.LINE] * 4)
    src, dst = R.one_slice_table(4 * R.TILE, extra_per_tile=(0, 5))  # 20 in all: never a line, a held tail
    assert ((dst >> 19) == 0).sum() == 20 < R.LINE


@pytest.mark.parametrize("fill", [1, R.STEP - 1, R.STEP, R.STEP + 1, R.TILE])
def test_fill_tables(fill):
    src, dst = R.fill_table(fill)
    in0 = (dst >> 19) == 0
    assert len(src) == R.TILE and in0.sum() == fill and len(np.unique(dst[in0])) == fill
    assert (src[in0] == dst[in0]).sum() >= 1
    assert R.distinct_from_frontier(R.N, src, dst) == _enumerate(src, dst)
