"""The numpy restatement of hop 2's end bitmap (pool_hop2_ref.py) against oracle.cpu.two_hop_enumerate on every
graph of test_gpu_pool_hop2.py, and the shapes those graphs must have.  No GPU."""
import numpy as np
import pytest

import pool_hop2_ref as R
import pool_split_ref as P
from oracle import cpu


def _enumerate(src, dst, b=None, c=None):
    k = P.inside(R.N, src, dst)
    return cpu.two_hop_enumerate(R.N, src[k], dst[k], None, b, c)[1]


def _bit(w, ids):
    ids = np.asarray(ids)
    return (w[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1


@pytest.mark.parametrize("tiles", [1, 4])
def test_hot_cold_graph(tiles):
    src, dst, ids = R.hot_cold_graph(tiles)
    assert len(src) == tiles * R.TILE and ((dst >> 19) == 1).all() and not (src == dst).any()
    hot_pairs = np.isin(dst, ids["hot"])
    assert 0.88 < hot_pairs.mean() < 0.92 and np.isin(src[hot_pairs], ids["hot"]).all()
    indeg = np.bincount(dst, minlength=R.N)
    cold = np.concatenate([ids["one"], ids["none"]])
    assert len(cold) >= 200 and indeg[cold].min() >= 2 and indeg[cold].max() <= 6
    x1, _ = P.frontier(R.N, src, dst)
    live = x1[src]  # the pair's source has an in-relationship
    assert (np.bincount(dst[live], minlength=R.N)[ids["one"]] == 1).all()
    assert (np.bincount(dst[live], minlength=R.N)[ids["none"]] == 0).all()
    w = R.hop2_words(R.N, src, dst)
    assert _bit(w, ids["hot"]).all() and _bit(w, ids["one"]).all() and not _bit(w, ids["none"]).any()
    # the two kinds of cold pairs are interleaved in the table (and so in the pool): every 512-pair stretch holds
    # pairs into targets that must stay unset, and most hold a cold pair that must set its target
    none_pairs = np.isin(dst, ids["none"]).reshape(-1, R.STEP).sum(axis=1)
    one_pairs = (np.isin(dst, ids["one"]) & live).reshape(-1, R.STEP).sum(axis=1)
    assert none_pairs.min() >= 1 and (one_pairs >= 1).mean() > 0.8
    assert _popcount(w) == len(ids["hot"]) + len(ids["one"]) == _enumerate(src, dst)


def _popcount(w):
    return int(np.unpackbits(w.view(np.uint8)).sum())


@pytest.mark.parametrize("fill", R.FILLS)
def test_fill_graph(fill):
    src, dst = R.fill_graph(fill)
    in0 = (dst >> 19) == 0
    assert len(src) == R.TILE and in0.sum() == fill and len(np.unique(dst[in0])) == fill
    assert ((dst[~in0] >> 19) == 1).all() and (src[in0] == dst[in0]).sum() == 1
    x1, _ = P.frontier(R.N, src, dst)
    if fill >= 64:
        assert 0.3 < x1[src[in0]].mean() < 0.7
    bits = R.hop2_bits(R.N, src, dst)
    assert _popcount(P.words(bits)) == int(bits.sum()) == _enumerate(src, dst)
    if fill >= 64:  # both answers occur among the slice's targets
        assert 0 < bits[:R.S].sum() < fill


@pytest.mark.parametrize("b,c", [("full", "full"), ("b", "c")])
def test_main_graph(b, c):
    src, dst, masks = P.main_graph()
    w = R.hop2_words(R.N, src, dst, masks[b], masks[c])
    assert len(w) == (R.N + 31) // 32
    assert _popcount(w) == _enumerate(src, dst, masks[b], masks[c])
    assert _popcount(w) == P.distinct_from_frontier(R.N, src, dst, masks[b], masks[c])


def test_loops_graph():
    src, dst = P.loops_graph()
    bits = R.hop2_bits(R.N, src, dst)
    assert int(bits.sum()) == _enumerate(src, dst)
    # a single loop at v and nothing else into v: the loop pair asks X2(v), which is unset
    for v in P.LOOP_IDS + (P.ONE_LOOP_ONLY,):
        assert not bits[v]
    assert bits[P.TWO_LOOPS_ONLY] and bits[P.ONE_LOOP_ONE_IN]
    # the out-relationships of the loop cases end paths through X1
    assert bits[4000] and bits[4001] and bits[4002] and bits[4003] and bits[5000:5004].all()
