"""Shared by test_pool_hop2_cpu.py and test_gpu_pool_hop2.py: hop 2's whole end bitmap restated in numpy, and
the graphs of the pipelined pool hop 2's tests (k_part.hip k_pool_hop2<true> over part::walk_chunks_st_pipe).
The CPU test pins the restatement's popcount to oracle.cpu.two_hop_enumerate; the GPU test then compares the
device's words with it one by one.

Where a pair lands inside its chunk is not deterministic (pass 1 ranks with LDS atomics), so the graphs are
built so that the bitmap shows a wrong word wherever it lands: sources with and without an in-relationship
are mixed at random, and the targets that must stay unset sit among ones that must be set.  All graphs use
the domain of pool_split_ref.py."""
import numpy as np

import pool_split_ref as P

S, N, TILE = P.S, P.N, P.TILE
STEP = 512           # pairs per wave step of hop 2 (8 per lane)
FILLS = (1, STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP + 1, TILE)
HOT = 16


def hop2_bits(n, src, dst, b_ok=None, c_ok=None):
    """C of the 2-hop with a full a_ok, a bool per id: distinct_from_frontier of pool_split_ref.py without the
    final sum.  The second relationship (s, t) ends a path if X1(s), or X2(s) when it is itself a loop."""
    x1, x2 = P.frontier(n, src, dst, b_ok)
    k = P.inside(n, src, dst)
    src, dst = src[k], dst[k]
    ok = np.where(src == dst, x2[src], x1[src])
    c = np.zeros(n, bool)
    c[dst[ok]] = True
    if c_ok is not None:
        c &= np.asarray(c_ok).astype(bool)
    return c


def hop2_words(n, src, dst, b_ok=None, c_ok=None):
    return P.words(hop2_bits(n, src, dst, b_ok, c_ok))


def hot_cold_graph(tiles):
    """`tiles` * 8192 pairs, all into slice 1.  About 90 % go to 16 hot targets from other hot targets (sources
    with an in-relationship: after its first pair a hot target is set, so most lanes of a step need nothing and
    most source loads are skipped).  The rest go to cold targets with 2-6 in-pairs each: the `one` half have
    exactly one in-pair from a hot target and the others from sources that are nobody's target; the `none` half
    have only such sources and must stay unset.  Returns src, dst and the three target sets."""
    rng = np.random.default_rng(71 + tiles)
    rows = tiles * TILE
    cold_n = rows // 40                                  # 4 in-pairs on average: about 10 % of the pairs
    ids = S + rng.choice(S, HOT + cold_n, replace=False)  # distinct targets in slice 1: hot, then cold
    hot, cold = ids[:HOT], ids[HOT:]
    deg = rng.integers(2, 7, cold_n)
    one, none = cold[0::2], cold[1::2]
    src, dst = [], []
    dead = lambda k: np.where(rng.random(k) < 0.5, rng.integers(0, S, k), 2 * S + rng.integers(0, S, k))  # noqa: E731
    for i, (t, d) in enumerate(zip(cold, deg)):
        s = dead(d)
        if i % 2 == 0:
            s[rng.integers(0, d)] = hot[rng.integers(0, HOT)]
        src.append(s)
        dst.append(np.full(d, t))
    nhot = rows - int(deg.sum())
    ht = rng.integers(0, HOT, nhot)
    hs = (ht + rng.integers(1, HOT, nhot)) % HOT  # another hot target: no loops
    src.append(hot[hs])
    dst.append(hot[ht])
    src, dst = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    p = rng.permutation(rows)
    return src[p], dst[p], {"hot": hot, "one": one, "none": none}


def fill_graph(fill):
    """one tile: exactly `fill` pairs into slice 0 -- one chunk of that fill, its targets distinct, a loop among
    them -- and the rest into slice 1.  About half the sources are targets of the table, the others (ids of
    slice 2) are nobody's target."""
    rng = np.random.default_rng(73 + fill)
    dst = (S + rng.integers(0, S, TILE)).astype(np.int64)
    at = rng.choice(TILE, fill, replace=False)
    dst[at] = rng.choice(S, fill, replace=False)
    src = np.where(rng.random(TILE) < 0.5, dst[rng.integers(0, TILE, TILE)], 2 * S + rng.integers(0, S, TILE))
    src = src.astype(np.int64)
    src[src == dst] = 2 * S + 7
    src[at[0]] = dst[at[0]]
    return src, dst
