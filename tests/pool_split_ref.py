"""Shared by test_pool_split_cpu.py and test_gpu_pool_split.py: the graphs of the split-pool tests and numpy
restatements of what the device leaves behind -- hop 1's frontier words (X1, X2) and the digest of the cells.
The CPU test checks the restatements against oracle.cpu; the GPU test then compares the device with them.

The main graph follows test_gpu_pass1_nohist.py: 3 * 2^19 + 1000 ids (three full target slices and a short
fourth), 2^18 + 5 relationships, about 85 % of the targets in slice 1 (a block's tiles bring it more than one
chunk of 8192 pairs: runs cross chunk boundaries and chunks retire full), nine targets in slice 2 (fewer than
one 32-pair line of the split pool: a held tail only, flushed at the end), none in slice 3, some self-loops and
some endpoints outside the domain."""
import numpy as np

S = 1 << 19          # ids per slice
N = 3 * S + 1000
M = (1 << 18) + 5
LINE = 32            # pairs per 128-byte line of the split pool's word arrays
TILE = 8192          # pairs per pass-1 tile and per chunk
STEP = 1024          # targets per wave step of hop 1 over the split pool (16 per lane)


def mix64(x):
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def inside(n, src, dst):
    return (src >= 0) & (src < n) & (dst >= 0) & (dst < n)


def np_digest(n, src, dst, ncells, ns, sbits, tbits):
    """per 2-D cell (target slice major): pair count and wrapping sum of mix64(source << 32 | target)"""
    keep = inside(n, src, dst)
    x, y = src[keep].astype(np.uint64), dst[keep].astype(np.uint64)
    cell = (y >> np.uint64(tbits)).astype(np.int64) * ns + (x >> np.uint64(sbits)).astype(np.int64)
    want_n = np.bincount(cell, minlength=ncells)
    want_s = np.zeros(ncells, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(want_s, cell, mix64((x << np.uint64(32)) | y))
    return want_n, want_s, int(keep.sum())


def frontier(n, src, dst, b_ok=None):
    """hop 1 with a full a_ok (frontier() of scripts/pool_reads_model.py, through b_ok): X1(b) = b has an
    in-relationship that is no self-loop, or at least one self-loop; X2(b) = the same, or at least two."""
    k = inside(n, src, dst)
    src, dst = src[k], dst[k]
    loop = src == dst
    m = np.zeros(n, bool)
    m[dst[~loop]] = True
    selfc = np.bincount(dst[loop], minlength=n)
    b = np.ones(n, bool) if b_ok is None else np.asarray(b_ok).astype(bool)
    return (m | (selfc >= 1)) & b, (m | (selfc >= 2)) & b


def distinct_from_frontier(n, src, dst, b_ok=None, c_ok=None):
    """count(DISTINCT c) of the 2-hop with a full a_ok, from the frontier: the second relationship (s, t) ends
    a path if X1(s), or X2(s) when it is itself a loop (the first must then be another loop at s, or no loop)"""
    x1, x2 = frontier(n, src, dst, b_ok)
    k = inside(n, src, dst)
    src, dst = src[k], dst[k]
    ok = np.where(src == dst, x2[src], x1[src])
    c = np.zeros(n, bool)
    c[dst[ok]] = True
    if c_ok is not None:
        c &= np.asarray(c_ok).astype(bool)
    return int(c.sum())


def words(bits):
    """bool per id -> uint32 words, bit i of word w = id 32 w + i"""
    pad = (-len(bits)) % 32
    b = np.concatenate([np.asarray(bits, bool), np.zeros(pad, bool)])
    return np.packbits(b, bitorder="little").view(np.uint32)


def main_graph():
    rng = np.random.default_rng(47)
    dst = np.where(rng.random(M) < 0.85, S + rng.integers(0, S, M), rng.integers(0, S, M)).astype(np.int64)
    src = rng.integers(0, 2 * S, M).astype(np.int64)  # sources in slices 0 and 1: every middle can have out-rels
    at = rng.choice(M, 9 + 40 + 12, replace=False)
    dst[at[:9]] = 2 * S + rng.integers(0, S, 9)  # slice 2: nine pairs
    src[at[9:49]] = dst[at[9:49]]                # self-loops
    src[at[49:53]] = -3                          # outside the domain
    dst[at[53:57]] = N
    src[at[57:61]] = N + (1 << 33)
    masks = {"full": np.ones(N, np.uint8), "b": (rng.random(N) < 0.7).astype(np.uint8),
             "c": (rng.random(N) < 0.6).astype(np.uint8)}
    return src, dst, masks


# ids of the self-loop cases: the first id, the last of a slice, the first of the next, the last of the domain
LOOP_IDS = (0, S - 1, S, N - 1)
TWO_LOOPS_ONLY = 2 * S + 17      # two loops, no other in-relationship: X1 and X2
ONE_LOOP_ONLY = 2 * S + 18       # one loop, nothing else: X1, not X2
ONE_LOOP_ONE_IN = S + 77         # one loop and one other in-relationship: X1 and X2
SAME_OFFSET = (5, S + 5)         # a non-loop pair whose ends differ only in bit 19: same in-slice offset


def loops_graph():
    """a few hundred background relationships that never point at the loop cases' ids, then the cases"""
    rng = np.random.default_rng(53)
    special = set(LOOP_IDS) | {TWO_LOOPS_ONLY, ONE_LOOP_ONLY, ONE_LOOP_ONE_IN, SAME_OFFSET[1]}
    m = 700
    src = rng.integers(0, N, m).astype(np.int64)
    dst = rng.integers(0, N, m).astype(np.int64)
    bad = np.isin(dst, list(special)) | (src == dst)
    dst[bad] = 1234  # an ordinary id
    src[bad] = 99
    extra = [(v, v) for v in LOOP_IDS]
    extra += [(TWO_LOOPS_ONLY, TWO_LOOPS_ONLY)] * 2 + [(ONE_LOOP_ONLY, ONE_LOOP_ONLY)]
    extra += [(ONE_LOOP_ONE_IN, ONE_LOOP_ONE_IN), (3, ONE_LOOP_ONE_IN)]
    extra += [SAME_OFFSET]
    # out-relationships of the cases, so that X1 / X2 at them decide the count
    extra += [(TWO_LOOPS_ONLY, 4000), (ONE_LOOP_ONLY, 4001), (ONE_LOOP_ONE_IN, 4002), (SAME_OFFSET[1], 4003)]
    extra += [(v, 5000 + i) for i, v in enumerate(LOOP_IDS)]
    e = np.array(extra, np.int64)
    src, dst = np.concatenate([src, e[:, 0]]), np.concatenate([dst, e[:, 1]])
    p = rng.permutation(len(src))
    return src[p], dst[p]


def one_slice_table(rows, extra_per_tile=None):
    """`rows` relationships all into slice 1; with extra_per_tile = (slice, k), every 8192-row tile also carries
    k relationships into that slice (they replace rows of the tile)"""
    rng = np.random.default_rng(59 + rows)
    src = rng.integers(0, N, rows).astype(np.int64)
    dst = (S + rng.integers(0, S, rows)).astype(np.int64)
    if extra_per_tile:
        j, k = extra_per_tile
        for t0 in range(0, rows, TILE):
            if t0 + k <= rows:
                at = t0 + rng.choice(min(TILE, rows - t0), k, replace=False)
                dst[at] = j * S + rng.integers(0, min(S, N - j * S), k)
    return src, dst


def fill_table(fill):
    """one tile (8192 rows): exactly `fill` pairs into slice 0 -- one chunk of that fill -- and the rest into
    slice 1; every target of slice 0 distinct, a loop among them, so a dropped or doubled pair shows in X"""
    rng = np.random.default_rng(61 + fill)
    src = rng.integers(0, N, TILE).astype(np.int64)
    dst = (S + rng.integers(0, S, TILE)).astype(np.int64)
    at = rng.choice(TILE, fill, replace=False)
    dst[at] = rng.choice(S, fill, replace=False)
    src[at[0]] = dst[at[0]]
    return src, dst
