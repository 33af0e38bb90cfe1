"""The tile loop of the whole-line pass 1 (k_part.hip k_scatter_l) at the edges a software-pipelined loop can
break: a tile's loads are issued one iteration ahead, into the registers the tile before it has just left, so a
block's first tile is loaded before the loop, its last one has no successor, and wave 0 settles a tile's chunk
bookkeeping one tile late (after the loop for the last).  Whatever order the loop's loads, waits and stores are
given, these are the cases in which a tile is dropped, ranked twice or ranked from another tile's registers.

Every case builds the cold 2-hop with a full a_ok and compares with the numpy restatements of pool_split_ref.py
and pool_hop2_ref.py:
- hop 1's words (X1 = M | S1, X2 = M | S2), which see every target word and its self-loop flag;
- the end bitmap of the 2-hop, word for word, which sees every (source, target) pair;
- the kept count, which is the sum of the chunks' fills, before anything has read the cells;
- the digest of the cells (per target slice and source slice the pair count and a wrapping sum of a mix of the
  pair, so per target slice the multiset of its pairs), built from the pool afterwards.
in three modes: the split pool, the pool of pairs (CAPSMI_POOL=pairs) and pass 1 with the cell counts
(CAPSMI_HOP2=cells, the HIST instantiation).  The domain has more than 2^20 ids and four target slices, where
the whole-line kernel runs; the route counts say which pool and which hop 2 ran.

Row counts: tables of at most 2^24 rows get a pass-1 block per two tiles, so 1 ... 3 * 8192 rows give blocks of
one and two tiles with the last tile full, one row long, five rows long, or missing; a table just above 2^24 rows
gets a block per CU with 8 or 9 tiles each and a last tile of 1000 rows."""
import functools

import numpy as np
import pytest

import pool_hop2_ref as H
import pool_split_ref as P

pytestmark = pytest.mark.gpu

S, N, TILE = P.S, P.N, P.TILE
NW = (N + 31) // 32
MODES = ("split", "pairs", "cells")
ROWS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5, 3 * TILE)
BIG = (1 << 24) + 1000


def _graph(rows, seed, outside=False):
    """`rows` relationships among a few thousand ids of slices 0-2: about 85 % of the targets in slice 1 (two tiles
    bring it more than a chunk, so runs cross chunk boundaries and chunks retire full), the rest in slice 0 but
    for nine in slice 2 (a held tail only); half the sources are targets too; some self-loops.  With `outside`,
    rows of the first and of the last tile have an endpoint below, at the end of, or far above the domain."""
    rng = np.random.default_rng(seed)
    per = 3000 if rows <= (1 << 20) else 60000
    ids = np.concatenate([j * S + rng.choice(S, per, replace=False) for j in range(3)])
    pick = lambda j, k: ids[j * per + rng.integers(0, per, k)]
    dst = np.where(rng.random(rows) < 0.85, pick(1, rows), pick(0, rows))
    src = np.where(rng.random(rows) < 0.5, ids[rng.integers(0, len(ids), rows)], rng.integers(0, N, rows))
    if rows >= 64:
        at = rng.choice(rows, 9 + rows // 200, replace=False)
        dst[at[:9]] = pick(2, 9)
        src[at[9:]] = dst[at[9:]]
    if outside:
        last = (rows - 1) // TILE * TILE
        first_rows, last_rows = np.array([0, 5, TILE - 1]), np.array([last, rows - 2, rows - 1])
        src[first_rows], dst[last_rows] = [-3, N, N + (1 << 33)], [-1, N, N + (1 << 40)]
        dst[7], src[last + 1], dst[last + 2] = N + 5, -(1 << 35), N + 9  # four rows in the first tile, five in the last
    return src.astype(np.int64), dst.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    """a case's tables (one graph cut into them) and what the device must leave behind: made once, read-only,
    shared by the three modes"""
    skip = 0
    if name.startswith("rows"):
        rows = int(name[4:])
        src, dst = _graph(rows, 211 + rows)
        cuts = []
    elif name == "odd_off_boundary":      # an odd count behind skip(1): columns 8 bytes off a 16-byte boundary
        src, dst = _graph(2 * TILE + 6, 223)
        cuts, skip = [], 1
    elif name == "two_tables":            # two launches into one pool, the first ends inside a tile
        src, dst = _graph(3 * TILE, 227)
        cuts = [TILE + 7]
    elif name == "outside":
        src, dst = _graph(2 * TILE + 5, 229, outside=True)
        cuts = []
    elif name == "big":
        src, dst = _graph(BIG, 233, outside=True)
        cuts = []
    else:
        raise KeyError(name)
    s, d = src[skip:], dst[skip:]
    x1, x2 = P.frontier(N, s, d)
    want = {"x1": P.words(x1), "x2": P.words(x2), "end": H.hop2_words(N, s, d), "kept": int(P.inside(N, s, d).sum())}
    for v in (src, dst, want["x1"], want["x2"], want["end"]):
        v.setflags(write=False)
    return {"src": src, "dst": dst, "cuts": cuts, "skip": skip, "want": want}


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)),
                          ColumnData("source", I64, src), ColumnData("target", I64, dst)])


@pytest.fixture(scope="module")
def full_bm(session):
    from capsmi import ColumnData, I64, graph
    return graph.NodeBitmap(session, 0, N).add_scan(session.table([ColumnData("id", I64, np.arange(N, dtype=np.int64))]))


@pytest.fixture(scope="module")
def tables(session):
    """a case's device tables, uploaded once"""
    made = {}

    def get(name):
        if name not in made:
            g = _case(name)
            parts = zip(np.split(g["src"], g["cuts"]), np.split(g["dst"], g["cuts"]))
            made[name] = [_table(session, s, d) for s, d in parts]
            if g["skip"]:
                made[name] = [t.skip(g["skip"]) for t in made[name]]
        return made[name]

    return get


ROUTES = ("pool_split", "hop2_pool", "hop2_cells", "chunk_hist")


def _run(session, knobs, full_bm, tables, name, mode):
    import torch
    from capsmi import graph
    g = _case(name)
    if mode == "cells":
        knobs(session, CAPSMI_HOP2="cells")
    else:
        knobs(session, CAPSMI_HOP2="pool", CAPSMI_POOL=mode)
    mid = torch.zeros(2 * NW, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(NW, dtype=torch.int32, device="cuda")
    end = torch.zeros(NW, dtype=torch.int32, device="cuda")
    before = {r: session.route_count(r) for r in ROUTES}
    rp = graph.RelPartition.build_mark_mid(session, tables(name), full_bm, full_bm, mid.data_ptr(), scratch.data_ptr())
    rp.mark_dst(full_bm, full_bm, mid.data_ptr(), end.data_ptr())
    session.sync()
    ran = {r: session.route_count(r) - before[r] for r in ROUTES}
    kept = rp.size
    x = mid.cpu().numpy().view(np.uint32)
    w = end.cpu().numpy().view(np.uint32)
    # which pass 1 and which hop 2: the split pool, the pairs, or the cell counts made in pass 1 itself
    assert ran == {"pool_split": int(mode == "split"), "hop2_pool": int(mode != "cells"),
                   "hop2_cells": int(mode == "cells"), "chunk_hist": 0}, ran
    want = g["want"]
    assert kept == want["kept"]
    np.testing.assert_array_equal(x[:NW], want["x1"])
    np.testing.assert_array_equal(x[NW:], want["x2"])
    np.testing.assert_array_equal(w, want["end"])
    return rp, g


def _check_cells(rp, g):
    counts, sums, bad, (ns, sbits, tbits) = rp.digest()
    if "digest" not in g["want"]:
        g["want"]["digest"] = P.np_digest(N, g["src"][g["skip"]:], g["dst"][g["skip"]:], len(counts), ns, sbits, tbits)
    want_n, want_s, kept = g["want"]["digest"]
    assert bad == 0 and rp.size == kept == g["want"]["kept"]
    np.testing.assert_array_equal(counts, want_n)
    np.testing.assert_array_equal(sums, want_s)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", ROWS)
def test_blocks_of_one_and_two_tiles(session, knobs, full_bm, tables, rows, mode):
    rp, g = _run(session, knobs, full_bm, tables, f"rows{rows}", mode)
    _check_cells(rp, g)
    rp.release()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["odd_off_boundary", "two_tables", "outside"])
def test_scalar_loads_two_launches_rows_outside(session, knobs, full_bm, tables, name, mode):
    rp, g = _run(session, knobs, full_bm, tables, name, mode)
    _check_cells(rp, g)
    rp.release()


@pytest.mark.parametrize("mode", MODES)
def test_a_block_per_cu_with_eight_or_nine_tiles(session, knobs, full_bm, tables, mode):
    """2^24 + 1000 rows: 2049 tiles over one block per CU, the last tile 1000 rows long, rows outside the domain in
    the first tile and in the last"""
    rp, g = _run(session, knobs, full_bm, tables, "big", mode)
    _check_cells(rp, g)  # with so many pairs per id the bitmaps alone would not miss a tile
    rp.release()
