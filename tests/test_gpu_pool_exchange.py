"""The exchange of hop 2 over the split pool (k_part.hip k_pool_hop2<true, XW>, CAPSMI_HOP2_EXCHANGE): the blocks
that share a target slice OR the global C into their LDS slice and publish their own bits while they walk.  The
end bitmap is exact whatever the timing, so every case compares all of it word for word with the numpy
restatement of pool_hop2_ref.py, with the exchange on and off, and asserts the route counts.

Shapes.  The pool hops take a block per 16 * 8192 pairs (pool_grid) and pass 1 gives two tiles to each of its
blocks, so a table of T tiles whose targets lie in one slice has about T chunks there, shared by T // 16
blocks.  A wave exchanges when it enters a chunk after its first, and a block's 16 waves take its first 16
chunks, so a block needs 17 or more: 47 tiles give 2 blocks of 23 or 24 chunks, 63 tiles 3 blocks of 21.  The
17th chunk a block enters brings window 0 and the 80th window 63.  The cases that need every window of a slice
give their rows as 256 tables of 1600: pass 1 leaves a chunk of 1600 pairs per table, 256 part-full chunks,
shared by 3 blocks of 85 or 86.

Where a pair lands in its chunk is not deterministic, and which block resolves a target first is not either;
the graphs are built so that the bitmap shows a wrong word wherever they land."""
import functools

import numpy as np
import pytest

import pool_hop2_ref as R
import pool_split_ref as P

pytestmark = pytest.mark.gpu

S, N, TILE = P.S, P.N, P.TILE
NW = (N + 31) // 32
WIN = 256            # words per exchange window (one 16-byte load per lane)
T2, T3 = 47, 63      # tiles: 2 and 3 hop blocks
PARTS, PART_ROWS = 256, 1600   # or 256 tables of 1600 rows: 3 hop blocks, 85 or 86 chunks each


def _pure(rng, k, lo_slice=0):
    """k sources that are nobody's target: ids of slice `lo_slice` (the graphs put no target there)"""
    return lo_slice * S + rng.integers(0, S, k)


def _one_pair_graph():
    """T2 tiles into slice 1.  Targets `a` have exactly one in-pair from a source with an in-relationship (another
    target), all of them in the first four tiles, that is in the first block's share; their other in-pairs, and all
    in-pairs of targets `b`, come from sources that are nobody's target, in every block's share."""
    rng = np.random.default_rng(151)
    rows = T2 * TILE
    ids = S + rng.choice(S, 40000, replace=False)
    a, b = ids[:20000], ids[20000:]
    dst = ids[rng.integers(0, len(ids), rows)]
    src = _pure(rng, rows, 2)
    at = rng.permutation(4 * TILE)[:len(a)]
    dst[at] = a
    src[at] = ids[rng.integers(0, len(ids), len(a))]
    same = src[at] == dst[at]
    src[at[same]] = b[0]  # no loops: b[0] is a target too, and never in a
    return src.astype(np.int64), dst.astype(np.int64), {"a": a, "b": b}


def _mixed_graph(seed, rows, slice_, span=S, loops=False):
    """`rows` pairs into `span` ids of one slice; half the sources are targets of the table, the others
    nobody's target (slice 0, or slice 2 when the targets are in slice 0).  With loops: targets with one and two
    self-loops among them, some with another in-relationship and some with none."""
    rng = np.random.default_rng(seed)
    ids = slice_ * S + rng.choice(span, min(span, 60000), replace=False)
    dst = ids[rng.integers(0, len(ids), rows)]
    pure = _pure(rng, rows, 2 if slice_ == 0 else 0)
    src = np.where(rng.random(rows) < 0.5, ids[rng.integers(0, len(ids), rows)], pure)
    src[src == dst] = pure[src == dst]
    info = {}
    if loops:
        # ids that no other row targets: their only in-relationships are the ones written here
        lone = slice_ * S + np.setdiff1d(np.arange(span), ids - slice_ * S)[:6000]
        one, two, one_in, none_in = lone[:1500], lone[1500:3000], lone[3000:4500], lone[4500:]
        at = rng.permutation(rows)[:1500 + 3000 + 3000 + 1500 + 6000]
        k = 0

        def put(s, d):
            nonlocal k
            src[at[k:k + len(d)]], dst[at[k:k + len(d)]] = s, d
            k += len(d)
        put(one, one)                                          # one loop only: X1, not X2
        put(np.concatenate([two, two]), np.concatenate([two, two]))  # two loops: X1 and X2
        put(one_in, one_in)                                    # one loop and one other in-relationship
        put(ids[rng.integers(0, len(ids), 1500)], one_in)
        put(_pure(rng, 1500, 2 if slice_ == 0 else 0), none_in)  # no loop: reached from a pure source only
        put(lone[rng.integers(0, len(lone), 6000)], ids[rng.integers(0, len(ids), 6000)])  # the cases' out-relationships
        info = {"one": one, "two": two, "one_in": one_in, "none_in": none_in}
    return src.astype(np.int64), dst.astype(np.int64), info


def _window_graph():
    """256 x 1600 pairs into slice 1; the only targets that can be set are the ids of four words: the first and the
    last of the slice, and the first and the last of window 5.  Every other target has sources that are nobody's."""
    rng = np.random.default_rng(157)
    rows = PARTS * PART_ROWS
    words = np.array([0, 5 * WIN, 5 * WIN + WIN - 1, (S >> 5) - 1])
    hot = S + (words[:, None] * 32 + np.arange(32)[None, :]).ravel()
    cold = S + np.setdiff1d(rng.choice(S, 50000, replace=False), hot - S)
    dst = cold[rng.integers(0, len(cold), rows)]
    src = _pure(rng, rows, 2)
    at = rng.permutation(rows)[:40 * len(hot)]              # the hot ids' pairs, in every block's share
    dst[at] = np.tile(hot, 40)
    src[at] = np.roll(np.tile(hot, 40), 1)                   # from another hot id: no loops
    return src.astype(np.int64), dst.astype(np.int64), {"hot": hot, "words": (S >> 5) + words}


def _span_graph():
    """T3 tiles, 3 blocks: slice 0's targets only in the first eight tiles (four chunks), slice 1's only in the
    first two (one chunk), the rest in slice 2: the first block's share spans three slices and visits the first
    two alone, and all three blocks share slice 2."""
    rng = np.random.default_rng(163)
    rows = T3 * TILE
    ids = np.concatenate([j * S + rng.choice(S, 20000, replace=False) for j in range(3)])
    dst = ids[40000 + rng.integers(0, 20000, rows)]
    k0 = rng.permutation(8 * TILE)[:6000]
    dst[k0] = ids[rng.integers(0, 20000, len(k0))]
    k1 = np.setdiff1d(rng.permutation(2 * TILE)[:3000], k0)
    dst[k1] = ids[20000 + rng.integers(0, 20000, len(k1))]
    pure = 3 * S + rng.integers(0, N - 3 * S, rows)          # the short last slice: nobody's target
    src = np.where(rng.random(rows) < 0.5, ids[rng.integers(0, len(ids), rows)], pure)
    src[src == dst] = pure[src == dst]
    return src.astype(np.int64), dst.astype(np.int64), {}


@functools.lru_cache(maxsize=None)
def _case(name):
    """graph, masks and the expected words of a case: made once, shared by the exchange's two settings"""
    rng = np.random.default_rng(167)
    full = np.ones(N, np.uint8)
    b = c = full
    if name == "one_pair":
        src, dst, info = _one_pair_graph()
    elif name == "partial_c":
        src, dst, info = _mixed_graph(171, T2 * TILE, 1)
        c = (rng.random(N) < 0.6).astype(np.uint8)
    elif name == "partial_b_loops":
        src, dst, info = _mixed_graph(173, T2 * TILE, 1, loops=True)
        b = (rng.random(N) < 0.7).astype(np.uint8)
    elif name == "windows":
        src, dst, info = _window_graph()
    elif name == "last_slice":
        src, dst, info = _mixed_graph(179, PARTS * PART_ROWS, 3, span=N - 3 * S)
    elif name == "last_slice_partial_c":
        src, dst, info = _mixed_graph(181, PARTS * PART_ROWS, 3, span=N - 3 * S)
        c = (rng.random(N) < 0.6).astype(np.uint8)
    elif name == "span":
        src, dst, info = _span_graph()
        c = (rng.random(N) < 0.6).astype(np.uint8)
    else:
        raise KeyError(name)
    want = R.hop2_words(N, src, dst, None if b is full else b, None if c is full else c)
    want.setflags(write=False)
    parts = PARTS if name in ("windows", "last_slice", "last_slice_partial_c") else 1
    return {"src": src, "dst": dst, "b": b, "c": c, "info": info, "want": want, "parts": parts}


def _table(session, src, dst):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)),
                          ColumnData("source", I64, src), ColumnData("target", I64, dst)])


@functools.lru_cache(maxsize=None)
def _mask_ids(key):
    name, which = key
    return np.nonzero(_case(name)[which])[0].astype(np.int64)


def _bitmap(session, ids):
    from capsmi import ColumnData, I64, graph
    return graph.NodeBitmap(session, 0, N).add_scan(session.table([ColumnData("id", I64, ids)]))


@pytest.fixture(scope="module")
def full_bm(session):
    return _bitmap(session, np.arange(N, dtype=np.int64))


def _end_words(session, knobs, full_bm, name, exchange):
    """the cold build with a full a_ok and both hops over the split pool: hop 2's end bitmap as words"""
    import torch
    from capsmi import graph
    g = _case(name)
    knobs(session, CAPSMI_HOP2="pool", CAPSMI_POOL="split", CAPSMI_HOP2_EXCHANGE=exchange)
    b = full_bm if g["b"].all() else _bitmap(session, _mask_ids((name, "b")))
    c = full_bm if g["c"].all() else _bitmap(session, _mask_ids((name, "c")))
    mid = torch.zeros(2 * NW, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(NW, dtype=torch.int32, device="cuda")
    dstw = torch.zeros(NW, dtype=torch.int32, device="cuda")
    before = {r: session.route_count(r) for r in ("hop2_pool", "pool_split", "hop2_exchange")}
    tables = [_table(session, s_, d_) for s_, d_ in zip(np.split(g["src"], g["parts"]), np.split(g["dst"], g["parts"]))]
    rp = graph.RelPartition.build_mark_mid(session, tables, full_bm, b, mid.data_ptr(), scratch.data_ptr())
    rp.mark_dst(b, c, mid.data_ptr(), dstw.data_ptr())
    session.sync()
    w = dstw.cpu().numpy().view(np.uint32)
    rp.release()
    assert session.route_count("hop2_pool") == before["hop2_pool"] + 1
    assert session.route_count("pool_split") == before["pool_split"] + 1
    assert session.route_count("hop2_exchange") == before["hop2_exchange"] + (1 if exchange == "on" else 0)
    return w, g


def _bit(w, ids):
    ids = np.asarray(ids)
    return (w[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1


EXCHANGE = pytest.mark.parametrize("exchange", ["on", "off"])


@EXCHANGE
def test_one_qualifying_pair_in_one_share(session, knobs, full_bm, exchange):
    """a target reached through exactly one qualifying pair, all of them in one block's share, is set; one whose
    in-neighbours have no in-relationship stays clear in every block that meets it"""
    w, g = _end_words(session, knobs, full_bm, "one_pair", exchange)
    np.testing.assert_array_equal(w, g["want"])
    assert _bit(w, g["info"]["a"]).all() and not _bit(w, g["info"]["b"]).any()


@EXCHANGE
def test_partial_c_ok_publishes_no_excluded_bit(session, knobs, full_bm, exchange):
    """excluded targets have qualifying in-neighbours and share words with included ones: the preset bits of the
    LDS slice, and the bits pulled from other blocks, leave through c_ok only"""
    w, g = _end_words(session, knobs, full_bm, "partial_c", exchange)
    assert not (w & ~P.words(g["c"].astype(bool))).any()
    np.testing.assert_array_equal(w, g["want"])


@EXCHANGE
def test_partial_b_ok_and_loops(session, knobs, full_bm, exchange):
    """a partial b_ok, and in the exchanged slice targets with one loop only (clear), two loops (set iff in b_ok),
    one loop and another in-relationship (set if in b_ok: X2 through the loop; the other pair may set it too) and
    no loop and no qualifying in-neighbour (clear)"""
    w, g = _end_words(session, knobs, full_bm, "partial_b_loops", exchange)
    np.testing.assert_array_equal(w, g["want"])
    i, b = g["info"], g["b"].astype(bool)
    assert not _bit(w, i["one"]).any() and not _bit(w, i["none_in"]).any()
    np.testing.assert_array_equal(_bit(w, i["two"]).astype(bool), b[i["two"]])
    assert _bit(w, i["one_in"][b[i["one_in"]]]).all()


@EXCHANGE
def test_window_boundaries(session, knobs, full_bm, exchange):
    """the only set bits are in the first and the last word of the slice and of an exchange window; every block
    takes every window of the slice"""
    w, g = _end_words(session, knobs, full_bm, "windows", exchange)
    np.testing.assert_array_equal(w, g["want"])
    assert (w[g["info"]["words"]] == 0xFFFFFFFF).all() and np.count_nonzero(w) == 4


@EXCHANGE
@pytest.mark.parametrize("name", ["last_slice", "last_slice_partial_c"])
def test_short_last_slice(session, knobs, full_bm, name, exchange):
    """the last slice of a domain that is no multiple of 2^19 ids: the bitmap ends inside the first window, which
    every block takes twice"""
    w, g = _end_words(session, knobs, full_bm, name, exchange)
    np.testing.assert_array_equal(w, g["want"])
    assert w[3 * (S >> 5):].any() and not w[:3 * (S >> 5)].any()


@EXCHANGE
def test_share_over_three_slices(session, knobs, full_bm, exchange):
    """two slices visited by one block alone, whose share goes on into a third that three blocks walk: the window
    rotation starts again at every visit; a partial c_ok on top"""
    w, g = _end_words(session, knobs, full_bm, "span", exchange)
    np.testing.assert_array_equal(w, g["want"])
    assert all(w[j * (S >> 5):(j + 1) * (S >> 5)].any() for j in range(3))
