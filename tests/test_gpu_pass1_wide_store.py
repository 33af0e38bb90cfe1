"""The split pool's store loop of pass 1 (k_part.hip k_scatter_l, SPLIT) taking four staged pairs per lane: two
16-byte LDS reads, one decode of the slice's word, one 16-byte store of the four target words and one of the
four source words, or two 16-byte LDS writes into the slice's held line.  p1l_plan pads every slice's staged
length (held + run) to a multiple of 4 for it, and the stage region has 4 more entries per slice.

What can go wrong is a group that straddles something: the end of a slice's sequence (padding stored as pairs, or
real pairs dropped), the chunk the run leaves for the one it opens, the cut between stored lines and the held
tail, or the end of the stage region.  The cases put the end of a sequence at every residue mod 4, on and off a
32-pair line, at a chunk's end exactly, and make the padded total exceed the unpadded region.

Every case builds the cold 2-hop over the split pool (pool_split == 1 asserted) with a full node bitmap and
compares exactly with the numpy restatements of pool_split_ref.py and pool_hop2_ref.py, as
test_gpu_pass1_pipeline.py does: hop 1's words X1 / X2 (every target word and its self-loop flag), the end bitmap
(every pair), the kept count (the chunks' fills) and the digest of the cells (per cell the pair count and a
wrapping sum of a mix of source and target, which sees a target stored beside a neighbour's source).  Every case
runs over registered tables (pass 1 over the 32-bit copies, `pass1_narrow` asserted) and over unregistered ones
(the int64 instantiation); the restatement is made once per case and shared.

A table of at most 2 * 8192 rows is one block that walks tile 0, then tile 1; rows outside the window fill a tile
up without being staged.  The window starts at 2^20, and the outside rows stay within 2^31 ids of it, so that every
table is eligible for the copies.  The reused cases are test_gpu_narrow_endpoints.py's forms of the pipeline test's
(its `outside` rows, unlike the pipeline module's own, keep the table eligible); their restatements are shared
with that module."""
import functools

import numpy as np
import pytest

import pool_hop2_ref as H
import pool_split_ref as P

pytestmark = pytest.mark.gpu

S, TILE = P.S, P.TILE
LO = 1 << 20
N_BIG = 1 << 26      # 128 target slices
ROUTES = ("pass1_narrow", "pool_split", "hop2_pool")


def _tiles(n, plan, seed):
    """one tile per entry (rows, {target slice: count}) of `plan`: `count` rows into each slice at random places of
    the tile, the tile's other rows outside the window (below it through the source, above it through the target).
    Half the sources are targets of the table, so hop 2 has paths to find; every 23rd row inside is a self-loop."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for rows, per in plan:
        d = np.full(rows, -1, np.int64)
        at = rng.permutation(rows)
        k = 0
        for j, c in per.items():
            d[at[k:k + c]] = j * S + rng.integers(0, min(S, n - j * S), c)
            k += c
        assert k <= rows
        dst.append(d)
    dst = np.concatenate(dst)
    ins = dst >= 0
    m = len(dst)
    pool = dst[ins]
    src = np.where(rng.random(m) < 0.5, pool[rng.integers(0, len(pool), m)], rng.integers(0, n, m)).astype(np.int64)
    loops = np.flatnonzero(ins)[::23]
    src[loops] = dst[loops]
    out = np.flatnonzero(~ins)
    low = out[0::2]
    src[low] = -1 - (low % 3)                       # below the window, the target inside it
    dst[low] = rng.integers(0, n, len(low))
    dst[out[1::2]] = n + (out[1::2] % 7)            # at and above the window's end
    return src, dst


def _plan(name):
    if name.startswith("tiny"):           # a: one partial group, everything held, written by the tail path
        r = int(name[4:])
        return P.N, [(r, {1: r})]
    if name == "residues_a":              # b: held 1, 2, 3 -> held + run 4, 5, 33; the large slice crosses chunks
        return P.N, [(TILE, {0: 1, 2: 2, 3: 3, 1: 8100}), (TILE, {0: 3, 2: 3, 3: 30, 1: 8000})]
    if name == "residues_b":              # b: held + run 31, 6, 7
        return P.N, [(TILE, {0: 1, 2: 2, 3: 3, 1: 8100}), (TILE, {0: 30, 2: 4, 3: 4, 1: 8000})]
    if name == "exact_chunk":             # c: fill kCh, nothing held, cut = kCh; then room 0 with an open chunk
        return P.N, [(TILE, {1: TILE}), (TILE, {1: TILE})]
    if name == "exact_32_4":              # c: lengths 32 (all stored) and 4 (one whole group held), then 32 + 32, 4 + 28
        return P.N, [(TILE, {0: 32, 2: 4, 1: TILE - 36}), (TILE, {0: 32, 2: 28, 1: TILE - 60})]
    if name == "padding":                 # d: 31 held + 62 or 66, all = 1 mod 4: 12,544 padded entries staged
        return N_BIG, [(TILE, {j: 31 for j in range(128)}), (TILE, {j: 62 + 4 * (j & 1) for j in range(128)})]
    raise KeyError(name)


REUSED = {"odd_off_boundary": "skip1a", "two_tables": "two_tables", "outside": "outside", "big": "big"}


def _want(n, s, d):
    x1, x2 = P.frontier(n, s, d)
    want = {"x1": P.words(x1), "x2": P.words(x2), "end": H.hop2_words(n, s, d), "kept": int(P.inside(n, s, d).sum())}
    for v in (want["x1"], want["x2"], want["end"]):
        v.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _case(name):
    """a case's tables as (source, target, skip) in window-relative ids, its domain and what the device must leave
    behind: made once, read-only, shared by the registered and the unregistered run"""
    if name in REUSED:
        import test_gpu_narrow_endpoints as NE
        g = NE._case(REUSED[name])
        assert NE.LO == LO and all(g["eligible"])
        return {"n": NE.N, "tabs": [t[:3] for t in g["tabs"]], "src": g["src"], "dst": g["dst"], "want": g["want"]}
    n, plan = _plan(name)
    src, dst = _tiles(n, plan, 19 + sum(map(ord, name)))
    for v in (src, dst):
        v.setflags(write=False)
    return {"n": n, "tabs": [(src, dst, 0)], "src": src, "dst": dst, "want": _want(n, src, dst)}


@pytest.fixture(scope="module")
def bitmaps(session):
    """the full node bitmap of a domain, its words written directly (2^26 ids need no node table)"""
    import torch
    from capsmi import graph
    made = {}

    def get(n):
        if n not in made:
            nw = (n + 31) // 32
            w = np.full(nw, 0xFFFFFFFF, np.uint32)
            if n % 32:
                w[-1] = (1 << (n % 32)) - 1
            t = torch.from_numpy(w.view(np.int32)).cuda()
            bm = graph.NodeBitmap(session, LO, LO + n)
            bm.copy_words(0, nw, t.data_ptr(), True)
            session.sync()
            made[n] = bm.assume(n)
        return made[n]

    return get


@pytest.fixture(scope="module")
def tables(session):
    made = {}

    def get(name, registered):
        from capsmi import ColumnData, I64
        if (name, registered) not in made:
            out = []
            for src, dst, skip in _case(name)["tabs"]:
                t = session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)),
                                   ColumnData("source", I64, src + LO), ColumnData("target", I64, dst + LO)])
                t = t.skip(skip) if skip else t
                out.append(t.as_rel_table("id", "source", "target") if registered else t)
            made[(name, registered)] = out
        return made[(name, registered)]

    return get


def _run(session, bitmaps, tables, name, registered):
    import torch
    from capsmi import graph
    g = _case(name)
    n, want = g["n"], g["want"]
    nw = (n + 31) // 32
    bm = bitmaps(n)
    with session.configured(CAPSMI_NARROW="auto"):
        tabs = tables(name, registered)
    with session.configured(CAPSMI_NARROW="auto", CAPSMI_HOP2="pool", CAPSMI_POOL="split"):
        mid = torch.zeros(2 * nw, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(nw, dtype=torch.int32, device="cuda")
        end = torch.zeros(nw, dtype=torch.int32, device="cuda")
        before = {r: session.route_count(r) for r in ROUTES}
        rp = graph.RelPartition.build_mark_mid(session, tabs, bm, bm, mid.data_ptr(), scratch.data_ptr())
        rp.mark_dst(bm, bm, mid.data_ptr(), end.data_ptr())
        session.sync()
        ran = {r: session.route_count(r) - before[r] for r in ROUTES}
        kept = rp.size
        x = mid.cpu().numpy().view(np.uint32)
        w = end.cpu().numpy().view(np.uint32)
        counts, sums, bad, (ns, sbits, tbits) = rp.digest()
        rp.release()
    # the split pool, every table launched over its copies (registered) or over its int64 columns
    assert ran == {"pass1_narrow": len(tabs) if registered else 0, "pool_split": 1, "hop2_pool": 1}, ran
    if "digest" not in want:
        want["digest"] = P.np_digest(n, g["src"], g["dst"], len(counts), ns, sbits, tbits)
    want_n, want_s, want_kept = want["digest"]
    assert bad == 0 and kept == want_kept == want["kept"], (bad, kept, want_kept)
    np.testing.assert_array_equal(x[:nw], want["x1"])
    np.testing.assert_array_equal(x[nw:], want["x2"])
    np.testing.assert_array_equal(w, want["end"])
    np.testing.assert_array_equal(counts, want_n)
    np.testing.assert_array_equal(sums, want_s)


REG = pytest.mark.parametrize("registered", [True, False], ids=["u32", "i64"])


@REG
@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5])
def test_tiny_tables_one_partial_group_all_held(session, bitmaps, tables, rows, registered):
    _run(session, bitmaps, tables, f"tiny{rows}", registered)


@REG
@pytest.mark.parametrize("name", ["residues_a", "residues_b"])
def test_every_residue_over_two_tiles(session, bitmaps, tables, name, registered):
    """tile 0 leaves 1, 2 and 3 pairs held in three slices and 8100 in the fourth (held 4, written prefix 8096,
    room 96); tile 1 brings the small ones to 4, 5, 33 (a) or 31, 6, 7 (b) staged items and the large one 8000
    more, across the chunk boundary"""
    _run(session, bitmaps, tables, name, registered)


@REG
@pytest.mark.parametrize("name", ["exact_chunk", "exact_32_4"])
def test_lengths_that_end_on_a_chunk_a_line_a_group(session, bitmaps, tables, name, registered):
    _run(session, bitmaps, tables, name, registered)


@REG
def test_padded_total_beyond_the_unpadded_stage(session, bitmaps, tables, registered):
    """2^26 ids, 128 target slices, every slice staging 31 + 62 or 31 + 66 items in tile 1: 12,544 padded entries
    where the region held 12,288 before it had the groups' padding"""
    g = _case("padding")
    per = np.bincount((g["dst"][TILE:] >> 19), minlength=128)
    assert g["n"] == N_BIG and set(per[:128]) == {62, 66} and sum((31 + c + 3) // 4 * 4 for c in per[:128]) == 12544
    _run(session, bitmaps, tables, "padding", registered)


@REG
@pytest.mark.parametrize("name", ["odd_off_boundary", "two_tables", "outside"])
def test_scalar_loads_two_launches_rows_outside(session, bitmaps, tables, name, registered):
    _run(session, bitmaps, tables, name, registered)


@REG
def test_a_block_per_cu_with_eight_or_nine_tiles(session, bitmaps, tables, registered):
    _run(session, bitmaps, tables, "big", registered)
