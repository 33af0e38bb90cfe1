"""The 32-bit endpoint copies of a registered relationship table (Column::narrow, CAPSMI_NARROW) and pass 1 of
the chunk partition reading them (k_part.hip k_scatter_l / k_scatter_c over uint32_t, part_common.h load_tile).

Every 2-hop case registers its tables and builds the cold 2-hop with a full a_ok under CAPSMI_NARROW=auto and
under off, and compares both with the numpy restatements of pool_split_ref.py and pool_hop2_ref.py and with each
other, word for word: hop 1's words (X1, X2), the end bitmap, the kept count and the digest of the cells.  The
route counters say what ran: narrow_built one per eligible table registered under auto, pass1_narrow one per
launch over such a table, both zero under off.

The window is [LO, LO + N) with LO = 2^20, and a table's copies are relative to the table's own minimum, which
differs from LO in every case (above it; below it where rows lie under the window): a pass 1 that took the words
as relative to the window would misplace every pair.  A 16-byte load of the copies is four relationships, so the
rows of a last, short tile are read by the scalar path in another item order than the int64 columns': rows 1 ...
3 * 8192 put the end of the table at every place in a load and in a tile.

The issue asked for a pool of one eligible table and one with a nullable endpoint.  No such pool exists: a
relationship table with a nullable endpoint is refused at registration (EntityTable.verify) and again by the
partition's entry points (rel_col), before any kernel.  The ineligible tables here are the two kinds a pool can
hold: a registered table whose endpoints span more than 2^32 ids, and a table that was never registered.

The storage cases build a plain partition (pass 1 with the cell counts) from tables at the edges of the
eligibility rule and compare its digest; they read the copies through pass 1, the only reader there is."""
import functools

import numpy as np
import pytest

import pool_hop2_ref as H
import pool_split_ref as P

pytestmark = pytest.mark.gpu

S, N, TILE = P.S, P.N, P.TILE
NW = (N + 31) // 32
LO = 1 << 20
EDGE_ROWS = (8191, 8192, 8193, 2 * 8192 + 5, 3 * 8192)
SMALL_ROWS = (1, 3, 4, 5)
BIG = (1 << 24) + 1000
MODES = ("split", "pairs", "cells")
ROUTES = ("narrow_built", "pass1_narrow", "pool_split", "hop2_pool", "hop2_cells")


def _graph(rows, seed, outside=False):
    """`rows` relationships over a few thousand ids of slices 0-2 of the window, relative to it: most targets in
    slice 1 (runs cross chunk boundaries), some in slice 0, nine in slice 2, half the sources targets too, some
    self-loops.  With `outside`, rows of the first and of the last tile lie below the window, at its end and
    above it, within 2^31 ids of it (the table stays eligible; its lowest id is 5, so its copies' base is neither
    0 nor the window's lo)."""
    rng = np.random.default_rng(seed)
    per = 3000 if rows <= (1 << 20) else 60000
    ids = np.concatenate([j * S + 100 + rng.choice(S - 100, per, replace=False) for j in range(3)])
    pick = lambda j, k: ids[j * per + rng.integers(0, per, k)]
    dst = np.where(rng.random(rows) < 0.85, pick(1, rows), pick(0, rows))
    src = np.where(rng.random(rows) < 0.5, ids[rng.integers(0, len(ids), rows)], 100 + rng.integers(0, N - 100, rows))
    if rows >= 64:
        at = rng.choice(rows, 9 + rows // 200, replace=False)
        dst[at[:9]] = pick(2, 9)
        src[at[9:]] = dst[at[9:]]
    if outside:
        last = (rows - 1) // TILE * TILE
        src[[0, 5, TILE - 1]] = [-3, N, N + (1 << 31)]
        dst[[last, rows - 2, rows - 1]] = [-1, N, N + (1 << 30)]
        dst[7], src[last + 1], dst[last + 2] = N + 5, 5 - LO, N + 9
    return src.astype(np.int64), dst.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    """a case's tables as (source, target, skip, register before the skip) in window-relative ids, the narrow
    copies expected under auto, and what the device must leave behind: made once, read-only"""
    cut = lambda src, dst, at: list(zip(np.split(src, at), np.split(dst, at)))
    eligible = None
    if name.startswith("rows"):
        rows = int(name[4:])
        src, dst = _graph(rows, 311 + rows)
        tabs = [(src, dst, 0, False)]
    elif name.startswith("skip"):  # skip{k}{a|b}: the copies start k words off a 16-byte boundary
        k, before = int(name[4]), name[5] == "b"
        src, dst = _graph(2 * TILE + 6 + k, 331 + k)
        tabs = [(src, dst, k, before)]
    elif name == "two_tables":     # own minima differ from each other and from LO; the first ends inside a tile
        src, dst = _graph(3 * TILE, 337)
        (s0, d0), (s1, d1) = cut(src, dst, [TILE + 7])
        s0[3], s1[3] = 11, 57
        tabs = [(s0, d0, 0, False), (s1, d1, 0, False)]
    elif name == "outside":
        src, dst = _graph(2 * TILE + 5, 347, outside=True)
        tabs = [(src, dst, 0, False)]
    elif name == "mixed":          # eligible, too wide (> 2^32 ids), never registered: three launches
        src, dst = _graph(3 * TILE + 77, 349)
        (s0, d0), (s1, d1), (s2, d2) = cut(src, dst, [TILE + 9, 2 * TILE + 1])
        s1[5] = N + (1 << 33)
        tabs = [(s0, d0, 0, False), (s1, d1, 0, False), (s2, d2, 0, None)]
        eligible = [True, False, False]
    elif name == "big":
        src, dst = _graph(BIG, 353, outside=True)
        tabs = [(src, dst, 0, False)]
    else:
        raise KeyError(name)
    s = np.concatenate([t[0][t[2]:] for t in tabs])
    d = np.concatenate([t[1][t[2]:] for t in tabs])
    x1, x2 = P.frontier(N, s, d)
    want = {"x1": P.words(x1), "x2": P.words(x2), "end": H.hop2_words(N, s, d), "kept": int(P.inside(N, s, d).sum())}
    for v in (s, d, want["x1"], want["x2"], want["end"]):
        v.setflags(write=False)
    return {"tabs": tabs, "src": s, "dst": d, "want": want, "eligible": eligible or [True] * len(tabs)}


def _raw(session, src, dst, lo=LO):
    from capsmi import ColumnData, I64
    return session.table([ColumnData("id", I64, np.arange(len(src), dtype=np.int64)),
                          ColumnData("source", I64, src + lo), ColumnData("target", I64, dst + lo)])


def _register(t):
    return t.as_rel_table("id", "source", "target")


@pytest.fixture(scope="module")
def full_bm(session):
    from capsmi import ColumnData, I64, graph
    ids = session.table([ColumnData("id", I64, np.arange(LO, LO + N, dtype=np.int64))])
    return graph.NodeBitmap(session, LO, LO + N).add_scan(ids)


@pytest.fixture(scope="module")
def tables(session):
    """a case's registered device tables per knob setting, made once; with them the narrow_built count of
    the registration"""
    made = {}

    def get(name, narrow):
        if (name, narrow) not in made:
            out = []
            before = session.route_count("narrow_built")
            with session.configured(CAPSMI_NARROW=narrow):
                for src, dst, skip, reg_before in _case(name)["tabs"]:
                    t = _raw(session, src, dst)
                    if reg_before is None:
                        pass
                    elif reg_before:
                        t = _register(t)
                        t = t.skip(skip) if skip else t
                    else:
                        t = _register(t.skip(skip) if skip else t)
                    out.append(t)
            made[(name, narrow)] = (out, session.route_count("narrow_built") - before)
        return made[(name, narrow)]

    return get


def _run(session, full_bm, tables, name, mode):
    import torch
    from capsmi import graph
    g = _case(name)
    want = g["want"]
    got = {}
    for narrow in ("auto", "off"):
        tabs, built = tables(name, narrow)
        n_elig = sum(g["eligible"]) if narrow == "auto" else 0
        assert built == n_elig, (narrow, built)
        kn = {"CAPSMI_HOP2": "cells"} if mode == "cells" else {"CAPSMI_HOP2": "pool", "CAPSMI_POOL": mode}
        with session.configured(CAPSMI_NARROW=narrow, **kn):
            mid = torch.zeros(2 * NW, dtype=torch.int32, device="cuda")
            scratch = torch.zeros(NW, dtype=torch.int32, device="cuda")
            end = torch.zeros(NW, dtype=torch.int32, device="cuda")
            before = {r: session.route_count(r) for r in ROUTES}
            rp = graph.RelPartition.build_mark_mid(session, tabs, full_bm, full_bm, mid.data_ptr(), scratch.data_ptr())
            rp.mark_dst(full_bm, full_bm, mid.data_ptr(), end.data_ptr())
            session.sync()
            ran = {r: session.route_count(r) - before[r] for r in ROUTES}
            kept = rp.size
            x = mid.cpu().numpy().view(np.uint32)
            w = end.cpu().numpy().view(np.uint32)
            counts, sums, bad, (ns, sbits, tbits) = rp.digest()
            rp.release()
        # every table is launched, the eligible ones over their copies; which pool and which hop 2
        assert ran == {"narrow_built": 0, "pass1_narrow": n_elig, "pool_split": int(mode == "split"),
                       "hop2_pool": int(mode != "cells"), "hop2_cells": int(mode == "cells")}, (narrow, ran)
        if "digest" not in want:
            want["digest"] = P.np_digest(N, g["src"], g["dst"], len(counts), ns, sbits, tbits)
        want_n, want_s, want_kept = want["digest"]
        assert bad == 0 and kept == want_kept == want["kept"], (narrow, bad, kept)
        np.testing.assert_array_equal(x[:NW], want["x1"], err_msg=narrow)
        np.testing.assert_array_equal(x[NW:], want["x2"], err_msg=narrow)
        np.testing.assert_array_equal(w, want["end"], err_msg=narrow)
        np.testing.assert_array_equal(counts, want_n, err_msg=narrow)
        np.testing.assert_array_equal(sums, want_s, err_msg=narrow)
        got[narrow] = (x, w, kept, counts, sums)
    for a, b in zip(got["auto"], got["off"]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("rows", SMALL_ROWS)
def test_one_load_short_and_exact(session, full_bm, tables, rows):
    _run(session, full_bm, tables, f"rows{rows}", "split")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", EDGE_ROWS)
def test_tile_edges_and_the_scalar_tail(session, full_bm, tables, rows, mode):
    _run(session, full_bm, tables, f"rows{rows}", mode)


@pytest.mark.parametrize("name", ["skip1a", "skip2a", "skip3a", "skip1b", "skip2b", "skip3b"])
def test_copies_at_every_alignment_of_a_load(session, full_bm, tables, name):
    """a table behind skip(k), registered after the skip (a: the copies are made under the offset) and before
    it (b: the offset is applied to copies made without)"""
    _run(session, full_bm, tables, name, "split")


@pytest.mark.parametrize("name", ["two_tables", "outside"])
def test_bases_apart_and_rows_outside_the_window(session, full_bm, tables, name):
    _run(session, full_bm, tables, name, "split")


def test_eligible_and_ineligible_tables_in_one_pool(session, full_bm, tables):
    """narrow_built counts the eligible table alone, pass1_narrow its launch alone, and all three launches run
    (the restatement holds every table's pairs)"""
    _run(session, full_bm, tables, "mixed", "split")


def test_a_block_per_cu_with_several_tiles(session, full_bm, tables):
    _run(session, full_bm, tables, "big", "split")


# ---- storage: the eligibility rule's edges, read back through a plain partition ------------------------------
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
# name: (the window's lo, the table's lowest id, ids forced into the table, eligible)
STORAGE = {
    "from_2p40": ((1 << 40) + 12345, (1 << 40) + 12345, [], True),
    "negative_lo": (-5000, -5000 - 77, [], True),
    "span_2p32": ((1 << 31), 3, [3, (1 << 32) + 2], True),
    "span_2p32_plus_1": ((1 << 31), 3, [3, (1 << 32) + 3], False),
    "min_to_max": (0, 0, [I64_MIN, I64_MAX], False),
    "top_of_int64": (I64_MAX - N, I64_MAX - (1 << 32) + 1, [I64_MAX - (1 << 32) + 1, I64_MAX], True),
    "top_of_int64_one_more": (I64_MAX - N, I64_MAX - (1 << 32), [I64_MAX - (1 << 32), I64_MAX], False),
}


@pytest.mark.parametrize("name", list(STORAGE))
def test_storage_at_the_rule_edges(session, name):
    from capsmi import ColumnData, I64, graph
    wlo, tlo, forced, eligible = STORAGE[name]
    rows = 2 * TILE + 13
    src, dst = _graph(rows, 401)
    src, dst = src + wlo, dst + wlo   # absolute ids, inside the window
    src[1] = tlo if not forced else src[1]
    for k, v in enumerate(forced):
        (src if k % 2 == 0 else dst)[10 + k] = v
    rel = lambda v: (v.astype(object) - wlo)
    inside = np.array([0 <= a < N and 0 <= b < N for a, b in zip(rel(src), rel(dst))])
    rs = np.where(inside, (src - np.int64(wlo)), -1).astype(np.int64)  # rows outside: any id outside
    rd = np.where(inside, (dst - np.int64(wlo)), -1).astype(np.int64)
    got = {}
    for narrow in ("auto", "off"):
        with session.configured(CAPSMI_NARROW=narrow):
            b0, p0 = session.route_count("narrow_built"), session.route_count("pass1_narrow")
            t = _register(session.table([ColumnData("id", I64, np.arange(rows, dtype=np.int64)),
                                         ColumnData("source", I64, src), ColumnData("target", I64, dst)]))
            rp = graph.RelPartition(session, [t], wlo, wlo + N)
            counts, sums, bad, (ns, sbits, tbits) = rp.digest()
            kept = rp.size
            rp.release()
            use = int(eligible and narrow == "auto")
            assert (session.route_count("narrow_built") - b0, session.route_count("pass1_narrow") - p0) == (use, use)
        want_n, want_s, want_kept = P.np_digest(N, rs, rd, len(counts), ns, sbits, tbits)
        assert bad == 0 and kept == want_kept == int(inside.sum())
        np.testing.assert_array_equal(counts, want_n, err_msg=narrow)
        np.testing.assert_array_equal(sums, want_s, err_msg=narrow)
        got[narrow] = (counts, sums)
    np.testing.assert_array_equal(got["auto"][0], got["off"][0])
    np.testing.assert_array_equal(got["auto"][1], got["off"][1])


def test_no_rows_no_copy(session):
    from capsmi import ColumnData, I64, graph
    e = np.zeros(0, np.int64)
    b0, p0 = session.route_count("narrow_built"), session.route_count("pass1_narrow")
    t = _register(session.table([ColumnData("id", I64, e), ColumnData("source", I64, e), ColumnData("target", I64, e)]))
    rp = graph.RelPartition(session, [t], LO, LO + N)
    assert rp.size == 0
    rp.release()
    assert (session.route_count("narrow_built") - b0, session.route_count("pass1_narrow") - p0) == (0, 0)
