"""The cold 2-hop count(DISTINCT c) with both hops over the pass-1 chunk pool (k_part.hip k_pool_hop1 /
k_pool_hop2, CAPSMI_HOP2=pool) against the cells path (pass 2 + k_hop_2d, CAPSMI_HOP2=cells) and against
binding enumeration (oracle.cpu.two_hop_enumerate).

One graph serves most cases: 3 * 2^19 + 1000 ids (three full target slices and a short fourth) and 2^21
skewed relationships (R-MAT draws folded into the domain), so every slice spans many 8192-pair chunks, some
part-full, and several blocks' shares -- the flush of a shared slice is an atomicOr merge.  Laid over it, on
ids no R-MAT relationship touches:
- middles whose only in-relationship is one self-loop (X1 holds, X2 does not) or two (both hold), each with an
  out-relationship, so the end c = that middle is reached only through the second loop;
- targets whose every in-relationship comes from a source without in-relationships (never an end);
- targets whose first-stored in-relationships come from such sources and a later one from a live source: a
  failed source must leave the target unset for the later one (the dead sources' rows are first in the table);
- a hub target with 70,000 in-relationships (many lanes of one step on one LDS word)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 1 << 19
N = 3 * S + 1000
M = 1 << 21
MODES = ("pool", "cells")


def _build_graph():
    from oracle import cpu
    rng = np.random.default_rng(17)
    src, dst = cpu.rmat_edges(21, 0, M)
    src, dst = src % N, dst % N
    special = np.arange(24) * 65001 + 4321  # spread over slices 0..2
    keep = ~(np.isin(src, special) | np.isin(dst, special))
    src, dst = src[keep], dst[keep]
    live = np.unique(dst)[:64]  # sources that have in-relationships
    loop1, loop2, end1, end2 = special[0:2], special[2:4], special[4:6], special[6:8]
    dead_src, dead_dst, late_dst, hub = special[8:12], special[12:16], special[16:20], special[20]
    head_s = np.concatenate([np.repeat(dead_src, 4), np.repeat(dead_src, 4)])
    head_d = np.concatenate([np.tile(dead_dst, 4), np.tile(late_dst, 4)])
    tail_s = np.concatenate([loop1, loop2, loop2, loop1, loop2, live[:4], rng.integers(0, N, 70_000)])
    tail_d = np.concatenate([loop1, loop2, loop2, end1, end2, late_dst, np.full(70_000, hub)])
    tail_s[-70_000:][np.isin(tail_s[-70_000:], special)] = live[5]
    src = np.concatenate([head_s, src, tail_s]).astype(np.int64)
    dst = np.concatenate([head_d, dst, tail_d]).astype(np.int64)
    masks = {"full": np.ones(N, np.uint8), "a": (rng.random(N) < 0.8).astype(np.uint8),
             "b": (rng.random(N) < 0.7).astype(np.uint8), "c": (rng.random(N) < 0.6).astype(np.uint8)}
    for m in masks.values():
        m[special] = 1
    return src, dst, masks, {"loop1": loop1, "loop2": loop2, "dead_dst": dead_dst, "late_dst": late_dst, "hub": hub}


@pytest.fixture(scope="module")
def G():
    src, dst, masks, ids = _build_graph()
    return {"src": src, "dst": dst, "masks": masks, "ids": ids, "want": {}}


def _want(G, a, b, c):
    """enumeration's count(DISTINCT c) for the filter triple, computed once per triple"""
    from oracle import cpu
    if (a, b, c) not in G["want"]:
        m = G["masks"]
        G["want"][(a, b, c)] = cpu.two_hop_enumerate(N, G["src"], G["dst"], m[a], m[b], m[c])[1]
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
    """the graph's table and the filter bitmaps on the device, shared by the cases"""
    return {"rels": _table(session, G["src"], G["dst"]),
            "bm": {k: _bitmap(session, N, m) for k, m in G["masks"].items()}}


def _both(session, knobs, rels, a, b, c):
    from capsmi import graph
    got = {}
    for mode in MODES:
        knobs(session, CAPSMI_HOP2=mode)
        name = "hop2_" + mode
        before = session.route_count(name)
        got[mode] = graph.two_hop_count_distinct(session, rels, a, b, c)
        if sum(r.size for r in rels) > 0:  # a is the full filter in every caller
            assert session.route_count(name) == before + 1, f"forced {mode} did not run hop 2 over the {mode}"
    return got


def test_graph_has_the_special_shapes(G):
    """the overlay is what the cases below rely on (host only)"""
    src, dst, ids = G["src"], G["dst"], G["ids"]
    indeg = np.bincount(dst, minlength=N)
    assert (np.bincount(dst[src == dst], minlength=N)[ids["loop1"]] == 1).all() and (indeg[ids["loop1"]] == 1).all()
    assert (np.bincount(dst[src == dst], minlength=N)[ids["loop2"]] == 2).all() and (indeg[ids["loop2"]] == 2).all()
    assert indeg[ids["hub"]] >= 70_000
    first = {int(t): int(np.nonzero(dst == t)[0][0]) for t in ids["late_dst"]}
    assert all(indeg[src[i]] == 0 for i in first.values())  # first-stored in-relationship: a dead source
    assert all((indeg[src[dst == t]] > 0).any() for t in ids["late_dst"])
    assert all((indeg[src[dst == t]] == 0).all() for t in ids["dead_dst"])


@pytest.mark.parametrize("b,c", [("full", "full"), ("b", "full"), ("full", "c"), ("b", "c")])
def test_pool_and_cells_equal_enumeration(session, knobs, G, dev, b, c):
    """a_ok full: hop 1 and hop 2 over the pool (b_ok at hop 1's flush; c_ok partial = the preset of k_pool_hop2)
    against the cells path and enumeration"""
    bm = dev["bm"]
    got = _both(session, knobs, [dev["rels"]], bm["full"], bm[b], bm[c])
    want = _want(G, "full", b, c)
    assert got == {"pool": want, "cells": want}


def test_special_targets_as_ends(session, knobs, G, dev):
    """the end bitmap itself: dead-source targets stay 0, late-live targets are set, the one-loop middles are not
    ends, the two-loop middles are"""
    import torch
    from capsmi import graph
    nw = (N + 31) // 32
    bm, ids = dev["bm"], G["ids"]
    marks = {}
    for mode in MODES:
        knobs(session, CAPSMI_HOP2=mode)
        mid = torch.zeros(2 * nw, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(nw, dtype=torch.int32, device="cuda")
        dstw = torch.zeros(nw, dtype=torch.int32, device="cuda")
        rp = graph.RelPartition.build_mark_mid(session, [dev["rels"]], bm["full"], bm["full"], mid.data_ptr(),
                                               scratch.data_ptr())
        rp.mark_dst(bm["full"], bm["full"], mid.data_ptr(), dstw.data_ptr())
        session.sync()
        w = dstw.cpu().numpy().view(np.uint32)
        rp.release()
        marks[mode] = w
        bit = lambda x: (w[np.asarray(x) >> 5] >> (np.asarray(x) & 31)) & 1  # noqa: E731
        assert not bit(ids["dead_dst"]).any()
        assert bit(ids["late_dst"]).all()
        assert not bit(ids["loop1"]).any() and bit(ids["loop2"]).all()
        assert bit(ids["hub"]) == 1
    np.testing.assert_array_equal(marks["pool"], marks["cells"])


def test_partial_a_takes_the_cells_path(session, knobs, G, dev):
    """a_ok partial: hop 1 needs the source test, so the build completes the cells whatever the knob says"""
    from capsmi import graph
    bm = dev["bm"]
    want = _want(G, "a", "b", "c")
    for mode in MODES + ("auto",):
        knobs(session, CAPSMI_HOP2=mode)
        before = session.route_count("hop2_pool")
        assert graph.two_hop_count_distinct(session, [dev["rels"]], bm["a"], bm["b"], bm["c"]) == want
        assert session.route_count("hop2_pool") == before


def test_several_tables_and_empty_ones(session, knobs, G, dev):
    from capsmi import graph
    src, dst, bm = G["src"], G["dst"], dev["bm"]
    cut = len(src) // 3 + 777
    parts = [_table(session, src[:cut], dst[:cut]), _table(session, src[:0], dst[:0]), _table(session, src[cut:], dst[cut:])]
    want = _want(G, "full", "full", "full")
    assert _both(session, knobs, parts, bm["full"], bm["full"], bm["full"]) == {"pool": want, "cells": want}
    assert _both(session, knobs, [parts[1]], bm["full"], bm["full"], bm["full"]) == {"pool": 0, "cells": 0}
    for mode in MODES:
        knobs(session, CAPSMI_HOP2=mode)
        assert graph.two_hop_count_distinct(session, [], bm["full"], bm["full"], bm["full"]) == 0


def test_same_query_twice(session, knobs, G, dev):
    bm = dev["bm"]
    first = _both(session, knobs, [dev["rels"]], bm["full"], bm["b"], bm["c"])
    assert _both(session, knobs, [dev["rels"]], bm["full"], bm["b"], bm["c"]) == first


def test_auto_chooses_by_first_encounters(session, knobs, G, dev):
    """auto: the skewed table (most pairs find their target set) runs on the pool; a permutation table (every
    target in-degree 1, 2^21 relationships: no early exit, one X read per relationship) over 2^27 ids, where
    the frontier bitmap no longer sits in the caches, goes through the cells.  Over a domain of at most 2^26
    ids the pool's hops measured no slower even without any early exit (the choice is by the
    domain), so the same permutation folded into 2^21 ids stays on the pool.  All three are correct."""
    from capsmi import graph
    from oracle import cpu
    knobs(session, CAPSMI_HOP2="auto")
    bm = dev["bm"]
    routes = lambda: (session.route_count("hop2_pool"), session.route_count("hop2_cells"))  # noqa: E731
    pool0, cells0 = routes()
    assert graph.two_hop_count_distinct(session, [dev["rels"]], bm["full"], bm["full"], bm["full"]) == \
        _want(G, "full", "full", "full")
    assert routes() == (pool0 + 1, cells0)
    m = 1 << 21
    rng = np.random.default_rng(23)
    for logn, want_route in ((27, (pool0 + 1, cells0 + 1)), (21, (pool0 + 2, cells0 + 1))):
        n = 1 << logn
        pdst = (np.arange(m, dtype=np.int64) << (logn - 21)) + rng.integers(0, 1 << (logn - 21), m)  # distinct targets
        psrc = pdst[rng.integers(0, m, m)]
        full = graph.NodeBitmap(session, 0, n).add_scan(graph.rmat_nodes(session, logn, graph.NODES_ALL), "id")
        got = graph.two_hop_count_distinct(session, [_table(session, psrc, pdst)], full, full, full)
        assert routes() == want_route
        assert got == cpu.two_hop_enumerate(n, psrc, pdst)[1]


def test_kept_handle_completes_its_cells(session, knobs, G, dev):
    """build_mark_mid + mark_dst over the pool, then mark_mid / mark_dst on the same handle with other filters
    (hop 1 with a partial a_ok needs the cells: built lazily from the kept pool), then the layout digest, which
    equals the one of a handle built with the cells path"""
    import torch
    from capsmi import graph
    nw = (N + 31) // 32
    bm = dev["bm"]
    out = {}
    for mode in MODES:
        knobs(session, CAPSMI_HOP2=mode)
        mid = torch.zeros(2 * nw, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(nw, dtype=torch.int32, device="cuda")
        dstw = torch.zeros(nw, dtype=torch.int32, device="cuda")
        rp = graph.RelPartition.build_mark_mid(session, [dev["rels"]], bm["full"], bm["b"], mid.data_ptr(),
                                               scratch.data_ptr())
        rp.mark_dst(bm["b"], bm["c"], mid.data_ptr(), dstw.data_ptr())
        first = graph.words_popcount(session, dstw.data_ptr(), 0, nw)
        rp.mark_mid(bm["a"], bm["full"], mid.data_ptr(), scratch.data_ptr())
        rp.mark_dst(bm["full"], bm["c"], mid.data_ptr(), dstw.data_ptr())
        second = graph.words_popcount(session, dstw.data_ptr(), 0, nw)
        counts, sums, bad, geo = rp.digest()
        size = rp.size
        rp.release()
        assert bad == 0 and size == len(G["src"]) and counts.sum() == size
        out[mode] = (first, second, counts, sums, geo)
    assert out["pool"][:2] == out["cells"][:2] == (_want(G, "full", "b", "c"), _want(G, "a", "full", "c"))
    np.testing.assert_array_equal(out["pool"][2], out["cells"][2])
    np.testing.assert_array_equal(out["pool"][3], out["cells"][3])
    assert out["pool"][4] == out["cells"][4]


# ---- the distributed routes with the pool forced (the launch pattern of tests/test_gpu_dist_route.py) ---------
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ranks(graph, lo, hi, world, rels_by, backend, out):
    env = dict(os.environ, CAPSMI_DIST_BACKEND=backend, MASTER_ADDR="127.0.0.1", CAPSMI_HOP2="pool")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", f"--master-port={_port()}", os.path.join(ROOT, "tests", "dist_route_worker.py"),
           str(graph), str(lo), str(hi), "owned", "--rels-by", rels_by, "--queries", "c3", "--out", out]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    i = p.stderr.find("Traceback (most recent call last)")
    assert p.returncode == 0, p.stderr[i:i + 5000] if i >= 0 else p.stderr[-4000:]
    res = []
    for r in range(world):
        with open(f"{out}.rank{r}.json") as f:
            res.append(json.load(f))
    return res


@pytest.mark.parametrize("rels_by", ["target", "source"])
def test_dist_world1_rccl_pool_forced(tmp_path, rels_by):
    """BY_TARGET / BY_SOURCE shards at world size 1 over RCCL, the pool hops forced, against the closed form
    (tests/golden/rmat_full.json, C3 at s = 20)"""
    with open(os.path.join(ROOT, "tests", "golden", "rmat_full.json")) as f:
        c3 = json.load(f)["cases"]["c3_s20"]
    o = _ranks("rmat:20", 0, 1 << 20, 1, rels_by, "nccl", str(tmp_path / "r20"))[0]
    assert o["backend"] == "nccl" and o["world"] == 1
    assert o["count_distinct_c"] == c3["count_distinct_c"], o
    assert o["count_star"] == c3["count_star"], o


@pytest.mark.parametrize("rels_by", ["target", "source"])
def test_dist_two_gloo_ranks_pool_forced(tmp_path, rels_by):
    """two ranks sharing the GPU over gloo, hub edge list (hubs at ids 0..999), the pool hops forced"""
    from oracle import cpu
    rng = np.random.default_rng(7)
    n, m, hubs = 1 << 16, 400_000, 1000
    src = np.where(rng.random(m) < 0.5, rng.integers(0, hubs, m), rng.integers(0, n, m)).astype(np.int64)
    dst = np.where(rng.random(m) < 0.5, rng.integers(0, hubs, m), rng.integers(0, n, m)).astype(np.int64)
    src[:500] = dst[:500]  # self-loops
    edges = tmp_path / "hubs.txt"
    np.savetxt(edges, np.stack([src, dst], axis=1), fmt="%d", delimiter=" ")
    _, distinct = cpu.two_hop_closed_form(n, src, dst)
    _, distinct_a = cpu.two_hop_closed_form(n, dst, src)
    for o in _ranks(edges, 0, n, 2, rels_by, "gloo", str(edges)):
        assert o["count_distinct_c"] == distinct, o
        assert o["count_distinct_a"] == distinct_a, o
