"""Hash ownership of a distributed graph (include/capsmi.h capsmi_graph_distribute) and the exchanges of
the distributed two-hop routes (csrc/plan_dist.hip dist_two_hop_distinct / dist_two_hop_count), restated
with numpy and rehearsed on CPU with gloo ranks (world size 2 and 4).

Ownership: h(x) = ((x - lo) * 0x9E3779B97F4A7C15) mod 2^k, rank r owns h in [r*32*S, (r+1)*32*S),
S = ceil(2^k / 32 / world).  The graph is an edge list whose hubs sit at ids 0..999 -- contiguous
owner ranges of the raw ids would load the first rank with most of the relationships."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

MUL = 0x9E3779B97F4A7C15


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def scramble(lo, hi, world):
    k = 5
    while (1 << k) < hi - lo:
        k += 1
    slice_words = -(-(1 << k) // 32 // world)
    return k, slice_words


def h_of(x, lo, k):
    """h(x) as numpy uint64 arithmetic (wrapping multiply, then the low k bits)"""
    v = (np.asarray(x, dtype=np.int64) - lo).astype(np.uint64)
    with np.errstate(over="ignore"):
        return ((v * np.uint64(MUL)) & np.uint64((1 << k) - 1)).astype(np.int64)


def owner_of(x, lo, hi, world):
    k, S = scramble(lo, hi, world)
    return h_of(x, lo, k) // (32 * S)


def hub_edges(seed=7, n=1 << 16, m=400_000, hubs=1000):
    rng = np.random.default_rng(seed)
    src = np.where(rng.random(m) < 0.5, rng.integers(0, hubs, m), rng.integers(0, n, m))
    dst = np.where(rng.random(m) < 0.5, rng.integers(0, hubs, m), rng.integers(0, n, m))
    src[:500] = dst[:500]
    return n, src.astype(np.int64), dst.astype(np.int64)


@pytest.mark.parametrize("lo,hi,world", [(0, 1 << 16, 2), (0, 1 << 26, 8), (1 << 40, (1 << 40) + 1000, 3),
                                         (-500, 70_000, 6)])
def test_owner_restatement_matches_library(lo, hi, world):
    from capsmi import _lib
    lib = _lib.load()
    rng = np.random.default_rng(world)
    ids = np.concatenate([rng.integers(lo, hi, 200), [lo, hi - 1]])
    want_owner = owner_of(ids, lo, hi, world)
    k, _ = scramble(lo, hi, world)
    want_dense = h_of(ids, lo, k)
    for x, o, d in zip(ids.tolist(), want_owner.tolist(), want_dense.tolist()):
        r, dd = ctypes.c_int32(), ctypes.c_int64()
        assert lib.capsmi_id_owner(lo, hi, world, x, ctypes.byref(r), ctypes.byref(dd)) == 0
        assert (r.value, dd.value) == (o, d)
    assert 0 <= want_owner.min() and want_owner.max() < world


def test_scramble_is_a_bijection():
    k = 12
    assert len(np.unique(h_of(np.arange(1 << k), 0, k))) == 1 << k


@pytest.mark.parametrize("world", [2, 4, 8])
def test_hash_ownership_balances_hubs(world):
    n, src, dst = hub_edges()
    per = np.bincount(owner_of(dst, 0, n, world), minlength=world)
    assert np.abs(per / per.mean() - 1).max() < 0.05, per
    contiguous = np.bincount(dst * world // n, minlength=world)  # raw-id ranges: the hubs on rank 0
    assert contiguous.max() / contiguous.mean() > 1.4


def _rank_main(rank, world, port, result_q):
    """One rank of the distributed C3 route, in numpy over the scrambled ids: the shard (relationships
    whose target it owns), the node-scan bitmap slices all-gathered, hop 1 for owned middle ids, the
    frontier slices all-gathered, hop 2 for owned end ids, owned popcount all-reduced; and the count(*)
    route's owned in-degrees all-gathered and the parts all-reduced."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "cypher-for-apache-spark_amd"), os.path.dirname(os.path.abspath(__file__))]
    import torch
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, src, dst = hub_edges(m=60_000)
    k, S = scramble(0, n, world)
    D = world * 32 * S
    own_lo, own_hi = rank * 32 * S, (rank + 1) * 32 * S
    hs, ht = h_of(src, 0, k), h_of(dst, 0, k)
    mine = (ht >= own_lo) & (ht < own_hi)
    s, t = hs[mine], ht[mine]
    # node scan (every endpoint is a :V node), owned rows only, then the bitmap all-gather
    present = np.zeros(D, np.uint8)
    ends = np.unique(np.concatenate([hs, ht]))
    present[ends[(ends >= own_lo) & (ends < own_hi)]] = 1
    parts = [torch.zeros(32 * S, dtype=torch.uint8) for _ in range(world)]
    dist.all_gather(parts, torch.from_numpy(present[own_lo:own_hi].copy()))
    ok = torch.cat(parts).numpy()
    # hop 1 (owned middles), the frontier exchange, hop 2 (owned ends)
    M = np.zeros(D, np.uint8)
    keep = (ok[s] == 1) & (ok[t] == 1)
    M[t[keep & (s != t)]] = 1
    loops = np.bincount(t[keep & (s == t)], minlength=D)
    X1, X2 = (M | (loops >= 1)).astype(np.uint8), (M | (loops >= 2)).astype(np.uint8)
    for X in (X1, X2):
        parts = [torch.zeros(32 * S, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(X[own_lo:own_hi].copy()))
        X[:] = torch.cat(parts).numpy()
    hit = np.where(s != t, X1[s], X2[s]).astype(bool) & (ok[t] == 1)
    C = np.zeros(D, np.uint8)
    C[t[hit]] = 1
    distinct = torch.tensor([int(C[own_lo:own_hi].sum())], dtype=torch.int64)
    dist.all_reduce(distinct)
    # count(*): owned in-degrees, all-gathered, summed over this rank's relationships
    own_in = np.bincount(t[ok[s] == 1] - own_lo, minlength=32 * S).astype(np.int64) * ok[own_lo:own_hi]
    parts = [torch.zeros(32 * S, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(parts, torch.from_numpy(own_in))
    in_all = torch.cat(parts).numpy()
    c_ok = ok[t] == 1
    rows = int(in_all[s[c_ok]].sum()) - int(((s == t) & (ok[s] == 1)).sum())
    rows_t = torch.tensor([rows], dtype=torch.int64)
    dist.all_reduce(rows_t)
    result_q.put((rank, int(distinct.item()), int(rows_t.item()), int(mine.sum())))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_distributed_c3_route_gloo(world):
    from oracle import cpu
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    n, src, dst = hub_edges(m=60_000)
    rows, distinct = cpu.two_hop_closed_form(n, src, dst)
    for _, d, r, _ in got:
        assert (d, r) == (distinct, rows)
    per = np.array([m for *_, m in got])
    assert per.sum() == len(src) and np.abs(per / per.mean() - 1).max() < 0.05
