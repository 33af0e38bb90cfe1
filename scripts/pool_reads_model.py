"""CPU model of the X reads of the pool's hop 2 (csrc/k_part.hip k_pool_hop2) on the oracle's R-MAT graph.

The pairs of one 2^19-id target slice are taken in ingest order and cut into block shares of `--share` pairs.
A share starts with an empty C slice; its pairs go by in steps of `--step` pairs (512 = one wave step, 8192 =
every wave of a block at once), and every pair of a step that finds its target unset at the start of the step
reads X(source); the ones whose source passes set the target.  Printed per share size and step: X reads per
relationship, the first encounters per relationship (distinct targets per share: what k_pool_hop1 counts as
R_est, the reads' lower bound) and the model's count(DISTINCT c) against the oracle's closed form.

Over the split pool hop 2 reads the source words on demand: a lane's 16-byte S load covers four consecutive
pairs of the step and is issued only if one of the four finds its target unset, and a 128-byte S line (32
pairs, eight lanes) is fetched only if one of its eight loads is.  Printed too: the share of S loads issued and
of S lines fetched.

With `--exchanges E` (CAPSMI_HOP2_EXCHANGE, k_pool_hop2<true, XW>) the shares of a slice advance in lockstep, as
the blocks of one launch do, and at E evenly spaced points of a share's length, its start included, every share
ORs in the bits all the slice's shares have set so far.  E = 1 exchanges at the start alone, where nothing is set
yet: the kernel without the exchange.  A 4-Mi share that covers its slice every 64 chunks exchanges about 8 times.

The share of the GPU's grid at scale 26 (2^30 relationships): 4 Mi pairs at 256 blocks, 2 Mi at 512 (the grid
chosen, two blocks per CU).  The model keeps the share size, not the block count, when run at a smaller scale.

    python scripts/pool_reads_model.py --scale 22
    python scripts/pool_reads_model.py --scale 22 --steps 512 --exchanges 1,8,16
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLICE_BITS = 19


def frontier(n, src, dst):
    """X1 = M | (>= 1 self-loop), X2 = M | (>= 2 self-loops) with every node filter full"""
    loop = src == dst
    M = np.zeros(n, bool)
    M[dst[~loop]] = True
    selfc = np.bincount(dst[loop], minlength=n)
    return M | (selfc >= 1), M | (selfc >= 2)


def any_of(flags, width):
    """per group of `width` consecutive pairs of a step: whether any is flagged"""
    pad = (-len(flags)) % width
    return np.concatenate([flags, np.zeros(pad, bool)]).reshape(-1, width).any(axis=1)


def model(n, src, dst, share, step, exchanges=1):
    X1, X2 = frontier(n, src, dst)
    ok = np.where(src == dst, X2[src], X1[src])
    j = dst >> SLICE_BITS
    order = np.argsort(j, kind="stable")  # ingest order within a slice
    bounds = np.searchsorted(j[order], np.arange((n >> SLICE_BITS) + 2))
    reads = first = 0
    s_loads = s_loads_all = s_lines = s_lines_all = 0
    C_all = np.zeros(n, bool)
    width = 1 << SLICE_BITS
    # the steps before which the shares exchange: E evenly spaced points of a share, the first at its start
    nsteps = (share + step - 1) // step
    at = {(e * nsteps) // exchanges for e in range(exchanges)}
    for sl, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        if a == b:
            continue
        base = sl << SLICE_BITS
        shares = []
        for s0 in range(a, b, share):
            idx = order[s0:min(s0 + share, b)]
            shares.append((dst[idx] - base, ok[idx], np.zeros(width, bool)))  # in-slice targets, passes, C
            first += len(np.unique(dst[idx]))
        for q in range(nsteps):  # lockstep: step q of every share
            k = q * step
            if q in at and len(shares) > 1 and q > 0:
                u = np.logical_or.reduce([C for _, _, C in shares])
                for _, _, C in shares:
                    C |= u
            for t, p, C in shares:
                if k >= len(t):
                    continue
                tt = t[k:k + step]
                unset = ~C[tt]
                reads += int(unset.sum())
                ld, ln = any_of(unset, 4), any_of(unset, 32)  # 16-byte loads (4 pairs), 128-byte lines (32)
                s_loads += int(ld.sum())
                s_loads_all += len(ld)
                s_lines += int(ln.sum())
                s_lines_all += len(ln)
                C[tt[unset & p[k:k + step]]] = True
        for _, _, C in shares:
            C_all[base:base + width] |= C[:len(C_all) - base]
    return reads, first, int(C_all.sum()), s_loads / max(1, s_loads_all), s_lines / max(1, s_lines_all)


def main():
    from oracle import cpu
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--shares", default="4194304,2097152")
    ap.add_argument("--steps", default="512,8192")
    ap.add_argument("--exchanges", default="1", help="exchange points per share, comma-separated (1: none)")
    args = ap.parse_args()
    n, m = 1 << args.scale, args.edge_factor << args.scale
    src, dst = cpu.rmat_edges(args.scale, 0, m)
    X1, _ = frontier(n, src, dst)
    _, want = cpu.two_hop_closed_form_mt(n, src, dst)
    print(f"scale {args.scale}: {m} relationships, sources with X1: {X1[src].mean():.4f} of the relationships, "
          f"oracle distinct {want}")
    for share in (int(x) for x in args.shares.split(",")):
        for step in (int(x) for x in args.steps.split(",")):
            for ex in (int(x) for x in args.exchanges.split(",")):
                reads, first, got, loads, lines = model(n, src, dst, share, step, ex)
                print(f"share {share} step {step} exchanges {ex}: X reads / rel {reads / m:.4f}, "
                      f"first encounters / rel {first / m:.4f}, "
                      f"S loads issued {loads:.4f}, S lines fetched {lines:.4f}, "
                      f"distinct {got} ({'ok' if got == want else 'MISMATCH'})")


if __name__ == "__main__":
    main()
