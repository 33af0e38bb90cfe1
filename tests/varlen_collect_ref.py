"""Reference for collect(DISTINCT b) over a bounded var-length expand (the yardstick, not the code under test).

``reach_lists``: for every start node of a_mask, the sorted ids of D(a) = (nodes reached from a by a walk of
1..upper relationships) & b_mask, plus a itself when lower = 0; and the sorted union of the D(a).  One plain
breadth-first search per source over an adjacency list: no bit tricks, and nothing shared with
varlen_distinct_ref.reach_sets, which test_varlen_collect_cpu.py compares it with.
"""
import numpy as np


def reach_lists(n, src, dst, a_mask, b_mask, lower, upper):
    """({a: sorted int64 ndarray of D(a)} for the a with a non-empty D(a), the sorted int64 ndarray of their union).
    Ids are relative to the window [0, n); relationships with an endpoint outside it are ignored."""
    assert lower in (0, 1) and upper >= 1
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    a_mask = np.asarray(a_mask, dtype=bool)
    b_mask = np.asarray(b_mask, dtype=bool)
    keep = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    src, dst = src[keep], dst[keep]
    order = np.argsort(src, kind="stable")
    heads = dst[order]
    starts = np.searchsorted(src[order], np.arange(n + 1))  # out-neighbours of v: heads[starts[v]:starts[v + 1]]
    lists = {}
    union = np.zeros(n, dtype=bool)
    for a in np.nonzero(a_mask)[0]:
        reached = np.zeros(n, dtype=bool)
        frontier = np.array([a], dtype=np.int64)
        for _ in range(upper):
            deg = starts[frontier + 1] - starts[frontier]
            total = int(deg.sum())
            if total == 0:
                break
            # the out-neighbours of the whole frontier: each node's run of `heads`, laid end to end
            at = np.repeat(starts[frontier] - (np.cumsum(deg) - deg), deg) + np.arange(total)
            new = np.zeros(n, dtype=bool)
            new[heads[at]] = True
            new &= ~reached
            reached |= new
            frontier = np.nonzero(new)[0]
        d = reached & b_mask
        if lower == 0:
            d[a] = True  # the zero-length path: a without b's filter, once
        if d.any():
            lists[int(a)] = np.nonzero(d)[0].astype(np.int64)
            union |= d
    return lists, np.nonzero(union)[0].astype(np.int64)
