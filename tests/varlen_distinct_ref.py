"""References for count(DISTINCT b) over a bounded var-length expand (the yardstick, not the code under test).

``trail_ends``: the distinct end nodes of the relationship-distinct paths from one start node, by depth-first
enumeration -- the reference's semantics, tiny and slow.
``reach_sets``: the same sets for every start node at once as a bit-parallel walk BFS in numpy (64 sources per
word), valid for lower <= 1 by the lemma of DESIGN.md section 4; also the size of their union.
"""
import numpy as np


def trail_ends(n, src, dst, a, lower, upper):
    """The set of b that end a path of lower..upper distinct relationships from a (a itself for length 0)."""
    out = [[] for _ in range(n)]
    for e, (u, v) in enumerate(zip(src, dst)):
        out[int(u)].append((e, int(v)))
    ends = set()
    if lower == 0:
        ends.add(a)
    used = set()

    def walk(v, depth):
        if depth >= lower and depth >= 1:
            ends.add(v)
        if depth == upper:
            return
        for e, w in out[v]:
            if e not in used:
                used.add(e)
                walk(w, depth + 1)
                used.discard(e)

    walk(a, 0)
    return ends


def reach_sets(n, src, dst, a_mask, b_mask, lower, upper):
    """Per-source counts |D(a)| (an int64 array over the n ids, 0 outside a_mask) and |U_a D(a)|, where
    D(a) = (nodes reached from a by a walk of 1..upper relationships) & b_mask, plus a itself when lower = 0
    -- whatever b_mask says of a, and once."""
    assert lower in (0, 1) and upper >= 1
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    a_mask = np.asarray(a_mask, dtype=bool)
    b_mask = np.asarray(b_mask, dtype=bool)
    keep = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    src, dst = src[keep], dst[keep]
    order = np.argsort(dst, kind="stable")
    src, dst = src[order], dst[order]
    heads, starts = np.unique(dst, return_index=True)  # runs of equal targets
    sources = np.nonzero(a_mask)[0]
    counts = np.zeros(n, dtype=np.int64)
    union = np.zeros(n, dtype=bool)
    for base in range(0, len(sources), 64):
        batch = sources[base:base + 64]
        bits = np.uint64(1) << np.arange(len(batch), dtype=np.uint64)
        seen = np.zeros(n, dtype=np.uint64)
        front = np.zeros(n, dtype=np.uint64)
        front[batch] = bits
        for _ in range(upper):
            nxt = np.zeros(n, dtype=np.uint64)
            if len(src):
                nxt[heads] = np.bitwise_or.reduceat(front[src], starts)
            front = nxt & ~seen
            seen |= front
            if not front.any():
                break
        if lower == 0:  # the zero-length path: a is in D(a) without b's filter
            hit = seen & np.where(b_mask, ~np.uint64(0), np.uint64(0))
            hit[batch] |= bits
        else:
            hit = seen & np.where(b_mask, ~np.uint64(0), np.uint64(0))
        union |= hit != 0
        for j, a in enumerate(batch):
            counts[a] = int(((hit >> np.uint64(j)) & np.uint64(1)).sum())
    return counts, int(union.sum())
