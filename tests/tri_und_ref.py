"""Shared by the tests of the undirected triangle (csrc/k_tri_nodes.hip, routes "triangle_undirected" and
"triangle_undirected_grouped"):
  MATCH (a)-[r1]-(b)-[r2]-(c)-[r3]-(a) RETURN count(*)            (r1, r2, r3 pairwise distinct)
  MATCH (a)-[r1]-(b)-[r2]-(c)-[r3]-(a) RETURN id(a), count(*)     (or id(b), or id(c))
An enumeration of the plan RelationalPlanner emits for it and a dense closed form of the per-node counts; neither
shares anything with the device kernels.  The graphs are those of tests/tri_trans_ref.py, re-exported.

The plan is a union of eight branches, one per orientation of the three hops.  The two Expands (hops a-b and b-c)
run their outgoing branch over every relationship and their incoming branch over the relationships with
start <> end, so they bind a self-loop once.  The closing ExpandInto between c and a is a union of two joins, (c
at the start, a at the end) and (a at the start, c at the end), neither filtered: it binds a self-loop twice.

The closed form.  With m(x,y) the multiplicity of x -> y for x != y, s(x) the self-loops at x, A the loop-free
multiplicity matrix, U = A + A^T and Q = U (U - 1) elementwise:
  three distinct nodes   U(a,b) U(b,c) U(c,a) per ordered triple; T(x) = sum_{y,z} U(x,y) U(y,z) U(z,x) is the row
                         sum of (U @ U) * U and goes to x at every position
  a = b = x, c = y       s(x) Q[x,y]         (r1 a loop)
  b = c = y, a = x       Q[x,y] s(y)         (r2 a loop)
  a = c = x, b = y       2 s(x) Q[x,y]       (r3 a loop, bound twice)
  a = b = c = x          2 s(x) (s(x)-1) (s(x)-2)
so a and c (the ends of the ExpandInto) get T + sum_y [3 s(x) + s(y)] Q[x,y] + self and b (the middle) gets
T + sum_y [2 s(x) + 2 s(y)] Q[x,y] + self.
"""
import numpy as np

from tri_trans_ref import (BY_NODE_WIN, PRIME_LOOPS, PRIMES, TILE_GRID_CAP, TILE_SLOTS,  # noqa: F401
                           clique_and_triangles, degree_order, disjoint_triangles, heavy_triangle, prime_triangle,
                           random_multigraph, relabel, rows_of, star_behind, tagged_graph, walk_slots)

END, MIDDLE = 0, 1            # include/capsmi.h CAPSMI_TRI_UND_*: the class of positions a and c, and of b
CLASSES = (END, MIDDLE)
CLASS_OF = (END, MIDDLE, END)  # of positions a, b, c


# ---- the enumeration of the plan ----------------------------------------------------------------------------

def bindings(src, dst, ok=None):
    """every row (a, b, c) of the eight branches; ok = (ok_a, ok_b, ok_c) boolean node filters"""
    src, dst = [int(x) for x in src], [int(x) for x in dst]
    m = len(src)
    # an Expand from x: (relationship, the node reached), outgoing over every relationship, incoming over the
    # relationships with start <> end
    step = {}
    for r in range(m):
        step.setdefault(src[r], []).append((r, dst[r]))
        if src[r] != dst[r]:
            step.setdefault(dst[r], []).append((r, src[r]))
    # the ExpandInto between c and a: both joins over every relationship
    into = {}
    for r in range(m):
        into.setdefault((src[r], dst[r]), []).append(r)   # c at the start, a at the end
        into.setdefault((dst[r], src[r]), []).append(r)   # a at the start, c at the end
    for a in sorted(step):
        if ok is not None and not ok[0][a]:
            continue
        for r1, b in step[a]:
            if ok is not None and not ok[1][b]:
                continue
            for r2, c in step.get(b, ()):
                if r2 == r1 or (ok is not None and not ok[2][c]):
                    continue
                for r3 in into.get((c, a), ()):
                    if r3 != r1 and r3 != r2:
                        yield a, b, c


def per_node_enumerate_all(n, src, dst, ok=None):
    """3 x n: rows per node at position a, b, c"""
    cnt = np.zeros((3, n), dtype=np.int64)
    for t in bindings(src, dst, ok):
        for p in range(3):
            cnt[p, t[p]] += 1
    return cnt


# ---- the closed form ----------------------------------------------------------------------------------------

def per_node_dense_all(n, src, dst, dtype=np.int64):
    """3 x n (positions a, b, c), the closed form over the dense multiplicity matrix.  dtype=object computes in
    Python ints (a few nodes); int64 is used up to 400 nodes and float64 products above that (every value below
    2^53, checked)."""
    M = np.zeros((n, n), dtype=np.int64)
    np.add.at(M, (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)), 1)
    M = M.astype(dtype)
    s = np.diagonal(M).copy()
    A = M.copy()
    np.fill_diagonal(A, 0)
    U = A + A.T
    if dtype is object or n <= 400:
        UU = U.dot(U)
    else:
        Uf = U.astype(np.float64)
        assert float(n) * n * float(U.max()) ** 3 < 2.0 ** 53  # every entry of the product below and the sums
        UU = np.rint(Uf @ Uf).astype(np.int64)
    T = (UU * U).sum(axis=1)
    Q = U * (U - 1)
    qs, qy = Q.sum(axis=1), Q.dot(s)  # sum_y Q[x,y], sum_y Q[x,y] s(y)
    self3 = 2 * s * (s - 1) * (s - 2)
    end = T + 3 * s * qs + qy + self3
    middle = T + 2 * s * qs + 2 * qy + self3
    return np.stack([end, middle, end])
