"""Shared by the tests of the transitive triangle (csrc/k_tri_nodes.hip, routes "triangle_transitive" and
"triangle_transitive_grouped"):
  MATCH (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a) RETURN count(*)            (r1, r2, r3 pairwise distinct)
  MATCH (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a) RETURN id(a), count(*)     (or id(b), or id(c))
A brute-force enumeration of the bindings and a dense closed form of the per-node counts; neither shares anything
with the device kernels.  The graphs are those of tests/tri_ref.py and tests/tri_grouped_ref.py, re-exported.

The closed form.  With m(x,y) the multiplicity of x -> y for x != y, s(x) the self-loops at x, A the loop-free
multiplicity matrix and Q = A (A - 1), R = A A^T elementwise:
  three distinct nodes   T = (A @ A) * A: T[a,c] = sum_b m(a,b) m(b,c) m(a,c); its row sums are the source's
                         counts, its column sums the sink's, and the middle's are the row sums of (A^T @ A) * A
                         (sum over a and c of m(a,b) m(a,c) m(b,c))
  a = b = x, c = y       s(x) Q[x,y]       to x as source and middle, to y as sink
  b = c = y, a = x       Q[x,y] s(y)       to x as source, to y as middle and sink
  a = c = x, b = y       R[x,y] s(x)       to x as source and sink, to y as middle
  a = b = c = x          s(x) (s(x)-1) (s(x)-2)
"""
import numpy as np

from tri_ref import random_multigraph  # noqa: F401  (re-exported)
from tri_grouped_ref import (BY_NODE_WIN, PRIME_LOOPS, PRIMES, TILE_SLOTS, clique_and_triangles,  # noqa: F401
                             degree_order, disjoint_triangles, heavy_triangle, prime_triangle, relabel, star_behind,
                             tagged_graph, walk_slots)

SOURCE, MIDDLE, SINK = 0, 1, 2  # include/capsmi.h CAPSMI_TRI_ROLE_*: the positions a, b, c
ROLES = (SOURCE, MIDDLE, SINK)
TRANSITIVE = (">", ">", "<")    # (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a)
TILE_GRID_CAP = 8 * 256         # csrc/tile_owner.h tile_grid: 8 workgroups per CU, 256 CUs on an MI355X


# ---- the enumeration ----------------------------------------------------------------------------------------

def bindings(src, dst, ok=None, dirs=TRANSITIVE):
    """every binding (a, b, c) of the closed path (a) d1 (b) d2 (c) d3 (a): a triple loop over the relationships,
    r1, r2, r3 pairwise distinct; dirs[i] is ">" where r_i points along the path (a to b, b to c, c to a) and "<"
    where it points against it.  The default is the transitive pattern.  ok = (ok_a, ok_b, ok_c) boolean node
    filters."""
    src, dst = [int(x) for x in src], [int(x) for x in dst]
    out, inn = {}, {}
    for r, (s, d) in enumerate(zip(src, dst)):
        out.setdefault(s, []).append(r)
        inn.setdefault(d, []).append(r)
    d1, d2, d3 = dirs
    for r1 in range(len(src)):
        a, b = (src[r1], dst[r1]) if d1 == ">" else (dst[r1], src[r1])
        if ok is not None and not (ok[0][a] and ok[1][b]):
            continue
        for r2 in (out if d2 == ">" else inn).get(b, ()):  # r2 leaves b along the path, or enters it against it
            if r2 == r1:
                continue
            c = dst[r2] if d2 == ">" else src[r2]
            if ok is not None and not ok[2][c]:
                continue
            for r3 in (out if d3 == ">" else inn).get(c, ()):
                if r3 != r1 and r3 != r2 and (dst[r3] if d3 == ">" else src[r3]) == a:
                    yield a, b, c


def per_node_enumerate_all(n, src, dst, ok=None, dirs=TRANSITIVE):
    """3 x n: bindings per node at position a, b, c (for the transitive pattern: per role)"""
    cnt = np.zeros((3, n), dtype=np.int64)
    for t in bindings(src, dst, ok, dirs):
        for p in range(3):
            cnt[p, t[p]] += 1
    return cnt


def per_node_enumerate(n, src, dst, role, ok=None):
    """bindings of the transitive pattern per node in `role`"""
    return per_node_enumerate_all(n, src, dst, ok)[role]


def roles_of(dirs):
    """the role of positions a, b, c in a mixed spelling, from the out-degrees among its three relationships:
    2 the source, 1 the middle, 0 the sink (None for the two uniform spellings, the directed cycle)"""
    ends = ((0, 1), (1, 2), (2, 0))
    od = [0, 0, 0]
    for (x, y), d in zip(ends, dirs):
        od[x if d == ">" else y] += 1
    if od == [1, 1, 1]:
        return None
    return tuple({2: SOURCE, 1: MIDDLE, 0: SINK}[k] for k in od)


# ---- the closed form ----------------------------------------------------------------------------------------

def per_node_dense_all(n, src, dst, dtype=np.int64):
    """3 x n, the closed form over the dense multiplicity matrix.  dtype=object computes in Python ints (a few
    nodes); int64 is used up to 400 nodes and float64 products above that (every value below 2^53, checked)."""
    M = np.zeros((n, n), dtype=np.int64)
    np.add.at(M, (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)), 1)
    M = M.astype(dtype)
    s = np.diagonal(M).copy()
    A = M.copy()
    np.fill_diagonal(A, 0)
    if dtype is object or n <= 400:
        AA, AtA = A.dot(A), A.T.dot(A)
    else:
        Af = A.astype(np.float64)
        assert float(n) * n * float(A.max()) ** 3 < 2.0 ** 53  # every entry of the products below and their sums
        AA, AtA = np.rint(Af @ Af).astype(np.int64), np.rint(Af.T @ Af).astype(np.int64)
    T = AA * A
    Q, R = A * (A - 1), A * A.T
    t1, t2, t3 = s[:, None] * Q, Q * s[None, :], R * s[:, None]
    self3 = s * (s - 1) * (s - 2)
    source = T.sum(axis=1) + t1.sum(axis=1) + t2.sum(axis=1) + t3.sum(axis=1) + self3
    middle = (AtA * A).sum(axis=1) + t1.sum(axis=1) + t2.sum(axis=0) + t3.sum(axis=0) + self3
    sink = T.sum(axis=0) + t1.sum(axis=0) + t2.sum(axis=0) + t3.sum(axis=1) + self3
    return np.stack([source, middle, sink])


def per_node_dense(n, src, dst, role):
    return per_node_dense_all(n, src, dst)[role]


def rows_of(cnt, ids=None):
    """the result rows [(id, count)] of a count vector: the nodes with a non-zero count"""
    nz = np.nonzero(cnt)[0]
    return [{"id": int(ids[i] if ids is not None else i), "n": int(cnt[i])} for i in nz]
