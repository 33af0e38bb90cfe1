"""Shared by the tests of the grouped cyclic triangle (csrc/k_tri_nodes.hip, route "triangle_grouped"):
  MATCH (a)-[r1]->(b)-[r2]->(c)-[r3]->(a) RETURN id(a), count(*)     (r1, r2, r3 pairwise distinct)
Two plain restatements of the per-node counts that share nothing with the device kernels, mirrors of the
kernel's constants, and the hand-built graphs that sit on its edges.

The closed form.  With m(x,y) the multiplicity of x -> y for x != y and s(x) the self-loops at x, a binding
that starts at x has three distinct nodes (a closed 3-walk of the loop-free multiplicity matrix A: diag(A^3)),
two (one relationship is a self-loop, at a, at b or at c: m(x,y) m(y,x) (s(x) + s(y) + s(x))), or one (three
different self-loops at x):
  count(x) = diag(A^3)[x] + sum_{y != x} m(x,y) m(y,x) (2 s(x) + s(y)) + s(x) (s(x)-1) (s(x)-2).
"""
import functools

import numpy as np

# csrc/k_tri_nodes.hip kByNodeWin: the degree-order ids [0, BY_NODE_WIN) are counted in the workgroup's LDS window
BY_NODE_WIN = 64
# csrc/capsmi_impl.h kExplodeTile: slots (oriented edge, position in the walked list) per tile of the walk
TILE_SLOTS = 2048


# ---- the restatements ---------------------------------------------------------------------------------------

def bindings(src, dst, ok=None):
    """every binding (a, b, c): a triple loop over the relationships, r1, r2, r3 pairwise distinct, r2 starting
    where r1 ends, r3 where r2 ends, and ending where r1 starts; ok = (ok_a, ok_b, ok_c) boolean node filters"""
    src, dst = [int(x) for x in src], [int(x) for x in dst]
    out = {}
    for r, s in enumerate(src):
        out.setdefault(s, []).append(r)
    for r1 in range(len(src)):
        a, b = src[r1], dst[r1]
        if ok is not None and not (ok[0][a] and ok[1][b]):
            continue
        for r2 in out.get(b, ()):
            if r2 == r1:
                continue
            c = dst[r2]
            if ok is not None and not ok[2][c]:
                continue
            for r3 in out.get(c, ()):
                if r3 != r1 and r3 != r2 and dst[r3] == a:
                    yield a, b, c


def per_node_enumerate(n, src, dst, group="a", ok=None):
    """bindings per node at position `group` (a, b or c)"""
    cnt = np.zeros(n, dtype=np.int64)
    at = "abc".index(group)
    for t in bindings(src, dst, ok):
        cnt[t[at]] += 1
    return cnt


def per_node_dense(n, src, dst):
    """the closed form over the dense multiplicity matrix: int64 up to 400 nodes, float64 above that (every
    value below 2^53, checked, as tests/test_gpu_triangles.py test_complete_digraph_chunks)"""
    M = np.zeros((n, n), dtype=np.int64)
    np.add.at(M, (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)), 1)
    s = np.diagonal(M).copy()
    A = M.copy()
    np.fill_diagonal(A, 0)
    if n <= 400:
        tri = np.einsum("ij,ji->i", A @ A, A)
    else:
        Af = A.astype(np.float64)
        trif = np.einsum("ij,ji->i", Af @ Af, Af)
        assert float(n) * n * float(A.max()) ** 3 < 2.0 ** 53  # every entry of A^2 . A^T's rows, and their sums
        tri = np.rint(trif).astype(np.int64)
    R = A * A.T  # m(x,y) m(y,x)
    pair = 2 * s * R.sum(axis=1) + R @ s
    return tri + pair + s * (s - 1) * (s - 2)


def rows_of(cnt, ids=None):
    """the result rows [(id, count)] of a count vector: the nodes with a non-zero count"""
    nz = np.nonzero(cnt)[0]
    return [{"id": int(ids[i] if ids is not None else i), "n": int(cnt[i])} for i in nz]


# ---- a mirror of the walk's slots ---------------------------------------------------------------------------

def degree_order(n, src, dst):
    """degree-order id of every node, as tri_build ranks them: by (relationship count without loops, id), the
    highest first (exact degrees: every graph here has fewer than 2^22 relationships)"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    nl = src != dst
    deg = np.bincount(src[nl], minlength=n) + np.bincount(dst[nl], minlength=n)
    order = np.lexsort((np.arange(n), deg))      # ascending (degree, id)
    rid = np.empty(n, dtype=np.int64)
    rid[order] = n - 1 - np.arange(n)            # degree-order id: 0 = the highest (degree, id)
    return rid


def walk_slots(n, src, dst):
    """The slots of k_tri_walk on the graph: vertices in degree order, each pair oriented from its lower-ranked
    end, out-lists sorted by rank; the edge u -> v at position p of out(u) owns min(od(v), p) slots.  Returns the
    slots per oriented edge in (u, position) order."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    nl = src != dst
    rid = degree_order(n, src, dst)
    a, b = rid[src[nl]], rid[dst[nl]]
    pairs = np.unique(np.stack([np.maximum(a, b), np.minimum(a, b)], axis=1), axis=0)  # from (larger id) -> to
    od = np.bincount(pairs[:, 0], minlength=n)
    first = np.concatenate([[0], np.cumsum(od)])[:-1]
    p = np.arange(len(pairs)) - first[pairs[:, 0]]  # np.unique sorted the rows by (from, to)
    return np.minimum(od[pairs[:, 1]], p)


# ---- builders -----------------------------------------------------------------------------------------------

def _frozen(n, src, dst, seed):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    perm = np.random.default_rng(seed).permutation(len(src))
    src, dst = src[perm], dst[perm]
    src.setflags(write=False)
    dst.setflags(write=False)
    return n, src, dst


@functools.lru_cache(maxsize=None)
def disjoint_triangles(t):
    """t disjoint directed triangles: each owns exactly one slot (its lowest-ranked corner's second edge)"""
    x = 3 * np.arange(t, dtype=np.int64)
    return _frozen(3 * t, np.concatenate([x, x + 1, x + 2]), np.concatenate([x + 1, x + 2, x]), 401)


CLIQUE_K = 20    # one large clique: C(20, 3) = 1140 slots in rows of up to 18
SMALL_K, SMALL_COPIES = 5, 150  # then small cliques, 10 slots each in rows of 1, 2 and 3: the first tile end falls here


@functools.lru_cache(maxsize=None)
def clique_and_triangles(slots):
    """a complete digraph on CLIQUE_K nodes with multiplicities 1..3, SMALL_COPIES complete digraphs on SMALL_K
    nodes (rows of more than one slot around the first tile end), then as many disjoint triangles (the lowest
    degrees: the last rows) as bring the walk to `slots` slots"""
    rng = np.random.default_rng(402)
    M = rng.integers(1, 4, (CLIQUE_K, CLIQUE_K))
    np.fill_diagonal(M, 0)
    a, b = np.nonzero(M)
    src, dst = [np.repeat(a, M[a, b])], [np.repeat(b, M[a, b])]
    sa, sb = np.nonzero(~np.eye(SMALL_K, dtype=bool))
    n = CLIQUE_K
    for _ in range(SMALL_COPIES):
        src.append(sa + n), dst.append(sb + n)
        n += SMALL_K
    base = int(walk_slots(n, np.concatenate(src), np.concatenate(dst)).sum())
    t = slots - base
    assert t > 0
    x = n + 3 * np.arange(t, dtype=np.int64)
    src += [x, x + 1, x + 2]
    dst += [x + 1, x + 2, x]
    g = _frozen(n + 3 * t, np.concatenate(src), np.concatenate(dst), 403)
    assert int(walk_slots(*g).sum()) == slots
    return g


STAR_T = 3  # directed triangles through the star's centre


@functools.lru_cache(maxsize=None)
def star_behind(fillers):
    """(graph, centre): a star of STAR_T directed triangles through one centre (with two self-loops and one
    reciprocal spoke: pair and self terms on the same counter) whose degree-order id is exactly `fillers`:
    that many filler nodes have a higher degree (a fan of leaves each; the first three also close a triangle
    and the first carries self-loops and a reciprocal leaf), every other node a lower one."""
    T = STAR_T
    D = 2 * T + 3
    c = 0
    src, dst = [], []
    nxt = 1
    for i in range(T):  # c -> x -> y -> c
        x, y = nxt, nxt + 1
        nxt += 2
        src += [c, x, y]
        dst += [x, y, c]
    src += [1, c, c]  # x_0 -> c as well; two self-loops at c
    dst += [c, c, c]
    f0 = nxt
    nxt += fillers
    for j in range(fillers):
        for _ in range(D):
            src.append(f0 + j)
            dst.append(nxt)
            nxt += 1
    if fillers >= 3:
        src += [f0, f0 + 1, f0 + 2, f0, f0, f0, f0 + fillers]  # a triangle, three loops, a leaf's way back
        dst += [f0 + 1, f0 + 2, f0, f0, f0, f0, f0]
    n = nxt
    g = _frozen(n, src, dst, 404)
    nl = g[1] != g[2]
    deg = np.bincount(g[1][nl], minlength=n) + np.bincount(g[2][nl], minlength=n)
    assert int((deg > deg[c]).sum()) == fillers and int((deg == deg[c]).sum()) == 1  # the centre's id is `fillers`
    return g, c


@functools.lru_cache(maxsize=None)
def heavy_triangle():
    """one triangle with multiplicity 1700 on each of its six directed edges and 3 self-loops on one corner:
    per-node counts above 2^32, every coded multiplicity field at its all-ones value"""
    e = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 0), (0, 2)]
    src = np.repeat([a for a, _ in e], 1700).tolist() + [2, 2, 2]
    dst = np.repeat([b for _, b in e], 1700).tolist() + [2, 2, 2]
    return _frozen(3, src, dst, 405)


def heavy_triangle_counts():
    m = 1700
    w = 2 * m ** 3
    return np.array([w + m * m * 3, w + m * m * 3, w + 2 * m * m * 6 + 6], dtype=np.int64)


# one triangle, six different multiplicities, every degree order (shared with the transitive and undirected tests)
PRIMES = {(0, 1): 2, (1, 0): 3, (1, 2): 5, (2, 1): 7, (0, 2): 11, (2, 0): 13}
PRIME_LOOPS = (1, 2, 4)   # self-loops at the corners 0, 1, 2
PENDANT_UNIT = 40         # see prime_triangle


@functools.lru_cache(maxsize=None)
def prime_triangle(pendants):
    """The triangle {0, 1, 2} with m(0,1), m(1,0), m(1,2), m(2,1), m(0,2), m(2,0) = 2, 3, 5, 7, 11, 13 and 1, 2, 4
    self-loops, and pendants[i] bundles of pendant relationships at corner i.  A corner's degree counts its
    relationships with their multiplicities (29, 17 and 36 here), so single pendant relationships would leave the
    degree order where the primes put it: a bundle is PENDANT_UNIT relationships, each to a leaf of its own and
    pointing out of or into the corner in turn, which outweighs the triangle's own spread of 19.  The six
    permutations of (1, 2, 3) bundles put the corners into the six degree orders, so a walk that takes a payload
    half or a payload for another shows under at least one of them."""
    src, dst = [], []
    for (x, y), m in PRIMES.items():
        src += [x] * m
        dst += [y] * m
    for x, s in enumerate(PRIME_LOOPS):
        src += [x] * s
        dst += [x] * s
    n = 3
    for x, k in enumerate(pendants):
        for j in range(k * PENDANT_UNIT):
            a, b = (x, n) if j % 2 else (n, x)
            src.append(a), dst.append(b)
            n += 1
    return _frozen(n, src, dst, 501)


# ---- the tagged-id graph ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tagged_graph():
    """(node ids, src, dst, tag of each node id): 500 nodes at most with ids below 2^20, 8000 relationships with
    skewed endpoints and self-loops -- the construction of tests/test_gpu_sparse_ids.py
    test_triangles_on_tagged_ids -- and every second node id carrying graph tag 3 in its top 10 bits"""
    rng = np.random.default_rng(7)
    n, m, spread = 500, 8000, 1 << 20
    ids = np.unique(rng.integers(0, spread, n))
    n = len(ids)
    w = rng.zipf(1.6, m) % n  # skewed endpoints (hubs)
    u = rng.integers(0, n, m)
    src, dst = ids[np.where(rng.random(m) < 0.5, w, u)], ids[rng.integers(0, n, m)]
    src[: m // 50] = dst[: m // 50]  # self-loops
    tags = {int(v): (int(v) | (3 << 54)) if i % 2 else int(v) for i, v in enumerate(ids)}
    return ids.astype(np.int64), src.astype(np.int64), dst.astype(np.int64), tags


def relabel(ids, src, dst):
    """(k, src, dst as indices into ids): every endpoint here is a node id"""
    pos = {int(v): i for i, v in enumerate(ids)}
    return len(ids), np.array([pos[int(x)] for x in src]), np.array([pos[int(x)] for x in dst])
