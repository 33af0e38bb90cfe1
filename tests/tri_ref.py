"""Shared by the tests of the sorted triangle build (csrc/k_tri.hip, tri_build's path for CAPSMI_TRI_BUILD=sorted
and for every domain above 2^24 ids):
  MATCH (a)-[r1]->(b)-[r2]->(c)-[r3]->(a) RETURN count(*)      (r1, r2, r3 pairwise distinct, a, b, c nodes)
Hand-built graphs that sit on that build's kernel edges, placements of their nodes into id windows on both
sides of the 2^24-id limit of the key layouts, and a plain restatement of the count that shares nothing with
the device kernels or with oracle/rmat.c.

The restatement.  With M the multiplicity matrix of the kept relationships (both ends in the window and in
the node table) and s(u) = M[u, u], the closed 3-walks number trace(M^3).  A relationship can repeat inside a
closed 3-walk only when it is a self-loop (two different steps of a walk that use one non-loop relationship
would need a = b = c), so the walks to take off are those on one vertex that use a loop twice or more:
  count = trace(M^3) - sum_u (s(u)^3 - s(u) (s(u) - 1) (s(u) - 2)).

The edges the graphs are built around (k_tri.hip):
  - k_und_runs walks an undirected run (all relationships between two nodes, either direction) of up to
    kShortRun = 32 keys in its lane and lists longer ones for k_und_long, a workgroup per run with a stride
    of 256 lanes over four waves of 64;
  - k_orient codes multiplicities below 15 in 4 bits per direction and appends the others to the exception
    list by wave ballot (k_exc_place puts them back after the key-only sort);
  - k_pack keeps the direction bit at bit 31 for windows of up to 2^24 ids (msh = 0) and below the upper end's
    id above that (msh = 1); dropped relationships become all-ones keys, which must sort behind a valid key
    whose upper end is 2^24 - 1 (all ones in its sorted digits);
  - the degree sort takes one digit per 8 bits of the largest degree (none when every degree is 0).

Graphs are (k, src, dst) over core indices 0 .. k - 1.  A placement maps core index i to the relative id
rel[i], increasing in i, so "lower" and "upper" mean the same by core index and by placed id.
"""
import functools
from collections import namedtuple

import numpy as np

RUN_LENGTHS = (1, 2, 14, 15, 16, 31, 32, 33, 63, 64, 65, 255, 256, 257, 600)
RUN_MODES = ("up", "down", "split")  # all lower -> upper, all upper -> lower, ceil(L/2) up and floor(L/2) down
RUNS_K = 48
RUNS_LOOPS = ((5, 1), (11, 2), (19, 3), (23, 1), (29, 5), (35, 40))  # (core node, self-loops)
EXC_K = 70
EXC_MULT = 15  # the 4-bit code's saturation: the exact payload is an exception
HUB_K = 70_001  # hub + 70,000 neighbours: a degree of at least 2^16 (three digits in the degree sort)
DENSE_K = 2200  # out-degrees above one 2048-entry LDS chunk
W24 = 1 << 24
FAR_LO = (1 << 40) + 12345


# ---- the restatement ----------------------------------------------------------------------------------------

def _kept(k, src, dst, ok):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if ok is None:
        return src, dst
    keep = ok[src] & ok[dst]
    return src[keep], dst[keep]


def _loop_walks(loops):
    return sum(s ** 3 - s * (s - 1) * (s - 2) for s in loops)


def dense_count(k, src, dst, ok=None):
    """(count(*), distinct unordered non-loop pairs) of the relationships with both ends ok, from the k x k
    multiplicity matrix: Python ints up to 256 nodes, above that float64 (exact below 2^53, checked)."""
    assert k <= 4096, "the dense form is for a few thousand nodes at the most"
    s, d = _kept(k, src, dst, ok)
    M = np.zeros((k, k), dtype=np.int64)
    np.add.at(M, (s, d), 1)
    und = (M + M.T) > 0
    np.fill_diagonal(und, False)
    pairs = int(und.sum()) // 2
    loops = [int(x) for x in np.diagonal(M)]
    if k <= 256:
        Mo = M.astype(object)
        walks = int(np.trace(Mo.dot(Mo).dot(Mo)))
    else:
        assert k * k * int(M.max()) ** 3 < 2 ** 53  # every entry of M^3 and the trace
        Mf = M.astype(np.float64)
        walks = int(round(np.trace(Mf @ Mf @ Mf)))
    return walks - _loop_walks(loops), pairs


def sparse_count(k, src, dst, ok=None):
    """the same from a dict of multiplicities: sum over a -> b, b -> c of m(a,b) m(b,c) m(c,a) (c taken from the
    shorter of b's out-list and a's in-list), Python ints"""
    s, d = _kept(k, src, dst, ok)
    m = {}
    for a, b in zip(s.tolist(), d.tolist()):
        m[(a, b)] = m.get((a, b), 0) + 1
    out, inn = {}, {}
    for a, b in m:
        out.setdefault(a, []).append(b)
        inn.setdefault(b, []).append(a)
    walks = 0
    for (a, b), mab in m.items():
        ob, ia = out.get(b, ()), inn.get(a, ())
        if len(ob) <= len(ia):
            walks += mab * sum(m[(b, c)] * m.get((c, a), 0) for c in ob)
        else:
            walks += mab * sum(m.get((b, c), 0) * m[(c, a)] for c in ia)
    pairs = len({(min(a, b), max(a, b)) for a, b in m if a != b})
    return walks - _loop_walks(m.get((u, u), 0) for u in out), pairs


# ---- builders (core indices) --------------------------------------------------------------------------------

Graph = namedtuple("Graph", "k src dst")


def _graph(k, src, dst, seed=None):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if seed is not None:  # relationship order shuffled
        p = np.random.default_rng(seed).permutation(len(src))
        src, dst = src[p], dst[p]
    src.setflags(write=False)
    dst.setflags(write=False)
    return Graph(k, src, dst)


@functools.lru_cache(maxsize=None)
def runs_pairs():
    """the unordered pairs (lower, upper) of `runs` in key order, seeded density 0.3"""
    rng = np.random.default_rng(101)
    take = rng.random((RUNS_K, RUNS_K)) < 0.3
    return [(i, j) for i in range(RUNS_K) for j in range(i + 1, RUNS_K) if take[i, j]]


def runs_spec():
    """[(lower, upper, relationships lower -> upper, relationships upper -> lower)] of the first pairs: every
    run length three times"""
    pairs = runs_pairs()
    spec = []
    for L in RUN_LENGTHS:
        for mode in RUN_MODES:
            i, j = pairs[len(spec)]
            up = {"up": L, "down": 0, "split": (L + 1) // 2}[mode]
            spec.append((i, j, up, L - up))
    return spec


@functools.lru_cache(maxsize=None)
def runs():
    rng = np.random.default_rng(102)
    spec = runs_spec()
    src, dst = [], []
    for i, j, up, down in spec:
        src += [i] * up + [j] * down
        dst += [j] * up + [i] * down
    for i, j in runs_pairs()[len(spec):]:
        both, flip = rng.random() < 0.1, rng.random() < 0.5
        if both or not flip:
            src.append(i), dst.append(j)
        if both or flip:
            src.append(j), dst.append(i)
    for v, s in RUNS_LOOPS:
        src += [v] * s
        dst += [v] * s
    return _graph(RUNS_K, src, dst, seed=103)


@functools.lru_cache(maxsize=None)
def all_exceptions():
    """complete digraph on 70 nodes, every direction 15 times: every lane of every wave of k_orient appends"""
    a, b = np.nonzero(~np.eye(EXC_K, dtype=bool))
    return _graph(EXC_K, np.repeat(a, EXC_MULT), np.repeat(b, EXC_MULT), seed=104)


@functools.lru_cache(maxsize=None)
def one_exception():
    """the same with multiplicity 1, but 15 both ways on the pair that is last in (lower, upper) key order"""
    a, b = np.nonzero(~np.eye(EXC_K, dtype=bool))
    reps = np.where((np.minimum(a, b) == EXC_K - 2) & (np.maximum(a, b) == EXC_K - 1), EXC_MULT, 1)
    return _graph(EXC_K, np.repeat(a, reps), np.repeat(b, reps), seed=105)


@functools.lru_cache(maxsize=None)
def hub():
    """core 0 is the hub: hub -> w_i, w_i -> w_{i+1} (cyclic), w_j -> hub for every 13th j"""
    w = np.arange(1, HUB_K, dtype=np.int64)
    back = w[::13]
    src = np.concatenate([np.zeros(len(w), np.int64), w, back])
    dst = np.concatenate([w, np.roll(w, -1), np.zeros(len(back), np.int64)])
    return _graph(HUB_K, src, dst, seed=106)


@functools.lru_cache(maxsize=None)
def dense():
    """complete loop-free digraph on 2200 nodes, multiplicity 1"""
    a, b = np.nonzero(~np.eye(DENSE_K, dtype=bool))
    return _graph(DENSE_K, a, b)


@functools.lru_cache(maxsize=None)
def random_multigraph(seed):
    """the generator of tests/test_gpu_triangles.py test_random_multigraphs: n 3..60, m < 600, self-loops"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 60))
    m = int(rng.integers(0, 600))
    src = rng.integers(0, n, m).astype(np.int64)
    dst = rng.integers(0, n, m).astype(np.int64)
    src[: m // 6] = dst[: m // 6]
    return _graph(n, src, dst)


def no_relationships():
    return _graph(RUNS_K, [], [])


LOOPS_ONLY = ((3, 1), (17, 2), (30, 3), (47, 40))


def loops_only():
    v = [u for u, s in LOOPS_ONLY for _ in range(s)]
    return _graph(RUNS_K, v, v, seed=107)


def all_dropped():
    """(graph, node filter): every relationship, the self-loops too, has an end at an odd core node, and the
    node table holds the even ones: no key survives, every degree is 0"""
    rng = np.random.default_rng(108)
    odd = rng.integers(0, RUNS_K // 2, 400) * 2 + 1
    other = rng.integers(0, RUNS_K, 400)
    other[:40] = odd[:40]
    flip = rng.random(400) < 0.5
    g = _graph(RUNS_K, np.where(flip, odd, other), np.where(flip, other, odd))
    return g, np.arange(RUNS_K) % 2 == 0


BUILDERS = {"runs": runs, "all_exceptions": all_exceptions, "one_exception": one_exception, "hub": hub,
            "dense": dense}


# ---- placements ---------------------------------------------------------------------------------------------

Placement = namedtuple("Placement", "lo n rel")  # the window [lo, lo + n), relative id of each core index


def _spread(k, n, named, seed):
    """k distinct increasing relative ids below n that include `named`"""
    rng = np.random.default_rng(seed)
    ids = set(named)
    while len(ids) < k:
        ids.update(int(x) for x in rng.integers(0, n, k - len(ids)))
    return np.array(sorted(ids), dtype=np.int64)


PLACEMENTS = ("low", "edge24", "wide", "wide_offset", "last_far")


@functools.lru_cache(maxsize=None)
def place(name, k):
    """low: the window is the k core ids.  edge24: 2^24 ids, the last window of the bit-31 layout, core ids 0, 1,
    2^24 - 2 and 2^24 - 1 among seeded others.  wide: 2^24 + 1 ids, the first window of the wide layout, with 0,
    2^24 - 1 and 2^24.  wide_offset: the same relative ids from 2^40 + 12345.  last_far: 0 .. k - 2 and 2^24 in
    the wide window (a big graph's own ids with its last node moved)."""
    if name == "low":
        p = Placement(0, k, np.arange(k, dtype=np.int64))
    elif name == "edge24":
        p = Placement(0, W24, _spread(k, W24, (0, 1, W24 - 2, W24 - 1), 201))
    elif name in ("wide", "wide_offset"):
        p = Placement(0 if name == "wide" else FAR_LO, W24 + 1, _spread(k, W24 + 1, (0, W24 - 1, W24), 202))
    elif name == "last_far":
        rel = np.arange(k, dtype=np.int64)
        rel[-1] = W24
        p = Placement(0, W24 + 1, rel)
    else:
        raise KeyError(name)
    p.rel.setflags(write=False)
    return p


# ---- cases: a graph in a window, as the tables the library sees ---------------------------------------------

Case = namedtuple("Case", "lo n node_ids src dst k core_src core_dst core_ok")
N_DROPPED = 200


def node_filter(k):
    """removes one core node in five: 4, 9, 14, ... (never one of the two lowest or the two highest, which the
    placements name)"""
    i = np.arange(k)
    return ~((i % 5 == 4) & (i < k - 2))


def materialise(g, p, dropped=False, core_ok=None):
    """The node ids and the relationships' Long ids of graph g under placement p.  `dropped`: a node filter that
    removes one core node in five, and 200 more relationships with an end at lo - 1, at hi, or at an in-window id
    that is in no node table, mixed into the row order."""
    lo, n, rel = p
    assert len(rel) == g.k
    ok = np.ones(g.k, bool) if core_ok is None else core_ok.copy()
    src, dst = lo + rel[g.src], lo + rel[g.dst]
    if dropped:
        ok &= node_filter(g.k)
        rng = np.random.default_rng(301)
        present = set(rel.tolist())
        holes = [r for r in [int(x) + 1 for x in rel[:40].tolist()] + [n // 2, n - 2] if r < n and r not in present]
        holes += [int(r) for r in rel[~ok][:8].tolist()]  # a core node that the filter removed
        assert holes
        good = lo + rel[ok]
        xs, xd = [], []
        for t in range(N_DROPPED):
            bad = (lo - 1, lo + n, lo + holes[(t // 3) % len(holes)])[t % 3]
            other = int(good[rng.integers(0, len(good))])
            if t % 7 == 0:  # both ends outside, for different reasons
                other = (lo + n, lo + holes[0], lo - 1)[t % 3]
            if t % 11 == 0:  # a self-loop outside
                other = bad
            a, b = (bad, other) if t % 2 else (other, bad)
            xs.append(a), xd.append(b)
        src = np.concatenate([src, np.array(xs, dtype=np.int64)])
        dst = np.concatenate([dst, np.array(xd, dtype=np.int64)])
        perm = rng.permutation(len(src))
        src, dst = src[perm], dst[perm]
    return Case(lo, n, lo + rel[ok], src, dst, g.k, g.src, g.dst, ok)


@functools.lru_cache(maxsize=None)
def case(graph, placement, dropped=False):
    g = BUILDERS[graph]()
    return materialise(g, place(placement, g.k), dropped)


@functools.lru_cache(maxsize=None)
def expected(graph, dropped=False):
    """(count(*), distinct kept pairs) of a builder's graph, with or without the `dropped` node filter; the
    placement does not enter (the count is label-invariant): sparse form for the hub, dense otherwise"""
    g = BUILDERS[graph]()
    ok = node_filter(g.k) if dropped else None
    return (sparse_count if graph == "hub" else dense_count)(g.k, g.src, g.dst, ok)


def expected_of(c):
    """the same for any Case (the random and the trivial graphs)"""
    return dense_count(c.k, c.core_src, c.core_dst, c.core_ok)
