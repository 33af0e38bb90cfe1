"""Shared by the grouped 2-hop tests (csrc/k_grouped.hip):
  MATCH (a)-[r1]->(b)-[r2]->(c) RETURN id(a), count(*), count(DISTINCT c)
Hand-built graphs that sit on the kernels' edges, and a pure-Python restatement of the per-start counts
that shares nothing with the device kernels or with oracle/rmat.c.

The edges the graphs are built around (k_grouped.hip):
  - k_gd_large walks the c ids in ranges of R = 2^20 with one LDS bitmap per range, so the windows are
    R (one range), R + 1 (a second range of one id) and 3R + 4097 (four ranges);
  - k_gd_class sends a start to the one-wave LDS set when its work is at most 1024, else to the workgroup
    bitmap; the work of a start is the sum, over its distinct ok b's, of each b's distinct ok c's;
  - gd_walk takes a start's b's 64 at a time, and in k_gd_large chunk wv + 16k goes to wave wv;
  - drop_self = loops[a] < 2 drops c = a reached through b = a by the one self-loop.

Every builder returns (lo, n, src, dst, labels_of_node): Long ids lo + relative id with lo = 2^33 + 12345,
lo and lo + n - 1 present as nodes (so the library's id window is exactly [lo, lo + n)), src / dst the
relationships in row order, labels_of_node {id: frozenset of labels} of the ids that are nodes.  A node's
labels are the bits of its relative id % 8 (1 = A, 2 = B, 4 = C), so every combination occurs; the two
window ends carry all three so that every pattern scans them.  Row r has type S when r % 3 == 2, else R.
"""
import functools

import numpy as np

R = 1 << 20
LO = (1 << 33) + 12345
WINDOWS = (R, R + 1, 3 * R + 4097)
SMALL_MAX = 1024  # k_gd_class: work <= 1024 -> k_gd_small (2048 slots), above -> k_gd_large
LABELS = ("A", "B", "C")

# label per position (a, b, c), None = no label
PREDICATES = {"none": (None, None, None), "abc": ("A", "B", "C"), "b_only": (None, "B", None)}

HAS_A, HAS_B, HAS_C, NO_C = (1, 3, 5, 7), (2, 3, 6, 7), (4, 5, 6, 7), (0, 1, 2, 3)


def reference(src, dst, a_ok, b_ok, c_ok):
    """({a: (count(*), count(DISTINCT c))} of the starts with a binding, {a: work}) over relative ids;
    r1 <> r2 by row number."""
    src, dst = [int(x) for x in src], [int(x) for x in dst]
    out = {}
    for r, s in enumerate(src):
        out.setdefault(s, []).append(r)
    res, work = {}, {}
    for a, rows in out.items():
        if not a_ok[a]:
            continue
        cs = [dst[r2] for r1 in rows if b_ok[dst[r1]] for r2 in out.get(dst[r1], ()) if r2 != r1 and c_ok[dst[r2]]]
        if cs:
            res[a] = (len(cs), len(set(cs)))
        bs = {dst[r1] for r1 in rows if b_ok[dst[r1]]}
        work[a] = sum(len({dst[r2] for r2 in out.get(b, ()) if c_ok[dst[r2]]}) for b in bs)
    return res, work


class _Build:
    """Relative ids handed out in increasing order, 8 * slot + label code"""

    def __init__(self, n, seed):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.src, self.dst, self.not_nodes, self.slot = [], [], set(), 1
        self.marks = {}  # what the shape tests look up: name -> ids

    def new(self, code, node=True):
        v = 8 * self.slot + code
        self.slot += 1
        if not node:
            self.not_nodes.add(v)
        return v

    def many(self, codes, k):
        return [self.new(codes[i % len(codes)]) for i in range(k)]

    def rel(self, s, d, times=1):
        self.src += [s] * times
        self.dst += [d] * times

    def dangling(self, a, b, c):
        """endpoints in no node table: as b (a -> x -> c) and as c (b -> y)"""
        x, y = self.new(7, node=False), self.new(7, node=False)
        self.rel(a, x)
        self.rel(x, c)
        self.rel(b, y)

    def finish(self):
        n = self.n
        assert 8 * self.slot < R // 2
        src, dst = np.array(self.src, dtype=np.int64), np.array(self.dst, dtype=np.int64)
        assert src.min() >= 0 and dst.min() >= 0 and src.max() < n and dst.max() < n
        nodes = np.setdiff1d(np.unique(np.concatenate([src, dst, [0, n - 1]])), sorted(self.not_nodes))
        code = nodes % 8
        code[(nodes == 0) | (nodes == n - 1)] = 7
        labels = {int(v) + LO: frozenset(l for i, l in enumerate(LABELS) if c >> i & 1) for v, c in zip(nodes, code)}
        for x in (src, dst):
            x += LO
            x.setflags(write=False)
        return (LO, n, src, dst, labels), {k: tuple(v) for k, v in self.marks.items()}


def range_edges(n):
    """the ids around every range boundary of the window: k * R - 1 | k * R (and k * R + 4, which carries C)"""
    ids = {0, 4, n - 1}
    for k in range(1, 4):
        ids |= {k * R - 1, k * R, k * R + 4}
    return sorted(x for x in ids if 0 <= x < n)


def _hub(n):
    """Three starts over the same 1100 B-labelled b's (17 full chunks and one of 12: waves 0 and 1 of
    k_gd_large take a second chunk) plus 20 b's without B.  Every b goes to the ids around each range
    boundary and to 32 random ids of the window, so b's share c's across waves and ranges; the b's at
    sorted positions 0, 62, 63, 64 and last (with and without the b predicate) have no relationship, so
    that positions 63 and 64 are empty too where a looped hub is its own first b.  Hub 2 has one
    self-loop and comes back to itself through another b, hub 3 has two self-loops."""
    g = _Build(n, 1)
    hubs = [g.new(7) for _ in range(3)]
    bs = g.many(HAS_B, 1100)
    nonb = g.many((1, 5), 20)
    empty = {bs[0], bs[62], bs[63], bs[64], bs[-1], nonb[-1]}
    edges = range_edges(n)
    for b in bs + nonb:
        if b in empty:
            continue
        for c in edges:
            g.rel(b, c)
        for c in g.rng.integers(0, n, 32):
            g.rel(b, int(c))
    for h in hubs:
        for b in bs + nonb:
            g.rel(h, b)
    g.rel(hubs[1], hubs[1])
    g.rel(bs[500], hubs[1])
    g.rel(hubs[2], hubs[2], times=2)
    g.dangling(hubs[0], bs[1], bs[2])
    g.marks = {"hubs": hubs, "bs": bs}
    return g.finish()


def _boundary(n):
    """Starts whose work is exactly 1023, 1024 and 1025 under every predicate set: one b with that many
    C-labelled c's.  Three more whose b also has 50 c's without C (the work counts what the c predicate
    leaves); and two with two b's over the same c's, 512 + 512 and 513 + 512 (the work is the sum over
    the b's, not the union), some relationships tripled (the work counts distinct c's)."""
    g = _Build(n, 2)
    pool = g.many(HAS_C, 1025)
    other = g.many(NO_C, 50)
    exact, mixed, two = [], [], []
    for k in (1023, 1024, 1025):
        for extra, into in (((), exact), (other, mixed)):
            a, b = g.new(HAS_A[k % 4]), g.new(HAS_B[k % 4])
            g.rel(a, b)
            for c in list(pool[:k]) + list(extra):
                g.rel(b, c, times=3 if c % 16 == 12 else 1)
            into.append(a)
    for k in (512, 513):
        a, b1, b2 = g.new(7), g.new(7), g.new(3)
        g.rel(a, b1, times=2)
        g.rel(a, b2)
        for c in pool[:k]:
            g.rel(b1, c)
        for c in pool[:512]:
            g.rel(b2, c)
        two.append(a)
    g.dangling(exact[0], g.new(7), pool[0])
    g.marks = {"exact": exact, "mixed": mixed, "two": two}
    return g.finish()


CHUNK_SIZES = (63, 64, 65, 128, 129)


def _chunks(n):
    """Starts with 63, 64, 65, 128 and 129 distinct B-labelled b's; the b's at sorted positions 0, 63, 64
    and last have no ok target at all (no relationship, or one to an id that is no node), those at
    positions 1 and 62 only targets without C (empty under the c predicate alone)."""
    g = _Build(n, 3)
    cs, xs = g.many(HAS_C, 8), g.many(NO_C, 4)
    none = g.new(7, node=False)
    starts = []
    for nb in CHUNK_SIZES:
        a = g.new(HAS_A[nb % 4])
        bs = g.many(HAS_B, nb)
        for i, b in enumerate(bs):
            g.rel(a, b, times=2 if i % 5 == 0 else 1)
            if i in (0, 63, 64, nb - 1):
                if i in (63, nb - 1):
                    g.rel(b, none)
            elif i in (1, 62):
                g.rel(b, xs[i % 4])
            else:
                g.rel(b, cs[i % 8])
                g.rel(b, cs[(3 * i + 1) % 8])
                if i % 7 == 0:
                    g.rel(b, xs[i % 4])
        starts.append(a)
    g.dangling(starts[0], g.new(7), cs[0])
    g.marks = {"starts": starts}
    return g.finish()


def _loops(n):
    """Starts with 0, 1, 2 and 3 self-loops whose labels pass every predicate (ABC), fail b (AC), fail c
    (AB) or fail a (B), each with tripled relationships on both hops; a -> b -> a with 0, 1 and 2 loops
    at a; a start whose only b lacks B; a start whose only c lacks C."""
    g = _Build(n, 4)
    cs = g.many(HAS_C, 6)
    looped, back = [], []
    for code in (7, 5, 3, 2):
        for nl in range(4):
            a, b = g.new(code), g.new(7)
            g.rel(a, a, times=nl)
            g.rel(a, b, times=3)
            for c in cs[:3]:
                g.rel(b, c, times=3)
            looped.append(a)
    for nl in range(3):
        a, b = g.new(7), g.new(7)
        g.rel(a, b)
        g.rel(b, a)
        g.rel(b, cs[1])
        g.rel(a, a, times=nl)
        back.append(a)
    a, b = g.new(7), g.new(5)
    g.rel(a, b)
    g.rel(b, cs[0])
    a2, b2 = g.new(7), g.new(7)
    g.rel(a2, b2)
    g.rel(b2, g.new(3))
    g.dangling(looped[0], g.new(7), cs[0])
    g.marks = {"looped": looped, "back": back, "fails_b": [a], "fails_c": [a2]}
    return g.finish()


BUILDERS = {"hub": _hub, "boundary": _boundary, "chunks": _chunks, "loops": _loops}
CASES = [(g, n, p) for g in BUILDERS for n in WINDOWS for p in PREDICATES]
CASE_IDS = [f"{g}-{n}-{p}" for g, n, p in CASES]


@functools.lru_cache(maxsize=None)
def _built(name, n):
    return BUILDERS[name](n)


def graph(name, n):
    """(lo, n, src, dst, labels_of_node) of a builder; built once, never written"""
    return _built(name, n)[0]


def marks(name, n):
    """the relative ids a builder names for the shape tests, e.g. {"hubs": (..), "bs": (..)}"""
    return _built(name, n)[1]


def rel_types(m):
    return np.where(np.arange(m) % 3 == 2, "S", "R")


def masks(lo, n, labels_of_node, pred):
    """a_ok, b_ok, c_ok over the relative ids: a node, carrying the position's label"""
    out = []
    for want in PREDICATES[pred]:
        m = np.zeros(n, dtype=np.uint8)
        m[[v - lo for v, ls in labels_of_node.items() if want is None or want in ls]] = 1
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, n, pred):
    """(rows {relative a: (count(*), count(DISTINCT c))}, work {relative a: work}) of a case"""
    lo, n, src, dst, labels = graph(name, n)
    return reference(src - lo, dst - lo, *masks(lo, n, labels, pred))
