"""Shared by the tests of the fused undirected Expand counts (capsmi_undirected_count: csrc/k_undirected.hip,
csrc/k_und_part.hip and the UND form of k_rec_part in csrc/k_count.hip):
  MATCH (a)-[r]-(b)             RETURN count(*) | count(DISTINCT b) | count(DISTINCT a)
  MATCH (a)-[r1]-(b)-[r2]-(c)   RETURN count(*) | count(DISTINCT c) | count(DISTINCT a)      (r1 <> r2)
A numpy reference over arcs and the hand-built graphs of tests/test_gpu_undirected_edges.py; nothing here touches
the device, so tests/test_und_ref_cpu.py pins the reference to binding enumeration and checks every graph's stated
preconditions where no GPU exists.

An undirected hop is the outgoing branch over every relationship and the incoming branch over the relationships
with start <> end (RelationalPlanner.scala:126-136): relationship (s, t) is the arc s -> t and, when s != t, the
arc t -> s.  The 2-hop:
  count(*)          = sum_b b(b) inU(b) outU(b) - corr, inU(b) the a_ok arcs into b, outU(b) the c_ok arcs out of b,
                      corr the bindings with r1 = r2: [a(s) b(t) c(s)] + [a(t) b(s) c(t)] per non-loop, [a b c](s)
                      per loop
  count(DISTINCT c) : K(b) = the a_ok arcs into b capped at 2 (b_ok(b) only), x(b) the start of the only arc where
                      K(b) = 1; the arc b -> c extends a binding iff K(b) = 2, or K(b) = 1 and c != x(b)
  count(DISTINCT a) : the same with a_ok and c_ok exchanged (the arcs are symmetric)
Ids are relative to the domain [0, n); a relationship with an endpoint outside it has no node there and is dropped.
A mask is a boolean array over the domain, or None for a filter that covers it.
"""
import functools

import numpy as np

SLICE_BITS = 19
SLICE = 1 << SLICE_BITS   # ids per slice of the 2-D cell layout (part_common.h kSliceBits)
WALK_BLOCK = 1024 * 8     # arcs per workgroup share of k_und_2d (kBlock x kUnroll), also its smallest share
LOAD_MIN = 8192           # hop 2 pulls the from-slice's K2 words into LDS for a share of a cell this long (kLoadMin)
BUCKET = 1 << 16          # ids per bucket of the count(*) records, 16-bit LDS counters (k_count.hip kBits)
GRID_STRIDE = 16384 * 256  # threads of the streaming kernels' largest grid (k_undirected.hip grid_for)


# ---- the reference ------------------------------------------------------------------------------------------

def _mask(n, m):
    return np.ones(n, dtype=bool) if m is None else np.asarray(m).astype(bool)


def in_domain(n, src, dst):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keep = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    return src[keep], dst[keep]


def arcs(n, src, dst):
    """(start, end) of every arc: (s, t) per relationship inside the domain, and (t, s) where s != t"""
    s, t = in_domain(n, src, dst)
    nl = s != t
    return np.concatenate([s, t[nl]]), np.concatenate([t, s[nl]])


def one_hop(n, src, dst, a=None, b=None):
    """(arcs with a(start) and b(end), distinct ends, distinct starts)"""
    a, b = _mask(n, a), _mask(n, b)
    f, t = arcs(n, src, dst)
    k = a[f] & b[t]
    return int(k.sum()), int(len(np.unique(t[k]))), int(len(np.unique(f[k])))


def arcs_into(n, src, dst, a=None):
    """per id, the arcs into it whose start is a_ok (inU before b_ok)"""
    f, t = arcs(n, src, dst)
    return np.bincount(t[_mask(n, a)[f]], minlength=n)


def reach_state(n, src, dst, a=None, b=None):
    """(K, x): K(b) uncapped (0 where b_ok fails), x(b) the start of an a_ok arc into b (the only one where K = 1)"""
    a, b = _mask(n, a), _mask(n, b)
    f, t = arcs(n, src, dst)
    k = a[f] & b[t]
    K = np.bincount(t[k], minlength=n)
    x = np.full(n, -1, dtype=np.int64)
    x[t[k]] = f[k]
    return K, x


def _distinct_ends(n, src, dst, a, b, c, exclude):
    K, x = reach_state(n, src, dst, a, b)
    f, t = arcs(n, src, dst)  # the arcs b -> c: start b, end c
    one = K[f] == 1
    if exclude:
        one &= x[f] != t
    return int(len(np.unique(t[c[t] & ((K[f] >= 2) | one)])))


def two_hop(n, src, dst, a=None, b=None, c=None, exclude=True):
    """(count(*), count(DISTINCT c), count(DISTINCT a)).  exclude=False drops the c != x(b) test of the distinct
    counts: only for tests to show that their inputs tell a wrong K(b) = 1 path from a right one."""
    a, b, c = _mask(n, a), _mask(n, b), _mask(n, c)
    f, t = arcs(n, src, dst)
    inu = np.bincount(t[a[f]], minlength=n).astype(np.int64)
    outu = np.bincount(f[c[t]], minlength=n).astype(np.int64)
    s, d = in_domain(n, src, dst)
    nl = s != d
    corr = int((a[s] & b[d] & c[s] & nl).sum()) + int((a[d] & b[s] & c[d] & nl).sum()) + int((a[s] & b[s] & c[s] & ~nl).sum())
    rows = int((inu * outu)[b].sum()) - corr
    return rows, _distinct_ends(n, src, dst, a, b, c, exclude), _distinct_ends(n, src, dst, c, b, a, exclude)


def compact(n, src, dst, masks, id_sets=False):
    """The same graph over the ids it uses, relabelled 0 .. k-1 in id order: (k, src, dst, masks) with the masks
    gathered (id_sets: each mask is given as the array of its ok ids, so no n-sized array is needed)."""
    s, t = in_domain(n, src, dst)
    used = np.unique(np.concatenate([s, t]))
    out = []
    for m in masks:
        if m is None:
            out.append(None)
        elif id_sets:
            out.append(np.isin(used, np.asarray(m, dtype=np.int64)))
        else:
            out.append(np.asarray(m).astype(bool)[used])
    return int(len(used)), np.searchsorted(used, s), np.searchsorted(used, t), out


# ---- the walk order of the 2-D cell layout -------------------------------------------------------------------

def cell_sizes(n, src, dst):
    """cnt[j, i] = relationships inside the domain with target slice j and source slice i"""
    s, t = in_domain(n, src, dst)
    nt = (n + SLICE - 1) >> SLICE_BITS
    cnt = np.zeros((nt, nt), dtype=np.int64)
    np.add.at(cnt, (t >> SLICE_BITS, s >> SLICE_BITS), 1)
    return cnt


def item_offsets(cnt):
    """Start positions of the items of k_und_2d's walk (and the total): group q = the slice the arcs go into, its
    forwards cells (q, i) by source slice i, then its backwards cells (j, q) by target slice j.  A backwards cell
    keeps the positions of its self-loops."""
    nt = cnt.shape[0]
    sizes = []
    for q in range(nt):
        sizes += [cnt[q, i] for i in range(nt)] + [cnt[j, q] for j in range(nt)]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def item_of_arc(nt, start, end, back):
    """the item holding the arc start -> end: forwards (the relationship start -> end) or backwards (end -> start)"""
    return (end >> SLICE_BITS) * 2 * nt + (nt if back else 0) + (start >> SLICE_BITS)


def min_distance(off, va, vb):
    """the least distance of a position of item va from one of item vb"""
    lo, hi = min(va, vb), max(va, vb)
    return int(off[hi] - (off[lo + 1] - 1)) if lo != hi else 0


# ---- the graphs ----------------------------------------------------------------------------------------------

class Case:
    """A graph over [lo, lo + n), ids relative to lo, with its three filters.  sets: the filters are arrays of ok
    ids (a domain too large for host masks) and the reference runs on the compacted graph."""

    def __init__(self, name, n, src, dst, a=None, b=None, c=None, lo=0, sets=False, **notes):
        self.name, self.n, self.lo, self.sets = name, int(n), int(lo), sets
        self.src = np.ascontiguousarray(src, dtype=np.int64)
        self.dst = np.ascontiguousarray(dst, dtype=np.int64)
        self.masks = (a, b, c)
        self.notes = notes
        self._memo = {}

    @property
    def full(self):
        return all(m is None for m in self.masks)

    def ok_ids(self, which):
        """the ok ids of filter `which` (0 a, 1 b, 2 c), relative to lo"""
        m = self.masks[which]
        if m is None:
            return np.arange(self.n, dtype=np.int64)
        return np.asarray(m, dtype=np.int64) if self.sets else np.nonzero(m)[0].astype(np.int64)

    def dense(self):
        """(n, src, dst, (a, b, c)) for the reference: the graph itself, or its compacted form"""
        if "dense" not in self._memo:
            if self.sets:
                k, s, t, ms = compact(self.n, self.src, self.dst, self.masks, id_sets=True)
                self._memo["dense"] = (k, s, t, tuple(ms))
            else:
                s, t = in_domain(self.n, self.src, self.dst)
                self._memo["dense"] = (self.n, s, t, self.masks)
        return self._memo["dense"]

    def two_hop(self, exclude=True):
        key = ("two", exclude)
        if key not in self._memo:
            n, s, t, (a, b, c) = self.dense()
            self._memo[key] = two_hop(n, s, t, a, b, c, exclude=exclude)
        return self._memo[key]

    def one_hop(self):
        if "one" not in self._memo:
            n, s, t, (a, b, _) = self.dense()
            self._memo["one"] = one_hop(n, s, t, a, b)
        return self._memo["one"]

    def expected(self, hops, kind):
        return (self.one_hop() if hops == 1 else self.two_hop())[kind]


def _shuffled(rng, src, dst):
    p = rng.permutation(len(src))
    return np.asarray(src, dtype=np.int64)[p], np.asarray(dst, dtype=np.int64)[p]


THREE_SLICE_HUBS = (0, 31, 32, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE, 2 * SLICE + 76)


def three_slices(full=False):
    """2 * 2^19 + 77 ids (three slices, the last one and the last bitmap word ragged), about 200k relationships:
    hubs at the slice edges, 10 % reciprocal copies, parallel duplicates, self-loops (on the hubs too), and so few
    relationships per id that most middles have K(b) = 1."""
    rng = np.random.default_rng(5)
    n, m0 = 2 * SLICE + 77, 178_000
    hubs = np.array(THREE_SLICE_HUBS, dtype=np.int64)
    src, dst = rng.integers(0, n, m0), rng.integers(0, n, m0)
    src[:15_000] = hubs[rng.integers(0, len(hubs), 15_000)]
    dst[15_000:30_000] = hubs[rng.integers(0, len(hubs), 15_000)]
    loops = np.concatenate([rng.integers(0, n, 400), np.repeat(hubs, 20)])
    rec = rng.choice(m0, 20_000, replace=False)
    par = rng.choice(m0, 600, replace=False)
    s, t = _shuffled(rng, np.concatenate([src, loops, dst[rec], src[par]]), np.concatenate([dst, loops, src[rec], dst[par]]))
    if full:
        return Case("three_slices_full", n, s, t, hubs=hubs)
    return Case("three_slices", n, s, t, rng.random(n) < 0.7, rng.random(n) < 0.8, rng.random(n) < 0.75, hubs=hubs)


KB_PLANTED = 64


def kb_across_workgroups(full=False):
    """Three slices (3 * 2^19 - 51 ids).  Every one of the nine cells holds more than 8192 filler relationships, so two
    arcs in items of one group that are not neighbours lie more than a workgroup's share apart.  Planted in slice 0,
    and mirrored into slices 1 and 2 (slice + r, so every group has them), KB_PLANTED times each, all kinds within
    one bitmap word:
      two    b with exactly two a_ok arcs, s0 -> b forwards from b's own slice and t2 -> b backwards from slice + 2
             (the relationship b -> t2): K(b) = 2 only through the flush's atomicOr across workgroups; s0 and t2 have
             no other relationship, so each is an end only if b -> s0 / b -> t2 extend
      one    b with one relationship, to x in slice + 2 (either direction): K(b) = 1, x(b) = x, and x, a c_ok
             candidate, must not be counted
      one_y  b with one a_ok arc (from x) and arcs from y1, y2 that are not a_ok: K(b) = 1 in the masked graph, where
             y1 and y2 are ends and x is not
      par    x -> b twice: K(b) = 2 from one neighbour, so x is an end
      rec    x -> b and b -> x: the arcs x -> b forwards and backwards, in items two apart
    notes: pairs = (start, end, back) of both arcs of every `two` and `rec`."""
    rng = np.random.default_rng(11)
    n = 3 * SLICE - 51
    src, dst, pairs, not_a = [], [], [], []
    for r in range(3):
        def nid(sl, off):
            return ((sl + r) % 3) * SLICE + off + 2048 * r
        for i in range(KB_PLANTED):
            o = 16 * i
            b, s0, t2 = nid(0, o), nid(0, o + 1), nid(2, o + 1)                      # two
            src += [s0, b]
            dst += [b, t2]
            pairs.append(((s0, b, False), (t2, b, True)))
            b, x = nid(0, o + 2), nid(2, o + 2)                                      # one
            src.append(x if i % 2 == 0 else b)
            dst.append(b if i % 2 == 0 else x)
            b, x, y1, y2 = nid(0, o + 3), nid(2, o + 3), nid(1, o + 3), nid(0, o + 4)  # one_y
            src += [x, y1, b]
            dst += [b, b, y2]
            not_a += [y1, y2]
            b, x = nid(0, o + 5), nid(2, o + 5)                                      # par
            src += [x, x]
            dst += [b, b]
            b, x = nid(0, o + 6), nid(2, o + 6)                                      # rec
            src += [x, b]
            dst += [b, x]
            pairs.append(((x, b, False), (x, b, True)))
    planted = np.unique(np.array(src + dst, dtype=np.int64))
    for j in range(3):
        for i in range(3):  # fillers: offsets clear of the planted ones (below 8192)
            k = 8200 + 13 * (3 * j + i)
            src += (i * SLICE + rng.integers(8192, SLICE - 64, k)).tolist()
            dst += (j * SLICE + rng.integers(8192, SLICE - 64, k)).tolist()
    s, t = _shuffled(rng, src, dst)
    notes = dict(pairs=pairs, planted=planted)
    if full:
        return Case("kb_wg_full", n, s, t, **notes)
    a, b, c = rng.random(n) < 0.85, rng.random(n) < 0.85, rng.random(n) < 0.85
    for m in (a, b, c):
        m[planted] = True
    a[np.array(not_a)] = False
    return Case("kb_wg", n, s, t, a, b, c, **notes)


def pull_threshold(m):
    """One non-empty cell pair: m relationships from slice 0 to slice 1 (2 * 2^19 - 19 ids), forwards the cell (1, 0)
    of group 1, backwards the same cell in group 0.  m = 8191 stays below hop 2's pull of the from-slice's K2 words,
    m = 8193 gives one workgroup a share of 8192, m = 50_000 is a hub cell.  About a third of the sources and targets
    have one relationship, the filters are partial: the middles of both from-slices have K = 0, 1 and 2."""
    rng = np.random.default_rng(100 + m % 97)
    n = 2 * SLICE - 19
    ps = np.unique(np.concatenate([[0, 31, 32, SLICE - 1], rng.integers(0, SLICE, m // 2)]))
    pt = np.unique(np.concatenate([[SLICE, SLICE + 33, n - 1], rng.integers(SLICE, n, m // 2)]))
    src, dst = ps[rng.integers(0, len(ps), m)], pt[rng.integers(0, len(pt), m)]
    k = min(len(ps), len(pt), m // 4)
    src[:k] = ps[:k]                    # every source once at least, a quarter of them against ...
    dst[k:2 * k] = pt[:k]               # ... and every target
    if m >= 40_000:  # a hub target and a hub source
        dst[2 * k: 2 * k + 20_000] = SLICE + 7
        src[2 * k + 20_000: 2 * k + 25_000] = 5
    s, t = _shuffled(rng, src, dst)
    return Case(f"pull_{m}", n, s, t, rng.random(n) < 0.6, rng.random(n) < 0.8, rng.random(n) < 0.7, cell=(1, 0), m=m)


ODD_CELL_SIZES = ((1, 3, 8191), (5, 11, 7), (8193, 9, 1))


def odd_cells():
    """Three slices with cells of odd sizes (cell (j, i): target slice j, source slice i, stored in that order): cells
    start at odd pair offsets, where the even-aligned first load of a cell begins in the cell before."""
    rng = np.random.default_rng(13)
    n = 3 * SLICE - 45
    src, dst = [], []
    for j, row in enumerate(ODD_CELL_SIZES):
        for i, k in enumerate(row):
            s = i * SLICE + rng.integers(0, 6000, k) * 80
            t = j * SLICE + rng.integers(0, 6000, k) * 80
            if i == j and k >= 3:
                t[:2] = s[:2]  # self-loops in the diagonal cells
            src += s.tolist()
            dst += t.tolist()
    s, t = _shuffled(rng, src, dst)
    return Case("odd_cells", n, s, t, rng.random(n) < 0.7, rng.random(n) < 0.8, rng.random(n) < 0.75)


def offset_domain():
    """A domain [lo, lo + n) far from 0, n = 2^19 + 70_003 (no multiple of 32 or 2^16; two slices, ten buckets), with
    relationships that leave it by the source, by the target and by both, above and below, next to the edges
    (ids -1 and n) and far away; their inner endpoints have few other relationships, so keeping one arc of a
    dropped relationship changes K."""
    rng = np.random.default_rng(31)
    lo, n, m = (1 << 33) + 12_345, SLICE + 70_003, 150_000
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    src[:300] = dst[:300]                                   # self-loops
    src[300:5300], dst[300:5300] = dst[5300:10300], src[5300:10300]  # reciprocal copies
    dst[10_300:14_300] = np.array([0, n - 1, SLICE - 1, SLICE])[rng.integers(0, 4, 4000)]
    out_hi = np.concatenate([[n, n + 1], n + rng.integers(0, 1 << 20, 98)])
    out_lo = np.concatenate([[-1, -2], -rng.integers(1, 1 << 20, 98)])
    inner = rng.integers(0, n, 100)
    xs = np.concatenate([src, out_hi, out_lo, inner, inner, out_hi, out_lo, out_hi, [n, -1]])
    xt = np.concatenate([dst, inner, inner, out_hi, out_lo, out_lo, out_hi, out_hi, [n, -1]])
    s, t = _shuffled(rng, xs, xt)
    return Case("offset", n, s, t, rng.random(n) < 0.8, rng.random(n) < 0.9, rng.random(n) < 0.85, lo=lo, leaving=702)


def above_2_26():
    """2^26 + 77 ids: above the 2-D cell layout and the record partition, so the library takes the streaming distinct
    form and the atomic count(*) by itself.  About 20k relationships over about 3000 ids spread over the domain,
    with ids in the first word and in the last, partial one, and four hubs.  The filters are id sets."""
    rng = np.random.default_rng(41)
    n = (1 << 26) + 77
    edge = np.array([0, 31, 32, (1 << 26) - 1, 1 << 26, (1 << 26) + 40, (1 << 26) + 64, (1 << 26) + 70, n - 2, n - 1],
                    dtype=np.int64)
    ids = np.unique(np.concatenate([edge, rng.integers(0, n, 2990)]))
    m = 14_000
    src, dst = ids[rng.integers(0, len(ids), m)], ids[rng.integers(0, len(ids), m)]
    hubs = np.array([n - 1, 1 << 26, 31, int(ids[len(ids) // 2])], dtype=np.int64)
    hs = np.repeat(hubs, 1500)
    ho = ids[rng.integers(0, len(ids), len(hs))]
    flip = rng.random(len(hs)) < 0.5
    loops = ids[rng.integers(0, len(ids), 60)]
    lone = np.setdiff1d(rng.integers(0, n, 220), ids)[:200]  # 100 pairs with one relationship: K = 1 decides them
    xs = np.concatenate([src, np.where(flip, hs, ho), loops, hubs, lone[:100]])
    xt = np.concatenate([dst, np.where(flip, ho, hs), loops, hubs, lone[100:]])
    ids = np.union1d(ids, lone)
    s, t = _shuffled(rng, xs, xt)
    spare = rng.integers(0, n, 500)  # ok ids no relationship uses
    sets = [np.unique(np.concatenate([ids[rng.random(len(ids)) < p], spare, edge[::2]])) for p in (0.7, 0.8, 0.75)]
    return Case("above_2_26", n, s, t, sets[0], sets[1], sets[2], sets=True, ids=ids, hubs=hubs)


# a_ok arcs into each hub as (relationships into it, relationships out of it): each side below 2^16, the sum above it
# for the even ids; the odd neighbours end at 65535 mod 65536, where a carry out of the low half finds 0xFFFF
WRAP_HUBS = {2000: (50_001, 50_000), 2001: (32_767, 32_768), 4000: (32_768, 32_768), 4001: (32_767, 32_768),
             65_534: (60_000, 60_000), 65_535: (65_535, 65_536), 131_070: (35_000, 35_001), 131_071: (32_768, 32_767)}


def count_wraps():
    """count(*) records: 2^18 ids (four buckets of 2^16), pairs (x even, x + 1) of hubs whose a_ok arcs, counted over
    both directions, pass 2^16 while the relationships into each and out of each stay below it (65_535, the last id
    of bucket 0, apart: 2^17 + 1 arcs); the odd ones hold 65535 mod 65536.  Unequal partial filters."""
    rng = np.random.default_rng(107)
    n = 1 << 18
    a, b, c = rng.random(n) < 0.9, rng.random(n) < 0.95, rng.random(n) < 0.8
    hubs = np.array(sorted(WRAP_HUBS), dtype=np.int64)
    b[hubs] = True
    a[hubs] = True
    nbr = np.setdiff1d(np.nonzero(a)[0], hubs)  # a_ok neighbours, never a hub
    src, dst = [], []
    for h, (kin, kout) in WRAP_HUBS.items():
        src += [nbr[rng.integers(0, len(nbr), kin)], np.full(kout, h, dtype=np.int64)]
        dst += [np.full(kin, h, dtype=np.int64), nbr[rng.integers(0, len(nbr), kout)]]
    rs, rt = rng.integers(0, n, 300_000), rng.integers(0, n, 300_000)
    rs[np.isin(rs, hubs)] += 10  # the hubs' counts stay as planted
    rt[np.isin(rt, hubs)] += 10
    rs[:200] = rt[:200]  # self-loops
    s, t = _shuffled(rng, np.concatenate(src + [rs]), np.concatenate(dst + [rt]))
    return Case("wraps", n, s, t, a, b, c, hubs=hubs)


def grid_stride():
    """16384 * 256 + 12_345 relationships over 100k ids: the streaming kernels' grid-stride loops take a second turn.
    The relationships of that turn have the last 10k ids to themselves, so every count, the distinct ones too,
    needs them (ids that the first turn reaches as well would be marked without it)."""
    rng = np.random.default_rng(53)
    n, m, head = 100_000, GRID_STRIDE + 12_345, 90_000
    src, dst = rng.integers(0, head, m), rng.integers(0, head, m)
    src[GRID_STRIDE:], dst[GRID_STRIDE:] = rng.integers(head, n, 12_345), rng.integers(head, n, 12_345)
    src[-3000:] = dst[-3000:]  # self-loops, in the second turn too
    return Case("grid_stride", n, src, dst, rng.random(n) < 0.7, rng.random(n) < 0.6, rng.random(n) < 0.8)


def degenerate():
    n = 100
    every = None
    e = np.zeros(0, dtype=np.int64)
    loops = np.array([3, 3, 40, 99, 0], dtype=np.int64)
    rng = np.random.default_rng(3)
    s, t = rng.integers(0, n, 60), rng.integers(0, n, 60)
    none, single = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    single[int(t[0])] = True
    return [Case("no_rels", n, e, e, every, every, every),
            Case("only_loops", n, loops, loops, every, every, every),
            Case("single_rel", n, [7], [64], every, every, every),
            Case("a_empty", n, s, t, none, every, every),
            Case("b_single", n, s, t, every, single, every)]


BUILDERS = {
    "three_slices": three_slices,
    "three_slices_full": functools.partial(three_slices, full=True),
    "kb_wg": kb_across_workgroups,
    "kb_wg_full": functools.partial(kb_across_workgroups, full=True),
    "pull_8191": functools.partial(pull_threshold, 8191),
    "pull_8193": functools.partial(pull_threshold, 8193),
    "pull_hub": functools.partial(pull_threshold, 50_000),
    "odd_cells": odd_cells,
    "offset": offset_domain,
    "wraps": count_wraps,
    "grid_stride": grid_stride,
    "above_2_26": above_2_26,
}
DEGENERATE = ("no_rels", "only_loops", "single_rel", "a_empty", "b_single")


@functools.lru_cache(maxsize=None)
def case(name):
    """the graph `name`, built once per process (its reference answers are kept with it)"""
    if name in DEGENERATE:
        return {c.name: c for c in degenerate()}[name]
    return BUILDERS[name]()


# ---- the preconditions the graphs state ----------------------------------------------------------------------

def _k_classes(K, ids):
    return set(np.minimum(K[ids], 2).tolist())


def check_preconditions(cs, num_cus=256):
    """Asserts what the graph `cs` is said to have (on the host: tests/test_und_ref_cpu.py; again with the device's
    CU count before the GPU runs).  num_cus bounds k_und_2d's grid: with 2 * rows <= 8192 * 4 * num_cus every
    workgroup's share is exactly WALK_BLOCK positions of the walk."""
    n, name = cs.n, cs.name
    dn, ds, dt, (a, b, c) = cs.dense()
    if name in ("three_slices", "three_slices_full", "kb_wg", "kb_wg_full", "pull_8191", "pull_8193", "pull_hub",
                "odd_cells", "offset"):
        plain, loose = cs.two_hop(), cs.two_hop(exclude=False)
        assert loose[1] != plain[1] and loose[2] != plain[2], name  # the K = 1 exclusion decides the distinct counts
    if name.startswith("three_slices"):
        assert n == 2 * SLICE + 77 and n % 32 and (n + SLICE - 1) // SLICE == 3 and 190_000 <= len(ds) <= 210_000
        assert cs.full == name.endswith("full")
        loops = ds[ds == dt]
        assert len(loops) >= 400 and all((loops == h).sum() >= 20 for h in cs.notes["hubs"])
        deg = np.bincount(np.concatenate([ds, dt]), minlength=n)
        assert all(deg[h] > 1000 for h in cs.notes["hubs"])
        key = ds * n + dt
        assert np.isin(dt * n + ds, key)[ds != dt].sum() >= 0.15 * len(ds)  # both copies of 10 % of the relationships
        assert len(key) - len(np.unique(key)) >= 500                        # parallel duplicates
        assert (cell_sizes(n, ds, dt) > 0).all()
    if name.startswith("kb_wg"):
        cnt = cell_sizes(n, ds, dt)
        assert cnt.shape == (3, 3) and (cnt >= WALK_BLOCK).all() and n % 32
        assert 2 * len(cs.src) <= WALK_BLOCK * 4 * num_cus  # shares of exactly WALK_BLOCK positions
        off = item_offsets(cnt)
        assert len(cs.notes["pairs"]) == 2 * 3 * KB_PLANTED
        groups = set()
        for (f1, t1, k1), (f2, t2, k2) in cs.notes["pairs"]:
            assert t1 == t2
            v1, v2 = item_of_arc(3, f1, t1, k1), item_of_arc(3, f2, t2, k2)
            assert v1 // 6 == v2 // 6 == t1 >> SLICE_BITS  # one group: the slice of b
            assert min_distance(off, v1, v2) >= WALK_BLOCK  # so never in one workgroup
            groups.add(v1 // 6)
        assert groups == {0, 1, 2}
        K, x = reach_state(n, ds, dt, a, b)
        planted = cs.notes["planted"]
        assert (K[planted] == 1).sum() >= 3 * KB_PLANTED and (K[planted] >= 2).sum() >= 3 * 3 * KB_PLANTED
        one = planted[K[planted] == 1]
        assert len(set((one >> SLICE_BITS).tolist())) == 3
        assert ((x[one] >> SLICE_BITS) != (one >> SLICE_BITS)).sum() >= 3 * KB_PLANTED  # x(b) in another slice
        assert _mask(n, c)[x[one]].all()                                                # and a c_ok candidate
    if name.startswith("pull_"):
        cnt = cell_sizes(n, ds, dt)
        m = cs.notes["m"]
        assert cnt[1, 0] == m == len(cs.src) and cnt.sum() == m and cnt.shape == (2, 2)
        assert (m < LOAD_MIN) == (name == "pull_8191")
        K, _ = reach_state(n, ds, dt, a, b)
        Kc, _ = reach_state(n, ds, dt, c, b)  # count(DISTINCT a) walks from the other end
        for k in (K, Kc):
            assert _k_classes(k, np.unique(ds)) == {0, 1, 2} and _k_classes(k, np.unique(dt)) == {0, 1, 2}
        if name == "pull_hub":
            assert np.bincount(dt).max() >= 20_000 and np.bincount(ds).max() >= 5_000
    if name == "odd_cells":
        cnt = cell_sizes(n, ds, dt)
        assert cnt.tolist() == [list(r) for r in ODD_CELL_SIZES] and (cnt % 2 == 1).all()
        starts = np.concatenate([[0], np.cumsum(cnt.ravel())])[:-1]
        assert (starts % 2 == 1).sum() >= 4 and (ds == dt).sum() >= 2
    if name == "offset":
        assert cs.lo > 1 << 32 and n % 32 and n % BUCKET and n > SLICE
        s, t = cs.src, cs.dst
        so, to = (s < 0) | (s >= n), (t < 0) | (t >= n)
        assert (so & ~to).sum() >= 100 and (~so & to).sum() >= 100 and (so & to).sum() >= 100
        assert ((s < 0) & ~to).any() and ((s >= n) & ~to).any() and (~so & (t < 0)).any() and (~so & (t >= n)).any()
        assert (s == n).any() and (s == -1).any() and (t == n).any() and (t == -1).any()
        assert len(s) - len(ds) == cs.notes["leaving"]
        # keeping the inner arc of the dropped relationships would change every answer
        inner = np.where(so, t, s)[so ^ to]
        assert two_hop(n, np.concatenate([ds, inner]), np.concatenate([dt, inner]), a, b, c)[0] != cs.two_hop()[0]
    if name == "above_2_26":
        assert n > 1 << 26 and n % 32 and cs.sets
        ids = cs.notes["ids"]
        assert 2900 <= len(ids) <= 3300 and 19_000 <= len(cs.src) <= 21_000
        assert (ids >= (n // 32) * 32).sum() >= 3 and ids.min() == 0 and ids.max() == n - 1
        assert ids[-1] - ids[0] > 0.99 * n and np.diff(ids).max() < n // 100  # spread over the domain
        deg = np.bincount(np.concatenate([ds, dt]))
        assert (deg >= 1500).sum() >= 4
        plain, loose = cs.two_hop(), cs.two_hop(exclude=False)
        assert loose[1] != plain[1] and loose[2] != plain[2]
    if name == "wraps":
        inu = arcs_into(n, ds, dt, a)
        rin, rout = np.bincount(dt, minlength=n), np.bincount(ds, minlength=n)
        for h, (kin, kout) in WRAP_HUBS.items():
            assert inu[h] == kin + kout and b[h], h
            if h % 2:
                assert inu[h] % BUCKET == BUCKET - 1, h
        for h in (2000, 65_534, 131_070):  # more than 2^16 arcs enter, from fewer than 2^16 relationships either way
            assert inu[h] > BUCKET and rin[h] < BUCKET and rout[h] < BUCKET, h
        assert inu[4000] == BUCKET and inu[65_535] > BUCKET
        assert 65_535 % BUCKET == BUCKET - 1 and 131_071 % BUCKET == BUCKET - 1
        nl = ds != dt
        fwd, bwd = a[ds] & b[dt] & c[ds] & nl, a[dt] & b[ds] & c[dt] & nl
        assert (fwd & ~bwd).any() and (bwd & ~fwd).any()
        assert not (np.array_equal(a, b) or np.array_equal(b, c) or np.array_equal(a, c))
    if name == "grid_stride":
        assert len(cs.src) == GRID_STRIDE + 12_345 and n == 100_000
        assert (cs.src[GRID_STRIDE:] == cs.dst[GRID_STRIDE:]).any() and (cs.src[GRID_STRIDE:] != cs.dst[GRID_STRIDE:]).any()
        # without the second turn every answer is another one
        first = (n, cs.src[:GRID_STRIDE], cs.dst[:GRID_STRIDE], a, b)
        assert max(cs.src[:GRID_STRIDE].max(), cs.dst[:GRID_STRIDE].max()) < min(cs.src[GRID_STRIDE:].min(), cs.dst[GRID_STRIDE:].min())
        assert all(x != y for x, y in zip(one_hop(*first), cs.one_hop()))
        assert all(x != y for x, y in zip(two_hop(*first, c), cs.two_hop()))
    if name in DEGENERATE:
        assert {"no_rels": len(ds) == 0, "only_loops": len(ds) > 0 and (ds == dt).all(), "single_rel": len(ds) == 1,
                "a_empty": a is not None and not a.any(), "b_single": b is not None and b.sum() == 1}[name]
