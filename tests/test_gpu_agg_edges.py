"""The hash aggregates (k_hash.hip k_agg_*) at the edges -- DESIGN.md "Value semantics at the edges":
about as many groups as rows with keys that are multiples of 2^32 or sit at the Long extremes (long probe
chains, the table at its 2n capacity), one group holding nine rows in ten, Long sums that wrap, Double sums
whose every partial sum is exact (so the order of the atomic adds cannot matter), truncating Long averages,
min / max over Doubles with NaN of either sign (NaN is the greatest value), +-inf, all-NaN and all-null
groups, and count(DISTINCT) at the Long extremes.

Nothing is rounded: rows are matched by their group key and compared word for word -- Long words exactly,
Doubles bit for bit except that NaN matches NaN and that min / max may return either zero (Spark keeps
whichever it saw first).  Expected values come from the pinned checker (oracle/relational.py), from numpy
or from literals.  Group keys hold no NaN and no -0.0: keys compare by their words, which is out of scope."""
import math

import numpy as np
import pytest

from edge_ref import F64, I64, INT64_MAX, INT64_MIN, NAN_BITS, f64_bits, hidden_words

pytestmark = pytest.mark.gpu


def _pair(session, cols):
    from oracle.relational import NumpyBackend
    return session.table(cols), NumpyBackend(session.dictionary).table(cols)


def _host(col, n):
    valid = np.ones(n, bool) if col.valid is None else np.asarray(col.valid, bool)
    return np.asarray(col.values), valid


def _by_key(columns, by, n):
    """{key tuple (None under a null): row}"""
    keys = [_host(columns[k], n) for k in by]
    out = {}
    for r in range(n):
        key = tuple((int(v[r]) if ok[r] else None) for v, ok in keys)
        assert key not in out, f"group {key} twice"
        out[key] = r
    return out


def _same_groups(got, want, by, aggs):
    """device table `got` against checker table `want`, rows matched by the group key"""
    assert got.physicalColumns == want.physicalColumns
    n = want.size
    assert got.size == n
    gcols = {c.name: c for c in got.to_columns()}
    wcols = {c.name: c for c in want.to_columns()}
    grow, wrow = _by_key(gcols, by, n), _by_key(wcols, by, n)
    assert set(grow) == set(wrow)
    keys = sorted(wrow, key=repr)
    gi = np.array([grow[k] for k in keys], dtype=np.int64)
    wi = np.array([wrow[k] for k in keys], dtype=np.int64)
    for kind, _, _, name in aggs:
        assert gcols[name].type == wcols[name].type, name
        gv, gm = _host(gcols[name], n)
        wv, wm = _host(wcols[name], n)
        gv, gm, wv, wm = gv[gi], gm[gi], wv[wi], wm[wi]
        bad = np.nonzero(gm != wm)[0]
        assert len(bad) == 0, f"{name}: validity differs for groups {[keys[b] for b in bad[:5]]}"
        gv, wv = gv[gm], wv[wm]
        if wcols[name].type == F64:
            gv, wv = gv.astype(np.float64), wv.astype(np.float64)
            same = (gv.view(np.uint64) == wv.view(np.uint64)) | (np.isnan(gv) & np.isnan(wv))
            if kind in ("min", "max"):
                same |= (gv == 0.0) & (wv == 0.0)
        else:
            same = gv.astype(np.int64) == wv.astype(np.int64)
        bad = np.nonzero(~same)[0]
        shown = [(keys[np.nonzero(gm)[0][b]], gv[b], wv[b]) for b in bad[:5]]
        assert len(bad) == 0, f"{name}: (group, device, checker) {shown}"


LONG_AGGS = [("count_star", None, False, "n"), ("count", "v", False, "c"), ("sum", "v", False, "s"),
             ("min", "v", False, "mn"), ("max", "v", False, "mx"), ("avg", "w", False, "a")]


def test_about_as_many_groups_as_rows(session):
    """Keys that differ only above bit 32, at both Long extremes, negative and null, over two key columns:
    nearly every row its own group, so the table sits at its 2n capacity and probe chains are long."""
    from capsmi import ColumnData
    rng = np.random.default_rng(41)
    n = 50_000
    j = rng.integers(-(1 << 31), 1 << 31, n)
    k1 = (j << 32).astype(np.int64)
    k1[:6] = [INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, 0, -1]
    k1[6:3006] = k1[3006:6006]  # some groups of two and more
    v1 = rng.random(n) >= 0.1
    k2 = rng.choice(np.array([INT64_MIN, -(1 << 32), 0, 1 << 32, INT64_MAX], dtype=np.int64), n)
    v2 = rng.random(n) >= 0.1
    cols = [ColumnData("k1", I64, np.where(v1, k1, hidden_words(rng, n, I64)), v1),
            ColumnData("k2", I64, np.where(v2, k2, hidden_words(rng, n, I64)), v2),
            ColumnData("v", I64, rng.integers(-(1 << 40), 1 << 40, n), rng.random(n) >= 0.2),
            ColumnData("w", I64, rng.integers(-9, 10, n), rng.random(n) >= 0.2)]
    g, o = _pair(session, cols)
    want = o.group(["k1", "k2"], LONG_AGGS)
    assert want.size > 0.8 * n
    _same_groups(g.group(["k1", "k2"], LONG_AGGS), want, ["k1", "k2"], LONG_AGGS)
    one = o.group(["k1"], LONG_AGGS)
    _same_groups(g.group(["k1"], LONG_AGGS), one, ["k1"], LONG_AGGS)


def test_one_group_holds_nine_rows_in_ten(session):
    """Every atomic of 54 000 rows lands on one slot; the singletons sit beside it.  The Long sum of values
    near +-2^62 wraps many times over: numpy's int64 wraps the same way."""
    from capsmi import ColumnData
    rng = np.random.default_rng(42)
    n = 60_000
    k = np.where(rng.random(n) < 0.9, 7, np.arange(n) + 100).astype(np.int64)
    near = rng.choice(np.array([1 << 62, -(1 << 62)], dtype=np.int64), n) + rng.integers(-1000, 1000, n)
    cols = [ColumnData("k", I64, k, None), ColumnData("v", I64, near, rng.random(n) >= 0.1),
            ColumnData("w", I64, rng.integers(-9, 10, n), None)]
    g, o = _pair(session, cols)
    got = g.group(["k"], LONG_AGGS)
    _same_groups(got, o.group(["k"], LONG_AGGS), ["k"], LONG_AGGS)
    _same_groups(g.group([], LONG_AGGS), o.group([], LONG_AGGS), [], LONG_AGGS)
    valid = np.asarray(cols[1].valid, bool)
    with np.errstate(over="ignore"):
        hot = np.sum(near[valid & (k == 7)], dtype=np.int64)  # wraps
    exact = sum(int(x) for x in near[valid & (k == 7)])
    assert exact != int(hot) and (exact - int(hot)) % (1 << 64) == 0  # the sum did wrap
    row = _by_key({c.name: c for c in got.to_columns()}, ["k"], got.size)[(7,)]
    assert int(got.column("s").values[row]) == int(hot)


def test_double_sums_whose_partial_sums_are_exact(session):
    """Values j / 1024 with |j| < 2^20 and at most 2^13 rows a group: every partial sum is a multiple of
    2^-10 below 2^23, exactly representable, so sum and avg are bit-exact in any order of the adds."""
    from capsmi import ColumnData
    rng = np.random.default_rng(43)
    n = 30_000
    k = rng.integers(0, 6, n).astype(np.int64)  # ~5 000 rows a group
    assert np.bincount(k).max() <= 1 << 13
    f = rng.integers(-(1 << 20) + 1, 1 << 20, n) / 1024.0
    l = rng.integers(-50, 50, n).astype(np.int64)
    cols = [ColumnData("k", I64, k, rng.random(n) >= 0.05), ColumnData("f", F64, f, rng.random(n) >= 0.2),
            ColumnData("l", I64, l, rng.random(n) >= 0.2)]
    aggs = [("sum", "f", False, "sf"), ("avg", "f", False, "af"), ("min", "f", False, "mnf"), ("max", "f", False, "mxf"),
            ("avg", "l", False, "al"), ("sum", "l", False, "sl"), ("count", "f", False, "cf")]
    g, o = _pair(session, cols)
    _same_groups(g.group(["k"], aggs), o.group(["k"], aggs), ["k"], aggs)
    _same_groups(g.group([], aggs), o.group([], aggs), [], aggs)  # 24 000 rows: j sums below 2^35, still exact


def _decode(table, by, name):
    cols = {c.name: c for c in table.to_columns()}
    n = table.size
    v, ok = _host(cols[name], n)
    out = {}
    for key, r in _by_key(cols, by, n).items():
        x = v[r]
        out[key[0]] = None if not ok[r] else ("NaN" if isinstance(x, np.floating) and math.isnan(x) else x.item())
    return out


def test_long_average_truncates_toward_zero(session):
    """avg(..).cast(Long): -7 / 2 = -3.5 -> -3 (a cast truncates, it does not floor)."""
    from capsmi import ColumnData
    k = np.array([0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4], dtype=np.int64)
    v = np.array([-7, 0, -1, -2, 7, 0, 5, 9, -9, INT64_MAX, INT64_MIN], dtype=np.int64)
    valid = np.array([1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1], bool)
    g, o = _pair(session, [ColumnData("k", I64, k, None), ColumnData("v", I64, v, valid)])
    aggs = [("avg", "v", False, "a"), ("sum", "v", False, "s"), ("count", "v", False, "c")]
    got = g.group(["k"], aggs)
    assert _decode(got, ["k"], "a") == {0: -3, 1: -1, 2: 3, 3: None, 4: 0}
    assert _decode(got, ["k"], "s") == {0: -7, 1: -3, 2: 7, 3: None, 4: -1}
    assert _decode(got, ["k"], "c") == {0: 2, 1: 2, 2: 2, 3: 0, 4: 2}
    _same_groups(got, o.group(["k"], aggs), ["k"], aggs)


def test_min_max_over_doubles_nan_is_greatest(session):
    """The pinned table of tests/test_relational_pins_cpu.py on the device, against the same literals: max is
    NaN when any value is, min only when all are, whatever the NaN's sign bit; all-null groups give null."""
    from capsmi import ColumnData
    NAN, NEG_NAN, SNAN, ONES = f64_bits(NAN_BITS)
    inf = math.inf
    k = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 5, 5, 6, 6], dtype=np.int64)
    v = np.array([1.0, NEG_NAN, -inf, NAN, NEG_NAN, SNAN, 7.0, inf, -inf, 0.0, ONES, NEG_NAN, 5e-324, -1e300, NEG_NAN])
    valid = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 1, 1], bool)
    assert v.view(np.uint64)[1] == NAN_BITS[1] and v.view(np.uint64)[10] == NAN_BITS[3]
    g, o = _pair(session, [ColumnData("k", I64, k, None), ColumnData("v", F64, v, valid)])
    aggs = [("min", "v", False, "mn"), ("max", "v", False, "mx"), ("sum", "v", False, "s")]
    got = g.group(["k"], aggs)
    assert _decode(got, ["k"], "mn") == {0: -inf, 1: "NaN", 2: None, 3: -inf, 4: "NaN", 5: 5e-324, 6: -1e300}
    assert _decode(got, ["k"], "mx") == {0: "NaN", 1: "NaN", 2: None, 3: inf, 4: "NaN", 5: "NaN", 6: "NaN"}
    assert _decode(got, ["k"], "s") == {0: "NaN", 1: "NaN", 2: None, 3: "NaN", 4: "NaN", 5: "NaN", 6: "NaN"}  # inf + -inf
    _same_groups(got, o.group(["k"], aggs), ["k"], aggs)
    every = g.group([], aggs)
    assert math.isnan(every.column("mx").values[0]) and every.column("mn").values[0] == -inf


def test_min_max_over_the_double_edge_pool(session):
    from capsmi import ColumnData
    rng = np.random.default_rng(44)
    n = 30_000
    pool = np.concatenate([f64_bits(NAN_BITS), [np.inf, -np.inf, 1e300, -1e300, 5e-324, -5e-324, 1.0, -1.0, 2.5]])
    k = rng.integers(0, 400, n).astype(np.int64)
    # each group draws from a few pool values only: groups with and without NaN, of NaN alone, of one sign
    lo = (k * 7) % len(pool)
    v = pool[(lo + rng.integers(0, 1 + k % 4, n)) % len(pool)]
    valid = (rng.random(n) >= 0.2) & (k % 11 != 0)  # every 11th group is all null
    cols = [ColumnData("k", I64, k, None), ColumnData("v", F64, np.where(valid, v, hidden_words(rng, n, F64)), valid)]
    aggs = [("min", "v", False, "mn"), ("max", "v", False, "mx"), ("count", "v", False, "c")]
    g, o = _pair(session, cols)
    want = o.group(["k"], aggs)
    mn, mx = want.cols["mn"], want.cols["mx"]
    assert (~mn.valid).sum() >= 30 and np.isnan(mn.values[mn.valid]).sum() >= 10  # all-null and all-NaN groups
    assert 50 < np.isnan(mx.values[mx.valid]).sum() < 350
    _same_groups(g.group(["k"], aggs), want, ["k"], aggs)


def test_count_distinct_at_the_long_extremes(session):
    from capsmi import ColumnData
    rng = np.random.default_rng(45)
    n = 20_000
    ext = np.array([INT64_MIN, INT64_MIN + 1, -(1 << 32), -1, 0, 1, 1 << 32, INT64_MAX - 1, INT64_MAX], dtype=np.int64)
    k = rng.integers(0, 300, n).astype(np.int64)
    v = np.where(rng.random(n) < 0.7, rng.choice(ext, n), rng.integers(-3, 4, n) << 32)
    valid = rng.random(n) >= 0.15
    cols = [ColumnData("k", I64, k, None), ColumnData("v", I64, np.where(valid, v, hidden_words(rng, n, I64)), valid)]
    aggs = [("count", "v", True, "d"), ("count", "v", False, "c"), ("min", "v", False, "mn"), ("max", "v", False, "mx")]
    g, o = _pair(session, cols)
    got = g.group(["k"], aggs)
    _same_groups(got, o.group(["k"], aggs), ["k"], aggs)
    d = _decode(got, ["k"], "d")
    assert d == {key: len(set(v[valid & (k == key)].tolist())) for key in range(300)}  # plain Python sets
    _same_groups(g.group([], aggs), o.group([], aggs), [], aggs)
