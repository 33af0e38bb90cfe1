"""ORDER BY on the device (k_sort.hip k_order_keys, api.hip order_perm) against the pure-Python reference
sort of tests/edge_ref.py, at the null, NaN and Long edges (DESIGN.md "Value semantics at the edges").

The whole permutation is compared through a row-id column: multi-key order, DESC, nulls with arbitrary
words under them, every NaN bit pattern, the Long extremes under the DESC complement, nulls the device
made itself (outer join, withColumns), offset views, and the degenerate sizes.  collect()'s sort_array
uses the same keys (k_list.hip) and is checked on a Double column holding both NaN signs.  The reference
is independent of both the kernels and oracle/relational.py (whose orderBy the CPU suite checks against
the same reference on the same tables)."""
import numpy as np
import pytest

from edge_ref import F64, I64, NAN_BITS, f64_bits, hidden_words, order_cases, reference_order

pytestmark = pytest.mark.gpu

_CASES = {}


def _cases(session):
    if not _CASES:
        for name, cols, items in order_cases(session.dictionary):
            _CASES[name] = (cols, items)
    return _CASES


CASE_IDS = [f"hidden_{t}_{a}_{b}" for t in ("long", "double") for a in ("asc", "desc") for b in ("asc", "desc")] + \
    ["mixed_s_f_b", "mixed_k_b_f", "mixed_b_s_k"] + \
    [f"{c}_{o}" for c in ("edges_double", "edges_double_nullable", "edges_long") for o in ("asc", "desc")]


def _ids(t):
    return np.asarray(t.column("i").values, dtype=np.int64)


def _check(t, items, what=""):
    """order the device table `t` and compare the permutation with the reference over its exported rows"""
    cols = t.to_columns()
    want = reference_order(cols, items)
    base = _ids(t)
    np.testing.assert_array_equal(_ids(t.orderBy(*items)), base[np.array(want, dtype=np.int64)] if len(want) else base,
                                  err_msg=f"{what} {items}")


@pytest.mark.parametrize("case", CASE_IDS)
def test_order_by_edge_tables(session, case):
    cases = _cases(session)
    assert sorted(cases) == sorted(CASE_IDS)
    cols, items = cases[case]
    got = _ids(session.table(cols).orderBy(*items))
    np.testing.assert_array_equal(got, np.array(reference_order(cols, items), dtype=np.int64))


def test_order_by_nulls_made_by_an_outer_join(session):
    """The right side of an unmatched left_outer row is NULL with whatever the gather left under it."""
    from capsmi import ColumnData
    rng = np.random.default_rng(21)
    n = 10_007
    left = [ColumnData("a", I64, rng.integers(0, 60, n).astype(np.int64), None),
            ColumnData("lv", I64, rng.integers(0, 5, n).astype(np.int64), None),
            ColumnData("i", I64, np.arange(n, dtype=np.int64), None)]
    rk = np.arange(0, 60, 2, dtype=np.int64)  # the odd keys find no partner
    right = [ColumnData("b", I64, rk, None), ColumnData("rv", I64, (rk * 7919) % 5 - 2, None),
             ColumnData("rf", F64, np.where(rk % 3 == 0, f64_bits(NAN_BITS[1:2])[0], rk / 4.0), None)]
    j = session.table(left).join(session.table(right), "left_outer", ("a", "b"))
    assert j.size == n
    rv = j.column("rv")
    assert rv.valid is not None and 0 < int(np.sum(~rv.valid)) < n
    for items in ([("rv", "asc"), ("lv", "asc")], [("rv", "desc"), ("lv", "desc")], [("rf", "desc"), ("lv", "asc")],
                  [("rf", "asc"), ("rv", "desc"), ("lv", "asc")]):
        _check(j, items, "left_outer")


def test_order_by_nulls_made_by_with_columns(session):
    from capsmi import ColumnData
    from capsmi.expr import BinOp, Case, Col, Lit
    rng = np.random.default_rng(22)
    n = 10_007
    cols = [ColumnData("x", I64, rng.integers(-4, 5, n).astype(np.int64), rng.random(n) >= 0.25),
            ColumnData("y", F64, rng.choice(np.array([-1.0, 0.0, 2.5, np.inf]), n), rng.random(n) >= 0.25),
            ColumnData("z", I64, rng.integers(0, 7, n).astype(np.int64), None),
            ColumnData("i", I64, np.arange(n, dtype=np.int64), None)]
    t = session.table(cols).withColumns(
        (BinOp("*", Col("x"), Col("y")), "p"),  # NULL where either is; inf * 0 and -1 * inf add NaN and -inf
        (Case(((BinOp(">", Col("x"), Lit(0)), Col("z")),)), "c"))  # NULL unless x > 0
    p = t.column("p")
    assert p.valid is not None and np.isnan(p.values[p.valid]).any()
    for items in ([("p", "asc"), ("z", "desc")], [("p", "desc"), ("c", "asc"), ("z", "asc")], [("c", "desc"), ("p", "asc")]):
        _check(t, items, "withColumns")


def test_order_by_offset_view_zero_keys_and_tiny_tables(session):
    from capsmi import ColumnData
    rng = np.random.default_rng(23)
    n = 4100
    kv = np.where(rng.random(n) < 0.3, hidden_words(rng, n, I64), rng.integers(-2, 3, n))
    cols = [ColumnData("k", I64, kv.astype(np.int64), rng.random(n) >= 0.3),
            ColumnData("f", F64, rng.choice(f64_bits(NAN_BITS[:2] + (0, 1 << 63)), n), rng.random(n) >= 0.3),
            ColumnData("i", I64, np.arange(n, dtype=np.int64), None)]
    t = session.table(cols)
    view = t.skip(3)  # the columns of a skip are offset views of the parent's
    assert view.size == n - 3 and int(_ids(view)[0]) == 3
    _check(view, [("k", "asc"), ("f", "desc")], "skip(3)")
    _check(view.limit(4097), [("f", "asc"), ("k", "desc")], "skip(3).limit(4097)")
    np.testing.assert_array_equal(_ids(t.orderBy()), np.arange(n))  # no key: the identity
    for m in (0, 1, 2):
        small = session.table([ColumnData(c.name, c.type, c.values[:m], None if c.valid is None else c.valid[:m])
                               for c in cols])
        for items in ([("k", "desc")], [("f", "asc"), ("k", "asc")]):
            _check(small, items, f"n={m}")
    two = session.table([ColumnData("k", F64, f64_bits([NAN_BITS[1], 0x7FF0000000000000]), None),
                         ColumnData("i", I64, np.arange(2), None)])
    assert _ids(two.orderBy(("k", "asc"))).tolist() == [1, 0]  # +inf, then the sign-bit NaN
    assert _ids(two.orderBy(("k", "desc"))).tolist() == [0, 1]


def test_collect_lists_end_with_their_nans(session):
    """sort_array(collect_list) takes ORDER BY's keys: NaN of either sign is the greatest element."""
    from capsmi import ColumnData
    rng = np.random.default_rng(24)
    n = 5000
    g = rng.integers(0, 37, n).astype(np.int64)
    pool = np.concatenate([f64_bits(NAN_BITS), [-np.inf, -3.5, 0.0, 1.0, 2.0, np.inf]])
    v = rng.choice(pool, n)
    valid = rng.random(n) >= 0.2
    t = session.table([ColumnData("g", I64, g, None), ColumnData("v", F64, v, valid)])
    out = t.group(["g"], [("collect", "v", False, "vs")])
    keys = np.asarray(out.column("g").values)
    lists = out.column("vs").values
    assert sorted(keys.tolist()) == list(range(37))
    saw = set()
    for key, got in zip(keys, lists):
        sel = valid & (g == key)
        mine = v[sel]
        nn = np.sort(mine[~np.isnan(mine)])  # no NaN left: numpy's order is the number line
        got = np.asarray(got, dtype=np.float64)
        assert len(got) == len(mine)
        k = len(nn)
        np.testing.assert_array_equal(got[:k], nn)
        assert np.isnan(got[k:]).all(), f"group {key}: {got[k:]} after the numbers"
        # the NaNs keep their own bits (which of them comes first among equals is the input order)
        assert sorted(got[k:].view(np.uint64).tolist()) == sorted(mine[np.isnan(mine)].view(np.uint64).tolist())
        np.testing.assert_array_equal(got[k:].view(np.uint64), mine[np.isnan(mine)].view(np.uint64))
        saw |= set(got[k:].view(np.uint64).tolist())
    assert saw == set(NAN_BITS)


def test_collect_distinct_holds_one_nan_whatever_the_bits(session):
    """collect(DISTINCT) removes repeats among neighbours of the sorted group.  The sort ties every NaN, so
    NaNs of different bits interleave in input order; all of them are still one element (Spark's collect_set
    compares boxed Doubles, whose equals canonicalises NaN), while -0.0 and 0.0 stay two."""
    from capsmi import ColumnData
    from oracle.relational import NumpyBackend
    rng = np.random.default_rng(25)
    n = 5000
    g = rng.integers(0, 41, n).astype(np.int64)
    pool = np.concatenate([f64_bits(NAN_BITS), [-np.inf, -3.5, -0.0, 0.0, 1.0, np.inf]])
    v = rng.choice(pool, n)
    head = f64_bits([NAN_BITS[0], NAN_BITS[1], NAN_BITS[0], NAN_BITS[3], NAN_BITS[1]])
    g[:5], v[:5] = 40, head  # group 40 opens with NaN signs interleaved
    g[5:9], v[5:9] = 39, f64_bits([NAN_BITS[1], NAN_BITS[0], NAN_BITS[1], NAN_BITS[2]])  # and 39 holds NaN alone
    g[9:][g[9:] >= 39] = 0
    valid = rng.random(n) >= 0.2
    valid[:9] = True
    valid[g == 38] = False  # a group of nulls only: the empty list
    cols = [ColumnData("g", I64, g, None), ColumnData("v", F64, np.where(valid, v, hidden_words(rng, n, F64)), valid)]
    out = session.table(cols).group(["g"], [("collect", "v", True, "vs")])
    want = NumpyBackend(session.dictionary).table(cols).group(["g"], [("collect", "v", True, "vs")])
    checker = {int(k): xs for k, xs in zip(want.cols["g"].values, want.cols["vs"].values)}
    keys = np.asarray(out.column("g").values)
    assert sorted(keys.tolist()) == list(range(41))
    for key, got in zip(keys, out.column("vs").values):
        got = np.asarray(got, dtype=np.float64)
        mine = v[valid & (g == key)]
        numbers = sorted({x for x in mine[~np.isnan(mine)].view(np.uint64).tolist()},  # distinct words, -0.0 first
                         key=lambda w: (f64_bits([w])[0], -(w >> 63)))
        k = len(numbers)
        assert got[:k].view(np.uint64).tolist() == numbers, f"group {key}"
        assert len(got) == k + (1 if np.isnan(mine).any() else 0), f"group {key}: {got[k:]} after the numbers"
        assert np.isnan(got[k:]).all()
        ref = checker[int(key)]  # the pinned checker agrees, NaN matching NaN
        assert len(ref) == len(got) and ref[:k].view(np.uint64).tolist() == numbers
    by = dict(zip(keys.tolist(), out.column("vs").values))
    assert len(by[38]) == 0 and len(by[39]) == 1 and np.isnan(by[39][0])
