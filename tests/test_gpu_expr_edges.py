"""The expression interpreter (k_expr.hip) and the bitmap scan's inline range predicate (k_graph.hip
range_ok / compile_range_pred) at the null, NaN and Long edges -- DESIGN.md "Value semantics at the edges".

A seeded, typed generator builds 300 trees over every opcode; each is run through withColumns (and, when
Boolean, filter) and compared with the pinned checker (oracle/relational.py, whose edge rules
tests/test_relational_pins_cpu.py pins by literals): validity exact, Long / Boolean / String words exact,
Double words bit-exact (one IEEE operation per opcode: nothing to contract) except that any NaN matches any
NaN.  Hand-written cases pin the NaN truth table, Long wrap and Long-versus-Double comparison on the device
against literals.  The interpreter's limits (32 stack slots, 64 columns) are exercised at the limit and
refused one past it, on the host, before any launch."""
import numpy as np
import pytest

from edge_ref import (BOOL, F64, I64, INT64_MAX, INT64_MIN, NAN_TRUTH, OPS, STR, f64_pool_expr, hidden_words, i64_pool,
                      nan_truth_columns)

pytestmark = pytest.mark.gpu

N_ROWS = 2051  # not a multiple of the 256-lane block
STRINGS = ["", "a", "ab", "b", "zz", "s010"]
TYPES = (I64, F64, BOOL, STR)
SCALAR_PARAMS = {I64: (0, 5), F64: (1, 0.5), STR: (2, "ab"), BOOL: (3, True)}
PARAMS = [5, 0.5, "ab", True, [1, 2, None, 2 ** 53 + 1], [1, 0.5, float("nan")], None]
LIST_PARAMS = {I64: (4, (1, 2, None, 2 ** 53 + 1)), F64: (5, (1.0, 0.5, float("nan")))}


def _edge_tables(session):
    from capsmi import ColumnData
    from oracle.relational import NumpyBackend
    rng = np.random.default_rng(2051)
    n = N_ROWS
    session.dictionary.extend(STRINGS)
    codes = np.array([session.dictionary.encode(x) for x in STRINGS], dtype=np.int64)
    ipool = np.concatenate([i64_pool(), np.arange(-4, 5, dtype=np.int64)])
    fpool = f64_pool_expr()

    def col(name, ty, nullable):
        if ty == I64:
            v = rng.choice(ipool, n)
        elif ty == F64:
            v = rng.choice(fpool, n)
        elif ty == BOOL:
            v = rng.integers(0, 2, n).astype(np.int64)
        else:
            v = codes[rng.integers(0, len(codes), n)]
        if not nullable:
            return ColumnData(name, ty, v, None)
        valid = rng.random(n) >= 0.2
        return ColumnData(name, ty, np.where(valid, v, hidden_words(rng, n, ty)), valid)

    cols = [col("i0", I64, True), col("i1", I64, True), col("i2", I64, False),
            col("f0", F64, True), col("f1", F64, True), col("f2", F64, False),
            col("b0", BOOL, True), col("b1", BOOL, False), col("s0", STR, True), col("s1", STR, False),
            ColumnData("i", I64, np.arange(n, dtype=np.int64), None)]
    return session.table(cols), NumpyBackend(session.dictionary).table(cols)


COLS = {I64: ("i0", "i1", "i2"), F64: ("f0", "f1", "f2"), BOOL: ("b0", "b1"), STR: ("s0", "s1")}


class Gen:
    """Typed random trees.  Every method returns (device tree, checker tree): they differ only where the
    device tree holds a Param, which the checker sees as the literal(s) it is bound to."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.ipool = [int(x) for x in i64_pool()] + [2, -3]
        self.fpool = [float(x) for x in f64_pool_expr()]

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def lit(self, ty):
        from capsmi.expr import Lit
        if ty == I64:
            e = Lit(self.pick(self.ipool))
        elif ty == F64:
            e = Lit(self.pick(self.fpool))
        elif ty == BOOL:
            e = Lit(bool(self.rng.integers(0, 2)))
        else:
            e = Lit(self.pick(STRINGS))
        return e, e

    def leaf(self, ty):
        from capsmi.expr import Col, Lit, Param
        r = self.rng.random()
        if r < 0.55:
            e = Col(self.pick(COLS[ty]))
            return e, e
        if r < 0.8:
            return self.lit(ty)
        if r < 0.9:
            e = Lit(None, ty)
            return e, e
        idx, value = SCALAR_PARAMS[ty]
        return Param(idx), Lit(value)

    def many(self, ty, d, lo, hi):
        pairs = [self.gen(ty, d) for _ in range(int(self.rng.integers(lo, hi + 1)))]
        return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)

    def numeric(self, d):
        return self.gen(I64 if self.rng.random() < 0.5 else F64, d)

    def gen(self, ty, d):
        from capsmi.expr import Ands, BinOp, Case, Coalesce, In, IsNotNull, IsNull, Lit, Neg, Not, Ors, Param
        if d <= 0 or self.rng.random() < 0.2:
            return self.leaf(ty)
        r = self.rng.random()
        if r < 0.12:  # any type: Coalesce of operands of one type
            a, b = self.many(ty, d - 1, 1, 3)
            return Coalesce(a), Coalesce(b)
        if r < 0.24:  # any type: Case with values of one type, with or without a default
            alts = [(self.gen(BOOL, d - 1), self.gen(ty, d - 1)) for _ in range(int(self.rng.integers(1, 3)))]
            dflt = self.gen(ty, d - 1) if self.rng.random() < 0.6 else (None, None)
            return (Case(tuple((p[0], v[0]) for p, v in alts), dflt[0]),
                    Case(tuple((p[1], v[1]) for p, v in alts), dflt[1]))
        if ty == STR:
            return self.leaf(ty)
        if ty == I64:
            if r < 0.34:
                a = self.gen(I64, d - 1)
                return Neg(a[0]), Neg(a[1])
            a = self.gen(I64, d - 1)
            if r < 0.7:
                op = self.pick(("+", "-", "*"))
                b = self.gen(I64, d - 1)
            else:
                op = self.pick(("&", "|", "<<", ">>>"))
                if op in ("<<", ">>>") and self.rng.random() < 0.7:
                    e = Lit(self.pick((0, 63, 64, -1, 1, 5)))
                    b = (e, e)
                else:
                    b = self.gen(I64, d - 1)
            return BinOp(op, a[0], b[0]), BinOp(op, a[1], b[1])
        if ty == F64:
            if r < 0.34:
                a = self.gen(F64, d - 1)
                return Neg(a[0]), Neg(a[1])
            op = self.pick(("+", "-", "*"))
            a, b = self.gen(F64, d - 1), self.numeric(d - 1)  # at least one Double operand
            if self.rng.random() < 0.5:
                a, b = b, a
            return BinOp(op, a[0], b[0]), BinOp(op, a[1], b[1])
        # BOOL
        if r < 0.5:
            op = self.pick(OPS)
            if self.rng.random() < 0.6:
                a, b = self.numeric(d - 1), self.numeric(d - 1)  # Long / Double in any mix
            else:
                t = self.pick(TYPES)
                a, b = self.gen(t, d - 1), self.gen(t, d - 1)
            return BinOp(op, a[0], b[0]), BinOp(op, a[1], b[1])
        if r < 0.58:
            a = self.gen(BOOL, d - 1)
            return Not(a[0]), Not(a[1])
        if r < 0.74:
            a, b = self.many(BOOL, d - 1, 1, 4)
            return (Ands(a), Ands(b)) if self.rng.random() < 0.5 else (Ors(a), Ors(b))
        if r < 0.84:
            a = self.gen(self.pick(TYPES), d - 1)
            return (IsNull(a[0]), IsNull(a[1])) if self.rng.random() < 0.5 else (IsNotNull(a[0]), IsNotNull(a[1]))
        t = self.pick(TYPES)  # In: 0-5 elements, a null among them now and then, Long / Double mixed
        x = self.gen(t, d - 1)
        dev, chk = [], []
        for _ in range(int(self.rng.integers(0, 6))):
            q = self.rng.random()
            if q < 0.15:
                e = Lit(None, t) if self.rng.random() < 0.5 else Lit(None)
                dev.append(e)
                chk.append(e)
            elif q < 0.3 and t in LIST_PARAMS and len(dev) < 3:  # a list parameter stands for its values
                idx, values = LIST_PARAMS[t]
                dev.append(Param(idx))
                chk.extend(Lit(v, t) if v is None else Lit(v) for v in values)
            else:
                et = t if t not in (I64, F64) or self.rng.random() < 0.6 else (F64 if t == I64 else I64)
                e = self.lit(et) if self.rng.random() < 0.7 else self.gen(et, min(d - 1, 1))
                dev.append(e[0])
                chk.append(e[1])
        return In(x[0], tuple(dev)), In(x[1], tuple(chk))


def _mask(c, n):
    return np.ones(n, bool) if c.valid is None else np.asarray(c.valid, bool)


def _same_column(got, want, ty, what):
    """validity exact; words exact where valid, except that a Double NaN matches any NaN"""
    n = len(want.values)
    gm, wm = _mask(got, n), np.asarray(want.valid, bool)
    bad = np.nonzero(gm != wm)[0]
    assert len(bad) == 0, f"{what}: validity differs at rows {bad[:8]} (device {gm[bad[:8]]})"
    if ty == F64:
        g = np.asarray(got.values, dtype=np.float64)[gm]
        w = np.asarray(want.values, dtype=np.float64)[wm]
        both_nan = np.isnan(g) & np.isnan(w)
        bad = np.nonzero(~both_nan & (g.view(np.uint64) != w.view(np.uint64)))[0]
        assert len(bad) == 0, f"{what}: Doubles differ, device {g[bad[:8]]!r} checker {w[bad[:8]]!r}"
    else:
        g = np.asarray(got.values, dtype=np.int64)[gm]
        w = np.asarray(want.values).astype(np.int64)[wm]
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{what}: words differ, device {g[bad[:8]]} checker {w[bad[:8]]}"


SEED, TREES, PER_CALL = 20261019, 300, 20


def test_generated_trees_match_the_checker(session):
    g, o = _edge_tables(session)
    session.set_params(PARAMS)
    try:
        gen = Gen(SEED)
        trees = [(ty,) + gen.gen(ty, 4) for ty in (TYPES[k % 4] if k % 3 else BOOL for k in range(TREES))]
        seen_ops = set()
        for base in range(0, TREES, PER_CALL):
            chunk = trees[base:base + PER_CALL]
            names = [f"x{base + j}" for j in range(len(chunk))]
            gw = g.withColumns(*[(dev, nm) for (_, dev, _), nm in zip(chunk, names)])
            ow = o.withColumns(*[(chk, nm) for (_, _, chk), nm in zip(chunk, names)])
            gtypes = gw.columnType
            for (ty, dev, chk), nm in zip(chunk, names):
                what = f"seed {SEED} tree {nm}: {dev!r}"
                seen_ops.update(w for w in ("Coalesce", "Case", "Neg", "In(", "Param", "'>>>'", "'-'", "Ors", "IsNull")
                                if w in repr(dev))
                assert gtypes[nm] == ow.cols[nm].type == ty, what
                _same_column(gw.column(nm), ow.cols[nm], ty, what)
                if ty == BOOL:
                    kept = np.sort(np.asarray(g.filter(dev).column("i").values))
                    want = np.sort(o.filter(chk).cols["i"].values)
                    assert np.array_equal(kept, want), f"filter, {what}"
        assert len(seen_ops) == 9, seen_ops  # the generator reached every kind of node
    finally:
        session.set_params([])


def _tv(col):
    n = len(col.values)
    m = _mask(col, n)
    return [(bool(v) if ok else None) for v, ok in zip(col.values, m)]


def test_nan_truth_table_on_the_device(session):
    from capsmi import ColumnData
    from capsmi.expr import BinOp, Col, In, Lit
    cols = [ColumnData(*c) for c in nan_truth_columns()] + [ColumnData("i", I64, np.arange(len(NAN_TRUTH)), None)]
    t = session.table(cols)
    w = t.withColumns(*[(BinOp(op, Col("a"), Col("b")), f"r{j}") for j, op in enumerate(OPS)])
    for j, op in enumerate(OPS):
        want = [row[2][j] for row in NAN_TRUTH]
        assert _tv(w.column(f"r{j}")) == want, op
        kept = t.filter(BinOp(op, Col("a"), Col("b"))).column("i").values.tolist()
        assert kept == [r for r, x in enumerate(want) if x is True], op
    T, F, N = True, False, None
    nan = Lit(float("nan"))
    lits = t.withColumns((BinOp("=", Col("a"), nan), "e"), (BinOp("<", Col("a"), nan), "l"),
                         (BinOp(">", nan, Col("a")), "g"), (In(Col("a"), (Lit(1.0), nan)), "in"),
                         (In(Col("a"), (Lit(None, F64), nan)), "inn"), (In(Col("b"), (Lit(7), Lit(2))), "inl"))
    assert _tv(lits.column("e")) == [T, T, T, T, F, F, F, N, T, F]
    assert _tv(lits.column("l")) == [F, F, F, F, T, T, T, N, F, T]
    assert _tv(lits.column("g")) == [F, F, F, F, T, T, T, N, F, T]
    assert _tv(lits.column("in")) == [T, T, T, T, T, F, F, N, T, F]
    assert _tv(lits.column("inn")) == [T, T, T, T, N, N, N, N, T, N]
    assert _tv(lits.column("inl")) == [F, F, T, F, F, F, F, F, N, F]  # Long elements against a Double; NaN in none


def test_long_wrap_and_long_versus_double(session):
    from capsmi import ColumnData
    from capsmi.expr import BinOp, Col, Lit, Neg
    l = np.array([INT64_MAX, INT64_MIN, 2 ** 53 + 1, 5, -7], dtype=np.int64)
    d = np.array([2.0 ** 63, -(2.0 ** 63), 2.0 ** 53, 5.5, -7.0])
    t = session.table([ColumnData("l", I64, l, None), ColumnData("d", F64, d, None)])
    w = t.withColumns((BinOp("+", Col("l"), Lit(1)), "inc"), (BinOp("-", Col("l"), Lit(1)), "dec"),
                      (BinOp("*", Col("l"), Lit(-1)), "mul"), (Neg(Col("l")), "neg"),
                      (BinOp("=", Col("l"), Col("d")), "eq"), (BinOp("<", Col("l"), Col("d")), "lt"),
                      (BinOp(">=", Col("d"), Col("l")), "ge"), (BinOp("*", Col("l"), Col("l")), "sq"))
    for c in ("inc", "dec", "mul", "neg", "sq"):
        assert w.columnType[c] == I64 and _mask(w.column(c), len(l)).all()
    assert w.column("inc").values.tolist() == [INT64_MIN, INT64_MIN + 1, 2 ** 53 + 2, 6, -6]   # MAX + 1 wraps
    assert w.column("dec").values.tolist() == [INT64_MAX - 1, INT64_MAX, 2 ** 53, 4, -8]       # MIN - 1 wraps
    assert w.column("mul").values.tolist() == [-INT64_MAX, INT64_MIN, -(2 ** 53 + 1), -5, 7]   # MIN * -1 = MIN
    assert w.column("neg").values.tolist() == [-INT64_MAX, INT64_MIN, -(2 ** 53 + 1), -5, 7]   # -MIN = MIN
    # (2^63 - 1)^2 = 2^126 - 2^64 + 1, (-2^63)^2 = 2^126, (2^53 + 1)^2 = 2^106 + 2^54 + 1, all modulo 2^64
    assert w.column("sq").values.tolist() == [1, 0, 2 ** 54 + 1, 25, 49]
    # the Long side is cast to Double: 2^63 - 1 rounds to 2^63, 2^53 + 1 to 2^53
    assert _tv(w.column("eq")) == [True, True, True, False, True]
    assert _tv(w.column("lt")) == [False, False, False, True, False]
    assert _tv(w.column("ge")) == [True, True, True, True, True]


def test_stack_limit_is_reached_and_refused_one_past_it(session):
    """kMaxStack = 32: 32 operands on the stack evaluate; 33 are refused by validate_program on the host."""
    from capsmi import ColumnData, _lib
    from capsmi.expr import Ands, BinOp, Col
    rng = np.random.default_rng(32)
    n = 777
    bools, longs = [], []
    for j in range(33):
        v = (np.arange(n) % 35 != j).astype(np.int64)  # each column FALSE on rows of its own
        valid = np.arange(n) % 41 != j                 # and NULL on others
        bools.append(ColumnData(f"b{j}", BOOL, v, valid))
        longs.append(ColumnData(f"l{j}", I64, rng.integers(-(1 << 62), 1 << 62, n), None))
    tb, tl = session.table(bools), session.table(longs)

    def chain(k):  # l0 + (l1 + (... + l{k-1})): all k leaves are pushed before the first add
        e = Col(f"l{k - 1}")
        for j in range(k - 2, -1, -1):
            e = BinOp("+", Col(f"l{j}"), e)
        return e

    w = tb.withColumns((Ands(tuple(Col(f"b{j}") for j in range(32))), "all")).column("all")
    r = np.arange(n)
    any_false = (r % 35) < 32  # a FALSE operand decides, null or not elsewhere
    any_null = (r % 41) < 32
    # a row that is FALSE in column j is NULL there only if r % 41 == j too: then that operand is NULL, not FALSE
    false_seen = any_false & ~((r % 41) == (r % 35))
    want = [False if f else (None if nl else True) for f, nl in zip(false_seen, any_null)]
    assert _tv(w) == want
    assert {False, None, True} <= set(want)
    s = tl.withColumns((chain(32), "sum")).column("sum").values
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(s, np.sum([c.values for c in longs[:32]], axis=0, dtype=np.int64))
    for t, e in ((tb, Ands(tuple(Col(f"b{j}") for j in range(33)))), (tl, chain(33))):
        with pytest.raises(_lib.NotImplementedException, match="expression too deep"):
            t.withColumns((e, "x"))
        with pytest.raises(_lib.NotImplementedException, match="expression too deep"):
            t.filter(e if t is tb else BinOp(">", e, Col("l0")))


def test_column_limit_is_reached_and_refused_one_past_it(session):
    """kMaxCols = 64: column index 63 is read; index 64 of a 65-column table is refused on the host."""
    from capsmi import ColumnData, _lib
    from capsmi.expr import BinOp, Col, Lit
    n = 300
    cols = [ColumnData(f"c{j}", I64, np.arange(n, dtype=np.int64) * 65 + j, None) for j in range(65)]
    t = session.table(cols)
    got = t.withColumns((BinOp("+", Col("c63"), Lit(1)), "y")).column("y").values
    np.testing.assert_array_equal(got, np.arange(n, dtype=np.int64) * 65 + 64)
    assert t.filter(BinOp("=", Col("c63"), Lit(65 * 7 + 63))).column("c0").values.tolist() == [65 * 7]
    with pytest.raises(_lib.NotImplementedException, match="column >= 64"):
        t.withColumns((BinOp("+", Col("c64"), Lit(1)), "y"))
    with pytest.raises(_lib.NotImplementedException, match="column >= 64"):
        t.filter(BinOp("=", Col("c64"), Lit(64)))


# ---- the inline range predicate of the bitmap scan ------------------------------------------------------
N_IDS, ID_LO = 5000, 1000


def _node_columns():
    from capsmi import ColumnData
    rng = np.random.default_rng(5000)
    n = N_IDS
    ids = rng.permutation(np.arange(ID_LO, ID_LO + n)).astype(np.int64)
    pool = np.concatenate([i64_pool(), np.arange(0, 9, dtype=np.int64), [4, 5, 6]])
    cols = {"id": ids, "c": rng.choice(pool, n), "cn": rng.choice(pool, n)}
    for k in range(1, 5):
        cols[f"d{k}"] = rng.integers(0, 4, n).astype(np.int64)
    valid = {"cn": rng.random(n) >= 0.25, "d4": rng.random(n) >= 0.25}
    cd = [ColumnData(k, I64, np.where(valid[k], v, hidden_words(rng, n, I64)) if k in valid else v, valid.get(k))
          for k, v in cols.items()]
    return cd, cols, valid


def _range_predicates():
    """[(id, predicate, mask(cols, valid)), ...]; the masks are plain numpy over the host columns"""
    from capsmi.expr import Ands, BinOp, Col, Lit, Param
    c, cn = Col("c"), Col("cn")
    MIN, MAX = INT64_MIN, INT64_MAX
    out = [
        ("lt_min", BinOp("<", c, Lit(MIN)), lambda v, ok: v["c"] < MIN),
        ("le_min", BinOp("<=", c, Lit(MIN)), lambda v, ok: v["c"] <= MIN),
        ("ge_min", BinOp(">=", c, Lit(MIN)), lambda v, ok: v["c"] >= MIN),
        ("gt_max", BinOp(">", c, Lit(MAX)), lambda v, ok: v["c"] > MAX),
        ("ge_max", BinOp(">=", c, Lit(MAX)), lambda v, ok: v["c"] >= MAX),
        ("le_max", BinOp("<=", c, Lit(MAX)), lambda v, ok: v["c"] <= MAX),
        ("gt_min", BinOp(">", c, Lit(MIN)), lambda v, ok: v["c"] > MIN),
        ("lt_max", BinOp("<", c, Lit(MAX)), lambda v, ok: v["c"] < MAX),
        ("eq", BinOp("=", c, Lit(2 ** 53 + 1)), lambda v, ok: v["c"] == 2 ** 53 + 1),
        ("eq_min", BinOp("=", c, Lit(MIN)), lambda v, ok: v["c"] == MIN),
        ("lit_first_gt", BinOp(">", Lit(5), c), lambda v, ok: 5 > v["c"]),
        ("lit_first_le", BinOp("<=", Lit(5), c), lambda v, ok: 5 <= v["c"]),
        ("lit_first_lt_max", BinOp("<", Lit(MAX), c), lambda v, ok: MAX < v["c"]),
        ("lit_first_ge_min", BinOp(">=", Lit(MIN), c), lambda v, ok: MIN >= v["c"]),
        ("two_terms", Ands((BinOp(">=", c, Lit(-7)), BinOp("<", c, Lit(2 ** 31)))),
         lambda v, ok: (v["c"] >= -7) & (v["c"] < 2 ** 31)),
        ("three_terms", Ands((BinOp(">", c, Lit(0)), BinOp("<=", c, Lit(2 ** 62)), BinOp(">", Lit(2 ** 53 + 1), c))),
         lambda v, ok: (v["c"] > 0) & (v["c"] <= 2 ** 62) & (2 ** 53 + 1 > v["c"])),
        ("contradiction", Ands((BinOp(">", c, Lit(5)), BinOp("<", c, Lit(3)))),
         lambda v, ok: (v["c"] > 5) & (v["c"] < 3)),
        ("eq_and_range", Ands((BinOp("=", c, Lit(4)), BinOp(">=", c, Lit(4)), BinOp("<=", c, Lit(4)))),
         lambda v, ok: v["c"] == 4),
        ("four_columns", Ands((BinOp(">=", c, Lit(0)), BinOp("<", Col("d1"), Lit(3)), BinOp(">", Col("d2"), Lit(0)),
                               BinOp("=", Col("d3"), Lit(2)))),
         lambda v, ok: (v["c"] >= 0) & (v["d1"] < 3) & (v["d2"] > 0) & (v["d3"] == 2)),
        # a conjunct that is no column-against-literal comparison: not compiled, whatever the column count
        ("non_range_term", Ands((BinOp(">=", c, Lit(0)), BinOp("<", Col("d1"), Lit(3)), BinOp(">", Col("d2"), Lit(0)),
                               BinOp("<>", Lit(9), Lit(8)), BinOp("<=", Col("d3"), Lit(2)), BinOp(">=", cn, Lit(1)))),
         lambda v, ok: (v["c"] >= 0) & (v["d1"] < 3) & (v["d2"] > 0) & (v["d3"] <= 2) & ok["cn"] & (v["cn"] >= 1)),
        # five range terms on five columns, one more than kMaxRangeTerms = 4: falls back to the interpreter
        ("five_range_columns", Ands((BinOp(">=", c, Lit(0)), BinOp("<", Col("d1"), Lit(3)), BinOp(">", Col("d2"), Lit(0)),
                                     BinOp("<=", Col("d3"), Lit(2)), BinOp(">=", cn, Lit(1)))),
         lambda v, ok: (v["c"] >= 0) & (v["d1"] < 3) & (v["d2"] > 0) & (v["d3"] <= 2) & ok["cn"] & (v["cn"] >= 1)),
        ("nullable", BinOp("<=", cn, Lit(MAX)), lambda v, ok: ok["cn"]),  # NULL <= MAX is NULL: not kept
        ("nullable_two", Ands((BinOp(">", cn, Lit(-2)), BinOp("<", Col("d4"), Lit(2)))),
         lambda v, ok: ok["cn"] & (v["cn"] > -2) & ok["d4"] & (v["d4"] < 2)),
        ("param", BinOp(">", c, Param(0)), lambda v, ok: v["c"] > 5),
        ("param_two", Ands((BinOp(">=", c, Param(1)), BinOp("<", cn, Param(0)))),
         lambda v, ok: (v["c"] >= -1) & ok["cn"] & (v["cn"] < 5)),
    ]
    return out


RANGE_IDS = ["lt_min", "le_min", "ge_min", "gt_max", "ge_max", "le_max", "gt_min", "lt_max", "eq", "eq_min",
             "lit_first_gt", "lit_first_le", "lit_first_lt_max", "lit_first_ge_min", "two_terms", "three_terms",
             "contradiction", "eq_and_range", "four_columns", "non_range_term", "five_range_columns", "nullable",
             "nullable_two", "param", "param_two"]
_NODES = {}


@pytest.mark.parametrize("case", RANGE_IDS)
def test_inline_range_predicate_equals_the_interpreter_and_numpy(session, case):
    """The predicate as written compiles to a RangePred (at most 4 columns); wrapped as AND(p, TRUE) it does
    not, so the interpreter fills a flag column.  Both bitmaps and numpy must agree word for word.  The
    library's "expr_eval" timer counts interpreter launches, so the path each scan took is observed: none
    for the inline form (but for the two cases compile_range_pred must reject), one for the wrapped form."""
    import ctypes
    import torch
    from capsmi import _lib, graph
    from capsmi.expr import Ands, Lit
    if not _NODES:
        cd, cols, valid = _node_columns()
        _NODES.update(table=session.table(cd), cols=cols, valid=valid)
    preds = {name: (p, m) for name, p, m in _range_predicates()}
    assert sorted(preds) == sorted(RANGE_IDS)
    pred, mask = preds[case]
    cols, valid = _NODES["cols"], _NODES["valid"]
    keep = np.asarray(mask(cols, valid), dtype=bool) & np.ones(N_IDS, bool)
    wlo, whi = ID_LO - 37, ID_LO + N_IDS + 91
    nw = (whi - wlo + 31) // 32
    want = np.zeros(nw, dtype=np.uint32)
    x = cols["id"][keep] - wlo
    np.bitwise_or.at(want, x >> 5, (np.uint32(1) << (x & 31).astype(np.uint32)))
    launches, ms = ctypes.c_int64(), ctypes.c_double()

    def interpreter_launches():  # since the last call (reading resets the counter)
        _lib.call("capsmi_session_kernel_time", session.handle, b"expr_eval", ctypes.byref(launches), ctypes.byref(ms))
        return launches.value

    session.set_params([5, -1])
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        for form, p in (("inline", pred), ("interpreted", Ands((pred, Lit(True))))):
            interpreter_launches()
            bm = graph.NodeBitmap(session, wlo, whi).add_scan(_NODES["table"], "id", p)
            inline = form == "inline" and case not in ("non_range_term", "five_range_columns")
            assert interpreter_launches() == (0 if inline else 1), f"{case} {form}"
            w = torch.zeros(nw, dtype=torch.int32, device="cuda")
            bm.copy_words(0, nw, w.data_ptr(), to_bitmap=False)
            session.sync()
            np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), want, err_msg=f"{case} {form}")
            assert bm.stats() == (int(keep.sum()), True), f"{case} {form}"
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)
        session.set_params([])
    if case in ("lt_min", "gt_max", "contradiction", "lit_first_lt_max"):
        assert keep.sum() == 0
    elif case in ("ge_min", "le_max"):
        assert keep.all()
    else:
        assert 0 < keep.sum() < N_IDS
