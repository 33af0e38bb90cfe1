"""The two restatements of the transitive triangle's per-node counts in tests/tri_trans_ref.py against each other:
the dense closed form equals the enumeration of the bindings, for every role, and the three roles' counts have the
same sum (each binding has one source, one middle and one sink)."""
import numpy as np
import pytest

import tri_trans_ref as tt


@pytest.mark.parametrize("seed", range(8))
def test_closed_form_equals_the_enumeration(seed):
    n, src, dst = tt.random_multigraph(seed)
    want = tt.per_node_enumerate_all(n, src, dst)
    got = tt.per_node_dense_all(n, src, dst)
    for role in tt.ROLES:
        assert got[role].tolist() == want[role].tolist(), f"role {role}"
        assert tt.per_node_enumerate(n, src, dst, role).tolist() == want[role].tolist()
        assert tt.per_node_dense(n, src, dst, role).tolist() == want[role].tolist()
    totals = want.sum(axis=1)
    assert totals[0] == totals[1] == totals[2] == sum(1 for _ in tt.bindings(src, dst))
    assert got.astype(object).tolist() == tt.per_node_dense_all(n, src, dst, dtype=object).tolist()


def test_some_seed_has_every_kind_of_binding():
    """the seeds reach three, two and one distinct nodes per binding (else the comparison above shows little)"""
    kinds = set()
    for seed in range(8):
        _, src, dst = tt.random_multigraph(seed)
        for a, b, c in tt.bindings(src, dst):
            kinds.add((a == b, b == c, a == c))
    assert kinds == {(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                     (True, True, True)}


def test_roles_of_the_spellings():
    assert tt.roles_of((">", ">", "<")) == (tt.SOURCE, tt.MIDDLE, tt.SINK)
    assert tt.roles_of((">", ">", ">")) is None and tt.roles_of(("<", "<", "<")) is None
    seen = set()
    for d1 in "<>":
        for d2 in "<>":
            for d3 in "<>":
                r = tt.roles_of((d1, d2, d3))
                if r is not None:
                    assert sorted(r) == [0, 1, 2]
                    seen.add(r)
    assert len(seen) == 6  # the six mixed spellings are the six assignments of the roles to a, b, c


def test_a_spelling_counts_its_roles():
    """a mixed spelling's bindings per position are the transitive pattern's per role (relabelling)"""
    n, src, dst = tt.random_multigraph(3)
    want = tt.per_node_enumerate_all(n, src, dst)
    for dirs in (("<", ">", ">"), (">", "<", "<"), ("<", "<", ">")):
        got = tt.per_node_enumerate_all(n, src, dst, dirs=dirs)
        for p, role in enumerate(tt.roles_of(dirs)):
            assert got[p].tolist() == want[role].tolist()


def test_complete_digraph_closed_form():
    n = 12
    a, b = np.nonzero(~np.eye(n, dtype=bool))
    got = tt.per_node_dense_all(n, a, b)
    assert (got == (n - 1) * (n - 2)).all()
