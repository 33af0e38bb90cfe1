"""Without a GPU: the references of the undirected triangle's tests against each other -- the enumeration of the
eight-branch plan and the dense closed form (tests/tri_und_ref.py) -- and the library's declarations: the
CAPSMI_TRI_UND_COUNT knob and the four entry points."""
import numpy as np
import pytest

import tri_und_ref as tu


@pytest.mark.parametrize("seed", range(8))
def test_enumeration_equals_closed_form(seed):
    n, src, dst = tu.random_multigraph(seed)
    want = tu.per_node_enumerate_all(n, src, dst)
    assert want.tolist() == tu.per_node_dense_all(n, src, dst).tolist()
    assert want.tolist() == tu.per_node_dense_all(n, src, dst, dtype=object).tolist()
    assert want[0].tolist() == want[2].tolist()                   # the ends of the ExpandInto
    assert want[0].sum() == want[1].sum() == want[2].sum()        # every position sums to the count


def test_random_multigraphs_have_rows_of_every_kind():
    """taken together the eight graphs have triangles, looped pairs and nodes whose classes differ"""
    wants = [tu.per_node_enumerate_all(*tu.random_multigraph(seed)) for seed in range(8)]
    assert sum(int(w[0].sum() > 0) for w in wants) >= 6
    assert any(w[0].tolist() != w[1].tolist() for w in wants)


def test_middle_differs_from_the_ends_at_a_looped_corner():
    """x = 0 has a loop and a double pair with 1: end(0) = 3 s Q = 6, middle(0) = 2 s Q = 4, and 1 gets the rest"""
    src = np.array([0, 0, 0], dtype=np.int64)
    dst = np.array([0, 1, 1], dtype=np.int64)
    want = tu.per_node_enumerate_all(2, src, dst)
    assert want.tolist() == [[6, 2], [4, 4], [6, 2]]
    assert want.tolist() == tu.per_node_dense_all(2, src, dst).tolist()
    assert want[0].tolist() == want[2].tolist() and want[1].tolist() != want[0].tolist()
    assert want[0].sum() == want[1].sum() == 8


def test_lone_loop_beside_a_double_relationship():
    """x -> x, x -> y, y -> x: s = 1, U = 2, Q = 2.  r1 a loop: s Q = 2; r2 a loop: Q s = 2; r3 a loop, bound by both
    joins of the ExpandInto: 2 s Q = 4.  4 s Q = 8 rows."""
    src = np.array([0, 0, 1], dtype=np.int64)
    dst = np.array([0, 1, 0], dtype=np.int64)
    rows = sorted(tu.bindings(src, dst))
    assert len(rows) == 8
    assert rows.count((0, 0, 1)) == 2 and rows.count((1, 0, 0)) == 2 and rows.count((0, 1, 0)) == 4
    want = tu.per_node_enumerate_all(2, src, dst)
    assert want.tolist() == tu.per_node_dense_all(2, src, dst).tolist()
    assert int(want[0].sum()) == 8


def test_simple_triangle():
    """one relationship per pair, any directions: 6 rows, 2 per corner at every position"""
    src = np.array([0, 2, 2], dtype=np.int64)
    dst = np.array([1, 1, 0], dtype=np.int64)
    assert tu.per_node_enumerate_all(3, src, dst).tolist() == [[2, 2, 2]] * 3


def test_loops_only():
    v = np.repeat(np.arange(5, dtype=np.int64), np.arange(5))
    assert tu.per_node_enumerate_all(5, v, v).tolist() == [[0, 0, 0, 12, 48]] * 3


def test_node_filters():
    n, src, dst = tu.random_multigraph(3)
    mask = np.arange(n) % 3 != 0
    keep = mask[src] & mask[dst]
    assert tu.per_node_enumerate_all(n, src, dst, ok=(mask, mask, mask)).tolist() == \
        tu.per_node_dense_all(n, src[keep], dst[keep]).tolist()


def test_count_knob_is_checked():
    from capsmi import _lib
    lib = _lib.load()
    for v in (b"hash", b"walk", None):
        assert lib.capsmi_config_check(b"CAPSMI_TRI_UND_COUNT", v) == _lib.OK, v
    assert lib.capsmi_config_check(b"CAPSMI_TRI_UND_COUNT", b"both") == _lib.ERR_ILLEGAL_ARGUMENT


def test_entry_points_are_exported():
    from capsmi import _lib, graph
    lib = _lib.load()
    for name in ("capsmi_trigraph_count_undirected", "capsmi_trigraph_count_undirected_by_node",
                 "capsmi_triangle_count_undirected", "capsmi_triangle_count_undirected_by_node"):
        assert hasattr(lib, name), name
    assert (graph.TRI_UND_END, graph.TRI_UND_MIDDLE) == (tu.END, tu.MIDDLE) == (0, 1)
    assert callable(graph.TriGraph.count_undirected) and callable(graph.TriGraph.count_undirected_by_node)
    assert callable(graph.triangle_count_undirected) and callable(graph.triangle_count_undirected_by_node)
