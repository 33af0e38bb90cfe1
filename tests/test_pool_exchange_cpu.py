"""Without a GPU: the CAPSMI_HOP2_EXCHANGE knob is checked, and the graphs of test_gpu_pool_exchange.py hold what
their tests say of them -- the properties are asserted here on the numpy restatement's words (pinned to the CPU
oracle in test_pool_hop2_cpu.py), so that on the GPU a failure is the kernel's."""
import numpy as np
import pytest

import pool_split_ref as P
import test_gpu_pool_exchange as X

S, N = P.S, P.N


def test_exchange_knob_is_checked():
    from capsmi import _lib
    lib = _lib.load()
    for v in (b"on", b"off", None):
        assert lib.capsmi_config_check(b"CAPSMI_HOP2_EXCHANGE", v) == _lib.OK, v
    assert lib.capsmi_config_check(b"CAPSMI_HOP2_EXCHANGE", b"1") == _lib.ERR_ILLEGAL_ARGUMENT
    assert "configuration" in _lib.last_error()


@pytest.mark.parametrize("name,tiles", [("one_pair", X.T2), ("partial_c", X.T2), ("partial_b_loops", X.T2), ("span", X.T3)])
def test_shapes_one_table(name, tiles):
    g = X._case(name)
    assert g["parts"] == 1 and len(g["src"]) == len(g["dst"]) == tiles * X.TILE
    assert tiles // 16 >= 2 and tiles > 17 * (tiles // 16)  # several hop blocks, 17 or more chunks for each
    assert len(g["want"]) == X.NW


@pytest.mark.parametrize("name", ["windows", "last_slice", "last_slice_partial_c"])
def test_shapes_many_tables(name):
    g = X._case(name)
    rows = X.PARTS * X.PART_ROWS
    assert g["parts"] == X.PARTS and len(g["src"]) == len(g["dst"]) == rows and X.PART_ROWS < X.TILE
    blocks = rows // (16 * X.TILE)
    assert blocks >= 2 and X.PARTS // blocks >= 16 + 64  # every block enters 64 chunks after its waves' first 16
    assert len(set(g["dst"] >> 19)) == 1                 # one chunk per table, all in one slice
    assert len(g["want"]) == X.NW


def test_graph_properties():
    w = X._case("one_pair")["want"]
    i = X._case("one_pair")["info"]
    assert X._bit(w, i["a"]).all() and not X._bit(w, i["b"]).any()

    g = X._case("partial_c")
    c = P.words(g["c"].astype(bool))
    full = X.R.hop2_words(N, g["src"], g["dst"])
    assert (full & ~c).any() and not (g["want"] & ~c).any()           # excluded targets qualify
    assert ((full & ~c) != 0)[(g["want"] != 0)].any()                   # and share words with included ones

    g = X._case("partial_b_loops")
    w, i, b = g["want"], g["info"], g["b"].astype(bool)
    assert not X._bit(w, i["one"]).any() and not X._bit(w, i["none_in"]).any()
    np.testing.assert_array_equal(X._bit(w, i["two"]).astype(bool), b[i["two"]])
    assert X._bit(w, i["one_in"][b[i["one_in"]]]).all()
    assert b[i["two"]].any() and not b[i["two"]].all()

    g = X._case("windows")
    w = g["want"]
    assert (w[g["info"]["words"]] == 0xFFFFFFFF).all() and np.count_nonzero(w) == 4
    rel = g["info"]["words"] - (S >> 5)
    assert list(rel) == [0, 5 * X.WIN, 6 * X.WIN - 1, (S >> 5) - 1]

    for name in ("last_slice", "last_slice_partial_c"):
        w = X._case(name)["want"]
        assert w[3 * (S >> 5):].any() and not w[:3 * (S >> 5)].any()
    assert (N - 3 * S) // 32 < X.WIN and N % (1 << 19)

    g = X._case("span")
    w = g["want"]
    assert all(w[j * (S >> 5):(j + 1) * (S >> 5)].any() for j in range(3))
    j = g["dst"] >> 19
    assert (j[8 * X.TILE:] == 2).all() and not (j[2 * X.TILE:] == 1).any() and (j == 0).any() and (j == 1).any()
