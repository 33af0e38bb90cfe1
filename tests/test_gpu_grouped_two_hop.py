"""The grouped 2-hop (csrc/k_grouped.hip, route "two_hop_grouped") on hand-built graphs at its kernel edges
(tests/grouped_ref.py): more than one 2^20-id range in k_gd_large, starts with work 1023 / 1024 / 1025
around the k_gd_class threshold, empty hop-2 lists at the ends of gd_walk's chunks of 64 b's and hubs
whose waves take a second chunk, the self-loop rule, a window that does not start at 0, two relationship
types, endpoints in no node table and three different node predicates.  Every row is compared, with its
original id, with the plain Python restatement that tests/test_grouped_ref_cpu.py pins against the C
enumeration; counts are integers and must match exactly."""
import ctypes

import numpy as np
import pytest

import grouped_ref as gr
from golden_util import same_rows

pytestmark = pytest.mark.gpu


def scan_graph(backend, name, n):
    """one node table per label combination (as ScanGraph.from_property_graph), one relationship table per type"""
    from capsmi import ColumnData, I64
    from capsmi.planner import EntityTable, ScanGraph
    lo, n, src, dst, labels = gr.graph(name, n)
    combos = {}
    for v, ls in labels.items():
        combos.setdefault(ls, []).append(v)
    nodes = []
    for ls in sorted(combos, key=sorted):
        t = backend.table([ColumnData("id", I64, np.array(sorted(combos[ls]), dtype=np.int64))]).as_node_table("id")
        nodes.append(EntityTable("node", ls, {}, t, id_col="id"))
    types, rid = gr.rel_types(len(src)), np.arange(len(src), dtype=np.int64) + (1 << 50)
    rels = []
    for ty in ("R", "S"):
        k = types == ty
        t = backend.table([ColumnData("id", I64, rid[k]), ColumnData("source", I64, src[k]),
                           ColumnData("target", I64, dst[k])]).as_rel_table("id", "source", "target")
        rels.append(EntityTable("rel", frozenset({ty}), {}, t, id_col="id", src_col="source", dst_col="target"))
    return ScanGraph(backend, nodes, rels)


def query(pred, items=("a", "dc", "n")):
    la, lb, lc = [f":{x}" if x else "" for x in gr.PREDICATES[pred]]
    specs = {"a": ["id", "a"], "dc": ["count_distinct", ["id", "c"]], "n": ["count*"]}
    return {"clauses": [{"match": f"(a{la})-[:R|S]->(b{lb})-[:R|S]->(c{lc})"}],
            "return": {"items": [[k, specs[k]] for k in items]}}


def want_rows(name, n, pred, items=("a", "dc", "n")):
    rows, _ = gr.expected(name, n, pred)
    full = [{"a": a + gr.LO, "dc": dc, "n": cnt} for a, (cnt, dc) in rows.items()]
    return [{k: r[k] for k in items} for r in full]


@pytest.fixture(scope="module")
def graphs(session):
    """``graphs(name, n)``: the ScanGraph of a builder, uploaded once; released before the session closes"""
    made = {}

    def get(name, n):
        if (name, n) not in made:
            made[(name, n)] = scan_graph(session, name, n)
        return made[(name, n)]

    yield get
    made.clear()


def _run(session, sg, q, fused=True):
    from capsmi.planner import Planner, result_rows
    session.set_fused(fused)
    try:
        t, outs = Planner(sg).run(q)
        return result_rows(t, outs, session.dictionary)
    finally:
        session.set_fused(True)


def _routed(session, sg, q):
    before = session.route_count("two_hop_grouped")
    got = _run(session, sg, q)
    assert session.route_count("two_hop_grouped") == before + 1, "plan not routed to 'two_hop_grouped'"
    return got


def _launches(session, name):
    """launches of a timer since the last call (the read resets it)"""
    from capsmi import _lib
    cnt, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", session.handle, name, ctypes.byref(cnt), ctypes.byref(ms))
    return cnt.value


@pytest.mark.parametrize("name,n,pred", gr.CASES, ids=gr.CASE_IDS)
def test_grouped_rows(session, graphs, name, n, pred):
    """both aggregates in one query, and each alone, on the LDS-set path (the default)"""
    sg = graphs(name, n)
    got = _routed(session, sg, query(pred))
    assert same_rows(got, want_rows(name, n, pred))
    for items in (("a", "n"), ("a", "dc")):
        got = _routed(session, sg, query(pred, items))
        assert same_rows(got, want_rows(name, n, pred, items))


@pytest.mark.parametrize("name,n,pred", gr.CASES, ids=gr.CASE_IDS)
def test_grouped_rows_key_sort(session, graphs, knobs, name, n, pred):
    """CAPSMI_GROUPED=keys: the per-binding key sort gives the same rows; the grouped_distinct timer runs on
    the default path and not on the keys path"""
    from capsmi import _lib
    sg = graphs(name, n)
    want = want_rows(name, n, pred)
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        _launches(session, b"grouped_distinct")
        assert same_rows(_routed(session, sg, query(pred)), want)
        assert _launches(session, b"grouped_distinct") > 0
        knobs(session, CAPSMI_GROUPED="keys")
        got = _routed(session, sg, query(pred))
        assert _launches(session, b"grouped_distinct") == 0
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)
    assert same_rows(got, want)
    got = _routed(session, sg, query(pred, ("a", "dc")))
    assert same_rows(got, want_rows(name, n, pred, ("a", "dc")))


@pytest.mark.parametrize("name,n,pred", gr.CASES, ids=gr.CASE_IDS)
def test_grouped_rows_unfused(session, graphs, name, n, pred):
    """the same plan operator by operator (every graph here has fewer than 10^6 bindings)"""
    rows, _ = gr.expected(name, n, pred)
    assert sum(cnt for cnt, _ in rows.values()) < 1_000_000
    sg = graphs(name, n)
    before = session.route_count("two_hop_grouped")
    got = _run(session, sg, query(pred), fused=False)
    assert session.route_count("two_hop_grouped") == before
    assert same_rows(got, want_rows(name, n, pred))
