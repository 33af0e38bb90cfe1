"""The fused undirected Expand counts (capsmi_undirected_count) called directly, no planner, on the hand-built graphs
of tests/und_ref.py, in every form the library has:
  count(*) of the 2-hop   the two-sided record partition with both arcs (k_count.hip k_rec_part<UND>; its
                          full-filter form and, CAPSMI_REC_FULL=0, the general one), and the per-relationship atomic
                          degrees (k_undirected.hip k_und_deg, CAPSMI_COUNT=atomic, the form above 2^26 ids)
  the distinct counts     the 2-D cell layout (k_und_part.hip k_und_2d, CAPSMI_UND=part) and the streaming form
                          (k_und_hop1 / k_und_hop2, CAPSMI_UND=stream, the form above 2^26 ids)
  one hop                 k_und_deg without degree arrays, k_und_mark1
Each graph aims at one edge of those kernels (its docstring in und_ref.py says which) and states preconditions that
tests/test_und_ref_cpu.py checks without a GPU; here they are asserted again with the device's CU count.  Every
expected value is an integer from the numpy reference (pinned to binding enumeration and to oracle/closed.c there),
every comparison is exact."""
import numpy as np
import pytest

import und_ref as ur

pytestmark = pytest.mark.gpu

FORMS = {
    "rec": dict(CAPSMI_COUNT="rec", CAPSMI_REC_FULL="1"),
    "rec_general": dict(CAPSMI_COUNT="rec", CAPSMI_REC_FULL="0"),
    "atomic": dict(CAPSMI_COUNT="atomic"),
    "layout": dict(CAPSMI_UND="part"),
    "stream": dict(CAPSMI_UND="stream"),
}
KINDS = {"rec": (0,), "rec_general": (0,), "atomic": (0,), "layout": (1, 2), "stream": (1, 2)}
TWO_HOP_GRAPHS = ("three_slices", "three_slices_full", "kb_wg", "kb_wg_full", "pull_8191", "pull_8193", "pull_hub",
                  "odd_cells", "offset", "wraps")


def _forms(name):
    # CAPSMI_REC_FULL matters only where every filter covers the domain: both values there
    return [f for f in FORMS if f != "rec_general" or name.endswith("_full")]


class Device:
    """a graph on the device: its relationship table(s) and the three node bitmaps"""

    def __init__(self, session, cs, cut=None):
        from capsmi import ColumnData, I64, graph
        self.cs = cs
        bounds = [0, len(cs.src)] if cut is None else [0, cut, len(cs.src)]
        self.rels = [session.table([ColumnData("id", I64, np.arange(b0, b1, dtype=np.int64)),
                                    ColumnData("source", I64, cs.src[b0:b1] + cs.lo),
                                    ColumnData("target", I64, cs.dst[b0:b1] + cs.lo)])
                     for b0, b1 in zip(bounds[:-1], bounds[1:])]
        self.bitmaps = []
        for which in range(3):
            ids = cs.ok_ids(which)
            bm = graph.NodeBitmap(session, cs.lo, cs.lo + cs.n)
            if len(ids):
                bm.add_scan(session.table([ColumnData("id", I64, ids + cs.lo)]))
            assert bm.stats() == (len(ids), True)
            self.bitmaps.append(bm)

    def count(self, session, hops, kind):
        from capsmi import graph
        a, b, c = self.bitmaps
        return graph.undirected_count(session, self.rels, hops, a, b, c if hops == 2 else None, kind)


@pytest.fixture(scope="module")
def device(session):
    """Device(name) built once per module; the host graphs and their answers are kept by und_ref.case"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    held = {}

    def get(name, cut=None):
        if (name, cut) not in held:
            cs = ur.case(name)
            ur.check_preconditions(cs, num_cus=cus)
            held[(name, cut)] = Device(session, cs, cut)
        return held[(name, cut)]

    yield get
    held.clear()


def _check(session, knobs, dev, form, hops=2):
    knobs(session, **FORMS[form])
    for kind in KINDS[form]:
        assert dev.count(session, hops, kind) == dev.cs.expected(hops, kind), (dev.cs.name, form, hops, kind)


@pytest.mark.parametrize("name,form", [(n, f) for n in TWO_HOP_GRAPHS for f in _forms(n)])
def test_two_hop(session, knobs, device, name, form):
    """Layout and slices (three_slices: three slices, a ragged tail, hubs at the slice edges; kb_wg: K(b) = 2 only across
    workgroups, x(b) read from another slice; pull_*: a cell just below and just above hop 2's pull of the K2 words,
    and a hub cell; odd_cells: odd cell starts), the offset domain with relationships leaving it, and count(*) with
    unequal filters and wrapping 16-bit counters (wraps) -- each in every form."""
    _check(session, knobs, device(name), form)


@pytest.mark.parametrize("name", ["pull_8191", "pull_8193", "pull_hub"])
def test_layout_and_stream_agree(session, device, name):
    dev, got = device(name), {}
    for form in ("layout", "stream"):
        with session.configured(**FORMS[form]):
            got[form] = [dev.count(session, 2, kind) for kind in (1, 2)]
    assert got["layout"] == got["stream"] == list(dev.cs.two_hop()[1:])


@pytest.mark.parametrize("form", list(FORMS))
def test_two_tables(session, knobs, device, form):
    """the three-slice graph as two tables of unequal size (a third and the rest): the answers of the one table"""
    for name in ("three_slices", "three_slices_full"):
        if form in _forms(name):
            cs = ur.case(name)
            dev = device(name, cut=len(cs.src) // 3)
            assert len(dev.rels) == 2 and dev.rels[0].size * 2 < dev.rels[1].size
            _check(session, knobs, dev, form)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_above_2_26_ids_takes_the_large_forms_unasked(session, device, kind):
    """2^26 + 77 ids, no knob set: count(*) by the atomic degrees, the distinct counts by the streaming kernels; the
    reference runs on the compacted graph"""
    dev = device("above_2_26")
    assert dev.cs.n > 1 << 26
    assert dev.count(session, 2, kind) == dev.cs.expected(2, kind)
    assert dev.count(session, 1, kind) == dev.cs.expected(1, kind)


@pytest.mark.parametrize("name", ["three_slices", "three_slices_full", "offset", "grid_stride"])
def test_one_hop(session, device, name):
    """kinds 0, 1, 2 of one hop (grid_stride: more relationships than the largest grid has threads)"""
    dev = device(name)
    assert [dev.count(session, 1, kind) for kind in (0, 1, 2)] == list(dev.cs.one_hop())


@pytest.mark.parametrize("form", ["atomic", "stream"])
def test_two_hop_grid_stride(session, knobs, device, form):
    """the streaming 2-hop kernels on the same table: every one of them loops past 16384 x 256 threads"""
    _check(session, knobs, device("grid_stride"), form)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ur.DEGENERATE)
def test_degenerate(session, knobs, device, name, form):
    """no relationships, only self-loops, a single relationship, an empty a_ok, a b_ok of one id: every (hops, kind)"""
    dev = device(name)
    _check(session, knobs, dev, form)
    knobs(session, **FORMS[form])
    assert [dev.count(session, 1, kind) for kind in (0, 1, 2)] == list(dev.cs.one_hop())


def test_no_tables_at_all(session, device):
    """an empty list of relationship tables counts nothing"""
    from capsmi import graph
    a, b, c = device("no_rels").bitmaps
    assert [graph.undirected_count(session, [], hops, a, b, c, kind) for hops in (1, 2) for kind in (0, 1, 2)] == [0] * 6
