"""The sorted build of the cyclic triangle count's oriented graph (csrc/k_tri.hip tri_build: undirected key
sort, k_und_runs / k_und_long, k_orient, oriented sort, k_exc_place, k_offsets, k_targets) in both of its key
layouts: the direction bit at bit 31 with coded targets (windows of up to 2^24 ids, taken with
CAPSMI_TRI_BUILD=sorted) and the wide layout (every window above 2^24 ids, taken by default).  The hand-built
graphs of tests/tri_ref.py sit on the kernels' thresholds -- undirected runs of 1 to 600 relationships in
either and both directions around kShortRun = 32, the wave width 64 and k_und_long's stride 256, multiplicities
at the 4-bit code's saturation 15 in every lane and in the last one alone, a hub of degree 2^16 and more, lists
longer than an LDS chunk -- and are placed at the ends of the windows: the all-ones id 2^24 - 1 beside the
dropped relationships' all-ones keys, the first wide id 2^24, a window that starts at 2^40 + 12345.  Every count
is compared with the plain restatement that tests/test_tri_ref_cpu.py pins to the oracle, exactly; so are the
number of oriented edges and, by the build phases' kernel timers, the path taken."""
import ctypes

import numpy as np
import pytest

import tri_ref as tr

pytestmark = pytest.mark.gpu

VMODE = ["0", "2", "default"]  # CAPSMI_TRI_VMODE_T: every edge from u / almost every edge from v / 256
SORTED_BY_DEFAULT = ("wide", "wide_offset", "last_far")  # windows above 2^24 ids


def _launches(session, name):
    """launches of a timer since the last call (the read resets it)"""
    from capsmi import _lib
    cnt, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", session.handle, name, ctypes.byref(cnt), ctypes.byref(ms))
    return cnt.value


def _trigraph(session, knobs, c, build, expect_sorted, cuts=None):
    """the TriGraph of a Case over its node table and its relationship table (or the tables of the rows
    between `cuts`), built by `build` ("sorted": CAPSMI_TRI_BUILD=sorted, "auto": nothing set); asserts the
    build taken from the phase timers (tri_sort_und: the sorted build's first sort, tri_deg: the direct
    build's degree sample)"""
    from capsmi import ColumnData, I64, _lib, graph
    assert build in ("sorted", "auto")
    if build == "sorted":
        knobs(session, CAPSMI_TRI_BUILD="sorted")
    cuts = [0, len(c.src)] if cuts is None else cuts
    rels = [session.table([ColumnData("id", I64, np.arange(a, b, dtype=np.int64) + (1 << 50)),
                           ColumnData("source", I64, np.ascontiguousarray(c.src[a:b])),
                           ColumnData("target", I64, np.ascontiguousarray(c.dst[a:b]))])
            for a, b in zip(cuts[:-1], cuts[1:])]
    nodes = session.table([ColumnData("id", I64, np.ascontiguousarray(c.node_ids))])
    ok = graph.NodeBitmap(session, c.lo, c.lo + c.n).add_scan(nodes)
    _lib.call("capsmi_session_set_profiling", session.handle, 1)
    try:
        _launches(session, b"tri_sort_und")
        _launches(session, b"tri_deg")
        g = graph.TriGraph(session, rels, ok)
        und, deg = _launches(session, b"tri_sort_und"), _launches(session, b"tri_deg")
    finally:
        _lib.call("capsmi_session_set_profiling", session.handle, 0)
    if expect_sorted:
        assert und >= 1 and deg == 0, "the sorted build did not run"
    else:
        assert und == 0 and deg >= 1, "the direct build did not run"
    return g


def _check(session, knobs, c, want, build, placement, parts=(1,), vmode="default", split="default", cuts=None):
    if vmode != "default":
        knobs(session, CAPSMI_TRI_VMODE_T=vmode)
    if split != "default":
        knobs(session, CAPSMI_TRI_SPLIT=split)
    g = _trigraph(session, knobs, c, build, build == "sorted" or placement in SORTED_BY_DEFAULT, cuts)
    try:
        count, pairs = want
        assert g.stats() == (c.n, pairs)
        for nparts in parts:
            assert sum(g.count(p, nparts) for p in range(nparts)) == count
    finally:
        g.release()


@pytest.mark.parametrize("vmode", ["0", "default"])
@pytest.mark.parametrize("seed", range(8))
def test_random_multigraphs(session, knobs, seed, vmode):
    g = tr.random_multigraph(seed)
    c = tr.materialise(g, tr.place("low", g.k))
    _check(session, knobs, c, tr.expected_of(c), "sorted", "low", vmode=vmode)


@pytest.mark.parametrize("vmode", VMODE)
@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("placement", ["low", "edge24"])
@pytest.mark.parametrize("dropped", [False, True], ids=["plain", "dropped"])
def test_runs_bit31_layout(session, knobs, dropped, placement, split, vmode):
    """msh = 0, coded targets: run lengths around 15 (the code's cap: k_orient's exceptions, k_exc_place), 32
    (k_und_runs' list of long runs), 64 and 256 (k_und_long's waves and stride), in either and both directions;
    at edge24 the keys of upper end 2^24 - 1 next to the dropped keys, which k_heads / k_first_none cut off"""
    c = tr.case("runs", placement, dropped)
    _check(session, knobs, c, tr.expected("runs", dropped), "sorted", placement, (1, 3), vmode, split)


def test_runs_parity_with_direct_build(session, knobs):
    """the restatement against the direct build (the default at 2^24 ids), which tests/test_gpu_triangles.py
    compares with the oracle: the reference of this file and the known-good build agree"""
    c = tr.case("runs", "edge24", True)
    _check(session, knobs, c, tr.expected("runs", True), "auto", "edge24")


@pytest.mark.parametrize("vmode", VMODE)
@pytest.mark.parametrize("placement", ["wide", "wide_offset"])
@pytest.mark.parametrize("dropped", [False, True], ids=["plain", "dropped"])
def test_runs_wide_layout(session, knobs, dropped, placement, vmode):
    """msh = 1, uncoded: payloads sorted as values, unpacked in-keys, combined walks; ids 2^24 - 1 and 2^24,
    v-mode thresholds other than 256, parts, a node filter, a window from 2^40 + 12345"""
    c = tr.case("runs", placement, dropped)
    _check(session, knobs, c, tr.expected("runs", dropped), "auto", placement, (1, 3), vmode)


@pytest.mark.parametrize("placement,build", [("low", "sorted"), ("wide", "auto")])
def test_runs_over_three_tables(session, knobs, placement, build):
    """k_pack once per relationship table into one key array: tables of unequal size, one of them empty"""
    c = tr.case("runs", placement)
    m = len(c.src)
    _check(session, knobs, c, tr.expected("runs"), build, placement, cuts=[0, m // 5, m // 5, m])


@pytest.mark.parametrize("vmode", ["0", "default"])
@pytest.mark.parametrize("placement,build", [("low", "sorted"), ("edge24", "sorted"), ("wide", "auto")])
@pytest.mark.parametrize("graph", ["all_exceptions", "one_exception"])
def test_exceptions(session, knobs, graph, placement, build, vmode):
    """multiplicity 15 both ways on every pair (every lane of every wave of k_orient appends an exception) and
    on the last pair alone (one lane of the last wave); uncoded in the wide window"""
    c = tr.case(graph, placement)
    _check(session, knobs, c, tr.expected(graph), build, placement, vmode=vmode)


@pytest.mark.parametrize("vmode", ["default", "0"])
@pytest.mark.parametrize("placement,build", [("low", "sorted"), ("last_far", "auto")])
@pytest.mark.parametrize("dropped", [False, True], ids=["plain", "dropped"])
def test_hub(session, knobs, dropped, placement, build, vmode):
    """a degree of 2^16 and more: three digits in the degree sort, and under the exact degree order every one
    of the hub's 70,000 edges points at it (one in-list of 70,000); with the node filter, a fifth of the
    neighbours' keys dropped"""
    c = tr.case("hub", placement, dropped)
    _check(session, knobs, c, tr.expected("hub", dropped), build, placement, (1, 3), vmode)


@pytest.mark.parametrize("placement,build", [("low", "sorted"), ("last_far", "auto")])
def test_dense(session, knobs, placement, build):
    """complete digraph on 2200 nodes behind the sorted build: out-degrees above one 2048-entry LDS chunk"""
    c = tr.case("dense", placement)
    _check(session, knobs, c, tr.expected("dense"), build, placement)


@pytest.mark.parametrize("placement,build", [("low", "sorted"), ("wide", "auto")])
@pytest.mark.parametrize("kind", ["no_relationships", "loops_only", "all_dropped"])
def test_trivial_inputs(session, knobs, kind, placement, build):
    """no keys at all, self-loops only (count = sum of s (s - 1) (s - 2)), and every key dropped by the node
    filter: no run, every degree 0 (a degree sort without a digit), empty lists"""
    if kind == "all_dropped":
        g, ok = tr.all_dropped()
    else:
        g, ok = getattr(tr, kind)(), None
    c = tr.materialise(g, tr.place(placement, g.k), core_ok=ok)
    want = tr.expected_of(c)
    assert want == ((sum(s * (s - 1) * (s - 2) for _, s in tr.LOOPS_ONLY) if kind == "loops_only" else 0), 0)
    _check(session, knobs, c, want, build, placement)
