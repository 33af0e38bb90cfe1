"""The reference of the grouped 2-hop device tests (tests/grouped_ref.py), pinned on the CPU: the plain
Python restatement equals the C enumeration (oracle/rmat.c orc_two_hop_enumerate) row for row on every
graph, window and predicate set, and the builders deliver the shapes they claim.  The shape checks are
conditions on the inputs: they hold or the test fails."""
import numpy as np
import pytest

import grouped_ref as gr
from grouped_ref import R, WINDOWS

PREDS = list(gr.PREDICATES)


@pytest.mark.parametrize("name,n,pred", gr.CASES, ids=gr.CASE_IDS)
def test_restatement_equals_enumeration(name, n, pred):
    from oracle import cpu
    lo, n, src, dst, labels = gr.graph(name, n)
    assert lo == (1 << 33) + 12345 and lo in labels and lo + n - 1 in labels
    assert len(src) < 100_000
    a_ok, b_ok, c_ok = gr.masks(lo, n, labels, pred)
    rows, _ = gr.expected(name, n, pred)
    total, _, grows, gdist = cpu.two_hop_enumerate(n, src - lo, dst - lo, a_ok, b_ok, c_ok, grouped=True)
    assert 0 < total < 3_000_000
    starts = np.nonzero(grows)[0]
    assert sorted(rows) == starts.tolist()
    assert [rows[a] for a in starts.tolist()] == list(zip(grows[starts].tolist(), gdist[starts].tolist()))


def _ok_lists(name, n, pred):
    """({a: sorted distinct ok b's}, {b: distinct ok c's}) over relative ids"""
    lo, n, src, dst, labels = gr.graph(name, n)
    a_ok, b_ok, c_ok = gr.masks(lo, n, labels, pred)
    s, d = src - lo, dst - lo
    h1 = (a_ok[s] != 0) & (b_ok[d] != 0)
    h2 = (b_ok[s] != 0) & (c_ok[d] != 0)
    bs, cs = {}, {}
    for x, y in zip(s[h1].tolist(), d[h1].tolist()):
        bs.setdefault(x, set()).add(y)
    for x, y in zip(s[h2].tolist(), d[h2].tolist()):
        cs.setdefault(x, set()).add(y)
    return {a: sorted(v) for a, v in bs.items()}, cs


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("n", WINDOWS)
def test_hub_shape(n, pred):
    """each hub: at least 1025 distinct ok b's (a wave of k_gd_large takes a second chunk), work in the
    large class, ok c's on both sides of every range boundary inside the window, empty lists at chunk
    positions 0, 63, 64 and last"""
    rows, work = gr.expected("hub", n, pred)
    bs, cs = _ok_lists("hub", n, pred)
    hubs = gr.marks("hub", n)["hubs"]
    for h in hubs:
        assert len(bs[h]) >= 1025 and work[h] > gr.SMALL_MAX
        seen = set().union(*[cs.get(b, set()) for b in bs[h]])
        for k in range(1, (n + R - 1) // R):
            assert any(k * R - 8 <= c < k * R for c in seen) and any(k * R <= c < min(n, k * R + 8) for c in seen)
            if pred != "abc":  # k * R itself carries no label
                assert k * R - 1 in seen and k * R in seen
        assert n - 1 in seen and max(seen) == n - 1
        # c's shared between b's of different waves' chunks
        assert cs[bs[h][2]] & cs[bs[h][70]] and cs[bs[h][2]] & cs[bs[h][1030]]
        for i in (0, 63, 64, len(bs[h]) - 1):  # a looped hub is its own b, in front of the others
            assert not cs.get(bs[h][i]) or (i == 0 and bs[h][0] == h and not cs.get(bs[h][1]))
    h1, h2, h3 = hubs
    assert h1 not in bs[h1] and h2 in bs[h2] and h3 in bs[h3]
    assert any(h2 in cs.get(b, set()) for b in bs[h2] if b != h2)  # back to hub 2 through another b
    # hub 1's ends include hub 2 (through another b); the one loop at hub 2 adds hub 2's own b's but not
    # hub 2 again, the two loops at hub 3 add hub 3 as well
    seen1 = set().union(*[cs.get(b, set()) for b in bs[h1]])
    assert h2 in seen1 and h3 not in seen1 and h3 in cs[h3]
    assert rows[h2][1] == rows[h1][1] + len(cs[h2] - seen1) and rows[h3][1] == rows[h1][1] + len(cs[h3] - seen1)
    lo, _, src, dst, labels = gr.graph("hub", n)
    c_ok = gr.masks(lo, n, labels, pred)[2]
    for h, nl in ((h2, 1), (h3, 2)):  # each loop as r1 meets every other relationship of the hub
        out_ok = int(c_ok[dst[src - lo == h] - lo].sum())
        assert rows[h][0] == rows[h1][0] + nl * (out_ok - 1)
    if n > R:
        assert len({c // R for b in bs[h1] for c in cs.get(b, ())}) == (n + R - 1) // R


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("n", WINDOWS)
def test_boundary_shape(n, pred):
    rows, work = gr.expected("boundary", n, pred)
    m = gr.marks("boundary", n)
    assert [work[a] for a in m["exact"]] == [1023, 1024, 1025]
    extra = 0 if pred == "abc" else 50
    assert [work[a] for a in m["mixed"]] == [1023 + extra, 1024 + extra, 1025 + extra]
    assert [work[a] for a in m["two"]] == [1024, 1025]
    assert [rows[a][1] for a in m["two"]] == [512, 513]
    assert [rows[a][1] for a in m["exact"]] == [1023, 1024, 1025]
    assert all(rows[a][0] > rows[a][1] for a in m["exact"])  # tripled relationships


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("n", WINDOWS)
def test_chunks_shape(n, pred):
    rows, work = gr.expected("chunks", n, pred)
    bs, cs = _ok_lists("chunks", n, pred)
    starts = gr.marks("chunks", n)["starts"]
    assert [len(bs[a]) for a in starts] == list(gr.CHUNK_SIZES)
    for a in starts:
        nb = len(bs[a])
        for i in {0, 63, 64, nb - 1}:
            if i < nb:
                assert not cs.get(bs[a][i])
        assert cs.get(bs[a][2]) and cs.get(bs[a][nb // 2 + 3])
        assert bool(cs.get(bs[a][1])) == (pred != "abc")
        assert 0 < work[a] <= gr.SMALL_MAX and a in rows


@pytest.mark.parametrize("n", WINDOWS)
def test_loops_shape(n):
    lo, _, src, dst, labels = gr.graph("loops", n)
    m = gr.marks("loops", n)
    nloops = {a: int(((src - lo == a) & (dst - lo == a)).sum()) for a in m["looped"] + m["back"]}
    assert [nloops[a] for a in m["looped"]] == [0, 1, 2, 3] * 4
    assert [nloops[a] for a in m["back"]] == [0, 1, 2]
    none, _ = gr.expected("loops", n, "none")
    abc, _ = gr.expected("loops", n, "abc")
    # unlabelled, ABC starts: b = other gives 3 * 9 bindings over 3 c's; L loops add L * (3 + L - 1) bindings
    # (the other loops and the tripled a -> b), c = a only with a second loop, c = b always
    assert [none[a] for a in m["looped"][:4]] == [(27, 3), (27 + 3, 4), (27 + 8, 5), (27 + 15, 5)]
    # labelled: a start without B is not its own b; one without C is its own b (each loop then reaches b over
    # the tripled a -> b) but never its own c; one without A is no start
    assert [abc[a] for a in m["looped"][:4]] == [(27, 3), (27 + 3, 4), (27 + 8, 5), (27 + 15, 5)]
    assert [abc[a] for a in m["looped"][4:8]] == [(27, 3)] * 4
    assert [abc[a] for a in m["looped"][8:12]] == [(27, 3), (27 + 3, 4), (27 + 6, 4), (27 + 9, 4)]
    assert not any(a in abc for a in m["looped"][12:]) and all(a in none for a in m["looped"][12:])
    # a -> b -> a: c = a through b is kept whatever the loops
    assert [none[a] for a in m["back"]] == [(2, 2), (2 + 1, 3), (2 + 4, 3)]
    (fb,), (fc,) = m["fails_b"], m["fails_c"]
    assert fb in none and fb not in abc and fc in none and fc not in abc
    # tripled parallel relationships on both hops, over both types
    t = gr.rel_types(len(src))
    pairs = {}
    for s, d, ty in zip((src - lo).tolist(), (dst - lo).tolist(), t.tolist()):
        pairs.setdefault((s, d), set()).add(ty)
    assert pairs[(m["looped"][0], m["looped"][0] + 8)] == {"R", "S"}


def test_dangling_endpoints_and_types():
    """every graph has an endpoint in no node table used as b and one used as c, and both types"""
    for name in gr.BUILDERS:
        lo, n, src, dst, labels = gr.graph(name, WINDOWS[0])
        not_node = np.array([v not in labels for v in dst.tolist()])
        as_c = set(dst[not_node].tolist())
        as_b = as_c & set(src.tolist())
        assert as_b and as_c - as_b
        starts = set(src.tolist())
        assert any(s in labels for s, d in zip(src.tolist(), dst.tolist()) if d in as_b)
        assert set(gr.rel_types(len(src)).tolist()) == {"R", "S"}
        combos = {ls for ls in labels.values()}
        assert len(combos) == 8 if name == "hub" else len(combos) >= 4
        assert starts
