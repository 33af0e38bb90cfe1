"""Undirected triangle timing: the forms of csrc/k_tri_nodes.hip -- TriGraph.count_undirected by the hash walks
(CAPSMI_TRI_UND_COUNT=hash) and by the search walk (=walk), and TriGraph.count_undirected_by_node for the END and the
MIDDLE class -- on the C4 graph of bench.py (R-MAT with seed parameters (57, 19, 19), edge factor 16, every node
scanned) over one trigraph handle, alternating in one process, from the library's own kernel timers
(capsmi_session_kernel_time).  Yardsticks in the same process, all on code paths older than the undirected forms:
  cyclic_nosplit   TriGraph.count over a second handle built with CAPSMI_TRI_SPLIT=0 -- the same combined hash
                   walks with the cyclic weight, v-mode on there and off in `hash`
  cyclic_nosplit_novm  the same over a third handle built with CAPSMI_TRI_VMODE_T=0 as well: `hash`'s launches exactly,
                   with the other weight -- the difference to cyclic_nosplit is what the missing v-mode costs
  cyclic_split     TriGraph.count over the first handle (the default split walks; for scale)
  transitive       TriGraph.count_transitive -- the search walk with the transitive weights, for `walk`
  cyclic_by_node   TriGraph.count_by_node -- for the per-node forms
Every repetition asserts hash = walk = the sum of the END rows = the sum of the MIDDLE rows.  Writes one JSON
document (--out) and prints it.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import wall_ms  # noqa: E402

HASH = ("tri_und_terms", "triangles_undirected")
WALK = ("tri_und_terms", "tri_und_plan", "triangles_undirected_walk")
BY_NODE = ("tri_und_by_node_terms", "tri_und_by_node_plan", "triangles_undirected_by_node", "tri_und_by_node_rows")
CYCLIC = ("triangles",)
TRANS = ("tri_trans_terms", "tri_trans_plan", "triangles_transitive")
CYC_BY_NODE = ("tri_by_node_terms", "tri_by_node_plan", "triangles_by_node", "tri_by_node_rows")
TIMERS = tuple(dict.fromkeys(HASH + WALK + BY_NODE + CYCLIC + TRANS + CYC_BY_NODE))
# case: (its timers, the timer of its triangle walk, its yardstick)
CASES = {"hash": (HASH, "triangles_undirected", "cyclic_nosplit"),
         "walk": (WALK, "triangles_undirected_walk", "transitive"),
         "end": (BY_NODE, "triangles_undirected_by_node", "cyclic_by_node"),
         "middle": (BY_NODE, "triangles_undirected_by_node", "cyclic_by_node"),
         "cyclic_nosplit": (CYCLIC, "triangles", None), "cyclic_nosplit_novm": (CYCLIC, "triangles", None),
         "cyclic_split": (CYCLIC, "triangles", None),
         "transitive": (TRANS, "triangles_transitive", None), "cyclic_by_node": (CYC_BY_NODE, "triangles_by_node", None)}


def read_timers(s):
    from capsmi import _lib
    out = {}
    for name in TIMERS:
        cnt, ms = ctypes.c_int64(), ctypes.c_double()
        _lib.call("capsmi_session_kernel_time", s.handle, name.encode(), ctypes.byref(cnt), ctypes.byref(ms))
        out[name] = ms.value
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join("profiles", f"r22_tri_und_s{a.scale}.json")
    from capsmi import Session, _lib, graph
    n, m = 1 << a.scale, a.edge_factor << a.scale
    s = Session(0)
    rels = graph.rmat_rels(s, a.scale, 0, m, graph.RMAT_GRAPH500, 42)
    nodes = graph.rmat_nodes(s, a.scale, graph.NODES_ALL, 42)
    ok = graph.NodeBitmap(s, 0, n).add_scan(nodes, "id")
    g = graph.TriGraph(s, [rels], ok)
    with s.configured(CAPSMI_TRI_SPLIT="0"):
        g0 = graph.TriGraph(s, [rels], ok)  # the combined lists and their in-lists: the cyclic hash walks' yardstick
    with s.configured(CAPSMI_TRI_SPLIT="0", CAPSMI_TRI_VMODE_T="0"):
        g1 = graph.TriGraph(s, [rels], ok)  # and no v-mode: every edge walked from its u
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    classes = {"end": graph.TRI_UND_END, "middle": graph.TRI_UND_MIDDLE}
    runs = {case: [] for case in CASES}
    cyclic_total, trans_total = g.count(), g.count_transitive()
    assert g0.count() == cyclic_total and g1.count() == cyclic_total
    total = None
    rows = {}

    def counted(form):
        with s.configured(CAPSMI_TRI_UND_COUNT=form):
            return g.count_undirected()

    for rep in range(a.warmup + a.reps):
        got = {}
        for case in CASES:  # alternating, in one process
            read_timers(s)  # the read resets the timers
            if case in ("hash", "walk"):
                w, got[case] = wall_ms(s, lambda: counted(case))
            elif case in ("cyclic_nosplit", "cyclic_nosplit_novm", "cyclic_split", "transitive"):
                f = {"cyclic_nosplit": g0.count, "cyclic_nosplit_novm": g1.count, "cyclic_split": g.count,
                     "transitive": g.count_transitive}[case]
                w, got[case] = wall_ms(s, f)
            else:
                f = g.count_by_node if case == "cyclic_by_node" else (lambda: g.count_undirected_by_node(classes[case]))
                w, t = wall_ms(s, f)
                w2, rows[case] = wall_ms(s, lambda: t.size)
                w += w2
            r = read_timers(s)
            if case in ("end", "middle", "cyclic_by_node"):
                got[case] = int(t.column("count").values.sum())
                del t
            r["wall_ms"] = w
            if rep >= a.warmup:
                runs[case].append(r)
        assert got["hash"] == got["walk"] == got["end"] == got["middle"], got
        assert total is None or total == got["hash"]
        total = got["hash"]
        for case in ("cyclic_nosplit", "cyclic_nosplit_novm", "cyclic_split", "cyclic_by_node"):
            assert got[case] == cyclic_total, got
        assert got["transitive"] == trans_total, got
    nodes_n, oriented = g.stats()
    g.release()
    g0.release()
    g1.release()
    doc = {"scale": a.scale, "edge_factor": a.edge_factor, "nodes": n, "relationships": m, "oriented_edges": oriented,
           "reps": a.reps, "warmup": a.warmup, "undirected_count": total, "cyclic_count": cyclic_total,
           "transitive_count": trans_total, "rows": rows, "sum_check": "ok", "cases": {}}
    for case, (names, walk, _) in CASES.items():
        rs = runs[case]
        d = {name + "_ms": stats([r[name] for r in rs]) for name in names}
        d["kernels_ms"] = stats([sum(r[k] for k in names) for r in rs])
        d["wall_ms"] = stats([r["wall_ms"] for r in rs])
        doc["cases"][case] = d
    doc["walk_over_yardstick_median"] = {
        case: {"yardstick": yard, "ratio": doc["cases"][case][walk + "_ms"]["median"] /
               doc["cases"][yard][CASES[yard][1] + "_ms"]["median"]}
        for case, (_, walk, yard) in CASES.items() if yard}
    doc["hash_walk_over_cyclic_nosplit_novm_median"] = (doc["cases"]["hash"]["triangles_undirected_ms"]["median"] /
                                                        doc["cases"]["cyclic_nosplit_novm"]["triangles_ms"]["median"])
    doc["hash_over_walk_kernels_median"] = (doc["cases"]["hash"]["kernels_ms"]["median"] /
                                            doc["cases"]["walk"]["kernels_ms"]["median"])
    s.close()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
