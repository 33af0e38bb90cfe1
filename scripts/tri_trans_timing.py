"""Transitive triangle timing: the walks of csrc/k_tri_nodes.hip -- TriGraph.count_transitive_by_node for the
source, the middle and the sink, and TriGraph.count_transitive -- against the cyclic grouped walk
(TriGraph.count_by_node, the yardstick: the same slots with one weight and symmetric adds), on the C4 graph of
bench.py -- R-MAT with seed parameters (57, 19, 19), edge factor 16, every node scanned -- over one trigraph handle,
alternating in one process, from the library's own kernel timers (capsmi_session_kernel_time).  Per case: the term
passes (self terms, per-edge sources and slots, pair terms), the plan of the slots, the walk, and for the per-node
forms the compaction of the non-zero counters.  Every per-node run's counts are summed against the ungrouped
count of its pattern.  Writes one JSON document (--out) and prints it.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import wall_ms  # noqa: E402

CYCLIC = ("tri_by_node_terms", "tri_by_node_plan", "triangles_by_node", "tri_by_node_rows")
BY_ROLE = ("tri_trans_by_node_terms", "tri_trans_by_node_plan", "triangles_transitive_by_node", "tri_trans_by_node_rows")
COUNT = ("tri_trans_terms", "tri_trans_plan", "triangles_transitive")
TIMERS = CYCLIC + BY_ROLE + COUNT
CASES = {"cyclic_by_node": (CYCLIC, "triangles_by_node"), "source": (BY_ROLE, "triangles_transitive_by_node"),
         "middle": (BY_ROLE, "triangles_transitive_by_node"), "sink": (BY_ROLE, "triangles_transitive_by_node"),
         "count": (COUNT, "triangles_transitive")}


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
    out_path = a.out or os.path.join("profiles", f"r21_tri_trans_s{a.scale}.json")
    from capsmi import Session, _lib, graph
    n, m = 1 << a.scale, a.edge_factor << a.scale
    s = Session(0)
    rels = graph.rmat_rels(s, a.scale, 0, m, graph.RMAT_GRAPH500, 42)
    nodes = graph.rmat_nodes(s, a.scale, graph.NODES_ALL, 42)
    g = graph.TriGraph(s, [rels], graph.NodeBitmap(s, 0, n).add_scan(nodes, "id"))
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    roles = {"source": graph.TRI_ROLE_SOURCE, "middle": graph.TRI_ROLE_MIDDLE, "sink": graph.TRI_ROLE_SINK}
    runs = {case: [] for case in CASES}
    cyclic_total = g.count()
    total = g.count_transitive()
    rows = {}
    for rep in range(a.warmup + a.reps):
        for case in CASES:  # alternating, in one process
            read_timers(s)  # the read resets the timers
            if case == "count":
                w, got = wall_ms(s, g.count_transitive)
            else:
                f = g.count_by_node if case == "cyclic_by_node" else (lambda: g.count_transitive_by_node(roles[case]))
                w, t = wall_ms(s, f)
                w2, rows[case] = wall_ms(s, lambda: t.size)
                w += w2
            r = read_timers(s)
            if case != "count":
                got = int(t.column("count").values.sum())
                del t
            want = cyclic_total if case == "cyclic_by_node" else total
            assert got == want, f"{case}: counts sum to {got}, the ungrouped count is {want}"
            r["wall_ms"] = w
            if rep >= a.warmup:
                runs[case].append(r)
    nodes_n, oriented = g.stats()
    g.release()
    doc = {"scale": a.scale, "edge_factor": a.edge_factor, "nodes": n, "relationships": m, "oriented_edges": oriented,
           "reps": a.reps, "warmup": a.warmup, "cyclic_count": cyclic_total, "transitive_count": total, "rows": rows,
           "sum_check": "ok", "cases": {}}
    for case, (names, walk) in CASES.items():
        rs = runs[case]
        d = {name + "_ms": stats([r[name] for r in rs]) for name in names}
        d["kernels_ms"] = stats([sum(r[k] for k in names) for r in rs])
        d["wall_ms"] = stats([r["wall_ms"] for r in rs])
        doc["cases"][case] = d
    yard = doc["cases"]["cyclic_by_node"]["triangles_by_node_ms"]["median"]
    doc["walk_over_cyclic_walk_median"] = {case: doc["cases"][case][walk + "_ms"]["median"] / yard
                                           for case, (_, walk) in CASES.items() if case != "cyclic_by_node"}
    s.close()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
