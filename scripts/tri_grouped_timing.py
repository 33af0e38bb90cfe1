"""Grouped triangle timing: graph.triangle_count_by_node (RETURN id(a), count(*)) against graph.triangle_count
(RETURN count(*)) on the C4 graph of bench.py -- R-MAT with seed parameters (57, 19, 19), edge factor 16, every
node scanned -- over the same resident tables, alternating in one process, from the library's own kernel
timers (capsmi_session_kernel_time).  Both entry points build the trigraph (the tri_* build timers, common to
both) and walk it: `triangles` is the ungrouped walk, `tri_by_node_terms` (self terms, per-edge sources and
slots, pair terms), `tri_by_node_plan` (scan of the slots, compaction of the edges that own some),
`triangles_by_node` (tile heads + the walk) and `tri_by_node_rows` (compaction of the non-zero counters) the
grouped one.  Every grouped run's counts are summed against the ungrouped count.  Writes one JSON document
(--out) and prints it.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import wall_ms  # noqa: E402

BUILD = ("tri_deg", "tri_order", "tri_pack", "tri_sort_und", "tri_sort_or", "tri_post")
GROUPED = ("tri_by_node_terms", "tri_by_node_plan", "triangles_by_node", "tri_by_node_rows")
TIMERS = BUILD + ("triangles",) + GROUPED


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
    out_path = a.out or os.path.join("profiles", f"r20_tri_grouped_s{a.scale}.json")
    from capsmi import Session, _lib, graph
    n, m = 1 << a.scale, a.edge_factor << a.scale
    s = Session(0)
    rels = graph.rmat_rels(s, a.scale, 0, m, graph.RMAT_GRAPH500, 42)
    nodes = graph.rmat_nodes(s, a.scale, graph.NODES_ALL, 42)
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    runs = {"count": [], "by_node": []}
    total = rows = None
    for rep in range(a.warmup + a.reps):
        for case in runs:  # alternating, in one process
            ok = graph.NodeBitmap(s, 0, n).add_scan(nodes, "id")
            read_timers(s)  # the read resets the timers
            if case == "count":
                w, total = wall_ms(s, lambda: graph.triangle_count(s, [rels], ok))
            else:
                w, t = wall_ms(s, lambda: graph.triangle_count_by_node(s, [rels], ok))
                w2, rows = wall_ms(s, lambda: t.size)
                w += w2
            r = read_timers(s)
            if case == "by_node":
                got = int(t.column("count").values.sum())
                assert got == total, f"grouped counts sum to {got}, the ungrouped count is {total}"
                del t
            r["wall_ms"] = w
            if rep >= a.warmup:
                runs[case].append(r)
    doc = {"scale": a.scale, "edge_factor": a.edge_factor, "nodes": n, "relationships": m, "reps": a.reps,
           "warmup": a.warmup, "count": total, "rows": rows, "sum_check": "ok", "cases": {}}
    for case, rs in runs.items():
        d = {name + "_ms": stats([r[name] for r in rs]) for name in TIMERS if any(r[name] > 0 for r in rs)}
        d["build_ms"] = stats([sum(r[k] for k in BUILD) for r in rs])
        d["wall_ms"] = stats([r["wall_ms"] for r in rs])
        doc["cases"][case] = d
    walk = stats([sum(r[k] for k in GROUPED) for r in runs["by_node"]])
    doc["by_node_walk_ms"] = walk
    tri = doc["cases"]["count"]["triangles_ms"]
    doc["by_node_walk_over_count_walk_median"] = walk["median"] / tri["median"]
    doc["by_node_wall_over_count_wall_median"] = (doc["cases"]["by_node"]["wall_ms"]["median"]
                                                  / doc["cases"]["count"]["wall_ms"]["median"])
    s.close()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
