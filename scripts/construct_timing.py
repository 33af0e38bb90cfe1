"""Timing of CONSTRUCT through the planner mirror (capsmi/construct.py), from the library's kernel timers
(capsmi_session_kernel_time / _bytes, `expr_eval` among them: the interpreter launches that make the ids) and wall time.

  R-MAT scale 20 nodes, 2^24 relationships:
      MATCH (a)-[r]->(b) CONSTRUCT CLONE a, b CREATE (a)-[:E {w: r.id}]->(b)
  timed in three parts, each run on a session state in which the parts before it are done:
    1. construct_table   the bindings and the construct table (the pinned withColumns nodes), materialised
    2. entity_tables     PatternGraph.entity_tables(): per variable select / filter / distinct, the group over the flag
                         columns, one table per combination, each materialised
    3. first_two_hop     to_scan_graph() (the tables registered and compacted) and the first routed
                         MATCH (a)-[:E]->(b)-[:E]->(c) RETURN count(DISTINCT c) over it, timed apart

One process, 2 warm-up + 10 timed runs.  Writes one JSON document (--out) and prints it.  Needs the GPU."""
import argparse
import ctypes
import gc
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import wall_ms  # noqa: E402

TIMERS = ("expr_eval",)


def read_timers(s):
    from capsmi import _lib
    out = {}
    for name in TIMERS:
        nb = ctypes.c_double()
        _lib.call("capsmi_session_kernel_bytes", s.handle, name.encode(), ctypes.byref(nb))
        cnt, ms = ctypes.c_int64(), ctypes.c_double()
        _lib.call("capsmi_session_kernel_time", s.handle, name.encode(), ctypes.byref(cnt), ctypes.byref(ms))
        out[name] = {"launches": cnt.value, "ms": ms.value, "bytes": nb.value}
    return out


def one_run(s, sg, a):
    from capsmi.planner import Planner, result_rows
    spec = {"clones": [["a", "a"], ["b", "b"]], "creates": [{"rel": "e", "src": "a", "dst": "b", "type": "E"}],
            "sets": [["prop", "e", "w", ["id", "r"]]]}
    p = Planner(sg, {"rmat": sg})
    r = {}

    def part(name, f):
        read_timers(s)  # reset
        w, out = wall_ms(s, f)
        r[name] = dict(read_timers(s)["expr_eval"], wall_ms=w)
        return out

    def build():
        g, _ = p.run({"clauses": [{"match": "(a)-[r]->(b)"}, {"construct": spec}], "return": "graph"})
        return g, p.pattern_graphs[-1].table.size

    g, rows = part("construct_table", build)
    pattern = p.pattern_graphs[-1]

    def tables():
        nodes, rels = pattern.entity_tables()
        return [e.table.size for e in nodes + rels]

    sizes = part("entity_tables", tables)
    stored = part("to_scan_graph", g.to_scan_graph)
    q = {"clauses": [{"match": "(a:Person)-[:E]->(b:Person)-[:E]->(c:Person)"}],
         "return": {"items": [["n", ["count_distinct", ["id", "c"]]]]}}
    before = s.route_count("two_hop")

    def two_hop():
        t, outs = Planner(stored).run(q)
        return result_rows(t, outs, s.dictionary)

    got = part("first_two_hop", two_hop)
    assert s.route_count("two_hop") == before + 1, "the stored constructed graph's 2-hop was not routed"
    r["rows"], r["entity_table_rows"], r["two_hop"] = rows, sizes, got[0]["n"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--log-rels", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r27_construct.json"))
    a = ap.parse_args()
    from capsmi import Session, _lib, graph
    from capsmi.planner import EntityTable, ScanGraph
    s = Session(0)
    rels = graph.rmat_rels(s, a.scale, 0, 1 << a.log_rels, (57, 19, 19), 42)
    nodes = graph.rmat_nodes(s, a.scale, graph.NODES_ALL, 42)
    sg = ScanGraph(s, [EntityTable("node", frozenset({"Person"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"FRIEND_OF"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    gc.collect()
    gc.disable()
    rs = []
    for rep in range(a.warmup + a.reps):
        r = one_run(s, sg, a)
        print("run", rep, json.dumps({k: v if not isinstance(v, dict) else round(v["wall_ms"], 1) for k, v in r.items()
                                      if k != "entity_table_rows"}), flush=True)
        if rep >= a.warmup:
            rs.append(r)
        gc.collect()
    parts = ("construct_table", "entity_tables", "to_scan_graph", "first_two_hop")
    doc = {"scale": a.scale, "relationships": 1 << a.log_rels, "reps": a.reps, "warmup": a.warmup, "rows": rs[0]["rows"],
           "entity_table_rows": rs[0]["entity_table_rows"], "two_hop": rs[0]["two_hop"], "parts": {}}
    for name in parts:
        doc["parts"][name] = {"wall_ms": stats([r[name]["wall_ms"] for r in rs]),
                              "expr_eval_ms": stats([r[name]["ms"] for r in rs]),
                              "expr_eval_launches": rs[0][name]["launches"],
                              "expr_eval_declared_bytes": rs[0][name]["bytes"]}
    s.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
