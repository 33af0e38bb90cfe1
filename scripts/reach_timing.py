"""Var-length count(DISTINCT b) timing ("k-hop reach"), on R-MAT LDBC shape (0.45, 0.15, 0.15), edge
factor 32, every node a Person, from the library's own kernel timers (capsmi_session_kernel_time / _bytes):
  - the planner's grouped *1..3 query routed and run operator by operator under an unrouted limit of 1 GiB, at
    growing scales until the operator path is refused;
  - the grouped *1..3 entry at scales 14 and 16 for every CAPSMI_REACH_WORDS value, and for 1 and 8 words through
    the flat level pass (CAPSMI_REACH=flat);
  - the grouped *1..3 and *1..6 entries and the global *1..6 entry at growing scales until a query passes 3.5 s.
With --collect, collect(DISTINCT b) instead ("reach lists"):
  - the planner's grouped *1..3 collect query, operator by operator under the 1 GiB limit and routed, at growing
    scales until the operator path is refused;
  - the grouped *1..3 collect entry at scales 14 and 16 at auto width, with the count entry beside it in the same
    process, the extraction's timers and the total element count.
With --collect --sparse-ids, the same R-MAT graph twice in one process, plain ids against ids spread near 2^40
("reach lists on compacted graphs"), scales 14 and 16 (or --scales 14,16), *1..3, auto width:
  - the grouped collect entry on plain ids, then the mapped entry over the same dense ids with orig = the spread ids
    in random order, and with orig = the identity (the gather reading in order: the plain kernel's access pattern);
    the mapped entry sorts the n ids per call (timer reach_list_order), the gather is timer reach_list_gather;
  - the planner's grouped collect on the graph stored with the spread ids and compacted (the order kept with the graph);
  - with --global SCALE, the global entry plain and mapped (the bitmap permutation) at that scale;
  - with --operator (or --operator-only), the planner's grouped collect on the compacted graph operator by operator
    under the 1 GiB limit and routed, at growing scales until the operator path is refused.
Per case: the first call, three repeats' wall times (the entry returns after its row-count read-back, so the
clock stops behind a device synchronise), and one profiled run's timers.  Prints one JSON line per case.
Needs the GPU: there is no CPU path."""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cypher-for-apache-spark_amd")]
from capsmi import Session, _lib, graph
from capsmi.planner import EntityTable, Planner, ScanGraph

TIMERS = ["reach_part", "reach_level", "reach_final", "reach_count_level", "reach_count_final", "reach_list_count",
          "reach_list_write", "reach_list_starts", "reach_list_gather", "reach_list_order"]
PROBS = (45, 15, 15)


def emit(**kv):
    print(json.dumps(kv), flush=True)


def timers(s):
    out = {}
    for name in TIMERS:
        cnt, ms, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        _lib.call("capsmi_session_kernel_time", s.handle, name.encode(), ctypes.byref(cnt), ctypes.byref(ms))
        _lib.call("capsmi_session_kernel_bytes", s.handle, name.encode(), ctypes.byref(by))
        if cnt.value:
            out[name] = {"launches": cnt.value, "ms": round(ms.value, 4), "ms_per_launch": round(ms.value / cnt.value, 5),
                         "GB": round(by.value / 1e9, 4), "GBps": round(by.value / 1e6 / ms.value, 1) if ms.value > 0 and by.value else None}
    return out


def direct(s, scale, form, lower, upper, words="auto", mode="sliced", reps=3, what="count"):
    n, m = 1 << scale, 32 << scale
    rels = graph.rmat_rels(s, scale, 0, m, PROBS, 42)
    nodes = graph.rmat_nodes(s, scale, graph.NODES_ALL, 42)
    p = graph.NodeBitmap(s, 0, n).add_scan(nodes)
    s.set_config("CAPSMI_REACH_WORDS", words)
    s.set_config("CAPSMI_REACH", mode)

    elements = None
    if what == "collect":  # the element total, outside the timed calls
        t = graph.var_length_collect_distinct(s, [rels], p, p, lower, upper, count_name="count")
        elements = int(t.column("count").values.sum())
        del t

    def once():
        if what == "collect":
            return graph.var_length_collect_distinct(s, [rels], p, p, lower, upper).size
        if form == "grouped":
            t = graph.var_length_count_distinct(s, [rels], p, p, lower, upper)
            return t.size
        return graph.var_length_reach_count(s, [rels], p, p, lower, upper)
    t0 = time.perf_counter()
    res = once()  # warm
    first = time.perf_counter() - t0
    times = []
    if first > 8:  # too slow to repeat: report the one run
        emit(kind="direct", scale=scale, form=form, lower=lower, upper=upper, words=words, mode=mode, result=res,
             first_ms=round(first * 1e3, 3), step_ms=[], timers={})
        return first
    for _ in range(reps):
        t0 = time.perf_counter()
        once()
        times.append(time.perf_counter() - t0)
        if times[-1] > 10:
            break
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    timers(s)
    once()
    tm = timers(s)
    _lib.call("capsmi_session_set_profiling", s.handle, 0)
    emit(kind="direct", what=what, scale=scale, form=form, lower=lower, upper=upper, words=words, mode=mode, result=res,
         elements=elements, first_ms=round(first * 1e3, 3), step_ms=[round(t * 1e3, 3) for t in times], timers=tm)
    s.set_config("CAPSMI_REACH_WORDS", None)
    s.set_config("CAPSMI_REACH", None)
    return min(times)


def spread_ids(scale):
    """2^scale distinct ids spread near 2^40, in random order: ids[d] is the id of R-MAT node d"""
    import numpy as np
    n = 1 << scale
    rng = np.random.default_rng(scale)
    return (1 << 40) + rng.permutation(n).astype(np.int64) * (1 << 26) + rng.integers(0, 1 << 25, n)  # beyond 2^30 from scale 5 on


def spread_graph(s, scale, rels):
    """the R-MAT graph of `rels` stored with the spread ids, compacted: (ids, node table, relationship table)"""
    import numpy as np
    from capsmi import ColumnData, I64
    m = 32 << scale
    ids = spread_ids(scale)
    src, dst = rels.column("source").values, rels.column("target").values
    sn = s.table([ColumnData("id", I64, ids)]).as_node_table("id")
    sr = s.table([ColumnData("id", I64, np.arange(m, dtype=np.int64) + (1 << 50)), ColumnData("source", I64, ids[src]),
                  ColumnData("target", I64, ids[dst])]).as_rel_table("id", "source", "target")
    assert s.compact_if_sparse([sn], [sr])
    return ids, sn, sr


def planned(s, scale, fused, lo=1, hi=3, reps=3, agg="count_distinct", sparse_ids=False):
    rels = graph.rmat_rels(s, scale, 0, 32 << scale, PROBS, 42)
    nodes = graph.rmat_nodes(s, scale, graph.NODES_ALL, 42)
    if sparse_ids:
        _, nodes, rels = spread_graph(s, scale, rels)
    sg = ScanGraph(s, [EntityTable("node", frozenset({"Person"}), {}, nodes, id_col="id")],
                   [EntityTable("rel", frozenset({"KNOWS"}), {}, rels, id_col="id", src_col="source", dst_col="target")])
    q = {"clauses": [{"match": f"(a:Person)-[:KNOWS*{lo}..{hi}]->(b:Person)"}],
         "return": {"items": [["a", ["id", "a"]], ["n", [agg, ["id", "b"]]]]}}
    s.set_fused(fused)
    s.set_unrouted_limit(1 << 30)
    times, rows, err = [], None, None
    try:
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            t, outs = Planner(sg).run(q)
            rows = t.size
            times.append(time.perf_counter() - t0)
            if times[-1] > 10:
                break
    except _lib.CapsmiError as e:
        err = str(e)[:160]
    finally:
        s.set_fused(True)
        s.set_unrouted_limit(0)
    emit(kind="planned", agg=agg, scale=scale, fused=fused, sparse_ids=sparse_ids, lower=lo, upper=hi, rows=rows,
         step_ms=[round(t * 1e3, 3) for t in times[1:]], first_ms=round(times[0] * 1e3, 3) if times else None, refused=err)
    return err is None


def timed(s, label, once, reps=3, **kv):
    """first call, `reps` repeats, one profiled run's timers"""
    t0 = time.perf_counter()
    res = once()
    first = time.perf_counter() - t0
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        once()
        times.append(time.perf_counter() - t0)
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    timers(s)
    once()
    tm = timers(s)
    _lib.call("capsmi_session_set_profiling", s.handle, 0)
    emit(kind="sparse", case=label, result=res, first_ms=round(first * 1e3, 3), step_ms=[round(t * 1e3, 3) for t in times],
         timers=tm, **kv)


def sparse(s, scale, global_form=False):
    """plain ids against spread ids on one R-MAT graph: the direct entries (dense ids + orig) and the compacted graph"""
    import torch
    n, m = 1 << scale, 32 << scale
    rels = graph.rmat_rels(s, scale, 0, m, PROBS, 42)
    nodes = graph.rmat_nodes(s, scale, graph.NODES_ALL, 42)
    p = graph.NodeBitmap(s, 0, n).add_scan(nodes)
    ids = spread_ids(scale)
    spread = torch.from_numpy(ids).cuda()
    ident = torch.arange(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    if global_form:
        timed(s, "global_plain", lambda: len(graph.var_length_reach_list(s, [rels], p, p, 1, 3)), scale=scale)
        timed(s, "global_mapped", lambda: len(graph.var_length_reach_list(s, [rels], p, p, 1, 3, orig=(spread.data_ptr(), n))),
              scale=scale)
        return
    timed(s, "entry_plain", lambda: graph.var_length_collect_distinct(s, [rels], p, p, 1, 3).size, scale=scale)
    timed(s, "entry_mapped_identity",
          lambda: graph.var_length_collect_distinct(s, [rels], p, p, 1, 3, orig=(ident.data_ptr(), n)).size, scale=scale)
    timed(s, "entry_mapped_spread",
          lambda: graph.var_length_collect_distinct(s, [rels], p, p, 1, 3, orig=(spread.data_ptr(), n)).size, scale=scale)
    # the same graph stored with the spread ids, compacted: the planner's route, the order kept with the graph
    _, sn, sr = spread_graph(s, scale, rels)
    q = {"clauses": [{"match": "(a:Person)-[:KNOWS*1..3]->(b:Person)"}],
         "return": {"items": [["a", ["id", "a"]], ["ds", ["collect_distinct", ["id", "b"]]]]}}
    for label, nt, rt in (("planned_plain", nodes, rels), ("planned_compacted", sn, sr)):
        sg = ScanGraph(s, [EntityTable("node", frozenset({"Person"}), {}, nt, id_col="id")],
                       [EntityTable("rel", frozenset({"KNOWS"}), {}, rt, id_col="id", src_col="source", dst_col="target")])
        before = s.route_count("var_length_distinct")
        timed(s, label, lambda: Planner(sg).run(q)[0].size, scale=scale)
        emit(kind="sparse", case=label + "_routed", scale=scale, routed=s.route_count("var_length_distinct") - before)


def main():
    import torch
    s = Session(0)
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    args = sys.argv[1:]
    if "--collect" in args and "--sparse-ids" in args:
        scales = [int(x) for x in args[args.index("--scales") + 1].split(",")] if "--scales" in args else [14, 16]
        for scale in ([] if "--operator-only" in args else scales):
            sparse(s, scale)
        if "--global" in args:
            sparse(s, int(args[args.index("--global") + 1]), global_form=True)
        if "--operator" in args or "--operator-only" in args:  # the compacted graph under the 1 GiB limit
            for scale in (6, 8, 9, 10, 11):
                ok = planned(s, scale, False, agg="collect_distinct", sparse_ids=True)
                planned(s, scale, True, agg="collect_distinct", sparse_ids=True)
                if not ok:
                    break
        s.close()
        return
    if "--collect" in sys.argv[1:]:
        for scale in (6, 8, 9, 10):
            ok = planned(s, scale, False, agg="collect_distinct")
            planned(s, scale, True, agg="collect_distinct")
            if not ok:
                break
        for scale in (14, 16):
            direct(s, scale, "grouped", 1, 3, what="collect")
            direct(s, scale, "grouped", 1, 3)
        s.close()
        return
    # the route against the operator path (the plan run operator by operator: the code before this route)
    for scale in (6, 8, 9, 10, 11, 12):
        ok = planned(s, scale, False)
        planned(s, scale, True)
        if not ok:
            break
    # widths and the two level passes
    for scale in (14, 16):
        for words in ("1", "2", "4", "8", "auto"):
            direct(s, scale, "grouped", 1, 3, words)
        for words in ("1", "8"):
            direct(s, scale, "grouped", 1, 3, words, "flat")
    # route times
    for scale in (14, 16, 18, 19, 20):
        if direct(s, scale, "grouped", 1, 3) > 3.5:
            break
        if direct(s, scale, "grouped", 1, 6) > 3.5:
            break
    for scale in (14, 16, 18, 20, 22):
        if direct(s, scale, "global", 1, 6) > 5:
            break
    s.close()


main()
