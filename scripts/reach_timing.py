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
Per case: the first call, three repeats' wall times (the entry returns after its row-count read-back, so the
clock stops behind a device synchronise), and one profiled run's timers.  Prints one JSON line per case.
Needs the GPU: there is no CPU path."""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cypher-for-apache-spark_amd")]
from capsmi import Session, _lib, graph
from capsmi.planner import EntityTable, Planner, ScanGraph

TIMERS = ["reach_part", "reach_level", "reach_final", "reach_count_level", "reach_count_final", "reach_list_count",
          "reach_list_write", "reach_list_starts"]
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


def planned(s, scale, fused, lo=1, hi=3, reps=3, agg="count_distinct"):
    rels = graph.rmat_rels(s, scale, 0, 32 << scale, PROBS, 42)
    nodes = graph.rmat_nodes(s, scale, graph.NODES_ALL, 42)
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
    emit(kind="planned", agg=agg, scale=scale, fused=fused, lower=lo, upper=hi, rows=rows,
         step_ms=[round(t * 1e3, 3) for t in times[1:]], first_ms=round(times[0] * 1e3, 3) if times else None, refused=err)
    return err is None


def main():
    import torch
    s = Session(0)
    s.set_stream(torch.cuda.current_stream().cuda_stream)
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
